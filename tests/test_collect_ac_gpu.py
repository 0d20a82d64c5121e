"""The episode-chain path of the rollout collector on the GPU (mfx_collect_end_linked, mfx_chain_returns,
ActorCritic.train_rollout, play_rollout_episodes).

Links: a linked collector (EpisodesBuffer rows) and an unlinked one (MemoryGroup rows, the path tests/test_collect_gpu.py
pins to the oracle) on twin engines fed the same scripted actions give the same ordinary columns byte for byte, and the
link columns are replay.chain_links of the key column.  Returns: mfx_chain_returns on those rows equals, row for row and
bit for bit, EpisodesBuffer.batch() + mf.mfac_returns; on synthetic forests it equals the oracle's mfac_returns per
chain.  Gradient: train_rollout's chunked gradient against the one-piece gradient of the batch()-ordered copy, both
judged by a float64 evaluation.  Driver: two rounds of play_rollout_episodes train an MFAC and an AC model.

AC_ROLLOUT_ERROR_OUT=<path>: the gradient test appends its measured figures per case there."""
import copy
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import common
from test_collect_gpu import MAX_STEPS, PLANS, STEPS
from test_policy_big_gpu import interleaved_positions, scripted_actions

sys.path.insert(0, os.path.join(common.REPO, "oracle"))
import mf_oracle  # noqa: E402

gpu = pytest.mark.gpu
VIEW, F, NA = (13, 13, 7), 34, 21
ORDINARY = ("ids", "obs", "feat", "act", "rew", "term", "prob")
GAMMA = 0.95


def _engine(plan):
    import torch
    from mfrl_amd.battle import BattleBatch
    map_size, n_side, E, small_e, path = PLANS[plan]
    old = os.environ.get("MFX_SMALL_E")
    if small_e is not None:
        os.environ["MFX_SMALL_E"] = small_e
    try:
        eng = BattleBatch(map_size, E, stream=torch.cuda.current_stream())
        eng.rollout_init(interleaved_positions(map_size, n_side), max_steps=MAX_STEPS, eps=0.2, seed=3, stagger=False)
    finally:
        if small_e is not None:
            if old is None:
                del os.environ["MFX_SMALL_E"]
            else:
                os.environ["MFX_SMALL_E"] = old
    assert eng.rollout_policy_path() == path
    return eng


def _scripted(eng, col, steps=STEPS, seed=31):
    """`steps` scripted policy steps with the collector around each; the rows stay in the collector's buffer."""
    import torch
    rng = np.random.default_rng(seed)
    keep = []
    eng.rollout_policy_observe()
    for _ in range(steps):
        keep.append(torch.from_numpy(scripted_actions(rng, eng.n_envs, eng.rowcap)).cuda())
        eng.rollout_write("actions", keep[-1])
        col.begin()
        eng.rollout_policy_step()
        col.end()
    n = col.finish()
    eng.rollout_check()
    return n


def _buffer(use_mean=True):
    from mfrl_amd.algo.tools import EpisodesBuffer
    buf = EpisodesBuffer(use_mean=use_mean)
    buf.prepare(VIEW, (F,), NA if use_mean else 1)
    return buf


_CACHE = {}


def _run(plan):
    """The plan's scripted run twice: `ref`, the columns of an unlinked collector (MemoryGroup), and `buf`, the
    EpisodesBuffer a linked collector filled (rows left in place), with host copies of its columns in `got`."""
    if plan in _CACHE:
        return _CACHE[plan]
    from mfrl_amd.algo.tools import MemoryGroup
    from mfrl_amd.replay import RolloutCollector
    mg = MemoryGroup(VIEW, (F,), NA, 1000, 64, 8, use_mean=True)
    eng = _engine(plan)
    plain = RolloutCollector(eng, mg, 0)
    assert not plain.linked
    n_ref = _scripted(eng, plain)
    ref = {k: v[:n_ref].cpu().numpy() for k, v in mg._rows.cols.items()}
    buf = _buffer()
    eng2 = _engine(plan)
    col = RolloutCollector(eng2, buf, 0)
    assert col.linked
    n = _scripted(eng2, col)
    got = {k: v[:n].cpu().numpy() for k, v in buf._rows.cols.items()}
    res = {"ref": ref, "n_ref": n_ref, "buf": buf, "got": got, "n": n, "E": eng.n_envs, "stride": col.id_stride(),
           "col": col}
    _CACHE[plan] = res
    return res


def _conditions(res):
    """The input conditions, on the unlinked collector's key and terminal columns alone; returns whether some chain
    has one row."""
    key, term, E, stride = res["ref"]["ids"], res["ref"]["term"].astype(bool), res["E"], res["stride"]
    assert res["n_ref"] > 1024                                  # the storage (1,024 rows at first) has to grow
    episode, env = key // (E * stride), (key // stride) % E
    for e in range(E):
        assert episode[env == e].max() >= 2, (e, "restarted fewer than twice")
    # some chain ends on a terminal row before its episode's end.  Every agent of an episode is there from its
    # first step, so a row's step within the episode is the number of earlier rows of its key.
    run = episode * E + env                                     # = key // stride
    seen, step = {}, np.zeros(len(key), np.int64)
    for r, k in enumerate(key.tolist()):
        step[r] = seen.get(k, 0)
        seen[k] = step[r] + 1
    run_len = {r: int(step[run == r].max()) + 1 for r in np.unique(run).tolist()}
    early = [r for r in np.nonzero(term)[0].tolist() if step[r] + 1 < run_len[int(run[r])]]
    assert early, "no chain ends on a terminal row before its episode's end"
    assert all(not (key[r + 1:] == key[r]).any() for r in early[:20])         # a terminal row is its key's last
    _, counts = np.unique(key, return_counts=True)
    return bool((counts == 1).any())


@gpu
@pytest.mark.parametrize("plan", ["fused", "few"])
def test_links_against_the_key_column(plan):
    """25 scripted steps, max_steps 12 (every env restarts twice; the third episode is one step long, so its chains
    have one row): the ordinary columns are the unlinked collector's, prev / tail are chain_links(key column)."""
    from mfrl_amd.replay import chain_links
    res = _run(plan)
    single = _conditions(res)
    assert single, "the scripted run has no one-row chain (test_synthetic_forest covers that case)"
    assert res["n"] == res["n_ref"]
    assert res["buf"]._rows.cap > 1024                          # it grew during the run
    assert list(res["got"]) == list(ORDINARY) + ["prev", "tail"]
    for k in ORDINARY:
        assert res["got"][k].dtype == res["ref"][k].dtype, k
        assert res["got"][k].tobytes() == res["ref"][k].tobytes(), k
    prev, tail = chain_links(res["ref"]["ids"])
    assert np.array_equal(res["got"]["prev"], prev)
    assert res["got"]["tail"].view(np.uint8).tobytes() == tail.view(np.uint8).tobytes()      # 0 / 1 exactly
    # what the links mean: a predecessor is an earlier row of the same key, a chain's rows are all rows of its key
    has = prev >= 0
    assert (prev[has] < np.nonzero(has)[0]).all() and (res["ref"]["ids"][prev[has]] == res["ref"]["ids"][has]).all()
    assert tail.sum() == len(np.unique(res["ref"]["ids"]))


@gpu
@pytest.mark.parametrize("numpy1", [True, False])
@pytest.mark.parametrize("plan", ["fused", "few"])
def test_returns_equal_the_batch_path(plan, numpy1):
    """mfx_chain_returns on a clone of the collected reward column = EpisodesBuffer.batch() order, offsets from its
    counts and mf.mfac_returns, the tail values matched by key; row for row, bit for bit."""
    import torch
    from mfrl_amd import mf, replay
    res = _run(plan)
    _conditions(res)
    buf, n = res["buf"], res["n"]
    c = buf._rows.cols
    key = res["ref"]["ids"]
    tails = c["tail"][:n].nonzero().reshape(-1)
    t_host = tails.cpu().numpy()
    assert np.array_equal(t_host, np.nonzero(replay.chain_links(key)[1])[0])
    val = np.random.default_rng(17).standard_normal(len(t_host)).astype(np.float32)
    # the existing path
    order, counts, uniq = buf._rows.grouped()
    rows, counts2 = buf.batch()
    assert torch.equal(counts, counts2) and torch.equal(rows["ids"], c["ids"][:n][order])
    by_key = dict(zip(key[t_host].tolist(), val.tolist()))
    assert len(by_key) == len(t_host) == len(uniq)
    val_b = np.array([by_key[k] for k in uniq.cpu().tolist()], dtype=np.float32)
    offsets = torch.zeros(len(counts) + 1, dtype=torch.int64, device="cuda")
    offsets[1:] = torch.cumsum(counts, 0)
    want = mf.mfac_returns(rows["rew"].clone(), offsets, torch.from_numpy(val_b).cuda(), GAMMA, numpy1=numpy1)
    # the chain path, in place on the step-major rows
    rew = c["rew"][:n].clone()
    got = replay.chain_returns(rew, c["prev"], tails, torch.from_numpy(val).cuda(), GAMMA, numpy1=numpy1)
    assert got.data_ptr() == rew.data_ptr()
    assert not torch.equal(rew, c["rew"][:n])
    assert got[order].cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    # and the host restatement agrees
    host = replay.chain_returns_host(res["got"]["rew"], res["got"]["prev"], t_host, val, GAMMA, numpy1)
    assert host.tobytes() == got.cpu().numpy().tobytes()


def _abi():
    dll = ctypes.CDLL(common.HIP_LIB)
    dll.mfx_chain_returns.restype = ctypes.c_int
    dll.mfx_chain_returns.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_int64, ctypes.c_double,
                                                               ctypes.c_int, ctypes.c_void_p]
    return dll


def _forest(rng, lens):
    owner = np.repeat(np.arange(len(lens)), lens)
    rng.shuffle(owner)
    prev = np.full(len(owner), -1, np.int64)
    rows = [np.nonzero(owner == k)[0] for k in range(len(lens))]
    for r in rows:
        prev[r[1:]] = r[:-1]
    return prev, np.array([r[-1] for r in rows], np.int64), rows


def _chain_call(dll, rew, prev, tails, val, n_rows, numpy1):
    import torch
    d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (rew, prev, tails, val)]
    for t in d:                      # (empty tensors have no storage: give the call valid memory all the same)
        assert t.numel() == 0 or t.data_ptr() != 0
    pad = torch.zeros(8, dtype=torch.int64, device="cuda")
    ptr = [ctypes.c_void_p(t.data_ptr() if t.numel() else pad.data_ptr()) for t in d]
    rc = dll.mfx_chain_returns(*ptr, len(tails), n_rows, GAMMA, int(numpy1),
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, d[0].cpu().numpy()


@gpu
@pytest.mark.parametrize("numpy1", [True, False])
def test_synthetic_forest(numpy1):
    """Straight through the C ABI against mf_oracle.mfac_returns per chain, bitwise: zero tails; one chain of one
    row; 300 interleaved chains of 1..40 rows plus one of 400 (more tails than a workgroup; the episode cap)."""
    dll = _abi()
    rng = np.random.default_rng(23)
    rew = rng.standard_normal(5).astype(np.float32)
    rc, out = _chain_call(dll, rew, np.full(5, -1, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32), 5, numpy1)
    assert rc == 0 and out.tobytes() == rew.tobytes()
    for lens in ([1], np.concatenate([rng.integers(1, 41, size=300), [400]])):
        prev, tails, rows = _forest(rng, np.asarray(lens))
        assert len(tails) == len(lens) and min(len(r) for r in rows) == 1
        rew = rng.standard_normal(len(prev)).astype(np.float32)
        val = rng.standard_normal(len(tails)).astype(np.float32)
        rc, out = _chain_call(dll, rew, prev, tails, val, len(prev), numpy1)
        assert rc == 0
        for r, v in zip(rows, val):
            assert out[r].tobytes() == mf_oracle.mfac_returns(rew[r], v, GAMMA, numpy1=numpy1).tobytes(), len(r)
    assert len(tails) > 256 and max(len(r) for r in rows) == 400


@gpu
@pytest.mark.parametrize("bad", [1000, -2, 7])
def test_a_prev_outside_the_rows_is_reported(bad):
    """An argument check on valid memory: a predecessor outside the rows (1000 of 12; -2; 7, which is not below its
    row 5) ends the walk there -- the rows before it in the walk hold their returns, nothing else of the chain is
    touched, the call returns -1 with a message -- and the next call is clean."""
    dll = _abi()
    dll.mfx_last_error.restype = ctypes.c_char_p
    prev = np.array([-1, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9], np.int64)      # two chains: even rows, odd rows
    tails = np.array([10, 11], np.int64)
    rew = np.arange(1, 13, dtype=np.float32)
    val = np.array([0.5, -0.5], np.float32)
    broken = prev.copy()
    broken[5] = bad                                                        # the odd chain: 11, 9, 7, 5 | 3, 1
    rc, out = _chain_call(dll, rew, broken, tails, val, 12, True)
    assert rc == -1 and b"chain_returns" in dll.mfx_last_error() and str(bad).encode() in dll.mfx_last_error()
    even = mf_oracle.mfac_returns(rew[0::2], val[0], GAMMA)
    odd = mf_oracle.mfac_returns(rew[5::2], val[1], GAMMA)                 # rows 5..11 were walked before the bad link
    assert out[0::2].tobytes() == even.tobytes()
    assert out[5::2].tobytes() == odd.tobytes()
    assert out[[1, 3]].tobytes() == rew[[1, 3]].tobytes()                  # nothing stored past it
    rc, out = _chain_call(dll, rew, prev, tails, val, 12, True)            # the error word was cleared
    assert rc == 0 and out[1::2].tobytes() == mf_oracle.mfac_returns(rew[1::2], val[1], GAMMA).tobytes()
    rc, _ = _chain_call(dll, rew, prev, np.array([10, 12], np.int64), val, 12, True)      # a tail outside the rows
    assert rc == -1
    rc, _ = _chain_call(dll, rew, prev, tails, val, 12, True)
    assert rc == 0


@gpu
def test_linked_overflow_is_reported_without_a_store():
    """A linked collector capped below one step's rows: finish() raises, and neither the columns (prev and tail
    included) nor the table of newest rows were written -- the table is all -1 after the first step (the session's
    reset) and keeps a marker through the second."""
    import torch
    from mfrl_amd.replay import CollectOverflow, RolloutCollector
    eng = _engine("few")
    E, n_side = 2, 64
    buf = _buffer()
    rows = buf._rows
    rows._ensure(1024)
    for c in rows.cols.values():
        c.view(torch.uint8).fill_(0xA5)
    col = RolloutCollector(eng, buf, 0, capacity=10)
    assert col.linked and 10 < E * n_side
    eng.rollout_policy_observe()
    actn = torch.from_numpy(scripted_actions(np.random.default_rng(5), E, eng.rowcap)).cuda()
    for k in range(2):
        eng.rollout_write("actions", actn)
        col.begin()
        eng.rollout_policy_step()
        col.end()
        eng.sync()
        if k == 0:
            assert col._last.numel() == E * col.id_stride() and bool((col._last == -1).all())
            col._last.fill_(0x5A5A5A5A)
    with pytest.raises(CollectOverflow, match="did not fit"):
        col.finish()
    eng.rollout_check()
    assert rows.n == 0 and rows.cap == 1024
    for k, c in rows.cols.items():
        assert bool((c.view(torch.uint8) == 0xA5).all()), k
    assert bool((col._last == 0x5A5A5A5A).all())
    # and the collector works again afterwards, uncapped: one step, every row a chain of its own
    col.capacity = None
    eng.rollout_write("actions", actn)
    col.begin()
    eng.rollout_policy_step()
    col.end()
    n = col.finish()
    assert 0 < n <= E * n_side
    assert bool((rows.cols["prev"][:n] == -1).all()) and bool(rows.cols["tail"][:n].all())


@gpu
def test_linked_begin_refuses_pushed_rows():
    from mfrl_amd.replay import RolloutCollector
    eng = _engine("few")
    buf = _buffer()
    col = RolloutCollector(eng, buf, 0)
    buf.push(ids=np.arange(5), state=[np.zeros((5,) + VIEW, np.float32), np.zeros((5, F), np.float32)],
             acts=np.arange(5, dtype=np.int32), rewards=np.zeros(5, np.float32), alives=np.ones(5, bool),
             prob=np.zeros((5, NA), np.float32))
    assert buf._rows.n == 5 and buf._rows.links
    import torch
    eng.rollout_policy_observe()
    eng.rollout_write("actions", torch.from_numpy(scripted_actions(np.random.default_rng(5), 2, eng.rowcap)).cuda())
    with pytest.raises(ValueError, match="no links"):
        col.begin()
    buf.clear()
    col.begin()
    eng.rollout_policy_step()
    col.end()
    assert col.finish() > 0


def _model(algo, name, max_steps=MAX_STEPS):
    import magent
    import torch
    from mfrl_amd.algo import spawn_ai
    env = magent.GridWorld("battle", map_size=40)
    torch.manual_seed(3)
    return spawn_ai(algo, None, env, env.get_handles()[0], name, max_steps), env


def _block_errors(g, g64):
    out = []
    for a, b in zip(g, g64):
        scale = float(b.abs().max())
        out.append((float((a.double() - b).abs().max()) / scale if scale > 0 else float("inf"), scale))
    return out


@gpu
@pytest.mark.parametrize("algo", ["ac", "mfac"])
def test_gradient_of_train_rollout(algo):
    """One set of collected rows ("few", 25 scripted steps), one set of weights: the gradient of
    train_rollout(step=False) in chunks of 600 rows (more than three, the last ragged) and the gradient of
    ActorCritic.losses on the batch()-ordered copy in one piece, each against the same loss evaluated by torch in
    float64: per parameter block e = max|g - g64| / max|g64| and e_rollout <= 4 e_onepiece, the margin
    tests/test_qtrain_gpu.py gives a re-ordered f32 sum against torch's own."""
    import torch
    from mfrl_amd import mf
    model, _ = _model(algo, algo + "-grad")
    use_mf = algo == "mfac"
    eng = _engine("few")
    col = model.rollout_collector(eng, 0)
    assert col.linked and col.mg is model.replay_buffer
    n = _scripted(eng, col)
    chunk = 600
    assert n > 3 * chunk and n % chunk != 0
    buf = model.replay_buffer
    assert ("prob" in buf._rows.cols) == use_mf
    # the existing path, without the step: batch() order, bootstrap values of the last rows, mfac_returns
    rows, counts = buf.batch()
    prob = rows.get("prob")
    last = torch.cumsum(counts, 0) - 1
    with torch.no_grad():
        _, keep, _ = model._hip_net().forward(rows["obs"][last], rows["feat"][last], prob[last] if use_mf else None,
                                              want_policy=False, want_value=True, want_act=False)
    offsets = torch.zeros(len(counts) + 1, dtype=torch.int64, device="cuda")
    offsets[1:] = torch.cumsum(counts, 0)
    ret = mf.mfac_returns(rows["rew"].clone(), offsets, keep.float().contiguous(), model.gamma)
    params = list(model.net.parameters())
    total = sum(model.losses(rows["obs"], rows["feat"], rows["act"], ret, prob)[:3])
    g_one = [g.detach().clone() for g in torch.autograd.grad(total, params)]
    # the same loss in float64
    net32 = model.net
    model.net = copy.deepcopy(net32).double()
    try:
        total64 = sum(model.losses(rows["obs"].double(), rows["feat"].double(), rows["act"], ret.double(),
                                   prob.double() if use_mf else None)[:3])
        g64 = [g.detach().clone() for g in torch.autograd.grad(total64, list(model.net.parameters()))]
    finally:
        model.net = net32
    key_before = [p.detach().clone() for p in params]
    g_roll = model.train_rollout(chunk_rows=chunk, step=False)
    assert all(torch.equal(a, b) for a, b in zip(key_before, params))          # step=False: no step
    assert buf._rows.n == 0 and model.replay_buffer is buf
    e_roll, e_one = _block_errors(g_roll, g64), _block_errors(g_one, g64)
    names = [k for k, _ in model.net.named_parameters()]
    rec = {"algo": algo, "rows": n, "chunk": chunk, "blocks": names, "e_rollout": [e[0] for e in e_roll],
           "e_onepiece": [e[0] for e in e_one], "max_g64": [e[1] for e in e_roll]}
    print(json.dumps(rec))
    if os.environ.get("AC_ROLLOUT_ERROR_OUT"):
        with open(os.environ["AC_ROLLOUT_ERROR_OUT"], "a") as f:
            f.write(json.dumps(rec) + "\n")
    for k, name in enumerate(names):
        assert e_roll[k][1] > 0, name
        assert e_roll[k][0] <= 4.0 * e_one[k][0], (name, e_roll[k][0], e_one[k][0])


@gpu
@pytest.mark.parametrize("algo", ["mfac", "ac"])
def test_play_rollout_episodes_trains(algo):
    """Two rounds of play_rollout_episodes (40x40, 2 envs, 10 steps, train): the parameters moved and are finite, the
    rows are empty after training, the same EpisodesBuffer and -- no grow being needed -- the same column storage
    serve round two; an MFQ model is refused."""
    import torch
    from mfrl_amd.algo import spawn_ai
    from mfrl_amd.algo.play import play_rollout_episodes
    from mfrl_amd.battle import BattleBatch
    map_size, E, max_steps = 40, 2, 10
    me, env = _model(algo, algo + "-0", max_steps)
    other = spawn_ai(algo, None, env, env.get_handles()[1], algo + "-1", max_steps)
    models = [me, other]
    eng = BattleBatch(map_size, E, stream=torch.cuda.current_stream())
    before = [p.detach().clone() for p in me.net.parameters()]
    buf = me.replay_buffer
    state = np.random.get_state()[1].copy()
    seen = []
    for k in range(2):
        out = play_rollout_episodes(eng, k, map_size, max_steps, models, eps=1.0, train=True, left_id=0)
        assert len(out) == 4 and out[0] == [128, 128] and all(len(x) == 2 for x in out)
        assert 0 < me._rollout_collector.last_rows <= E * 64 * max_steps
        assert me.replay_buffer is buf and buf._rows.n == 0 and buf._rows.links
        assert ("prob" in buf._rows.cols) == (algo == "mfac")
        seen.append((buf._rows.cap, {n: c.data_ptr() for n, c in buf._rows.cols.items()}))
        if k == 0:
            mid = [p.detach().clone() for p in me.net.parameters()]
    assert seen[0][0] >= E * 64 * max_steps                     # round two needed no grow ...
    assert seen[1] == seen[0]                                   # ... and ran on the same storage
    after = list(me.net.parameters())
    assert all(bool(torch.isfinite(p).all()) for p in after)
    assert any(not torch.equal(a, b) for a, b in zip(mid, before))
    assert any(not torch.equal(a, b) for a, b in zip(after, mid))
    assert np.array_equal(np.random.get_state()[1], state)      # no host randomness was drawn
    mfq = spawn_ai("mfq", None, env, env.get_handles()[0], "mfq-x", max_steps, memory_size=1500)
    with pytest.raises(TypeError, match="EpisodesBuffer"):
        play_rollout_episodes(eng, 0, map_size, max_steps, [mfq, mfq], train=True, left_id=0)
