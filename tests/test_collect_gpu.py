"""Replay rows collected from the device rollout loop (mfrl_amd.replay.RolloutCollector, csrc/collect_kernels.hip)
against the C oracle stepped in lockstep: every collected row -- view, feature, action, reward, terminal, former mean
action, key -- is the oracle's, byte for byte and row for row, on the three plans that take a learned policy; the
rings after tight() are those of the per-step push() path; the rollout's new ids / alive buffers are the oracle's
get_agent_id / get_alive before clear_dead; a collector capped below one step's rows reports it without a store;
and play_rollout trains an MFQ model through the captured graph.
"""
import os

import numpy as np
import pytest

from test_policy_big_gpu import Lockstep, interleaved_positions, scripted_actions

gpu = pytest.mark.gpu
VIEW, VF, F, NA = (13, 13, 7), 13 * 13 * 7, 34, 21
MAX_STEPS, STEPS = 12, 25
MAX_LEN, SUB_LEN = 1000, 8
PLANS = {       # name: (map size, agents per side, envs, MFX_SMALL_E, policy path)
    "fused": (64, 128, 3, "0", "k_rollout"),
    "few": (40, 64, 2, None, "k_observe_items+k_rollout_big"),
    "large": (200, 1250, 2, None, "k_observe_items+k_rollout_big"),
}
COLS = ("obs", "feat", "act", "rew", "term", "prob")


def _memory(use_mean=True):
    from mfrl_amd.algo.tools import MemoryGroup
    return MemoryGroup(VIEW, (F,), NA, MAX_LEN, 64, SUB_LEN, use_mean=use_mean)


def _oracle_step(lock, actn, former, episode, ep_len):
    """One step of every oracle env with actn [E][2][rowcap]: group 0's rows of the step (pre-step view, feature,
    action and former mean action; post-step reward, alive flag and id, before clear_dead), env by env."""
    rows = []
    for e, (env, h, _) in enumerate(lock.envs):
        n = [lock.n(e, g) for g in range(2)]
        view, feat = env.get_observation(h[0])
        acts = [np.ascontiguousarray(actn[e, g, :n[g]]) for g in range(2)]
        for g in range(2):
            env.set_action(h[g], acts[g])
        done = env.step()
        rew = env.get_reward(h[0]).copy()
        alive = env.get_alive(h[0]).copy()
        ids = env.get_agent_id(h[0]).copy()
        env.clear_dead()
        if not lock.restarts[e]:
            lock.lost[e][0] |= not alive.all()
        rows.append({"env": e, "episode": episode[e], "n": n[0], "obs": view.reshape(n[0], VF).copy(),
                     "feat": feat.copy(), "act": acts[0].copy(), "rew": rew, "alive": alive.astype(bool), "ids": ids,
                     "prob": np.tile(former[e], (n[0], 1))})
        ep_len[e] += 1
        if bool(done) or ep_len[e] >= lock.max_steps:
            ep_len[e] = 0
            episode[e] += 1
            lock.restarts[e] += 1
            former[e] = np.zeros(NA, dtype=np.float32)           # former_act_prob = 0 at an episode's first step
            lock._reset(env, h)
        else:
            former[e] = (np.bincount(acts[0], minlength=NA) / n[0]).astype(np.float32) if n[0] else \
                np.zeros(NA, dtype=np.float32)
    return rows


def _run(plan, use_mean=True, fresh_stream=False, seed=31):
    """STEPS scripted policy steps of the plan with a collector around each, the oracle in lockstep: the collected
    columns (host copies), the oracle's step rows, the per-step ids / alive buffers, and the MemoryGroup itself
    (rows not yet tight)."""
    import torch
    from mfrl_amd.battle import BattleBatch
    from mfrl_amd.replay import RolloutCollector, rollout_key
    map_size, n_side, E, small_e, path = PLANS[plan]
    placement = interleaved_positions(map_size, n_side)
    old = os.environ.get("MFX_SMALL_E")
    if small_e is not None:
        os.environ["MFX_SMALL_E"] = small_e
    try:
        stream = torch.cuda.Stream() if fresh_stream else torch.cuda.current_stream()
        eng = BattleBatch(map_size, E, stream=stream)
        eng.rollout_init(placement, max_steps=MAX_STEPS, eps=0.2, seed=3, stagger=False)
    finally:
        if small_e is not None:
            if old is None:
                del os.environ["MFX_SMALL_E"]
            else:
                os.environ["MFX_SMALL_E"] = old
    assert eng.rollout_policy_path() == path
    if fresh_stream:
        assert eng.stream_handle() != torch.cuda.current_stream().cuda_stream
    rc = eng.rowcap
    lock = Lockstep(eng, map_size, placement, MAX_STEPS, False)
    mg = _memory(use_mean)
    col = RolloutCollector(eng, mg, 0)
    rng = np.random.default_rng(seed)
    former = [np.zeros(NA, dtype=np.float32) for _ in range(E)]
    episode, ep_len = [0] * E, [0] * E
    ids_log = torch.empty((STEPS, E, 2, rc), dtype=torch.int32, device="cuda")
    alive_log = torch.empty((STEPS, E, 2, rc), dtype=torch.uint8, device="cuda")
    steps, keep = [], []
    eng.rollout_policy_observe()
    for t in range(STEPS):
        actn = scripted_actions(rng, E, rc)
        keep.append(torch.from_numpy(actn).cuda())   # (kept: the engine's stream copies it asynchronously)
        eng.rollout_write("actions", keep[-1])
        col.begin()                                  # (outside any stream context: the collector orders itself)
        eng.rollout_policy_step()
        col.end()
        eng.rollout_copy("ids", ids_log[t])
        eng.rollout_copy("alive", alive_log[t])
        steps.append(_oracle_step(lock, actn, former, episode, ep_len))
    n = col.finish()
    assert mg._rows.n == n
    eng.rollout_check()
    cols = {k: v[:n].cpu().numpy() for k, v in mg._rows.cols.items()}
    flat = [r for s in steps for r in s]
    want = {k: np.concatenate([r[k] for r in flat]) for k in ("obs", "feat", "act", "rew", "prob")}
    want["term"] = ~np.concatenate([r["alive"] for r in flat])
    want["env"] = np.concatenate([np.full(r["n"], r["env"]) for r in flat])
    want["episode"] = np.concatenate([np.full(r["n"], r["episode"]) for r in flat])
    want["id"] = np.concatenate([r["ids"] for r in flat]).astype(np.int64)
    want["key"] = rollout_key(want["env"], want["episode"], want["id"], E, col.id_stride())
    return {"n": n, "cols": cols, "want": want, "steps": steps, "lock": lock, "mg": mg, "E": E, "rowcap": rc,
            "ids_log": ids_log.cpu().numpy(), "alive_log": alive_log.cpu().numpy()}


_CACHE = {}


def _cached(plan):
    if plan not in _CACHE:
        _CACHE[plan] = _run(plan)
    return _CACHE[plan]


def _check_rows(res, use_mean=True):
    want, cols, lock = res["want"], res["cols"], res["lock"]
    # input conditions, on the oracle alone
    assert min(lock.restarts) >= 2, lock.restarts
    assert all(a for a, _ in lock.lost), lock.lost
    assert min(r["n"] for s in res["steps"] for r in s) < res["rowcap"]
    assert res["n"] == len(want["act"])
    for k in COLS:
        if k == "prob" and not use_mean:
            assert "prob" not in cols
            continue
        got = cols[k].reshape(res["n"], -1)
        exp = want[k].reshape(res["n"], -1)
        assert got.dtype == exp.dtype or k == "term", (k, got.dtype, exp.dtype)
        bad = np.nonzero((got.view(np.uint8).reshape(res["n"], -1) != exp.view(np.uint8).reshape(res["n"], -1)).any(1))[0]
        assert len(bad) == 0, (k, "first differing rows", bad[:5], len(bad))
    # two rows share a key exactly when they share (env, episode, id)
    trip = np.stack([want["env"], want["episode"], want["id"]], 1)
    _, a = np.unique(trip, axis=0, return_inverse=True)
    _, b = np.unique(cols["ids"], return_inverse=True)
    a, b = a.reshape(-1), b.reshape(-1)
    pairs = len(np.unique(np.stack([a, b], 1), axis=0))
    assert pairs == a.max() + 1 == b.max() + 1, (pairs, a.max() + 1, b.max() + 1)
    assert np.array_equal(cols["ids"], want["key"])          # and it is replay.rollout_key


@gpu
@pytest.mark.parametrize("plan", list(PLANS))
def test_rows_equal_the_oracle(plan):
    """The collected step rows of 25 scripted steps (max_steps 12: every env restarts twice, agents die before the
    first restart, group 0 shrinks below rowcap) are the oracle's."""
    _check_rows(_cached(plan))


@gpu
def test_rows_on_a_fresh_stream_outside_any_stream_context():
    """The engine on a torch.cuda.Stream() of its own, the collector called from the default stream's context: the
    same rows as with the engine on the current stream."""
    res = _run("few", fresh_stream=True)
    _check_rows(res)
    base = _cached("few")
    assert res["n"] == base["n"]
    for k in COLS + ("ids",):
        assert res["cols"][k].tobytes() == base["cols"][k].tobytes(), k


@gpu
def test_rows_without_mean_field():
    """A DQN-style buffer (use_mean=False): no prob column, the other columns as before."""
    _check_rows(_run("few", use_mean=False), use_mean=False)


@gpu
def test_rings_equal_the_push_path():
    """tight() on the collected rows fills the rings exactly as it does on the same rows pushed step by step with
    MemoryGroup.push (same np.random seed): ring shorter than the rows (it wraps), sequences longer than sub_len
    (the per-agent truncation runs)."""
    from mfrl_amd.replay import rollout_key
    res = _run("few")                      # (a run of its own: tight() consumes the step rows)
    _check_rows(res)
    mg, E = res["mg"], res["E"]
    ref = _memory()
    stride = 2 * res["rowcap"]
    for rows in res["steps"]:
        keys = np.concatenate([rollout_key(r["env"], r["episode"], r["ids"].astype(np.int64), E, stride) for r in rows])
        ref.push(ids=keys, state=[np.concatenate([r["obs"] for r in rows]).reshape((-1,) + VIEW),
                                  np.concatenate([r["feat"] for r in rows])],
                 acts=np.concatenate([r["act"] for r in rows]), rewards=np.concatenate([r["rew"] for r in rows]),
                 alives=np.concatenate([r["alive"] for r in rows]), prob=np.concatenate([r["prob"] for r in rows]))
    assert ref._rows.n == mg._rows.n == res["n"] > MAX_LEN
    assert max(np.unique(res["want"]["key"], return_counts=True)[1]) > SUB_LEN
    for m in (mg, ref):
        np.random.seed(7)
        m.tight()
    assert mg._new_add == ref._new_add > MAX_LEN            # the ring wrapped
    for name in ("obs0", "feat0", "actions", "rewards", "terminals", "masks", "prob"):
        a, b = getattr(mg, name), getattr(ref, name)
        assert a.length == b.length == MAX_LEN and a._flag == b._flag, name
        assert a.data[:a.length].cpu().numpy().tobytes() == b.data[:b.length].cpu().numpy().tobytes(), name


@gpu
def test_ids_and_alive_buffers():
    """The rollout's ids / alive buffers after each policy step are the oracle's get_agent_id / get_alive before
    clear_dead on the live rows; they are not writable."""
    import torch
    res = _cached("fused")
    for t, rows in enumerate(res["steps"]):
        for r in rows:
            e, n = r["env"], r["n"]
            assert np.array_equal(res["ids_log"][t, e, 0, :n], r["ids"]), (t, e, "ids")
            assert np.array_equal(res["alive_log"][t, e, 0, :n].astype(bool), r["alive"]), (t, e, "alive")
    assert not all(r["alive"].all() for s in res["steps"] for r in s)
    eng = res["lock"].eng
    for name in ("ids", "alive"):
        with pytest.raises(ValueError, match="not writable"):
            eng.rollout_write(name, torch.zeros(4, dtype=torch.int32, device="cuda"))


@gpu
def test_capacity_overflow_is_reported_without_a_store():
    """A collector capped below one step's rows: finish() raises, _rows.n is unchanged, and neither the capped
    storage nor the guard rows behind it were written."""
    import torch
    from mfrl_amd.battle import BattleBatch
    from mfrl_amd.replay import CollectOverflow, RolloutCollector
    map_size, n_side, E = 40, 64, 2
    placement = interleaved_positions(map_size, n_side)
    eng = BattleBatch(map_size, E, stream=torch.cuda.current_stream())
    eng.rollout_init(placement, max_steps=MAX_STEPS, eps=0.2, seed=3, stagger=False)
    mg = _memory()
    mg._rows._ensure(1024)
    for c in mg._rows.cols.values():
        c.view(torch.uint8).fill_(0xA5)
    cap = 10
    assert cap < E * n_side
    col = RolloutCollector(eng, mg, 0, capacity=cap)
    eng.rollout_policy_observe()
    actn = scripted_actions(np.random.default_rng(5), E, eng.rowcap)
    for _ in range(2):
        eng.rollout_write("actions", torch.from_numpy(actn).cuda())
        col.begin()
        eng.rollout_policy_step()
        col.end()
    with pytest.raises(CollectOverflow, match="did not fit"):
        col.finish()
    eng.rollout_check()
    assert mg._rows.n == 0 and mg._rows.cap == 1024
    for k, c in mg._rows.cols.items():
        assert bool((c.view(torch.uint8) == 0xA5).all()), k
    # and the collector works again afterwards, uncapped
    col.capacity = None
    eng.rollout_write("actions", torch.from_numpy(actn).cuda())
    col.begin()
    eng.rollout_policy_step()
    col.end()
    assert 0 < col.finish() <= E * n_side


@gpu
def test_play_rollout_trains_mfq():
    """Two rounds of play_rollout with two MFQ models (40x40, 2 envs, 10 steps, train): the ring holds min(rows,
    max_len) entries, the eval net moved and is finite, the second round replays the first's captured graph; an
    actor-critic run is refused."""
    import torch
    import magent
    from mfrl_amd import train_battle
    from mfrl_amd.algo import spawn_ai
    from mfrl_amd.algo.play import play_rollout
    from mfrl_amd.battle import BattleBatch
    map_size, E, max_steps, max_len = 40, 2, 10, 1500
    env = magent.GridWorld("battle", map_size=map_size)
    h = env.get_handles()
    torch.manual_seed(3)
    models = [spawn_ai("mfq", None, env, h[g], "mfq-%d" % g, max_steps, memory_size=max_len) for g in range(2)]
    eng = BattleBatch(map_size, E, stream=torch.cuda.current_stream())
    before = [p.detach().clone() for p in models[0].eval_net.parameters()]
    rows, graph = 0, None
    np.random.seed(1)
    for k in range(2):
        out = play_rollout(eng, k, map_size, max_steps, models, eps=1.0, train=True, left_id=0)
        assert len(out) == 4 and out[0] == [128, 128] and all(len(x) == 2 for x in out)
        got = models[0]._rollout_collector.last_rows
        assert 0 < got <= E * 64 * max_steps
        rows += got
        assert models[0].replay_buffer.nb_entries == min(rows, max_len)
        assert models[0].replay_buffer._rows.n == 0
        if k == 0:
            graph = models[0]._graph
            assert graph is not None
    assert rows > max_len
    assert models[0]._graph is graph
    after = list(models[0].eval_net.parameters())
    assert all(bool(torch.isfinite(p).all()) for p in after)
    assert any(not torch.equal(a, b) for a, b in zip(after, before))
    with pytest.raises(SystemExit):
        train_battle.main(["--algo", "ac", "--envs", "2", "--rollout"])
    ac = spawn_ai("ac", None, env, h[0], "ac-0", max_steps)
    with pytest.raises(TypeError, match="DQN / MFQ only"):
        play_rollout(eng, 0, map_size, max_steps, [ac, ac], train=True, left_id=0)
