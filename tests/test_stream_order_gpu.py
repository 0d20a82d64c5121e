"""Cross-stream hand-offs with the producer's stream stalled (tests/stream_stall.py; DESIGN "streams").

The Python layer runs on two streams: weights, weight images, the ACNet support image and all training go on torch's
current stream; every act_rollout, the collector and the neighbourhood mean go on the engine's.  On an idle GPU the
producer finishes before the host has enqueued the consumer, so a missing edge never shows.  Every case here runs twice:

    serial    everything on one stream (the caller inside the engine's stream), private handles, no stall
    stalled   the engine on S, the caller inside torch.cuda.stream(C), S and C measured independent and neither the
              default stream, the producer's stream kept busy by a stall armed first, no synchronisation in between

and the two must agree bit for bit, with the stall still pending after the last enqueue (`outlived`).  A case whose
entry point synchronises on the host asserts the opposite -- the stall is over when the call returns -- and names the
line that synchronises.  The control goes through the C entries with explicit streams, which promise no ordering: it is
the one test that expects the stale result, and so shows that the harness sees a missing edge.
"""
import copy
import json
import os
import time

import numpy as np
import pytest

import stream_stall as ss

pytestmark = pytest.mark.gpu

VIEW, FEAT, NA = (13, 13, 7), (34,), 21
_RIG = {}


class Rig:
    """C (the caller's stream), S1 and S2 (the engines'): pairwise independent, none the default stream.  Engines of 3
    envs on S1 and 70 on S2 (past one 64-env chunk of the row list), 64x64, 20 steps in, observed and never stepped
    again: act_rollout only writes their action buffers, so every arm acts on the same observation."""

    def __init__(self):
        import torch
        from test_policy_gpu import _small_engine
        self.C, self.S1, self.S2 = ss.independent_streams(3)
        assert all(s.cuda_stream != 0 for s in (self.C, self.S1, self.S2))
        self.engs = [_small_engine(E, steps=20, stream=s) for E, s in ((3, self.S1), (70, self.S2))]
        self.blank = [torch.full((e.n_envs, 2, e.rowcap), -7, dtype=torch.int32, device="cuda") for e in self.engs]
        torch.cuda.synchronize()

    def clear(self):
        import torch
        for e, b in zip(self.engs, self.blank):
            e.rollout_write("actions", b)
        torch.cuda.synchronize()

    def actions(self):
        from test_policy_gpu import _actions
        return [_actions(e).clone() for e in self.engs]


def rig():
    if "rig" not in _RIG:
        _RIG["rig"] = Rig()
    return _RIG["rig"]


def _env():
    if "env" not in _RIG:
        import magent
        _RIG["env"] = magent.GridWorld("battle", map_size=40)
    return _RIG["env"]


def _model(algo, lr=0.05):
    """A model of `algo` with the weights and the draw seed every other call of this gives (two arms: two models)."""
    import torch
    from mfrl_amd.algo import spawn_ai
    env = _env()
    torch.manual_seed(3)
    m = spawn_ai(algo, None, env, env.get_handles()[0], "order-" + algo, 50, memory_size=256)
    for g in m.optimizer.param_groups:                  # one step moves every weight by about lr: other actions
        g["lr"] = lr
    return m


def _net_of(m):
    return m.eval_net if hasattr(m, "eval_net") else m.net


def _tensors(algo, seed):
    """Fixed tensors shaped like the model's parameters (the gradients of the optimiser step; with 0.05 x them added, a
    second set of weights for load_state_dict)."""
    import torch
    key = ("tensors", algo, seed)
    if key not in _RIG:
        g = torch.Generator(device="cuda").manual_seed(seed)
        _RIG[key] = [torch.randn(p.shape, device="cuda", generator=g) for p in _net_of(_model(algo)).parameters()]
        torch.cuda.synchronize()
    return _RIG[key]


def _state_dict2(algo):
    import torch
    key = ("sd2", algo)
    if key not in _RIG:
        net = copy.deepcopy(_net_of(_model(algo)))
        with torch.no_grad():
            for p, t in zip(net.parameters(), _tensors(algo, 77)):
                p.add_(0.05 * t)
        _RIG[key] = {k: v.detach().clone() for k, v in net.state_dict().items()}
        torch.cuda.synchronize()
    return _RIG[key]


def move_step(m, algo):
    """A torch optimiser step (Adam) from fixed gradients."""
    for p, g in zip(_net_of(m).parameters(), _tensors(algo, 5)):
        p.grad = g
    m.optimizer.step()


def move_load(m, algo):
    _net_of(m).load_state_dict(_state_dict2(algo))


def move_none(m, algo):
    pass


MOVES = {"step": move_step, "load_state_dict": move_load}
ORDER2 = [(0, 0), (1, 0), (0, 1), (1, 1)]          # (engine, group): both engines alternately, both groups


def _act_calls(models, engs, order, only=None):
    """model.act_rollout per (engine k, group) of `order`, the draw counter set so that call i draws with step i + 1
    whichever model makes it (a private model per engine draws what the shared one does)."""
    for i, (k, grp) in enumerate(order):
        if only is not None and k != only:
            continue
        models[k]._draws = i
        models[k].act_rollout(engs[k], grp)


def _serial(r, algo, move, order, setup=None):
    """The serial arm: per engine a private model, the caller on that engine's stream, no stall."""
    import torch
    r.clear()
    for k in sorted({k for k, _ in order}):
        m = _model(algo)
        if setup:
            setup(m)
        with torch.cuda.stream(r.engs[k].torch_stream()):
            move(m, algo)
            _act_calls({k: m}, r.engs, order, only=k)
    torch.cuda.synchronize()
    return r.actions()


def _stalled(r, name, algo, move, order, setup=None, stalled=None):
    """The stalled arm: one model, the caller on C, C stalled first; -> (actions, the case)."""
    import torch

    def seq(m):
        with torch.cuda.stream(r.C):
            move(m, algo)
            _act_calls({0: m, 1: m}, r.engs, order)
        return m

    def fresh():
        m = _model(algo)
        if setup:
            setup(m)
        return m

    case = ss.Case(name, stalled if stalled is not None else r.C)
    case.warm(lambda: seq(fresh()))
    m = fresh()
    r.clear()
    case.run(lambda: seq(m))
    return r.actions(), case


def _same(got, want, ks=(0, 1)):
    import torch
    for k in ks:
        assert torch.equal(got[k], want[k]), "engine %d: %d of %d action slots differ" % (
            k, int((got[k] != want[k]).sum()), got[k].numel())
        assert int((want[k] >= 0).sum()) > 100


def _differ(a, b, k=0):
    """The moved weights act differently from the unmoved ones on at least a tenth of the live rows: a stale read
    would show."""
    live = a[k] >= 0
    assert int((a[k][live] != b[k][live]).sum()) * 10 >= int(live.sum()), (
        int((a[k][live] != b[k][live]).sum()), int(live.sum()))


# ----------------------------------------------------------------------------------------------- the harness itself
def test_streams_are_independent_and_the_stall_is_linear():
    """The three streams of every case below are pairwise independent as measured, none is the default stream, and a
    stall of 50 ms takes 50 ms within a factor of 1.5."""
    r = rig()
    cal = ss.calibration()
    assert len({s.cuda_stream for s in (r.C, r.S1, r.S2)}) == 3
    assert r.engs[0].stream_handle() == r.S1.cuda_stream and r.engs[1].stream_handle() == r.S2.cuda_stream
    assert cal["asked_ms"] / 1.5 <= cal["timed_ms"] <= cal["asked_ms"] * 1.5, cal


def test_control_c_entries_promise_no_ordering():
    """The control.  mfx_qnet_set_weights(W2, stream=C) with C stalled, then mfx_qnet_act_rollout(stream=S) on a handle
    that holds W1: the C entries order nothing between streams, so the engine acts with W1 -- bit for bit a private W1
    handle's actions, and not a private W2 handle's.  If this ever sees W2's actions the harness no longer shows a
    missing edge (the streams share a queue, the stall is too short, or something synchronises), and every other case
    in this file passes vacuously.  Every access is inside a live allocation and reads fully written data: the blob
    and the images hold W1 until the stall ends."""
    import torch
    from mfrl_amd import check
    from mfrl_amd.policy import QNetHIP, _rollout_args
    from test_policy_gpu import _net
    r = rig()
    eng = r.engs[0]
    w1 = _net(True, 9)
    w2 = copy.deepcopy(w1)
    g = torch.Generator(device="cuda").manual_seed(4)
    with torch.no_grad():
        for p in w2.parameters():
            p.add_(0.1 * torch.randn(p.shape, device="cuda", generator=g))

    def handle(net):
        return QNetHIP(VIEW, FEAT, NA, True).load(net)

    def act(q, stream_handle):
        buf, rows, total = _rollout_args(q._rows, eng, 0, ("view", "feature", "group_num", "mean_action", "actions"))
        check(q._L.mfx_qnet_act_rollout(q.handle, buf["view"], buf["feature"], buf["group_num"], buf["mean_action"],
                                        int(eng.mean_stride()), eng.n_envs, 2, 0, eng.rowcap, rows, total,
                                        buf["actions"], stream_handle), "mfx_qnet_act_rollout")

    def serial(net):
        r.clear()
        with torch.cuda.stream(r.S1):
            q = handle(net)
            act(q, r.S1.cuda_stream)
        torch.cuda.synchronize()
        return r.actions()

    a1, a2 = serial(w1), serial(w2)
    live = a1[0][:, 0] >= 0
    n_live = int(live.sum())
    assert n_live >= 100
    assert int((a1[0][:, 0][live] != a2[0][:, 0][live]).sum()) * 4 >= n_live          # the serial arm's precondition

    def seq(q, blob):
        check(q._L.mfx_qnet_set_weights(q.handle, blob.data_ptr(), q.blob_n, r.C.cuda_stream), "mfx_qnet_set_weights")
        act(q, r.S1.cuda_stream)
        return q

    blob2 = handle(w2)._blob
    shared = handle(w1)
    act(shared, r.S1.cuda_stream)                               # (the handle's first launch on S: its per-stream buffer)
    case = ss.Case("control", r.C)
    case.warm(lambda: seq(handle(w1), blob2))
    r.clear()
    case.run(lambda: seq(shared, blob2))
    got = r.actions()
    assert case.outlived, "the stall was over before act_rollout was enqueued: the control proves nothing"
    assert torch.equal(got[0], a1[0]), "the control saw ordered (or torn) weights: the harness no longer shows a missing edge"
    assert not torch.equal(got[0], a2[0])
    # after the stall the handle does hold W2
    r.clear()
    act(shared, r.S1.cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(r.actions()[0], a2[0])


# ------------------------------------------------------------------------------- weights moved, then act_rollout
def _boltzmann(m):
    m.explore = "boltzmann"
    m.temperature = 0.7


@pytest.mark.parametrize("move", sorted(MOVES))
@pytest.mark.parametrize("algo,explore", [("mfq", "greedy"), ("mfq", "boltzmann"), ("ac", None), ("mfac", None)])
def test_weights_moved_then_act_rollout(algo, explore, move):
    """The weights move on C (a torch optimiser step, load_state_dict) behind the stall; act_rollout on the engine's
    stream follows at once.  The upload is enqueued on C behind the move, and the engine's stream waits for it
    (StreamOrder).  For AC / MFAC the handle is fresh: its support image is built in this call too."""
    r = rig()
    setup = _boltzmann if explore == "boltzmann" else None
    order = [(0, 0), (0, 1)]
    want = _serial(r, algo, MOVES[move], order, setup)
    _differ(want, _serial(r, algo, move_none, order, setup))
    got, case = _stalled(r, "moved-%s-%s-%s" % (algo, explore, move), algo, MOVES[move], order, setup)
    assert case.outlived
    _same(got, want, ks=(0,))


@pytest.mark.parametrize("algo", ["mfq", "mfac"])
def test_weights_moved_on_a_model_that_has_acted(algo):
    """As above with a model that acted on the engine before (the handle exists, the support is set, the engine's
    stream has seen the handle): only the upload is new in the sequence."""
    import torch
    r = rig()
    order = [(0, 0), (0, 1)]

    def acted_on(stream):
        def setup(m):
            with torch.cuda.stream(stream):
                m.act_rollout(r.engs[0], 0)
            torch.cuda.synchronize()
        return setup

    want = _serial(r, algo, move_step, order, acted_on(r.S1))
    got, case = _stalled(r, "moved-acted-%s" % algo, algo, move_step, order, acted_on(r.C))
    assert case.outlived
    _same(got, want, ks=(0,))


@pytest.mark.parametrize("algo", ["mfq", "mfac"])
def test_one_model_two_engines(algo):
    """One model, engines on S1 and S2, the caller on C, the weights just moved: act_rollout on both engines
    alternately.  Both engines' streams wait for the upload, not only the one that acted first."""
    r = rig()
    want = _serial(r, algo, move_step, ORDER2)
    _differ(want, _serial(r, algo, move_none, ORDER2), k=1)
    got, case = _stalled(r, "two-engines-%s" % algo, algo, move_step, ORDER2)
    assert case.outlived
    _same(got, want)


def test_act_precision_bf16_first_images():
    """act_precision = "bf16" on a fresh MFAC model after a move: the upload and the mode's first images are built on
    C behind the stall."""
    r = rig()

    def setup(m):
        m.act_precision = "bf16"

    want = _serial(r, "mfac", move_step, ORDER2, setup)
    got, case = _stalled(r, "bf16-first-images", "mfac", move_step, ORDER2, setup)
    assert case.outlived
    _same(got, want)


# ------------------------------------------------------------------------------------------- the raw ACNetHIP
def _acnet_blob():
    import torch
    from mfrl_amd.policy import ACNetHIP
    from test_policy_gpu import _acnet
    if "acblob" not in _RIG:
        _RIG["acblob"] = ACNetHIP(VIEW, FEAT, NA, True).pack(_acnet(True, 31)).contiguous()
        torch.cuda.synchronize()
    return _RIG["acblob"]


def _raw_acnet(precision="f32"):
    """A loaded, synchronised ACNetHIP whose support is not set yet."""
    import torch
    from mfrl_amd.policy import ACNetHIP
    hip = ACNetHIP(VIEW, FEAT, NA, True, precision=precision).set_blob(_acnet_blob())
    torch.cuda.synchronize()
    assert hip.input_support_size() == 0
    return hip


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_raw_acnet_builds_its_support_in_the_call(precision):
    """ACNetHIP.act_rollout(eng, support=True) on a loaded handle without a support, shared by the engines on S1 and
    S2, the caller on C with C stalled: the first call builds the support image on C (k_gather_rows,
    launch_weight_image) behind the stall, and k_acnet on each engine's stream waits for it."""
    import torch
    r = rig()

    def calls(hips, only=None):
        for i, (k, grp) in enumerate(ORDER2):
            if only is None or k == only:
                hips[k].act_rollout(r.engs[k], grp, seed=11, step=i + 1)

    r.clear()
    for k in (0, 1):
        hip = _raw_acnet(precision)
        with torch.cuda.stream(r.engs[k].torch_stream()):
            calls({k: hip}, only=k)
    torch.cuda.synchronize()
    want = r.actions()

    def seq(hip):
        with torch.cuda.stream(r.C):
            calls({0: hip, 1: hip})
        return hip

    case = ss.Case("raw-acnet-support-%s" % precision, r.C)
    case.warm(lambda: seq(_raw_acnet(precision)))
    hip = _raw_acnet(precision)
    r.clear()
    case.run(lambda: seq(hip))
    got = r.actions()
    assert hip.input_support_size() == 903
    assert case.outlived
    _same(got, want)


def test_replacing_a_support_synchronises_on_the_host():
    """set_input_support *replacing* a support frees the old one first: acnet_support_free (csrc/acnet_kernels.hip) goes
    through hipFree, which waits for the device.  So the stall is over when the call returns, and the forward after it
    is the serial one."""
    import torch
    from test_policy_gpu import _rollout_obs
    r = rig()
    view, feat, prob = (x[:300].contiguous() for x in _rollout_obs(E=4, steps=5))
    mask = r.engs[0].view_support(0)
    other = mask.copy()
    other[np.nonzero(mask == 0)[0][:7]] = 1                     # (a superset: the view is zero there all the same)
    hip = _raw_acnet().set_input_support(mask)
    want = hip.forward(view, feat, seed=3, step=2)
    torch.cuda.synchronize()

    def replace(h):
        with torch.cuda.stream(r.C):
            h.set_input_support(other)
        return h

    case = ss.Case("support-replaced", r.C)
    case.warm(lambda: replace(_raw_acnet().set_input_support(mask)))
    hip2 = _raw_acnet().set_input_support(mask)
    torch.cuda.synchronize()
    case.run(lambda: replace(hip2))                             # (`outlived` is read as set_input_support returns)
    assert case.outlived is False
    with torch.cuda.stream(r.C):
        got = hip2.forward(view, feat, seed=3, step=2)
    torch.cuda.synchronize()
    assert hip2.input_support_size() == int(other.sum())
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])


def test_refused_support_leaves_the_handle_alone():
    """A mask of the wrong size is refused before anything is freed: input_support_size() is unchanged and a forward
    is bit-identical to the one before (it used to drop the handle to the dense order while ACNetHIP._support still
    held the old mask)."""
    import torch
    from mfrl_amd import EngineError
    from test_policy_gpu import _rollout_obs
    r = rig()
    view, feat, prob = (x[:300].contiguous() for x in _rollout_obs(E=4, steps=5))
    mask = r.engs[0].view_support(0)
    hip = _raw_acnet().set_input_support(mask)
    before = hip.forward(view, feat, prob, want_value=True, seed=3, step=2)
    torch.cuda.synchronize()
    gen = hip._order.gen
    for bad in (mask[:-1], np.concatenate([mask, mask[:1]])):
        with pytest.raises(EngineError, match="entries"):
            hip.set_input_support(bad)
        assert hip.input_support_size() == 903 and np.array_equal(hip._support, mask) and hip._order.gen == gen
        after = hip.forward(view, feat, prob, want_value=True, seed=3, step=2)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, after))
    hip.set_input_support(None)
    assert hip.input_support_size() == 0


# ------------------------------------------------------------------------------------ the "hip" training backends
def test_value_net_hip_backend_then_act_rollout(capsys):
    """train_batches under the "hip" backend, then act_rollout.  _train_batches_hip synchronises on the host
    (algo/base.py: `code, bad = tr.error()`, "the one synchronisation of the round") before it exports the blobs into
    the torch modules, whose version counters move: the next act_rollout re-packs and uploads.  So the stall is over
    when train_batches returns; the upload after it is ordered by the handle like any other."""
    import torch
    from test_qtrain_gpu import _filled_memory, ctx
    r = rig()
    c = ctx(True, 11)
    order = [(0, 0), (1, 0)]

    def setup(m):
        m.eval_net.load_state_dict(c.eval_net.state_dict())
        m.target_net.load_state_dict(c.target_net.state_dict())
        _filled_memory(m, c)
        m.train_backend = "hip"
        m.lr = 0.01
        torch.cuda.synchronize()

    def move(m, algo):
        np.random.seed(5)
        m.train_batches(m.replay_buffer, 2, True)

    want = _serial(r, "mfq", move, order, setup)
    _differ(want, _serial(r, "mfq", move_none, order, setup))
    got, case = _stalled(r, "mfq-hip-backend", "mfq", move, order, setup)
    capsys.readouterr()
    assert case.outlived is False
    _same(got, want)


def _pushed_rows(m):
    """40 rows of 8 agents pushed into the model's EpisodesBuffer (tests/test_actrain_gpu.py builds them so)."""
    import actrain_ref as ar
    from mfrl_amd.algo import tools
    rows = ar.rows(int(np.prod(VIEW)), FEAT[0], NA, m._use_mf, 11, 40)
    np.random.seed(7)                                           # (push inserts the agents in a drawn order)
    m.replay_buffer = tools.EpisodesBuffer(use_mean=m._use_mf)
    m.flush_buffer(state=(rows["obs"].reshape(-1, 13, 13, 7), rows["feat"]), acts=rows["act"], rewards=rows["ret"],
                   alives=np.ones(40, dtype=bool), ids=np.arange(40) % 8, prob=rows.get("prob"))


@pytest.mark.parametrize("algo", ["ac", "mfac"])
def test_ac_hip_backend_train_then_act_rollout(algo, capsys):
    """train() under the "hip" backend, then act_rollout on both engines.  _hip_train hands the trained blob to the
    acting handle itself (set_blob on the current stream) and moves _hip_key, so the next act_rollout sees an unchanged
    key: it is the handle, not the key, that orders the engines behind the upload.  train() then synchronises on the
    host (algo/ac.py: `self._hip_train(cols, len(reward))[1].tolist()`, after set_blob on the same stream), so the
    stall is over when it returns."""
    import torch
    r = rig()

    def setup(m):
        m.train_backend = "hip"
        m.learning_rate = 0.01
        _pushed_rows(m)
        torch.cuda.synchronize()

    def move(m, algo):
        m.train()

    want = _serial(r, algo, move, ORDER2, setup)
    _differ(want, _serial(r, algo, move_none, ORDER2, setup), k=1)
    got, case = _stalled(r, "%s-hip-train" % algo, algo, move, ORDER2, setup)
    capsys.readouterr()
    assert case.outlived is False
    _same(got, want)


# ------------------------------------------------------------------------------------- train_rollout and its rows
class _Round:
    """A model of `algo` with the rows of 25 scripted steps of the "few" plan (40x40, 2 envs) collected from an engine
    on `stream`, left in its buffer; acts: the scripted actions of a next round of 4 steps, made ahead."""

    def __init__(self, algo, stream, backend, advantage="returns"):
        import torch
        import test_collect_ac_gpu as tc
        from test_policy_big_gpu import scripted_actions
        with torch.cuda.stream(stream):
            self.eng = tc._engine("few")
        assert self.eng.stream_handle() == stream.cuda_stream
        self.model = m = _model(algo)
        m.train_backend = backend
        m.learning_rate = 0.01
        m.advantage = advantage
        self.col = m.rollout_collector(self.eng, 0)
        self.n = tc._scripted(self.eng, self.col)
        self.rows = m.replay_buffer._rows
        self.snap = self.rows.cols["rew"][:self.n].clone()
        rng = np.random.default_rng(17)
        self.acts = [torch.from_numpy(scripted_actions(rng, self.eng.n_envs, self.eng.rowcap)).cuda() for _ in range(4)]
        assert self.n > 1000
        torch.cuda.synchronize()

    def restore(self):
        import torch
        self.rows.cols["rew"][:self.n].copy_(self.snap)
        self.rows.n = self.n
        torch.cuda.synchronize()

    def next_round(self):
        """Four scripted steps with the collector around each: the rows land where the trained rows lay."""
        for a in self.acts:
            self.eng.rollout_write("actions", a)
            self.col.begin()
            self.eng.rollout_policy_step()
            self.col.end()

    def next_rows(self):
        n = self.col.finish()
        assert n > 100
        return {k: v[:n].clone() for k, v in self.rows.cols.items()}


def _grads_equal(a, b):
    import torch
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("backend", ["hip", "torch"])
@pytest.mark.parametrize("algo", ["ac", "mfac"])
def test_train_rollout_behind_a_stalled_engine(algo, backend, capsys):
    """train_rollout(step=False) with S stalled before the call: the chain walk and the bootstrap forward sit behind
    the stall on the engine's stream, and the training on C waits for them (algo/ac.py:
    `torch.cuda.current_stream().wait_stream(col.eng.torch_stream())`).  The call synchronises on the host before that
    edge matters -- `tails = c["tail"][:n].nonzero()` under the engine's stream, and chain_returns waits for its error
    word -- so the stall is over when it returns.  The gradient is the serial arm's: bit for bit under "hip", and under
    "torch" when torch repeats its own gradient bit for bit on these rows (the rule of tests/test_gae_gpu.py)."""
    import torch
    r = rig()
    a = _Round(algo, r.S1, backend)
    with torch.cuda.stream(r.S1):
        want = a.model.train_rollout(step=False)
        a.restore()
        again = a.model.train_rollout(step=False)
    torch.cuda.synchronize()
    repeats = _grads_equal(want, again)
    b = _Round(algo, r.S1, backend)

    def seq(x):
        with torch.cuda.stream(r.C):
            return x.model.train_rollout(step=False)

    case = ss.Case("train-rollout-S-stalled-%s-%s" % (algo, backend), r.S1)
    a.restore()
    case.warm(lambda: seq(a))
    got = case.run(lambda: seq(b))
    capsys.readouterr()
    print("%s repeats its own gradient bit for bit: %s" % (backend, repeats))
    assert case.outlived is False
    assert backend == "torch" or repeats
    assert _grads_equal(got, want) or not repeats


@pytest.mark.parametrize("backend", ["hip", "torch"])
def test_next_round_overwrites_the_trained_rows(backend, capsys):
    """train_rollout(step=False) with C stalled before the call, and at once the next round's scripted steps on S,
    whose rows overwrite the rows the training reads: the engine's stream waits for the training (algo/ac.py:
    `col.eng.torch_stream().wait_stream(torch.cuda.current_stream())`, both backends).  train_rollout then reads its
    statistics back (`stats.tolist()` / `sums.tolist()`, behind the training on the same stream), so the stall is over
    when it returns and the next round starts on an idle C.  The gradient and the next round's rows are the serial
    arm's."""
    import torch
    r = rig()
    a = _Round("mfac", r.S1, backend)

    def seq(x, stream):
        with torch.cuda.stream(stream):
            g = x.model.train_rollout(step=False)
            x.next_round()
        return g

    want = seq(a, r.S1)
    torch.cuda.synchronize()
    want_rows = a.next_rows()
    b, w = _Round("mfac", r.S1, backend), _Round("mfac", r.S1, backend)
    case = ss.Case("next-round-C-stalled-%s" % backend, r.C)
    case.warm(lambda: seq(w, r.C))
    got = case.run(lambda: seq(b, r.C))
    got_rows = b.next_rows()
    capsys.readouterr()
    assert case.outlived is False
    if backend == "hip":
        assert _grads_equal(got, want)
    assert sorted(got_rows) == sorted(want_rows)
    for k in want_rows:
        assert torch.equal(got_rows[k], want_rows[k]), k


def test_gae_round_after_a_move_then_a_second_engine(capsys):
    """advantage = "gae" under the "hip" backend after the weights moved on C behind the stall, then act_rollout on a
    second engine.  The value forward of the round runs on the collector's engine's stream with the handle's upload
    taken on the caller's stream, where torch wrote the parameters; the second engine's stream waits for the handle's
    last upload (the trained blob) like the first.  train_rollout synchronises on the host (the chain walk's error
    word, `stats.tolist()`), so the stall is over when it returns.  The parameters after the step and the second
    engine's actions are the serial arm's."""
    import torch
    r = rig()

    def seq(x, stream, eng_k):
        with torch.cuda.stream(stream):
            move_step(x.model, "mfac")
            x.model.train_rollout()
            for grp in (0, 1):
                x.model._draws = 10 + grp
                x.model.act_rollout(r.engs[eng_k], grp)
        return x

    a = _Round("mfac", r.S2, "hip", "gae")                      # serial: everything on the second engine's stream
    r.clear()
    seq(a, r.S2, 1)
    torch.cuda.synchronize()
    want, want_p = r.actions(), [p.detach().clone() for p in a.model.net.parameters()]
    b, w = _Round("mfac", r.S1, "hip", "gae"), _Round("mfac", r.S1, "hip", "gae")
    case = ss.Case("gae-second-engine", r.C)
    case.warm(lambda: seq(w, r.C, 1))
    r.clear()
    case.run(lambda: seq(b, r.C, 1))
    got = r.actions()
    capsys.readouterr()
    assert case.outlived is False
    assert _grads_equal([p.detach() for p in b.model.net.parameters()], want_p)
    _same(got, want, ks=(1,))


# --------------------------------------------------------------------------------------- the neighbourhood mean
def test_prob_rows_from_the_neighbourhood_mean():
    """NeighborMean.rows, written on the engine's stream by update(), read by QNetHIP.act_rollout(prob_rows=) and by
    the collector's begin() on the same stream, the caller on C and S stalled first: three steps enqueued behind the
    stall.  The edge is same-stream, as the docstrings claim: the actions and the collected rows (the prob column
    among them) are the serial arm's."""
    import torch
    from mfrl_amd import mf
    from mfrl_amd.algo.tools import MemoryGroup
    from mfrl_amd.policy import QNetHIP
    from mfrl_amd.replay import RolloutCollector
    from test_policy_gpu import _net, _small_engine
    r = rig()
    net = _net(True, 9)

    class Arm:
        def __init__(self):
            self.eng = _small_engine(3, steps=20, stream=r.S1)
            with torch.cuda.stream(r.S1):
                self.q = QNetHIP(VIEW, FEAT, NA, True).load(net)
            self.nm = mf.NeighborMean(self.eng, 0, 6)
            self.nm.reset()
            self.mg = MemoryGroup(VIEW, FEAT, NA, 1000, 64, 8, use_mean=True)
            self.col = RolloutCollector(self.eng, self.mg, 0, prob_rows=self.nm.rows)
            torch.cuda.synchronize()

        def steps(self, stream):
            with torch.cuda.stream(stream):
                for _ in range(3):
                    self.q.act_rollout(self.eng, 0, prob_rows=self.nm.rows)
                    self.q.act_rollout(self.eng, 1)
                    self.col.begin()
                    self.eng.rollout_policy_step()
                    self.col.end()
                    self.nm.update()
            return self

        def result(self):
            from test_policy_gpu import _actions
            n = self.col.finish()
            assert n > 300
            out = {k: v[:n].clone() for k, v in self.mg._rows.cols.items()}
            out["nm"], out["actions"] = self.nm.rows.clone(), _actions(self.eng)
            return out

    want = Arm().steps(r.S1).result()
    assert float(want["prob"].abs().sum()) > 0 and float(want["nm"].abs().sum()) > 0
    case = ss.Case("prob-rows-S-stalled", r.S1)
    case.warm(lambda: Arm().steps(r.C))
    b = Arm()
    case.run(lambda: b.steps(r.C))
    got = b.result()
    assert case.outlived
    assert sorted(got) == sorted(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


# ------------------------------------------------------------------------------------------------- end to end
def _losses(text):
    return [line for line in text.splitlines() if line.startswith("[*] LOSS:") or line.startswith("[*] PG_LOSS:")]


@pytest.mark.parametrize("algo", ["mfq", "mfac"])
def test_two_training_rounds_with_the_engine_on_its_own_stream(algo, capsys):
    """Two rounds of play_rollout (mfq) / play_rollout_episodes (mfac) with train=True under the "hip" backend, 40x40,
    2 envs, 10 steps: the engine on S1 and the caller on C, a stall armed on C as each round's loop begins (behind the
    round's rollout_policy_observe, so that the round's first uploads and acts are enqueued under it), against the
    engine on the caller's own stream.  The final parameters and the printed losses are equal.

    The stall is still pending at each round's first policy step: nothing between the round's first upload and its
    first step synchronises on the host.  (The blocking hipMemcpy of mfx_acnet_set_input_support runs on the null
    stream; it held the host for the whole stall whenever the stalled stream shared its hardware queue with the null
    stream, which is why stream_stall.independent_streams also measures every stream against the null stream.)"""
    import torch
    import magent
    from mfrl_amd.algo import spawn_ai
    from mfrl_amd.algo.play import play_rollout, play_rollout_episodes
    from mfrl_amd.battle import BattleBatch
    r = rig()
    map_size, E, max_steps = 40, 2, 10
    play = play_rollout if algo == "mfq" else play_rollout_episodes
    env = magent.GridWorld("battle", map_size=map_size)

    def run(stream, stall_ms):
        torch.manual_seed(3)
        np.random.seed(1)
        models = [spawn_ai(algo, None, env, env.get_handles()[g], "e2e-%s-%d" % (algo, g), max_steps, memory_size=1500)
                  for g in range(2)]
        for m in models:
            m.train_backend = "hip"
        eng = BattleBatch(map_size, E, stream=stream)
        seen, host_ms = [], []
        observe, step = eng.rollout_policy_observe, eng.rollout_policy_step
        pending = []

        def observe_then_stall():
            observe()
            torch.cuda.synchronize()
            ev = ss.stall(r.C, stall_ms[len(seen)]) if stall_ms else None
            pending.append((ev, time.perf_counter()))

        def step_and_look():
            if pending:                                     # the round's first step: its first acts are enqueued
                ev, t0 = pending.pop()
                host_ms.append(1e3 * (time.perf_counter() - t0))
                seen.append(ev is not None and not ev.query())
            step()

        eng.rollout_policy_observe, eng.rollout_policy_step = observe_then_stall, step_and_look
        capsys.readouterr()
        with torch.cuda.stream(r.C):
            for k in range(2):
                play(eng, k, map_size, max_steps, models, eps=1.0, train=True, left_id=0)
        torch.cuda.synchronize()
        net = models[0].eval_net if algo == "mfq" else models[0].net
        return [p.detach().clone() for p in net.parameters()], _losses(capsys.readouterr().out), seen, host_ms

    # the stall's length by the rule of every case: 20 x the host time the same enqueues took in the other arm (a first
    # round makes the handles and the row storage: tens of milliseconds of allocation), at least 50 ms, at most 500
    want_p, want_l, _, host_ms = run(r.C, None)
    stall_ms = [min(ss.MAX_MS, max(ss.MIN_MS, ss.FACTOR * t)) for t in host_ms]
    got_p, got_l, seen, host2 = run(r.S1, stall_ms)
    rec = json.dumps({"case": "e2e-" + algo, "enqueue_ms_serial": host_ms, "enqueue_ms": host2, "stall_ms": stall_ms,
                      "outlived": seen, "calibration": ss.calibration()})
    print(rec)
    if os.environ.get("STREAM_STALL_OUT"):
        with open(os.environ["STREAM_STALL_OUT"], "a") as f:
            f.write(rec + "\n")
    assert seen == [True, True]
    assert len(want_l) >= 2 and got_l == want_l
    assert _grads_equal(got_p, want_p)
