"""The opt-in Boltzmann mean-field value target on the GPU: the stand-alone kernel k_mfq_target_soft
(mfrl_amd.mf.mfq_target_boltzmann) against the numpy restatement tests/qtarget_ref.py and the float64 softmax, the soft
instantiation of the HIP training step (QTrainHIP.set_target) against tests/qtrain_ref.py, and ValueNet.target_rule on
both training backends.

Inputs of the training-step tests: those of tests/test_qtrain_gpu.py (its contexts are shared, built once).

QTARGET_ERROR_OUT=<path>: the gradient test appends its measured figures per case there (profiles/qtarget_error.jsonl
is such a run)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import common
import qsample_ref as qs
import qtarget_ref as qt
import qtrain_ref as qr
from test_qtrain_gpu import GAMMA, N, A, F, _filled_memory, _first_loss, ctx, same_bits, states

pytestmark = pytest.mark.gpu

LOW_T = 2.5e-5
FINITE_BATCHES = (0, 2, 3)
_ROWS = {}


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def rows(M, A_):
    """Random rows of the fixture's scale: e_q in +-3, t_q in +-10, done bytes 0 / 1 / other non-zero values."""
    key = (M, A_)
    if key not in _ROWS:
        rs = np.random.RandomState(1000 * A_ + M)
        _ROWS[key] = (rs.uniform(-3, 3, (M, A_)).astype(np.float32), rs.uniform(-10, 10, (M, A_)).astype(np.float32),
                      rs.randn(M).astype(np.float32), rs.choice(np.array([0, 0, 0, 1, 2, 255], dtype=np.uint8), M))
    return _ROWS[key]


def fixture():
    return np.load(os.path.join(common.GOLDEN, "algo_mfq_target.npz"))


def soft(eq, tq, r, done, T, want_w=True, gamma=GAMMA):
    from mfrl_amd import mf
    out = mf.mfq_target_boltzmann(dev(eq), dev(tq), dev(r), dev(done), gamma, T, want_w=want_w)
    return (out[0].cpu().numpy(), out[1].cpu().numpy()) if want_w else out.cpu().numpy()


# ------------------------------------------------------------------------------------------------- the stand-alone kernel
@pytest.mark.parametrize("T", [1.0, 0.1])
@pytest.mark.parametrize("A_", [2, 21, 32])
@pytest.mark.parametrize("M", [1, 255, 256, 257, 1000])
def test_kernel(M, A_, T):
    """The weights are q_sample's bit for bit; the target is the restatement on those weights bit for bit (sequential
    float64 sums of exact products); and v is within eps (max t_q - min t_q) of the float64 softmax's, per row, with
    eps = 2 (X 2^-23 + 2^-22), X = min(max_a |(e_q[a] - m) / T|, 104): the exponent's two float32 roundings (relative
    2^-24 each: X 2^-23 on the weight), expf's last place doubled for denormal weights (2^-22), and sum |p - p64| <=
    2 max relative weight error."""
    from mfrl_amd import mf
    eq, tq, r, done = rows(M, A_)
    assert M < 16 or (set(np.unique(done)) == {0, 1, 2, 255})
    y, w = soft(eq, tq, r, done, T)
    _, w_draw = mf.q_sample(dev(eq), T, 7, 3, want_w=True)
    assert w.dtype == np.float32 and w.tobytes() == w_draw.cpu().numpy().tobytes()
    assert y.dtype == np.float64 and y.tobytes() == qt.target(eq, tq, r, done, GAMMA, T, w=w).tobytes()
    assert (y[done != 0] == r[done != 0].astype(np.float64)).all()
    assert same_bits(soft(eq, tq, r, done, T, want_w=False), y)
    v = qt.value(w, tq)
    v64 = (qs.softmax64(eq, T) * tq.astype(np.float64)).sum(axis=1)
    x = np.abs((eq.astype(np.float64) - eq.max(axis=1, keepdims=True)) / float(np.float32(T))).max(axis=1)
    eps = 2.0 * (np.minimum(x, 104.0) * 2.0 ** -23 + 2.0 ** -22)
    bound = eps * (tq.max(axis=1).astype(np.float64) - tq.min(axis=1))
    err = np.abs(v - v64)
    print(json.dumps({"M": M, "A": A_, "T": T, "max_err_over_bound": float((err / bound).max())}))
    assert (err <= bound).all(), float((err / bound).max())


def test_fixture_limits_on_the_device():
    """T = 2.5e-5 on the fixture's finite, untied rows: the reference's max-rule target and mf.mfq_target, bit for bit.
    T = 1e30: every weight exactly 1, v the sequential float64 mean.  The NaN / 1e30 / tie batch: the restatement on the
    device's weights, non-finite rows one-hot at the greedy action."""
    from mfrl_amd import mf
    fx = fixture()
    for b in FINITE_BATCHES:
        eq, tq, r, done = [fx["b%d_%s" % (b, k)] for k in ("eq", "tq", "r", "done")]
        d8 = done.astype(np.uint8)
        y, w = soft(eq, tq, r, d8, LOW_T)
        assert ((w == 0) | (w == 1)).all() and (w.sum(1) == 1).all()
        assert y.tobytes() == fx["b%d_target" % b].tobytes(), b
        assert y.tobytes() == mf.mfq_target(dev(eq), dev(tq), dev(r), dev(d8), GAMMA).cpu().numpy().tobytes(), b
        y, w = soft(eq, tq, r, d8, 1e30)
        assert (w == 1).all()
        assert y.tobytes() == qt.target(eq, tq, r, d8, GAMMA, 1e30, w=np.ones_like(eq)).tobytes(), b
        assert y.tobytes() == qt.target(eq, tq, r, d8, GAMMA, 1e30).tobytes(), b
    eq, tq, r, done = [fx["b1_%s" % k] for k in ("eq", "tq", "r", "done")]
    d8 = done.astype(np.uint8)
    bad = ~qs.finite_rows(eq)
    assert bad.any()
    for T in (1.0, 0.1):
        y, w = soft(eq, tq, r, d8, T)
        assert w[bad].tobytes() == qt.weights(eq, T)[bad].tobytes()
        assert w.tobytes() == mf.q_sample(dev(eq), T, 1, 1, want_w=True)[1].cpu().numpy().tobytes()
        assert y.tobytes() == qt.target(eq, tq, r, d8, GAMMA, T, w=w).tobytes()
        assert np.isfinite(y).all()


def test_graph_follows_the_temperature():
    """One call captured with a tensor temperature (single stream, linear capture); each replay equals the direct call at
    the value the tensor then holds."""
    from mfrl_amd import mf
    eq, tq, r, done = (dev(x) for x in rows(257, 21))
    T = torch.ones(1, dtype=torch.float32, device="cuda")
    direct = {t: mf.mfq_target_boltzmann(eq, tq, r, done, GAMMA, t).cpu().numpy() for t in (1.0, 0.1)}
    assert same_bits(mf.mfq_target_boltzmann(eq, tq, r, done, GAMMA, T).cpu().numpy(), direct[1.0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = mf.mfq_target_boltzmann(eq, tq, r, done, GAMMA, T)
    got = {}
    for t in (1.0, 0.1):
        T.fill_(t)
        g.replay()
        got[t] = out.cpu().numpy().copy()
    assert same_bits(got[1.0], direct[1.0]) and same_bits(got[0.1], direct[0.1])
    assert not same_bits(got[1.0], got[0.1])


def test_refusals_launch_nothing():
    from mfrl_amd import lib, mf
    L = lib()
    L.mfx_mfq_target_boltzmann.restype = ctypes.c_int
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    M = 64
    out = torch.full((M,), -7.0, dtype=torch.float64, device="cuda")
    w = torch.full((M, 33), -7.0, dtype=torch.float32, device="cuda")
    buf = {a: [dev(x) for x in rows(M, a)] for a in (2, 21)}
    wide = torch.zeros((M, 33), dtype=torch.float32, device="cuda")

    def call(eq, tq, r, done, A_, T, d_T=None, m=M):
        return L.mfx_mfq_target_boltzmann(P(eq), P(tq), P(r), P(done), m, A_, ctypes.c_double(GAMMA), ctypes.c_float(T),
                                          P(d_T) if d_T is not None else None, P(out), P(w), None)

    eq, tq, r, done = buf[21]
    for A_ in (1, 33):
        assert call(wide, wide, r, done, A_, 0.1) != 0
    for T in (0.0, -1.0, float("inf"), float("nan")):
        assert call(eq, tq, r, done, 21, T) != 0
        with pytest.raises(ValueError):
            mf.mfq_target_boltzmann(eq, tq, r, done, GAMMA, T)
    assert call(eq, tq, r, done, 21, 0.1, m=0) == 0                 # M = 0: a no-op
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((w == -7.0).all())
    # a device-side temperature that is not finite and > 0: every target of the launch is NaN (the host's T is not read)
    for t in (0.0, -1.0, float("inf"), float("nan")):
        d_T = torch.full((1,), t, dtype=torch.float32, device="cuda")
        y = mf.mfq_target_boltzmann(eq, tq, r, done, GAMMA, d_T)
        assert bool(torch.isnan(y).all()), t
    d_T = torch.full((1,), 0.1, dtype=torch.float32, device="cuda")
    assert call(eq, tq, r, done, 21, float("nan"), d_T=d_T) == 0    # with d_T the host's T is not validated either
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), mf.mfq_target_boltzmann(eq, tq, r, done, GAMMA, 0.1).cpu().numpy())


# ------------------------------------------------------------------------------------------------- the HIP training step
def _next_q64(c, idx):
    nxt = (np.asarray(idx) + 1) % N
    pn = c.ring["prob"][nxt] if c.use_mf else None
    e64, t64 = c.eb.astype(np.float64), c.tb.astype(np.float64)
    q_t = qr.qnet_ref.forward(t64, c.off, F, A, c.use_mf, c.ring["obs"][nxt], c.ring["feat"][nxt], pn)
    q_e = qr.qnet_ref.forward(e64, c.off, F, A, c.use_mf, c.ring["obs"][nxt], c.ring["feat"][nxt], pn)
    return q_e, q_t


def _torch_soft_target(c, idx, T):
    """torch's own f32 soft target on the GPU from its own f32 forwards of the next rows."""
    nxt = (np.asarray(idx) + 1) % N
    t = lambda x: torch.as_tensor(np.asarray(x), device="cuda").float()
    with torch.no_grad():
        args = (t(c.ring["obs"][nxt]), t(c.ring["feat"][nxt]), t(c.ring["prob"][nxt]) if c.use_mf else None)
        if "cuda_nets" not in c.__dict__:
            import copy
            c.cuda_nets = (copy.deepcopy(c.eval_net).cuda(), copy.deepcopy(c.target_net).cuda())
        q_e, q_t = c.cuda_nets[0](*args), c.cuda_nets[1](*args)
        v = (torch.softmax(q_e / T, dim=1) * q_t).sum(dim=1)
        y = t(c.ring["rew"][idx]) + ((1.0 - t(c.ring["term"][idx])) * v) * GAMMA
    return y.cpu().numpy()


@pytest.mark.parametrize("T", [1.0, 0.1])
@pytest.mark.parametrize("B", [64, 20])
@pytest.mark.parametrize("use_mf", [False, True])
def test_gradient_accuracy(use_mf, B, T):
    """test_qtrain_gpu.test_gradient_accuracy's method and margin under the soft rule: per block of the blob,
    e = max |g - g64| / max |g64| against the float64 restatement fed the float64 soft target; the yardstick is torch's
    f32 autograd on the GPU over the same rows with its own f32 soft target from its own forwards, so both sides carry
    the target's f32 error: e_hip <= 4 e_torch.  Stats within 1e-4 max(1, .)."""
    seed = 11
    c = ctx(use_mf, seed)
    idx = qr.index_list(seed, B)
    assert (N - 1) in idx and len(set(idx.tolist())) < B and c.ring["mask"][idx].sum() >= 15
    e64, t64 = c.eb.astype(np.float64), c.tb.astype(np.float64)
    q_e, q_t = _next_q64(c, idx)
    y = qt.target64(q_e, q_t, c.ring["rew"][idx], c.ring["term"][idx], GAMMA, T)
    g64, loss64, qa64 = qr.gradient(e64, t64, c.off, F, A, use_mf, c.ring, N, idx, GAMMA, y=y)
    tr = c.handle()
    tr.set_target("boltzmann", T)
    g, stats = tr.grads(c.cols, N, torch.as_tensor(idx, device="cuda"))
    tr.check_error()
    g, stats = g.cpu().numpy(), stats.cpu().numpy()
    y_t = _torch_soft_target(c, idx, T)
    named, t_loss, t_qa = qr.torch_gradient(c.eval_net, use_mf, c.ring, idx, y_t, torch.float32, "cuda")
    g_t = qr.pack64(named, F, A, use_mf, c.off, c.n)
    e_hip, e_torch = qr.block_errors(g, g64, c.off, c.n), qr.block_errors(g_t, g64, c.off, c.n)
    rec = {"use_mf": int(use_mf), "seed": seed, "B": B, "T": T, "e_hip": [e[0] for e in e_hip],
           "e_torch": [e[0] for e in e_torch], "max_g64": [e[1] for e in e_hip], "loss": float(stats[0]), "loss64": loss64,
           "torch_loss": t_loss, "mean_qa": float(stats[1]), "mean_qa64": qa64,
           "max_ratio": max(e_hip[k][0] / e_torch[k][0] for k in range(18) if e_torch[k][0] > 0)}
    print(json.dumps(rec))
    if os.environ.get("QTARGET_ERROR_OUT"):
        with open(os.environ["QTARGET_ERROR_OUT"], "a") as f:
            f.write(json.dumps(rec) + "\n")
    assert np.all(g[c.pad].view(np.uint32) == 0)
    for k in range(18):
        if not use_mf and 8 <= k < 12:
            assert e_hip[k] == (0.0, 0.0), k
            continue
        assert e_hip[k][1] >= 1e-3, (k, e_hip[k])        # the block's scale is far above f32 noise: the ratio means something
        assert e_hip[k][0] <= 4.0 * e_torch[k][0], (k, e_hip[k][0], e_torch[k][0])
    assert abs(float(stats[0]) - loss64) <= 1e-4 * max(1.0, loss64)
    assert abs(float(stats[1]) - qa64) <= 1e-4 * max(1.0, abs(qa64))


@pytest.mark.parametrize("B", [64, 20])
@pytest.mark.parametrize("use_mf", [False, True])
def test_low_temperature_limit_is_the_max_step(use_mf, B):
    """No ring row's eval argmax is a near tie (gap > 2e-5), so at T = 1e-7 every non-maximal weight is exactly 0 and the
    soft step must be the max step bit for bit: weights from eval(next), values from target(next)."""
    c = ctx(use_mf, 11)
    assert c.gap > 2e-5, c.gap
    idx = torch.as_tensor(qr.index_list(11, B), device="cuda")
    a, b = c.handle(), c.handle()
    b.set_target("boltzmann", 1e-7)
    ga, sa = a.grads(c.cols, N, idx)
    gb, sb = b.grads(c.cols, N, idx)
    b.check_error()
    assert torch.equal(ga, gb) and torch.equal(sa, sb) and bool(torch.isfinite(sa).all())
    b.set_target("boltzmann", 1.0)                       # (and at T = 1 it is another step)
    assert not torch.equal(b.grads(c.cols, N, idx)[0], ga)


@pytest.mark.parametrize("T", [1.0, 0.1])
@pytest.mark.parametrize("use_mf", [False, True])
def test_bitwise_deterministic_and_run_is_the_loop(use_mf, T):
    c = ctx(use_mf, 11)
    idx = c.batches(6, B=20)
    a, b, l = c.handle(), c.handle(), c.handle()
    for tr in (a, b, l):
        tr.set_target("boltzmann", T)
    ga = a.grads(c.cols, N, idx[3])[0].cpu().numpy()
    gb = a.grads(c.cols, N, idx[3])[0].cpu().numpy()
    assert same_bits(ga, gb)
    sa = a.run(c.cols, N, idx).cpu().numpy()
    sb = b.run(c.cols, N, idx).cpu().numpy()
    sl = np.concatenate([l.run(c.cols, N, idx[i:i + 1]).cpu().numpy() for i in range(6)])
    for tr in (a, b, l):
        tr.check_error()
        assert tr.step_count() == 6
    assert same_bits(sa, sb) and same_bits(sa, sl) and np.all(np.isfinite(sa))
    for x, y, z in zip(states(a), states(b), states(l)):
        assert same_bits(x, y) and same_bits(x, z)


def test_max_after_boltzmann_is_a_fresh_max_handle():
    from mfrl_amd import qtrain
    c = ctx(True, 11)
    idx = c.batches(3)
    fresh, back = c.handle(), c.handle()
    assert back.target_rule == "max"
    back.set_target("boltzmann", 0.1)
    g_soft = back.grads(c.cols, N, idx[0])[0]
    with pytest.raises(ValueError):
        back.set_target("softmax", 0.1)
    for T in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(Exception):
            back.set_target("boltzmann", T)
    assert back.target_rule == "boltzmann" and torch.equal(back.grads(c.cols, N, idx[0])[0], g_soft)   # refusals change nothing
    assert back._L.mfx_qtrain_set_target(None, 0, ctypes.c_float(0.1)) != 0
    assert back._L.mfx_qtrain_set_target(back.handle, 2, ctypes.c_float(0.1)) != 0
    back.set_target("max", float("nan"))                 # the temperature is read only for "boltzmann"
    assert back.target_rule == "max"
    g_f, s_f = fresh.grads(c.cols, N, idx[0])
    g_b, s_b = back.grads(c.cols, N, idx[0])
    assert torch.equal(g_f, g_b) and torch.equal(s_f, s_b) and not torch.equal(g_f, g_soft)
    sf = fresh.run(c.cols, N, idx).cpu().numpy()
    sb = back.run(c.cols, N, idx).cpu().numpy()
    fresh.check_error()
    back.check_error()
    assert same_bits(sf, sb)
    for x, y in zip(states(fresh), states(back)):
        assert same_bits(x, y)
    assert qtrain.TARGET_RULES == {"max": 0, "boltzmann": 1}


# ------------------------------------------------------------------------------------------------- ValueNet
def test_value_net_target_rule(capsys, monkeypatch):
    import magent
    from mfrl_amd import mf, qtrain
    from mfrl_amd.algo import spawn_ai
    c = ctx(True, 11)
    env = magent.GridWorld("battle", map_size=20)
    h = env.get_handles()
    models = [spawn_ai("mfq", None, env, h[0], "mfq-" + k, 50, memory_size=256) for k in ("torch", "hip", "max")]
    for m in models:
        m.eval_net.load_state_dict(c.eval_net.state_dict())
        m.target_net.load_state_dict(c.target_net.state_dict())
        _filled_memory(m, c)
    mt, mh, mx = models
    mh.train_backend = "hip"
    for m in (mt, mh):
        assert m.target_rule == "max" and m.target_temperature is None
        with pytest.raises(ValueError):
            m.target_rule = "softmax"
        m.target_rule = "boltzmann"
        m.temperature = 0.1
    losses = []
    for m in (mt, mh):
        np.random.seed(5)
        capsys.readouterr()
        m.train_batches(m.replay_buffer, 4, True)
        losses.append(_first_loss(capsys.readouterr().out))
    loss_t, loss_h = losses
    assert abs(loss_h - loss_t) <= 1e-4 * max(1.0, abs(loss_t)), (loss_h, loss_t)
    assert mh._qtrain.target_rule == "boltzmann" and mh._qtrain.step_count() == 4
    # ... and it is the soft target that was trained: calc_target_q_dev is mf.mfq_target_boltzmann on the model's nets
    view, feat, prob = c.cols["obs0"][:N].reshape(-1, 13, 13, 7), c.cols["feat0"][:N], c.cols["prob"][:N]
    kw = dict(obs=view, feature=feat, prob=prob, rewards=c.cols["rewards"][:N], dones=c.cols["terminals"][:N])
    with torch.no_grad():
        e_q, t_q = mt.eval_net(view, feat, prob), mt.target_net(view, feat, prob)
    y_soft = mt.calc_target_q_dev(**kw)
    assert torch.equal(y_soft, mf.mfq_target_boltzmann(e_q, t_q, c.cols["rewards"][:N], c.cols["terminals"][:N], GAMMA, 0.1))
    mt.target_temperature = 1.0                              # a float overrides the last eps
    assert torch.equal(mt.calc_target_q_dev(**kw),
                       mf.mfq_target_boltzmann(e_q, t_q, c.cols["rewards"][:N], c.cols["terminals"][:N], GAMMA, 1.0))
    mt.target_temperature = None
    # the captured graph reads the temperature of the call at hand, not the one it was captured at
    graph = mt._graph
    assert graph is not None and float(mt._s_T.item()) == float(np.float32(0.1))
    mt.temperature = 1.0
    mt.train_batches(mt.replay_buffer, 1, True)
    assert mt._graph is graph and float(mt._s_T.item()) == 1.0
    mt.temperature = 0.0                                     # refused before anything is trained
    with pytest.raises(ValueError):
        mt.train_batches(mt.replay_buffer, 1, True)
    with pytest.raises(ValueError):
        mh.temperature = float("nan")
        mh.train_batches(mh.replay_buffer, 1, True)
    assert mh._qtrain.step_count() == 4
    mt.target_rule = "max"                                   # another rule drops the captured graph
    assert mt._graph is None
    assert not torch.equal(mt.calc_target_q_dev(**kw), y_soft)
    capsys.readouterr()
    # a model left at "max" never touches the new entry points, on either backend
    def boom(*a, **k):
        raise AssertionError("the max rule reached a Boltzmann-target entry point")
    monkeypatch.setattr(mf, "mfq_target_boltzmann", boom)
    monkeypatch.setattr(qtrain.QTrainHIP, "set_target", boom)
    mx.train_batches(mx.replay_buffer, 4, True)
    mx.calc_target_q_dev(**kw)
    mx.train_backend = "hip"
    mx.train_batches(mx.replay_buffer, 2, True)
    assert mx._qtrain.step_count() == 2 and mx._qtrain.target_rule == "max" and mx.target_rule == "max"
