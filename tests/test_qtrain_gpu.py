"""The HIP training step of the Q network (csrc/qtrain_kernels.hip, mfrl_amd.qtrain.QTrainHIP) on the GPU against
the float64 restatement tests/qtrain_ref.py: gradient accuracy with torch's own f32 autograd as the yardstick, padding,
one step = Adam on its own gradient, determinism, run = the loop, the device guards, and the "hip" backend of
ValueNet.train_batches.

Inputs (qtrain_ref): the 256 fixture observation rows, n = 200 live ring entries inside 256-row tensors (an unguarded
idx = n would still stay inside the allocation), columns from RandomState(100 + seed), nets qnet_bf16_ref.net(use_mf,
seed) (eval) and net(use_mf, seed + 100) (target), seeds 11 and 12.

QTRAIN_ERROR_OUT=<path>: the gradient test appends its measured figures per case there (profiles/qtrain_error.jsonl
is such a run)."""
import json
import os

import numpy as np
import pytest
import torch

import qnet_bf16_ref as qb
import qtrain_ref as qr

pytestmark = pytest.mark.gpu

F, A, N = qr.F, qr.A, qr.N_RING
LR, TAU, GAMMA = 1e-4, 0.005, 0.95
_CTX = {}


class Ctx:
    def __init__(self, use_mf, seed):
        from mfrl_amd.policy import blob_layout
        self.use_mf, self.seed = use_mf, seed
        self.n, self.off = blob_layout(F, A, use_mf)
        self.eval_net, self.target_net = qr.nets(use_mf, seed)
        self.eb = qb.packed(self.eval_net, use_mf)[0]
        self.tb = qb.packed(self.target_net, use_mf)[0]
        self.ring = r = qr.ring(seed)
        dev = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x), device="cuda").to(dt).contiguous()
        self.cols = {"obs0": dev(r["obs"], torch.float32), "feat0": dev(r["feat"], torch.float32),
                     "actions": dev(r["act"], torch.int32), "rewards": dev(r["rew"], torch.float32),
                     "terminals": dev(r["term"], torch.uint8), "masks": dev(r["mask"], torch.uint8),
                     "prob": dev(r["prob"], torch.float32) if use_mf else None}
        self.pad = qr.padding_mask(self.off, F, A, use_mf, self.n)
        # precondition of every comparison with the float64 target: no ring row's argmax is a near tie
        q = np.sort(qr.qnet_ref.forward(self.eb.astype(np.float64), self.off, F, A, use_mf, r["obs"][:N], r["feat"][:N],
                                        r["prob"][:N] if use_mf else None), axis=1)
        self.gap = float((q[:, -1] - q[:, -2]).min())

    def handle(self, eb=None, tb=None):
        from mfrl_amd import qtrain
        tr = qtrain.QTrainHIP((13, 13, 7), (F,), A, self.use_mf, lr=LR, tau=TAU, gamma=GAMMA)
        tr.set_state(qtrain.EVAL, torch.as_tensor(self.eb if eb is None else eb))
        tr.set_state(qtrain.TARGET, torch.as_tensor(self.tb if tb is None else tb))
        return tr

    def batches(self, k, B=64):
        """k index lists of B from RandomState(400 + seed)."""
        return torch.as_tensor(np.random.RandomState(400 + self.seed).randint(N, size=(k, B)).astype(np.int64), device="cuda")


def ctx(use_mf, seed):
    key = (bool(use_mf), seed)
    if key not in _CTX:
        _CTX[key] = Ctx(*key)
    return _CTX[key]


def states(tr):
    """(eval, target, m, v) as numpy float32."""
    return [tr.get_state(k).cpu().numpy() for k in range(4)]


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ------------------------------------------------------------------------------------------------- 1: gradient
@pytest.mark.parametrize("B", [64, 20, 272])
@pytest.mark.parametrize("seed", [11, 12])
@pytest.mark.parametrize("use_mf", [False, True])
def test_gradient_accuracy(use_mf, seed, B):
    """Per block of the blob, e = max |g - g64| / max |g64| against the float64 restatement; torch's f32 autograd on
    the GPU over the same rows is the yardstick: e_hip <= 4 e_torch (another summation tree over at most 7,744 terms,
    each product rounded once on both sides; a layout, permutation or masking mistake gives errors of order 1).
    Stats: |loss - loss64| <= 1e-4 max(1, loss64), the same for mean q[a]."""
    c = ctx(use_mf, seed)
    assert c.gap > 2e-5, c.gap
    idx = qr.index_list(seed, B)
    assert (N - 1) in idx and len(set(idx.tolist())) < B and c.ring["mask"][idx].sum() >= 15
    e64, t64 = c.eb.astype(np.float64), c.tb.astype(np.float64)
    y, _ = qr.targets(e64, t64, c.off, F, A, use_mf, c.ring, N, idx, GAMMA)
    g64, loss64, qa64 = qr.gradient(e64, t64, c.off, F, A, use_mf, c.ring, N, idx, GAMMA, y=y)
    tr = c.handle()
    g, stats = tr.grads(c.cols, N, torch.as_tensor(idx, device="cuda"))
    tr.check_error()
    g, stats = g.cpu().numpy(), stats.cpu().numpy()
    named, t_loss, t_qa = qr.torch_gradient(c.eval_net, use_mf, c.ring, idx, y, torch.float32, "cuda")
    g_t = qr.pack64(named, F, A, use_mf, c.off, c.n)
    e_hip, e_torch = qr.block_errors(g, g64, c.off, c.n), qr.block_errors(g_t, g64, c.off, c.n)
    rec = {"use_mf": int(use_mf), "seed": seed, "B": B, "e_hip": [e[0] for e in e_hip], "e_torch": [e[0] for e in e_torch],
           "max_g64": [e[1] for e in e_hip], "loss": float(stats[0]), "loss64": loss64, "torch_loss": t_loss,
           "mean_qa": float(stats[1]), "mean_qa64": qa64, "min_gap": c.gap}
    print(json.dumps(rec))
    if os.environ.get("QTRAIN_ERROR_OUT"):
        with open(os.environ["QTRAIN_ERROR_OUT"], "a") as f:
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


# ------------------------------------------------------------------------------------------------- 2: padding
@pytest.mark.parametrize("use_mf", [False, True])
def test_padding_stays_zero(use_mf):
    c = ctx(use_mf, 11)
    tr = c.handle()
    tr.run(c.cols, N, c.batches(10))
    tr.check_error()
    assert tr.step_count() == 10
    for k, s in enumerate(states(tr)):
        assert np.all(s[c.pad].view(np.uint32) == 0), k
        assert np.any(s[~c.pad] != 0), k


# ------------------------------------------------------------------------------------------------- 3: one step
@pytest.mark.parametrize("use_mf", [False, True])
def test_step_is_adam_on_its_gradient(use_mf):
    """Ten consecutive steps; each: read the state, mfx_qtrain_grads, mfx_qtrain_run of that one minibatch, read the
    state again.  The after-state must be the float64 restatement (qtrain_ref.adam, step number t) applied to the
    before-state and that gradient, per element within
        eval, target:  2^-23 |p| + lr 2^-16     (an update is at most ~4 lr; a dozen f32 operations of 2^-24 relative)
        m:             2^-22 (|b1 m| + |(1 - b1) g|);   v: 2^-22 v      (three roundings and two rounded constants)
    A stuck step counter, a stale weight in da2 or a wrong soft-update order each give ~1e-4 (five orders more)."""
    c = ctx(use_mf, 12)
    tr = c.handle()
    idx = c.batches(10)
    for t in range(1, 11):
        before = states(tr)
        g, _ = tr.grads(c.cols, N, idx[t - 1])
        g = g.cpu().numpy().astype(np.float64)
        assert same_bits(states(tr), before)                      # grads changes no state
        tr.run(c.cols, N, idx[t - 1:t])
        tr.check_error()
        assert tr.step_count() == t
        after = states(tr)
        p, tg, m, v = qr.adam(*before, g, t, lr=LR, tau=TAU)
        for name, got, want, bound in (
                ("eval", after[0], p, 2.0 ** -23 * np.abs(p) + LR * 2.0 ** -16),
                ("target", after[1], tg, 2.0 ** -23 * np.abs(tg) + LR * 2.0 ** -16),
                ("m", after[2], m, 2.0 ** -22 * (np.abs(0.9 * before[2].astype(np.float64)) + np.abs(0.1 * g))),
                ("v", after[3], v, 2.0 ** -22 * v)):
            err = np.abs(got.astype(np.float64) - want)
            worst = int(np.argmax(err - bound))
            assert np.all(err <= bound), (t, name, worst, err[worst], bound[worst])
    assert np.abs(after[0] - c.eb).max() > 5 * LR             # ten steps moved the weights


# ------------------------------------------------------------------------------------------------- 4: determinism
@pytest.mark.parametrize("use_mf", [False, True])
def test_bitwise_deterministic(use_mf):
    c = ctx(use_mf, 11)
    idx = c.batches(10)
    a, b = c.handle(), c.handle()
    ga = a.grads(c.cols, N, idx[3])[0].cpu().numpy()
    gb = a.grads(c.cols, N, idx[3])[0].cpu().numpy()
    assert same_bits(ga, gb)
    sa = a.run(c.cols, N, idx).cpu().numpy()
    sb = b.run(c.cols, N, idx).cpu().numpy()
    a.check_error()
    b.check_error()
    assert same_bits(sa, sb) and np.all(np.isfinite(sa))
    for x, y in zip(states(a), states(b)):
        assert same_bits(x, y)


# ------------------------------------------------------------------------------------------------- 5: run = loop
def test_run_is_the_loop():
    c = ctx(True, 12)
    idx = c.batches(6, B=20)
    a, b = c.handle(), c.handle()
    sa = a.run(c.cols, N, idx).cpu().numpy()
    sb = np.concatenate([b.run(c.cols, N, idx[i:i + 1]).cpu().numpy() for i in range(6)])
    a.check_error()
    b.check_error()
    assert a.step_count() == b.step_count() == 6
    assert same_bits(sa, sb)
    for x, y in zip(states(a), states(b)):
        assert same_bits(x, y)


# ------------------------------------------------------------------------------------------------- 6: guards
def test_guards():
    from mfrl_amd import qtrain
    c = ctx(True, 11)
    tr = c.handle()
    tr.run(c.cols, N, c.batches(2))
    tr.check_error()
    before = states(tr)
    good = c.batches(1)[0]
    for bad_idx, code in ((N, 1), (-1, 1)):
        idx = good.clone()
        idx[7] = bad_idx
        tr.run(c.cols, N, idx.reshape(1, -1))
        assert tr.error() == (code, bad_idx)
        assert tr.error() == (0, 0)                              # cleared
        assert tr.step_count() == 2 and same_bits(states(tr), before)
    cols = dict(c.cols)
    cols["actions"] = c.cols["actions"].clone()
    cols["actions"][int(good[5])] = A
    tr.run(cols, N, good.reshape(1, -1))
    with pytest.raises(qtrain.QTrainError):
        tr.check_error()
    assert tr.step_count() == 2 and same_bits(states(tr), before)
    for B in (0, 4097):
        with pytest.raises(ValueError):
            tr.run(c.cols, N, torch.zeros((1, B), dtype=torch.int64, device="cuda"))
        import ctypes
        ring = tr._ring(c.cols)
        z = torch.zeros(max(B, 1), dtype=torch.int64, device="cuda")
        assert tr._L.mfx_qtrain_run(tr.handle, ctypes.byref(ring), ctypes.c_longlong(N), ctypes.c_void_p(z.data_ptr()), 1,
                                    B, None, None) != 0          # the C entry refuses it too
    tr.run(c.cols, N, good.reshape(1, -1))                       # and the handle still works
    tr.check_error()
    assert tr.step_count() == 3 and not same_bits(states(tr)[0], before[0])


# ------------------------------------------------------------------------------------------------- 7: ValueNet
def _filled_memory(model, c):
    """The model's MemoryGroup holding the shared ring: N live entries."""
    buf = model.replay_buffer
    src = {"obs0": c.cols["obs0"].reshape(-1, 13, 13, 7), "feat0": c.cols["feat0"], "actions": c.cols["actions"],
           "rewards": c.cols["rewards"], "terminals": c.cols["terminals"].bool(), "masks": c.cols["masks"].bool(),
           "prob": c.cols["prob"]}
    for k, t in src.items():
        mb = getattr(buf, k)
        mb.data[:N] = t[:N]
        mb.length = N
    return buf


def _first_loss(text):
    line = [l for l in text.splitlines() if l.startswith("[*] LOSS:")][0]
    return float(line.split()[2])


def test_value_net_backend(capsys):
    import magent
    from mfrl_amd import qtrain
    from mfrl_amd.algo import spawn_ai
    from mfrl_amd.algo.base import weights_key
    from mfrl_amd.policy import pack_qnet
    c = ctx(True, 11)
    env = magent.GridWorld("battle", map_size=20)
    h = env.get_handles()
    models = [spawn_ai("mfq", None, env, h[0], "mfq-" + k, 50, memory_size=256) for k in ("torch", "hip")]
    for m in models:
        m.eval_net.load_state_dict(c.eval_net.state_dict())
        m.target_net.load_state_dict(c.target_net.state_dict())
        _filled_memory(m, c)
    mt, mh = models
    assert mt.train_backend == "torch" and mh.train_backend == "torch"
    mh.train_backend = "hip"
    with pytest.raises(ValueError):
        mh.train_backend = "triton"
    key0 = weights_key(mh.eval_net, mh._wgen)
    a0 = mh.act_dev(state=[c.cols["obs0"].reshape(-1, 13, 13, 7), c.cols["feat0"]], prob=c.cols["prob"], eps=0.1)
    np.random.seed(5)
    capsys.readouterr()
    mt.train_batches(mt.replay_buffer, 4, True)
    loss_t = _first_loss(capsys.readouterr().out)
    rs_t = np.random.get_state()
    np.random.seed(5)
    mh.train_batches(mh.replay_buffer, 4, True)
    loss_h = _first_loss(capsys.readouterr().out)
    rs_h = np.random.get_state()
    assert rs_t[0] == rs_h[0] and np.array_equal(rs_t[1], rs_h[1]) and rs_t[2:] == rs_h[2:]
    assert abs(loss_h - loss_t) <= 1e-4 * max(1.0, abs(loss_t)), (loss_h, loss_t)
    assert getattr(mt, "_qtrain", None) is None                  # the default path never touches the handle
    tr = mh._qtrain
    assert tr.step_count() == 4
    layout = (tr.blob_n, tr.offsets)
    assert torch.equal(pack_qnet(mh.eval_net, F, A, True, layout), tr.get_state(qtrain.EVAL))
    assert torch.equal(pack_qnet(mh.target_net, F, A, True, layout), tr.get_state(qtrain.TARGET))
    assert weights_key(mh.eval_net, mh._wgen) != key0
    mh.act_dev(state=[c.cols["obs0"].reshape(-1, 13, 13, 7), c.cols["feat0"]], prob=c.cols["prob"], eps=0.1)
    assert torch.equal(mh._hip._blob, tr.get_state(qtrain.EVAL)) and a0.shape[0] == qr.RING_ROWS
    # a second call packs nothing (the nets did not move) and goes on from the handle's moments
    mh.train_batches(mh.replay_buffer, 2, True)
    assert tr.step_count() == 6
    # the model's hyper-parameters are read at every call, as on the torch path: with lr = 0 the eval net stands still
    mh.lr = 0.0
    before = tr.get_state(qtrain.EVAL).clone()
    mh.train_batches(mh.replay_buffer, 1, True)
    assert tr.step_count() == 7 and torch.equal(tr.get_state(qtrain.EVAL), before)


def test_ring_of_two_million_rows():
    """train_battle keeps up to 2,000,000 replay rows (9.5 GB of views): row offsets pass 2^31 floats and 2^32 bytes.
    The shared ring's 200 live rows sit at the top of a 2,000,000-entry ring (row 0 = the small ring's row 0, where the
    last row wraps to), so the gradient must be bit for bit the small ring's; one minibatch is then applied."""
    c = ctx(True, 11)
    n_big = 2000000
    base = n_big - N
    cols = {}
    for k, t in c.cols.items():
        big = torch.empty((n_big,) + tuple(t.shape[1:]), dtype=t.dtype, device="cuda")
        big[base:] = t[:N]
        big[0] = t[0]
        big[1:base:max(1, base // 64)] = t[1]            # (a few rows in between: valid actions wherever probed)
        cols[k] = big
    idx = torch.as_tensor(qr.index_list(11, 20), device="cuda")
    small, big = c.handle(), c.handle()
    g_small, s_small = small.grads(c.cols, N, idx)
    g_big, s_big = big.grads(cols, n_big, idx + base)
    big.check_error()
    assert torch.equal(g_small, g_big) and torch.equal(s_small, s_big)
    big.run(cols, n_big, (idx + base).reshape(1, -1))
    small.run(c.cols, N, idx.reshape(1, -1))
    big.check_error()
    assert big.step_count() == 1
    for x, y in zip(states(big), states(small)):
        assert same_bits(x, y)
    bad = idx + base
    bad[3] = n_big
    big.run(cols, n_big, bad.reshape(1, -1))
    assert big.error() == (1, n_big)
    del cols, big
    torch.cuda.empty_cache()


def test_host_refusals():
    """eps = 0 (an all-zero entry would compute 0 / 0), a ring length outside int32 and a null handle are refused."""
    import ctypes
    c = ctx(False, 11)
    tr = c.handle()
    with pytest.raises(Exception):
        tr.set_hyper(LR, eps=0.0)
    tr.set_hyper(LR, tau=TAU, gamma=GAMMA)
    ring = tr._ring(c.cols)
    z = torch.zeros(64, dtype=torch.int64, device="cuda")
    L = tr._L
    for n in (0, 2 ** 31):
        assert L.mfx_qtrain_run(tr.handle, ctypes.byref(ring), ctypes.c_longlong(n), ctypes.c_void_p(z.data_ptr()), 1, 64,
                                None, None) != 0
    t = ctypes.c_longlong()
    assert L.mfx_qtrain_step_count(None, ctypes.byref(t)) != 0
    assert L.mfx_qtrain_run(None, ctypes.byref(ring), ctypes.c_longlong(N), ctypes.c_void_p(z.data_ptr()), 1, 64, None,
                            None) != 0
    assert L.mfx_qtrain_set_hyper(None, *[ctypes.c_double(x) for x in (LR, 0.9, 0.999, 1e-8, TAU, GAMMA)]) != 0
    assert tr.step_count() == 0


def test_backend_refuses_other_shapes():
    from mfrl_amd import qtrain
    assert not qtrain.supported((13, 13, 5), (34,), 21)
    assert not qtrain.supported((13, 13, 7), (34,), 33)
    with pytest.raises(ValueError):
        qtrain.QTrainHIP((9, 9, 7), (34,), 21)
