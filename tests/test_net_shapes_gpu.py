"""The four network paths on the GPU off the Battle shape (view 13 x 13 x 7, F = 34, A = 21 -- the one shape every other
test of these kernels builds), over the ranges include/magent_amd.h documents.  tests/net_shapes.py holds the cases, the
networks, the inputs and the float64 references; tests/test_net_shapes_cpu.py pins them and their preconditions
without a GPU.  One batch everywhere: 131 rows -- two full 64-agent tiles and a 3-row tail, whose wave has 13 clamped
junk lanes while the tile's other three waves are all junk.

What the shapes reach that the Battle shape never ran:

* k_acnet with h_emb held in registers (F >= 37, one workgroup per CU); with h_emb in LDS and the bias through
  relu_unit (F = 36, no free input row to fold it into); the bias row on the last feature register (F = 35);
  Vp % 16 = 4, 8, 12 (a partial last chunk of the view GEMM); V < 16 (one chunk, the two-ahead view ring past the end
  from the start); V < 48 (the 3-slot ring never wraps); V = 4096; A = 32 (no padded policy column), A = 2,
  Ap != A at A = 21 and elsewhere; the plain (kMF = false) instantiation on a mean-field net (value not asked for).
* The Q network, f32 and bf16: Fp % 16 != 0, F = 1, F = 256 (the bf16 head's eight-step unroll), A = 1, 2, 32.
* The training step: backward through padded Fp / Ap rows at three more (F, A) pairs, padding staying zero -- under the
  max target and under the opt-in Boltzmann target (qt_row<kSoft>) at T = 1 and 0.1.

Bounds: the project's own for a correct kernel -- policy 1e-5, value 1e-5 max(1, max |value|), q 1e-5 max(1, max |q|)
(the torch f32 modules differ from the float64 network on the same weights by at most 1.8e-6, 4e-7 and 9e-7 of those
scales on these inputs); bf16: tests/qnet_bf16_ref.py's self-calibrating e_q per case.  Every forward case first asserts
the sensitivity precondition on its float64 reference (net_shapes), so a kernel that reads zeros for an operand -- what
an LDS region outside the workgroup's allocation gives -- fails by three orders of magnitude."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import acnet_ref
import net_shapes as ns
import qnet_bf16_ref as qb
import qtrain_ref as qr

pytestmark = pytest.mark.gpu
N = ns.N


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


# ------------------------------------------------------------------------------------------------- ACNet
def _acnet_hip(r):
    from mfrl_amd.policy import ACNetHIP
    V, F, A, mf = r.case
    net = copy.deepcopy(r.net).cuda()
    return ACNetHIP((V,), (F,), A, mf).load(net), net


def _acnet_check(tag, got, want_policy, want_value, vscale):
    """got = (policy, value, act) of a forward with seed 77, step 5: within the bounds of the reference, and the draw
    the host restatement on the kernel's own policy rows."""
    pol, val, act = (x.cpu().numpy() for x in got)
    perr = float(np.abs(pol.astype(np.float64) - want_policy).max())
    verr = float(np.abs(val.astype(np.float64) - want_value).max())
    print("%s: policy err %.3e, value err %.3e (scale %.3f)" % (tag, perr, verr, vscale))
    assert perr <= ns.TOL, (tag, perr)
    assert verr <= ns.TOL * vscale, (tag, verr, vscale)
    assert np.array_equal(act, acnet_ref.draw(pol, 77, 5, 0, np.arange(len(pol)))), tag


@pytest.mark.parametrize("case", ns.ACNET_CASES, ids=ns.case_id)
def test_acnet_forward(case):
    """Policy, value and draw of all 131 rows against the float64 forward on the packed blob and against the torch
    ACNet; without the value (the kMF = false instantiation, also for a mean-field net) the policy and the draw are the
    same bits."""
    V, F, A, mf = case
    r = ns.acnet_case(*case)
    for k, x in r.sensitivity().items():
        assert x >= ns.SENSITIVITY, (k, x)
    hip, net = _acnet_hip(r)
    view, feat, prob = _dev(r.view), _dev(r.feat), _dev(r.prob)
    got = hip.forward(view, feat, prob, want_value=True, seed=77, step=5)
    pol2, val2, act2 = hip.forward(view, feat, None, want_value=False, seed=77, step=5)
    with torch.no_grad():
        wp, wv = net(view, feat, prob if mf else None)
    torch.cuda.synchronize()
    assert got[0].shape == (N, A) and got[1].shape == (N,) and got[2].shape == (N,) and val2 is None
    _acnet_check("acnet %s vs float64" % (case,), got, r.policy, r.value, r.vscale)
    _acnet_check("acnet %s vs torch" % (case,), got, wp.double().cpu().numpy(), wv.double().cpu().numpy(),
                 max(1.0, float(wv.abs().max())))
    assert torch.equal(pol2, got[0]) and torch.equal(act2, got[2])


@pytest.mark.parametrize("case", ns.ACNET_SUPPORT_CASES, ids=ns.case_id)
def test_acnet_input_support(case):
    """A random support of density 0.55, the view zero outside it: the forward over the support equals the dense one
    bit for bit and is within the bounds of the reference (F = 40: the packed order needs h_emb in LDS and is not
    taken; the result must be right all the same).  A support with one input in 20 floats, whose packed chunks span more
    than 255 floats, is refused with the documented error, leaves no support set, and the next dense forward is right."""
    from magent.c_lib import EngineError
    V, F, A, mf = case
    r = ns.acnet_case(*case)
    mask = ns.support_mask(V)
    assert 0.45 * V < mask.sum() < 0.65 * V
    v = r.view * mask
    want_p, want_v = r.forward(v, r.feat, r.prob)
    p0, _ = r.forward(0 * v, r.feat, r.prob)
    assert np.median(np.abs(p0 - want_p).max(1)) >= ns.SENSITIVITY * ns.TOL      # (the masked view still matters)
    hip, _ = _acnet_hip(r)
    view, feat, prob = _dev(v), _dev(r.feat), _dev(r.prob)
    dense = hip.forward(view, feat, prob, want_value=True, seed=77, step=5)
    hip.set_input_support(mask)
    assert hip.input_support_size() == int(mask.sum())
    packed = hip.forward(view, feat, prob, want_value=True, seed=77, step=5)
    torch.cuda.synchronize()
    for a, b in zip(dense, packed):
        assert torch.equal(a, b)
    vscale = max(1.0, float(np.abs(want_v).max()))
    _acnet_check("acnet %s support" % (case,), packed, want_p, want_v, vscale)
    with pytest.raises(EngineError, match="packed chunk .* spans"):
        hip.set_input_support(ns.sparse_mask(V))
    assert hip.input_support_size() == 0
    again = hip.forward(view, feat, prob, want_value=True, seed=77, step=5)
    torch.cuda.synchronize()
    _acnet_check("acnet %s after the refusal" % (case,), again, want_p, want_v, vscale)
    for a, b in zip(dense, again):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- Q-net
def _qnet_hip(r, precision="f32"):
    from mfrl_amd.policy import QNetHIP
    F, A, mf = r.case
    hip = QNetHIP((13, 13, 7), (F,), A, mf, precision=precision).load(copy.deepcopy(r.net).cuda())
    q, act = hip.forward(_dev(r.view), _dev(r.feat), _dev(r.prob) if mf else None)
    torch.cuda.synchronize()
    assert q.shape == (N, A) and act.shape == (N,)
    return q.cpu().double().numpy(), act.cpu().numpy()


@pytest.mark.parametrize("case", ns.QNET_CASES, ids=ns.case_id)
def test_qnet_forward(case):
    """Q values against the float64 forward on the packed blob; the greedy action equal wherever the float64 top-two
    gap exceeds the bound, which at least 99 % of rows do; one action: always action 0."""
    F, A, mf = case
    r = ns.qnet_case(*case)
    for k, x in r.sensitivity().items():
        assert x >= ns.SENSITIVITY * ns.TOL * r.scale, (k, x, r.scale)
    q, act = _qnet_hip(r)
    err = float(np.abs(q - r.q).max())
    clear = r.clear(ns.TOL * r.scale)
    print("qnet %s: err %.3e scale %.3f clear %.3f" % (case, err, r.scale, clear.mean()))
    assert err <= ns.TOL * r.scale, (err, r.scale)
    assert clear.mean() >= 0.99
    assert np.array_equal(act[clear], np.argmax(r.q, 1)[clear])
    if A == 1:
        assert not act.any()


@pytest.mark.parametrize("case", ns.BF16_CASES, ids=ns.case_id)
def test_qnet_bf16_forward(case):
    """precision="bf16" on the fixture views: |q - reference| <= e_q and |q - exact| <= 2 e_q with the case's own e_q
    (tests/test_policy_bf16_gpu.py's bounds), the actions on the clear rows, the kernel's argmax its own first maximum."""
    F, A, mf = case
    r = ns.qnet_case(F, A, mf, True)
    for k, x in r.sensitivity_bf16().items():
        assert x > 2.0 * r.e_q, (k, x, r.e_q)
    q, act = _qnet_hip(r, "bf16")
    d_exact, d_ref = float(np.abs(q - r.q).max()), float(np.abs(q - r.quant).max())
    clear = qb.clear_rows(r.q, r.e_q)
    print("bf16 %s: e_q %.4e scale %.3f |q-exact|/e_q %.3f |q-ref|/e_q %.3f clear %.3f"
          % (case, r.e_q, r.scale, d_exact / r.e_q, d_ref / r.e_q, clear.mean()))
    assert d_exact <= 2.0 * r.e_q, (d_exact, r.e_q)
    assert d_ref <= r.e_q, (d_ref, r.e_q)
    assert np.array_equal(act[clear], np.argmax(r.q, 1)[clear])
    assert np.array_equal(act, np.argmax(q, 1))


# ------------------------------------------------------------------------------------------------- training step
LR, TAU, GAMMA = 1e-4, 0.005, 0.95
_CTX = {}


class Ctx:
    """tests/test_qtrain_gpu.py's context at another (F, A): nets, blobs, the ring on the device, the padding mask and
    the ring's smallest argmax gap."""

    def __init__(self, F, A, use_mf, seed):
        from mfrl_amd.policy import blob_layout
        self.F, self.A, self.use_mf, self.seed = F, A, use_mf, seed
        self.n, self.off = blob_layout(F, A, use_mf)
        self.eval_net, self.target_net = qr.nets(use_mf, seed, F, A)
        self.eb = qb.packed(self.eval_net, use_mf, F, A)[0]
        self.tb = qb.packed(self.target_net, use_mf, F, A)[0]
        self.ring = r = qr.ring(seed, F, A)
        dev = lambda x, dt: _dev(x).to(dt).contiguous()
        self.cols = {"obs0": dev(r["obs"], torch.float32), "feat0": dev(r["feat"], torch.float32),
                     "actions": dev(r["act"], torch.int32), "rewards": dev(r["rew"], torch.float32),
                     "terminals": dev(r["term"], torch.uint8), "masks": dev(r["mask"], torch.uint8),
                     "prob": dev(r["prob"], torch.float32) if use_mf else None}
        self.pad = qr.padding_mask(self.off, F, A, use_mf, self.n)
        NR = qr.N_RING
        q = np.sort(qr.qnet_ref.forward(self.eb.astype(np.float64), self.off, F, A, use_mf, r["obs"][:NR], r["feat"][:NR],
                                        r["prob"][:NR] if use_mf else None), axis=1)
        self.gap = float((q[:, -1] - q[:, -2]).min())

    def handle(self):
        from mfrl_amd import qtrain
        tr = qtrain.QTrainHIP((13, 13, 7), (self.F,), self.A, self.use_mf, lr=LR, tau=TAU, gamma=GAMMA)
        tr.set_state(qtrain.EVAL, torch.as_tensor(self.eb))
        tr.set_state(qtrain.TARGET, torch.as_tensor(self.tb))
        return tr


def _ctx(case):
    if case not in _CTX:
        _CTX[case] = Ctx(*case)
    return _CTX[case]


@pytest.mark.parametrize("case", ns.QTRAIN_CASES, ids=ns.case_id)
def test_qtrain_gradient_accuracy(case):
    """tests/test_qtrain_gpu.py::test_gradient_accuracy's method at (F, A, use_mf) = (37, 32, mean field), (1, 2, mean
    field) and (256, 20, DQN), B = 20: per block e_hip <= 4 e_torch against the float64 restatement (torch's f32
    autograd on the GPU the yardstick), the gradient's padding bits all zero, the loss and mean q[a] within 1e-4.

    The seeds were chosen on the CPU from the restatement alone (the first from 11 on that meets the preconditions
    below; tests/test_net_shapes_cpu.py::test_qtrain_preconditions asserts them without a GPU) -- all three are 11:
        (37, 32, mf)   smallest argmax gap 6.714e-05, smallest block scale max |g64| 6.668e-03 (block 8, wp1)
        (1, 2, mf)     gap 4.883e-01, scale 4.593e-02 (block 10, wp2)
        (256, 20, DQN) gap 6.385e-05, scale 4.451e-02 (block 4, wd)
    QTRAIN_ERROR_OUT=<path>: the measured figures are appended there (profiles/qtrain_shapes_error.jsonl is such a run)."""
    F, A, use_mf, seed = case
    c = _ctx(case)
    NR, B = qr.N_RING, ns.QTRAIN_B
    assert c.gap > 2e-5, c.gap
    idx = qr.index_list(seed, B)
    assert (NR - 1) in idx and len(set(idx.tolist())) < B and c.ring["mask"][idx].sum() >= 15
    e64, t64 = c.eb.astype(np.float64), c.tb.astype(np.float64)
    y, _ = qr.targets(e64, t64, c.off, F, A, use_mf, c.ring, NR, idx, GAMMA)
    g64, loss64, qa64 = qr.gradient(e64, t64, c.off, F, A, use_mf, c.ring, NR, idx, GAMMA, y=y)
    tr = c.handle()
    g, stats = tr.grads(c.cols, NR, torch.as_tensor(idx, device="cuda"))
    tr.check_error()
    g, stats = g.cpu().numpy(), stats.cpu().numpy()
    named, t_loss, t_qa = qr.torch_gradient(c.eval_net, use_mf, c.ring, idx, y, torch.float32, "cuda")
    g_t = qr.pack64(named, F, A, use_mf, c.off, c.n)
    e_hip, e_torch = qr.block_errors(g, g64, c.off, c.n), qr.block_errors(g_t, g64, c.off, c.n)
    rec = {"F": F, "A": A, "use_mf": int(use_mf), "seed": seed, "B": B, "e_hip": [e[0] for e in e_hip],
           "e_torch": [e[0] for e in e_torch], "max_g64": [e[1] for e in e_hip], "loss": float(stats[0]), "loss64": loss64,
           "torch_loss": t_loss, "mean_qa": float(stats[1]), "mean_qa64": qa64, "min_gap": c.gap}
    print(json.dumps(rec))
    if os.environ.get("QTRAIN_ERROR_OUT"):
        with open(os.environ["QTRAIN_ERROR_OUT"], "a") as f:
            f.write(json.dumps(rec) + "\n")
    assert c.pad.any() and np.all(g[c.pad].view(np.uint32) == 0)
    for k in range(18):
        if not use_mf and 8 <= k < 12:
            assert e_hip[k] == (0.0, 0.0), k
            continue
        assert e_hip[k][1] >= 1e-3, (k, e_hip[k])
        assert e_hip[k][0] <= 4.0 * e_torch[k][0], (k, e_hip[k][0], e_torch[k][0])
    assert abs(float(stats[0]) - loss64) <= 1e-4 * max(1.0, loss64)
    assert abs(float(stats[1]) - qa64) <= 1e-4 * max(1.0, abs(qa64))


@pytest.mark.parametrize("case", ns.QTRAIN_CASES, ids=ns.case_id)
def test_qtrain_padding_stays_zero(case):
    """After ten steps of 64-row minibatches the eval and target blobs and both Adam moments are zero, bit for bit,
    on every padding entry (we rows past F, wp1 rows past A, wq / bq columns past A, conv1's 64th row; a DQN blob's
    mean-field blocks) and not zero elsewhere."""
    c = _ctx(case)
    tr = c.handle()
    idx = _dev(np.random.RandomState(400 + c.seed).randint(qr.N_RING, size=(10, 64)).astype(np.int64))
    tr.run(c.cols, qr.N_RING, idx)
    tr.check_error()
    assert tr.step_count() == 10
    for k in range(4):
        s = tr.get_state(k).cpu().numpy()
        assert np.all(s[c.pad].view(np.uint32) == 0), k
        assert np.any(s[~c.pad] != 0), k


def _torch_soft_target(c, idx, T):
    """torch's own f32 Boltzmann target on the GPU from its own f32 forwards of the next rows
    (tests/test_qtarget_gpu.py's yardstick)."""
    nxt = (np.asarray(idx) + 1) % qr.N_RING
    t = lambda x: torch.as_tensor(np.asarray(x), device="cuda").float()
    with torch.no_grad():
        args = (t(c.ring["obs"][nxt]), t(c.ring["feat"][nxt]), t(c.ring["prob"][nxt]) if c.use_mf else None)
        q_e = copy.deepcopy(c.eval_net).cuda()(*args)
        q_t = copy.deepcopy(c.target_net).cuda()(*args)
        v = (torch.softmax(q_e / T, dim=1) * q_t).sum(dim=1)
        y = t(c.ring["rew"][idx]) + ((1.0 - t(c.ring["term"][idx])) * v) * GAMMA
    return y.cpu().numpy()


@pytest.mark.parametrize("T", ns.QTRAIN_SOFT_T)
@pytest.mark.parametrize("case", ns.QTRAIN_CASES, ids=ns.case_id)
def test_qtrain_boltzmann_gradient_accuracy(case, T):
    """test_qtrain_gradient_accuracy under set_target("boltzmann", T) -- qt_row<kSoft>, tested at the Battle shape alone
    by tests/test_qtarget_gpu.py::test_gradient_accuracy, whose method this is: the float64 restatement is fed the
    float64 Boltzmann target (qtarget_ref.target64), the yardstick is torch's f32 autograd with its own f32 Boltzmann
    target from its own forwards, so both sides carry the target's f32 error.  The checks and the bound are unchanged:
    per block e_hip <= 4 e_torch on a block scale of at least 1e-3, the padding bits zero, the stats within 1e-4.
    tests/test_net_shapes_cpu.py::test_qtrain_boltzmann_preconditions holds the case seeds to this rule's own
    preconditions.  QTRAIN_ERROR_OUT=<path>: the figures are appended there
    (profiles/qtrain_boltzmann_shapes_error.jsonl is such a run)."""
    F, A, use_mf, seed = case
    c = _ctx(case)
    NR, B = qr.N_RING, ns.QTRAIN_B
    idx = qr.index_list(seed, B)
    assert (NR - 1) in idx and len(set(idx.tolist())) < B and c.ring["mask"][idx].sum() >= 15
    e64, t64 = c.eb.astype(np.float64), c.tb.astype(np.float64)
    y, q_e, q_t = ns.qtrain_soft_target64(e64, t64, c.off, F, A, use_mf, c.ring, NR, idx, GAMMA, T)
    assert np.isfinite(q_e).all() and np.isfinite(q_t).all()
    g64, loss64, qa64 = qr.gradient(e64, t64, c.off, F, A, use_mf, c.ring, NR, idx, GAMMA, y=y)
    tr = c.handle()
    tr.set_target("boltzmann", T)
    g, stats = tr.grads(c.cols, NR, torch.as_tensor(idx, device="cuda"))
    tr.check_error()
    g, stats = g.cpu().numpy(), stats.cpu().numpy()
    named, t_loss, t_qa = qr.torch_gradient(c.eval_net, use_mf, c.ring, idx, _torch_soft_target(c, idx, T), torch.float32,
                                            "cuda")
    g_t = qr.pack64(named, F, A, use_mf, c.off, c.n)
    e_hip, e_torch = qr.block_errors(g, g64, c.off, c.n), qr.block_errors(g_t, g64, c.off, c.n)
    rec = {"target": "boltzmann", "T": T, "F": F, "A": A, "use_mf": int(use_mf), "seed": seed, "B": B,
           "e_hip": [e[0] for e in e_hip], "e_torch": [e[0] for e in e_torch], "max_g64": [e[1] for e in e_hip],
           "loss": float(stats[0]), "loss64": loss64, "torch_loss": t_loss, "mean_qa": float(stats[1]), "mean_qa64": qa64,
           "max_ratio": max(e_hip[k][0] / e_torch[k][0] for k in range(18) if e_torch[k][0] > 0)}
    print(json.dumps(rec))
    if os.environ.get("QTRAIN_ERROR_OUT"):
        with open(os.environ["QTRAIN_ERROR_OUT"], "a") as f:
            f.write(json.dumps(rec) + "\n")
    assert c.pad.any() and np.all(g[c.pad].view(np.uint32) == 0)
    for k in range(18):
        if not use_mf and 8 <= k < 12:
            assert e_hip[k] == (0.0, 0.0), k
            continue
        assert e_hip[k][1] >= 1e-3, (k, e_hip[k])
        assert e_hip[k][0] <= 4.0 * e_torch[k][0], (k, e_hip[k][0], e_torch[k][0])
    assert abs(float(stats[0]) - loss64) <= 1e-4 * max(1.0, loss64)
    assert abs(float(stats[1]) - qa64) <= 1e-4 * max(1.0, abs(qa64))
