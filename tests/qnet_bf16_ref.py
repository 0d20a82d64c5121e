"""Test infrastructure: the numerical contract of the Q network's bf16 forward (csrc/qnet_bf16_kernels.hip,
QNetHIP(precision="bf16")) restated in float64 numpy on the packed weight blob, in the manner of tests/qnet_ref.py.

    * operands of every matrix product rounded to bf16, nearest even: the nine weight matrices; the view and the
      feature inputs (f32 -> bf16); the mean action (f32 -> bf16, or f64 -> f32 -> bf16 when it arrives as float64,
      as on the rollout path); each layer's activation after bias and ReLU;
    * biases f32, added unrounded; ReLU unrounded; the Q values unrounded.

Accumulation here is float64 (the kernels': f32, the MFMA accumulator), so an activation is rounded f64 -> f32 -> bf16
where the kernels round their f32 sum: the difference the GPU tests' bounds leave room for.

Also the inputs and networks the bf16 tests share: the 256 real observation rows of tests/golden/battle64.npz and
networks initialised as tests/test_policy_gpu.py::_net (Glorot + 0.05 randn)."""
import os

import numpy as np

import qnet_ref

F, A = 34, 21


def bf16_round(x):
    """float32 array -> the float32 values of its round-to-nearest-even bf16 (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def _q(x):
    """Any float array -> float32 -> bf16, as float64."""
    return bf16_round(np.asarray(x).astype(np.float32)).astype(np.float64)


def forward(blob, offsets, F, A, use_mf, view, feat, prob=None):
    """view [n, 13, 13, 7], feat [n, F], prob [n, A] (float32, or float64 as the rollout's mean action) -> q [n, A]
    (float64) under the bf16 contract."""
    w1, b1, w2, b2, wd, bd, we, be, wp1, bp1, wp2, bp2, w2d, b2d, wo, bo, wq, bq = qnet_ref.blocks(
        np.asarray(blob, dtype=np.float32), offsets, F, A, use_mf)
    w1, w2, wd, we, wp1, wp2, w2d, wo, wq = (_q(w) for w in (w1, w2, wd, we, wp1, wp2, w2d, wo, wq))
    act = lambda x: _q(np.maximum(x, 0.0))               # bias added, ReLU, then the next product's operand
    v = _q(view)
    n = v.shape[0]
    cols = np.stack([v[:, ky:ky + 11, kx:kx + 11, :] for ky in range(3) for kx in range(3)], axis=3)
    c1 = act(cols.reshape(n, 11, 11, 63) @ w1[:63] + b1)
    cols = np.stack([c1[:, ky:ky + 9, kx:kx + 9, :] for ky in range(3) for kx in range(3)], axis=3)
    c2 = act(cols.reshape(n, 9, 9, 288) @ w2 + b2)
    h_obs = act(c2.reshape(n, 2592) @ wd + bd)
    f = np.zeros((n, we.shape[0]))
    f[:, :F] = _q(feat)
    h = [h_obs, act(f @ we + be)]
    if use_mf:
        p = np.zeros((n, wp1.shape[0]))
        p[:, :A] = _q(prob)
        h.append(act(act(p @ wp1 + bp1) @ wp2 + bp2))
    x = act(np.concatenate(h, axis=1) @ w2d + b2d)
    x = act(x @ wo + bo)
    return (x @ wq + bq)[:, :A]


def fixture_rows():
    """(view [256, 13, 13, 7], feat [256, 34], prob [256, 21]) float32: both groups' step-0 observations of env 0 of
    tests/golden/battle64.npz, and per group the mean action of 128 drawn actions (what the env would hand the net)."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "battle64.npz"))
    view = np.concatenate([z["e0_view_s0_g0"], z["e0_view_s0_g1"]]).astype(np.float32)
    feat = np.concatenate([z["e0_feat_s0_g0"], z["e0_feat_s0_g1"]]).astype(np.float32)
    rng = np.random.RandomState(17)
    prob = np.concatenate([np.tile(np.bincount(rng.randint(A, size=128), minlength=A) / 128.0, (128, 1))
                           for _ in range(2)]).astype(np.float32)
    return view, feat, prob


def net(use_mf, seed, F=F, A=A):
    """A torch QNet on the CPU, initialised as tests/test_policy_gpu.py::_net: Glorot + 0.05 randn on every parameter
    (F features, A actions: the Battle shape unless given)."""
    import torch
    from mfrl_amd.algo.nets import QNet
    torch.manual_seed(seed)
    m = QNet((13, 13, 7), (F,), A, use_mf)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return m


def packed(m, use_mf, F=F, A=A):
    """(blob float32 numpy, offsets) of net m."""
    from mfrl_amd.policy import blob_layout, pack_qnet
    layout = blob_layout(F, A, use_mf)
    return pack_qnet(m, F, A, use_mf, layout).cpu().numpy(), layout[1]


def quantisation(m, use_mf, view, feat, prob, F=F, A=A):
    """(q_exact, q_bf16, e_q, scale) of net m on the rows: the float64 unrounded forward, the bf16 reference, the
    reference's quantisation error max |q_bf16 - q_exact| and the Q scale max(1, max |q_exact|)."""
    blob, off = packed(m, use_mf, F, A)
    exact = qnet_ref.forward(blob.astype(np.float64), off, F, A, use_mf, view, feat, prob if use_mf else None)
    quant = forward(blob, off, F, A, use_mf, view, feat, prob if use_mf else None)
    return exact, quant, float(np.abs(quant - exact).max()), max(1.0, float(np.abs(exact).max()))


def clear_rows(exact, e_q):
    """Rows whose top-two exact Q values are more than 2 e_q apart (one action: every row)."""
    if exact.shape[1] < 2:
        return np.ones(len(exact), dtype=bool)
    s = np.sort(exact, axis=1)
    return (s[:, -1] - s[:, -2]) > 2.0 * e_q
