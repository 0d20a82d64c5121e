"""Test infrastructure: the numerical contract of the actor-critic network's bf16 acting forward
(csrc/acnet_bf16_kernels.hip, ACNetHIP(precision="bf16")) restated in float64 numpy on the packed weight blob, built
from acnet_ref.blocks and qnet_bf16_ref.bf16_round.

    * operands of every matrix product rounded to bf16, nearest even: the four weight matrices (view, feature, dense,
      policy); the view and the feature inputs (f32 -> bf16); h_view and h_emb after bias and ReLU; relu(d) / 0.1 --
      the f32 division the f32 kernel does (correctly rounded), then one rounding to bf16;
    * biases f32, added unrounded; ReLU, softmax and the clip unrounded.  The value heads are not part of the mode.

Accumulation here is float64 (the kernel's: f32, the MFMA accumulator), so an activation is rounded f64 -> f32 -> bf16
where the kernel rounds its f32 sum: the difference the GPU tests' bounds leave room for.

Also the networks and rows the bf16 tests share: the 256 real observation rows of tests/golden/battle64.npz
(qnet_bf16_ref.fixture_rows) and ACNets initialised as qnet_bf16_ref.net does (default init + 0.05 randn)."""
import numpy as np

import acnet_ref
import qnet_bf16_ref as qb

V, F, A = 1183, 34, 21
_q = qb._q


def tenth_operand(d):
    """relu'd dense activations (any float array) -> the policy layer's operand: f32, / 0.1 in f32 (IEEE, as
    div_tenth), one rounding to bf16; float64."""
    x = np.asarray(d).astype(np.float32) / np.float32(0.1)
    return qb.bf16_round(x).astype(np.float64)


def forward(blob, offsets, V, F, A, use_mf, view, feat):
    """view [n, ...] (V floats), feat [n, F] float32 -> policy [n, A] (float64) under the bf16 contract."""
    wv, bv, we, be, wd0, wd1, bd, wp, bp = acnet_ref.blocks(np.asarray(blob, dtype=np.float32), offsets, V, F, A,
                                                            use_mf)[:9]
    wv, we, wd, wp = _q(wv), _q(we), _q(np.concatenate([wd0, wd1], axis=1)), _q(wp)
    act = lambda x: _q(np.maximum(x, 0.0))               # bias added, ReLU, then the next product's operand
    x = _q(np.asarray(view, dtype=np.float32).reshape(len(view), -1))
    n = x.shape[0]
    xv = np.zeros((n, wv.shape[0]))
    xv[:, :V] = x
    f = np.zeros((n, we.shape[0]))
    f[:, :F] = _q(feat)
    concat = np.concatenate([act(xv @ wv + bv), act(f @ we + be)], axis=1)
    d = np.maximum(concat @ wd + bd, 0.0)
    logits = (tenth_operand(d) @ wp + bp)[:, :A]
    e = np.exp(logits - logits.max(1, keepdims=True))
    return np.clip(e / e.sum(1, keepdims=True), 1e-10, 1 - 1e-10)


def fixture_rows():
    """(view [256, 1183], feat [256, 34]) float32: qnet_bf16_ref.fixture_rows, the views flattened."""
    view, feat, _ = qb.fixture_rows()
    return view.reshape(len(view), -1), feat


def net(use_mf, seed, V=V, F=F, A=A):
    """A torch ACNet on the CPU, initialised as qnet_bf16_ref.net: + 0.05 randn on every parameter."""
    import torch
    from mfrl_amd.algo.nets import ACNet
    torch.manual_seed(seed)
    m = ACNet((V,), (F,), A, use_mf=bool(use_mf))
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return m


def packed(m, use_mf, V=V, F=F, A=A):
    """(blob float32 numpy, offsets) of net m."""
    from mfrl_amd.policy import acnet_layout, pack_acnet
    layout = acnet_layout(V, F, A, use_mf)
    return pack_acnet(m, V, F, A, use_mf, layout).cpu().numpy(), layout[1]


def quantisation_blob(blob, offsets, V, F, A, use_mf, view, feat):
    """(exact, quant, e_p): the float64 unrounded policy (acnet_ref.forward), the bf16 reference and the
    reference's quantisation error max |quant - exact|."""
    exact = acnet_ref.forward(np.asarray(blob, dtype=np.float64), offsets, V, F, A, use_mf, view, feat,
                              np.zeros((len(view), A)))[0]
    quant = forward(blob, offsets, V, F, A, use_mf, view, feat)
    return exact, quant, float(np.abs(quant - exact).max())


def quantisation(m, use_mf, rows, V=V, F=F, A=A):
    """quantisation_blob of net m on rows = (view, feat)."""
    blob, off = packed(m, use_mf, V, F, A)
    return quantisation_blob(blob, off, V, F, A, use_mf, rows[0], rows[1])


def cumulative(policy):
    """The normalised cumulative policy [n, A] (float64): the draw picks the first action whose entry exceeds u."""
    c = np.cumsum(np.asarray(policy, dtype=np.float64), axis=1)
    return c / c[:, -1:]


def clear_rows(exact, quant, u):
    """Rows whose uniform u lies more than 2 e_c from every boundary of the exact normalised cumulative policy, e_c =
    the reference's own maximum cumulative error max |cumulative(quant) - cumulative(exact)|: a policy within that
    of the exact one draws the exact policy's action there.  -> (mask [n], e_c)."""
    ce = cumulative(exact)
    e_c = float(np.abs(cumulative(quant) - ce).max())
    gap = np.abs(ce[:, :-1] - np.asarray(u, dtype=np.float64)[:, None]).min(1)        # (the last boundary is 1 > u)
    return gap > 2.0 * e_c, e_c
