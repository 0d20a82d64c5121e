"""The four network paths off the Battle shape, on the CPU (tests/net_shapes.py holds the shapes and inputs that
tests/test_net_shapes_gpu.py runs on the kernels):

* the packed blobs (pack_acnet, pack_qnet) restated in float64 (tests/acnet_ref.py, tests/qnet_ref.py) are the torch
  modules at every shape -- tests/test_policy_cpu.py's two tests, parametrised over view, feature and action widths;
* unpack_qnet inverts pack_qnet at padded widths;
* every blob_size / create refuses the first value outside each documented range (include/magent_amd.h), before any
  device call;
* the preconditions the GPU tests rest on hold for the float64 references: the sensitivity precondition of every
  forward case, and the argmax gap and gradient scale of the training cases."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import net_shapes as ns
import qnet_bf16_ref as qb
import qtrain_ref as qr

GAMMA = 0.95


# ------------------------------------------------------------------------------------------------- blob = module
@pytest.mark.parametrize("case", ns.ACNET_CASES, ids=ns.case_id)
def test_packed_acnet_blob_is_the_torch_network(case):
    """The float32 blob in float64 against the module cast to float64 -- the same weights, so they agree to rounding
    of the float64 sums (1e-9 leaves five orders; a misplaced row or block gives 1e-2)."""
    V, F, A, mf = case
    r = ns.acnet_case(*case)
    t = lambda x: torch.tensor(x, dtype=torch.float64)
    with torch.no_grad():
        pol, val = copy.deepcopy(r.net).double()(t(r.view), t(r.feat), t(r.prob) if mf else None)
    assert r.blob.dtype == np.float32 and r.policy.shape == (ns.N, A) and r.value.shape == (ns.N,)
    assert np.abs(r.policy - pol.numpy()).max() < 1e-9
    assert np.abs(r.value - val.numpy()).max() < 1e-9 * r.vscale
    assert float(r.policy.max(1).mean()) < 0.999            # (a policy that is not one-hot everywhere)


@pytest.mark.parametrize("case", ns.QNET_CASES, ids=ns.case_id)
def test_packed_qnet_blob_is_the_torch_network(case):
    F, A, mf = case
    r = ns.qnet_case(*case)
    t = lambda x: torch.tensor(x, dtype=torch.float64)
    with torch.no_grad():
        want = copy.deepcopy(r.net).double()(t(r.view), t(r.feat), t(r.prob) if mf else None).numpy()
    assert r.q.shape == (ns.N, A)
    assert np.abs(r.q - want).max() < 1e-9 * r.scale
    # the greedy-action rule of the GPU test: at least 99 % of rows are decided by more than the bound
    assert r.clear(ns.TOL * r.scale).mean() >= 0.99


@pytest.mark.parametrize("F,A", [(37, 32), (1, 2)])
@pytest.mark.parametrize("use_mf", [False, True])
def test_unpack_is_the_inverse_of_pack(use_mf, F, A):
    from mfrl_amd.policy import blob_layout, pack_qnet, unpack_qnet
    layout = blob_layout(F, A, use_mf)
    src, dst = qb.net(use_mf, 11, F, A), qb.net(use_mf, 12, F, A)
    blob = pack_qnet(src, F, A, use_mf, layout)
    assert unpack_qnet(blob, dst) is dst
    for (k, a), (_, b) in zip(src.named_parameters(), dst.named_parameters()):
        assert a.detach().numpy().tobytes() == b.detach().numpy().tobytes(), k
    assert pack_qnet(dst, F, A, use_mf, layout).numpy().tobytes() == blob.numpy().tobytes()
    pad = qr.padding_mask(layout[1], F, A, use_mf, layout[0])
    assert pad.any() and not blob.numpy()[pad].any()


# ------------------------------------------------------------------------------------------------- ranges
def _lib():
    from mfrl_amd import lib
    L = lib()
    for fn in ("mfx_acnet_blob_size", "mfx_acnet_create", "mfx_qnet_blob_size", "mfx_qnet_create", "mfx_qtrain_create"):
        getattr(L, fn).restype = ctypes.c_int
    return L


ACNET_BAD = [(0, 34, 21), (4097, 34, 21), (1183, 0, 21), (1183, 257, 21), (1183, 34, 1), (1183, 34, 33)]
QNET_BAD = [(0, 21), (257, 21), (34, 0), (34, 33)]


@pytest.mark.parametrize("use_mf", [0, 1])
def test_acnet_refuses_shapes_outside_the_documented_ranges(use_mf):
    """View 1 .. 4096 floats, feature 1 .. 256, n_action 2 .. 32: the first value outside each is refused by
    mfx_acnet_blob_size and mfx_acnet_create (no handle, a message naming the ranges), the last inside is laid out."""
    L = _lib()
    n, off = ctypes.c_size_t(), (ctypes.c_size_t * 19)()
    for V, F, A in ACNET_BAD:
        assert L.mfx_acnet_blob_size(V, F, A, use_mf, ctypes.byref(n), off) != 0, (V, F, A)
        msg = L.mfx_last_error().decode()
        assert "4096" in msg and "256" in msg and "32" in msg, msg
        h = ctypes.c_void_p()
        assert L.mfx_acnet_create(V, F, A, use_mf, ctypes.byref(h)) != 0 and not h.value, (V, F, A)
    for V, F, A in ((1, 1, 2), (4096, 256, 32)):
        assert L.mfx_acnet_blob_size(V, F, A, use_mf, ctypes.byref(n), off) == 0 and n.value > 0


@pytest.mark.parametrize("use_mf", [0, 1])
def test_qnet_and_qtrain_refuse_shapes_outside_the_documented_ranges(use_mf):
    """Feature 1 .. 256, n_action 1 .. 32, the 13 x 13 x 7 view only: mfx_qnet_blob_size, mfx_qnet_create and
    mfx_qtrain_create, and the Python front ends."""
    from mfrl_amd import qtrain
    L = _lib()
    n, off = ctypes.c_size_t(), (ctypes.c_size_t * 18)()
    for F, A in QNET_BAD:
        assert L.mfx_qnet_blob_size(F, A, use_mf, ctypes.byref(n), off) != 0, (F, A)
        msg = L.mfx_last_error().decode()
        assert "256" in msg and "32" in msg, msg
        for create in (lambda h: L.mfx_qnet_create(13, 13, 7, F, A, use_mf, ctypes.byref(h)),
                       lambda h: L.mfx_qtrain_create(F, A, use_mf, ctypes.byref(h))):
            h = ctypes.c_void_p()
            assert create(h) != 0 and not h.value, (F, A)
        assert not qtrain.supported((13, 13, 7), (F,), A)
        with pytest.raises(ValueError):
            qtrain.QTrainHIP((13, 13, 7), (F,), A, bool(use_mf))
    for F, A in ((1, 1), (256, 32)):
        assert L.mfx_qnet_blob_size(F, A, use_mf, ctypes.byref(n), off) == 0 and n.value > 0
    h = ctypes.c_void_p()
    assert L.mfx_qnet_create(9, 9, 7, 34, 21, use_mf, ctypes.byref(h)) != 0 and not h.value
    assert "13 x 13 x 7" in L.mfx_last_error().decode()
    assert not qtrain.supported((9, 9, 7), (34,), 21)
    with pytest.raises(ValueError):
        qtrain.QTrainHIP((9, 9, 7), (34,), 21, bool(use_mf))


# ------------------------------------------------------------------------------------------------- preconditions
@pytest.mark.parametrize("case", ns.ACNET_CASES, ids=ns.case_id)
def test_acnet_sensitivity_precondition(case):
    s = ns.acnet_case(*case).sensitivity()
    assert len(s) == (5 if case[3] else 4)
    for k, x in s.items():
        assert x >= ns.SENSITIVITY, (k, x)


@pytest.mark.parametrize("case", ns.QNET_CASES, ids=ns.case_id)
def test_qnet_sensitivity_precondition(case):
    r = ns.qnet_case(*case)
    s = r.sensitivity()
    assert len(s) == (3 if case[2] else 2)
    for k, x in s.items():
        assert x >= ns.SENSITIVITY * ns.TOL * r.scale, (k, x, r.scale)


@pytest.mark.parametrize("case", ns.BF16_CASES, ids=ns.case_id)
def test_bf16_preconditions(case):
    """e_q is a real quantisation error (tests/test_policy_bf16_cpu.py's window), most rows are decided by more than
    2 e_q, the float64 forward meets the f32 sensitivity precondition on these inputs too, and zeroing an operand moves
    the bf16 reference by more than 2 e_q on the median row (net_shapes.QRef.sensitivity_bf16: why 2)."""
    r = ns.qnet_case(*case, True)
    assert 1e-4 * r.scale < r.e_q < 5e-2 * r.scale, (r.e_q, r.scale)
    clear = qb.clear_rows(r.q, r.e_q)
    assert np.array_equal(np.argmax(r.quant, 1)[clear], np.argmax(r.q, 1)[clear])
    assert clear.mean() >= 0.75, clear.mean()
    for k, x in r.sensitivity().items():
        assert x >= ns.SENSITIVITY * ns.TOL * r.scale, (k, x, r.scale)
    for k, x in r.sensitivity_bf16().items():
        assert x > 2.0 * r.e_q, (k, x, r.e_q)


@pytest.mark.parametrize("case", ns.QTRAIN_CASES, ids=ns.case_id)
def test_qtrain_preconditions(case):
    """The conditions tests/test_qtrain_gpu.py::test_gradient_accuracy asserts on the float64 restatement, at the other
    widths: every ring row's top-two eval-Q gap above 2e-5, every non-empty block's max |g64| at least 1e-3, the index
    list's wrap, repeat and mask count; and the restatement is torch's float64 autograd there too (1e-10)."""
    from mfrl_amd.policy import blob_layout
    F, A, mf, seed = case
    n, off = blob_layout(F, A, mf)
    ev, tg = qr.nets(mf, seed, F, A)
    eb, tb = (qb.packed(m, mf, F, A)[0].astype(np.float64) for m in (ev, tg))
    ring, idx = qr.ring(seed, F, A), qr.index_list(seed, ns.QTRAIN_B)
    N = qr.N_RING
    assert ring["feat"].shape == (qr.RING_ROWS, F) and ring["prob"].shape == (qr.RING_ROWS, A) and ring["act"].max() < A
    assert (N - 1) in idx and len(set(idx.tolist())) < ns.QTRAIN_B and ring["mask"][idx].sum() >= 15
    q = np.sort(qr.qnet_ref.forward(eb, off, F, A, mf, ring["obs"][:N], ring["feat"][:N], ring["prob"][:N] if mf else None), 1)
    assert (q[:, -1] - q[:, -2]).min() > 2e-5
    y, _ = qr.targets(eb, tb, off, F, A, mf, ring, N, idx, GAMMA)
    g, loss, qa = qr.gradient(eb, tb, off, F, A, mf, ring, N, idx, GAMMA, y=y)
    named, t_loss, t_qa = qr.torch_gradient(ev, mf, ring, idx, y, torch.float64)
    ref = qr.pack64(named, F, A, mf, off, n)
    for k, (err, scale) in enumerate(qr.block_errors(g, ref, off, n)):
        if not mf and 8 <= k < 12:
            assert err == 0.0 and scale == 0.0, k
            continue
        assert scale >= 1e-3 and err <= 1e-10, (k, err, scale)
    assert abs(loss - t_loss) <= 1e-10 * max(1.0, abs(t_loss)) and abs(qa - t_qa) <= 1e-10 * max(1.0, abs(t_qa))
    pad = qr.padding_mask(off, F, A, mf, n)
    assert pad.any() and np.all(g[pad] == 0.0)


@pytest.mark.parametrize("T", ns.QTRAIN_SOFT_T)
@pytest.mark.parametrize("case", ns.QTRAIN_CASES, ids=ns.case_id)
def test_qtrain_boltzmann_preconditions(case, T):
    """The case seeds were chosen for the max target.  Under the Boltzmann target (set_target("boltzmann", T)) they
    must meet that rule's own preconditions: qtarget_ref.check(A, T) passes, no next row of the index list has a
    non-finite Q value in either net, the float64 target is finite, and every non-empty block's max |g64| under that
    target is at least 1e-3 (the scale tests/test_net_shapes_gpu.py asserts before it reads a ratio)."""
    from mfrl_amd.policy import blob_layout
    F, A, mf, seed = case
    n, off = blob_layout(F, A, mf)
    ev, tg = qr.nets(mf, seed, F, A)
    eb, tb = (qb.packed(m, mf, F, A)[0].astype(np.float64) for m in (ev, tg))
    ring, idx = qr.ring(seed, F, A), qr.index_list(seed, ns.QTRAIN_B)
    N = qr.N_RING
    y, q_e, q_t = ns.qtrain_soft_target64(eb, tb, off, F, A, mf, ring, N, idx, GAMMA, T)
    assert np.isfinite(q_e).all() and np.isfinite(q_t).all() and np.isfinite(y).all()
    y_max, _ = qr.targets(eb, tb, off, F, A, mf, ring, N, idx, GAMMA)
    # another target than the max rule's, by more than f32 resolves ((1, 2) at T = 0.1, gap 0.49: 1.4e-4 at most)
    assert np.abs(y - y_max).max() > 1e-5
    g, loss, qa = qr.gradient(eb, tb, off, F, A, mf, ring, N, idx, GAMMA, y=y)
    for k, (err, scale) in enumerate(qr.block_errors(g, g, off, n)):
        if not mf and 8 <= k < 12:
            assert scale == 0.0, k
            continue
        assert scale >= 1e-3, (k, scale)
