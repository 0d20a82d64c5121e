"""The training step's float64 restatement (tests/qtrain_ref.py) against torch autograd on the CPU, the blob
pack / unpack round trip, and the register budget of csrc/qtrain_kernels.hip (hipcc cross-compile).  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import common
import qnet_bf16_ref as qb
import qtrain_ref as qr

F, A = qr.F, qr.A
GAMMA = 0.95


def _layout(use_mf):
    from mfrl_amd.policy import blob_layout
    return blob_layout(F, A, use_mf)


@pytest.mark.parametrize("B", [64, 20])
@pytest.mark.parametrize("use_mf", [False, True])
def test_restatement_matches_autograd_f64(use_mf, B):
    """Every tensor's gradient to 1e-10 relative (max |g - g_torch| / max |g_torch|), the loss and mean q[a] too;
    padding gradients exactly zero."""
    seed = 11
    n, off = _layout(use_mf)
    ev, tg = qr.nets(use_mf, seed)
    eb, tb = (qb.packed(m, use_mf)[0].astype(np.float64) for m in (ev, tg))
    ring, idx = qr.ring(seed), qr.index_list(seed, B)
    assert ring["mask"][idx].sum() >= 15
    y, _ = qr.targets(eb, tb, off, F, A, use_mf, ring, qr.N_RING, idx, GAMMA)
    g, loss, qa = qr.gradient(eb, tb, off, F, A, use_mf, ring, qr.N_RING, idx, GAMMA)
    named, t_loss, t_qa = qr.torch_gradient(ev, use_mf, ring, idx, y, torch.float64)
    ref = qr.pack64(named, F, A, use_mf, off, n)
    for k, (err, scale) in enumerate(qr.block_errors(g, ref, off, n)):
        if not use_mf and 8 <= k < 12:
            assert err == 0.0 and scale == 0.0, k
            continue
        assert scale > 0 and err <= 1e-10, (k, err, scale)
    assert abs(loss - t_loss) <= 1e-10 * max(1.0, abs(t_loss))
    assert abs(qa - t_qa) <= 1e-10 * max(1.0, abs(t_qa))
    pad = qr.padding_mask(off, F, A, use_mf, n)
    assert pad.any() and np.all(g[pad] == 0.0)


def test_restatement_adam_matches_torch_f64():
    """Two Adam steps + soft updates of the restatement against torch.optim.Adam in float64."""
    rng = np.random.RandomState(3)
    p0, tgt0 = rng.randn(50), rng.randn(50)
    grads = [rng.randn(50) * 1e-2 for _ in range(2)]
    p = torch.tensor(p0, requires_grad=True)
    tgt = torch.tensor(tgt0)
    opt = torch.optim.Adam([p], lr=1e-4)
    st = (p0, tgt0, np.zeros(50), np.zeros(50))
    for t, g in enumerate(grads, 1):
        p.grad = torch.tensor(g)
        opt.step()
        with torch.no_grad():
            tgt.mul_(1.0 - 0.005).add_(0.005 * p)
        st = qr.adam(*st, g, t)
        np.testing.assert_allclose(st[0], p.detach().numpy(), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(st[1], tgt.numpy(), rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("use_mf", [False, True])
def test_unpack_is_the_inverse_of_pack(use_mf):
    from mfrl_amd.policy import pack_qnet, unpack_qnet
    layout = _layout(use_mf)
    src = qb.net(use_mf, 11)
    dst = qb.net(use_mf, 12)
    blob = pack_qnet(src, F, A, use_mf, layout)
    assert unpack_qnet(blob, dst) is dst
    for (k, a), (_, b) in zip(src.named_parameters(), dst.named_parameters()):
        assert a.detach().numpy().tobytes() == b.detach().numpy().tobytes(), k
    assert pack_qnet(dst, F, A, use_mf, layout).numpy().tobytes() == blob.numpy().tobytes()


def test_argmax_gap_precondition():
    """Every ring row's top-two eval-Q gap exceeds 2e-5 for the four nets the GPU tests use (so the target's argmax
    cannot legitimately differ between f32 and f64), and every block of the reference gradient is well above zero."""
    view, feat, prob = qb.fixture_rows()
    for use_mf in (False, True):
        _, off = _layout(use_mf)
        for seed in (11, 12):
            blob = qb.packed(qb.net(use_mf, seed), use_mf)[0].astype(np.float64)
            q = np.sort(qr.qnet_ref.forward(blob, off, F, A, use_mf, view[:qr.N_RING], feat[:qr.N_RING],
                                            prob[:qr.N_RING] if use_mf else None), axis=1)
            assert (q[:, -1] - q[:, -2]).min() > 2e-5, (use_mf, seed)


def test_new_kernels_use_no_scratch():
    """ScratchSize 0 and no VGPR spills for every kernel of csrc/qtrain_kernels.hip."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(common.PKG, "csrc", "qtrain_kernels.hip")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                          "-mllvm", "-amdgpu-atomic-optimizer-strategy=None", "--cuda-device-only", "-c", "-x",
                          "hip", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    usage, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            usage[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\])?: (\d+)", line)
        if m and cur:
            usage[cur][m.group(1).strip()] = int(m.group(2))
    kernels = [k for k in usage if "k_qt_" in k]
    assert len(kernels) >= 13, sorted(usage)
    for k in kernels:
        assert usage[k].get("ScratchSize", -1) == 0, (k, usage[k])
        assert usage[k].get("VGPRs Spill", 0) == 0, (k, usage[k])
