"""The bf16 acting mode of the Q network (QNetHIP(precision="bf16"), csrc/qnet_bf16_kernels.hip) on the CPU: this file
pins the reference (tests/qnet_bf16_ref.py) and the conditions the GPU tests (tests/test_policy_bf16_gpu.py) rest on.

Inputs: the 256 real view / feature rows of tests/golden/battle64.npz.  Networks: Glorot + 0.05 randn as
tests/test_policy_gpu.py::_net, seeds 11, 12, 5, with and without mean field.  e_q is the reference's quantisation
error, max |bf16 reference - float64 unrounded forward|; the GPU tests bound the kernels by e_q (against the
reference) and 2 e_q (against the exact forward), so e_q has to be a real quantisation error -- neither zero (a
reference that forgot to round) nor wild -- and most rows have to be decided by more than it."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import common
import qnet_bf16_ref as ref

CASES = [(use_mf, seed) for use_mf in (False, True) for seed in (11, 12, 5)]


def test_rounding_helper_is_torch_bfloat16():
    rng = np.random.RandomState(0)
    x = np.concatenate([
        (rng.randn(4000) * np.exp(rng.uniform(-20, 20, 4000))).astype(np.float32),
        # exact ties (the 16 dropped bits are 0x8000) on even and odd kept mantissas, both signs, and their neighbours
        (rng.randint(0x3000, 0x5000, 2000).astype(np.uint32) << np.uint32(16) | np.uint32(0x8000)).view(np.float32),
        -(rng.randint(0x3000, 0x5000, 500).astype(np.uint32) << np.uint32(16) | np.uint32(0x8000)).view(np.float32),
        (rng.randint(0x3000, 0x5000, 500).astype(np.uint32) << np.uint32(16) | np.uint32(0x7FFF)).view(np.float32),
        (rng.randint(0x3000, 0x5000, 500).astype(np.uint32) << np.uint32(16) | np.uint32(0x8001)).view(np.float32),
        np.array([0.0, -0.0, 1.0, -1.0, 3.3895314e38, 1e-40], dtype=np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    got = ref.bf16_round(x)
    assert got.dtype == np.float32
    assert got.tobytes() == want.tobytes()
    ties = (x.view(np.uint32) & np.uint32(0xFFFF)) == np.uint32(0x8000)
    assert ties.sum() >= 2500 and np.all((got[ties].view(np.uint32) >> np.uint32(16)) & np.uint32(1) == 0)


@pytest.fixture(scope="module")
def quantised():
    view, feat, prob = ref.fixture_rows()
    assert view.shape == (256, 13, 13, 7) and feat.shape == (256, 34) and prob.shape == (256, 21)
    return {(use_mf, seed): ref.quantisation(ref.net(use_mf, seed), use_mf, view, feat, prob) for use_mf, seed in CASES}


@pytest.mark.parametrize("use_mf,seed", CASES)
def test_quantisation_error_is_a_quantisation_error(quantised, use_mf, seed):
    exact, quant, e_q, scale = quantised[(use_mf, seed)]
    print("use_mf %d seed %d: e_q %.3e, Q scale %.3f, e_q / scale %.3e" % (use_mf, seed, e_q, scale, e_q / scale))
    assert 1e-4 * scale < e_q < 5e-2 * scale, (e_q, scale)


@pytest.mark.parametrize("use_mf,seed", CASES)
def test_clear_rows_keep_their_action_and_are_most_rows(quantised, use_mf, seed):
    exact, quant, e_q, scale = quantised[(use_mf, seed)]
    clear = ref.clear_rows(exact, e_q)
    print("use_mf %d seed %d: clear share %.3f" % (use_mf, seed, clear.mean()))
    assert np.array_equal(np.argmax(quant, 1)[clear], np.argmax(exact, 1)[clear])
    assert clear.mean() >= 0.75, clear.mean()


def test_float64_mean_action_is_rounded_through_float32():
    """The rollout path's mean action is float64: the reference rounds it f64 -> f32 -> bf16, which differs from one
    rounding f64 -> bf16 exactly when the f32 rounding lands on a bf16 tie."""
    x = np.array([1.0 + 2.0 ** -8 + 2.0 ** -30], dtype=np.float64)      # above the tie 1 + 2^-8; f32 drops the 2^-30
    assert ref._q(x)[0] == 1.0                                          # tie -> even, as the kernels' two roundings
    assert ref._q(np.float32(1.0 + 2.0 ** -8 + 2.0 ** -20))[0] == 1.0 + 2.0 ** -7


def _usage():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(common.PKG, "csrc", "qnet_bf16_kernels.hip")
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
    return usage


def test_bf16_kernels_do_not_spill():
    usage = _usage()
    for want in ("k_qb16_conv", "k_qb16_head", "k_qb16_image"):
        assert any(want in k for k in usage), (want, sorted(usage))
    for k, u in usage.items():
        assert u.get("VGPRs Spill", 0) == 0, (k, u)
        assert u.get("ScratchSize", 0) == 0, (k, u)


def test_unknown_precision_is_refused_before_the_gpu():
    from mfrl_amd.policy import QNetHIP
    with pytest.raises(ValueError):
        QNetHIP((13, 13, 7), (34,), 21, use_mf=False, precision="fp8")
