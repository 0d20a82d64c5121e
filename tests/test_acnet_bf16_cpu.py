"""The bf16 acting mode of the actor-critic network (ACNetHIP(precision="bf16"), csrc/acnet_bf16_kernels.hip) on the
CPU: this file pins the reference (tests/acnet_bf16_ref.py) and the conditions the GPU tests
(tests/test_acnet_bf16_gpu.py) rest on.

Inputs: the 256 real view / feature rows of tests/golden/battle64.npz at the Battle shape, and net_shapes' 131 rows off
it.  e_p is the reference's quantisation error, max |bf16 reference policy - float64 unrounded policy|; the GPU tests
bound the kernel by e_p (against the reference) and 2 e_p (against the exact forward), so e_p has to be a real
quantisation error -- neither zero (a reference that forgot to round) nor wild -- the reference has to depend on both
inputs by more than the bound, and most rows' draws have to be decided by more than the cumulative error."""
import os
import re
import subprocess

import numpy as np
import pytest

import acnet_bf16_ref as ref
import acnet_ref
import common
import net_shapes as ns
import qnet_bf16_ref as qb

BATTLE_CASES = [(use_mf, seed) for use_mf in (False, True) for seed in (11, 12)]
# (V, F, A, use_mf) off the Battle shape: the smallest and the largest shape, the f32 kernel's form boundary (F = 37),
# the Battle view with three actions
SHAPE_CASES = [(5, 1, 2, True), (4096, 256, 32, True), (1188, 37, 21, True), (1183, 34, 3, True)]
SEED, STEP = 7, 3                                         # the draw's counters in the clear-row conditions


def test_rounding_helper_rounds_ties_to_even():
    bits = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000], dtype=np.uint32)
    got = qb.bf16_round(bits.view(np.float32)).view(np.uint32)
    want = np.array([0x3F800000, 0x3F820000, 0x3F800000, 0x3F810000, 0xBF800000, 0xBF820000], dtype=np.uint32)
    assert np.array_equal(got, want)


def test_tenth_operand_is_one_rounding_after_the_f32_division():
    """The policy layer's operand is bf16(f32(d) / 0.1f): the f32 quotient, then one rounding.  It is neither
    bf16(d) / 0.1 rounded again (an activation rounded before the division) nor the float64 quotient rounded."""
    rng = np.random.RandomState(3)
    d = np.abs(rng.randn(20000)).astype(np.float32)
    got = ref.tenth_operand(d)
    want = qb.bf16_round(d / np.float32(0.1)).astype(np.float64)
    assert np.array_equal(got, want)
    twice = qb.bf16_round(qb.bf16_round(d) / np.float32(0.1)).astype(np.float64)
    assert 0.05 < np.mean(twice != got) < 0.95            # (the test can tell the two apart)
    # the f32 quotient is the IEEE one: equal to the float64 quotient by f32(0.1) rounded to f32
    q64 = (d.astype(np.float64) / np.float64(np.float32(0.1))).astype(np.float32)
    assert np.array_equal(d / np.float32(0.1), q64)
    assert ref.tenth_operand(np.array([0.0]))[0] == 0.0


@pytest.fixture(scope="module")
def battle():
    rows = ref.fixture_rows()
    assert rows[0].shape == (256, 1183) and rows[1].shape == (256, 34)
    out = {}
    for use_mf, seed in BATTLE_CASES:
        m = ref.net(use_mf, seed)
        blob, off = ref.packed(m, use_mf)
        out[(use_mf, seed)] = (blob, off, rows) + ref.quantisation_blob(blob, off, ref.V, ref.F, ref.A, use_mf, *rows)
    return out


def _shape(case):
    r = ns.acnet_case(*case)
    V, F, A, mf = case
    return (r.blob, r.layout[1], (r.view, r.feat)) + ref.quantisation_blob(r.blob, r.layout[1], V, F, A, mf, r.view, r.feat)


@pytest.mark.parametrize("use_mf,seed", BATTLE_CASES)
def test_quantisation_error_is_a_quantisation_error(battle, use_mf, seed):
    e_p = battle[(use_mf, seed)][5]
    print("use_mf %d seed %d: e_p %.3e" % (use_mf, seed, e_p))
    assert 1e-3 < e_p < 5e-2, e_p


def _conditions(blob, off, rows, exact, quant, e_p, V, F, A, use_mf):
    u = acnet_ref.uniforms(SEED, STEP, 0, np.arange(len(exact)))
    clear, e_c = ref.clear_rows(exact, quant, u)
    rows_i = np.arange(len(exact))
    same = acnet_ref.draw(quant.astype(np.float32), SEED, STEP, 0, rows_i) == \
        acnet_ref.draw(exact.astype(np.float32), SEED, STEP, 0, rows_i)
    moved = {}
    for name, (v, f) in (("view", (0 * rows[0], rows[1])), ("feat", (rows[0], 0 * rows[1]))):
        z = ref.forward(blob, off, V, F, A, use_mf, v, f)
        moved[name] = float(np.median(np.abs(z - quant).max(1))) / e_p
    print("V %d F %d A %d mf %d: e_p %.3e e_c %.3e clear %.3f same draw %.3f, zeroed view %.1f e_p, features %.1f e_p"
          % (V, F, A, use_mf, e_p, e_c, clear.mean(), same.mean(), moved["view"], moved["feat"]))
    return clear, same, moved


@pytest.mark.parametrize("use_mf,seed", BATTLE_CASES)
def test_battle_clear_rows_and_sensitivity(battle, use_mf, seed):
    clear, same, moved = _conditions(*battle[(use_mf, seed)], ref.V, ref.F, ref.A, use_mf)
    assert clear.mean() >= 0.5, clear.mean()
    assert same[clear].all()                              # the reference itself keeps the exact draw on clear rows
    assert moved["view"] > 2.0 and moved["feat"] > 2.0, moved


@pytest.mark.parametrize("case", SHAPE_CASES, ids=ns.case_id)
def test_shape_cases_clear_rows_and_sensitivity(case):
    blob, off, rows, exact, quant, e_p = _shape(case)
    assert 1e-4 < e_p < 5e-2, e_p
    clear, same, moved = _conditions(blob, off, rows, exact, quant, e_p, *case)
    assert clear.mean() >= 0.5, clear.mean()
    assert same[clear].all()
    assert moved["view"] > 2.0 and moved["feat"] > 2.0, moved


def _usage():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(common.PKG, "csrc", "acnet_bf16_kernels.hip")
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
    for want in ("k_acb16", "k_acb16_image"):
        assert any(want in k for k in usage), (want, sorted(usage))
    for k, u in usage.items():
        assert u.get("VGPRs Spill", 0) == 0, (k, u)
        assert u.get("SGPRs Spill", 0) == 0, (k, u)
        assert u.get("ScratchSize", 0) == 0, (k, u)


def test_unknown_precision_is_refused_before_the_gpu():
    from mfrl_amd.policy import ACNetHIP
    with pytest.raises(ValueError):
        ACNetHIP((13, 13, 7), (34,), 21, use_mf=True, precision="fp8")
    assert ACNetHIP.__init__.__defaults__[-1] == "f32"


def test_the_abi_declares_the_mode():
    import ctypes
    header = open(os.path.join(common.REPO, "include", "magent_amd.h")).read()
    dll = ctypes.CDLL(common.HIP_LIB)
    for fn in ("mfx_acnet_set_precision", "mfx_acnet_precision"):
        assert re.search(r"\bint %s\(" % fn, header), fn
        assert hasattr(dll, fn), fn
