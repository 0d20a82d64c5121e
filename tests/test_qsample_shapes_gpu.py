"""The fused Boltzmann epilogue q_epilogue<kSample> (csrc/qsample.h) of k_qnet_head and k_qb16_head off the Battle
shape (F = 34, A = 21, the one shape tests/test_qsample_gpu.py runs it at): tests/test_qsample_gpu.py's
test_fused_epilogue_is_q_sample_on_the_forwards_q at the (F, A) pairs of tests/qsample_cases.py, on tests/net_shapes.py's
networks and 131 rows -- two full 64-agent tiles and a 3-row tail.

What they reach: A = 32, where lanes h = 2, 3 of tile t = 1 (actions 24 .. 31) carry real values in the gather
__shfl(qv[a >> 4][a & 3], 16 * ((a >> 2) & 3) + c); A = 2 and A = 20 (Ap = A, Ap != 21); F = 1, 37, 256 under the
sampling instantiation; and one action, which the forward accepts while mfx_q_sample refuses it.

The temperatures come from the references alone (qsample_cases.temperature; tests/test_qsample_cpu.py asserts that at
least 8 reference rows draw an action >= 24 at A = 32 and at least 8 do not draw the argmax), so the draw is neither
the greedy action nor confined to the lanes A = 21 fills."""
import copy

import numpy as np
import pytest
import torch

import net_shapes as ns
import qsample_cases as qc

pytestmark = pytest.mark.gpu


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def _hip(case):
    from mfrl_amd.policy import QNetHIP
    F, A, mf, prec = case
    r = ns.qnet_case(F, A, mf, prec == "bf16")
    hip = QNetHIP((13, 13, 7), (F,), A, mf, precision=prec).load(copy.deepcopy(r.net).cuda())
    return hip, (_dev(r.view), _dev(r.feat), _dev(r.prob) if mf else None)


@pytest.mark.parametrize("case", qc.CASES, ids=qc.case_id)
def test_fused_epilogue_is_q_sample_off_the_battle_shape(case):
    """forward(temperature=...): d_q is the greedy forward's bit for bit; (d_act, d_w) are mfx_q_sample's on that d_q
    with the same (T, seed, step) bit for bit; act() alone gives the same actions.  At least one draw is not the
    argmax, and at A = 32 at least one is an action >= 24."""
    from mfrl_amd import mf
    F, A, use_mf, prec = case
    T = qc.temperature(case)
    hip, args = _hip(case)
    q_g, a_g = hip.forward(*args)
    q_s, a_s, w_s = hip.forward(*args, temperature=T, seed=qc.SEED, step=qc.STEP, want_w=True)
    a_k, w_k = mf.q_sample(q_g, T, qc.SEED, qc.STEP, want_w=True)
    a_only = hip.act(*args, temperature=T, seed=qc.SEED, step=qc.STEP)
    torch.cuda.synchronize()
    assert q_s.shape == (ns.N, A) and w_s.shape == (ns.N, A) and a_s.shape == (ns.N,)
    assert torch.equal(q_s, q_g)
    assert torch.equal(a_s, a_k) and torch.equal(w_s, w_k)
    assert torch.equal(a_only, a_k)
    off, high = int((a_s != a_g).sum()), int((a_s >= qc.HIGH).sum())
    print("%s T %g: %d draws off the argmax, %d draws >= %d" % (qc.case_id(case), T, off, high, qc.HIGH))
    assert off >= 1
    assert 0 <= int(a_s.min()) and int(a_s.max()) < A
    if A > qc.HIGH:
        assert high >= 1


@pytest.mark.parametrize("case", qc.ONE_ACTION, ids=qc.case_id)
def test_one_action_under_sampling(case):
    """A = 1: mfx_q_sample refuses it, the fused forward takes it -- action 0 and weight 1.0f in every row, d_q the
    greedy forward's bit for bit."""
    F, A, use_mf, prec = case
    hip, args = _hip(case)
    q_g, a_g = hip.forward(*args)
    q_s, a_s, w_s = hip.forward(*args, temperature=0.5, seed=qc.SEED, step=qc.STEP, want_w=True)
    torch.cuda.synchronize()
    assert q_s.shape == (ns.N, 1) and torch.equal(q_s, q_g)
    assert not bool(a_s.any()) and not bool(a_g.any())
    assert w_s.cpu().numpy().tobytes() == np.ones((ns.N, 1), np.float32).tobytes()
