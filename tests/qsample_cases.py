"""Test infrastructure: the cases of tests/test_qsample_shapes_gpu.py -- the fused Boltzmann epilogue q_epilogue
(csrc/qsample.h) of k_qnet_head and k_qb16_head off A = 21, F = 34 -- and the property that makes them decisive,
computed from tests/net_shapes.py's references alone (tests/test_qsample_cpu.py asserts it without a GPU).

The epilogue gathers an agent's Q row from four lanes, action a from lane 16 ((a >> 2) & 3) + c; at A = 21 the lanes
that hold actions 24 .. 31 never carried a real value.  A case is decisive when the draw takes such an action (A = 32)
and is not the argmax everywhere (every case); both follow from the temperature, which is raised per case, from 0.05 in
the steps of TEMPERATURES, until at least MIN_ROWS of the 131 reference rows show each (the device's Q values differ
from the reference's by rounding, which moves the draw of a few rows at most: the GPU test then asserts one row)."""
import functools

import numpy as np

import net_shapes as ns
import qsample_ref as qs

FA = [(256, 32), (37, 2), (1, 21), (34, 20), (34, 32)]
assert all(fa in ns._QNET_FA for fa in FA)
CASES = [(F, A, mf, prec) for F, A in FA for mf in (False, True) for prec in ("f32", "bf16")
         if prec == "f32" or (F, A, mf) in ns.BF16_CASES]
ONE_ACTION = [(34, 1, mf, prec) for mf in (False, True) for prec in ("f32", "bf16")]
SEED, STEP = 991, 131
TEMPERATURES = (0.05, 0.1, 0.2, 0.5, 1.0, 2.0, 5.0)
MIN_ROWS = 8
HIGH = 24                                     # the first action of lanes h = 2, 3 of tile t = 1


def case_id(case):
    return "%d-%d-%s-%s" % (case[0], case[1], "mf" if case[2] else "dqn", case[3])


def reference_q(case):
    """The float32 Q rows the restatement draws from: the float64 forward (f32), the quantised reference (bf16)."""
    F, A, mf, prec = case
    r = ns.qnet_case(F, A, mf, prec == "bf16")
    return (r.quant if prec == "bf16" else r.q).astype(np.float32)


def decisive(case, T):
    """(rows whose reference draw is not the argmax, rows whose draw is >= HIGH) at temperature T."""
    q = reference_q(case)
    act = qs.sample(q, T, SEED, STEP, 0, np.arange(len(q)))
    return int((act != qs.greedy(q)).sum()), int((act >= HIGH).sum())


@functools.lru_cache(maxsize=None)
def temperature(case):
    """The first of TEMPERATURES at which the case is decisive."""
    for T in TEMPERATURES:
        off, high = decisive(case, T)
        if off >= MIN_ROWS and (high >= MIN_ROWS or case[1] <= HIGH):
            return T
    raise AssertionError("no temperature of %s makes %s decisive" % (TEMPERATURES, case))
