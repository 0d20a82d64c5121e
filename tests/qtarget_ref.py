"""Test infrastructure: the opt-in Boltzmann mean-field value target of the Q models (include/magent_amd.h,
mfx_mfq_target_boltzmann) restated in numpy.  For one row, e_q from the eval net and t_q from the target net
on the next state, 2 <= A <= 32, T finite and > 0:

    weights(e_q, T)     the acting weights of csrc/qsample.h (qsample_ref.weights: float32 (e_q - max) / T, one rounding
                        per operation, then exp), with its non-finite rule: a row with any NaN or +-inf gets 1 at its
                        greedy action (qsample_ref.greedy) and 0 elsewhere.  As qsample_ref.weights, within an ulp or so
                        of the device's expf and NOT bit-equal to it, except where a weight is exactly 0 or 1; tests that
                        need the device's bits pass the device's own weights as w
    value(w, t_q)       num = sum_a f64(w[a]) f64(t_q[a]), den = sum_a f64(w[a]), ascending action order in float64;
                        num / den
    target(e_q, t_q, r, done, gamma, T, w=None)   f64(r) + ((1 - done) * value) * gamma, float64; done: any non-zero byte
    target64(q_e, q_t, r, done, gamma, T)         the same rule with the float64 softmax of float64 Q values (the
                        accuracy yardstick of the training-step test; no float32 step anywhere)

The max rule's np.argmax lets the first NaN of e_q win; this rule follows the acting policy, which never takes a NaN."""
import math

import numpy as np

import qsample_ref as qs

MAX_A = 32


def check(A, T):
    if not 2 <= int(A) <= MAX_A:
        raise ValueError("qtarget: 2 <= A <= 32, got %d" % A)
    T = float(T)
    if not (math.isfinite(T) and T > 0.0):
        raise ValueError("qtarget: the temperature must be finite and > 0, got %r" % (T,))
    return T


def weights(e_q, T):
    e_q = np.asarray(e_q, dtype=np.float32)
    T = check(e_q.shape[1], T)
    w = np.array(qs.weights(e_q, T), dtype=np.float32)
    bad = ~qs.finite_rows(e_q)
    if bad.any():
        hot = np.zeros((int(bad.sum()), e_q.shape[1]), dtype=np.float32)
        hot[np.arange(len(hot)), qs.greedy(e_q[bad])] = 1.0
        w[bad] = hot
    return w


def value(w, t_q):
    w = np.asarray(w, dtype=np.float32).astype(np.float64)
    t = np.asarray(t_q, dtype=np.float32).astype(np.float64)
    num, den = np.zeros(len(w)), np.zeros(len(w))
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(w.shape[1]):
            num = num + w[:, a] * t[:, a]
            den = den + w[:, a]
        return num / den


def target(e_q, t_q, r, done, gamma, T, w=None):
    """w: the float32 weights to use (the device's own), else weights(e_q, T)."""
    e_q = np.asarray(e_q, dtype=np.float32)
    check(e_q.shape[1], T)
    v = value(weights(e_q, T) if w is None else w, t_q)
    notdone = 1.0 - (np.asarray(done) != 0).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(r, dtype=np.float32).astype(np.float64) + (notdone * v) * float(gamma)


def target64(q_e, q_t, r, done, gamma, T):
    p = qs.softmax64(q_e, T)
    v = (p * np.asarray(q_t, dtype=np.float64)).sum(axis=1)
    notdone = 1.0 - (np.asarray(done) != 0).astype(np.float64)
    return np.asarray(r, dtype=np.float64) + (notdone * v) * float(gamma)
