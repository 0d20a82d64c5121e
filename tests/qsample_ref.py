"""Test infrastructure: the Boltzmann draw of the Q models' opt-in acting mode (csrc/qsample.h) restated
in numpy.

    uniforms(seed, step, group, rows)   ac_uniform in uint32: the 24-bit float32 uniform of a row
    softmax64(q, T)                     the float64 softmax of q / T (the tolerance check of the kernel's weights)
    weights(q, T)                       float32 weights from q: np.exp in float64 of the float32 (q - max) / T, rounded
                                        once -- within an ulp or so of the device's expf, NOT bit-equal to it; tests
                                        that need the device's actions exactly run draw() on the device's own weights
    draw(w, u)                          the running-sum draw in float32 on given float32 weight rows
    greedy(q)                           the first maximum over the non-NaN entries (0 for an all-NaN row)
    sample(q, T, seed, step, group, rows, w=None)   the whole rule, non-finite rows included

The hash is written out here in full; tests/test_qsample_cpu.py holds it to tests/acnet_ref.py's (the device calls one
function for both networks)."""
import numpy as np

_U32 = np.uint32


def _mix32(h):
    h = np.asarray(h, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        h ^= h >> _U32(16)
        h *= _U32(0x85EBCA6B)
        h ^= h >> _U32(13)
        h *= _U32(0xC2B2AE35)
        h ^= h >> _U32(16)
    return h


def uniforms(seed, step, group, rows):
    with np.errstate(over="ignore"):
        a = np.array([(int(step) * 0x9E3779B9 + int(group) * 0x632BE5AB) & 0xFFFFFFFF], dtype=np.uint32)
        r = np.asarray(rows).astype(np.uint32) * _U32(0x85EBCA77) + _U32(0x165667B1)
    k = _U32(int(seed) & 0xFFFFFFFF) ^ _mix32(a)[0] ^ _mix32(r)
    return (_mix32(k) >> _U32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def softmax64(q, T):
    x = np.asarray(q, dtype=np.float64) / float(np.float32(T))
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def finite_rows(q):
    return np.isfinite(np.asarray(q)).all(axis=1)


def greedy(q):
    q = np.asarray(q, dtype=np.float32)
    nan = np.isnan(q)
    m = np.where(nan, -np.inf, q).max(axis=1, keepdims=True)
    return np.argmax(~nan & (q == m), axis=1).astype(np.int32)      # (no candidate: argmax of all-False is 0)


def weights(q, T):
    q = np.asarray(q, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (q - q.max(axis=1, keepdims=True)).astype(np.float32)
        x = (d / np.float32(T)).astype(np.float32)
        return np.exp(x.astype(np.float64)).astype(np.float32)


def draw(w, u):
    """The first action whose running float32 sum exceeds u * total (total: the float32 sum in action order);
    A - 1 if none does."""
    w = np.asarray(w, dtype=np.float32)
    n, A = w.shape
    tot = np.zeros(n, dtype=np.float32)
    for a in range(A):
        tot = (tot + w[:, a]).astype(np.float32)
    thr = (np.asarray(u, dtype=np.float32) * tot).astype(np.float32)
    run = np.zeros(n, dtype=np.float32)
    pick = np.full(n, -1, dtype=np.int64)
    for a in range(A):
        run = (run + w[:, a]).astype(np.float32)
        pick = np.where((pick < 0) & (run > thr), a, pick)
    return np.where(pick < 0, A - 1, pick).astype(np.int32)


def sample(q, T, seed, step, group, rows, w=None):
    """Actions [n] of Q rows [n, A]; w: the float32 weights to draw from (the device's own), else weights(q, T).
    Rows with a non-finite entry take greedy(q)."""
    q = np.asarray(q, dtype=np.float32)
    fin = finite_rows(q)
    ww = np.array(weights(q, T) if w is None else w, dtype=np.float32)
    ww[~fin] = 1.0                                    # (any finite row: the draw of these rows is discarded)
    act = draw(ww, uniforms(seed, step, group, rows))
    return np.where(fin, act, greedy(q)).astype(np.int32)
