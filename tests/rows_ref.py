"""TEST REFERENCE ONLY -- plain NumPy restatements of the kernels that move training rows, written from the contracts
in include/magent_amd.h (no torch, no engine library): the row mover (mfx_rows_copy_shift), the rollout collector
(mfx_collect_begin / _end / _end_linked), the compact row list (mfx_rollout_rows) and the mean-field kernels
(mfx_mean_action, mfx_mfq_target, mfx_mfac_returns; oracle/mf_oracle.py where it already states the rule).
tests/test_rows_ref_cpu.py checks each against an independent form."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import mf_oracle  # noqa: E402


# ---------------------------------------------------------------------------------------------------- the row mover
def rows_src(raw, src_mod, src_rows):
    """The source row of index raw: modulo src_mod when > 0 (the mathematical one, in [0, src_mod)), else numpy's
    indexing of src_rows rows; None when outside [0, src_rows)."""
    s = int(raw)
    if src_mod > 0:
        s %= int(src_mod)                  # python ints: exact at any magnitude, never negative
    elif s < 0:
        s += src_rows
    return s if 0 <= s < src_rows else None


def rows_copy_ref(dst, src, idx, src_mod, dst_start, dst_cap, n, shift_mask, shift):
    """mfx_rows_copy_shift on lists of arrays (first dimension = rows), in place on `dst`, one row at a time.  For
    i < n: raw = idx[i] (or i); columns without their bit in shift_mask read row rows_src(raw), the others
    rows_src(raw + shift) -- the shift is applied before the modulo / the negative-index rule --; with a shift mask the
    row is moved only when both are in range.  Destination row dst_start + i, modulo dst_cap when > 0.  Returns the
    list of reported indices in order of i (raw when the unshifted row is out of range, else raw + shift): the device
    reports whichever it meets first, so the first is only defined when there is one."""
    src_rows = min(len(s) for s in src)
    bad = []
    for i in range(int(n)):
        raw = int(idx[i]) if idx is not None else i
        s0 = rows_src(raw, src_mod, src_rows)
        s1 = rows_src(raw + int(shift), src_mod, src_rows) if shift_mask else s0
        if s0 is None or s1 is None:
            bad.append(raw if s0 is None else raw + int(shift))
            continue
        d = int(dst_start) + i
        if dst_cap > 0 and d >= dst_cap:
            d %= int(dst_cap)
        for k, (a, b) in enumerate(zip(dst, src)):
            a[d] = b[s1 if shift_mask >> k & 1 else s0]
    return bad


# ---------------------------------------------------------------------------------------------------- the row list
def rollout_rows_ref(counts, g, rowcap):
    """mfx_rollout_rows: rows e * rowcap + j for j < min(counts[e][g], rowcap), in env order (int32), and their
    number."""
    counts = np.asarray(counts)
    out = [e * rowcap + j for e in range(counts.shape[0]) for j in range(min(int(counts[e, g]), rowcap))]
    return np.asarray(out, dtype=np.int32), len(out)


# ---------------------------------------------------------------------------------------------------- the collector
def links_state(n_envs, id_stride):
    """The linked collector's state before a session's first step (mfx_collect_links_reset)."""
    return {"last": np.full(n_envs * id_stride, -1, dtype=np.int64), "key": np.zeros(0, dtype=np.int64),
            "tail": np.zeros(0, dtype=np.uint8), "prev": np.zeros(0, dtype=np.int64)}


def collect_ref(src_arrays, shape, n0, capacity, id_stride, linked_state=None, prob=True):
    """One mfx_collect_begin + mfx_collect_end (mfx_collect_end_linked when linked_state is given) pair.
    src_arrays: view [E, rowcap, V] f32, feat [E, rowcap, F] f32, actions / rewards / ids / alive [E, G, rowcap], mean
    [E, G, mean_stride] f64, stats [E, 4] f64, counts [E, G]; shape = (E, G, g, rowcap, V, F, A, mean_stride).
    Returns a dict: count (the list length), fits (n0 + count <= capacity), n (the row counter afterwards), err (bit 0:
    did not fit -- nothing at all is written; bit 1: an id outside [0, id_stride)), cols (obs feat act prob rew term
    key, `count` rows each when the step fits, else none) and, linked, state: the new {last, key, tail, prev} with
    key / tail / prev covering rows [0, n), tails of predecessors cleared.  linked_state is not modified.
    The link rule is chain_links' (the newest earlier row with the same key), kept across steps in the table `last`
    per (env, id): an entry whose row has another key (an earlier episode's) is stale and ignored; an id outside the
    table sets err bit 1, has no entry and starts a chain of its own."""
    E, G, g, rowcap, V, F, A, mean_stride = shape
    rows, count = rollout_rows_ref(src_arrays["counts"], g, rowcap)
    out = {"count": count, "fits": n0 + count <= capacity, "n": n0, "err": 0, "cols": None, "state": linked_state}
    if not out["fits"]:
        out["err"] = 1
        return out
    e, j = rows.astype(np.int64) // rowcap, rows.astype(np.int64) % rowcap      # list entry k = row j[k] of env e[k]
    ids = np.asarray(src_arrays["ids"])[e, g, j].astype(np.int64)
    episode = np.asarray(src_arrays["stats"])[e, 0].astype(np.int64)
    cols = {"obs": np.asarray(src_arrays["view"], np.float32).reshape(E, rowcap, V)[e, j],
            "feat": np.asarray(src_arrays["feat"], np.float32).reshape(E, rowcap, F)[e, j],
            "act": np.asarray(src_arrays["actions"], np.int32)[e, g, j],
            "rew": np.asarray(src_arrays["rewards"], np.float32)[e, g, j],
            "term": (np.asarray(src_arrays["alive"])[e, g, j] == 0).astype(np.uint8),
            "key": (episode * E + e) * id_stride + ids}              # replay.rollout_key, row by row
    if prob:
        cols["prob"] = np.asarray(src_arrays["mean"], np.float64)[e, g, :A].astype(np.float32)
    if ((ids < 0) | (ids >= id_stride)).any():
        out["err"] |= 2
    out["cols"], out["n"] = cols, n0 + count
    if linked_state is not None:
        last = linked_state["last"].copy()
        key = np.concatenate([linked_state["key"][:n0], cols["key"]])
        tail = np.concatenate([linked_state["tail"][:n0], np.ones(count, np.uint8)])
        prev = np.concatenate([linked_state["prev"][:n0], np.full(count, -1, np.int64)])
        for k, env in enumerate(e.tolist()):
            if 0 <= ids[k] < id_stride:
                p = int(last[env * id_stride + ids[k]])
                if p < 0 or p >= n0 or key[p] != key[n0 + k]:
                    p = -1
                last[env * id_stride + ids[k]] = n0 + k
                if p >= 0:
                    tail[p] = 0
                prev[n0 + k] = p
        out["state"] = {"last": last, "key": key, "tail": tail, "prev": prev}
    return out


# ---------------------------------------------------------------------------------------------------- mean field
def mean_action_ref(acts, counts, n_action):
    """mfx_mean_action: acts int32 [B, rowcap], counts [B] -> float64 [B, n_action].  Row b pools its first n =
    min(counts[b], rowcap) slots (a negative count reads as 0): where every pooled action is in [0, n_action) this is
    the oracle's np.mean of one-hot rows; an action outside the range is counted in no entry while n stays the
    divisor (a one-hot row of zeros); n = 0 gives NaN."""
    acts = np.asarray(acts)
    B, rowcap = acts.shape
    out = np.full((B, n_action), np.nan, dtype=np.float64)
    for b in range(B):
        n = max(0, min(int(counts[b]), rowcap))
        if n == 0:
            continue
        a = acts[b, :n]
        ok = (a >= 0) & (a < n_action)
        if ok.all():
            out[b] = mf_oracle.mean_action(a, n_action)[0]
        else:
            out[b] = np.bincount(a[ok], minlength=n_action).astype(np.float64) / np.float64(n)
    return out


def mfq_target_ref(e_q, t_q, rewards, dones, gamma=0.95):
    """mfx_mfq_target: the oracle's expression; a done byte is a flag (any non-zero value is done)."""
    return mf_oracle.mfq_target(np.asarray(e_q, np.float32), np.asarray(t_q, np.float32),
                                np.asarray(rewards, np.float32), np.asarray(dones) != 0, gamma)


def mfac_returns_ref(rewards, offsets, values, gamma=0.95, numpy1=True):
    """mfx_mfac_returns: the oracle's loop per episode rewards[offsets[e] : offsets[e + 1]] (an empty episode has no
    rows); a new float32 array."""
    out = np.array(rewards, dtype=np.float32)
    for e in range(len(values)):
        a, b = int(offsets[e]), int(offsets[e + 1])
        out[a:b] = mf_oracle.mfac_returns(out[a:b], values[e], gamma, numpy1=numpy1)
    return out
