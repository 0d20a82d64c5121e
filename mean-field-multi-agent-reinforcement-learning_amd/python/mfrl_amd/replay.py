"""Row moves of the device replay buffers (mfrl_amd.algo.tools) on the HIP kernel k_rows_copy
(csrc/replay_kernels.hip): every push / tight / sample of MemoryGroup and EpisodesBuffer (algo/tools.py:26-362)
is one launch that gathers whole rows of all its columns.  CUDA tensors only; a missing engine library raises.
"""
import ctypes

import numpy as np
import torch

from . import check, lib

_MAX_COLS = 12


def rows_copy(dst, src, idx=None, src_mod=0, dst_start=0, dst_cap=0, n=None, shift_mask=0, shift=0):
    """For i < n: row (idx[i] if idx is not None else i), taken modulo src_mod if > 0, of every tensor in
    `src` -> row dst_start + i (modulo dst_cap if > 0) of the matching tensor in `dst`.  Tensors: CUDA,
    contiguous, first dimension = rows, equal row byte sizes pairwise.  Without src_mod, an index in
    [-rows, 0) counts from the end as numpy's does; any other index outside the source rows is skipped on the
    device and raised by the next check_errors() (the reference's numpy indexing raises IndexError at once;
    checking here would synchronise every move).  Columns k with bit k of shift_mask set read row idx[i] + shift
    instead (before the modulo): MemoryGroup.sample's next-state columns in the launch of the current ones."""
    assert len(dst) == len(src) and 0 < len(dst) <= _MAX_COLS
    if n is None:
        n = len(idx) if idx is not None else src[0].shape[0]
    if n == 0:
        return
    rb = []
    for d, s in zip(dst, src):
        assert d.is_cuda and s.is_cuda and d.is_contiguous() and s.is_contiguous(), "rows_copy: contiguous CUDA tensors"
        b = d.element_size() * (d[0].numel() if d.dim() > 1 else 1)
        assert b == s.element_size() * (s[0].numel() if s.dim() > 1 else 1), "rows_copy: row sizes differ"
        rb.append(b)
    if idx is not None:
        idx = idx.to(device=dst[0].device, dtype=torch.int64).contiguous()
    k = len(dst)
    src_rows = min(s.shape[0] for s in src)
    L = lib()
    L.mfx_rows_copy.restype = ctypes.c_int
    P = ctypes.c_void_p * k
    L.mfx_rows_copy_shift.restype = ctypes.c_int
    check(L.mfx_rows_copy_shift(k, P(*[d.data_ptr() for d in dst]), P(*[s.data_ptr() for s in src]),
                                (ctypes.c_int64 * k)(*rb), ctypes.c_void_p(idx.data_ptr() if idx is not None else 0),
                                ctypes.c_int64(int(src_mod)), ctypes.c_int64(int(src_rows)),
                                ctypes.c_int64(int(dst_start)), ctypes.c_int64(int(dst_cap)), ctypes.c_int64(int(n)),
                                ctypes.c_uint32(int(shift_mask)), ctypes.c_int64(int(shift)),
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
          "mfx_rows_copy_shift")


def rows_plan(dst, src, shift_mask=0):
    """The launch form rows_copy would take for these columns (mfx_rows_copy_plan; nothing is launched): a dict of
    form (0 = k_rows_copy, 1 = k_rows_pipe), nw and nu (the pipelined form's template arguments, 0 otherwise), units
    (narrow units of a row) and cols (per column: 0 narrow in dwords, 1 narrow in bytes, 2 wide).  MFX_ROWS_PIPE is
    honoured as by the launcher.  For the tests: a case asserts the form it was written for."""
    assert len(dst) == len(src) and 0 < len(dst) <= _MAX_COLS
    rb = [d.element_size() * (d[0].numel() if d.dim() > 1 else 1) for d in dst]
    k = len(dst)
    L = lib()
    L.mfx_rows_copy_plan.restype = ctypes.c_int
    P = ctypes.c_void_p * k
    out = (ctypes.c_int32 * (4 + k))()
    check(L.mfx_rows_copy_plan(k, P(*[d.data_ptr() for d in dst]), P(*[s.data_ptr() for s in src]),
                               (ctypes.c_int64 * k)(*rb), ctypes.c_uint32(int(shift_mask)), out), "mfx_rows_copy_plan")
    return {"form": out[0], "nw": out[1], "nu": out[2], "units": out[3], "cols": list(out[4:4 + k])}


def rollout_key(env, episode, agent_id, n_envs, id_stride):
    """The agent key of a collected row (csrc/collect_kernels.hip collect_key): injective over env < n_envs,
    episode >= 0 and agent_id < id_stride.  Ids restart at 0 in every episode, so the episode number is part of it."""
    return (episode * n_envs + env) * id_stride + agent_id


class _CollectSrc(ctypes.Structure):      # mfx_collect_src (include/magent_amd.h)
    _fields_ = ([(k, ctypes.c_void_p) for k in ("view", "feat", "actions", "rewards", "mean", "stats", "counts", "ids",
                                                  "alive")] +
                [(k, ctypes.c_int32) for k in ("n_envs", "n_groups", "group", "rowcap", "view_floats", "feat_floats",
                                               "n_action", "mean_stride")])


class _CollectDst(ctypes.Structure):      # mfx_collect_dst
    _fields_ = ([(k, ctypes.c_void_p) for k in ("obs", "feat", "act", "rew", "term", "prob", "key")] +
                [("capacity", ctypes.c_int64)])


class CollectOverflow(RuntimeError):
    pass


class RolloutCollector:
    """Replay rows of group `group` straight from a BattleBatch's device rollout loop into a MemoryGroup's step rows
    (algo/tools.py _StepRows), one row per live agent per rollout_policy_step, on the HIP kernels of
    csrc/collect_kernels.hip:

        policy.act_rollout(eng, g) ...      # the actions are in the rollout's action buffer
        col.begin()                         # view, feature, action, former mean action, episode number
        eng.rollout_policy_step()
        col.end()                           # reward, terminal = !alive, key; the device row counter advances
        ...
        col.finish()                        # one synchronise: _StepRows.n = the counter; raises on overflow

    after which MemoryGroup.tight() / get_batch_num() / sample() and ValueNet.train_batches run unchanged.  Nothing is
    read back between the first begin() and finish(): the row count is on the device, so begin() reserves storage for
    the worst case of one more step (E * rowcap rows past a running upper bound of the count; geometric growth, the
    grow copy moves the rows up to the bound).  Every launch, allocation and copy is ordered on the engine's stream
    (eng.stream_handle()), whatever stream the caller is on.  capacity: never write a row at or past this index (a
    step that would is dropped whole and finish() raises CollectOverflow); None: grow as needed.

    `memory_group` is any owner of step rows in `_rows`: a MemoryGroup, or an EpisodesBuffer after prepare().  Rows
    with link columns (_StepRows(links=True), EpisodesBuffer's) take the linked path: end() also writes prev (the
    row of the same agent's previous step in the same episode, or -1) and tail (the row is its agent's last so far)
    through a device table of the newest row per (env, id), which the session's first begin() resets.  An agent's
    chain so ends at its death, at the end of its episode (done or the step cap), or at the end of the session.
    The linked path refuses rows pushed by other means (they have no links): ValueError at begin().

    prob_rows (None: the prob column is the env's mean action, the rollout's mean buffer cast to float): a float32 CUDA
    tensor [E, rowcap, n_action], contiguous -- the row of agent j of env e takes prob_rows[e, j] bit for bit (the
    neighbourhood mean, mfrl_amd.mf.NeighborMean.rows).  begin() reads it on the engine's stream: it must hold what
    the policy acted with.  end, end_linked and finish are the same on both paths."""

    def __init__(self, eng, memory_group, group=0, capacity=None, prob_rows=None):
        self.eng, self.mg, self.group, self.capacity = eng, memory_group, int(group), capacity
        self.prob_rows = prob_rows          # see the class docstring; may be set between steps
        self._bound = None                  # upper bound of the device row counter; None: no step since finish()
        self._state = self._scratch = self._last = None
        self._src = self._dst = None
        if memory_group._rows is None:
            raise ValueError("RolloutCollector: the buffer has no step rows yet (EpisodesBuffer.prepare() makes them)")
        if memory_group._rows.device != "cpu":
            L = lib()
            for fn in ("mfx_collect_reset", "mfx_collect_begin", "mfx_collect_end", "mfx_collect_end_linked",
                       "mfx_collect_links_reset"):
                getattr(L, fn).restype = ctypes.c_int
            if hasattr(L, "mfx_collect_begin_rows"):        # (absent from older builds, which the bench scripts may load)
                L.mfx_collect_begin_rows.restype = ctypes.c_int
            self._L = L

    @property
    def linked(self):
        return bool(getattr(self.mg._rows, "links", False))

    # ---- host bookkeeping (runs without a GPU)
    def step_rows(self):
        """Worst-case rows of one step: every row slot of the group in every env."""
        return self.eng.n_envs * self.eng.rowcap

    def id_stride(self):
        """Ids of an episode are below this: no more agents than row slots over all groups."""
        return len(self.eng.handles) * self.eng.rowcap

    def _reserve(self):
        """Storage for one more step past the bound; returns the capacity in rows the kernels may write."""
        rows = self.mg._rows
        if self._bound is None:
            self._bound = rows.n
        need = self._bound + self.step_rows()
        if self.capacity is not None:
            need = min(need, int(self.capacity))
        old = list(rows.cols.values()) if need > rows.cap else []
        rows._ensure(need, live=self._bound)
        for t in old:                       # the old columns may still be read by the grow copy on this stream
            if t.is_cuda:
                t.record_stream(torch.cuda.current_stream())
        self._bound = min(self._bound + self.step_rows(), rows.cap)
        return rows.cap if self.capacity is None else min(rows.cap, int(self.capacity))

    # ---- device
    def _buffer(self, name, group=0):
        p, nb = ctypes.c_void_p(), ctypes.c_size_t()
        self.eng._check(self.eng._dll.mfx_battle_rollout_buffer(self.eng.game, name.encode(), group, ctypes.byref(p),
                                                                ctypes.byref(nb)), "rollout_buffer")
        return p.value

    def begin(self):
        eng, rows = self.eng, self.mg._rows
        E, rc, G = eng.n_envs, eng.rowcap, len(eng.handles)
        st = ctypes.c_void_p(eng.stream_handle())
        fresh = self._bound is None
        if fresh and self.linked and rows.n != 0:
            raise ValueError("RolloutCollector: %d rows pushed by other means are present; they have no links "
                             "(clear the buffer first)" % rows.n)
        with torch.cuda.stream(self.eng.torch_stream()):
            if self._state is None:
                self._state = torch.zeros(2, dtype=torch.int64, device="cuda")
            if self._scratch is None or self._scratch.numel() < E * rc + 1 + (E + 63) // 64:
                self._scratch = torch.empty(E * rc + 1 + (E + 63) // 64, dtype=torch.int32, device="cuda")
            cap = self._reserve()
            if fresh:
                check(self._L.mfx_collect_reset(ctypes.c_void_p(self._state.data_ptr()), ctypes.c_int64(rows.n), st),
                      "mfx_collect_reset")
            if self.linked:
                slots = E * self.id_stride()
                if self._last is None or self._last.numel() != slots:
                    self._last = torch.empty(slots, dtype=torch.int64, device="cuda")
                    fresh = True
                if fresh:
                    check(self._L.mfx_collect_links_reset(ctypes.c_void_p(self._last.data_ptr()),
                                                          ctypes.c_int64(slots), st), "mfx_collect_links_reset")
        V = 1
        for x in rows.obs_shape:
            V *= int(x)
        F = 1
        for x in rows.feat_shape:
            F *= int(x)
        g = self.group
        self._src = _CollectSrc(self._buffer("view", g), self._buffer("feature", g), self._buffer("actions"),
                                self._buffer("rewards"), self._buffer("mean_action"), self._buffer("stats"),
                                self._buffer("group_num"), self._buffer("ids"), self._buffer("alive"),
                                E, G, g, rc, V, F, int(rows.act_n), eng.mean_stride())
        c = rows.cols
        self._dst = _CollectDst(c["obs"].data_ptr(), c["feat"].data_ptr(), c["act"].data_ptr(), c["rew"].data_ptr(),
                                c["term"].data_ptr(), c["prob"].data_ptr() if rows.use_mean else None,
                                c["ids"].data_ptr(), cap)
        self._links = ((ctypes.c_void_p(self._last.data_ptr()), ctypes.c_void_p(c["prev"].data_ptr()),
                        ctypes.c_void_p(c["tail"].data_ptr())) if self.linked else None)
        self._ptrs = (ctypes.c_void_p(self._scratch.data_ptr()), ctypes.c_void_p(self._scratch.data_ptr() + 4 * E * rc),
                      ctypes.c_void_p(self._state.data_ptr()))
        P = self.prob_rows
        if P is not None:
            if not rows.use_mean:
                raise ValueError("RolloutCollector: prob_rows given, but the step rows have no prob column")
            if (P.dtype != torch.float32 or not P.is_cuda or not P.is_contiguous()
                    or tuple(P.shape) != (E, rc, int(rows.act_n))):
                raise ValueError("RolloutCollector: prob_rows must be a contiguous float32 CUDA tensor [%d, %d, %d], got "
                                 "%s %s" % (E, rc, int(rows.act_n), P.dtype, tuple(P.shape)))
            check(self._L.mfx_collect_begin_rows(ctypes.byref(self._src), ctypes.byref(self._dst),
                                                 ctypes.c_void_p(P.data_ptr()), *self._ptrs, st), "mfx_collect_begin_rows")
            return
        check(self._L.mfx_collect_begin(ctypes.byref(self._src), ctypes.byref(self._dst), *self._ptrs, st),
              "mfx_collect_begin")

    def end(self):
        assert self._src is not None, "RolloutCollector.end() without begin()"
        if self._links is not None:
            check(self._L.mfx_collect_end_linked(ctypes.byref(self._src), ctypes.byref(self._dst), *self._ptrs,
                                                 ctypes.c_int64(self.id_stride()), *self._links,
                                                 ctypes.c_void_p(self.eng.stream_handle())), "mfx_collect_end_linked")
        else:
            check(self._L.mfx_collect_end(ctypes.byref(self._src), ctypes.byref(self._dst), *self._ptrs,
                                          ctypes.c_int64(self.id_stride()), ctypes.c_void_p(self.eng.stream_handle())),
                  "mfx_collect_end")
        self._src = None

    def discard(self):
        """Drop the rows collected since the last finish() without reading anything back: the next begin() restarts
        the device counter at _StepRows.n (and clears the error word)."""
        self._bound = None

    def finish(self):
        """Synchronise the engine's stream once; the step rows now hold the collected rows (returns their number).
        Raises CollectOverflow when a step did not fit below `capacity` (its rows were dropped; _StepRows.n is left
        as it was before the first begin())."""
        if self._bound is None:
            return self.mg._rows.n
        with torch.cuda.stream(self.eng.torch_stream()):
            n, err = self._state.cpu().tolist()
        self._bound = None
        if err:
            raise CollectOverflow("RolloutCollector: %s" % ("a step's rows did not fit below the capacity of %s rows"
                                                            % self.capacity if err & 1 else
                                                            "an agent id outside [0, %d)" % self.id_stride()))
        self.last_rows = int(n) - self.mg._rows.n      # rows of this session (begin() of its first step .. finish())
        self.mg._rows.n = int(n)
        return int(n)


def chain_returns(rew, prev, tails, values, gamma=0.95, numpy1=True):
    """Discounted returns in place on the float32 column `rew` of step-major rows (HIP kernel k_chain_returns):
    for chain i, keep = values[i], then along r = tails[i], prev[r], ... to -1: keep = keep * gamma + rew[r];
    rew[r] = keep, in mf.mfac_returns' two arithmetic forms.  A row index outside its chain's rows raises IndexError
    (the walk stops before it; the call synchronises the current stream to know)."""
    assert rew.is_cuda and rew.dtype == torch.float32 and rew.is_contiguous()
    assert prev.dtype == torch.int64 and prev.is_contiguous() and len(prev) >= len(rew)
    tails = tails.to(torch.int64).contiguous()
    values = values.to(torch.float32).contiguous()
    assert len(values) == len(tails)
    L = lib()
    L.mfx_chain_returns.restype = ctypes.c_int
    if L.mfx_chain_returns(ctypes.c_void_p(rew.data_ptr()), ctypes.c_void_p(prev.data_ptr()),
                           ctypes.c_void_p(tails.data_ptr()), ctypes.c_void_p(values.data_ptr()),
                           ctypes.c_int64(len(tails)), ctypes.c_int64(len(rew)), ctypes.c_double(gamma),
                           int(bool(numpy1)), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) != 0:
        L.mfx_last_error.restype = ctypes.c_char_p
        raise IndexError(L.mfx_last_error().decode())
    return rew


def chain_gae(rew, adv, prev, tails, values, gamma=0.95, lam=0.95):
    """GAE(lambda) along the chains chain_returns walks (HIP kernel k_chain_gae; the contract is mfx_chain_gae's in
    include/magent_amd.h): `values` holds one float32 value per row of `rew`; the advantages go to the float32 column
    `adv` and `rew` becomes advantage + value, in place.  -> (rew, adv).  gamma and lam must lie in [0, 1]
    (ValueError); a row index outside its chain's rows raises IndexError (the walk stops before it; the call
    synchronises the current stream to know)."""
    if not (0.0 <= gamma <= 1.0 and 0.0 <= lam <= 1.0):
        raise ValueError("chain_gae: gamma %r and lambda %r must lie in [0, 1]" % (gamma, lam))
    assert rew.is_cuda and rew.dtype == torch.float32 and rew.is_contiguous()
    n = len(rew)
    assert adv.is_cuda and adv.dtype == torch.float32 and adv.is_contiguous() and len(adv) >= n
    assert values.is_cuda and values.dtype == torch.float32 and values.is_contiguous() and len(values) >= n
    assert prev.dtype == torch.int64 and prev.is_contiguous() and len(prev) >= n
    tails = tails.to(torch.int64).contiguous()
    L = lib()
    L.mfx_chain_gae.restype = ctypes.c_int
    if L.mfx_chain_gae(ctypes.c_void_p(rew.data_ptr()), ctypes.c_void_p(adv.data_ptr()),
                       ctypes.c_void_p(prev.data_ptr()), ctypes.c_void_p(tails.data_ptr()),
                       ctypes.c_void_p(values.data_ptr()), ctypes.c_int64(len(tails)), ctypes.c_int64(n),
                       ctypes.c_double(gamma), ctypes.c_double(lam),
                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) != 0:
        L.mfx_last_error.restype = ctypes.c_char_p
        raise IndexError(L.mfx_last_error().decode())
    return rew, adv


def adv_normalize(adv):
    """adv <- (adv - mean) / (std + 1e-8) in place on the float32 column `adv` (mfx_adv_normalize: mean and population
    standard deviation in float64, one summation order per length, no atomics); nothing is read back."""
    assert adv.is_cuda and adv.dtype == torch.float32 and adv.is_contiguous()
    L = lib()
    L.mfx_adv_normalize.restype = ctypes.c_int
    check(L.mfx_adv_normalize(ctypes.c_void_p(adv.data_ptr()), ctypes.c_int64(adv.numel()),
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "mfx_adv_normalize")
    return adv


def chain_links(keys):
    """Host restatement of the linked collector's two columns, for the tests: for the key column of step-major
    rows, prev[r] = the latest earlier row with the same key (or -1) and tail[r] = no later row has it."""
    keys = np.asarray(keys, dtype=np.int64)
    prev = np.full(len(keys), -1, dtype=np.int64)
    tail = np.zeros(len(keys), dtype=bool)
    last = {}
    for r, k in enumerate(keys.tolist()):
        p = last.get(k, -1)
        prev[r] = p
        if p >= 0:
            tail[p] = False
        tail[r] = True
        last[k] = r
    return prev, tail


def chain_returns_host(rew, prev, tails, values, gamma=0.95, numpy1=True):
    """Host restatement of chain_returns in numpy, for the tests: a new float32 array.  numpy1: keep runs in
    float64 (the reference's NumPy-1 promotion); else keep and gamma are float32 (NEP 50)."""
    out = np.array(rew, dtype=np.float32)
    prev = np.asarray(prev, dtype=np.int64)
    T = np.float64 if numpy1 else np.float32
    g = T(gamma)
    for t, v in zip(np.asarray(tails, dtype=np.int64).tolist(), np.asarray(values, dtype=np.float32)):
        keep, r = T(v), t
        while r != -1:
            keep = T(T(keep * g) + T(out[r]))
            out[r] = keep
            r = int(prev[r])
    return out


def check_errors():
    """Synchronise the current stream; raise IndexError if a rows_copy since the last check met a source
    index outside its source rows (that row was skipped)."""
    L = lib()
    L.mfx_rows_copy_error.restype = ctypes.c_int
    bad = ctypes.c_int64()
    if L.mfx_rows_copy_error(ctypes.byref(bad), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) != 0:
        raise IndexError("rows_copy: source index %d out of range" % bad.value)
