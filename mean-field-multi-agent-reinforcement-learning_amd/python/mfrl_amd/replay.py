"""Row moves of the device replay buffers (mfrl_amd.algo.tools) on the HIP kernel k_rows_copy
(csrc/replay_kernels.hip): every push / tight / sample of MemoryGroup and EpisodesBuffer (algo/tools.py:26-362)
is one launch that gathers whole rows of all its columns.  CUDA tensors only; a missing engine library raises.
"""
import ctypes

import numpy as np
import torch

from . import check, lib
from .abi import ptr, stream, struct

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
    P = ctypes.c_void_p * k
    check(lib().mfx_rows_copy_shift(k, P(*[d.data_ptr() for d in dst]), P(*[s.data_ptr() for s in src]),
                                    (ctypes.c_int64 * k)(*rb), ptr(idx), int(src_mod), int(src_rows), int(dst_start),
                                    int(dst_cap), int(n), int(shift_mask), int(shift), stream()), "mfx_rows_copy_shift")


def rows_plan(dst, src, shift_mask=0):
    """The launch form rows_copy would take for these columns (mfx_rows_copy_plan; nothing is launched): a dict of
    form (0 = k_rows_copy, 1 = k_rows_pipe), nw and nu (the pipelined form's template arguments, 0 otherwise), units
    (narrow units of a row) and cols (per column: 0 narrow in dwords, 1 narrow in bytes, 2 wide).  MFX_ROWS_PIPE is
    honoured as by the launcher.  For the tests: a case asserts the form it was written for."""
    assert len(dst) == len(src) and 0 < len(dst) <= _MAX_COLS
    rb = [d.element_size() * (d[0].numel() if d.dim() > 1 else 1) for d in dst]
    k = len(dst)
    P = ctypes.c_void_p * k
    out = (ctypes.c_int32 * (4 + k))()
    check(lib().mfx_rows_copy_plan(k, P(*[d.data_ptr() for d in dst]), P(*[s.data_ptr() for s in src]),
                                   (ctypes.c_int64 * k)(*rb), int(shift_mask), out), "mfx_rows_copy_plan")
    return {"form": out[0], "nw": out[1], "nu": out[2], "units": out[3], "cols": list(out[4:4 + k])}


def rollout_key(env, episode, agent_id, n_envs, id_stride):
    """The agent key of a collected row (csrc/collect_kernels.hip collect_key): injective over env < n_envs,
    episode >= 0 and agent_id < id_stride.  Ids restart at 0 in every episode, so the episode number is part of it."""
    return (episode * n_envs + env) * id_stride + agent_id


_CollectSrc, _CollectDst = struct("mfx_collect_src"), struct("mfx_collect_dst")


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
            self._L = lib()

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
    def begin(self):
        eng, rows = self.eng, self.mg._rows
        E, rc, G = eng.n_envs, eng.rowcap, len(eng.handles)
        st = eng.stream_handle()
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
                check(self._L.mfx_collect_reset(ptr(self._state), rows.n, st), "mfx_collect_reset")
            if self.linked:
                slots = E * self.id_stride()
                if self._last is None or self._last.numel() != slots:
                    self._last = torch.empty(slots, dtype=torch.int64, device="cuda")
                    fresh = True
                if fresh:
                    check(self._L.mfx_collect_links_reset(ptr(self._last), slots, st), "mfx_collect_links_reset")
        V = 1
        for x in rows.obs_shape:
            V *= int(x)
        F = 1
        for x in rows.feat_shape:
            F *= int(x)
        g = self.group
        self._src = _CollectSrc(eng.rollout_buffer("view", g), eng.rollout_buffer("feature", g),
                                *[eng.rollout_buffer(k) for k in ("actions", "rewards", "mean_action", "stats", "group_num",
                                                                  "ids", "alive")],
                                E, G, g, rc, V, F, int(rows.act_n), eng.mean_stride())
        c = rows.cols
        self._dst = _CollectDst(ptr(c["obs"]), ptr(c["feat"]), ptr(c["act"]), ptr(c["rew"]), ptr(c["term"]),
                                ptr(c["prob"]) if rows.use_mean else None, ptr(c["ids"]), cap)
        self._links = (ptr(self._last), ptr(c["prev"]), ptr(c["tail"])) if self.linked else None
        self._ptrs = (ptr(self._scratch), ptr(self._scratch) + 4 * E * rc, ptr(self._state))
        P = self.prob_rows
        if P is not None:
            if not rows.use_mean:
                raise ValueError("RolloutCollector: prob_rows given, but the step rows have no prob column")
            if (P.dtype != torch.float32 or not P.is_cuda or not P.is_contiguous()
                    or tuple(P.shape) != (E, rc, int(rows.act_n))):
                raise ValueError("RolloutCollector: prob_rows must be a contiguous float32 CUDA tensor [%d, %d, %d], got "
                                 "%s %s" % (E, rc, int(rows.act_n), P.dtype, tuple(P.shape)))
            check(self._L.mfx_collect_begin_rows(ctypes.byref(self._src), ctypes.byref(self._dst), ptr(P), *self._ptrs, st),
                  "mfx_collect_begin_rows")
            return
        check(self._L.mfx_collect_begin(ctypes.byref(self._src), ctypes.byref(self._dst), *self._ptrs, st),
              "mfx_collect_begin")

    def end(self):
        assert self._src is not None, "RolloutCollector.end() without begin()"
        if self._links is not None:
            check(self._L.mfx_collect_end_linked(ctypes.byref(self._src), ctypes.byref(self._dst), *self._ptrs,
                                                 self.id_stride(), *self._links, self.eng.stream_handle()),
                  "mfx_collect_end_linked")
        else:
            check(self._L.mfx_collect_end(ctypes.byref(self._src), ctypes.byref(self._dst), *self._ptrs,
                                          self.id_stride(), self.eng.stream_handle()), "mfx_collect_end")
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
    if L.mfx_chain_returns(ptr(rew), ptr(prev), ptr(tails), ptr(values), len(tails), len(rew), gamma,
                           int(bool(numpy1)), stream()) != 0:
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
    if L.mfx_chain_gae(ptr(rew), ptr(adv), ptr(prev), ptr(tails), ptr(values), len(tails), n, gamma, lam,
                       stream()) != 0:
        raise IndexError(L.mfx_last_error().decode())
    return rew, adv


def adv_normalize(adv):
    """adv <- (adv - mean) / (std + 1e-8) in place on the float32 column `adv` (mfx_adv_normalize: mean and population
    standard deviation in float64, one summation order per length, no atomics); nothing is read back."""
    assert adv.is_cuda and adv.dtype == torch.float32 and adv.is_contiguous()
    check(lib().mfx_adv_normalize(ptr(adv), adv.numel(), stream()), "mfx_adv_normalize")
    return adv


def policy_logp(policy, act, out):
    """out[i] = log(policy[i, act[i]] + 1e-6) in float32 for the n rows of `policy` (HIP kernel k_policy_logp; the
    contract is mfx_policy_logp's in include/magent_amd.h): policy [n, A] float32 (ACNetHIP.forward's clamped policy),
    act int32 and out float32 of at least n rows.  A row whose action is outside [0, A) gets +0 -- the training step on
    those rows reports it.  Nothing is read back.  -> out."""
    assert policy.is_cuda and policy.dtype == torch.float32 and policy.is_contiguous() and policy.dim() == 2
    n, A = policy.shape
    assert act.is_cuda and act.dtype == torch.int32 and act.is_contiguous() and act.dim() == 1 and len(act) >= n
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 1 and len(out) >= n
    check(lib().mfx_policy_logp(ptr(policy), ptr(act), int(n), int(A), ptr(out), stream()), "mfx_policy_logp")
    return out


def ppo_order(seed, round, epoch, M):
    """The order in which epoch `epoch` of round `round` takes the M minibatch segments of ActorCritic.objective =
    "ppo": a permutation of range(M) from a generator of its own, keyed by the three integers -- equal keys give equal
    orders, and the global np.random stream is not drawn from."""
    rng = np.random.Generator(np.random.PCG64([int(seed), int(round), int(epoch)]))
    return [int(k) for k in rng.permutation(int(M))]


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
    bad = ctypes.c_int64()
    if lib().mfx_rows_copy_error(ctypes.byref(bad), stream()) != 0:
        raise IndexError("rows_copy: source index %d out of range" % bad.value)
