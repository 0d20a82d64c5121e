"""Mean-field pieces of the training loop on device (torch tensors in, torch tensors out).

    mean_action(actions, counts, n_action)   senario_battle.py:141 (former_act_prob), float64
    mfq_target(e_q, t_q, rewards, dones, g)  algo/base.py:192-220 (ValueNet.calc_target_q), float64
    mfac_returns(rewards, offsets, values, g) algo/ac.py:305-320 (discounted returns, float64 running
                                             return stored as float32: the reference's NumPy-1 rules)
    mfq_target_boltzmann(e_q, t_q, r, d, g, T)  the opt-in Boltzmann value target (the paper's v^MF), float64
    neighbor_mean(pos, actions, counts, ..)  the opt-in neighbourhood mean action (the paper's a_bar_j), float32
    NeighborMean(eng, group, radius)         the same per step of the device rollout loop, one row per agent
    q_sample(q, temperature, seed, step)     the Boltzmann draw over Q rows (csrc/qsample.h): the opt-in exploration
                                             of the Q models; no counterpart in the reference, whose act is greedy
"""
import math

import torch

from . import check, lib
from .abi import ptr, stream


def _dtype(what, **tensors):
    """Refuse a tensor of another dtype before any library call: the kernels read raw bytes."""
    for name, (t, want) in tensors.items():
        if t.dtype != want:
            raise TypeError("%s: %s must be %s, got %s" % (what, name, want, t.dtype))


def mean_action(actions, counts, n_action):
    """actions int32 [B, rowcap], counts int32 [B] -> float64 [B, n_action]: row b is the mean of the one-hot rows
    of its first n = min(counts[b], rowcap) slots (a count above rowcap is capped, as the row-list kernels cap it; a
    negative one reads as 0).  An action outside [0, n_action) is counted in no entry while n stays the divisor; n = 0
    gives a row of NaN.  Any other dtype raises TypeError."""
    _dtype("mean_action", actions=(actions, torch.int32), counts=(counts, torch.int32))
    B, rowcap = actions.shape
    if counts.shape != (B,):
        raise ValueError("mean_action: counts of shape %s for %d rows" % (tuple(counts.shape), B))
    out = torch.empty((B, n_action), dtype=torch.float64, device=actions.device)
    check(lib().mfx_mean_action(ptr(actions.contiguous()), ptr(counts.contiguous()), B, rowcap, n_action, ptr(out),
                                stream()), "mfx_mean_action")
    return out


MEAN_FIELDS = ("group", "neighbors")     # ValueNet.mean_field / ActorCritic.mean_field


def check_mean_field(model, value):
    """The mean_field setter of the models: "group" (the reference's group-wide mean) or "neighbors" (the opt-in
    neighbourhood mean, NeighborMean), the latter only on a mean-field model."""
    if value not in MEAN_FIELDS:
        raise ValueError("mean_field %r (one of %s)" % (value, ", ".join(MEAN_FIELDS)))
    if value != "group" and not getattr(model, "use_mf", getattr(model, "_use_mf", False)):
        raise ValueError("mean_field %r needs a mean-field model (MFQ / MFAC); %s reads no mean action"
                         % (value, type(model).__name__))
    return value


def check_mf_radius(value):
    """The mf_radius setter of the models: an int >= 0."""
    if isinstance(value, bool) or int(value) != value or int(value) < 0:
        raise ValueError("mf_radius must be an integer >= 0, got %r" % (value,))
    return int(value)


def neighbor_mean(pos, actions, counts, n_action, radius, map_w, map_h, out=None):
    """The neighbourhood mean action on compact lists (k_neighbor_mean; the contract of include/magent_amd.h part 4b,
    restated in tests/neighbor_mean_ref.py): pos int32 [B, rowcap, 2] (x, y), actions int32 [B, rowcap], counts int32
    [B] -> float32 [B, rowcap, n_action]; row j < counts[b] is the mean of the one-hot actions of list b's members
    within Chebyshev distance `radius` of member j, itself included, (float)(count / n) computed in float64.  An
    action outside [0, n_action) is counted in no entry while the divisor stays.  Rows at and past the count are left
    as they are (out: the tensor to write into; None: a new one of zeros).  The positions of a list must be distinct
    cells inside the map (not checked).  Any other dtype raises TypeError; 1 <= n_action <= 64, radius >= 0 and a map
    that fits the LDS grid (256 x 256 does, 512 x 512 does not) are the library's refusals."""
    _dtype("neighbor_mean", pos=(pos, torch.int32), actions=(actions, torch.int32), counts=(counts, torch.int32))
    if actions.dim() != 2 or pos.shape != tuple(actions.shape) + (2,) or counts.shape != (actions.shape[0],):
        raise ValueError("neighbor_mean: pos %s, actions %s, counts %s" % tuple(
            tuple(x.shape) for x in (pos, actions, counts)))
    B, rowcap = actions.shape
    if out is None:
        out = torch.zeros((B, rowcap, max(int(n_action), 0)), dtype=torch.float32, device=actions.device)
    else:
        _dtype("neighbor_mean", out=(out, torch.float32))
        if out.shape != (B, rowcap, n_action) or not out.is_contiguous():
            raise ValueError("neighbor_mean: out of shape %s for [%d, %d, %d]" % (tuple(out.shape), B, rowcap, n_action))
    check(lib().mfx_neighbor_mean(ptr(pos.contiguous()), ptr(actions.contiguous()), ptr(counts.contiguous()), B, rowcap,
                                  int(n_action), int(radius), int(map_w), int(map_h), ptr(out), stream()),
          "mfx_neighbor_mean")
    return out


class NeighborMean:
    """The neighbourhood mean action of group `group` of a BattleBatch on the device rollout loop (opt-in):

        eng.rollout_policy_observe();  nm.reset()
        per step:  model.act_rollout(eng, group, prob_rows=nm.rows) ... eng.rollout_policy_step();  nm.update()

    rows: float32 CUDA tensor [E, rowcap, n_action]; after update(), row j < group_num[e] of env e is the mean of the
    one-hot actions the step consumed over the survivors of the group within Chebyshev distance `radius` of survivor
    j (itself included; agents that died in the step count for nobody), and all zero when the env restarted in the
    step or after reset().  Rows at and past group_num keep what they held.  One launch per call on the engine's
    stream; the carried state (the group sizes and episode numbers of the previous call) lives on the device and
    nothing is read back.  Needs minimap_mode (the position comes from the feature row) and rollout_init."""

    def __init__(self, eng, group, radius):
        self.eng, self.group, self.radius = eng, int(group), check_mf_radius(radius)
        self.n_action = int(eng.env.get_action_space(eng.handles[self.group])[0])
        with torch.cuda.stream(eng.torch_stream()):
            self.rows = torch.zeros((eng.n_envs, eng.rowcap, self.n_action), dtype=torch.float32, device="cuda")
            self._state = torch.zeros(2 * eng.n_envs, dtype=torch.int32, device="cuda")

    def matches(self, eng, group, radius):
        """Whether this object serves (eng, group, radius) as the engine is laid out now."""
        return (self.eng is eng and self.group == int(group) and self.radius == int(radius)
                and self.rows.shape[:2] == (eng.n_envs, eng.rowcap))

    def reset(self):
        self.eng._check(self.eng._dll.mfx_neighbor_mean_reset(self.eng.game, self.group, ptr(self.rows),
                                                              ptr(self._state)), "neighbor_mean_reset")

    def update(self):
        self.eng._check(self.eng._dll.mfx_neighbor_mean_rollout(self.eng.game, self.group, self.radius, ptr(self.rows),
                                                                ptr(self._state)), "neighbor_mean_rollout")


def mfq_target(e_q, t_q, rewards, dones, gamma=0.95):
    """target = r + (1 - done) * t_q[argmax e_q] * gamma, float64 [M]; e_q, t_q float32 [M, A], rewards float32 [M]
    (any other dtype raises TypeError); dones: bool/uint8 [M], any non-zero byte is done."""
    _dtype("mfq_target", e_q=(e_q, torch.float32), t_q=(t_q, torch.float32), rewards=(rewards, torch.float32))
    M, A = e_q.shape
    if t_q.shape != (M, A) or rewards.shape != (M,) or dones.shape != (M,):
        raise ValueError("mfq_target: e_q %s, t_q %s, rewards %s, dones %s" % tuple(
            tuple(x.shape) for x in (e_q, t_q, rewards, dones)))
    out = torch.empty(M, dtype=torch.float64, device=e_q.device)
    d = dones.to(torch.uint8).contiguous()
    check(lib().mfx_mfq_target(ptr(e_q.contiguous()), ptr(t_q.contiguous()), ptr(rewards.contiguous()), ptr(d), M, A,
                               gamma, ptr(out), stream()), "mfx_mfq_target")
    return out


def check_temperature(t, what="explore 'boltzmann': the temperature (eps)"):
    """A Boltzmann temperature as a float; ValueError unless it is finite and > 0 (the library refuses it too)."""
    t = float(t)
    if not (math.isfinite(t) and t > 0.0):
        raise ValueError("%s must be finite and > 0, got %r" % (what, t))
    return t


def mfq_target_boltzmann(e_q, t_q, rewards, dones, gamma, temperature, want_w=False):
    """The opt-in Boltzmann mean-field value target (k_mfq_target_soft; the contract of include/magent_amd.h, DESIGN 7m,
    restated in tests/qtarget_ref.py): target = r + (1 - done) * v * gamma, float64 [M], with v the mean of t_q under
    the acting weights of q_sample on e_q (expf((e_q - max e_q) / temperature), its non-finite rule included), summed
    in float64.  e_q, t_q float32 [M, A], 2 <= A <= 32, rewards float32 [M], dones bool / uint8 [M]: the dtype and shape
    refusals of mfq_target.

    temperature: a Python float, finite and > 0 (ValueError otherwise; nothing is launched), or a one-element float32
    CUDA tensor read by the kernel when it runs -- a captured graph follows what is written into it; a value there
    that is not finite and > 0 makes every target of the launch NaN.  want_w: (target, weights float32 [M, A])."""
    _dtype("mfq_target_boltzmann", e_q=(e_q, torch.float32), t_q=(t_q, torch.float32), rewards=(rewards, torch.float32))
    M, A = e_q.shape
    if t_q.shape != (M, A) or rewards.shape != (M,) or dones.shape != (M,):
        raise ValueError("mfq_target_boltzmann: e_q %s, t_q %s, rewards %s, dones %s" % tuple(
            tuple(x.shape) for x in (e_q, t_q, rewards, dones)))
    if not 2 <= A <= 32:
        raise ValueError("mfq_target_boltzmann: 2 <= A <= 32, got %d" % A)
    if isinstance(temperature, torch.Tensor):
        _dtype("mfq_target_boltzmann", temperature=(temperature, torch.float32))
        if temperature.numel() != 1 or not temperature.is_cuda:
            raise ValueError("mfq_target_boltzmann: a tensor temperature is one float32 element on the device")
        T, d_T = 0.0, ptr(temperature)
    else:
        T, d_T = check_temperature(temperature, "mfq_target_boltzmann: the temperature"), None
    out = torch.empty(M, dtype=torch.float64, device=e_q.device)
    w = torch.empty((M, A), dtype=torch.float32, device=e_q.device) if want_w else None
    d = dones.to(torch.uint8).contiguous()
    check(lib().mfx_mfq_target_boltzmann(ptr(e_q.contiguous()), ptr(t_q.contiguous()), ptr(rewards.contiguous()), ptr(d),
                                         M, A, gamma, T, d_T, ptr(out), ptr(w), stream()), "mfx_mfq_target_boltzmann")
    return (out, w) if want_w else out


def q_sample(q, temperature, seed, step, group=0, rows=None, want_w=False):
    """The Boltzmann draw of the Q models' opt-in acting mode on a Q table (k_q_sample; the contract of csrc/qsample.h,
    restated in tests/qsample_ref.py): q float32 [n, A], 2 <= A <= 32 -> actions int32 [n], row i drawn from the
    weights expf((q - max q) / temperature) with the uniform (seed, step, group, rows[i] if rows is given else i); a
    row with a non-finite entry takes its greedy action.  rows: int32 [n] (e.g. e * rowcap + j of a rollout).
    want_w: (actions, weights float32 [n, A]).  A temperature that is not finite and > 0 raises; nothing is launched."""
    _dtype("q_sample", q=(q, torch.float32))
    if rows is not None:
        _dtype("q_sample", rows=(rows, torch.int32))
        if rows.shape != (q.shape[0],):
            raise ValueError("q_sample: rows of shape %s for %d table rows" % (tuple(rows.shape), q.shape[0]))
        rows = rows.contiguous()
    n, A = q.shape
    act = torch.empty(n, dtype=torch.int32, device=q.device)
    w = torch.empty((n, A), dtype=torch.float32, device=q.device) if want_w else None
    check(lib().mfx_q_sample_rows(ptr(q.contiguous()), ptr(rows), n, A, temperature, seed, step, int(group), ptr(w),
                                  ptr(act), stream()), "mfx_q_sample")
    return (act, w) if want_w else act


def mfac_returns(rewards, offsets, values, gamma=0.95, numpy1=True):
    """Per-episode discounted returns, in place on float32 contiguous rewards; offsets int64 [E+1], values float32
    [E] (any other dtype raises TypeError, a non-contiguous rewards or another length ValueError).

    numpy1: the promotion of the reference's NumPy-1 era (keep in float64); False: NEP 50 (float32)."""
    _dtype("mfac_returns", rewards=(rewards, torch.float32), offsets=(offsets, torch.int64),
           values=(values, torch.float32))
    if not rewards.is_contiguous():
        raise ValueError("mfac_returns: rewards must be contiguous (the returns are written in place)")
    if offsets.dim() != 1 or values.dim() != 1 or len(offsets) != len(values) + 1:
        raise ValueError("mfac_returns: %d offsets for %d values (one more is needed)" % (len(offsets), len(values)))
    check(lib().mfx_mfac_returns(ptr(rewards), ptr(offsets.contiguous()), ptr(values.contiguous()), len(values),
                                 gamma, int(bool(numpy1)), stream()), "mfx_mfac_returns")
    return rewards
