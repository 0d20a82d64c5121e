"""ACTrainHIP: the hand-written HIP training step (csrc/actrain_kernels.hip) of the reference's actor-critic models.

    ActorCritic.train / MFAC.train   examples/battle_model/algo/ac.py (the loss of :100-127 / :278-303, one Adam step)

The handle owns the parameters and Adam's moments (three blobs in pack_acnet's layout) and the step count.  ``step``
enqueues one gradient of pg + value_coef * vf + ent_coef * neg_entropy over n contiguous rows, read where they lie,
and one Adam step, in one call with nothing read back; ``grads`` is the same gradient without the update (the test
hook, and ActorCritic.train_rollout(step=False)).  f32 throughout; every sum has a fixed order given (n, chunk_rows,
shape), so equal state and rows give bitwise equal results.  The contract is in include/magent_amd.h (mfx_actrain_*),
the float64 restatement in tests/actrain_ref.py.
"""
import ctypes

import numpy as np
import torch

from . import check, lib
from .abi import ptr, stream, struct
from .policy import acnet_layout, pack_acnet, unpack_acnet

PARAMS, ADAM_M, ADAM_V = 0, 1, 2
_ERRORS = {1: "an action outside [0, n_action)"}
_Rows = struct("mfx_actrain_rows")


class ACTrainError(IndexError):
    pass


def supported(view_space, feature_space, num_actions):
    """Shapes the kernels take (mfx_acnet_create's): views of at most 4096 floats, feature <= 256, 2..32 actions."""
    return (1 <= int(np.prod(view_space)) <= 4096 and 1 <= int(feature_space[0]) <= 256 and
            2 <= int(num_actions) <= 32)


class ACTrainHIP:
    def __init__(self, view_space, feature_space, num_actions, use_mf=False, lr=1e-4, betas=(0.9, 0.999), eps=1e-8,
                 value_coef=0.1, ent_coef=0.08, chunk_rows=None):
        if not supported(view_space, feature_space, num_actions):
            raise ValueError("ACTrainHIP: the HIP training step takes views of at most 4096 floats, feature <= 256 and "
                             "2..32 actions; got %r, %r, %r" % (tuple(view_space), tuple(feature_space), num_actions))
        self.V, self.F, self.A = int(np.prod(view_space)), int(feature_space[0]), int(num_actions)
        self.use_mf = bool(use_mf)
        self._L = L = lib()
        self.blob_n, self.offsets = acnet_layout(self.V, self.F, self.A, self.use_mf)
        hdl = ctypes.c_void_p()
        check(L.mfx_actrain_create(self.V, self.F, self.A, int(self.use_mf), ctypes.byref(hdl)), "mfx_actrain_create")
        self.handle = hdl
        self._support = None
        self.set_hyper(lr, betas, eps, value_coef, ent_coef)
        if chunk_rows:
            self.set_chunk_rows(chunk_rows)

    def __del__(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self._L.mfx_actrain_destroy(self.handle)
            self.handle = None

    def set_hyper(self, lr, betas=(0.9, 0.999), eps=1e-8, value_coef=0.1, ent_coef=0.08):
        check(self._L.mfx_actrain_set_hyper(self.handle, lr, betas[0], betas[1], eps, value_coef, ent_coef),
              "mfx_actrain_set_hyper")

    def set_chunk_rows(self, chunk_rows):
        """Rows per chunk of kept activations (0 / None: the default, 12288)."""
        check(self._L.mfx_actrain_set_chunk_rows(self.handle, int(chunk_rows or 0)), "mfx_actrain_set_chunk_rows")

    # ------------------------------------------------------------------ state
    def set_state(self, which, blob):
        """blob: float32 CUDA tensor of blob_n floats in pack_acnet's layout.  Setting PARAMS keeps the moments."""
        blob = blob.to(device="cuda", dtype=torch.float32).contiguous()
        check(self._L.mfx_actrain_set_state(self.handle, int(which), ptr(blob), blob.numel(), stream()),
              "mfx_actrain_set_state")
        blob.record_stream(torch.cuda.current_stream())

    def get_state(self, which):
        out = torch.empty(self.blob_n, dtype=torch.float32, device="cuda")
        check(self._L.mfx_actrain_get_state(self.handle, int(which), ptr(out), self.blob_n, stream()),
              "mfx_actrain_get_state")
        return out

    def load(self, net):
        """Pack the torch ACNet into the handle (the moments and the step count stay)."""
        self.set_state(PARAMS, pack_acnet(net, self.V, self.F, self.A, self.use_mf, (self.blob_n, self.offsets)))

    def export(self, net):
        """The handle's parameters copied into the torch module's (policy.unpack_acnet); -> the blob."""
        blob = self.get_state(PARAMS)
        unpack_acnet(blob, net, self.V, self.F, self.A, self.use_mf, (self.blob_n, self.offsets))
        return blob

    def reset_optimizer(self):
        check(self._L.mfx_actrain_reset_optimizer(self.handle, stream()), "mfx_actrain_reset_optimizer")

    def step_count(self):
        t = ctypes.c_longlong()
        check(self._L.mfx_actrain_step_count(self.handle, ctypes.byref(t)), "mfx_actrain_step_count")
        return t.value

    def set_input_support(self, mask):
        """mask: uint8/bool [V], 1 where the view can be non-zero, or None for the dense order (the meaning and the
        caller's contract of ACNetHIP.set_input_support).  Waits for the current stream."""
        if mask is None:
            if self._support is not None:
                check(self._L.mfx_actrain_set_input_support(self.handle, None, 0, stream()),
                      "mfx_actrain_set_input_support")
            self._support = None
            return self
        m = np.ascontiguousarray(np.asarray(mask, dtype=np.uint8).reshape(-1))
        if self._support is None or not np.array_equal(self._support, m):
            check(self._L.mfx_actrain_set_input_support(self.handle, ptr(m), int(m.size), stream()),
                  "mfx_actrain_set_input_support")
            self._support = m.copy()
        return self

    # ------------------------------------------------------------------ the step
    def _rows(self, cols, n):
        """cols: dict of column tensors (obs [.., V], feat [.., F], act i32, ret f32, prob [.., A] with the mean
        field), CUDA and contiguous, at least n rows each; an optional "adv" column is grads' / step's."""
        want = {"obs": (torch.float32, self.V), "feat": (torch.float32, self.F), "act": (torch.int32, 1),
                "ret": (torch.float32, 1)}
        if self.use_mf:
            want["prob"] = (torch.float32, self.A)
        n = int(n)
        if n < 1:
            raise ValueError("ACTrainHIP: %d rows (at least 1)" % n)
        r = _Rows()
        for k, (dt, width) in want.items():
            t = cols[k]
            assert t.is_cuda and t.is_contiguous(), "ACTrainHIP: column %s must be a contiguous CUDA tensor" % k
            assert t.dtype == dt, "ACTrainHIP: column %s is %s" % (k, t.dtype)
            assert t.shape[0] >= n and t[0].numel() == width, "ACTrainHIP: column %s has shape %r" % (k, tuple(t.shape))
            setattr(r, k, t.data_ptr())
        return r, n

    def _set_advantage(self, cols, n):
        """cols.get("adv"): the float32 advantage column of the policy term (n rows; ActorCritic.advantage = "gae"), or
        None for the default ret - v.  Set on every call, so a handle never keeps a column of an earlier one."""
        adv = cols.get("adv")
        if adv is not None:
            assert adv.is_cuda and adv.is_contiguous() and adv.dtype == torch.float32 and adv.dim() == 1 and \
                adv.shape[0] >= n, "ACTrainHIP: column adv must be a contiguous float32 CUDA vector of at least n rows"
        check(self._L.mfx_actrain_set_advantage(self.handle, ptr(adv)), "mfx_actrain_set_advantage")

    def _set_ppo(self, cols, n, clip):
        """cols.get("logp_old") with clip: the float32 column of the behaviour log-probabilities (n rows;
        ActorCritic.objective = "ppo", replay.policy_logp) -- the policy term becomes PPO's clipped surrogate (the
        contract of mfx_actrain_set_ppo) -- or None for the default.  cols.get("logp_new"): an optional float32 output
        column, the rows' current log-probabilities.  Set on every call, like the advantage column."""
        old, new = cols.get("logp_old"), cols.get("logp_new")
        if old is None:
            if clip is not None or new is not None:
                raise ValueError("ACTrainHIP: clip / column logp_new belong to column logp_old: give that too")
            check(self._L.mfx_actrain_set_ppo(self.handle, None, 0.0, None), "mfx_actrain_set_ppo")
            return
        if clip is None:
            raise ValueError("ACTrainHIP: column logp_old needs clip=")
        for k, t in (("logp_old", old), ("logp_new", new)):
            assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.dim() == 1 and
                                 t.shape[0] >= n), \
                "ACTrainHIP: column %s must be a contiguous float32 CUDA vector of at least n rows" % k
        check(self._L.mfx_actrain_set_ppo(self.handle, ptr(old), float(clip), ptr(new)), "mfx_actrain_set_ppo")

    def ppo_stats(self):
        """(clip_frac, approx_kl) of the last grads / step call with a logp_old column: a float32 CUDA tensor of 2, copied
        on the current stream; nothing synchronises."""
        out = torch.empty(2, dtype=torch.float32, device="cuda")
        check(self._L.mfx_actrain_ppo_stats(self.handle, ptr(out), stream()), "mfx_actrain_ppo_stats")
        return out

    def grads(self, cols, n, clip=None):
        """(gradient blob, stats (pg_loss, vf_loss, ent_loss, mean value)) of rows [0, n).  No state changes.
        clip: with cols["logp_old"], the PPO head's clip range (_set_ppo)."""
        rows, n = self._rows(cols, n)
        self._set_advantage(cols, n)
        self._set_ppo(cols, n, clip)
        g = torch.empty(self.blob_n, dtype=torch.float32, device="cuda")
        stats = torch.zeros(4, dtype=torch.float32, device="cuda")
        check(self._L.mfx_actrain_grads(self.handle, ctypes.byref(rows), n, ptr(g), ptr(stats), stream()),
              "mfx_actrain_grads")
        return g, stats

    def step(self, cols, n, clip=None):
        """One gradient over rows [0, n) and one Adam step; -> the stats on the device.  Nothing synchronises: call
        check_error() before trusting the result.  clip: as grads'.  A minibatch is rows [a, b) passed as cols[k][a:b]
        with n = b - a: the columns are read from their first row, no gather is made."""
        rows, n = self._rows(cols, n)
        self._set_advantage(cols, n)
        self._set_ppo(cols, n, clip)
        stats = torch.zeros(4, dtype=torch.float32, device="cuda")
        check(self._L.mfx_actrain_step(self.handle, ctypes.byref(rows), n, ptr(stats), stream()), "mfx_actrain_step")
        return stats

    def error(self):
        """Synchronise; (code, bad value) of the sticky device error, cleared (0: none)."""
        code, bad = ctypes.c_int(), ctypes.c_longlong()
        check(self._L.mfx_actrain_error(self.handle, ctypes.byref(code), ctypes.byref(bad), stream()),
              "mfx_actrain_error")
        return code.value, bad.value

    def check_error(self):
        code, bad = self.error()
        if code:
            raise ACTrainError("ACTrainHIP: %s (%d); the step was not applied" % (_ERRORS.get(code, "error %d" % code), bad))
