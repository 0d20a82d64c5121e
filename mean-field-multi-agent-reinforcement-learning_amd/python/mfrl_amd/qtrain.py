"""QTrainHIP: the hand-written HIP minibatch step (csrc/qtrain_kernels.hip) of the reference's Q-network training.

    ValueNet.train / calc_target_q / update   examples/battle_model/algo/base.py:192-279
    DQN.train, MFQ.train (the minibatch loop) examples/battle_model/algo/q_learning.py:42-54, :110-131

The handle owns the eval and target parameters, Adam's moments (four blobs in pack_qnet's layout) and the step count.
``run`` enqueues a whole sequence of minibatches -- rows read straight from the MemoryGroup ring at the sampled
indices, target, masked-MSE loss, backward, Adam, soft update -- in one call with nothing read back; ``grads`` is the
same gradient without the update (the test hook).  f32 throughout; every sum has a fixed order, so equal state and
indices give bitwise equal results.  The contract is in include/magent_amd.h (mfx_qtrain_*), the float64 restatement
in tests/qtrain_ref.py.
"""
import ctypes

import torch

from . import check, lib
from .abi import ptr, stream, struct
from .policy import blob_layout, pack_qnet, unpack_qnet

EVAL, TARGET, ADAM_M, ADAM_V = 0, 1, 2, 3
MAX_BATCH = 4096
TARGET_RULES = {"max": 0, "boltzmann": 1}      # MFX_QTARGET_MAX / MFX_QTARGET_BOLTZMANN
_ERRORS = {1: "a sample index outside [0, nb_entries)", 2: "a replay action outside [0, n_action)"}
_Ring = struct("mfx_qtrain_ring")


class QTrainError(IndexError):
    pass


def supported(view_space, feature_space, num_actions):
    """Shapes the kernels take: the Battle view, feature <= 256, at most 32 actions."""
    return tuple(view_space) == (13, 13, 7) and 1 <= int(feature_space[0]) <= 256 and 1 <= int(num_actions) <= 32


class QTrainHIP:
    def __init__(self, view_space, feature_space, num_actions, use_mf=False, lr=1e-4, betas=(0.9, 0.999), eps=1e-8,
                 tau=0.005, gamma=0.95):
        if not supported(view_space, feature_space, num_actions):
            raise ValueError("QTrainHIP: the HIP training step takes the Battle view (13, 13, 7), feature <= 256 and at "
                             "most 32 actions; got %r, %r, %r" % (tuple(view_space), tuple(feature_space), num_actions))
        self.F, self.A, self.use_mf = int(feature_space[0]), int(num_actions), bool(use_mf)
        self._L = L = lib()
        self.blob_n, self.offsets = blob_layout(self.F, self.A, self.use_mf)
        hdl = ctypes.c_void_p()
        check(L.mfx_qtrain_create(self.F, self.A, int(self.use_mf), ctypes.byref(hdl)), "mfx_qtrain_create")
        self.handle = hdl
        self.target_rule = "max"
        self.set_hyper(lr, betas, eps, tau, gamma)

    def __del__(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self._L.mfx_qtrain_destroy(self.handle)
            self.handle = None

    def set_hyper(self, lr, betas=(0.9, 0.999), eps=1e-8, tau=0.005, gamma=0.95):
        check(self._L.mfx_qtrain_set_hyper(self.handle, lr, betas[0], betas[1], eps, tau, gamma), "mfx_qtrain_set_hyper")

    def set_target(self, rule, temperature=0.1):
        """The rule of the minibatches' target y, for the grads / run calls that follow: "max" (the default: the target
        net's value of the eval net's greedy next action) or "boltzmann" (opt-in, DESIGN 7m: the target net's next-state
        values averaged under the weights expf((q_eval - max q_eval) / temperature), as mf.mfq_target_boltzmann).
        temperature is read only for "boltzmann" and must be finite and > 0 (the library refuses others); a refusal
        leaves the handle as it was."""
        if rule not in TARGET_RULES:
            raise ValueError("QTrainHIP.set_target: rule %r (one of %s)" % (rule, ", ".join(TARGET_RULES)))
        check(self._L.mfx_qtrain_set_target(self.handle, TARGET_RULES[rule], temperature), "mfx_qtrain_set_target")
        self.target_rule = rule

    # ------------------------------------------------------------------ state
    def set_state(self, which, blob):
        """blob: float32 CUDA tensor of blob_n floats in pack_qnet's layout.  Setting EVAL or TARGET keeps the moments."""
        blob = blob.to(device="cuda", dtype=torch.float32).contiguous()
        check(self._L.mfx_qtrain_set_state(self.handle, int(which), ptr(blob), blob.numel(), stream()),
              "mfx_qtrain_set_state")
        blob.record_stream(torch.cuda.current_stream())

    def get_state(self, which):
        out = torch.empty(self.blob_n, dtype=torch.float32, device="cuda")
        check(self._L.mfx_qtrain_get_state(self.handle, int(which), ptr(out), self.blob_n, stream()),
              "mfx_qtrain_get_state")
        return out

    def load(self, eval_net, target_net):
        """Pack both torch QNets into the handle (the moments and the step count stay)."""
        layout = (self.blob_n, self.offsets)
        self.set_state(EVAL, pack_qnet(eval_net, self.F, self.A, self.use_mf, layout))
        self.set_state(TARGET, pack_qnet(target_net, self.F, self.A, self.use_mf, layout))

    def export(self, eval_net, target_net):
        """The handle's eval and target blobs copied into the torch modules' parameters (policy.unpack_qnet)."""
        layout = (self.blob_n, self.offsets)
        unpack_qnet(self.get_state(EVAL), eval_net, self.F, self.A, self.use_mf, layout)
        unpack_qnet(self.get_state(TARGET), target_net, self.F, self.A, self.use_mf, layout)

    def reset_optimizer(self):
        check(self._L.mfx_qtrain_reset_optimizer(self.handle, stream()), "mfx_qtrain_reset_optimizer")

    def step_count(self):
        t = ctypes.c_longlong()
        check(self._L.mfx_qtrain_step_count(self.handle, ctypes.byref(t)), "mfx_qtrain_step_count")
        return t.value

    # ------------------------------------------------------------------ minibatches
    def _ring(self, cols):
        """cols: dict of the ring's column tensors (obs0, feat0, actions i32, rewards f32, terminals / masks bool or
        uint8, prob f32 with the mean field), CUDA and contiguous, all with the same number of rows."""
        want = {"obs0": torch.float32, "feat0": torch.float32, "actions": torch.int32, "rewards": torch.float32,
                "terminals": None, "masks": None}
        if self.use_mf:
            want["prob"] = torch.float32
        r = _Ring()
        for k, dt in want.items():
            t = cols[k]
            assert t.is_cuda and t.is_contiguous(), "QTrainHIP: column %s must be a contiguous CUDA tensor" % k
            assert (t.dtype == dt) if dt is not None else t.element_size() == 1, "QTrainHIP: column %s is %s" % (k, t.dtype)
            setattr(r, k, t.data_ptr())
        r.rows = min(int(cols[k].shape[0]) for k in want)
        assert cols["obs0"][0].numel() == 13 * 13 * 7 and cols["feat0"][0].numel() == self.F
        assert not self.use_mf or cols["prob"][0].numel() == self.A
        return r

    def _idx(self, idx, n, rows):
        idx = idx.to(device="cuda", dtype=torch.int64).contiguous()
        B = int(idx.shape[-1]) if idx.dim() else 0
        if not 1 <= B <= MAX_BATCH:
            raise ValueError("QTrainHIP: a minibatch of %d rows (1..%d)" % (B, MAX_BATCH))
        if not 1 <= int(n) <= rows:
            raise ValueError("QTrainHIP: nb_entries %d outside the ring columns' rows" % int(n))
        return idx, B

    def grads(self, cols, n, idx):
        """(gradient blob, stats (loss, mean q[a])) of the minibatch at idx [B] (int64) over ring rows [0, n).  No
        state changes."""
        ring = self._ring(cols)
        idx, B = self._idx(idx, n, ring.rows)
        g = torch.empty(self.blob_n, dtype=torch.float32, device="cuda")
        stats = torch.zeros(2, dtype=torch.float32, device="cuda")
        check(self._L.mfx_qtrain_grads(self.handle, ctypes.byref(ring), int(n), ptr(idx), B, ptr(g), ptr(stats), stream()),
              "mfx_qtrain_grads")
        idx.record_stream(torch.cuda.current_stream())
        return g, stats

    def run(self, cols, n, idx):
        """The minibatches idx [n_batches][B] (int64), in order, in one call; -> stats [n_batches][2] (loss, mean
        q[a]) on the device.  Nothing synchronises: call check_error() before trusting the result."""
        ring = self._ring(cols)
        if idx.dim() and idx.shape[-1] > 0:
            idx = idx.reshape(-1, idx.shape[-1])
        idx, B = self._idx(idx, n, ring.rows)
        nb = int(idx.shape[0])
        stats = torch.zeros((nb, 2), dtype=torch.float32, device="cuda")
        check(self._L.mfx_qtrain_run(self.handle, ctypes.byref(ring), int(n), ptr(idx), nb, B, ptr(stats), stream()),
              "mfx_qtrain_run")
        idx.record_stream(torch.cuda.current_stream())
        return stats

    def error(self):
        """Synchronise; (code, bad value) of the sticky device error, cleared (0: none)."""
        code, bad = ctypes.c_int(), ctypes.c_longlong()
        check(self._L.mfx_qtrain_error(self.handle, ctypes.byref(code), ctypes.byref(bad), stream()), "mfx_qtrain_error")
        return code.value, bad.value

    def check_error(self):
        code, bad = self.error()
        if code:
            raise QTrainError("QTrainHIP: %s (%d); that minibatch and the ones after it were not applied"
                              % (_ERRORS.get(code, "error %d" % code), bad))
