"""BattleBatch: E independent Battle envs resident in HBM (include/magent_amd.h, mfx_battle_*).

The configuration path is the reference's own (magent.GridWorld serialises the config
through the env_*/gridworld_* ABI); then the env is switched to E instances before its
first reset.  Two ways to step it:

* per call, on device buffers (``observe / set_action / step / get / clear_dead``) -- the
  reference call sequence, batched;
* fused (``rollout_init / rollout_step``) -- one kernel launch per training-loop step
  (obs x G, on-device rush policy, set_action, step, reward, mean action, clear_dead,
  episode restart) for all envs: the throughput path measured by bench.py.
"""
import ctypes

import numpy as np

import magent
from magent.gridworld import GridWorld

from . import check, lib
from .abi import bind, ptr

GET_NUM, GET_REWARD, GET_ID, GET_ALIVE, GET_POS, GET_HP = range(6)


def _nbytes(a):
    """Bytes of a torch tensor or a numpy array."""
    return a.numel() * a.element_size() if hasattr(a, "numel") else a.nbytes


class BattleBatch:
    def __init__(self, map_size, n_envs, config="battle", stream=None):
        L = magent.load_library(lib()._name)
        self.env = GridWorld(config, map_size=map_size, lib=L) if isinstance(config, str) else GridWorld(config, lib=L)
        self._dll = bind(L.dll)             # (a CDLL of its own: the engine's entry points are declared on it too)
        self.handles = self.env.get_handles()
        self.n_envs = n_envs
        self.game = self.env.game
        self._check(self._dll.mfx_battle_set_num_envs(self.game, n_envs), "set_num_envs")
        if stream is not None:
            self.set_stream(stream)

    _check = staticmethod(check)

    def set_stream(self, stream):
        """stream: a torch.cuda.Stream (or a raw hipStream_t as int)."""
        raw = getattr(stream, "cuda_stream", stream)
        self._check(self._dll.mfx_battle_set_stream(self.game, raw), "set_stream")
        self._stream_raw = raw

    def stream_handle(self):
        """The hipStream_t the engine launches on (0: the null stream)."""
        return getattr(self, "_stream_raw", 0) or 0

    def torch_stream(self):
        """The same stream as a torch stream (for torch work that must be ordered with the engine's launches)."""
        import torch
        raw = self.stream_handle()
        if getattr(self, "_torch_stream", (None, None))[0] != raw:
            self._torch_stream = (raw, torch.cuda.ExternalStream(raw) if raw else torch.cuda.default_stream())
        return self._torch_stream[1]

    # ------------------------------------------------------------------ reference call sequence
    def reset(self):
        self.env.reset()

    def add_agents(self, group, pos):
        self.env.add_agents(self.handles[group], method="custom", pos=pos)

    def capacity(self, group):
        c = ctypes.c_int()
        self._check(self._dll.mfx_battle_group_capacity(self.game, group, ctypes.byref(c)), "capacity")
        return c.value

    def observe(self, group, view, feature, rowcap):
        self._check(self._dll.mfx_battle_observe(self.game, group, ptr(view), ptr(feature), rowcap), "observe")

    def set_action(self, group, actions, rowcap):
        self._check(self._dll.mfx_battle_set_action(self.game, group, ptr(actions), rowcap), "set_action")

    def step(self, done=None):
        self._check(self._dll.mfx_battle_step(self.game, ptr(done)), "step")

    def get(self, group, what, out, rowcap):
        self._check(self._dll.mfx_battle_get(self.game, group, what, ptr(out), rowcap), "get")

    def clear_dead(self):
        self._check(self._dll.mfx_battle_clear_dead(self.game), "clear_dead")

    def sync(self):
        self._check(self._dll.mfx_battle_sync(self.game), "sync")

    # ------------------------------------------------------------------ fused rollout
    def rollout_init(self, placement, max_steps=400, eps=0.2, seed=0, stagger=True):
        """placement: list over groups of [(x, y[, dir]), ...] re-applied at every episode start.

        stagger: spread the episode phase over envs (env e's first episode is cut short by
        e*max_steps/E steps), so after max_steps steps the batch holds every phase of an episode."""
        G = len(self.handles)
        n = (ctypes.c_int * G)(*[len(p) for p in placement])
        self._keep = [np.ascontiguousarray(np.asarray(p, dtype=np.int32)[:, :2]) for p in placement]
        xs = [np.ascontiguousarray(a[:, 0]) for a in self._keep]
        ys = [np.ascontiguousarray(a[:, 1]) for a in self._keep]
        self._keep += xs + ys
        P = ctypes.POINTER(ctypes.c_int)
        px = (P * G)(*[a.ctypes.data_as(P) for a in xs])
        py = (P * G)(*[a.ctypes.data_as(P) for a in ys])
        self._check(self._dll.mfx_battle_rollout_init(self.game, n, px, py, max_steps, eps, seed, int(stagger)),
                    "rollout_init")
        rc = ctypes.c_int()
        self._dll.mfx_battle_rollout_rowcap(self.game, ctypes.byref(rc))
        self.rowcap = rc.value

    def rollout_info(self):
        """(persistent grid in workgroups, dynamic LDS bytes per workgroup) of the fused rollout."""
        g, b = ctypes.c_int(), ctypes.c_int()
        self._check(self._dll.mfx_battle_rollout_info(self.game, ctypes.byref(g), ctypes.byref(b)), "rollout_info")
        return g.value, b.value

    def rollout_check(self):
        """Synchronise; raise on a device error word or an error of the large-env queue kernel
        (k_rollout_bigq: a stall, a workgroup outside XCDs 0-7, the hand-off guard)."""
        self._check(self._dll.mfx_battle_rollout_check(self.game), "rollout_check")

    PATHS = ("k_rollout", "k_rollout_obs+k_rollout", "k_observe_items+k_rollout_big", "k_rollout_bigq")

    def rollout_path(self):
        """Name of the kernels rollout_step runs (the path rollout_init / the last re-plan chose)."""
        p = ctypes.c_int()
        self._check(self._dll.mfx_battle_rollout_path(self.game, ctypes.byref(p)), "rollout_path")
        return self.PATHS[p.value]

    def rollout_sum_lanes(self, n_agents):
        """Lanes over which the rollout sums a group's rewards of an env with n_agents agents (the order
        of the episode-return sums; the oracle replay restates it)."""
        p = ctypes.c_int()
        self._check(self._dll.mfx_battle_rollout_sum_lanes(self.game, int(n_agents), ctypes.byref(p)),
                    "rollout_sum_lanes")
        return p.value

    def rollout_substeps(self, n_sub):
        """Consecutive steps of every env per k_rollout launch (results do not depend on it); 0: the engine
        picks per path and batch size (get_substeps reports it)."""
        self._check(self._dll.mfx_battle_rollout_set_substeps(self.game, int(n_sub)), "rollout_set_substeps")

    def get_substeps(self):
        """Steps per launch in force (after rollout_init)."""
        p = ctypes.c_int()
        self._check(self._dll.mfx_battle_rollout_get_substeps(self.game, ctypes.byref(p)), "rollout_get_substeps")
        return p.value

    def rollout_step(self, n_steps=1):
        self._check(self._dll.mfx_battle_rollout_step(self.game, n_steps), "rollout_step")

    # ------------------------------------------------------------------ learned policy in the loop
    # Every plan takes a learned policy except the observation/step pipeline (MFX_ROLLOUT_PIPE=1): large batches
    # of LDS-sized envs step on the fused k_rollout; large envs (256x256 / 4096 agents) and batches of few
    # LDS-sized envs (down to one env) on k_rollout_big + k_observe_items, one step per call on the engine's
    # stream (rollout_policy_path).  rollout_step and the policy steps interleave exactly.
    def rollout_policy_path(self):
        """Name of the kernels rollout_policy_step runs ("k_rollout" or "k_observe_items+k_rollout_big"); None
        when the plan refuses a learned policy (MFX_ROLLOUT_PIPE=1)."""
        p = ctypes.c_int()
        self._check(self._dll.mfx_battle_rollout_policy_path(self.game, ctypes.byref(p)), "rollout_policy_path")
        return self.PATHS[p.value] if p.value >= 0 else None

    def rollout_policy_observe(self):
        """Write every env's observation into the rollout buffers: the first call of a learned-policy loop, and
        needed again before the next rollout_policy_step after rollout_init, rollout_step or any per-call API
        use (the action buffer must follow the current observation).  Supported on every plan but
        MFX_ROLLOUT_PIPE=1 (rollout_policy_path)."""
        self._check(self._dll.mfx_battle_rollout_policy_step(self.game, 2), "rollout_policy_step")

    def rollout_policy_step(self):
        """Act with the rollout's action buffer (a policy's forward on the current observation, e.g.
        mfrl_amd.policy.QNetHIP.act_rollout, or any actions written with rollout_write), step every env, observe
        the new state.  Supported on every plan but MFX_ROLLOUT_PIPE=1 (rollout_policy_path); a
        rollout_policy_observe call must come first after rollout_init, rollout_step or any per-call API use."""
        self._check(self._dll.mfx_battle_rollout_policy_step(self.game, 1), "rollout_policy_step")

    def mean_stride(self):
        """Doubles per [env][group] row of the mean-action buffer (the largest n_action), as the engine laid
        it out (the buffer itself may be larger: device buffers are kept across re-initialisations)."""
        p = ctypes.c_int()
        self._check(self._dll.mfx_battle_rollout_mean_stride(self.game, ctypes.byref(p)), "rollout_mean_stride")
        return p.value

    STORE_SHAPES = tuple("%s per workgroup, %s%s" % (c, g, nt) for c, g in (
        ("4 KiB", "one workgroup per chunk"), ("8 KiB", "one workgroup per chunk"), ("16 KiB", "one workgroup per chunk"),
        ("4 KiB", "persistent grid (8 per CU)")) for nt in ("", ", nt"))       # mfx_store_ceiling shapes 0..7

    def store_ceiling(self, total_bytes, shape, group=0):
        """GB/s of a write-only float4 stream of total_bytes over this batch's view buffer of `group` (wrapping;
        mfx_store_ceiling, shape index into STORE_SHAPES) on the engine's stream.  Overwrites the views: call it
        only after their last use."""
        buf, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self._dll.mfx_battle_rollout_buffer(self.game, b"view", group, ctypes.byref(buf), ctypes.byref(n)),
                    "rollout_buffer")
        ms = ctypes.c_float()
        self._check(self._dll.mfx_store_ceiling(buf, n, int(total_bytes), int(shape), self.stream_handle(),
                                                ctypes.byref(ms)), "store_ceiling")
        return (int(total_bytes) // 4096 * 4096) / (ms.value * 1e-3) / 1e9

    def view_support(self, group):
        """uint8 [view_h * view_w * n_ch] (the view's NHWC order): 1 where group `group`'s observation view can be
        non-zero, 0 where it is always zero (cells outside the view range carry only the minimap channels)."""
        n = int(np.prod(self.env.get_view_space(self.handles[group])))
        mask = np.zeros(n, dtype=np.uint8)
        self._check(self._dll.mfx_battle_view_support(self.game, int(group), ptr(mask), n), "view_support")
        return mask

    def rollout_buffer(self, name, group=0):
        """The device address of rollout buffer `name` (`group`: which group's "view" / "feature").  The buffers may
        move at a rollout_init: take the address again after one."""
        p, nb = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self._dll.mfx_battle_rollout_buffer(self.game, name.encode(), group, ctypes.byref(p),
                                                        ctypes.byref(nb)), "rollout_buffer")
        return p.value

    def rollout_copy(self, name, dst, group=0, nbytes=None):
        """Copy a device rollout buffer into dst (numpy array or torch tensor, host or device)."""
        size = nbytes if nbytes is not None else _nbytes(dst)
        self._check(self._dll.mfx_battle_rollout_copy(self.game, name.encode(), group, ptr(dst), size), "rollout_copy")

    WRITABLE = ("actions",)

    def rollout_write(self, name, src, group=0):
        """Copy src (torch tensor or numpy array, device or host) into a device rollout buffer on the engine's
        stream: the inverse of rollout_copy.  Only "actions" ([E][G][rowcap] int32, the buffer
        rollout_policy_step acts with) is writable."""
        if name not in self.WRITABLE:
            raise ValueError("rollout_write: buffer %r is not writable (only %s)" % (name, ", ".join(self.WRITABLE)))
        self._check(self._dll.mfx_battle_rollout_write(self.game, name.encode(), group, ptr(src), _nbytes(src)),
                    "rollout_write")

    def rollout_copy_at(self, name, dst, offset, group=0, nbytes=None):
        """Copy bytes [offset, offset + nbytes) of a device rollout buffer into dst."""
        size = nbytes if nbytes is not None else _nbytes(dst)
        self._check(self._dll.mfx_battle_rollout_copy_at(self.game, name.encode(), group, offset, ptr(dst), size),
                    "rollout_copy_at")
