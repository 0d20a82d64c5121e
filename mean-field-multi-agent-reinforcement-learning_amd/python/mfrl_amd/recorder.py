"""Watch a few envs of the device rollout loop: record a trace on the device, re-run it on a one-env engine, and let
that engine write the reference's render frames (HIP kernels of csrc/trace_kernels.hip; include/magent_amd.h part 8
states the contract).

A frame lists the step's attack events in shuffle order, which the fused rollout kernels do not emit.  What the loop
gives cheaply is a trace: per step a watched env's action rows and the rows that prove a re-run right.  Every round
starts with eng.reset() + rollout_init, so the trace of one round re-runs the env from its start on the one-env per-call
engine, which records events and writes config.json / video_<n>.txt byte for byte like the reference.  One thing does
run on from round to round: an env's shuffle engine (the attack order's minstd state), which no reset re-seeds.  The
recorder takes its state at attach and the replay seeds the one-env engine with it.

    rec = RolloutRecorder(eng, envs=[0, 17], cap_steps=max_steps)
    eng.rollout_policy_observe()
    rec.attach(map_size, max_steps, placement)     # carry of every watched env, state zeroed
    for every step:
        models[g].act_rollout(eng, g) ...
        eng.rollout_policy_step()
        rec.update()                               # exactly one launch per step, nothing read back
    trace = rec.finish()                           # one synchronise; raises TraceError on the error word
    replay(trace, 0, render_dir="build/render")    # frames of env 0 under build/render/env_0/, or TraceMismatch

One launch per step is enough: a learned policy's step reads the action buffer and never writes it, and the group sizes
of before the step are carried on the device (the header says why).
"""
import ctypes
import os

import numpy as np

from . import check, lib
from .abi import bind, ptr, struct

MAX_ENVS, HEAD, CARRY = 16, 6, 4
VALID, N, EP_BEFORE, EP_AFTER, STEPS = 0, 1, 3, 4, 5          # the head's words
ERRORS = ((1, "a step was not recorded, or was recorded twice (agent_steps moved by something other than the group "
              "sizes carried over: update() must follow every rollout_policy_step exactly once)"),
          (2, "the episode count of a watched env moved by something other than 0 or 1 between two updates"),
          (4, "a group size outside [0, rowcap]"),
          (8, "full: more steps than cap_steps (the later ones were not recorded)"),
          (16, "a watched env index outside [0, n_envs) on the device"))
ROWS = (("actions", np.int32), ("ids", np.int32), ("rewards", np.float32), ("alive", np.uint8))


class TraceError(RuntimeError):
    pass


class TraceMismatch(RuntimeError):
    """The re-run of a watched env differs from its trace."""

    def __init__(self, env, step, group, field, detail=""):
        self.env, self.step, self.group, self.field = env, step, group, field
        RuntimeError.__init__(self, "replay of env %d differs from its trace at step %d, group %s: %s%s"
                              % (env, step, group, field, (" (" + detail + ")") if detail else ""))


_TraceSrc, _TraceDst = struct("mfx_trace_src"), struct("mfx_trace_dst")
DST_NAMES = ("envs", "carry", "head", "actions", "ids", "rewards", "alive", "state", "seeds")
SRC_NAMES = ("group_num", "alive", "stats", "agent_steps", "actions", "ids", "rewards", "rng")
trace_lib = lib                         # (the name the kernel tests reach the library by)


def error_text(word):
    return "; ".join(msg for bit, msg in ERRORS if word & bit) or "error word %d" % word


def check_watch(envs, n_envs, who="--watch"):
    """The watched env indices as a list, or ValueError: 1 to 16 of them, each in [0, n_envs), no duplicate."""
    envs = [int(e) for e in envs]
    if not 1 <= len(envs) <= MAX_ENVS:
        raise ValueError("%s takes 1 to %d envs, got %d" % (who, MAX_ENVS, len(envs)))
    for e in envs:
        if not 0 <= e < n_envs:
            raise ValueError("%s: env %d is outside [0, %d)" % (who, e, n_envs))
    if len(set(envs)) != len(envs):
        raise ValueError("%s: an env is given twice: %s" % (who, envs))
    return envs


def make_trace(envs, rowcap, steps, arrays, map_size, max_steps, placement, final=None):
    """The trace dict from the record arrays (host copies of mfx_trace_dst's head / actions / ids / rewards / alive, at
    least `steps` steps long, and seeds).  Every per-step array is [steps][K]...; placement: the round's, per group."""
    K = len(envs)
    head = np.asarray(arrays["head"]).reshape(-1, K, HEAD)[:steps]
    out = {"envs": np.asarray(envs, np.int32), "rowcap": int(rowcap), "steps": int(steps), "map_size": int(map_size),
           "max_steps": int(max_steps), "placement": [np.asarray(p, np.int32).copy() for p in placement],
           "valid": head[:, :, VALID] != 0, "n": head[:, :, N:N + 2].astype(np.int32),
           "ep_before": head[:, :, EP_BEFORE].copy(), "ep_after": head[:, :, EP_AFTER].copy(),
           "agent_steps": head[:, :, STEPS].copy(), "final": final,
           "seed": np.asarray(arrays["seeds"]).view(np.uint32).reshape(-1)[:K].copy()}
    for name, dt in ROWS:
        out[name] = np.asarray(arrays[name]).view(dt).reshape(-1, K, 2, rowcap)[:steps].copy()
    return out


class RolloutRecorder:
    """The recorder of a BattleBatch's device rollout loop (after rollout_init) for the watched envs `envs` (1 to 16
    indices, unsorted is fine) and at most cap_steps steps per round.  The buffers are allocated once per engine and
    reused across rounds; every launch goes to the engine's stream."""

    def __init__(self, eng, envs, cap_steps):
        if len(eng.handles) != 2:
            raise ValueError("RolloutRecorder: two groups only, got %d" % len(eng.handles))
        if int(cap_steps) < 1:
            raise ValueError("RolloutRecorder: cap_steps must be at least 1")
        self.eng, self.cap_steps = eng, int(cap_steps)
        self.envs = check_watch(envs, eng.n_envs, "RolloutRecorder")
        self._h_envs = (ctypes.c_int32 * len(self.envs))(*self.envs)
        self._L = lib()
        self._bufs = self._src = self._dst = self._shape = self._round = self.trace = None
        self._t = 0

    def _buffer(self, name):            # (the kernel tests put synthetic device arrays behind this)
        return self.eng.rollout_buffer(name)

    def _structs(self):
        import torch
        eng, K = self.eng, len(self.envs)
        E, rc = eng.n_envs, eng.rowcap
        if self._shape != (rc,):
            sizes = (ctypes.c_size_t * 9)()
            check(self._L.mfx_trace_sizes(K, rc, self.cap_steps, sizes), "mfx_trace_sizes")
            with torch.cuda.stream(eng.torch_stream()):
                self._bufs = [torch.zeros((int(n) + 7) // 8, dtype=torch.int64, device="cuda") for n in sizes]
            self._shape = (rc,)
        # (the rollout buffers may move at a rollout_init: their addresses are taken again at every attach)
        self._src = _TraceSrc(*[self._buffer(k) for k in SRC_NAMES], E, len(eng.handles), rc)
        self._dst = _TraceDst(*[ptr(b) for b in self._bufs], self.cap_steps, K)

    def attach(self, map_size, max_steps, placement):
        """After rollout_policy_observe, before the first policy step of the round.  map_size, max_steps and placement
        (per group, as given to rollout_init) go into the trace: the replay starts from them."""
        self._structs()
        self._round = (int(map_size), int(max_steps), [np.asarray(p, np.int32) for p in placement])
        self._t = 0
        check(self._L.mfx_trace_attach(ctypes.byref(self._src), ctypes.byref(self._dst), self._h_envs,
                                       self.eng.stream_handle()), "mfx_trace_attach")

    def update(self):
        """After every rollout_policy_step, exactly once."""
        assert self._round is not None, "RolloutRecorder.update() before attach()"
        check(self._L.mfx_trace_update(ctypes.byref(self._src), ctypes.byref(self._dst), self._t,
                                       self.eng.stream_handle()), "mfx_trace_update")
        self._t += 1

    def _final(self):
        """ids, positions and hp of the watched envs as the round left them (the per-call getters)."""
        import torch
        from .battle import GET_HP, GET_ID, GET_NUM, GET_POS
        eng = self.eng
        E, rc = eng.n_envs, eng.rowcap
        idx = torch.tensor(self.envs, dtype=torch.int64, device="cuda")
        out = {}
        with torch.cuda.stream(eng.torch_stream()):
            for name, what, dt, w in (("n", GET_NUM, torch.int32, 0), ("ids", GET_ID, torch.int32, 1),
                                      ("pos", GET_POS, torch.int32, 2), ("hp", GET_HP, torch.float32, 1)):
                per_group = []
                for g in range(2):
                    buf = torch.empty((E,) if w == 0 else (E, rc, w), dtype=dt, device="cuda")
                    eng.get(g, what, buf, rc)
                    per_group.append(buf.index_select(0, idx).cpu().numpy())
                out[name] = np.stack(per_group, axis=1)              # [K][2]...
        out["ids"], out["hp"] = out["ids"][..., 0], out["hp"][..., 0]
        return out

    def finish(self, final=True):
        """Synchronise once and return the trace: NumPy arrays [steps][K]... (valid, n, ep_before, ep_after,
        agent_steps, actions, ids, rewards, alive), seed [K], envs, rowcap, steps, map_size, max_steps, placement, and -- with
        `final` -- the watched envs' ids, positions and hp after the last step.  Raises TraceError on a non-zero error
        word."""
        import torch
        assert self._round is not None, "RolloutRecorder.finish() before attach()"
        K, rc = len(self.envs), self.eng.rowcap
        T = min(self._t, self.cap_steps)
        with torch.cuda.stream(self.eng.torch_stream()):
            state = self._bufs[7][:2].cpu().numpy()
            if state[1]:
                raise TraceError("RolloutRecorder: %s" % error_text(int(state[1])))
            if int(state[0]) != T:
                raise TraceError("RolloutRecorder: %d steps recorded, %d updates made" % (int(state[0]), T))
            arrays = {"head": self._bufs[2][:T * K * HEAD].cpu().numpy(), "seeds": self._bufs[8].cpu().numpy()}
            for i, (name, dt) in zip((3, 4, 5, 6), ROWS):
                nbytes = T * K * 2 * rc * np.dtype(dt).itemsize
                arrays[name] = self._bufs[i][:(nbytes + 7) // 8].cpu().numpy().view(np.uint8)[:nbytes]
        map_size, max_steps, placement = self._round
        self.trace = make_trace(self.envs, rc, T, arrays, map_size, max_steps, placement,
                                self._final() if final else None)
        return self.trace


# ------------------------------------------------------------------------------------------------------------ replay
def _place(env, handles, placement):
    env.reset()
    for g in range(2):
        env.add_agents(handles[g], method="custom", pos=placement[g])


def _hp(env, handle, n):
    """hp of a group through whichever extra the library has (mfx_battle_get on the engine, the "hp" info on the C
    oracle), or None (the reference shows hp only in the views)."""
    dll = getattr(env._lib, "dll", None)
    if dll is not None and hasattr(dll, "mfx_battle_get"):
        import torch
        from .battle import GET_HP
        buf = torch.empty(max(n, 1), dtype=torch.float32, device="cuda")
        check(dll.mfx_battle_get(env.game, int(handle.value), GET_HP, ptr(buf), max(n, 1)), "mfx_battle_get")
        check(dll.mfx_battle_sync(env.game), "mfx_battle_sync")
        return buf[:n].cpu().numpy()
    try:
        return env._info_array(handle, b"hp", (n,), np.float32)
    except Exception:
        return None


def replay(trace, k, render_dir=None, lib=None, episodes=None):
    """Re-run watched env k (an index into trace["envs"]) on a one-env engine through the per-call API -- the drop-in
    magent.GridWorld on `lib` (a magent.load_library object; default: the product library) -- and compare it with the
    trace bit for bit at every step: group sizes, ids, alive flags, rewards and whether the episode ended.  Any
    difference raises TraceMismatch.  The engine's shuffle engine starts from the state the watched env's had at
    attach (the "seed" config key: all three builds take a minstd state as it is).

    render_dir: frames go to <render_dir>/env_<e>/ (config.json, one video_<n>.txt per episode): render() once after
    every placement, which also turns event recording on, and once after every step.  episodes: stop after that many
    episodes.  When the whole trace was replayed and it holds the round's final state, ids, positions and hp are
    compared with it too.  Returns {"steps", "episodes", "dir"}."""
    import magent
    e = int(trace["envs"][k])
    T, max_steps, placement = trace["steps"], trace["max_steps"], trace["placement"]
    env = magent.GridWorld("battle", map_size=trace["map_size"], lib=lib if lib is not None else magent.load_library())
    if getattr(env._lib, "dll", None) is not None:
        bind(env._lib.dll)                               # (_hp calls mfx_battle_get through it)
    h = env.get_handles()
    out_dir = None
    if render_dir is not None:
        out_dir = os.path.join(render_dir, "env_%d" % e)
        env.set_render_dir(out_dir)
    try:
        env.set_seed(int(trace["seed"][k]))
        _place(env, h, placement)
        if out_dir is not None and T > 0:
            env.render()
        ep_len = n_ep = t = 0
        stopped = False
        for t in range(T):
            if not trace["valid"][t, k]:
                raise TraceMismatch(e, t, "-", "valid", "the record failed a guard on the device")
            n = [int(env.get_num(h[g])) for g in range(2)]
            for g in range(2):
                if n[g] != int(trace["n"][t, k, g]):
                    raise TraceMismatch(e, t, g, "n", "%d != %d" % (n[g], int(trace["n"][t, k, g])))
            for g in range(2):
                env.set_action(h[g], np.ascontiguousarray(trace["actions"][t, k, g, :n[g]], dtype=np.int32))
            done = bool(env.step())
            for g in range(2):
                got = (("ids", np.asarray(env.get_agent_id(h[g]), np.int32)),
                       ("alive", np.asarray(env.get_alive(h[g])).astype(np.uint8)),
                       ("rewards", np.asarray(env.get_reward(h[g]), np.float32)))
                for field, a in got:
                    want = trace[field][t, k, g, :n[g]]
                    if field == "alive":
                        want = (want != 0).astype(np.uint8)
                    if len(a) != n[g] or a.tobytes() != want.tobytes():
                        raise TraceMismatch(e, t, g, field)
            ep_len += 1
            ended = done or ep_len >= max_steps
            if ended != (int(trace["ep_after"][t, k]) == int(trace["ep_before"][t, k]) + 1):
                raise TraceMismatch(e, t, "-", "episode end", "replay %s, done %s, length %d" % (ended, done, ep_len))
            if out_dir is not None:
                env.render()
            env.clear_dead()
            if ended:
                n_ep += 1
                ep_len = 0
                if episodes is not None and n_ep >= episodes:
                    stopped = True                       # (no placement behind it: the final state is not compared)
                    break
                _place(env, h, placement)
                if out_dir is not None and t + 1 < T:
                    env.render()
        played = t + 1 if T else 0
        fin = trace.get("final")
        if fin is not None and played == T and not stopped:
            for g in range(2):
                m = int(env.get_num(h[g]))
                if m != int(fin["n"][k, g]):
                    raise TraceMismatch(e, T, g, "final n", "%d != %d" % (m, int(fin["n"][k, g])))
                if np.asarray(env.get_agent_id(h[g]), np.int32).tobytes() != fin["ids"][k, g, :m].tobytes():
                    raise TraceMismatch(e, T, g, "final ids")
                if np.asarray(env.get_pos(h[g]), np.int32).tobytes() != fin["pos"][k, g, :m].tobytes():
                    raise TraceMismatch(e, T, g, "final positions")
                hp = _hp(env, h[g], m)
                if hp is not None and np.asarray(hp, np.float32).tobytes() != fin["hp"][k, g, :m].tobytes():
                    raise TraceMismatch(e, T, g, "final hp")
        return {"steps": played, "episodes": n_ep, "dir": out_dir}
    finally:
        # the drop-in's resident step server leaves when its engine goes: nothing of the replay outlives this call
        del env
