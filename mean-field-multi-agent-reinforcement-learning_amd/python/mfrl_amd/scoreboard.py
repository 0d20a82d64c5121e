"""Per-episode outcomes of the device rollout loop, kept on the device (HIP kernels of csrc/score_kernels.hip;
include/magent_amd.h part 7 states the contract).

The rollout restarts a finished env inside its step and keeps only sums, so who won an episode has to be taken at
the step that ends it -- with Runner.run's own rule (algo/tools.py, train=False): kill[i] = max_nums[i] - nums[1 - i],
nums being get_num after the step and before clear_dead (the members of the last step, those that died in it
included); the larger kill wins, equal kills count for both.  Group 0 is "main", group 1 "opponent".

    eng.rollout_policy_observe()
    board.attach()                       # snapshot every env, zero the totals and the log
    for every step:
        models[g].act_rollout(eng, g) ...
        eng.rollout_policy_step()
        board.update()                   # exactly one launch per step, nothing read back
        if step % check_every == 0 and board.reached() == eng.n_envs: break     # one 8-byte readback
    out = board.finish()                 # one synchronise: totals, log, sums; raises on the error word
"""
import ctypes

import numpy as np
import torch

from . import check, lib
from .abi import ptr, struct

RECORD = np.dtype([("len", np.int32), ("nums", np.int32, 2), ("surv", np.int32, 2), ("kill", np.int32, 2),
                   ("winner", np.int32), ("ret", np.float64, 2)])          # mfx_score_record
CARRY = TOTALS = 8                      # int64 words per env
EPISODES, MAIN_WINS, OPPO_WINS, TIES, KILLS, STEPS, DROPPED = 0, 1, 2, 3, 4, 6, 7      # the totals' words
MAIN, OPPONENT, TIE = 0, 1, 2           # a record's winner
ERRORS = ((1, "a step was not scored, or was scored twice (agent_steps moved by something other than the group "
              "sizes carried over: update() must follow every rollout_policy_step exactly once)"),
          (2, "the episode count of an env moved by something other than 0 or 1 between two updates"),
          (4, "a group size outside [0, rowcap]"))


class ScoreError(RuntimeError):
    pass


_ScoreSrc, _ScoreDst = struct("mfx_score_src"), struct("mfx_score_dst")
score_lib = lib                         # (the name the kernel tests reach the library by)


def error_text(word):
    return "; ".join(msg for bit, msg in ERRORS if word & bit) or "error word %d" % word


class RolloutScoreboard:
    """The scorekeeper of a BattleBatch's device rollout loop (after rollout_init).  ep_cap: records kept per env (an
    env's later episodes are counted in the totals and in `dropped`, not logged); target: reached() counts the envs
    that have finished this many episodes since attach().  The buffers are allocated once per engine and reused
    across rounds; every launch goes to the engine's stream."""

    def __init__(self, eng, ep_cap=4, target=1):
        if len(eng.handles) != 2:
            raise ValueError("RolloutScoreboard: two groups only (main and opponent), got %d" % len(eng.handles))
        self.eng, self.ep_cap, self.target = eng, int(ep_cap), int(target)
        self._L = lib()
        self._bufs = self._src = self._dst = None
        self._shape = None

    def _structs(self):
        eng = self.eng
        E, rc = eng.n_envs, eng.rowcap
        if self._shape != (E, self.ep_cap):
            sizes = (ctypes.c_size_t * 5)()
            check(self._L.mfx_score_sizes(E, self.ep_cap, sizes), "mfx_score_sizes")
            with torch.cuda.stream(eng.torch_stream()):
                self._bufs = [torch.zeros(max(int(n), 8) // 8, dtype=torch.int64, device="cuda") for n in sizes]
            self._shape = (E, self.ep_cap)
        # (the rollout buffers may move at a rollout_init: their addresses are taken again at every attach)
        self._src = _ScoreSrc(*[eng.rollout_buffer(k) for k in ("group_num", "alive", "stats", "agent_steps")], E,
                              len(eng.handles), rc)
        self._dst = _ScoreDst(*[ptr(b) for b in self._bufs], self.ep_cap, self.target)

    def attach(self):
        """After rollout_policy_observe, before the first policy step of the round."""
        self._structs()
        check(self._L.mfx_score_attach(ctypes.byref(self._src), ctypes.byref(self._dst), self.eng.stream_handle()),
              "mfx_score_attach")

    def update(self):
        """After every rollout_policy_step, exactly once."""
        assert self._src is not None, "RolloutScoreboard.update() before attach()"
        check(self._L.mfx_score_update(ctypes.byref(self._src), ctypes.byref(self._dst), self.eng.stream_handle()),
              "mfx_score_update")

    def reached(self):
        """Envs that have finished `target` episodes since attach(): an 8-byte readback behind the engine's stream."""
        with torch.cuda.stream(self.eng.torch_stream()):
            return int(self._bufs[4][:1].cpu().item())

    def finish(self):
        """Synchronise once and return the outcome: per-env `totals` (int64 [E][8]: episodes, main wins, opponent
        wins, ties, kills of main and of opponent, steps of the finished episodes, dropped records), `log` (RECORD
        [E][ep_cap]; the first min(episodes, ep_cap) of an env are filled), and the totals summed over envs
        (episodes, main_wins, oppo_wins, ties, kills, steps, dropped), `reached`.  Raises ScoreError on a non-zero
        error word."""
        assert self._src is not None, "RolloutScoreboard.finish() before attach()"
        E = self.eng.n_envs
        with torch.cuda.stream(self.eng.torch_stream()):
            host = [b.cpu().numpy() for b in self._bufs]
        state = host[4][:2]
        if state[1]:
            raise ScoreError("RolloutScoreboard: %s" % error_text(int(state[1])))
        t = host[2][:E * TOTALS].reshape(E, TOTALS).copy()
        log = host[3].view(np.uint8)[:E * self.ep_cap * RECORD.itemsize].view(RECORD).reshape(E, self.ep_cap).copy()
        out = {"totals": t, "log": log, "reached": int(state[0]), "error": 0}
        for k, i in (("episodes", EPISODES), ("main_wins", MAIN_WINS), ("oppo_wins", OPPO_WINS), ("ties", TIES),
                     ("steps", STEPS), ("dropped", DROPPED)):
            out[k] = int(t[:, i].sum())
        out["kills"] = [int(t[:, KILLS].sum()), int(t[:, KILLS + 1].sum())]
        return out
