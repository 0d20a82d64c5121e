"""A learned policy's rollout steps on the large-env plans (mfx_battle_rollout_policy_step on every HBM plan:
k_rollout_big<ext> + k_observe_items on the engine's stream): large envs (state in HBM, clear_dead renumbers the
slots), batches of few LDS-sized envs (the env staged in LDS for its step; rollout_step's own form is the queue
kernel, pipelined for few envs), and both interleaved with rollout_step.

Every test runs in lockstep with one CPU oracle env per batch env: the oracle is stepped with the device's actions
(scripted ones written with rollout_write, a QNet's through act_rollout, or the rush policy's as a twin engine
recorded them); views, features, rewards and mean actions are compared bit for bit on the live rows, and
former_act_prob is zero after a restart under the policy form.
"""
import math
import re

import numpy as np
import pytest

import battle_driver as bd
import common

gpu = pytest.mark.gpu
VF, F, NA = 13 * 13 * 7, 34, 21
POLICY_PATH = "k_observe_items+k_rollout_big"


def interleaved_positions(map_size, n_side):
    """Both groups in one dense block around the map centre, group 0 on its even columns and group 1 on its odd
    ones: every agent has six enemy cells in attack range from the first step."""
    rows = max(r for r in range(1, int(math.sqrt(2 * n_side)) + 1) if n_side % r == 0)
    cols = n_side // rows
    x0, y0 = map_size // 2 - cols, map_size // 2 - rows // 2
    assert x0 >= 1 and y0 >= 1 and x0 + 2 * cols < map_size - 1 and y0 + rows < map_size - 1
    return [[[x0 + 2 * c + g, y0 + r, 0] for c in range(cols) for r in range(rows)] for g in range(2)]


def scripted_actions(rng, E, rc):
    """[E][2][rowcap] actions uniform over the 21 ids."""
    return rng.integers(0, NA, size=(E, 2, rc), dtype=np.int32)


class Lockstep:
    """One oracle env per batch env, stepped with the device's actions and compared with the rollout buffers."""

    def __init__(self, eng, map_size, placement, max_steps, stagger):
        self.eng, self.placement, self.max_steps = eng, placement, max_steps
        E = eng.n_envs
        self.envs = []
        for e in range(E):
            env, h = common.battle_env(common.ORACLE_LIB, map_size)
            self._reset(env, h)
            self.envs.append([env, h, e * max_steps // E if stagger else 0])
        self.restarts = [0] * E                    # restarts of env e so far
        self.done_restarts = 0                     # of them, by the oracle's done
        self.lost = [[False, False] for _ in range(E)]     # before the first restart: a death in group g
        self.relisted = [False] * E                #   and clear_dead changed a group's list (not just its tail)
        self.obs = None

    def _reset(self, env, h):
        env.reset()
        for g, pos in enumerate(self.placement):
            env.add_agents(h[g], method="custom", pos=pos)

    def n(self, e, g):
        env, h, _ = self.envs[e]
        return len(env.get_agent_id(h[g]))

    def grab(self):
        import torch
        eng = self.eng
        E, rc = eng.n_envs, eng.rowcap
        out = {}
        for g in range(2):
            out["view%d" % g] = torch.empty((E, rc, VF), dtype=torch.float32, device="cuda")
            out["feat%d" % g] = torch.empty((E, rc, F), dtype=torch.float32, device="cuda")
            eng.rollout_copy("view", out["view%d" % g], group=g)
            eng.rollout_copy("feature", out["feat%d" % g], group=g)
        out["mean"] = torch.empty((E, 2, NA), dtype=torch.float64, device="cuda")
        out["rew"] = torch.empty((E, 2, rc), dtype=torch.float32, device="cuda")
        out["act"] = torch.empty((E, 2, rc), dtype=torch.int32, device="cuda")
        eng.rollout_copy("mean_action", out["mean"])
        eng.rollout_copy("rewards", out["rew"])
        eng.rollout_copy("actions", out["act"])
        eng.sync()
        return out

    def check_obs(self, out, tag):
        """The observation in the rollout buffers is the oracle's current one."""
        for e, (env, h, _) in enumerate(self.envs):
            for g in range(2):
                v, f = env.get_observation(h[g])
                n = len(v)
                assert out["view%d" % g][e, :n].cpu().numpy().tobytes() == v.reshape(n, VF).tobytes(), (tag, e, g, "view")
                assert out["feat%d" % g][e, :n].cpu().numpy().tobytes() == f.tobytes(), (tag, e, g, "feature")

    def follow(self, actn, out, policy, tag, next_obs=True):
        """The device stepped every env with actn [E][2][rowcap] (out = grab() after the step): the same on the
        oracles.  policy: the step was a rollout_policy_step (the mean action is zeroed at a restart, and with
        next_obs the buffers hold the observation after the step); else a rollout_step."""
        rew, mean = out["rew"].cpu().numpy(), out["mean"].cpu().numpy()
        self.n_prev = [[self.n(e, g) for g in range(2)] for e in range(len(self.envs))]
        for e, st in enumerate(self.envs):
            env, h, _ = st
            acts = [np.ascontiguousarray(actn[e, g, :self.n(e, g)]) for g in range(2)]
            for g in range(2):
                env.set_action(h[g], acts[g])
            done = env.step()
            for g in range(2):
                rw = env.get_reward(h[g])
                assert rew[e, g, :len(rw)].tobytes() == rw.tobytes(), (tag, e, g, "reward")
            before = [env.get_agent_id(h[g]).copy() for g in range(2)]
            alive = [env.get_alive(h[g]).copy() for g in range(2)]
            env.clear_dead()
            if not self.restarts[e]:
                for g in range(2):
                    after = env.get_agent_id(h[g])
                    self.lost[e][g] |= not alive[g].all()
                    self.relisted[e] |= not np.array_equal(before[g][:len(after)], after)
            st[2] += 1
            restart = bool(done) or st[2] >= self.max_steps
            for g in range(2):
                n = len(acts[g])
                want = np.bincount(acts[g], minlength=NA) / n if n else np.full(NA, np.nan)
                if restart and policy:
                    assert not mean[e, g].any(), (tag, e, g, "mean reset")       # former_act_prob = 0 again
                else:
                    assert np.array_equal(mean[e, g], want, equal_nan=True), (tag, e, g, "mean")
            if restart:
                st[2] = 0
                self.restarts[e] += 1
                self.done_restarts += bool(done)
                self._reset(env, h)
        if next_obs:
            self.check_obs(out, tag)
            self.n_prev = [[self.n(e, g) for g in range(2)] for e in range(len(self.envs))]


def _engine(map_size, E, placement, max_steps, stagger, seed=3, eps=0.2):
    import torch
    from mfrl_amd.battle import BattleBatch
    eng = BattleBatch(map_size, E, stream=torch.cuda.current_stream())
    eng.rollout_init(placement, max_steps=max_steps, eps=eps, seed=seed, stagger=stagger)
    return eng


def _scripted_run(eng, lock, steps, seed):
    """observe, then `steps` policy steps with seeded uniform actions written with rollout_write."""
    import torch
    rng = np.random.default_rng(seed)
    E, rc = eng.n_envs, eng.rowcap
    eng.rollout_policy_observe()
    lock.check_obs(lock.grab(), "observe")
    for t in range(steps):
        actn = scripted_actions(rng, E, rc)
        eng.rollout_write("actions", torch.from_numpy(actn).cuda())
        eng.rollout_policy_step()
        out = lock.grab()
        assert np.array_equal(out["act"].cpu().numpy(), actn), (t, "the step left the action buffer as written")
        lock.follow(actn, out, True, t)


@gpu
@pytest.mark.parametrize("map_size,n_side,E", [(200, 1250, 2), (256, 2048, 2)])
def test_scripted_actions_large_envs(map_size, n_side, E):
    """Large envs (state in HBM, renumbering clear_dead; 256x256 has large-map bands) under scripted actions, every
    env restarting twice.  Input condition, on the oracle alone: before its first restart every env loses an
    agent of each group and clear_dead changes a group list, so the renumbering moves slots."""
    max_steps = 12
    placement = interleaved_positions(map_size, n_side)
    eng = _engine(map_size, E, placement, max_steps, False)
    assert eng.rollout_path() == "k_rollout_bigq"
    assert eng.rollout_policy_path() == POLICY_PATH
    lock = Lockstep(eng, map_size, placement, max_steps, False)
    _scripted_run(eng, lock, 2 * max_steps + 1, seed=11)
    eng.rollout_check()
    assert min(lock.restarts) >= 2
    assert all(a and b for a, b in lock.lost) and all(lock.relisted), (lock.lost, lock.relisted)


@gpu
def test_qnet_in_the_loop_large_envs():
    """Two mean-field QNets through act_rollout on 200x200 envs: the device's actions are the torch module's
    argmax on the device's own observation wherever the top two Q values are more than 1e-5 apart, then the
    oracle comparison."""
    import torch
    from mfrl_amd.algo.nets import QNet
    from mfrl_amd.policy import QNetHIP
    map_size, n_side, E, T = 200, 1250, 2, 6
    placement = list(bd.block_positions(map_size, n_side))
    eng = _engine(map_size, E, placement, 400, False)
    assert eng.rollout_policy_path() == POLICY_PATH
    nets = []
    for seed in (21, 22):
        torch.manual_seed(seed)
        net = QNet((13, 13, 7), (F,), NA, True).cuda()
        with torch.no_grad():
            for p in net.parameters():
                p.add_(0.05 * torch.randn_like(p))
        nets.append(net)
    pols = [QNetHIP((13, 13, 7), (F,), NA, True).load(n) for n in nets]
    lock = Lockstep(eng, map_size, placement, 400, False)
    eng.rollout_policy_observe()
    obs = lock.grab()
    lock.check_obs(obs, "observe")
    checked = 0
    for t in range(T):
        for g in range(2):
            pols[g].act_rollout(eng, g)
        act = torch.empty((E, 2, eng.rowcap), dtype=torch.int32, device="cuda")
        eng.rollout_copy("actions", act)
        eng.sync()
        actn = act.cpu().numpy()
        for g in range(2):
            for e in range(E):
                n = lock.n(e, g)
                prob = obs["mean"][e, g].float().expand(n, NA)
                with torch.no_grad():
                    qv = nets[g](obs["view%d" % g][e, :n].reshape(n, 13, 13, 7), obs["feat%d" % g][e, :n], prob)
                top2 = torch.topk(qv, 2, dim=1).values
                clear = ((top2[:, 0] - top2[:, 1]) > 1e-5).cpu().numpy()
                want = torch.argmax(qv, 1).cpu().numpy()
                assert np.array_equal(actn[e, g, :n][clear], want[clear]), (t, e, g)
                checked += int(clear.sum())
        eng.rollout_policy_step()
        obs = lock.grab()
        lock.follow(actn, obs, True, t)
    eng.rollout_check()
    assert checked >= 1000


@gpu
@pytest.mark.parametrize("map_size,n_side,E", [(40, 64, 1), (64, 128, 8)])
def test_scripted_actions_few_envs(map_size, n_side, E):
    """The few-env plans with no env overrides (the single 40x40 env; 8 envs of 64x64, whose rollout_step is the
    pipelined stepper): the policy step stages each env in LDS.  Restarts by the cap, and by done where the
    oracle reaches one.  On the 8-env batch one ACNetHIP.act_rollout step shows the actor-critic forward takes
    these buffers: its actions repeat at the same seed and step.  Then three rollout_step(1) launches (followed on
    the oracle with the recorded rush actions), an observe and one more policy step."""
    import torch
    max_steps = 12
    placement = interleaved_positions(map_size, n_side)
    eng = _engine(map_size, E, placement, max_steps, False)
    assert eng.rollout_path() == "k_rollout_bigq"
    assert eng.rollout_policy_path() == POLICY_PATH
    lock = Lockstep(eng, map_size, placement, max_steps, False)
    import magent
    with pytest.raises(magent.EngineError, match="observe first"):       # no observation yet: mode 1 is refused
        eng.rollout_policy_step()
    _scripted_run(eng, lock, 2 * max_steps + 1, seed=12)
    assert min(lock.restarts) >= 2
    if E == 8:
        from mfrl_amd.algo.nets import ACNet
        from mfrl_amd.policy import ACNetHIP
        torch.manual_seed(5)
        net = ACNet((13, 13, 7), (F,), NA, use_mf=False).cuda()
        pol = ACNetHIP((13, 13, 7), (F,), NA, False).load(net)
        got = []
        for _ in range(2):
            eng.rollout_write("actions", torch.full((E, 2, eng.rowcap), -1, dtype=torch.int32, device="cuda"))
            for g in range(2):
                pol.act_rollout(eng, g, 9, 0)
            got.append(lock.grab()["act"].cpu().numpy())
        assert np.array_equal(got[0], got[1])
        for e in range(E):
            for g in range(2):
                a = got[0][e, g, :lock.n(e, g)]
                assert ((a >= 0) & (a < NA)).all(), (e, g)
        eng.rollout_policy_step()
        lock.follow(got[0], lock.grab(), True, "acnet")
    # and back: rollout_step's own form here (the pipelined stepper keeps the env in LDS inside a launch) re-seeds
    # after the policy steps and leaves the state in HBM for the next observe
    for t in range(3):
        eng.rollout_step(1)
        out = lock.grab()
        lock.follow(out["act"].cpu().numpy(), out, False, ("rush", t), next_obs=False)
    eng.rollout_policy_observe()
    lock.check_obs(lock.grab(), "observe after rollout_step")
    actn = scripted_actions(np.random.default_rng(14), E, eng.rowcap)
    eng.rollout_write("actions", torch.from_numpy(actn).cuda())
    eng.rollout_policy_step()
    lock.follow(actn, lock.grab(), True, "policy after rollout_step")
    eng.rollout_check()


@gpu
def test_policy_steps_interleave_with_rollout_step():
    """rollout_step (the queue kernel, 5 steps per launch) and the policy form in turn on three staggered 200x200
    envs: 5 rush steps, observe + 4 policy steps, 7 rush steps, observe + 3 policy steps.  The oracle follows every
    step with the device's recorded actions; the rush steps' actions (and rewards and mean actions) are read from
    a twin engine on rollout_step(1) launches, which takes the same policy steps; after every segment the twin's
    buffers equal the first engine's."""
    import torch
    map_size, n_side, E, max_steps = 200, 1250, 3, 9
    placement = list(bd.block_positions(map_size, n_side))
    eng, twin = [_engine(map_size, E, placement, max_steps, True) for _ in range(2)]
    eng.rollout_substeps(5)
    twin.rollout_substeps(1)
    assert eng.rollout_path() == twin.rollout_path() == "k_rollout_bigq"
    assert eng.rollout_policy_path() == POLICY_PATH
    lock = Lockstep(eng, map_size, placement, max_steps, True)
    rng = np.random.default_rng(13)
    rc = eng.rowcap

    def same_buffers(tag):
        """Both engines hold the same rows: the observation rows of the agents the last launch observed, the
        action / reward rows of those that took the last step."""
        a, b = lock.grab(), Lockstep.grab(_Grab(twin))
        assert np.array_equal(a["mean"].cpu().numpy(), b["mean"].cpu().numpy(), equal_nan=True), (tag, "mean")
        for e in range(E):
            for g in range(2):
                n = lock.n_prev[e][g]
                for key in ("view%d" % g, "feat%d" % g):
                    assert torch.equal(a[key][e, :n], b[key][e, :n]), (tag, e, g, key)
                for key in ("act", "rew"):
                    assert torch.equal(a[key][e, g, :n], b[key][e, g, :n]), (tag, e, g, key)

    t = 0
    for rush, pol in ((5, 4), (7, 3)):
        eng.rollout_step(rush)
        for _ in range(rush):
            twin.rollout_step(1)
            out = Lockstep.grab(_Grab(twin))
            lock.follow(out["act"].cpu().numpy(), out, False, ("rush", t), next_obs=False)
            t += 1
        eng.rollout_check()
        twin.rollout_check()
        same_buffers(("rush", t))
        eng.rollout_policy_observe()
        twin.rollout_policy_observe()
        lock.check_obs(lock.grab(), ("observe", t))
        for _ in range(pol):
            actn = scripted_actions(rng, E, rc)
            for x in (eng, twin):
                x.rollout_write("actions", torch.from_numpy(actn).cuda())
                x.rollout_policy_step()
            lock.follow(actn, lock.grab(), True, ("policy", t))
            t += 1
        eng.rollout_check()
        twin.rollout_check()
        same_buffers(("policy", t))
    assert min(lock.restarts) >= 1


class _Grab:
    """Lockstep.grab on another engine (no oracles of its own)."""

    def __init__(self, eng):
        self.eng = eng


# ---------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------
def test_rollout_write_refuses_unknown_name():
    from mfrl_amd.battle import BattleBatch
    eng = BattleBatch.__new__(BattleBatch)          # no engine: the name is refused before any call into it
    for name in ("rewards", "view", "mean_action", "nonsense"):
        with pytest.raises(ValueError, match="not writable"):
            eng.rollout_write(name, np.zeros(4, dtype=np.int32))


def test_rollout_policy_path_declared_and_exported():
    import ctypes
    import os
    header = open(os.path.join(common.REPO, "include", "magent_amd.h")).read()
    for fn in ("mfx_battle_rollout_policy_path", "mfx_battle_rollout_write"):
        assert re.search(r"\bint %s\(void \*game" % fn, header), fn
        assert hasattr(ctypes.CDLL(common.HIP_LIB), fn), fn
