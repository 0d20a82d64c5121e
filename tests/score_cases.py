"""The scripted cases of the scoreboard tests: plans, placements and seeded actions, and the C oracle run over them.

oracle_run(plan) steps one oracle env per batch env with the plan's scripted actions, restarting an env at done or at
the step cap as the rollout does, and returns what a scorekeeper must find: per step the buffers' contents that matter
(group sizes before the step, alive flags before clear_dead) and per finished episode its record with Runner.run's
rule.  It runs on the CPU; tests/test_score_cpu.py asserts the cases' own conditions on it, tests/test_score_gpu.py
drives the device with the same actions and compares.
"""
import numpy as np

import common
import score_ref
from test_policy_big_gpu import interleaved_positions

NA = 21
ATTACK = np.arange(13, 21)              # the eight attack ids of the battle config (13 moves first)
MAX_STEPS, STEPS = 12, 25


def packed_positions(map_size, n_small, n_big):
    """n_small agents of group 0 in a column at the map centre, group 1 in the two columns on either side of it and
    beyond: every member of the small group is in attack range of several enemies from the first step."""
    cx, cy = map_size // 2, map_size // 2
    small = [[cx, cy + j, 0] for j in range(n_small)]
    big, k = [], 0
    for dx in (-1, 1, -2, 2, -3, 3):
        for j in range(-1, n_small + 1):
            if k < n_big:
                big.append([cx + dx, cy + j, 0])
                k += 1
    assert k == n_big
    return [small, big]


# name: map size, envs, MFX_SMALL_E, policy path, placement, probability of an attack id, seed
PLANS = {
    "fused": dict(map_size=64, envs=3, small_e="0", path="k_rollout", placement=lambda: interleaved_positions(64, 128),
                  p_attack=0.0, seed=31),
    "few": dict(map_size=40, envs=2, small_e=None, path="k_observe_items+k_rollout_big",
                placement=lambda: interleaved_positions(40, 64), p_attack=0.0, seed=31),
    "packed": dict(map_size=40, envs=2, small_e=None, path="k_observe_items+k_rollout_big",
                   placement=lambda: packed_positions(40, 2, 18), p_attack=0.9, seed=5),
}


def actions(rng, E, rowcap, p_attack):
    """[E][2][rowcap] int32: an attack id with probability p_attack, else uniform over the 21 ids."""
    a = rng.integers(0, NA, size=(E, 2, rowcap), dtype=np.int32)
    if p_attack > 0.0:
        hit = rng.random(size=a.shape) < p_attack
        a = np.where(hit, rng.choice(ATTACK, size=a.shape).astype(np.int32), a)
    return np.ascontiguousarray(a, dtype=np.int32)


def rowcap_of(placement):
    return (max(len(p) for p in placement) + 3) & ~3


_CACHE = {}


def oracle_run(name, rowcap=None):
    """{"actions": [STEPS] of [E][2][rowcap], "episodes": [E] lists of records (dicts: len, nums, surv, kill, winner,
    done), "steps": [STEPS][E] dicts (n before the step, alive before clear_dead, done), "rowcap"}.  rowcap: the
    engine's (the action arrays' width, which the draws depend on); the default is the placement's, rounded up to 4."""
    plan = PLANS[name]
    placement = plan["placement"]()
    rowcap = rowcap or rowcap_of(placement)
    key = (name, rowcap)
    if key in _CACHE:
        return _CACHE[key]
    E = plan["envs"]
    envs = []
    for e in range(E):
        env, h = common.battle_env(common.ORACLE_LIB, plan["map_size"])
        envs.append((env, h))

    def reset(env, h):
        env.reset()
        for g, pos in enumerate(placement):
            env.add_agents(h[g], method="custom", pos=pos)

    for env, h in envs:
        reset(env, h)
    rng = np.random.default_rng(plan["seed"])
    start = [[len(p) for p in placement] for _ in range(E)]
    ep_len = [0] * E
    out = {"actions": [], "episodes": [[] for _ in range(E)], "steps": [], "rowcap": rowcap, "placement": placement}
    for t in range(STEPS):
        actn = actions(rng, E, rowcap, plan["p_attack"])
        out["actions"].append(actn)
        row = []
        for e, (env, h) in enumerate(envs):
            n = [int(env.get_num(h[g])) for g in range(2)]
            for g in range(2):
                env.set_action(h[g], np.ascontiguousarray(actn[e, g, :n[g]]))
            done = bool(env.step())
            nums = [int(env.get_num(h[g])) for g in range(2)]             # before clear_dead: senario_battle.py:258
            alive = [env.get_alive(h[g]).astype(bool).copy() for g in range(2)]
            assert nums == n
            env.clear_dead()
            ep_len[e] += 1
            row.append({"n": n, "alive": alive, "done": done})
            if done or ep_len[e] >= MAX_STEPS:
                win, kill = score_ref.winner(start[e], nums)
                out["episodes"][e].append({"len": ep_len[e], "nums": nums, "surv": [int(a.sum()) for a in alive],
                                           "kill": kill, "winner": win, "done": done})
                ep_len[e] = 0
                reset(env, h)
        out["steps"].append(row)
    _CACHE[key] = out
    return out
