"""NumPy restatement of the recorder's contract (include/magent_amd.h part 8, csrc/trace_kernels.hip): attach and update
on plain arrays, one watched env at a time, with no cleverness.  The device buffers have exactly these dtypes and
layouts, so a test compares whole buffers byte for byte.

    src: dict of group_num int32 [E][2], alive uint8 [E][2][rowcap], stats float64 [E][4], agent_steps int64 [E],
         actions int32 [E][2][rowcap], ids int32 [E][2][rowcap], rewards float32 [E][2][rowcap], rng uint32 [E]
    rec: dict of envs int32 [K], carry int64 [2][K][4], head int64 [cap][K][6], actions / ids int32, rewards float32,
         alive uint8 [cap][K][2][rowcap], state int64 [2], seeds uint32 [K]

lockstep(name) builds a trace on the CPU: the scripted case `name` of tests/score_cases.py stepped on the C oracle, the
source arrays kept as the device keeps them (rows written up to the group size, stale entries behind it left), one
update per step.
"""
import numpy as np

HEAD, CARRY = 6, 4
VALID, N, EP_BEFORE, EP_AFTER, STEPS = 0, 1, 3, 4, 5
ERR_STEP, ERR_EPISODE, ERR_COUNT, FULL, ERR_ENV = 1, 2, 4, 8, 16
ROWS = (("actions", np.int32), ("ids", np.int32), ("rewards", np.float32), ("alive", np.uint8))
NAMES = ("envs", "carry", "head", "actions", "ids", "rewards", "alive", "state", "seeds")


def sizes(K, rowcap, cap):
    rows = cap * K * 2 * rowcap
    return {"envs": K * 4, "carry": 2 * K * CARRY * 8, "head": cap * K * HEAD * 8, "actions": rows * 4, "ids": rows * 4,
            "rewards": rows * 4, "alive": rows, "state": 16, "seeds": K * 4}


def new_record(K, rowcap, cap, fill=0):
    """Record arrays with every byte `fill` (what the device buffers hold before attach)."""
    shapes = {"envs": ((K,), np.int32), "carry": ((2, K, CARRY), np.int64), "head": ((cap, K, HEAD), np.int64),
              "actions": ((cap, K, 2, rowcap), np.int32), "ids": ((cap, K, 2, rowcap), np.int32),
              "rewards": ((cap, K, 2, rowcap), np.float32), "alive": ((cap, K, 2, rowcap), np.uint8),
              "state": ((2,), np.int64), "seeds": ((K,), np.uint32)}
    rec = {k: np.full(int(np.prod(sh)) * np.dtype(dt).itemsize, fill, np.uint8).view(dt).reshape(sh)
           for k, (sh, dt) in shapes.items()}
    rec["cap"] = int(cap)
    return rec


def _count_ok(n, rowcap):
    return 0 <= n <= rowcap


def _carry(src, e):
    return [int(src["group_num"][e, 0]), int(src["group_num"][e, 1]), int(np.int64(src["stats"][e, 0])),
            int(src["agent_steps"][e])]


def attach(rec, src, envs):
    E, rowcap = len(src["group_num"]), src["alive"].shape[2]
    rec["envs"][:] = envs
    rec["state"][:] = 0
    for k, e in enumerate(envs):
        rec["carry"][1, k] = 0
        if not 0 <= e < E:
            rec["carry"][0, k] = 0
            rec["seeds"][k] = 0
            rec["state"][1] |= ERR_ENV
            continue
        rec["carry"][0, k] = _carry(src, e)
        rec["seeds"][k] = src["rng"][e]
        if not (_count_ok(rec["carry"][0, k, 0], rowcap) and _count_ok(rec["carry"][0, k, 1], rowcap)):
            rec["state"][1] |= ERR_COUNT


def update(rec, src, step):
    E, rowcap = len(src["group_num"]), src["alive"].shape[2]
    if step < 0 or step >= rec["cap"]:
        rec["state"][1] |= FULL
        return
    for k, e in enumerate(rec["envs"]):
        e = int(e)
        if not 0 <= e < E:
            rec["state"][1] |= ERR_ENV
            rec["head"][step, k] = 0
            continue
        for name, _ in ROWS:
            rec[name][step, k] = src[name][e]
        n0, n1, ep, steps0 = (int(x) for x in rec["carry"][step & 1, k])
        new = _carry(src, e)
        err = 0
        if new[3] - steps0 != n0 + n1:
            err |= ERR_STEP
        if new[2] - ep not in (0, 1):
            err |= ERR_EPISODE
        if not all(_count_ok(n, rowcap) for n in (n0, n1, new[0], new[1])):
            err |= ERR_COUNT
        rec["state"][1] |= err
        rec["head"][step, k] = [0 if err else 1, n0, n1, ep, new[2], new[3]]
        rec["carry"][(step + 1) & 1, k] = new
    rec["state"][0] = step + 1


# ----------------------------------------------------------------------------------------------- the CPU lockstep
_CACHE = {}


def lockstep(name, watch=None, lib_path=None, seeds=None):
    """The scripted case `name` (score_cases.PLANS: 25 steps, a step cap of 12) on the C oracle -- or the build at
    lib_path --, the source arrays kept as the device rollout keeps them, one update() per step.  seeds: per env, the
    state its shuffle engine starts the round with (default 1, a new engine's).  Returns {"trace": the
    recorder's trace dict, "rec", "run": score_cases.oracle_run(name), "src": the arrays after the last step}."""
    import common
    import score_cases as sc
    from mfrl_amd import recorder
    plan, run = sc.PLANS[name], sc.oracle_run(name)
    E, rowcap, placement = plan["envs"], run["rowcap"], run["placement"]
    watch = list(range(E))[::-1] if watch is None else list(watch)
    seeds = [1] * E if seeds is None else [int(x) for x in seeds]
    key = (name, tuple(watch), lib_path, tuple(seeds))
    if key in _CACHE:
        return _CACHE[key]
    envs = [common.battle_env(lib_path or common.ORACLE_LIB, plan["map_size"]) for _ in range(E)]

    def reset(env, h):
        env.reset()
        for g, pos in enumerate(placement):
            env.add_agents(h[g], method="custom", pos=pos)

    for (env, h), seed in zip(envs, seeds):
        env.set_seed(seed)
        reset(env, h)
    rng = np.random.default_rng(99)
    src = {"group_num": np.array([[len(p) for p in placement]] * E, np.int32),
           "alive": rng.integers(0, 2, size=(E, 2, rowcap)).astype(np.uint8), "stats": np.zeros((E, 4), np.float64),
           "agent_steps": np.zeros(E, np.int64), "actions": np.zeros((E, 2, rowcap), np.int32),
           "ids": rng.integers(0, 1000, size=(E, 2, rowcap)).astype(np.int32),
           "rewards": rng.random((E, 2, rowcap)).astype(np.float32), "rng": np.array(seeds, np.uint32)}
    rec = new_record(len(watch), rowcap, sc.STEPS)
    attach(rec, src, watch)
    ep_len = [0] * E
    for t in range(sc.STEPS):
        src["actions"][:] = run["actions"][t]
        for e, (env, h) in enumerate(envs):
            n = [int(env.get_num(h[g])) for g in range(2)]
            for g in range(2):
                env.set_action(h[g], np.ascontiguousarray(src["actions"][e, g, :n[g]]))
            done = bool(env.step())
            for g in range(2):
                src["ids"][e, g, :n[g]] = env.get_agent_id(h[g])
                src["alive"][e, g, :n[g]] = env.get_alive(h[g])
                src["rewards"][e, g, :n[g]] = env.get_reward(h[g])
            env.clear_dead()
            src["agent_steps"][e] += sum(n)
            ep_len[e] += 1
            if done or ep_len[e] >= sc.MAX_STEPS:
                ep_len[e] = 0
                src["stats"][e, 0] += 1.0
                reset(env, h)
            src["group_num"][e] = [int(env.get_num(h[g])) for g in range(2)]
        update(rec, src, t)
    assert int(rec["state"][1]) == 0 and int(rec["state"][0]) == sc.STEPS
    trace = recorder.make_trace(watch, rowcap, sc.STEPS, rec, plan["map_size"], sc.MAX_STEPS, placement)
    _CACHE[key] = {"trace": trace, "rec": rec, "run": run, "src": src}
    return _CACHE[key]
