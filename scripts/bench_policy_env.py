"""A learned policy on the large-env plans, end to end: a randomly initialised mean-field QNet per group drives a
BattleBatch through observe / act / step (QNetHIP.act_rollout + BattleBatch.rollout_policy_step, which on these
plans runs k_rollout_big<ext> + k_observe_items), timed with device events on the engine's stream.  --net mfac: two
MFAC networks (ACNetHIP.act_rollout, the sampled policy, drawn with (--seed, the loop step)) drive the same loop.

    python scripts/bench_policy_env.py --map 256 --agents 4096 --envs 2048
    python scripts/bench_policy_env.py --map 40 --envs 1 --steps 2000 --warmup 100

--agents N: two blocks of N / 2 (tests/battle_driver.block_positions, bench.py's placement); 0 (default): the
reference's generate_map placement (4 % of the cells).  Prints one JSON line: agent-steps/s over the timed window
(host clock around the window, ending in a synchronise), the forward's and the env step's (step + observation)
device-event time per loop step, the network's precision (--precision f32 | bf16: the acting mode of QNetHIP / ACNetHIP;
with bf16 also f32_action_agreement, the share of live agents whose action on the final observation -- for mfac drawn
from the same seed and step -- is the f32 network's), and check.ok: after the clock, sampled envs are replayed on the C oracle from
rollout_init with the actions the device recorded at every step (warm-up included), and the final views, features,
rewards, mean actions and group sizes must agree bit for bit.

--collect: run a mfrl_amd.replay.RolloutCollector for group 0 (into an MF-Q MemoryGroup's step rows) around every
policy step of the loop, warm-up included: the record gains collect_ms (begin + end, device events), rows_per_step,
row_bytes and the collector's achieved bytes per second (read + write of the row bytes), and is appended to
profiles/policy_env_steps.jsonl.  When the rows of all steps would not fit in --collect-gb of HBM, every step's rows
are dropped again before the next (RolloutCollector.discard: the device counter restarts, nothing is read back).

--rush-step: time rollout_step(1) launches instead (the on-device rush policy; no network).  With MFX_BIG_FUSED=0 it
runs the same two kernels as the policy form's env step, on two sub-batch streams: the yardstick that step is
compared with.  Works with older builds of the library (MAGENT_LIB)."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mean-field-multi-agent-reinforcement-learning_amd", "python"))
sys.path.insert(0, os.path.join(REPO, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--map", type=int, default=256)
ap.add_argument("--agents", type=int, default=0)
ap.add_argument("--envs", type=int, default=2048)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--max-steps", type=int, default=400)
ap.add_argument("--check-envs", type=int, default=4)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--rush-step", action="store_true")
ap.add_argument("--precision", choices=["f32", "bf16"], default="f32")
ap.add_argument("--net", choices=["qnet", "mfac"], default="qnet")
ap.add_argument("--collect", action="store_true")
ap.add_argument("--collect-gb", type=float, default=48.0)
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

import battle_driver as bd  # noqa: E402
import common  # noqa: E402
import rollout_check as rck  # noqa: E402
from mfrl_amd.battle import BattleBatch  # noqa: E402

assert torch.cuda.is_available(), "bench_policy_env.py measures on the GPU"
torch.cuda.set_device(0)
if a.agents:
    placement = list(bd.block_positions(a.map, a.agents // 2))
else:
    _, left, right = bd.generate_map_positions(a.map, a.seed)
    placement = [left, right]
E, T = a.envs, a.warmup + a.steps
eng = BattleBatch(a.map, E, stream=torch.cuda.current_stream())
eng.rollout_init(placement, max_steps=a.max_steps, eps=0.2, seed=a.seed, stagger=True)
rc = eng.rowcap
res = {"script": "bench_policy_env.py", "map": a.map, "envs": E, "agents_per_env": sum(len(p) for p in placement),
       "steps": a.steps, "warmup": a.warmup, "rollout_path": eng.rollout_path(),
       "lib": os.path.basename(os.environ.get("MAGENT_LIB") or "libmagent.so")}


def agent_steps():
    buf = torch.empty(E, dtype=torch.int64, device="cuda")
    eng.rollout_copy("agent_steps", buf)
    eng.sync()
    return int(buf.sum().item())


def events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


if a.rush_step:
    eng.rollout_substeps(1)
    for _ in range(a.warmup):
        eng.rollout_step(1)
    n0 = agent_steps()
    ev = [events(2) for _ in range(a.steps)]
    t0 = time.perf_counter()
    for k in range(a.steps):
        ev[k][0].record()
        eng.rollout_step(1)
        ev[k][1].record()
    eng.sync()
    wall = time.perf_counter() - t0
    ms = [x.elapsed_time(y) for x, y in ev]
    eng.rollout_check()
    res.update({"mode": "rush-step", "big_fused": os.environ.get("MFX_BIG_FUSED", "1"),
                "agent_steps_per_s": (agent_steps() - n0) / wall,
                "env_step_ms": {"mean": statistics.fmean(ms), "median": statistics.median(ms), "max": max(ms)}})
    print(json.dumps(res))
    sys.exit(0)

from mfrl_amd.algo.nets import ACNet, QNet  # noqa: E402
from mfrl_amd.policy import ACNetHIP, QNetHIP  # noqa: E402

F, NA = 34, 21
Net, NetHIP = (ACNet, ACNetHIP) if a.net == "mfac" else (QNet, QNetHIP)
pols, nets = [], []
for g in range(2):
    torch.manual_seed(a.seed + g)
    nets.append(Net((13, 13, 7), (F,), NA, True).cuda())
    pols.append(NetHIP((13, 13, 7), (F,), NA, True, precision=a.precision).load(nets[g]))
res["policy_path"] = eng.rollout_policy_path()
res["net"] = a.net
res["precision"] = a.precision


def act(ps, g, t):
    """Group g's actions of loop step t from network ps[g] (mfac: the draw of (seed, t))."""
    if a.net == "mfac":
        ps[g].act_rollout(eng, g, seed=a.seed, step=t)
    else:
        ps[g].act_rollout(eng, g)


picks = rck.sample_envs(E, a.check_envs)
# the sampled envs' actions of every step since rollout_init, copied on the engine's stream after each forward
log = torch.empty((T, len(picks), 2, rc), dtype=torch.int32, device="cuda")


col, ROW_BYTES = None, 4 * (13 * 13 * 7 + F + 1 + 1 + NA) + 1 + 8      # view, feature, action, reward, prob; term; key
if a.collect:
    from mfrl_amd.algo.tools import MemoryGroup  # noqa: E402
    from mfrl_amd.replay import RolloutCollector  # noqa: E402
    col = RolloutCollector(eng, MemoryGroup((13, 13, 7), (F,), NA, 1024, 64, a.max_steps, use_mean=True), 0)
    col_keep = T * E * rc * ROW_BYTES <= a.collect_gb * 1e9


def loop_step(t, ev=None):
    if ev:
        ev[0].record()
    for g in range(2):
        act(pols, g, t)
    if ev:
        ev[1].record()
    for j, e in enumerate(picks):
        eng.rollout_copy_at("actions", log[t, j], e * 2 * rc * 4)
    if col:
        if not col_keep:
            col.discard()
        if ev:
            ev[4].record()
        col.begin()
        if ev:
            ev[5].record()
    if ev:
        ev[2].record()
    eng.rollout_policy_step()
    if ev:
        ev[3].record()
    if col:
        col.end()
        if ev:
            ev[6].record()


eng.rollout_policy_observe()
for t in range(a.warmup):
    loop_step(t)
n0 = agent_steps()
ev = [events(7) for _ in range(a.steps)]
t0 = time.perf_counter()
for k in range(a.steps):
    loop_step(a.warmup + k, ev[k])
eng.sync()
wall = time.perf_counter() - t0
n1 = agent_steps()
fwd = [x[0].elapsed_time(x[1]) for x in ev]
env = [x[2].elapsed_time(x[3]) for x in ev]
res.update({"mode": "policy", "agent_steps_per_s": (n1 - n0) / wall, "loop_ms": 1e3 * wall / a.steps,
            "forward_ms": {"mean": statistics.fmean(fwd), "median": statistics.median(fwd)},
            "env_step_ms": {"mean": statistics.fmean(env), "median": statistics.median(env), "max": max(env)}})

if col:
    n_rows = col.finish()
    per_step = n_rows / (T if col_keep else 1)
    cms = [x[4].elapsed_time(x[5]) + x[3].elapsed_time(x[6]) for x in ev]
    med = statistics.median(cms)
    res.update({"collect": True, "collect_kept_all_steps": col_keep, "rows_per_step": per_step, "row_bytes": ROW_BYTES,
                "collect_ms": {"mean": statistics.fmean(cms), "median": med, "max": max(cms),
                               "begin_median": statistics.median(x[4].elapsed_time(x[5]) for x in ev),
                               "end_median": statistics.median(x[3].elapsed_time(x[6]) for x in ev)},
                "collect_gb_per_s": 2 * per_step * ROW_BYTES / (med * 1e-3) / 1e9})

# ---------------------------------------------------------------- after the clock: the oracle replay
eng.rollout_check()
dev = rck.device_records(eng, picks)
acts = log.cpu().numpy()
if a.precision != "f32":
    # one more act on the final observation in both precisions: the share of live agents whose action is the f32 one
    num = torch.empty((E, 2), dtype=torch.int32, device="cuda")
    eng.rollout_copy("group_num", num)
    both = []
    for ps in (pols, [NetHIP((13, 13, 7), (F,), NA, True).load(n) for n in nets]):
        for g in range(2):
            act(ps, g, T)
        both.append(torch.empty((E, 2, rc), dtype=torch.int32, device="cuda"))
        eng.rollout_copy("actions", both[-1])
    eng.sync()
    live = torch.arange(rc, device="cuda")[None, None, :] < num[:, :, None]
    res["f32_action_agreement"] = {"agents": int(live.sum()), "share": float((both[0] == both[1])[live].float().mean())}
bad = []
for j, e in enumerate(picks):
    o, h = common.battle_env(common.ORACLE_LIB, a.map)

    def reset():
        o.reset()
        for g in range(2):
            o.add_agents(h[g], method="custom", pos=placement[g])

    reset()
    ep_len, last = e * a.max_steps // E, None
    for t in range(T):
        n = [len(o.get_agent_id(h[g])) for g in range(2)]
        act = [np.ascontiguousarray(acts[t, j, g, :n[g]]) for g in range(2)]
        for g in range(2):
            o.set_action(h[g], act[g])
        done = o.step()
        rew = [o.get_reward(h[g]).copy() for g in range(2)]
        o.clear_dead()
        ep_len += 1
        restart = bool(done) or ep_len >= a.max_steps
        if restart:
            ep_len = 0
            reset()
        last = (n, act, rew, restart)
    n, act, rew, restart = last
    for g in range(2):
        v, f = o.get_observation(h[g])
        m = len(v)
        if int(dev["group_num"][j, g]) != m:
            bad.append("env %d group %d: size" % (e, g))
            continue
        if dev["view"][g][j, :m].tobytes() != v.reshape(m, -1).tobytes():
            bad.append("env %d group %d: view" % (e, g))
        if dev["feature"][g][j, :m].tobytes() != f.tobytes():
            bad.append("env %d group %d: feature" % (e, g))
        if dev["rewards"][j, g, :n[g]].tobytes() != rew[g].tobytes():
            bad.append("env %d group %d: rewards" % (e, g))
        want = (np.zeros(NA) if restart else
                np.bincount(act[g], minlength=NA) / n[g] if n[g] else np.full(NA, np.nan))
        if not np.array_equal(dev["mean"][j, g, :NA], want, equal_nan=True):
            bad.append("env %d group %d: mean action" % (e, g))
res["check"] = {"ok": not bad, "envs": picks, "steps": T, "bad": bad[:8]}
print(json.dumps(res))
if col:
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "policy_env_steps.jsonl"), "a") as f:
        f.write(json.dumps(res) + "\n")
sys.exit(0 if not bad else 1)
