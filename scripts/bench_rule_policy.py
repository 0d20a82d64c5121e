"""The scripted rule opponent (csrc/rule_kernels.hip), measured.

    python scripts/bench_rule_policy.py --out profiles/rule_policy_ab.jsonl
    python scripts/bench_rule_policy.py --sections default --parent_lib <libmagent.so of the parent commit>

Sections (arms alternate inside one process -- rep 0: every arm, rep 1: every arm, ... --, --reps of each; one JSON
line per arm with the median, min and max):
  kernel   the acting call of one group on the live rows of --kernel_envs envs of 64 x 64 at step 0 (2048 envs: 262,144
           rows): the rule (eps 0), the random opponent (eps 1, which reads no row), the bf16 actor-critic acting
           forward, and the replay collector's begin (k_collect_begin: the row list and one copy of every row), each
           with its row list; bytes/s over the read floor rows x (view + feature + 4 B)
  step     a battle_rollout step -- both groups act, rollout_policy_step -- with an MF-Q main side and a rush opponent
           against the same step with an MF-Q opponent, at 64 envs of 40 x 40 and --step_envs (8192) envs of 64 x 64
  default  bench.py (no rule anywhere) in child processes, this build against --parent_lib, alternating; --aa_lib
           adds a byte-identical copy of the parent's library as a third arm (how far two files of one code measure apart)
Every timing of the first two is a device-event pair on the engine's stream."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mean-field-multi-agent-reinforcement-learning_amd", "python"))
sys.path.insert(0, os.path.join(REPO, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--sections", nargs="+", choices=["kernel", "step", "default"], default=["kernel", "step"])
ap.add_argument("--kernel_envs", type=int, default=2048)
ap.add_argument("--step_envs", type=int, default=8192)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--parent_lib", type=str, default=None, help="section default: the parent commit's libmagent.so")
ap.add_argument("--bench_steps", type=int, default=60)
ap.add_argument("--first", choices=["parent", "this"], default="parent",
                help="section default: the arm that runs first in every pair")
ap.add_argument("--aa_lib", type=str, default=None,
                help="section default: a byte-identical copy of --parent_lib under another name, run as a third arm")
ap.add_argument("--out", type=str, default=None, help="append the JSON lines to this file too")
a = ap.parse_args()

lines = []


def summary(section, arm, xs, **extra):
    ln = {"script": "bench_rule_policy.py", "section": section, "arm": arm, "reps": len(xs),
          "median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}
    ln.update(extra)
    lines.append(ln)
    print(json.dumps(ln), flush=True)


def alternate(arms):
    """arms: {name: (engine, callable)}; -> {name: [ms per call]}."""
    import torch
    for name, (eng, fn) in arms.items():
        for _ in range(a.warmup):
            fn()
        eng.sync()
    ms = {name: [] for name in arms}
    for _ in range(a.reps):
        for name, (eng, fn) in arms.items():
            with torch.cuda.stream(eng.torch_stream()):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    fn()
                e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.iters)
    return ms


if "kernel" in a.sections or "step" in a.sections:
    import torch

    import battle_driver as bd
    import magent
    from mfrl_amd.algo import spawn_ai
    from mfrl_amd.algo.nets import ACNet
    from mfrl_amd.algo.tools import MemoryGroup
    from mfrl_amd.battle import BattleBatch
    from mfrl_amd.policy import ACNetHIP
    from mfrl_amd.replay import RolloutCollector

    assert torch.cuda.is_available(), "bench_rule_policy.py measures on the GPU"
    torch.cuda.set_device(0)
    torch.manual_seed(3)
    VS, FS, NA = (13, 13, 7), (34,), 21

if "kernel" in a.sections:
    E = a.kernel_envs
    env = magent.GridWorld("battle", map_size=64)
    h = env.get_handles()
    left, right = bd.block_positions(64, 128)
    eng = BattleBatch(64, E, stream=torch.cuda.current_stream())
    eng.rollout_init([left, right], max_steps=400, eps=0.0, seed=1, stagger=False)
    eng.rollout_policy_observe()
    rows = E * len(left)
    rush = spawn_ai("rush", None, env, h[0], "bench-rush", 400)
    rnd = spawn_ai("random", None, env, h[0], "bench-random", 400)
    ac = ACNetHIP(VS, FS, NA, False, precision="bf16").load(ACNet(VS, FS, NA, use_mf=False).cuda())
    mg = MemoryGroup(VS, FS, NA, 1024, 64, 400, use_mean=True)
    mg._rows._ensure(rows + 1024)
    col = RolloutCollector(eng, mg, 0, capacity=rows + 1024)

    def collect():
        col.begin()
        col.discard()            # (nothing is kept: the next begin restarts the row counter)

    ms = alternate({"rule_rush": (eng, lambda: rush.act_rollout(eng, 0)),
                    "rule_random": (eng, lambda: rnd.act_rollout(eng, 0)),
                    "acnet_bf16": (eng, lambda: ac.act_rollout(eng, 0, seed=1, step=1)),
                    "collect_begin": (eng, collect)})
    floor = rows * (1183 * 4 + 34 * 4 + 4)
    for name, xs in ms.items():
        summary("kernel", name, xs, unit="ms per call", rows=rows, iters=a.iters,
                read_floor_gb_per_s=round(floor / (statistics.median(xs) * 1e-3) / 1e9, 1))
    del eng, col, mg

if "step" in a.sections:
    for E, size in ((64, 40), (a.step_envs, 64)):
        env = magent.GridWorld("battle", map_size=size)
        h = env.get_handles()
        left, right = bd.block_positions(size, 128) if size == 64 else bd.generate_map_positions(size, 0)[1:]
        eng = BattleBatch(size, E, stream=torch.cuda.current_stream())
        eng.rollout_init([left, right], max_steps=400, eps=0.0, seed=1, stagger=False)
        eng.rollout_policy_observe()
        main = spawn_ai("mfq", None, env, h[0], "bench-main", 400, memory_size=1024)
        oppo = {"learned": spawn_ai("mfq", None, env, h[1], "bench-oppo", 400, memory_size=1024),
                "rush": spawn_ai("rush", None, env, h[1], "bench-rush", 400)}

        def step(o):
            main.act_rollout(eng, 0)
            o.act_rollout(eng, 1)
            eng.rollout_policy_step()

        ms = alternate({"oppo_" + k: (eng, (lambda o=o: step(o))) for k, o in oppo.items()})
        for name, xs in ms.items():
            summary("step", name, xs, unit="ms per step", envs=E, map=size, iters=a.iters)
        eng.rollout_check()
        del eng, main, oppo

if "default" in a.sections:
    assert a.parent_lib and os.path.exists(a.parent_lib), "--parent_lib: the parent commit's libmagent.so"
    order = ["parent", "this"] if a.first == "parent" else ["this", "parent"]
    libs = {"parent": a.parent_lib, "this": None}
    if a.aa_lib:                 # an A/A arm: how far two files of the same code measure apart
        assert os.path.exists(a.aa_lib), a.aa_lib
        order.append("parent_copy")
        libs["parent_copy"] = a.aa_lib
    rates = {name: [] for name in order}
    for _ in range(a.reps):
        for name in order:
            envp = dict(os.environ)
            if libs[name]:
                envp["MAGENT_LIB"] = os.path.abspath(libs[name])
            else:
                envp.pop("MAGENT_LIB", None)
            out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps",
                                  str(a.bench_steps), "--warmup", "20"], env=envp, capture_output=True, text=True,
                                 check=True, timeout=300).stdout
            rec = json.loads([x for x in out.splitlines() if x.startswith("{")][-1])
            rates[name].append(float(rec["value"]))
    for name, xs in rates.items():
        summary("default", name, xs, unit="bench.py value", steps=a.bench_steps, first=a.first)

if a.out:
    with open(a.out, "a") as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + "\n")
