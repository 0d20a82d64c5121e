"""What the opt-in neighbourhood mean action (mean_field = "neighbors") costs, and that the default "group"
path costs what it did, in one process.

    python scripts/bench_neighbor_mean.py [--reps 5] [--parent_lib build/libmagent_parent.so] [--arms a b c]
                                          [--out profiles/neighbor_mean_ab.jsonl]

  arm a   the kernel alone: NeighborMean.update() (k_neighbor_mean<rollout>, R = 6, group 0) on a mid-episode batch --
          --rush rush steps, then one policy step with random actions -- at 64 envs of 40 x 40, 8192 envs of 64 x 64 and
          2048 envs of 256 x 256 / 4096 agents, against its own traffic floor: the bytes of the live output rows plus 8
          position bytes per row at the write ceiling measured in the same process (BattleBatch.store_ceiling, the best
          of three shapes).  (Repeating update() on one state repeats the same window scans; the carried group size
          then equals the new one.)
  arm b   play_rollout(train=False) of --steps steps with two MF-Q models, "neighbors" against "group", arms
          alternating, at the same three shapes: ms per step, round set-up included in both.
  arm c   the "group" arm of b against the same call on --parent_lib (the library of the commit before the feature,
          built by `make` in a checkout of it; skipped when the file is not given), its own engine and models.

Every timed call ends in a device synchronise; one JSON line per timed call and one summary line (median, min, max) per
arm and shape are appended to --out."""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mean-field-multi-agent-reinforcement-learning_amd", "python"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import battle_driver as bd  # noqa: E402
import magent  # noqa: E402
import mfrl_amd  # noqa: E402
from mfrl_amd import battle, mf, policy  # noqa: E402
from mfrl_amd.algo import play, spawn_ai  # noqa: E402

SHAPES = {"40x40x64": (40, 64, 64), "64x64x8192": (64, 128, 8192), "256x256x2048": (256, 2048, 2048)}   # map, per side, envs
NA, RADIUS = 21, 6


@contextlib.contextmanager
def library(dll):
    """Objects made inside bind to `dll` (None: this build's): the engine, the forwards."""
    if dll is None:
        yield
        return
    keep = battle.lib, policy.lib, mf.lib
    battle.lib = policy.lib = mf.lib = lambda: dll
    try:
        yield
    finally:
        battle.lib, policy.lib, mf.lib = keep


def summary(arm, shape, ms, **extra):
    out = dict(extra, arm=arm, shape=shape, summary=True, device=torch.cuda.get_device_name(0))
    for k, v in ms.items():
        out[k] = {"median": round(float(np.median(v)), 5), "min": round(float(min(v)), 5), "max": round(float(max(v)), 5)}
    return out


def arm_a(args, name, emit):
    map_size, n_side, E = SHAPES[name]
    eng = battle.BattleBatch(map_size, E, stream=torch.cuda.current_stream())
    eng.rollout_init(list(bd.block_positions(map_size, n_side)), max_steps=400, eps=0.2, seed=5, stagger=True)
    eng.rollout_step(args.rush)
    eng.rollout_policy_observe()
    nm = mf.NeighborMean(eng, 0, RADIUS)
    nm.reset()
    acts = torch.randint(0, NA, (E, 2, eng.rowcap), dtype=torch.int32, device="cuda")
    eng.rollout_write("actions", acts)
    eng.rollout_policy_step()
    for _ in range(3):
        nm.update()
    num = torch.empty((E, 2), dtype=torch.int32, device="cuda")
    eng.rollout_copy("group_num", num)
    eng.sync()
    live = int(num[:, 0].sum().item())
    ms = {"update": []}
    for rep in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):
            nm.update()
        b.record()
        b.synchronize()
        ms["update"].append(a.elapsed_time(b) / args.calls)
        emit({"arm": "a", "shape": name, "rep": rep, "calls": args.calls, "ms_per_call": round(ms["update"][-1], 5)})
    assert bool(torch.isfinite(nm.rows).all())
    eng.rollout_check()
    ceiling = max(eng.store_ceiling(1 << 30, s) for s in (0, 2, 6))        # (overwrites the views: their last use)
    floor_bytes = live * (NA * 4 + 8)
    floor_ms = floor_bytes / (ceiling * 1e9) * 1e3
    emit(summary("a", name, ms, unit="ms_per_call", radius=RADIUS, live_rows=live, rows=E * eng.rowcap,
                 floor_bytes=floor_bytes, write_ceiling_GBps=round(ceiling, 1), floor_ms=round(floor_ms, 5),
                 times_floor=round(float(np.median(ms["update"])) / floor_ms, 1)))


def round_ms(eng, models, map_size, steps, dll=None):
    with library(dll), contextlib.redirect_stdout(io.StringIO()):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        play.play_rollout(eng, 0, map_size, steps, models, eps=1.0, train=False, left_id=0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps


def arm_bc(args, name, emit, parent):
    """play_rollout's placement is generate_map's two blocks (0.04 * map^2 agents per side)."""
    map_size, _, E = SHAPES[name]
    env = magent.GridWorld("battle", map_size=map_size)
    h = env.get_handles()
    torch.manual_seed(0)
    arms = {}
    for arm, dll in (("group", None), ("neighbors", None), ("group_parent", parent)):
        if arm == "group_parent" and (parent is None or "c" not in args.arms or name not in args.parent_shapes):
            continue
        if arm == "neighbors" and "b" not in args.arms:
            continue
        with library(dll):
            if arm == "neighbors":
                eng = arms["group"][0]                               # (one engine serves both modes)
            else:
                eng = battle.BattleBatch(map_size, E, stream=torch.cuda.current_stream())
            models = [spawn_ai("mfq", None, env, h[g], "%s-%d" % (arm, g), args.steps, memory_size=1024) for g in range(2)]
            for m in models:
                if arm == "neighbors":
                    m.mean_field, m.mf_radius = "neighbors", RADIUS
            arms[arm] = (eng, models, dll)
    for eng, models, dll in arms.values():
        round_ms(eng, models, map_size, args.steps, dll)               # warm-up: weights, buffers, code objects
    ms = {k: [] for k in arms}
    for rep in range(args.reps):
        for k, (eng, models, dll) in arms.items():
            ms[k].append(round_ms(eng, models, map_size, args.steps, dll))
            emit({"arm": "bc", "shape": name, "mode": k, "rep": rep, "steps": args.steps, "ms_per_step": round(ms[k][-1], 4)})
    emit(summary("bc", name, ms, unit="ms_per_step (play_rollout, train=False, round set-up included)", steps=args.steps,
                 radius=RADIUS, agents_per_side=len(play.block_positions(map_size)[0])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="arm a: update() calls per timed window")
    ap.add_argument("--rush", type=int, default=40, help="arm a: rush steps before the measured state")
    ap.add_argument("--steps", type=int, default=10, help="arms b, c: steps per round")
    ap.add_argument("--arms", nargs="+", choices=["a", "b", "c"], default=["a", "b", "c"])
    ap.add_argument("--shapes", nargs="+", choices=list(SHAPES), default=list(SHAPES))
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--parent_shapes", nargs="+", choices=list(SHAPES), default=["40x40x64", "64x64x8192"],
                    help="arm c: the shapes that also get an engine on --parent_lib (a second copy of the batch in HBM)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "neighbor_mean_ab.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_neighbor_mean.py measures on the GPU"
    parent = None
    if args.parent_lib:
        mfrl_amd.lib()                                                   # (this build's library first: it pins the HIP runtime)
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib), mode=ctypes.RTLD_LOCAL)
        parent.mfx_last_error.restype = ctypes.c_char_p
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(line):
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")

    for name in args.shapes:
        if "a" in args.arms:
            arm_a(args, name, emit)
            torch.cuda.empty_cache()
        if "b" in args.arms or "c" in args.arms:
            arm_bc(args, name, emit, parent)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
