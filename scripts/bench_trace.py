"""What the recorder costs per step of the device rollout loop (mfrl_amd.recorder, csrc/trace_kernels.hip), and what
the replay costs per step.

A/B in one process with HIP-event pairs on the engine's stream: battle_rollout's loop (act_rollout for both groups,
rollout_policy_step, RolloutScoreboard.update) with RolloutRecorder.update() behind every step against the same loop
without it -- the loop of recorder=None --, rounds alternating; beside it one RolloutCollector.end() per step at the same
shape, for scale.  Then the replay: mfrl_amd.recorder.replay of one watched env of a recorded round on the one-env
engine, without and with frames, by a host clock (the replay synchronises at every call).

    python scripts/bench_trace.py --out profiles/trace_ab.jsonl

One JSON line per configuration; times are microseconds per step (median over rounds, each round one event pair).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mean-field-multi-agent-reinforcement-learning_amd", "python"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_score import models_for  # noqa: E402


def loop_us(eng, models, board, rec, steps, record):
    """One event pair around `steps` steps of the loop; microseconds per step."""
    import torch
    s = eng.torch_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    for _ in range(steps):
        for g in range(2):
            models[g].act_rollout(eng, g)
        eng.rollout_policy_step()
        board.update()
        if record:
            rec.update()
    b.record(s)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def collect_end_us(eng, models, max_steps):
    import torch
    from mfrl_amd.algo.tools import MemoryGroup
    from mfrl_amd.replay import RolloutCollector
    m = models[0]
    mg = MemoryGroup(m.view_space, m.feature_space, m.num_actions, 1024, 64, max_steps, use_mean=True)
    col = RolloutCollector(eng, mg, 0)
    s = eng.torch_stream()
    ends = []
    for k in range(6):
        for g in range(2):
            models[g].act_rollout(eng, g)
        col.begin()
        eng.rollout_policy_step()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        col.end()
        b.record(s)
        b.synchronize()
        ends.append(a.elapsed_time(b) * 1e3)
        col.discard()
    return statistics.median(ends[1:])


def ab(args, name, map_size, envs, watch, algos, precision, engines):
    import torch
    from mfrl_amd.algo.play import block_positions
    from mfrl_amd.battle import BattleBatch
    from mfrl_amd.recorder import RolloutRecorder, replay
    from mfrl_amd.scoreboard import RolloutScoreboard
    _, _, models = models_for(algos, map_size, args.max_steps, precision)
    key = (map_size, envs)
    if key not in engines:
        engines[key] = BattleBatch(map_size, envs, stream=torch.cuda.current_stream())
    eng = engines[key]
    placement = list(block_positions(map_size))

    def start():
        eng.reset()
        eng.rollout_init(placement, max_steps=args.max_steps, eps=0.0, seed=1, stagger=False)
        eng.rollout_policy_observe()
        board.attach()
        rec.attach(map_size, args.max_steps, placement)

    board = RolloutScoreboard(eng)
    rec = RolloutRecorder(eng, watch, args.steps)
    eng.reset()
    eng.rollout_init(placement, max_steps=args.max_steps, eps=0.0, seed=1, stagger=False)
    rec_warm = RolloutRecorder(eng, watch, args.warmup)
    eng.rollout_policy_observe()
    board.attach()
    rec_warm.attach(map_size, args.max_steps, placement)
    loop_us(eng, models, board, rec_warm, args.warmup, True)
    rec_warm.finish(final=False)
    with_r, without = [], []
    for r in range(args.rounds):
        for record in ((True, False) if r % 2 == 0 else (False, True)):
            start()                        # every round from the start: both arms play the same steps
            (with_r if record else without).append(loop_us(eng, models, board, rec, args.steps, record))
            if record:
                trace = rec.finish()
    board.finish()
    eng.rollout_check()
    out = {"case": name, "map_size": map_size, "envs": envs, "watched": len(watch), "algos": algos,
           "act_precision": precision, "rowcap": eng.rowcap, "steps": args.steps, "rounds": args.rounds,
           "policy_path": eng.rollout_policy_path(),
           "record_bytes_per_step": 13 * 2 * eng.rowcap * len(watch) + 48 * len(watch),
           "with_recorder_us": statistics.median(with_r), "without_recorder_us": statistics.median(without),
           "with_recorder_all_us": with_r, "without_recorder_all_us": without}
    out["difference_us"] = out["with_recorder_us"] - out["without_recorder_us"]
    try:
        out["collect_end_us"] = collect_end_us(eng, models, args.max_steps)
    except Exception as ex:                # (storage for 8192 x 164 rows of views may not be there)
        out["collect_end_us"] = None
        out["collect_end_note"] = repr(ex)[:200]
    # the replay of watched env 0 of the last recorded round: the comparison alone, then with frames
    t0 = time.time()
    done = replay(trace, 0)
    out["replay_us_per_step"] = (time.time() - t0) * 1e6 / max(done["steps"], 1)
    with tempfile.TemporaryDirectory() as d:
        t0 = time.time()
        done = replay(trace, 0, render_dir=d)
        out["replay_frames_us_per_step"] = (time.time() - t0) * 1e6 / max(done["steps"], 1)
    out["replay_steps"], out["replay_episodes"] = done["steps"], done["episodes"]
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "trace_ab.jsonl"))
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--rounds", type=int, default=6)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--max_steps", type=int, default=400)
    p.add_argument("--skip_big", action="store_true")
    args = p.parse_args()
    cases = [("64 envs 40x40, 1 watched", 40, 64, [0], ["mfq", "mfac"], "f32"),
             ("64 envs 40x40, 8 watched", 40, 64, [0, 9, 18, 27, 36, 45, 54, 63], ["mfq", "mfac"], "f32")]
    if not args.skip_big:
        cases.append(("8192 envs 64x64, 8 watched, MF-AC bf16", 64, 8192,
                      [0, 1170, 2340, 3510, 4680, 5850, 7020, 8191], ["mfac", "mfac"], "bf16"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    engines = {}
    with open(args.out, "w") as f:
        for c in cases:
            rec = ab(args, *c, engines)
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
