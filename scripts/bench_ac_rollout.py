"""Measurements of the episode-chain training path of AC / MFAC (ActorCritic.train_rollout, the linked
RolloutCollector), appended as JSON lines to --out (profiles/ac_rollout_ab.jsonl is such a run):

  prepare    one round of rows collected on the device rollout loop, then -- on those same rows, in this process,
             alternating --pairs times -- the time from the end of the last step to returns ready:
               chain  tail.nonzero() + gather of the tail rows + value forward (k_acnet) + mfx_chain_returns
               batch  EpisodesBuffer.batch() + value forward on view[last] + offsets + mfx_mfac_returns
             (device events on the engine's stream, which is the current stream; wall clock beside them)
  collector  begin() + end() per step with and without the link columns, device events around each half, --pairs
             alternated rounds of --max_steps steps each after one warm round that grows the storage
  rounds     train_battle --n_round 3 as a child process, with --rollout_episodes and without (play_batched): the
             [TIME] lines.  The two loops differ in restart semantics: play_batched idles an env once it is done,
             the rollout loop restarts it and keeps producing rows.

    python scripts/bench_ac_rollout.py --out profiles/ac_rollout_ab.jsonl prepare collector rounds
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "mean-field-multi-agent-reinforcement-learning_amd", "python")
sys.path.insert(0, PKG)


def emit(args, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def setup(args):
    import magent
    import torch
    from mfrl_amd.algo import spawn_ai
    from mfrl_amd.battle import BattleBatch
    env = magent.GridWorld("battle", map_size=args.map_size)
    h = env.get_handles()
    torch.manual_seed(3)
    models = [spawn_ai(args.algo, None, env, h[g], "%s-%d" % (args.algo, g), args.max_steps) for g in range(2)]
    eng = BattleBatch(args.map_size, args.envs, stream=torch.cuda.current_stream())
    return env, models, eng


def start_round(args, eng, seed):
    from mfrl_amd.algo.play import block_positions
    left, right = block_positions(args.map_size)
    eng.reset()
    eng.rollout_init([left, right], max_steps=args.max_steps, eps=0.0, seed=seed, stagger=False)
    eng.rollout_policy_observe()


def collect_round(args, eng, models, col, seed, timed=None):
    """max_steps policy steps with `col` around each; timed: [begin_ms, end_ms] accumulators (device events)."""
    import torch
    start_round(args, eng, seed)
    ev = []
    for _ in range(args.max_steps):
        for g in range(2):
            models[g].act_rollout(eng, g)
        if timed is not None:
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            col.begin()
            e[1].record()
            eng.rollout_policy_step()
            e[2].record()
            col.end()
            e[3].record()
            ev.append(e)
        else:
            col.begin()
            eng.rollout_policy_step()
            col.end()
    torch.cuda.synchronize()
    if timed is not None:
        timed[0] += sum(e[0].elapsed_time(e[1]) for e in ev)
        timed[1] += sum(e[2].elapsed_time(e[3]) for e in ev)


def do_prepare(args):
    import torch
    from mfrl_amd import mf, replay
    _, models, eng = setup(args)
    me = models[0]
    col = me.rollout_collector(eng, 0)
    collect_round(args, eng, models, col, 0)
    n = col.finish()
    eng.rollout_check()
    buf = me.replay_buffer
    c = buf._rows.cols
    use_mf = "prob" in c
    hip = me._hip_net()

    def chain():
        tails = c["tail"][:n].nonzero().reshape(-1)
        _, keep, _ = hip.forward(c["obs"][tails], c["feat"][tails], c["prob"][tails] if use_mf else None,
                                 want_policy=False, want_value=True, want_act=False)
        replay.chain_returns(rew, c["prev"], tails, keep, me.gamma)
        return len(tails)

    def batch():
        rows, counts = buf.batch()
        last = torch.cumsum(counts, 0) - 1
        prob = rows.get("prob")
        _, keep, _ = hip.forward(rows["obs"][last], rows["feat"][last], prob[last] if use_mf else None,
                                 want_policy=False, want_value=True, want_act=False)
        offsets = torch.zeros(len(counts) + 1, dtype=torch.int64, device="cuda")
        offsets[1:] = torch.cumsum(counts, 0)
        mf.mfac_returns(rows["rew"], offsets, keep.float().contiguous(), me.gamma)
        return len(counts)

    with torch.no_grad():
        for pair in range(-1, args.pairs):               # pair -1: warm-up (allocator, kernels), not reported
            for name, fn in (("chain", chain), ("batch", batch)):
                rew = c["rew"][:n].clone()               # the chain path works in place: a fresh copy, off the clock
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                a.record()
                chains = fn()
                b.record()
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                if pair >= 0:
                    emit(args, {"measure": "prepare", "path": name, "pair": pair, "algo": args.algo,
                                "map_size": args.map_size, "envs": args.envs, "max_steps": args.max_steps, "rows": n,
                                "chains": chains, "device_ms": a.elapsed_time(b), "wall_ms": wall})


def do_collector(args):
    from mfrl_amd.algo.tools import EpisodesBuffer, MemoryGroup
    from mfrl_amd.replay import RolloutCollector
    _, models, eng = setup(args)
    me = models[0]
    use_mf = me._use_mf
    act_n = me.num_actions if use_mf else 1
    linked = EpisodesBuffer(use_mean=use_mf)
    linked.prepare(me.view_space, me.feature_space, act_n)
    plain = MemoryGroup(me.view_space, me.feature_space, act_n, 1024, 64, 8, use_mean=use_mf)
    cols = {"linked": RolloutCollector(eng, linked, 0), "unlinked": RolloutCollector(eng, plain, 0)}
    for col in cols.values():                            # warm round: the storage grows to a round's rows
        collect_round(args, eng, models, col, 0)
        col.discard()
    for pair in range(args.pairs):
        for name, col in cols.items():
            t = [0.0, 0.0]
            collect_round(args, eng, models, col, 1 + pair, timed=t)
            rows = col.finish()
            col.mg._rows.clear()
            emit(args, {"measure": "collector", "path": name, "pair": pair, "algo": args.algo, "map_size": args.map_size,
                        "envs": args.envs, "steps": args.max_steps, "rows": rows,
                        "begin_us_per_step": 1e3 * t[0] / args.max_steps, "end_us_per_step": 1e3 * t[1] / args.max_steps})
    eng.rollout_check()


def do_rounds(args):
    base = ["--algo", args.algo, "--map_size", str(args.map_size), "--envs", str(args.envs), "--max_steps",
            str(args.max_steps), "--n_round", "3"]
    for loop, extra in (("play_rollout_episodes", ["--rollout_episodes"]), ("play_batched", [])):
        work = os.path.join(args.work, loop)
        os.makedirs(work, exist_ok=True)
        env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
        out = subprocess.run([sys.executable, "-m", "mfrl_amd.train_battle"] + base + extra + ["--base_dir", work],
                             env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.limit)
        if out.returncode != 0:
            print(out.stdout[-4000:])
            raise SystemExit("train_battle %s exited with %d" % (" ".join(extra), out.returncode))
        k = 0
        for line in out.stdout.splitlines():
            m = re.match(r"\[TIME\] play (\d+) steps x (\d+) envs: ([\d.]+) s \(([\d.e+-]+) agent-steps/s.*train ([\d.]+) s",
                         line)
            if m:
                emit(args, {"measure": "rounds", "command": "train_battle " + " ".join(base + extra), "loop": loop,
                            "round": k, "steps": int(m.group(1)), "envs": int(m.group(2)), "play_s": float(m.group(3)),
                            "agent_steps_per_s": float(m.group(4)), "train_s": float(m.group(5)), "line": line})
                k += 1
        for line in out.stdout.splitlines():
            m = re.match(r"\[TIME\] round (\d+): ([\d.]+) s", line)
            if m:
                emit(args, {"measure": "rounds", "loop": loop, "round": int(m.group(1)), "round_s": float(m.group(2))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="+", choices=["prepare", "collector", "rounds"])
    ap.add_argument("--algo", default="mfac", choices=["ac", "mfac"])
    ap.add_argument("--map_size", type=int, default=40)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--max_steps", type=int, default=100)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--work", default="bench_out/ac_rollout", help="base_dir of the train_battle children")
    ap.add_argument("--limit", type=int, default=240, help="seconds per train_battle child")
    args = ap.parse_args()
    if "rounds" in args.what:                            # children first: this process has not opened the GPU yet
        do_rounds(args)
    if "prepare" in args.what:
        do_prepare(args)
    if "collector" in args.what:
        do_collector(args)


if __name__ == "__main__":
    main()
