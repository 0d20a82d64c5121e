"""What the scorekeeper costs per step of the device rollout loop (mfrl_amd.scoreboard, csrc/score_kernels.hip).

A/B in one process with HIP-event pairs on the engine's stream: the battle_rollout loop (act_rollout for both groups,
rollout_policy_step, RolloutScoreboard.update) against the same loop on the same build with update() skipped (attach
only, so acting and stepping are identical), rounds alternating; beside it one RolloutCollector.end() (k_collect_end +
its advance) per step at the same shape, for scale.  Then the tournament's rate: battle_eval --envs 64 rounds beside
battle_eval --envs 1 rounds of the same pairing (untrained seeded models), the CLI's main() called in this process.

    python scripts/bench_score.py --out profiles/score_ab.jsonl

One JSON line per configuration; times are microseconds per step (median over rounds, each round one event pair).
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mean-field-multi-agent-reinforcement-learning_amd", "python"))


def models_for(algos, map_size, max_steps, precision, seed=3):
    import magent
    import torch
    from mfrl_amd.algo import spawn_ai
    env = magent.GridWorld("battle", map_size=map_size)
    h = env.get_handles()
    torch.manual_seed(seed)
    out = [spawn_ai(a, None, env, h[g], "%s-%d" % (a, g), max_steps, memory_size=1024) for g, a in enumerate(algos)]
    for m in out:
        if precision != "f32":
            m.act_precision = precision
    return env, h, out


def loop_us(eng, models, board, steps, update):
    """One event pair around `steps` steps of the loop; microseconds per step."""
    import torch
    s = eng.torch_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    for _ in range(steps):
        for g in range(2):
            models[g].act_rollout(eng, g)
        eng.rollout_policy_step()
        if update:
            board.update()
    b.record(s)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def ab(args, name, map_size, envs, algos, precision):
    import torch
    from mfrl_amd.algo.play import block_positions
    from mfrl_amd.battle import BattleBatch
    from mfrl_amd.scoreboard import RolloutScoreboard
    _, _, models = models_for(algos, map_size, args.max_steps, precision)
    eng = BattleBatch(map_size, envs, stream=torch.cuda.current_stream())
    eng.rollout_init(list(block_positions(map_size)), max_steps=args.max_steps, eps=0.0, seed=1, stagger=False)
    eng.rollout_policy_observe()
    board = RolloutScoreboard(eng)
    board.attach()
    loop_us(eng, models, board, args.warmup, True)
    with_u, without = [], []
    for r in range(args.rounds):
        for update in ((True, False) if r % 2 == 0 else (False, True)):
            board.attach()                 # (a round without updates leaves the carry behind: start every round afresh)
            (with_u if update else without).append(loop_us(eng, models, board, args.steps, update))
    board.attach()
    eng.rollout_check()
    rec = {"case": name, "map_size": map_size, "envs": envs, "algos": algos, "act_precision": precision,
           "rowcap": eng.rowcap, "steps": args.steps, "rounds": args.rounds,
           "policy_path": eng.rollout_policy_path(),
           "with_update_us": statistics.median(with_u), "without_update_us": statistics.median(without),
           "with_update_all_us": with_u, "without_update_all_us": without}
    rec["difference_us"] = rec["with_update_us"] - rec["without_update_us"]
    # one collector end per step at the same shape, for scale (an MFQ-style MemoryGroup of its own)
    try:
        from mfrl_amd.algo.tools import MemoryGroup
        from mfrl_amd.replay import RolloutCollector
        m = models[0]
        mg = MemoryGroup(m.view_space, m.feature_space, m.num_actions, 1024, 64, args.max_steps, use_mean=True)
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
        rec["collect_end_us"] = statistics.median(ends[1:])
    except Exception as ex:                # (storage for 8192 x 164 rows of views may not be there)
        rec["collect_end_us"] = None
        rec["collect_end_note"] = repr(ex)[:200]
    return rec


def tournament(args):
    """The CLI itself, in this process: battle_eval.main at --eval_envs envs and at one env, same pairing and seed,
    every round timed by a host clock between device synchronisations (the first round of each is the warm-up and is
    left out of the medians).  Agent-steps are exact: the device loop's from the rollout's agent_steps buffer, the one
    env's from the lengths of the action arrays play() hands to set_action."""
    import magent
    import torch
    from mfrl_amd import battle_eval
    from mfrl_amd.algo import tools
    argv = ["--algo", "mfq", "--oppo", "mfac", "--untrained", "--map_size", "40", "--max_steps", str(args.eval_steps),
            "--n_round", str(args.eval_rounds), "--seed", "3"]
    dev, one, acted = [], [], [0]
    real_rollout, real_run, real_set = battle_eval.battle_rollout, tools.Runner.run, magent.GridWorld.set_action

    def timed_rollout(*a, **kw):
        torch.cuda.synchronize()
        t0 = time.time()
        res = real_rollout(*a, **kw)
        torch.cuda.synchronize()
        dev.append({"s": time.time() - t0, "agent_steps": res[4]["agent_steps"], "steps_run": res[4]["steps_run"]})
        return res

    def counting_set(self, handle, actions):
        acted[0] += len(actions)
        return real_set(self, handle, actions)

    def timed_run(self, *a, **kw):
        acted[0] = 0
        torch.cuda.synchronize()
        t0 = time.time()
        info = real_run(self, *a, **kw)
        torch.cuda.synchronize()
        one.append({"s": time.time() - t0, "agent_steps": acted[0]})
        return info

    battle_eval.battle_rollout, tools.Runner.run, magent.GridWorld.set_action = timed_rollout, timed_run, counting_set
    try:
        battle_eval.main(argv + ["--envs", str(args.eval_envs)])
        battle_eval.main(argv + ["--envs", "1"])
    finally:
        battle_eval.battle_rollout, tools.Runner.run, magent.GridWorld.set_action = real_rollout, real_run, real_set

    def rate(rounds):
        return statistics.median(r["agent_steps"] / r["s"] for r in rounds[1:])

    return {"case": "battle_eval_rate", "argv": argv, "envs": args.eval_envs,
            "device_loop_agent_steps_per_s": rate(dev), "one_env_agent_steps_per_s": rate(one),
            "device_loop_rounds": dev, "one_env_rounds": one}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "score_ab.jsonl"))
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--rounds", type=int, default=6)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--max_steps", type=int, default=400)
    p.add_argument("--eval_envs", type=int, default=64)
    p.add_argument("--eval_steps", type=int, default=400)
    p.add_argument("--eval_rounds", type=int, default=4)
    p.add_argument("--skip_big", action="store_true")
    args = p.parse_args()
    cases = [("64 envs 40x40", 40, 64, ["mfq", "mfac"], "f32")]
    if not args.skip_big:
        cases.append(("8192 envs 64x64, MF-AC bf16", 64, 8192, ["mfac", "mfac"], "bf16"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for c in cases:
            rec = ab(args, *c)
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")
            f.flush()
        rec = tournament(args)
        print(json.dumps(rec), flush=True)
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
