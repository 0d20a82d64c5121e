"""The tournament, battle.py (reference root) without TensorFlow: two trained models, which may be different
algorithms, play --n_round evaluation rounds; the last line is the reference's WIN_RATE.

    python -m mfrl_amd.battle_eval --algo mfq --oppo mfac --n_round 50 --idx 1999 1999
    python -m mfrl_amd.battle_eval --algo mfq --oppo mfac --envs 64 --idx 1999 1999     # the device rollout loop
    python -m mfrl_amd.battle_eval --algo mfac --oppo ac --envs 8192 --act_precision bf16 --idx 1999 1999
    python -m mfrl_amd.battle_eval --algo mfq --oppo mfac --envs 64 --watch 0 63 --idx 1999 1999    # + frames of two envs
    python -m mfrl_amd.battle_eval --algo mfq --oppo mfac --envs 64 --explore boltzmann --temperature 0.1 --idx 1999 1999
    python -m mfrl_amd.battle_eval --algo mfq --oppo rush --envs 64 --idx 1999      # against the scripted rush opponent
    python -m mfrl_amd.battle_eval --algo rush --oppo random --envs 64               # two scripted sides: nothing loaded

Models are loaded from <base_dir>/data/models/<algo>-0 and <base_dir>/data/models/<oppo>-1 at the two --idx steps, as
the reference does (train_battle saves them there).  --envs 1 is the reference's path unchanged: tools.Runner with
play.battle and train=False, runner.run(0.0, k, win_cnt=win_cnt).  --envs E > 1 plays every round on the device
rollout loop (play.battle_rollout): E episodes per round, their outcomes kept on the device by
mfrl_amd.scoreboard.RolloutScoreboard with Runner.run's own win rule -- kill[i] = max_nums[i] - nums[1 - i], nums read
before clear_dead; a tie counts for both sides --, so WIN_RATE is over n_round * E episodes.  --watch ENV [ENV ...]
records those envs of the first --watch_rounds rounds on the device (mfrl_amd.recorder), re-runs each one's first episode
on the one-env engine and writes the reference's frame files under <render dir>/round_<k>/env_<e>/.

--algo / --oppo also take the scripted opponents rush and random (mfrl_amd.algo.rule): a fixed yardstick
that loads nothing, so --idx then takes one value per learned side, in order (two, one or none).  --rule_eps is the
share of uniform actions a rush side mixes in (default 0).
"""
import argparse
import math
import os
import time

import torch

import magent

from .algo import spawn_ai, tools
from .algo.play import battle, battle_rollout

ALGOS = ("ac", "mfac", "mfq", "il")
RULES = ("rush", "random")          # the scripted opponents (mfrl_amd.algo.rule): nothing to load


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--algo", type=str, choices=ALGOS + RULES, required=True,
                        help="the main model's algorithm, or a scripted opponent (rush, random)")
    parser.add_argument("--oppo", type=str, choices=ALGOS + RULES,
                        help="the opponent model's algorithm or scripted opponent (default: --algo)")
    parser.add_argument("--n_round", type=int, default=50)
    parser.add_argument("--render", action="store_true")
    parser.add_argument("--map_size", type=int, default=40)
    parser.add_argument("--max_steps", type=int, default=400)
    parser.add_argument("--idx", nargs="*", help="the saved steps of the learned models, one per learned side in order: "
                                                 "A B (a rush / random side loads nothing)")
    parser.add_argument("--envs", type=int, default=1, help="envs per round (>1: the device rollout loop)")
    parser.add_argument("--act_precision", type=str, choices=["f32", "bf16"], default="f32",
                        help="the acting forward's matrix operands on the device rollout loop (mfrl_amd.policy)")
    parser.add_argument("--base_dir", type=str, default=os.getcwd())
    parser.add_argument("--seed", type=int, default=0, help="torch / numpy / python seed (model initialisation, draws)")
    parser.add_argument("--untrained", action="store_true",
                        help="skip load: seeded initial weights (smoke runs and tests)")
    parser.add_argument("--watch", type=int, nargs="+", metavar="ENV",
                        help="with --envs > 1: record these envs (at most 16) on the device rollout loop and write the "
                             "frames of their first episode")
    parser.add_argument("--watch_rounds", type=int, default=1, help="rounds --watch records (the first ones)")
    parser.add_argument("--explore", type=str, choices=["greedy", "boltzmann"], default="greedy",
                        help="how the Q models (mfq / il) of the pairing act: greedy (the reference: argmax q) or boltzmann "
                             "(drawn from softmax(q / --temperature))")
    parser.add_argument("--temperature", type=float, default=None,
                        help="with --explore boltzmann: the temperature, finite and > 0 (default 0.1)")
    parser.add_argument("--mean_field", type=str, choices=["group", "neighbors"], default="group",
                        help="with --envs > 1: the mean action the mean-field models (mfq / mfac) of the pairing are given "
                             "-- group (the reference) or neighbors (the agents of the group within --mf_radius cells)")
    parser.add_argument("--mf_radius", type=int, default=None,
                        help="with --mean_field neighbors: the Chebyshev radius, >= 0 (default 6, the view's)")
    parser.add_argument("--rule_eps", type=float, default=None,
                        help="with a rush side: the probability of a uniform action instead of the rule's, in [0, 1] "
                             "(default 0)")
    args = parser.parse_args(argv)
    if args.oppo is None:
        args.oppo = args.algo
    learned = [i for i, a in enumerate((args.algo, args.oppo)) if a not in RULES]
    if args.rule_eps is not None:
        if "rush" not in (args.algo, args.oppo):
            parser.error("--rule_eps is the exploration of a rush side: neither --algo nor --oppo is rush (random is "
                         "eps = 1)")
        if not 0.0 <= args.rule_eps <= 1.0:
            parser.error("--rule_eps must be in [0, 1]")
    if args.mean_field != "group":
        if args.algo not in ("mfq", "mfac") and args.oppo not in ("mfq", "mfac"):
            parser.error("--mean_field neighbors is the mean action of a mean-field model: neither --algo nor --oppo is "
                         "mfq or mfac")
        if args.envs <= 1:
            parser.error("--mean_field neighbors runs on the device rollout loop: --envs > 1")
    if args.mf_radius is not None:
        if args.mean_field == "group":
            parser.error("--mf_radius is the radius of --mean_field neighbors: give that too")
        if args.mf_radius < 0:
            parser.error("--mf_radius must be >= 0")
    if args.explore != "greedy" and args.algo not in ("mfq", "il") and args.oppo not in ("mfq", "il"):
        parser.error("--explore boltzmann samples from the Q values: neither --algo nor --oppo is mfq or il")
    if args.temperature is not None and args.explore == "greedy":
        parser.error("--temperature is the Boltzmann temperature: give --explore boltzmann too")
    if args.explore != "greedy":
        args.temperature = 0.1 if args.temperature is None else args.temperature
        if not (math.isfinite(args.temperature) and args.temperature > 0):
            parser.error("--temperature must be finite and > 0")
    eps = args.temperature if args.explore != "greedy" else 0.0      # (greedy: the reference's battle() eps)
    if args.n_round < 1:
        parser.error("--n_round must be at least 1")
    if args.envs < 1:
        parser.error("--envs must be at least 1")
    if args.max_steps < 1:
        parser.error("--max_steps must be at least 1")
    if args.untrained and args.idx:
        parser.error("--untrained loads nothing: give it or --idx A B, not both")
    if len(learned) == 2:
        if not args.untrained and (args.idx is None or len(args.idx) != 2):
            parser.error("--idx takes the two saved steps A B (or give --untrained)")
    elif not args.untrained and len(args.idx or []) != len(learned):
        parser.error("--idx takes one saved step per learned side: {} here ({} vs {}; rush / random load nothing), or "
                     "give --untrained".format(len(learned), args.algo, args.oppo))
    if args.render and args.envs > 1:
        parser.error("--render draws one env through the drop-in API: --envs 1")
    if args.act_precision != "f32" and args.envs <= 1:
        parser.error("--act_precision bf16 is the device rollout loop's acting mode: --envs > 1")
    if args.watch is not None:
        from .recorder import check_watch
        if args.envs <= 1:
            parser.error("--watch records envs of the device rollout loop: --envs > 1")
        if args.watch_rounds < 1:
            parser.error("--watch_rounds must be at least 1")
        try:
            check_watch(args.watch, args.envs)
        except ValueError as err:
            parser.error(str(err))

    import random

    import numpy as np
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    random.seed(args.seed)
    env = magent.GridWorld("battle", map_size=args.map_size)
    render_dir = os.path.join(args.base_dir, "examples/battle_model", "build/render")
    env.set_render_dir(render_dir)                                                                # battle.py:41
    handles = env.get_handles()
    main_model_dir = os.path.join(args.base_dir, "data/models/{}-0".format(args.algo))
    oppo_model_dir = os.path.join(args.base_dir, "data/models/{}-1".format(args.oppo))
    # (no round trains: the replay ring of mfq / il stays empty, so it is made small)
    models = [spawn_ai(args.algo, None, env, handles[0], args.algo + "-me", args.max_steps, memory_size=1024),
              spawn_ai(args.oppo, None, env, handles[1], args.oppo + "-opponent", args.max_steps, memory_size=1024)]
    if not args.untrained:
        for i, step in zip(learned, args.idx or []):      # (a rule side loads nothing)
            models[i].load((main_model_dir, oppo_model_dir)[i], step=step)
    if args.rule_eps is not None:
        for m in models:
            if getattr(m, "rule", None) == "rush":
                m.eps = args.rule_eps
    for m in models:
        if args.explore != "greedy" and hasattr(type(m), "explore"):     # (the Q models of the pairing)
            m.explore = args.explore
        if args.mean_field != "group" and getattr(m, "use_mf", getattr(m, "_use_mf", False)):   # (the mean-field models)
            m.mean_field = args.mean_field
            if args.mf_radius is not None:
                m.mf_radius = args.mf_radius
    win_cnt = {"main": 0, "opponent": 0}
    t0 = time.time()
    if args.envs == 1:
        # (battle.py:62 passes render_every=0 whatever --render says; so does this)
        runner = tools.Runner(None, env, handles, args.map_size, args.max_steps, models, battle, render_every=0)
        for k in range(args.n_round):
            runner.run(eps, k, win_cnt=win_cnt)
        episodes = args.n_round
    else:
        from .battle import BattleBatch
        from .scoreboard import RolloutScoreboard
        for m in models:
            if args.act_precision != "f32":
                m.act_precision = args.act_precision
        eng = BattleBatch(args.map_size, args.envs, stream=torch.cuda.current_stream())
        board = RolloutScoreboard(eng, ep_cap=1, target=1)       # one set of buffers for all rounds
        rec = None
        if args.watch is not None:
            from .recorder import RolloutRecorder, replay
            rec = RolloutRecorder(eng, args.watch, args.max_steps)
        steps = 0
        for k in range(args.n_round):
            watching = rec is not None and k < args.watch_rounds
            out = battle_rollout(eng, k, args.map_size, args.max_steps, models, eps=eps, board=board,
                                 recorder=rec if watching else None)[4]
            if watching:         # behind the round: nothing of the one-env engine runs beside the rollout loop
                for j, e in enumerate(args.watch):
                    done = replay(out["trace"], j, render_dir=os.path.join(render_dir, "round_%d" % k), episodes=1)
                    print("[WATCH] round {} env {}: {} steps in {}".format(k, e, done["steps"], done["dir"]))
            first = out["first"]
            win_cnt["main"] += first["main_wins"] + first["ties"]
            win_cnt["opponent"] += first["oppo_wins"] + first["ties"]
            steps += out["steps_run"]
        episodes = args.n_round * args.envs
        torch.cuda.synchronize()
        print("[TIME] {} rounds x {} envs: {:.2f} s, {} steps of every env".format(args.n_round, args.envs,
                                                                                  time.time() - t0, steps))
    print("\n[*] >>> WIN_RATE: [{0}] {1} / [{2}] {3}".format(args.algo, win_cnt["main"] / episodes, args.oppo,
                                                           win_cnt["opponent"] / episodes))
    return win_cnt


if __name__ == "__main__":
    main()
