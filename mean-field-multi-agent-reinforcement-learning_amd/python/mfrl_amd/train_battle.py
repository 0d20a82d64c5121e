"""Self-play training, train_battle.py (reference root) without TensorFlow.

    python -m mfrl_amd.train_battle --algo mfq --n_round 2000 --map_size 40 --max_steps 400
    python -m mfrl_amd.train_battle --algo mfq --envs 256 ...     # batched engine, all in HBM
    python -m mfrl_amd.train_battle --algo mfq --envs 256 --rollout ...   # the device rollout loop (mfq / il)
    python -m mfrl_amd.train_battle --algo mfq --envs 64 --rollout --train_backend hip ...   # + the HIP training step
    python -m mfrl_amd.train_battle --algo mfac --envs 64 --rollout_episodes ...   # the device rollout loop (ac / mfac)
    python -m mfrl_amd.train_battle --algo mfac --envs 64 --rollout_episodes --ac_train_backend hip ...   # + the HIP step
    python -m mfrl_amd.train_battle --algo mfq --envs 64 --rollout --render --watch 0 63 ...   # + frames of two envs
    python -m mfrl_amd.train_battle --algo mfq --envs 64 --rollout --explore boltzmann ...   # sample from softmax(q / eps)
    python -m mfrl_amd.train_battle --algo mfq --envs 64 --rollout --explore boltzmann --target boltzmann ...   # + the paper's v^MF target
    python -m mfrl_amd.train_battle --algo mfq --envs 64 --rollout --mean_field neighbors --mf_radius 6 ...   # the paper's neighbourhood mean action
    python -m mfrl_amd.train_battle --algo mfac --envs 64 --rollout_episodes --advantage gae --gae_lambda 0.95 --adv_norm ...   # GAE(lambda) advantages, normalised per round
    python -m mfrl_amd.train_battle --algo mfac --envs 64 --rollout_episodes --advantage gae --adv_norm --objective ppo --ppo_epochs 4 --ppo_minibatches 4 ...   # + PPO's clipped surrogate, 16 steps per round
    python -m mfrl_amd.train_battle --algo mfq --envs 64 --rollout --eval_every 10 --eval_oppo rush ...   # + a round against the scripted opponent, logged to data/eval_<algo>.jsonl

Same arguments, epsilon schedule (linear_decay) and Runner as the reference; models from
mfrl_amd.algo (PyTorch-ROCm), the env from the drop-in magent (one env) or a BattleBatch (--envs).
Logs go to data/tmp/<algo>.jsonl, models to data/models/<algo>-{0,1}/<algo>_<round>.pt.
"""
import argparse
import math
import os
import time

import torch

import magent

from .algo import spawn_ai, tools
from .algo.play import play, play_batched, play_rollout, play_rollout_episodes


def linear_decay(epoch, x, y):
    """train_battle.py:15-35: piecewise-linear interpolation of y over the breakpoints x."""
    min_v = y[0]
    start = x[0]
    if epoch == start:
        return min_v
    eps = min_v
    for i, x_i in enumerate(x):
        if epoch <= x_i:
            interval = (y[i] - y[i - 1]) / (x_i - x[i - 1])
            eps = interval * (epoch - x[i - 1]) + y[i - 1]
            break
    return eps


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--algo", type=str, choices={"ac", "mfac", "mfq", "il"}, required=True)
    parser.add_argument("--save_every", type=int, default=10)
    parser.add_argument("--update_every", type=int, default=5)
    parser.add_argument("--n_round", type=int, default=2000)
    parser.add_argument("--render", action="store_true")
    parser.add_argument("--map_size", type=int, default=40)
    parser.add_argument("--max_steps", type=int, default=400)
    parser.add_argument("--envs", type=int, default=1, help="envs per round (>1: batched engine in HBM)")
    parser.add_argument("--base_dir", type=str, default=os.getcwd())
    parser.add_argument("--rollout", action="store_true",
                        help="with --envs > 1: act, step and collect replay rows on the device rollout loop (mfq / il)")
    parser.add_argument("--train_backend", type=str, choices=["torch", "hip"], default="torch",
                        help="mfq / il: the minibatch loop on torch autograd (graph replay) or on the hand-written HIP "
                             "training step (mfrl_amd.qtrain)")
    parser.add_argument("--rollout_episodes", action="store_true",
                        help="with --envs > 1: the device rollout loop for ac / mfac -- rows collected with their "
                             "episode chains into the EpisodesBuffer and trained in place")
    parser.add_argument("--act_precision", type=str, choices=["f32", "bf16"], default="f32",
                        help="the acting forward's matrix operands (mfrl_amd.policy: QNetHIP for mfq / il, ACNetHIP "
                             "for ac / mfac); training and the bootstrap values stay f32")
    parser.add_argument("--ac_train_backend", type=str, choices=["torch", "hip"], default="torch",
                        help="ac / mfac: train() / train_rollout() on torch autograd or on the hand-written HIP "
                             "training step (mfrl_amd.actrain), with or without --rollout_episodes")
    parser.add_argument("--watch", type=int, nargs="+", metavar="ENV",
                        help="with --rollout / --rollout_episodes: record these envs (at most 16) on the rounds --render "
                             "marks and write their frames (mfrl_amd.recorder)")
    parser.add_argument("--explore", type=str, choices=["greedy", "boltzmann"], default="greedy",
                        help="mfq / il: how the models act while they play -- greedy (the reference: argmax q, the eps "
                             "schedule unused) or boltzmann (drawn from softmax(q / eps), eps from the schedule)")
    parser.add_argument("--target", type=str, choices=["max", "boltzmann"], default="max",
                        help="mfq / il: what training bootstraps from -- max (the reference: the target net's value of the "
                             "greedy next action) or boltzmann (the paper's mean-field value: the target net's values "
                             "averaged under softmax(q / eps), eps from the schedule); either --train_backend")
    parser.add_argument("--mean_field", type=str, choices=["group", "neighbors"], default="group",
                        help="mfq / mfac with --rollout / --rollout_episodes: the mean action an agent is given -- group "
                             "(the reference: the mean over its whole group) or neighbors (the paper's: the mean over "
                             "the agents of its group within --mf_radius cells of it)")
    parser.add_argument("--mf_radius", type=int, default=None,
                        help="with --mean_field neighbors: the Chebyshev radius, >= 0 (default 6, the view's)")
    parser.add_argument("--advantage", type=str, choices=["returns", "gae"], default="returns",
                        help="ac / mfac with --rollout_episodes: the advantage of the policy term -- returns (the "
                             "reference: the bootstrapped discounted return minus the value) or gae (GAE(lambda) along "
                             "each agent's episode chain, from the values of all rows)")
    parser.add_argument("--gae_lambda", type=float, default=None,
                        help="with --advantage gae: lambda in [0, 1] (default 0.95)")
    parser.add_argument("--adv_norm", action="store_true",
                        help="with --advantage gae: normalise a round's advantages to zero mean and unit deviation")
    parser.add_argument("--objective", type=str, choices=["pg", "ppo"], default="pg",
                        help="ac / mfac with --rollout_episodes and --advantage gae: the policy term -- pg (the reference: "
                             "one gradient and one Adam step per round) or ppo (the clipped surrogate, --ppo_epochs passes "
                             "of --ppo_minibatches steps per round)")
    parser.add_argument("--ppo_clip", type=float, default=None,
                        help="with --objective ppo: the ratio's clip range, finite and > 0 (default 0.2)")
    parser.add_argument("--ppo_epochs", type=int, default=None,
                        help="with --objective ppo: passes over a round's rows, >= 1 (default 4)")
    parser.add_argument("--ppo_minibatches", type=int, default=None,
                        help="with --objective ppo: contiguous segments (Adam steps) per pass, >= 1 (default 4)")
    parser.add_argument("--ppo_target_kl", type=float, default=None,
                        help="with --objective ppo: start no further pass once a pass's mean approximate KL exceeds this "
                             "(finite, >= 0; default: no such stop, and nothing read back inside the step loop)")
    parser.add_argument("--eval_every", type=int, default=0,
                        help="after every K-th round play one evaluation round of the main model against a scripted "
                             "opponent on the device rollout loop and log the outcome (0: off)")
    parser.add_argument("--eval_oppo", type=str, choices=["rush", "random"], default=None,
                        help="with --eval_every: the scripted opponent (mfrl_amd.algo.rule; default rush)")
    parser.add_argument("--eval_envs", type=int, default=64, help="with --eval_every: envs (episodes) per evaluation round")
    parser.add_argument("--eval_eps", type=float, default=None,
                        help="with --eval_every and the rush opponent: its share of uniform actions, in [0, 1] (default 0)")
    args = parser.parse_args(argv)
    if args.eval_every < 0:
        parser.error("--eval_every must be >= 0")
    if args.eval_every == 0:
        if args.eval_oppo is not None or args.eval_eps is not None:
            parser.error("--eval_oppo / --eval_eps describe the evaluation rounds: give --eval_every K too")
    else:
        args.eval_oppo = args.eval_oppo or "rush"
        if args.eval_envs < 1:
            parser.error("--eval_envs must be at least 1")
        if args.eval_eps is not None:
            if args.eval_oppo != "rush":
                parser.error("--eval_eps is the exploration of the rush opponent (random is eps = 1)")
            if not 0.0 <= args.eval_eps <= 1.0:
                parser.error("--eval_eps must be in [0, 1]")
    if args.mean_field != "group":
        if args.algo not in ("mfq", "mfac"):
            parser.error("--mean_field neighbors is the mean action of a mean-field model: --algo mfq or mfac (ac / il "
                         "read no mean action)")
        if not (args.rollout or args.rollout_episodes):
            parser.error("--mean_field neighbors runs on the device rollout loops: --rollout (mfq) or --rollout_episodes "
                         "(mfac)")
    if args.mf_radius is not None:
        if args.mean_field == "group":
            parser.error("--mf_radius is the radius of --mean_field neighbors: give that too")
        if args.mf_radius < 0:
            parser.error("--mf_radius must be >= 0")
    if args.advantage != "returns":
        if args.algo not in ("ac", "mfac"):
            parser.error("--advantage gae is the advantage of an actor-critic model: --algo ac or mfac (mfq / il train on "
                         "their Q targets)")
        if not args.rollout_episodes:
            parser.error("--advantage gae runs on the device rollout loop: give --rollout_episodes")
    if args.gae_lambda is not None:
        if args.advantage != "gae":
            parser.error("--gae_lambda is the lambda of --advantage gae: give that too")
        if not 0.0 <= args.gae_lambda <= 1.0:
            parser.error("--gae_lambda must be in [0, 1]")
    if args.adv_norm and args.advantage != "gae":
        parser.error("--adv_norm normalises the advantages of --advantage gae: give that too")
    if args.objective != "pg":
        if args.algo not in ("ac", "mfac"):
            parser.error("--objective ppo is the policy term of an actor-critic model: --algo ac or mfac (mfq / il train "
                         "on their Q targets)")
        if not args.rollout_episodes:
            parser.error("--objective ppo runs on the device rollout loop: give --rollout_episodes")
        if args.advantage != "gae":
            parser.error("--objective ppo reads the advantage column of --advantage gae: give that too")
    ppo_flags = {"--ppo_clip": args.ppo_clip, "--ppo_epochs": args.ppo_epochs, "--ppo_minibatches": args.ppo_minibatches,
                 "--ppo_target_kl": args.ppo_target_kl}
    for flag, value in ppo_flags.items():
        if value is not None and args.objective != "ppo":
            parser.error("%s describes --objective ppo: give that too" % flag)
    if args.ppo_clip is not None and not (math.isfinite(args.ppo_clip) and args.ppo_clip > 0.0):
        parser.error("--ppo_clip must be finite and > 0")
    if args.ppo_epochs is not None and args.ppo_epochs < 1:
        parser.error("--ppo_epochs must be >= 1")
    if args.ppo_minibatches is not None and args.ppo_minibatches < 1:
        parser.error("--ppo_minibatches must be >= 1")
    if args.ppo_target_kl is not None and not (math.isfinite(args.ppo_target_kl) and args.ppo_target_kl >= 0.0):
        parser.error("--ppo_target_kl must be finite and >= 0")
    if args.target != "max" and args.algo not in ("mfq", "il"):
        parser.error("--target boltzmann bootstraps from the Q values: --algo mfq or il (ac / mfac train on their "
                     "returns)")
    if args.explore != "greedy" and args.algo not in ("mfq", "il"):
        parser.error("--explore boltzmann samples from the Q values: --algo mfq or il (ac / mfac sample from their "
                     "policy already)")
    if args.ac_train_backend == "hip" and args.algo not in ("ac", "mfac"):
        parser.error("--ac_train_backend hip trains the actor-critic network: --algo ac or mfac (mfq / il: "
                     "--train_backend hip)")
    if args.rollout_episodes:
        if args.rollout:
            parser.error("--rollout_episodes and --rollout are two loops (ac / mfac and mfq / il): give one")
        if args.algo not in ("ac", "mfac"):
            parser.error("--rollout_episodes collects into an EpisodesBuffer: --algo ac or mfac (mfq / il: --rollout)")
        if args.envs <= 1:
            parser.error("--rollout_episodes needs the batched engine: --envs > 1")
        if args.train_backend == "hip":
            parser.error("--rollout_episodes trains ac / mfac on torch autograd; --train_backend hip trains the Q network")
    if args.train_backend == "hip" and args.algo not in ("mfq", "il"):
        parser.error("--train_backend hip trains the Q network: --algo mfq or il")
    if args.rollout and args.envs <= 1:
        parser.error("--rollout needs the batched engine: --envs > 1")
    if args.rollout and args.algo not in ("mfq", "il"):
        parser.error("--rollout collects into a MemoryGroup: --algo mfq or il (ac / mfac train from an EpisodesBuffer: "
                     "--rollout_episodes)")
    if args.watch is not None:
        from .recorder import check_watch
        if not (args.rollout or args.rollout_episodes):
            parser.error("--watch records envs of the device rollout loop: --rollout or --rollout_episodes")
        try:
            check_watch(args.watch, args.envs)
        except ValueError as err:
            parser.error(str(err))
        if not args.render:
            parser.error("--watch writes frames on the rounds --render marks: give --render too")

    env = magent.GridWorld("battle", map_size=args.map_size)
    render_dir = os.path.join(args.base_dir, "examples/battle_model", "build/render")
    env.set_render_dir(render_dir)                                                            # train_battle.py:87
    handles = env.get_handles()
    log_dir = os.path.join(args.base_dir, "data/tmp")
    model_dir = os.path.join(args.base_dir, "data/models/{}".format(args.algo))
    # the reference's 80000 replay rows are sized for one env; with E envs keep E times as many
    # (capped at 2M rows = 9.5 GB of views in HBM)
    memory = min(80000 * args.envs, 2000000)
    models = [spawn_ai(args.algo, None, env, handles[0], args.algo + "-me", args.max_steps, memory_size=memory),
              spawn_ai(args.algo, None, env, handles[1], args.algo + "-opponent", args.max_steps, memory_size=memory)]
    for m in models:
        if args.train_backend != "torch":
            m.train_backend = args.train_backend
        if args.ac_train_backend != "torch":
            m.train_backend = args.ac_train_backend
        if args.act_precision != "f32":
            m.act_precision = args.act_precision
        if args.explore != "greedy":
            m.explore = args.explore
        if args.target != "max":
            m.target_rule = args.target
        if args.mean_field != "group":
            m.mean_field = args.mean_field
            if args.mf_radius is not None:
                m.mf_radius = args.mf_radius
        if args.advantage != "returns":
            m.advantage = args.advantage
            if args.gae_lambda is not None:
                m.gae_lambda = args.gae_lambda
            if args.adv_norm:
                m.adv_norm = True
        if args.objective != "pg":
            m.objective = args.objective
            for name in ("ppo_clip", "ppo_epochs", "ppo_minibatches", "ppo_target_kl"):
                if getattr(args, name) is not None:
                    setattr(m, name, getattr(args, name))
    play_handle = play
    if args.envs > 1:
        from .battle import BattleBatch
        eng = BattleBatch(args.map_size, args.envs, stream=torch.cuda.current_stream())
        rec = None
        if args.watch is not None:
            from .recorder import RolloutRecorder, replay
            rec = RolloutRecorder(eng, args.watch, args.max_steps)

        def play_handle(env, n_round, map_size, max_steps, handles, models, print_every, eps=1.0, render=False,
                        train=False):
            loop = (play_rollout if args.rollout else play_rollout_episodes if args.rollout_episodes
                    else play_batched)
            if rec is None or not render:
                return loop(eng, n_round, map_size, max_steps, models, print_every, eps, train)
            res = loop(eng, n_round, map_size, max_steps, models, print_every, eps, train, recorder=rec)
            for j, e in enumerate(args.watch):       # behind the round: nothing of it runs beside the rollout loop
                done = replay(rec.trace, j, render_dir=os.path.join(render_dir, "round_%d" % n_round))
                print("[WATCH] round {} env {}: {} steps, {} episodes in {}".format(n_round, e, done["steps"],
                                                                                    done["episodes"], done["dir"]))
            return res
    runner = tools.Runner(None, env, handles, args.map_size, args.max_steps, models, play_handle,
                          render_every=args.save_every if args.render else 0, save_every=args.save_every, tau=0.01,
                          log_name=args.algo, log_dir=log_dir, model_dir=model_dir, train=True)
    evaluate = _evaluator(args, env, handles, models[0]) if args.eval_every else None
    for k in range(args.n_round):
        eps = linear_decay(k, [0, int(args.n_round * 0.8), args.n_round], [1, 0.2, 0.1])
        t0 = time.time()
        runner.run(eps, k)
        torch.cuda.synchronize()
        print("[TIME] round {}: {:.2f} s ({} envs)".format(k, time.time() - t0, args.envs))
        if evaluate is not None and (k + 1) % args.eval_every == 0:
            evaluate(k)


def _evaluator(args, env, handles, model):
    """--eval_every: evaluate(k) plays one battle_rollout round of `model` (group 0) against the scripted opponent on
    its own BattleBatch and scoreboard (made once here), prints the [EVAL] line and appends it as JSON to
    <base_dir>/data/eval_<algo>.jsonl.  The model acts as battle_eval's default does -- the Q models greedily, the
    actor-critic ones sampling -- and is left as it was: its explore, temperature and draw counter are restored, no
    host random stream is consumed (left_id is k % 2), and nothing is trained or collected."""
    import json

    from .algo.play import battle_rollout
    from .battle import BattleBatch
    from .scoreboard import RolloutScoreboard
    oppo = spawn_ai(args.eval_oppo, None, env, handles[1], "eval-" + args.eval_oppo, args.max_steps)
    if args.eval_eps is not None:
        oppo.eps = args.eval_eps
    eng = BattleBatch(args.map_size, args.eval_envs, stream=torch.cuda.current_stream())
    board = RolloutScoreboard(eng, ep_cap=1, target=1)
    path = os.path.join(args.base_dir, "data", "eval_{}.jsonl".format(args.algo))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    kept = [a for a in ("explore", "temperature", "_draws") if hasattr(model, a)]

    def evaluate(k):
        saved = {a: getattr(model, a) for a in kept}
        try:
            if "explore" in saved:
                model.explore = "greedy"
            first = battle_rollout(eng, k, args.map_size, args.max_steps, [model, oppo], eps=0.0, left_id=k % 2,
                                   board=board)[4]["first"]
        finally:
            for a, v in saved.items():
                setattr(model, a, v)
        E = args.eval_envs
        rec = {"round": k, "oppo": args.eval_oppo, "envs": E,
               "win_rate": [(first["main_wins"] + first["ties"]) / E, (first["oppo_wins"] + first["ties"]) / E],
               "kills": first["kills"], "steps": first["steps"]}
        print("[EVAL] round {} vs {}: WIN_RATE {} / {}, kills {} / {}".format(k, args.eval_oppo, rec["win_rate"][0],
                                                                             rec["win_rate"][1], rec["kills"][0],
                                                                             rec["kills"][1]))
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")

    return evaluate


if __name__ == "__main__":
    main()
