"""The training-loop drivers of examples/battle_model/senario_battle.py, restated.

* generate_map / play / battle: the reference's single-env loop (senario_battle.py:8-37, 55-185)
  on the drop-in magent.GridWorld, with any of this package's models (numpy in and out, as there).
* play_batched: the same loop over E envs of a BattleBatch, everything in HBM -- observations go
  from the engine's buffers straight into the policy forward, actions straight back into
  set_action, and the replay rows into the device MemoryGroup / EpisodesBuffer (SURVEY.md 8(f)
  rows 1-2).  Agent keys in the buffers are env * cap + id.
* play_rollout: a round on the device rollout loop (act_rollout + rollout_policy_step, no host round trip
  per step), the replay rows collected by mfrl_amd.replay.RolloutCollector (DQN / MFQ).
* play_rollout_episodes: the same round for ActorCritic / MFAC -- the rows go into the model's EpisodesBuffer with
  their episode chains (the collector's linked path) and train_rollout() trains on them in place.
* battle_rollout: an evaluation round (battle) on the device rollout loop for any pairing of models with act_rollout,
  the outcomes of the episodes kept on the device by mfrl_amd.scoreboard.RolloutScoreboard.
* A model whose mean_field is "neighbors" (MFQ / MFAC, opt-in) gets the paper's neighbourhood mean action on the three
  device-loop rounds -- one row per agent from mfrl_amd.mf.NeighborMean in place of the group's mean, for acting and in
  the collected rows; the host loops (play, play_batched) refuse such a model.
* The three device-loop rounds take recorder=: a mfrl_amd.recorder.RolloutRecorder that records a few watched envs, to
  be re-run and rendered behind the round (mfrl_amd.recorder.replay).
"""
import math
import random
import time

import numpy as np
import torch

from .. import mf
from ..battle import GET_ALIVE, GET_ID, GET_NUM, GET_REWARD


def block_positions(map_size, side_gap=3):
    """The two square blocks of generate_map (stride 2, init_num = 0.04 * map_size^2 per side)."""
    width = height = map_size
    side = int(math.sqrt(map_size * map_size * 0.04)) * 2
    left = [[x, y, 0] for x in range(width // 2 - side_gap - side, width // 2 - side_gap, 2)
            for y in range((height - side) // 2, (height - side) // 2 + side, 2)]
    right = [[x, y, 0] for x in range(width // 2 + side_gap, width // 2 + side_gap + side, 2)
             for y in range((height - side) // 2, (height - side) // 2 + side, 2)]
    return left, right


def generate_map(env, map_size, handles):
    left, right = block_positions(map_size)
    left_id = random.randint(0, 1)
    env.add_agents(handles[left_id], method="custom", pos=left)
    env.add_agents(handles[1 - left_id], method="custom", pos=right)


def _one_hot_mean(acts, n_action):
    return np.mean(list(map(lambda x: np.eye(n_action)[x], acts)), axis=0, keepdims=True)


def _refuse_neighbors(name, models):
    """The host loops feed every agent its group's mean (the reference's loop): a model that asks for the
    neighbourhood mean is refused, not served the other definition quietly."""
    for m in models:
        if getattr(m, "mean_field", "group") != "group":
            raise ValueError("%s: %s has mean_field %r, which only the device rollout loops (play_rollout, "
                             "play_rollout_episodes, battle_rollout) provide" % (name, type(m).__name__, m.mean_field))


def play(env, n_round, map_size, max_steps, handles, models, print_every, eps=1.0, render=False, train=False):
    """One round of self-play on one env (senario_battle.py:55-185)."""
    _refuse_neighbors("play", models)
    env.reset()
    generate_map(env, map_size, handles)
    step_ct, done, n_group = 0, False, len(handles)
    state, acts, ids = [None] * n_group, [None] * n_group, [None] * n_group
    alives, rewards = [None] * n_group, [None] * n_group
    nums = [env.get_num(h) for h in handles]
    max_nums = nums.copy()
    n_action = [env.get_action_space(handles[0])[0], env.get_action_space(handles[1])[0]]
    print("\n\n[*] ROUND #{0}, EPS: {1:.2f} NUMBER: {2}".format(n_round, eps, nums))
    mean_rewards = [[] for _ in range(n_group)]
    total_rewards = [[] for _ in range(n_group)]
    former_act_prob = [np.zeros((1, n_action[0])), np.zeros((1, n_action[1]))]
    while not done and step_ct < max_steps:
        for i in range(n_group):
            state[i] = list(env.get_observation(handles[i]))
            ids[i] = env.get_agent_id(handles[i])
        for i in range(n_group):
            former_act_prob[i] = np.tile(former_act_prob[i], (len(state[i][0]), 1))
            acts[i] = models[i].act(state=state[i], prob=former_act_prob[i], eps=eps)
        for i in range(n_group):
            env.set_action(handles[i], acts[i])
        done = env.step()
        for i in range(n_group):
            rewards[i] = env.get_reward(handles[i])
            alives[i] = env.get_alive(handles[i])
        buffer = {"state": state[0], "acts": acts[0], "rewards": rewards[0], "alives": alives[0], "ids": ids[0],
                  "prob": former_act_prob[0]}
        for i in range(n_group):
            former_act_prob[i] = _one_hot_mean(acts[i], n_action[i])
        if train:
            models[0].flush_buffer(**buffer)
        nums = [env.get_num(h) for h in handles]
        for i in range(n_group):
            sum_reward = sum(rewards[i])
            rewards[i] = sum_reward / nums[i]
            mean_rewards[i].append(rewards[i])
            total_rewards[i].append(sum_reward)
        if render:
            env.render()
        env.clear_dead()
        info = {"Ave-Reward": np.round(rewards, decimals=6), "NUM": nums}
        step_ct += 1
        if step_ct % print_every == 0:
            print("> step #{}, info: {}".format(step_ct, info))
    if train:
        models[0].train()
    for i in range(n_group):
        mean_rewards[i] = sum(mean_rewards[i]) / len(mean_rewards[i])
        total_rewards[i] = sum(total_rewards[i])
    return max_nums, nums, mean_rewards, total_rewards


def battle(env, n_round, map_size, max_steps, handles, models, print_every, eps=1.0, render=False, train=False):
    """Evaluation round (senario_battle.py:188-263): play without buffers or training."""
    return play(env, n_round, map_size, max_steps, handles, models, print_every, eps, render, train=False)


def play_batched(eng, n_round, map_size, max_steps, models, print_every=50, eps=1.0, train=False, left_id=None):
    """One round on all E envs of `eng` (a BattleBatch), device-resident end to end.

    Returns (max_nums, nums, mean_rewards, total_rewards) summed over envs, like play()."""
    _refuse_neighbors("play_batched", models)
    E, G = eng.n_envs, 2
    eng.reset()
    left, right = block_positions(map_size)
    left_id = random.randint(0, 1) if left_id is None else left_id
    eng.add_agents(left_id, left)
    eng.add_agents(1 - left_id, right)
    rowcap = max(eng.capacity(g) for g in range(G))
    rowcap = (rowcap + 3) & ~3
    v_shape = tuple(models[0].view_space)
    f_shape = tuple(models[0].feature_space)
    n_action = [m.num_actions for m in models]
    key_stride = max(eng.capacity(g) for g in range(G)) * G + 1
    dev = "cuda"
    view = [torch.empty((E, rowcap) + v_shape, device=dev) for _ in range(G)]
    feat = [torch.empty((E, rowcap) + f_shape, device=dev) for _ in range(G)]
    nums_t = [torch.empty(E, dtype=torch.int32, device=dev) for _ in range(G)]
    ids_t = [torch.empty(E * rowcap, dtype=torch.int32, device=dev) for _ in range(G)]
    acts_t = [torch.zeros(E * rowcap, dtype=torch.int32, device=dev) for _ in range(G)]
    rew_t = [torch.empty(E * rowcap, dtype=torch.float32, device=dev) for _ in range(G)]
    alive_t = [torch.empty(E * rowcap, dtype=torch.uint8, device=dev) for _ in range(G)]
    done_t = torch.zeros(E, dtype=torch.int32, device=dev)
    finished = torch.zeros(E, dtype=torch.bool, device=dev)
    former = [torch.zeros((E, n_action[g]), dtype=torch.float32, device=dev) for g in range(G)]
    rows = torch.arange(rowcap, device=dev)
    env_of_row = torch.arange(E, device=dev).repeat_interleave(rowcap)
    for g in range(G):
        eng.get(g, GET_NUM, nums_t[g], rowcap)
    max_nums = [int(nums_t[g].sum().item()) for g in range(G)]
    nums = list(max_nums)
    print("\n\n[*] ROUND #{0}, EPS: {1:.2f} NUMBER: {2} ({3} envs)".format(n_round, eps, nums, E))
    mean_rewards = [[] for _ in range(G)]
    total_rewards = [[] for _ in range(G)]
    step_ct = 0
    t_play = time.time()
    agent_steps = 0
    while step_ct < max_steps and not bool(finished.all().item()):
        valid = []
        for g in range(G):
            eng.observe(g, view[g], feat[g], rowcap)
            eng.get(g, GET_NUM, nums_t[g], rowcap)
            eng.get(g, GET_ID, ids_t[g], rowcap)
            valid.append(((rows[None, :] < nums_t[g][:, None].long()) & ~finished[:, None]).reshape(-1))
        for g in range(G):
            sel = valid[g].nonzero().reshape(-1)
            prob = former[g][env_of_row[sel]]
            a = models[g].act_dev(state=[view[g].reshape((-1,) + v_shape)[sel], feat[g].reshape((-1,) + f_shape)[sel]],
                                  prob=prob, eps=eps)
            acts_t[g].zero_()
            acts_t[g][sel] = a
            eng.set_action(g, acts_t[g], rowcap)
        eng.step(done_t)
        for g in range(G):
            eng.get(g, GET_REWARD, rew_t[g], rowcap)
            eng.get(g, GET_ALIVE, alive_t[g], rowcap)
        sel0 = valid[0].nonzero().reshape(-1)
        agent_steps += int(valid[0].sum().item()) + int(valid[1].sum().item())
        if train:
            keys = env_of_row[sel0].long() * key_stride + ids_t[0][sel0].long()
            models[0].flush_buffer(state=[view[0].reshape((-1,) + v_shape)[sel0], feat[0].reshape((-1,) + f_shape)[sel0]],
                                   acts=acts_t[0][sel0], rewards=rew_t[0][sel0], alives=alive_t[0][sel0].bool(),
                                   ids=keys, prob=former[0][env_of_row[sel0]])
        for g in range(G):        # former_act_prob: mean one-hot over the env's agents (HIP kernel)
            counts = torch.where(finished, torch.zeros_like(nums_t[g]), nums_t[g])
            former[g] = mf.mean_action(acts_t[g].reshape(E, rowcap), counts, n_action[g]).float()
            former[g] = torch.nan_to_num(former[g], nan=0.0)
        for g in range(G):
            live = valid[g]
            sum_reward = float(rew_t[g][live].sum().item())
            n = int(live.sum().item())
            mean_rewards[g].append(sum_reward / max(n, 1))
            total_rewards[g].append(sum_reward)
        nums = [int(nums_t[g][~finished].sum().item()) for g in range(G)]
        eng.clear_dead()
        finished |= done_t.bool()
        step_ct += 1
        if step_ct % print_every == 0:
            print("> step #{}, Ave-Reward: {}, NUM: {}".format(step_ct, np.round([m[-1] for m in mean_rewards], 6), nums))
    torch.cuda.synchronize()
    t_play = time.time() - t_play
    t_train = time.time()
    if train:
        models[0].train()
        torch.cuda.synchronize()
    print("[TIME] play {} steps x {} envs: {:.2f} s ({:.3g} agent-steps/s incl. policy forward); train {:.2f} s"
          .format(step_ct, E, t_play, agent_steps / max(t_play, 1e-9), time.time() - t_train))
    for g in range(G):
        mean_rewards[g] = sum(mean_rewards[g]) / max(len(mean_rewards[g]), 1)
        total_rewards[g] = sum(total_rewards[g])
    return max_nums, nums, mean_rewards, total_rewards


def play_rollout(eng, n_round, map_size, max_steps, models, print_every=50, eps=1.0, train=False, left_id=None,
                 recorder=None):
    """One round of max_steps steps on all E envs of `eng` on the device rollout loop: ValueNet.act_rollout for both
    groups, BattleBatch.rollout_policy_step, and -- with train -- group 0's replay rows collected by a
    mfrl_amd.replay.RolloutCollector around every step, then models[0].train().  No host synchronisation inside
    the loop.  Q-learning models only (DQN, MFQ: a MemoryGroup replay buffer); others are refused.

    Unlike play_batched, which idles an env once it is done, an env that ends early (done, or max_steps steps into
    its episode) restarts inside the loop from the same placement and keeps producing rows: every round is exactly
    max_steps steps of every env.  The greedy policy does not use eps (as in play_batched); a model with
    explore = "boltzmann" samples at temperature eps (ValueNet.act_rollout).

    Returns (max_nums, nums, mean_rewards, total_rewards) summed over envs like play_batched, computed once at the
    end from the rollout's stats, episode_return and group_num buffers: total_rewards[g] is the return of every
    episode of the round (finished or running); mean_rewards[g] is that per agent-step, both groups' agent-steps
    counted evenly (the engine counts agent-steps per env, not per group)."""
    from ..replay import RolloutCollector
    from .tools import MemoryGroup
    E, G = eng.n_envs, 2
    for m in models[:G]:
        if not hasattr(m, "act_rollout"):
            raise TypeError("play_rollout: %s has no device rollout forward (DQN / MFQ only)" % type(m).__name__)
    if train and not isinstance(getattr(models[0], "replay_buffer", None), MemoryGroup):
        raise TypeError("play_rollout: %s does not train from a MemoryGroup (DQN / MFQ only; EpisodesBuffer "
                        "consumes host randomness per push -- play_rollout_episodes trains AC / MFAC)"
                        % type(models[0]).__name__)

    def collector():
        col = getattr(models[0], "_rollout_collector", None)
        if col is None or col.eng is not eng or col.mg is not models[0].replay_buffer:
            col = models[0]._rollout_collector = RolloutCollector(eng, models[0].replay_buffer, 0)
        return col

    return _rollout_round("play_rollout", eng, n_round, map_size, max_steps, models, eps, train, left_id, collector,
                          models[0].train, recorder)


def play_rollout_episodes(eng, n_round, map_size, max_steps, models, print_every=50, eps=1.0, train=False, left_id=None,
                          recorder=None):
    """play_rollout for the actor-critic models (ActorCritic, MFAC: act_rollout and an EpisodesBuffer): the same
    round -- max_steps steps of every env on the device rollout loop, an env that ends early restarting inside the
    loop, the statistics read once at the end from the rollout's buffers -- with group 0's rows collected into
    models[0]'s EpisodesBuffer by a linked RolloutCollector and trained by models[0].train_rollout().

    An agent's sequence ends at its death, at the end of its episode (done or the step cap) or at the end of the
    round, and every sequence is bootstrapped from the value of its last row, as the reference's loop and
    ActorCritic.train do for every agent.  No np.random is consumed: the reference's per-push permutation only orders
    the agents inside the batch, which changes the float summation order of the loss means and nothing else.
    A MemoryGroup model (DQN / MFQ) is refused: play_rollout is its loop."""
    from .tools import EpisodesBuffer
    for m in models[:2]:
        if not hasattr(m, "act_rollout"):
            raise TypeError("play_rollout_episodes: %s has no device rollout forward" % type(m).__name__)
    if not (isinstance(getattr(models[0], "replay_buffer", None), EpisodesBuffer) and hasattr(models[0], "train_rollout")):
        raise TypeError("play_rollout_episodes: %s does not train from an EpisodesBuffer (AC / MFAC only; play_rollout "
                        "trains DQN / MFQ)" % type(models[0]).__name__)
    return _rollout_round("play_rollout_episodes", eng, n_round, map_size, max_steps, models, eps, train, left_id,
                          lambda: models[0].rollout_collector(eng, 0), models[0].train_rollout, recorder)


def _act_rollout(model, eng, g, eps, nm=None):
    """model.act_rollout for one group of a device-loop round: a model that explores (ValueNet.explore other than
    "greedy") gets the round's eps as its temperature; every other model is called as it always was.  A model that
    trains on the Boltzmann target (ValueNet.target_rule) records the round's eps even while it acts greedily, as
    act_dev records it: its training reads model.temperature.  nm: the group's NeighborMean when the model's
    mean_field is "neighbors" (its rows are the mean action per agent), else None: exactly the calls above."""
    if getattr(model, "target_rule", "max") != "max":
        model.temperature = eps
    kw = {"prob_rows": nm.rows} if nm is not None else {}
    if getattr(model, "explore", "greedy") != "greedy":
        model.act_rollout(eng, g, eps=eps, **kw)
    else:
        model.act_rollout(eng, g, **kw)


def _neighbor_means(eng, models, G=2):
    """Per group: the mfrl_amd.mf.NeighborMean of a model whose mean_field is "neighbors" (made once and kept on the
    model while the engine's layout, the group and the radius stay the same), None for a model left at "group".
    Call it behind rollout_init: the rows have the rollout's rowcap."""
    out = [None] * G
    for g, m in enumerate(models[:G]):
        if getattr(m, "mean_field", "group") != "neighbors":
            continue
        kept = m.__dict__.setdefault("_neighbor_means", {})
        if g not in kept or not kept[g].matches(eng, g, m.mf_radius):
            kept[g] = mf.NeighborMean(eng, g, m.mf_radius)
        out[g] = kept[g]
    return out


def _rollout_round(name, eng, n_round, map_size, max_steps, models, eps, train, left_id, collector, train_fn,
                   recorder=None):
    """The round of play_rollout / play_rollout_episodes: collector() gives group 0's RolloutCollector, train_fn()
    trains models[0] on what it collected.  recorder: a mfrl_amd.recorder.RolloutRecorder of `eng` that records its
    watched envs over the round (one more launch per step; recorder.trace holds the round's trace afterwards), or None."""
    E, G = eng.n_envs, 2
    left, right = block_positions(map_size)
    left_id = random.randint(0, 1) if left_id is None else left_id
    placement = [None, None]
    placement[left_id], placement[1 - left_id] = left, right
    eng.reset()
    eng.rollout_init(placement, max_steps=max_steps, eps=0.0, seed=n_round, stagger=False)
    if eng.rollout_policy_path() is None:
        raise RuntimeError("%s: this rollout plan takes no learned policy (MFX_ROLLOUT_PIPE=1)" % name)
    eng.rollout_policy_observe()
    nms = _neighbor_means(eng, models, G)
    for nm in nms:
        if nm is not None:
            nm.reset()
    col = collector() if train else None
    if col is not None:
        col.prob_rows = nms[0].rows if nms[0] is not None else None
    if recorder is not None:
        recorder.attach(map_size, max_steps, placement)
    max_nums = [len(placement[g]) * E for g in range(G)]
    print("\n\n[*] ROUND #{0}, EPS: {1:.2f} NUMBER: {2} ({3} envs, device rollout)".format(n_round, eps, max_nums, E))
    t_play = time.time()
    for step_ct in range(max_steps):
        for g in range(G):
            _act_rollout(models[g], eng, g, eps, nms[g])
        if col is not None:
            col.begin()
        eng.rollout_policy_step()
        if col is not None:
            col.end()
        for nm in nms:                      # behind col.end(): the rows collected are those the policy acted with
            if nm is not None:
                nm.update()
        if recorder is not None:
            recorder.update()
    rows = col.finish() if col is not None else 0
    if recorder is not None:
        recorder.finish()
    eng.rollout_check()
    t_play = time.time() - t_play
    stats = torch.empty((E, 4), dtype=torch.float64, device="cuda")
    ret = torch.empty((E, G), dtype=torch.float32, device="cuda")
    num = torch.empty((E, G), dtype=torch.int32, device="cuda")
    steps = torch.empty(E, dtype=torch.int64, device="cuda")
    for name, buf in (("stats", stats), ("episode_return", ret), ("group_num", num), ("agent_steps", steps)):
        eng.rollout_copy(name, buf)
    eng.sync()
    agent_steps = int(steps.sum().item())
    nums = [int(x) for x in num.sum(0).tolist()]
    total_rewards = [float(stats[:, 1 + g].sum().item()) + float(ret[:, g].double().sum().item()) for g in range(G)]
    mean_rewards = [total_rewards[g] / max(agent_steps / G, 1.0) for g in range(G)]
    t_train = time.time()
    if train:
        train_fn()
        torch.cuda.synchronize()
    print("[TIME] play {} steps x {} envs: {:.2f} s ({:.3g} agent-steps/s incl. policy forward); train {:.2f} s"
          .format(max_steps, E, t_play, agent_steps / max(t_play, 1e-9), time.time() - t_train))
    if train:
        print("[INFO] device rollout: {} replay rows, {} episodes finished".format(rows, int(stats[:, 0].sum().item())))
    return max_nums, nums, mean_rewards, total_rewards


def battle_rollout(eng, n_round, map_size, max_steps, models, print_every=50, eps=1.0, left_id=None, check_every=25,
                   board=None, recorder=None):
    """One evaluation round (battle) on all E envs of `eng` on the device rollout loop: models[g].act_rollout for both
    groups -- any pairing of DQN / MFQ / AC / MFAC --, BattleBatch.rollout_policy_step, and one
    RolloutScoreboard.update() per step; no training, no buffers, no host synchronisation inside the loop except one
    8-byte readback every check_every steps.

    Only each env's first episode counts: every env finishes it within max_steps steps (the rollout's episode cap), so
    a round is exactly E episodes, as E rounds of battle() are; counting every episode that ends inside a fixed window
    would over-weight the short ones.  The round stops at max_steps steps, or at the first multiple of check_every
    steps at which every env has finished its first episode.  eps is the temperature of the Q models whose explore is
    "boltzmann" (it must then be finite and > 0) and is not used otherwise: act_rollout is greedy for the Q models by
    default and samples for the actor-critic ones, as battle() with eps 0 does.  board: a RolloutScoreboard of `eng`
    with target 1 and ep_cap >= 1 to keep score on, so that its buffers are reused from round to round (battle_eval
    passes one); None: one is made for this round.  recorder: a mfrl_amd.recorder.RolloutRecorder of `eng` that records
    its watched envs over the round (one more launch per step); the outcome then holds the round's "trace".

    Returns (max_nums, nums, mean_rewards, total_rewards, outcome) over those E episodes: the first four as play()
    gives them to Runner.run, summed over envs -- nums read before clear_dead at each episode's last step,
    total_rewards[g] the episodes' returns, mean_rewards[g] that per step and agent placed (the per-step group sizes
    are not kept) --; outcome is RolloutScoreboard.finish()'s dict plus "first" (main_wins, oppo_wins, ties, kills,
    steps of the counted episodes; a tie counts for both sides in Runner.run), "steps_run" and "agent_steps" (the
    round's agent-steps over all envs, later episodes included)."""
    from ..scoreboard import MAIN, OPPONENT, TIE, RolloutScoreboard
    E, G = eng.n_envs, 2
    for m in models[:G]:
        if not hasattr(m, "act_rollout"):
            raise TypeError("battle_rollout: %s has no device rollout forward" % type(m).__name__)
    if board is not None and (board.eng is not eng or board.target != 1 or board.ep_cap < 1):
        raise ValueError("battle_rollout: the scoreboard must be this engine's, with target 1 and ep_cap >= 1")
    check_every = max(int(check_every), 1)
    left, right = block_positions(map_size)
    left_id = random.randint(0, 1) if left_id is None else left_id
    placement = [None, None]
    placement[left_id], placement[1 - left_id] = left, right
    eng.reset()
    eng.rollout_init(placement, max_steps=max_steps, eps=0.0, seed=n_round, stagger=False)
    if eng.rollout_policy_path() is None:
        raise RuntimeError("battle_rollout: this rollout plan takes no learned policy (MFX_ROLLOUT_PIPE=1)")
    eng.rollout_policy_observe()
    nms = _neighbor_means(eng, models, G)
    for nm in nms:
        if nm is not None:
            nm.reset()
    if board is None:
        board = RolloutScoreboard(eng)
    board.attach()
    if recorder is not None:
        recorder.attach(map_size, max_steps, placement)
    max_nums = [len(placement[g]) * E for g in range(G)]
    print("\n\n[*] ROUND #{0}, EPS: {1:.2f} NUMBER: {2} ({3} envs, device rollout)".format(n_round, eps, max_nums, E))
    t_play = time.time()
    step_ct = 0
    while step_ct < max_steps:
        for g in range(G):
            _act_rollout(models[g], eng, g, eps, nms[g])
        eng.rollout_policy_step()
        for nm in nms:
            if nm is not None:
                nm.update()
        board.update()
        if recorder is not None:
            recorder.update()
        step_ct += 1
        if step_ct % check_every == 0 and step_ct < max_steps and board.reached() >= E:
            break
    out = board.finish()
    if recorder is not None:
        out["trace"] = recorder.finish()
    eng.rollout_check()
    t_play = time.time() - t_play
    steps_buf = np.empty(E, dtype=np.int64)
    eng.rollout_copy("agent_steps", steps_buf)
    eng.sync()
    out["agent_steps"] = int(steps_buf.sum())
    first = out["log"][:, 0]
    if int((out["totals"][:, 0] >= 1).sum()) != E:
        raise RuntimeError("battle_rollout: %d of %d envs finished an episode in %d steps"
                           % (int((out["totals"][:, 0] >= 1).sum()), E, step_ct))
    nums = [int(first["nums"][:, g].sum()) for g in range(G)]
    total_rewards = [float(first["ret"][:, g].sum()) for g in range(G)]
    steps = int(first["len"].sum())
    mean_rewards = [total_rewards[g] / max(steps * len(placement[g]), 1) for g in range(G)]
    out["first"] = {"main_wins": int((first["winner"] == MAIN).sum()), "oppo_wins": int((first["winner"] == OPPONENT).sum()),
                    "ties": int((first["winner"] == TIE).sum()),
                    "kills": [int(first["kill"][:, g].sum()) for g in range(G)], "steps": steps}
    out["steps_run"] = step_ct
    print("[TIME] battle {} steps x {} envs: {:.2f} s; first episodes: {}".format(step_ct, E, t_play, out["first"]))
    return max_nums, nums, mean_rewards, total_rewards, out
