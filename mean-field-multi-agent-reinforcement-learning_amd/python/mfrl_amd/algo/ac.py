"""ActorCritic and MFAC of algo/ac.py:8-361 on PyTorch-ROCm.

act samples the clipped softmax policy (tf.multinomial of its log) on the hand-written HIP forward
(mfrl_amd.policy.ACNetHIP, csrc/acnet_kernels.hip: the policy and a counter-hash draw, its weights re-packed
only when training changed them; act_precision = "bf16": its bf16 acting mode, the values still f32); train builds
one batch from the episode buffer, bootstraps every agent's sequence from the value of its last row, and runs the
discounted-return recursion keep = keep * gamma + r on the device (HIP kernel mfx_mfac_returns,
algo/ac.py:305-320), then one Adam step on pg + value_coef * vf + ent_coef * neg_entropy.

act_rollout / train_rollout are the same two on the device rollout loop: the actions go straight into a
BattleBatch's action buffer, and training runs on the rows a linked RolloutCollector left in the episode buffer,
in place -- the returns walk each agent's chain of rows (HIP kernel mfx_chain_returns) instead of regrouping the
rows per agent, and no np.random is drawn.  advantage = "gae" (opt-in) replaces that walk by GAE(lambda)
over the values of all rows (mfx_chain_gae) and hands the losses an advantage column.  objective = "ppo" (opt-in, on
top of "gae") trains a round in ppo_epochs x ppo_minibatches clipped-surrogate steps instead of one.
"""
import os
import zlib

import numpy as np
import torch

from .. import mf
from . import tools
from .base import as_dev, weights_key
from .nets import ACNet


class ActorCritic:
    _prefix = "ac"
    _use_mf = False
    # act_dev's / act_rollout's HIP forward: "f32", or "bf16" matrix operands (mfrl_amd.policy.ACNetHIP: the policy and
    # the draw only).  The bootstrap value of train() / train_rollout() always comes from the f32 forward, so training
    # is the same, bit for bit, on the same rows whatever this is.
    act_precision = "f32"
    # train() / train_rollout(): "torch" (autograd per chunk of rows and torch.optim.Adam, the default) or "hip" -- one
    # step of the hand-written training kernels on the rows in place (mfrl_amd.actrain.ACTrainHIP, f32), after which
    # the trained blob is copied into self.net and handed to the acting forward device to device.  The two backends
    # keep separate Adam moments and step counts.
    _train_backend = "torch"
    _mean_field = "group"       # the device rollout loops: "group" (the reference's mean), or "neighbors" 
    _mf_radius = 6              # mean_field "neighbors": the Chebyshev radius (the Battle view's)
    _advantage = "returns"      # train_rollout: "returns" (the reference's return - value), or "gae" 
    _gae_lambda = 0.95
    _adv_norm = False
    ADVANTAGES = ("returns", "gae")
    _objective = "pg"           # train_rollout: "pg" (the reference's loss, one step per round), or "ppo" 
    _ppo_clip = 0.2
    _ppo_epochs = 4
    _ppo_minibatches = 4
    _ppo_target_kl = None
    OBJECTIVES = ("pg", "ppo")
    # objective "ppo": rows per slice of the round's policy + value forward -- the transient [rows, n_action] policy of a
    # slice is 22 MB at Battle's 21 actions, whatever the round holds
    PPO_FORWARD_ROWS = 262144

    def __init__(self, sess, name, handle, env, value_coef=0.1, ent_coef=0.08, gamma=0.95, batch_size=64,
                 learning_rate=1e-4):
        self.env = env
        self.name = name
        self.name_scope = name
        self.view_space = tuple(env.get_view_space(handle))
        self.feature_space = tuple(env.get_feature_space(handle))
        self.num_actions = env.get_action_space(handle)[0]
        self.gamma = gamma
        self.reward_decay = gamma
        self.batch_size = batch_size
        self.learning_rate = learning_rate
        self.value_coef = value_coef
        self.ent_coef = ent_coef
        self.replay_buffer = tools.EpisodesBuffer(use_mean=self._use_mf)
        self.net = ACNet(self.view_space, self.feature_space, self.num_actions, use_mf=self._use_mf).cuda()
        self.optimizer = torch.optim.Adam(self.net.parameters(), lr=self.learning_rate)
        self._hip = None
        self._hip_key = None
        self._trainer = None        # ACTrainHIP (train_backend "hip"), made at the first training call
        self._trainer_key = None    # weights_key(self.net) the trainer's parameters were packed from / exported to
        self._draws = 0             # act() calls: the step counter of the device draw
        self._gae_value = None      # advantage "gae": the values and the advantages of a round's rows (float32, grown
        self._gae_adv = None        # geometrically, reused across rounds)
        self._ppo_logp = None       # objective "ppo": the rows' log-probabilities under the round's pre-update weights
        self._ppo_rounds = 0        # rounds trained under "ppo": the second key of replay.ppo_order
        # the draw's seed: the run's torch seed mixed with the model name, so runs seeded alike draw alike and
        # differently seeded runs differ, as tf.multinomial under TF's seed would; np.random is left
        # alone -- the reference consumes it in the replay buffers, and seeded runs must draw the same indices
        self.seed = zlib.crc32(("%s/%s/%d" % (self._prefix, name, torch.initial_seed())).encode())

    @property
    def vars(self):
        return list(self.net.parameters())

    @property
    def mean_field(self):
        """The mean action the model stores (its value head reads it in training) on the device rollout loops (play_rollout*, battle_rollout):
        "group" (the default and the reference's: one mean per (env, group), the group-wide mean of the previous
        step's one-hot actions) or "neighbors" (opt-in, DESIGN 7n: the paper's a_bar_j, one row per agent -- the mean
        over the agents of its own group within Chebyshev distance mf_radius of it, mfrl_amd.mf.NeighborMean).
        Mean-field models only; the host loops (play, play_batched) refuse a "neighbors" model."""
        return self._mean_field

    @mean_field.setter
    def mean_field(self, value):
        self._mean_field = mf.check_mean_field(self, value)

    @property
    def mf_radius(self):
        """The radius of mean_field = "neighbors": an integer >= 0 (default 6, the Battle view's radius)."""
        return self._mf_radius

    @mf_radius.setter
    def mf_radius(self, value):
        self._mf_radius = mf.check_mf_radius(value)

    @property
    def advantage(self):
        """The advantage of the policy term in train_rollout (the device rollout loop): "returns" (the default and the
        reference's: the discounted return bootstrapped from the chain's last row, minus the value) or "gae" (opt-in,
        DESIGN 7q: GAE(gae_lambda) along each agent's chain from the f32 values of all rows, replay.chain_gae; the value
        term regresses on advantage + value).  train(), the host-loop path, refuses a "gae" model."""
        return self._advantage

    @advantage.setter
    def advantage(self, value):
        if value not in self.ADVANTAGES:
            raise ValueError("advantage %r (one of %s)" % (value, ", ".join(self.ADVANTAGES)))
        if value != "gae" and self._adv_norm:
            raise ValueError("advantage %r: adv_norm is set, and normalises the column of advantage \"gae\" -- clear "
                             "it first" % (value,))
        if value != "gae" and self._objective == "ppo":
            raise ValueError("advantage %r: objective \"ppo\" is set, and reads the column of advantage \"gae\" -- set "
                             "objective \"pg\" first" % (value,))
        self._advantage = value

    @property
    def gae_lambda(self):
        """The lambda of advantage = "gae": a number in [0, 1] (default 0.95; 1: the reference's return - value, 0: the
        one-step TD error)."""
        return self._gae_lambda

    @gae_lambda.setter
    def gae_lambda(self, value):
        if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or \
                not 0.0 <= float(value) <= 1.0:
            raise ValueError("gae_lambda must be a number in [0, 1], got %r" % (value,))
        self._gae_lambda = float(value)

    @property
    def adv_norm(self):
        """advantage = "gae" only: normalise the round's advantages to zero mean and unit (population) standard
        deviation before the losses (replay.adv_normalize).  Default off."""
        return self._adv_norm

    @adv_norm.setter
    def adv_norm(self, value):
        if not isinstance(value, (bool, np.bool_)):
            raise ValueError("adv_norm must be a bool, got %r" % (value,))
        if value and self._advantage != "gae":
            raise ValueError("adv_norm normalises the advantage column of advantage = \"gae\": set that first")
        self._adv_norm = bool(value)

    @property
    def objective(self):
        """The policy term of train_rollout (the device rollout loop): "pg" (the default and the reference's: -mean(adv
        log pi), one gradient over the round's rows and one Adam step) or "ppo" (opt-in; needs advantage =
        "gae"): PPO's clipped surrogate of the ratio pi / pi_old, taken in ppo_epochs passes over the round's rows, each
        pass ppo_minibatches contiguous segments in replay.ppo_order's order, one gradient and one Adam step per segment.
        pi_old is the f32 policy of the round's pre-update weights on the collected rows (replay.policy_logp) -- under
        act_precision = "bf16" not exactly the distribution the actions were drawn from.  Not built: value clipping,
        per-minibatch advantage normalisation, random row gathers, bf16 training.  train(), the host-loop path, refuses
        a "ppo" model."""
        return self._objective

    @objective.setter
    def objective(self, value):
        if value not in self.OBJECTIVES:
            raise ValueError("objective %r (one of %s)" % (value, ", ".join(self.OBJECTIVES)))
        if value == "ppo" and self._advantage != "gae":
            raise ValueError("objective \"ppo\" reads the advantage column of advantage = \"gae\": set that first")
        self._objective = value

    @property
    def ppo_clip(self):
        """objective = "ppo": the clip range epsilon of the ratio, a finite number > 0 (default 0.2)."""
        return self._ppo_clip

    @ppo_clip.setter
    def ppo_clip(self, value):
        if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or \
                not (np.isfinite(float(value)) and float(value) > 0.0):
            raise ValueError("ppo_clip must be a finite number > 0, got %r" % (value,))
        self._ppo_clip = float(value)

    @property
    def ppo_epochs(self):
        """objective = "ppo": passes over a round's rows, an integer >= 1 (default 4)."""
        return self._ppo_epochs

    @ppo_epochs.setter
    def ppo_epochs(self, value):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or int(value) < 1:
            raise ValueError("ppo_epochs must be an integer >= 1, got %r" % (value,))
        self._ppo_epochs = int(value)

    @property
    def ppo_minibatches(self):
        """objective = "ppo": segments of a round's rows per pass (one Adam step each), an integer >= 1 (default 4)."""
        return self._ppo_minibatches

    @ppo_minibatches.setter
    def ppo_minibatches(self, value):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or int(value) < 1:
            raise ValueError("ppo_minibatches must be an integer >= 1, got %r" % (value,))
        self._ppo_minibatches = int(value)

    @property
    def ppo_target_kl(self):
        """objective = "ppo": None (the default: nothing is read back inside the step loop), or a finite number >= 0 --
        the mean approx_kl of a pass's steps is read once per pass, and no further pass starts once it exceeds this."""
        return self._ppo_target_kl

    @ppo_target_kl.setter
    def ppo_target_kl(self, value):
        if value is None:
            self._ppo_target_kl = None
            return
        if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or \
                not (np.isfinite(float(value)) and float(value) >= 0.0):
            raise ValueError("ppo_target_kl must be None or a finite number >= 0, got %r" % (value,))
        self._ppo_target_kl = float(value)

    @property
    def ppo_rounds(self):
        """Rounds trained under objective = "ppo" so far: the second key of replay.ppo_order, an integer >= 0.  It is
        not part of save() / load() (those hold the network's weights only, as the reference's do): a resumed run starts
        at 0 again and so replays the segment orders of the first rounds, unless the caller sets it."""
        return getattr(self, "_ppo_rounds", 0)

    @ppo_rounds.setter
    def ppo_rounds(self, value):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or int(value) < 0:
            raise ValueError("ppo_rounds must be an integer >= 0, got %r" % (value,))
        self._ppo_rounds = int(value)

    def reset_optimizer(self):
        """Fresh optimiser state on both training backends: a new torch Adam, and the HIP trainer dropped, so that the
        next "hip" training call makes one with zero moments at step 0 and packs the network's weights into it."""
        self.optimizer = torch.optim.Adam(self.net.parameters(), lr=self.learning_rate)
        self._trainer = None
        self._trainer_key = None

    def _ppo_column(self, cap):
        """The model's logp_old tensor, `cap` rows: sized with the buffer's row storage like _gae_columns."""
        if self._ppo_logp is None or self._ppo_logp.numel() < cap:
            self._ppo_logp = torch.empty(cap, dtype=torch.float32, device="cuda")
        return self._ppo_logp

    def _gae_columns(self, cap):
        """The model's value and advantage tensors, `cap` rows each -- the capacity of the buffer's row storage, so
        they grow geometrically with it and serve every later round that fits."""
        if self._gae_value is None or self._gae_value.numel() < cap:
            self._gae_value = torch.empty(cap, dtype=torch.float32, device="cuda")
            self._gae_adv = torch.empty(cap, dtype=torch.float32, device="cuda")
        return self._gae_value, self._gae_adv

    @property
    def train_backend(self):
        return self._train_backend

    @train_backend.setter
    def train_backend(self, name):
        if name not in ("torch", "hip"):
            raise ValueError("train_backend %r (torch or hip)" % (name,))
        if name == "hip" and not self._hip_ok():
            raise ValueError("train_backend hip: the HIP training step takes 2..32 actions, views of at most 4096 floats "
                             "and at most 256 features")
        self._train_backend = name

    def _hip_trainer(self):
        """The HIP training handle holding the network's current weights (re-packed only when they moved under it:
        a load(), the Runner's self-play update, a torch-backend step)."""
        if self._trainer is None:
            from ..actrain import ACTrainHIP
            self._trainer = ACTrainHIP(self.view_space, self.feature_space, self.num_actions, self._use_mf,
                                       lr=self.learning_rate, value_coef=self.value_coef, ent_coef=self.ent_coef)
        key = weights_key(self.net)
        if key != self._trainer_key:
            self._trainer.load(self.net)
            self._trainer_key = key
        return self._trainer

    def _hip_train(self, cols, n, step=True, support=None, chunk_rows=None):
        """One ACTrainHIP step (or, step=False, its gradient as per-parameter tensors) over rows [0, n) of cols where
        they lie; -> (grads or None, stats tensor).  After a step the trained blob is exported into self.net and set
        as the acting handle's weights device to device, with both keys moved so that nothing is re-packed."""
        from ..policy import ACNetHIP, unpack_acnet
        tr = self._hip_trainer()
        tr.set_input_support(support)
        tr.set_chunk_rows(chunk_rows)
        if not step:
            g, stats = tr.grads(cols, n)
            tr.check_error()
            return unpack_acnet(g, self.net, into=[torch.empty_like(p) for p in self.net.parameters()]), stats
        stats = tr.step(cols, n)
        tr.check_error()
        blob = tr.export(self.net)
        if self._hip is None:
            self._hip = ACNetHIP(self.view_space, self.feature_space, self.num_actions, self._use_mf)
        self._hip.set_blob(blob)
        self._trainer_key = self._hip_key = weights_key(self.net)
        return None, stats

    def flush_buffer(self, **kwargs):
        self.replay_buffer.push(**kwargs)

    @torch.no_grad()
    def act_dev(self, **kwargs):
        """Device in, device out: int32 actions drawn from the clipped softmax policy (algo/ac.py:43-46,
        tf.multinomial(log(policy))) by the HIP forward k_acnet; the draw's uniforms are a counter hash of
        (self.seed, the act() count, the row) instead of TensorFlow's stream."""
        view, feat = as_dev(kwargs["state"][0]), as_dev(kwargs["state"][1])
        if self._hip_ok():
            self._draws += 1
            return self._hip_net(self.act_precision).act(view, feat, seed=self.seed, step=self._draws)
        policy, _ = self.net(view, feat, need_value=False)
        return torch.multinomial(policy, 1).reshape(-1).to(torch.int32)

    def _hip_net(self, precision="f32"):
        """The HIP forward in mode `precision` with the network's current weights (re-packed only after they
        changed).  One handle: it keeps the f32 weights in both modes, so acting in bf16 and taking the bootstrap
        value in f32 is a mode flip, not a second copy."""
        if self._hip is None:
            from ..policy import ACNetHIP
            self._hip = ACNetHIP(self.view_space, self.feature_space, self.num_actions, self._use_mf,
                                 precision=precision)
        key = weights_key(self.net)
        if key != self._hip_key:
            self._hip.load(self.net)
            self._hip_key = key
        return self._hip.set_precision(precision)

    def _hip_ok(self):
        return 2 <= self.num_actions <= 32 and int(np.prod(self.view_space)) <= 4096 and self.feature_space[0] <= 256

    def act(self, **kwargs):
        return self.act_dev(**kwargs).cpu().numpy().astype(np.int32)

    def losses(self, view, feature, action, reward, prob=None, total_rows=None, adv=None, logp_old=None, clip=None):
        """total_rows: these rows are one chunk of that many (train_rollout) -- every mean becomes the chunk's sum
        over total_rows, so that the chunks' losses add up to the means over all rows.  adv: the rows' advantages
        (advantage = "gae") in place of (reward - value).detach(); the value term regresses on reward either way.
        logp_old with clip (objective = "ppo"): the policy term is the clipped surrogate of r = exp(log_prob - logp_old)
        by the HIP head's rule (mfx_actrain_set_ppo) -- an explicit mask and not torch.min, so that a row on the bound
        counts as not clipped on both backends -- and a fifth result follows the four: the chunk's sums of (clipped,
        (r - 1) - d), a detached float64 tensor of 2.  Without them the ops and the four results are the default's."""
        mean = torch.mean if total_rows is None else (lambda x: torch.sum(x) / total_rows)
        policy, value = self.net(view, feature, prob)
        action_mask = torch.nn.functional.one_hot(action.long(), self.num_actions).float()
        advantage = (reward - value).detach() if adv is None else adv
        log_policy = torch.log(policy + 1e-6)
        log_prob = torch.sum(log_policy * action_mask, dim=1)
        if logp_old is not None and clip is not None:
            lo, hi = float(np.float32(1.0 - clip)), float(np.float32(1.0 + clip))       # the head's f32 bounds
            d = log_prob - logp_old
            r = torch.exp(d)
            up = advantage > 0
            clipped = (up & (r > hi)) | ((advantage < 0) & (r < lo))
            bound = torch.where(up, torch.full_like(r, hi), torch.full_like(r, lo))
            pg_loss = -mean(torch.where(clipped, (advantage * bound).detach(), advantage * r))
            terms = torch.stack([clipped.sum().double(), ((r - 1.0) - d).detach().sum().double()])
        else:
            pg_loss = -mean(advantage * log_prob)
            terms = None
        vf_loss = self.value_coef * mean(torch.square(reward - value))
        neg_entropy = self.ent_coef * mean(torch.sum(policy * log_policy, dim=1))
        if terms is not None:
            return pg_loss, vf_loss, neg_entropy, value, terms
        return pg_loss, vf_loss, neg_entropy, value

    def train(self):
        if self._objective != "pg":
            raise ValueError("train: objective %r runs on the device rollout loop (train_rollout / "
                             "play_rollout_episodes); the host loops train on the reference's loss" % self._objective)
        if self._advantage != "returns":
            raise ValueError("train: advantage %r runs on the device rollout loop (train_rollout / "
                             "play_rollout_episodes); the host loops train on the reference's returns" % self._advantage)
        got = self.replay_buffer.batch()
        self.replay_buffer = tools.EpisodesBuffer(use_mean=self._use_mf)
        if got is None:
            return
        rows, counts = got
        view, feature, action = rows["obs"], rows["feat"], rows["act"]
        reward = rows["rew"].clone()
        prob = rows.get("prob")
        last = torch.cumsum(counts, 0) - 1
        with torch.no_grad():                     # value of every agent's last row (the bootstrap), on k_acnet
            if self._hip_ok():
                _, keep, _ = self._hip_net().forward(view[last], feature[last], prob[last] if prob is not None else None,
                                                     want_policy=False, want_value=True, want_act=False)
            else:
                _, keep = self.net(view[last], feature[last], prob[last] if prob is not None else None)
        offsets = torch.zeros(len(counts) + 1, dtype=torch.int64, device="cuda")
        offsets[1:] = torch.cumsum(counts, 0)
        mf.mfac_returns(reward, offsets, keep.float().contiguous(), self.gamma)
        if self._train_backend == "hip":
            cols = {"obs": view, "feat": feature, "act": action, "ret": reward, "prob": prob}
            pg, vf, ent, val = self._hip_train(cols, len(reward))[1].tolist()
            print("[*] PG_LOSS:", np.round(pg, 6), "/ VF_LOSS:", np.round(vf, 6), "/ ENT_LOSS:", np.round(ent, 6),
                  "/ VALUE:", val)
            return
        pg_loss, vf_loss, ent_loss, state_value = self.losses(view, feature, action, reward, prob)
        total = pg_loss + vf_loss + ent_loss
        self.optimizer.zero_grad(set_to_none=True)
        total.backward()
        self.optimizer.step()
        print("[*] PG_LOSS:", np.round(pg_loss.item(), 6), "/ VF_LOSS:", np.round(vf_loss.item(), 6),
              "/ ENT_LOSS:", np.round(ent_loss.item(), 6), "/ VALUE:", state_value.mean().item())

    # ---- the device rollout loop (play.play_rollout_episodes)
    @torch.no_grad()
    def act_rollout(self, eng, group, prob_rows=None):
        """Sampled actions of group `group` of a BattleBatch's rollout from its observation buffers into its action
        buffer (mfrl_amd.policy.ACNetHIP.act_rollout) with the current weights and the draw of act_dev (self.seed,
        the act count); nothing is read back.  Streams: the weights -- however they moved: an optimiser step,
        load_state_dict, a "hip"-backend step, which hands its blob to the acting handle itself -- a mode's first
        images and the support image are enqueued on the caller's current stream, the kernels on the engine's.  The
        handle orders the two (mfrl_amd.policy.StreamOrder): every engine that acts with this model, on whatever
        stream, waits for the handle's last change once, the first time it acts after it.  prob_rows (the mean
        action per agent of mean_field = "neighbors") is accepted and not read: the policy head takes no mean action,
        only the value head does, in training, from the collected rows."""
        if not self._hip_ok():
            raise ValueError("act_rollout: the HIP forward takes 2..32 actions, views of at most 4096 floats and at "
                             "most 256 features")
        hip = self._hip_net(self.act_precision)
        self._draws += 1
        hip.act_rollout(eng, group, seed=self.seed, step=self._draws)

    def rollout_collector(self, eng, group=0):
        """The RolloutCollector of this model's EpisodesBuffer on `eng` (linked rows; made once and kept while
        the engine and the buffer stay the same)."""
        from ..replay import RolloutCollector
        rows = self.replay_buffer.prepare(self.view_space, self.feature_space, self.num_actions if self._use_mf else 1)
        col = getattr(self, "_rollout_collector", None)
        if col is None or col.eng is not eng or col.mg is not self.replay_buffer or col.group != group:
            col = self._rollout_collector = RolloutCollector(eng, self.replay_buffer, group)
        assert col.mg._rows is rows
        return col

    # rows per autograd graph of train_rollout: the activations kept for backward are about 7 KB per row (the view
    # and its 256-wide layer, the 512-wide dense layer twice, the heads), so 65,536 rows hold about 0.5 GB -- large
    # enough that the launches of a chunk are not the cost, small against HBM at any round size.  Nothing depends
    # on the value beyond the float summation order of the gradient.
    ROLLOUT_CHUNK_ROWS = 65536

    def train_rollout(self, chunk_rows=None, step=True):
        """train() for rows collected by this model's RolloutCollector, where they lie.  finish() the collector;
        tails = the rows that end a chain (the host synchronisation the path needs: their number; chain_returns
        then waits once more, for its error word, with nothing left to overlap); the bootstrap value of
        every chain from its tail row on k_acnet, as train() takes it from every agent's last row; the returns in
        place on the reward column along the chains (replay.chain_returns); then the losses of train() over the
        rows in contiguous chunks of at most chunk_rows -- each chunk's sums divided by the total row count, so the
        chunks' gradients add up to the gradient of the means over all rows -- and one Adam step.  The losses are
        means over rows, so the step-major order changes their float summation order and nothing else.
        advantage = "gae": the f32 value forward runs over all n rows instead of the tail rows, replay.chain_gae
        walks the same chains (the reward column becomes advantage + value, the model's adv tensor the advantages,
        normalised when adv_norm is set), and the policy term of either backend reads that column.
        objective = "ppo" (DESIGN 7u): that all-rows forward also returns the policy (in slices of PPO_FORWARD_ROWS),
        replay.policy_logp leaves its log-probabilities of the taken actions in the model's logp_old tensor, and the one
        step becomes ppo_epochs passes of M = min(ppo_minibatches, n) steps: pass e takes the segments [k n // M,
        (k + 1) n // M) of the step-major rows, in place, in replay.ppo_order(self.seed, rounds trained, e, M)'s order --
        one gradient with means over the segment's rows and one Adam step each (the "hip" backend exports its blob once,
        after the last step).  ppo_target_kl: see there.  logp_old is the f32 policy of the pre-update weights: under
        act_precision = "bf16" it is not exactly the distribution the actions were drawn from.  The printed stats are
        the means over the steps taken.  step=False under "ppo": the gradient of the whole round as one minibatch at
        the unchanged weights (the ratio is 1 up to rounding).
        step=False: no Adam step; returns the gradients (one tensor per parameter, None where there is none).
        Afterwards the rows are cleared; the buffer and its storage are kept."""
        from .. import replay
        col = getattr(self, "_rollout_collector", None)
        if col is None or col.mg is not self.replay_buffer:
            raise RuntimeError("train_rollout: no rows were collected (rollout_collector() / play_rollout_episodes)")
        col.finish()
        rows = self.replay_buffer._rows
        n = rows.n
        if n == 0:
            return None
        chunk = int(chunk_rows or self.ROLLOUT_CHUNK_ROWS)
        assert chunk >= 1
        c = rows.cols
        prob = c["prob"] if self._use_mf else None
        gae = self._advantage == "gae"
        ppo = self._objective == "ppo"
        adv = logp = None
        if gae:
            if not self._hip_ok():
                raise ValueError("train_rollout: advantage \"gae\" takes its values from the HIP forward (2..32 actions, "
                                 "views of at most 4096 floats, at most 256 features)")
            value, adv = self._gae_columns(rows.cap)
            value.record_stream(col.eng.torch_stream())
            adv.record_stream(col.eng.torch_stream())
            if ppo:
                logp = self._ppo_column(rows.cap)
                logp.record_stream(col.eng.torch_stream())
        # the f32 handle with the current weights, taken on the caller's stream: an upload reads the parameters where
        # torch last wrote them, and the handle orders the engine's stream -- and every other engine's -- behind it
        hip = self._hip_net() if self._hip_ok() else None
        with torch.cuda.stream(col.eng.torch_stream()), torch.no_grad():
            tails = c["tail"][:n].nonzero().reshape(-1)
            if ppo:
                # the f32 policy and value of every row in one pass, a slice at a time
                for a in range(0, n, self.PPO_FORWARD_ROWS):
                    b = min(a + self.PPO_FORWARD_ROWS, n)
                    pol, v_rows, _ = hip.forward(c["obs"][a:b], c["feat"][a:b], prob[a:b] if prob is not None else None,
                                                 want_policy=True, want_value=True, want_act=False)
                    value[a:b].copy_(v_rows.reshape(-1))
                    replay.policy_logp(pol, c["act"][a:b], logp[a:b])
            elif gae:
                # the f32 value of every row (whatever act_precision is), then the walk along the same chains
                _, v_rows, _ = hip.forward(c["obs"][:n], c["feat"][:n], prob[:n] if prob is not None else None,
                                                       want_policy=False, want_value=True, want_act=False)
                value[:n].copy_(v_rows.reshape(-1))
            if gae:
                replay.chain_gae(c["rew"][:n], adv, c["prev"], tails, value, self.gamma, self._gae_lambda)
                if self._adv_norm:
                    replay.adv_normalize(adv[:n])
            else:
                p_t = prob[tails] if prob is not None else None
                if hip is not None:
                    _, keep, _ = hip.forward(c["obs"][tails], c["feat"][tails], p_t, want_policy=False,
                                                         want_value=True, want_act=False)
                else:
                    _, keep = self.net(c["obs"][tails], c["feat"][tails], p_t)
                replay.chain_returns(c["rew"][:n], c["prev"], tails, keep.float().reshape(-1), self.gamma)
        torch.cuda.current_stream().wait_stream(col.eng.torch_stream())
        if ppo:
            return self._train_ppo(col, c, prob, adv, logp, n, len(tails), chunk, chunk_rows, step)
        if self._train_backend == "hip":
            # the rows come from the engine: the view layer runs over its support, as act_rollout's does
            cols = {"obs": c["obs"], "feat": c["feat"], "act": c["act"], "ret": c["rew"], "prob": prob, "adv": adv}
            grads, stats = self._hip_train(cols, n, step=step, support=col.eng.view_support(col.group),
                                           chunk_rows=chunk_rows)
            col.eng.torch_stream().wait_stream(torch.cuda.current_stream())
            self.replay_buffer.clear()
            pg, vf, ent, val = stats.tolist()
            print("[*] PG_LOSS:", np.round(pg, 6), "/ VF_LOSS:", np.round(vf, 6), "/ ENT_LOSS:", np.round(ent, 6),
                  "/ VALUE:", val, "({} rows, {} chains)".format(n, len(tails)))
            return grads
        self.optimizer.zero_grad(set_to_none=True)
        sums = torch.zeros(4, dtype=torch.float64, device="cuda")
        for a in range(0, n, chunk):
            b = min(a + chunk, n)
            pg, vf, ent, value = self.losses(c["obs"][a:b], c["feat"][a:b], c["act"][a:b], c["rew"][a:b],
                                             prob[a:b] if prob is not None else None, total_rows=n,
                                             adv=adv[a:b] if adv is not None else None)
            (pg + vf + ent).backward()
            sums += torch.stack([pg.detach(), vf.detach(), ent.detach(), value.detach().sum() / n]).double()
        col.eng.torch_stream().wait_stream(torch.cuda.current_stream())     # the next round writes these rows
        grads = None
        if step:
            self.optimizer.step()
        else:
            grads = [None if p.grad is None else p.grad.detach().clone() for p in self.net.parameters()]
            self.optimizer.zero_grad(set_to_none=True)
        self.replay_buffer.clear()
        pg, vf, ent, val = sums.tolist()
        print("[*] PG_LOSS:", np.round(pg, 6), "/ VF_LOSS:", np.round(vf, 6), "/ ENT_LOSS:", np.round(ent, 6),
              "/ VALUE:", val, "({} rows, {} chains)".format(n, len(tails)))
        return grads

    def _train_ppo(self, col, c, prob, adv, logp, n, n_chains, chunk, chunk_rows, step):
        """train_rollout's step loop under objective = "ppo", the columns prepared and visible on the current stream."""
        from .. import replay
        from ..policy import ACNetHIP, unpack_acnet
        hip_backend = self._train_backend == "hip"
        cols = {"obs": c["obs"], "feat": c["feat"], "act": c["act"], "ret": c["rew"], "prob": prob, "adv": adv,
                "logp_old": logp}
        clip = self._ppo_clip

        def seg(a, b):
            return {k: (t[a:b] if t is not None else None) for k, t in cols.items()}

        def torch_grad(a, b):
            """The gradient of segment [a, b) (means over its rows) left in .grad; -> its six sums on the device."""
            self.optimizer.zero_grad(set_to_none=True)
            sums = torch.zeros(6, dtype=torch.float64, device="cuda")
            for s in range(a, b, chunk):
                e = min(s + chunk, b)
                pg, vf, ent, value, terms = self.losses(c["obs"][s:e], c["feat"][s:e], c["act"][s:e], c["rew"][s:e],
                                                        prob[s:e] if prob is not None else None, total_rows=b - a,
                                                        adv=adv[s:e], logp_old=logp[s:e], clip=clip)
                (pg + vf + ent).backward()
                sums += torch.cat([torch.stack([pg.detach(), vf.detach(), ent.detach(),
                                                value.detach().sum() / (b - a)]).double(), terms / (b - a)])
            return sums

        if hip_backend:
            tr = self._hip_trainer()
            tr.set_input_support(col.eng.view_support(col.group))
            tr.set_chunk_rows(chunk_rows)
        grads, steps = None, 0
        total = torch.zeros(6, dtype=torch.float64, device="cuda")
        if not step:
            if hip_backend:
                g, stats = tr.grads(cols, n, clip=clip)
                tr.check_error()
                grads = unpack_acnet(g, self.net, into=[torch.empty_like(p) for p in self.net.parameters()])
                total = torch.cat([stats, tr.ppo_stats()]).double()
            else:
                total = torch_grad(0, n)
                grads = [None if p.grad is None else p.grad.detach().clone() for p in self.net.parameters()]
                self.optimizer.zero_grad(set_to_none=True)
        else:
            M = min(self._ppo_minibatches, n)
            for epoch in range(self._ppo_epochs):
                kl = torch.zeros((), dtype=torch.float64, device="cuda")
                for k in replay.ppo_order(self.seed, self._ppo_rounds, epoch, M):
                    a, b = k * n // M, (k + 1) * n // M
                    if hip_backend:
                        stats = tr.step(seg(a, b), b - a, clip=clip)
                        six = torch.cat([stats, tr.ppo_stats()]).double()
                    else:
                        six = torch_grad(a, b)
                        self.optimizer.step()
                    total += six
                    kl += six[5]
                    steps += 1
                if self._ppo_target_kl is not None and kl.item() / M > self._ppo_target_kl:   # the pass's one read-back
                    break
            total /= steps
            self._ppo_rounds += 1
            if hip_backend:
                tr.check_error()
                blob = tr.export(self.net)
                if self._hip is None:
                    self._hip = ACNetHIP(self.view_space, self.feature_space, self.num_actions, self._use_mf)
                self._hip.set_blob(blob)
                self._trainer_key = self._hip_key = weights_key(self.net)
            else:
                self.optimizer.zero_grad(set_to_none=True)
        col.eng.torch_stream().wait_stream(torch.cuda.current_stream())     # the next round writes these rows
        self.replay_buffer.clear()
        pg, vf, ent, val, frac, kl = total.tolist()
        print("[*] PG_LOSS:", np.round(pg, 6), "/ VF_LOSS:", np.round(vf, 6), "/ ENT_LOSS:", np.round(ent, 6),
              "/ VALUE:", val, "/ CLIP_FRAC:", np.round(frac, 6), "/ KL:", np.round(kl, 8),
              "({} rows, {} chains, {} steps)".format(n, n_chains, steps))
        return grads

    def save(self, dir_path, step=0):
        os.makedirs(dir_path, exist_ok=True)
        path = os.path.join(dir_path, "{}_{}.pt".format(self._prefix, step))
        torch.save(self.net.state_dict(), path)
        print("[*] Model saved at: {}".format(path))

    def load(self, dir_path, step=0):
        path = os.path.join(dir_path, "{}_{}.pt".format(self._prefix, step))
        self.net.load_state_dict(torch.load(path, map_location="cuda", weights_only=True))
        print("[*] Loaded model from {}".format(path))


class MFAC(ActorCritic):
    _prefix = "mfac"
    _use_mf = True
