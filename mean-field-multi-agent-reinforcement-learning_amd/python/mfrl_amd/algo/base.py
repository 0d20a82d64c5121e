"""ValueNet (algo/base.py:7-279) on PyTorch-ROCm: eval / target Q networks, greedy act, the MF-Q
target on device (HIP kernel mfx_mfq_target), masked-MSE Adam step, soft target update.

Inputs may be numpy arrays (the reference's call sites) or device tensors (the batched engine);
outputs follow the reference: act -> int32 numpy, calc_target_q -> float64, train -> (loss, stats).
"""
import copy
import zlib

import numpy as np
import torch

from .. import mf, replay
from .nets import QNet


def as_dev(x, dtype=torch.float32):
    if isinstance(x, torch.Tensor):
        return x.to(device="cuda", dtype=dtype)
    return torch.as_tensor(np.asarray(x), dtype=dtype, device="cuda")


def weights_key(net, gen=0):
    """Changes whenever `net`'s weights may have changed: every in-place update of a parameter (optimiser
    steps, copy_, load_state_dict) bumps its version counter; `gen` covers updates torch does not see (a
    replayed HIP graph).  The HIP forwards re-pack their weight blob only when the key moves."""
    return (gen, tuple((p.data_ptr(), p._version) for p in net.parameters()))


EXPLORE = ("greedy", "boltzmann")       # ValueNet.explore


TARGET_RULES = ("max", "boltzmann")     # ValueNet.target_rule
check_temperature = mf.check_temperature    # finite and > 0, else ValueError: one rule for acting and for the target


class ValueNet:
    graph_train = True         # train() replays the minibatch step as a HIP graph (train_batches)
    act_precision = "f32"       # act_dev's HIP forward: "f32", or "bf16" operands (mfrl_amd.policy); training stays f32
    _train_backend = "torch"    # train_batches: "torch" (the graph below), or "hip" (mfrl_amd.qtrain, csrc/qtrain_kernels.hip)
    _explore = "greedy"         # act_dev / act_rollout: "greedy" (the reference's argmax), or "boltzmann" (csrc/qsample.h)
    _target_rule = "max"        # training target: "max" (the reference's rule), or "boltzmann" (the paper's v^MF)
    target_temperature = None   # target_rule "boltzmann": None = self.temperature (the last acting eps); a float overrides it
    _mean_field = "group"       # the device rollout loops: "group" (the reference's mean), or "neighbors" 
    _mf_radius = 6              # mean_field "neighbors": the Chebyshev radius (the Battle view's)

    def __init__(self, sess, env, handle, name, update_every=5, use_mf=False, learning_rate=1e-4, tau=0.005,
                 gamma=0.95):
        self.env = env
        self.name = name
        self.name_scope = name or "ValueNet"
        self.handle = handle
        self.view_space = tuple(env.get_view_space(handle))
        assert len(self.view_space) == 3
        self.feature_space = tuple(env.get_feature_space(handle))
        self.num_actions = env.get_action_space(handle)[0]
        self.update_every = update_every
        self.use_mf = use_mf
        self.temperature = 0.1
        self.lr = learning_rate
        self.tau = tau
        self.gamma = gamma
        self.eval_net = QNet(self.view_space, self.feature_space, self.num_actions, use_mf).cuda()
        self.target_net = copy.deepcopy(self.eval_net)     # TF initialises both; any start works
        for p in self.target_net.parameters():
            p.requires_grad_(False)
        # capturable: the step count lives on the device, so train_batches can replay the whole
        # minibatch update (sample gather, target, loss, backward, Adam, soft update) as a HIP graph
        self.optimizer = torch.optim.Adam(self.eval_net.parameters(), lr=self.lr, capturable=True)
        self._graph = None
        self._wgen = 0              # bumped after graph replays (they update the weights behind torch's back)
        self._hip_key = None
        self._draws = 0             # acting calls: the step counter of the Boltzmann draw (explore = "boltzmann")
        # the draw's seed, made as ActorCritic makes its own: the run's torch seed mixed with the model name; np.random
        # is left alone (the replay buffers consume it, and seeded runs must sample the same indices)
        self.seed = zlib.crc32(("%s/%s/%d" % ("mfq" if use_mf else "dqn", name, torch.initial_seed())).encode())

    @property
    def explore(self):
        """How act_dev / act_rollout choose: "greedy" (the default and the reference's act: argmax q; eps is only
        stored) or "boltzmann" (opt-in): the action is drawn from softmax(q / T) with T = the call's eps, by the
        contract of csrc/qsample.h -- the uniform of a row is the counter hash of (self.seed, the count of acting
        calls, the group, the row), so np.random is not consumed and seeded runs repeat.  Training is the same in both
        modes: the target is chosen by target_rule, on its own."""
        return self._explore

    @explore.setter
    def explore(self, value):
        if value not in EXPLORE:
            raise ValueError("explore %r (one of %s)" % (value, ", ".join(EXPLORE)))
        self._explore = value

    @property
    def mean_field(self):
        """The mean action the model acts on and stores on the device rollout loops (play_rollout*, battle_rollout):
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
    def target_rule(self):
        """What calc_target_q_dev and train_batches bootstrap from: "max" (the default and the reference's rule: the
        target net's value of the eval net's greedy next action) or "boltzmann" (opt-in; the paper's mean-field value
        v^MF = sum_a pi(a) Q_target(s', a) with pi = softmax(Q_eval(s') / T): mfrl_amd.mf.mfq_target_boltzmann, and
        QTrainHIP.set_target on the "hip" backend).  pi's weights are exactly those the "boltzmann" explore mode draws
        from.  T = target_temperature, or self.temperature (the last acting eps) while that is None; it must be finite
        and > 0 when a target is computed.  Setting another rule drops a captured training graph."""
        return self._target_rule

    @target_rule.setter
    def target_rule(self, value):
        if value not in TARGET_RULES:
            raise ValueError("target_rule %r (one of %s)" % (value, ", ".join(TARGET_RULES)))
        if value != self._target_rule:
            self._graph = None
        self._target_rule = value

    def _target_T(self):
        """The Boltzmann target's temperature for the call at hand (ValueError unless finite and > 0)."""
        T = self.temperature if self.target_temperature is None else self.target_temperature
        return mf.check_temperature(T, "target_rule 'boltzmann': the temperature (target_temperature, else the last eps)")

    def _target(self, e_q, t_q, rewards, dones, temperature):
        if self._target_rule == "boltzmann":
            return mf.mfq_target_boltzmann(e_q, t_q, rewards, dones, self.gamma, temperature)
        return mf.mfq_target(e_q, t_q, rewards, dones, self.gamma)

    @property
    def train_backend(self):
        """The minibatch loop of train_batches: "torch" (the default: autograd + torch.optim.Adam, replayed as a HIP
        graph) or "hip" (the hand-written training step, mfrl_amd.qtrain.QTrainHIP).  The two do not share optimizer
        state: Adam's moments and step count of the "hip" backend live in its handle, torch's in self.optimizer, and
        switching carries the weights over but neither backend's moments.  Setting "hip" on a model whose shapes the
        kernels do not take (Battle view 13 x 13 x 7, feature <= 256, at most 32 actions) raises ValueError."""
        return self._train_backend

    @train_backend.setter
    def train_backend(self, value):
        if value not in ("torch", "hip"):
            raise ValueError("train_backend %r (one of torch, hip)" % (value,))
        if value == "hip":
            from ..qtrain import supported
            if not supported(self.view_space, self.feature_space, self.num_actions):
                raise ValueError("train_backend 'hip' takes the Battle view (13, 13, 7), feature <= 256 and at most 32 "
                                 "actions; this model has %r, %r, %d" % (self.view_space, self.feature_space,
                                                                        self.num_actions))
        self._train_backend = value

    @property
    def vars(self):
        """Parameters in a fixed order (eval net, then target net), like the scope's variables."""
        return list(self.eval_net.parameters()) + list(self.target_net.parameters())

    def _prob(self, kwargs, n):
        if not self.use_mf:
            return None
        assert kwargs.get("prob", None) is not None
        return as_dev(kwargs["prob"]).reshape(n, self.num_actions)

    def calc_target_q(self, **kwargs):
        """kwargs: obs, feature, prob (mean field), dones, rewards -> float64 [n] (numpy)."""
        return self.calc_target_q_dev(**kwargs).cpu().numpy()

    @torch.no_grad()
    def calc_target_q_dev(self, **kwargs):
        obs, feat = as_dev(kwargs["obs"]), as_dev(kwargs["feature"])
        prob = self._prob(kwargs, len(obs))
        t_q = self.target_net(obs, feat, prob)
        e_q = self.eval_net(obs, feat, prob)
        return self._target(e_q.float().contiguous(), t_q.float().contiguous(), as_dev(kwargs["rewards"]),
                            as_dev(kwargs["dones"], torch.uint8),
                            self._target_T() if self._target_rule == "boltzmann" else None)

    @torch.no_grad()
    def update(self):
        """Soft update: target = tau * eval + (1 - tau) * target."""
        for t, e in zip(self.target_net.parameters(), self.eval_net.parameters()):
            t.mul_(1.0 - self.tau).add_(self.tau * e)

    # ------------------------------------------------------------------ minibatch loop on device
    def train_batches(self, buf, batch_num, use_mean):
        """The reference's train loop (algo/q_learning.py:42-54 DQN, :110-131 MFQ): batch_num times
        sample -> calc_target_q -> train -> update, printing the loss every 50 minibatches.

        The sample indices are drawn up front with the same np.random.choice calls sample() makes,
        and the minibatch step is captured once as a HIP graph (static index tensors, the replay
        rings' fixed storage) and replayed, so a minibatch is one graph launch instead of ~150
        kernel launches and three host syncs.  The first minibatches run eagerly on a side stream
        (the warm-up graph capture needs); the losses are read back once at the end."""
        if batch_num <= 0:
            return
        if self._train_backend == "hip":
            return self._train_batches_hip(buf, batch_num, use_mean)
        n, B = buf.nb_entries, buf.batch_size
        idx = np.stack([np.random.choice(n, size=B) for _ in range(batch_num)]).astype(np.int64)
        nxt = (idx + 1) % n
        idx_d = torch.as_tensor(idx, device="cuda")
        nxt_d = torch.as_tensor(nxt, device="cuda")
        stats = torch.zeros((batch_num, 2), dtype=torch.float32, device="cuda")
        if self._target_rule == "boltzmann":
            # the captured graph reads the temperature from a static device tensor, refilled at every call: eps moves
            # from round to round, and a graph captured in one round must not go on training at that round's value
            T = self._target_T()
            if getattr(self, "_s_T", None) is None:
                self._s_T = torch.zeros(1, dtype=torch.float32, device="cuda")
            self._s_T.fill_(T)
        if self._graph is None:
            self._s_idx = torch.zeros(B, dtype=torch.int64, device="cuda")
            self._s_nxt = torch.zeros(B, dtype=torch.int64, device="cuda")
            self._s_out = torch.zeros(2, dtype=torch.float32, device="cuda")
        warm = 0 if self._graph is not None else min(3, batch_num)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for i in range(warm):
                self._s_idx.copy_(idx_d[i])
                self._s_nxt.copy_(nxt_d[i])
                self._minibatch(buf, use_mean)
                stats[i].copy_(self._s_out)
        torch.cuda.current_stream().wait_stream(side)
        if warm < batch_num and self._graph is None:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._minibatch(buf, use_mean)
            self._graph = g
        for i in range(warm, batch_num):
            self._s_idx.copy_(idx_d[i])
            self._s_nxt.copy_(nxt_d[i])
            self._graph.replay()
            stats[i].copy_(self._s_out)
        self._wgen += 1
        st = stats.cpu().numpy()
        for i in range(0, batch_num, 50):
            print("[*] LOSS:", float(st[i, 0]), "/ Q:", {"Eval-Q": np.round(float(st[i, 1]), 6)})

    def _train_batches_hip(self, buf, batch_num, use_mean):
        """train_batches on the hand-written training step: the same np.random.choice draws, then the whole sequential
        minibatch loop enqueued by one call (mfx_qtrain_run) reading the ring rows in place; afterwards both blobs are
        unpacked into the torch modules, so act_dev / act_rollout / save / vars / self_play_update see the new weights.
        The nets are packed into the handle only when weights_key shows they moved since the handle last exported them
        (self_play_update, load, a per-call train()).  Raises mfrl_amd.qtrain.QTrainError on a device error (a sample
        index or a replay action out of range): the minibatches before it are applied, it and the later ones are not."""
        assert bool(use_mean) == bool(self.use_mf), "train_batches: use_mean must match the model"
        n, B = buf.nb_entries, buf.batch_size
        idx = np.stack([np.random.choice(n, size=B) for _ in range(batch_num)]).astype(np.int64)
        if getattr(self, "_qtrain", None) is None:
            from ..qtrain import QTrainHIP
            self._qtrain = QTrainHIP(self.view_space, self.feature_space, self.num_actions, self.use_mf, lr=self.lr,
                                     tau=self.tau, gamma=self.gamma)
            self._qtrain_key = None
        tr = self._qtrain
        tr.set_hyper(self.lr, tau=self.tau, gamma=self.gamma)      # the model's current values, as the torch path reads them
        if self._target_rule == "boltzmann":
            tr.set_target("boltzmann", self._target_T())
        elif tr.target_rule != "max":
            tr.set_target("max")
        key = (weights_key(self.eval_net, self._wgen), weights_key(self.target_net, self._wgen))
        if key != self._qtrain_key:
            tr.load(self.eval_net, self.target_net)
        cols = {"obs0": buf.obs0.data, "feat0": buf.feat0.data, "actions": buf.actions.data, "rewards": buf.rewards.data,
                "terminals": buf.terminals.data, "masks": buf.masks.data, "prob": buf.prob.data if use_mean else None}
        stats = tr.run(cols, n, torch.as_tensor(idx, device="cuda"))
        code, bad = tr.error()                      # the one synchronisation of the round
        tr.export(self.eval_net, self.target_net)
        self._qtrain_key = (weights_key(self.eval_net, self._wgen), weights_key(self.target_net, self._wgen))
        if code:
            from ..qtrain import QTrainError
            raise QTrainError("train_batches: device error %d (value %d); that minibatch and the later ones were not "
                              "applied" % (code, bad))
        st = stats.cpu().numpy()
        for i in range(0, batch_num, 50):
            print("[*] LOSS:", float(st[i, 0]), "/ Q:", {"Eval-Q": np.round(float(st[i, 1]), 6)})

    def _minibatch(self, buf, use_mean):
        """One sample + target + masked-MSE Adam step + soft update on the static index tensors."""
        i, j = self._s_idx, self._s_nxt
        # the minibatch rows: one HIP gather (k_rows_copy) per index list, into static tensors the
        # captured graph reuses (allocated by the first, eager call)
        cur = [buf.obs0, buf.feat0, buf.actions, buf.rewards, buf.terminals, buf.masks] + ([buf.prob] if use_mean else [])
        nxt = [buf.obs0, buf.feat0] + ([buf.prob] if use_mean else [])
        if getattr(self, "_mb", None) is None or self._mb[0][0].shape[0] != len(i):
            self._mb = [[torch.empty((len(i),) + tuple(b.data.shape[1:]), dtype=b.data.dtype, device="cuda")
                         for b in bufs] for bufs in (cur, nxt)]
        replay.rows_copy(self._mb[0], [b.data for b in cur], i)
        replay.rows_copy(self._mb[1], [b.data for b in nxt], j)
        obs, feat, acts, rew, done, mask = self._mb[0][:6]
        acts, mask = acts.long(), mask.float()
        obs_n, feat_n = self._mb[1][:2]
        prob = self._mb[0][6] if use_mean else None
        prob_n = self._mb[1][2] if use_mean else None
        with torch.no_grad():
            t_q = self.target_net(obs_n, feat_n, prob_n)
            e_qn = self.eval_net(obs_n, feat_n, prob_n)
            target = self._target(e_qn.float().contiguous(), t_q.float().contiguous(), rew, done,
                                  self._s_T if self._target_rule == "boltzmann" else None)
        e_q = self.eval_net(obs, feat, prob)
        e_q_max = e_q.gather(1, acts.reshape(-1, 1)).reshape(-1)
        loss = torch.sum(torch.square(target.float() - e_q_max) * mask) / torch.sum(mask)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.optimizer.step()
        with torch.no_grad():
            t_p = list(self.target_net.parameters())
            e_p = list(self.eval_net.parameters())
            torch._foreach_mul_(t_p, 1.0 - self.tau)
            torch._foreach_add_(t_p, torch._foreach_mul(e_p, self.tau))
            self._s_out[0].copy_(loss.detach())
            self._s_out[1].copy_(e_q_max.detach().mean())

    @torch.no_grad()
    def act_dev(self, **kwargs):
        """Device in, device out: int32 greedy actions (algo/base.py:228-254).  The Battle view runs the
        hand-written HIP forward (mfrl_amd.policy.QNetHIP, csrc/policy_kernels.hip; act_precision = "bf16":
        csrc/qnet_bf16_kernels.hip) with the eval net's current weights: argmax of e_q, the reference's argmax softmax(e_q / temperature) up to float ties.
        Other view shapes (not in the shipped configs) run the torch module.

        explore = "boltzmann" (opt-in): row i is drawn from softmax(e_q / eps) instead, with the uniform (self.seed,
        the count of acting calls, group 0, row i) -- fused into the HIP forward's epilogue for the Battle view,
        mfrl_amd.mf.q_sample on the torch module's Q values otherwise (2..32 actions).  eps must be finite and > 0."""
        view, feat = as_dev(kwargs["state"][0]), as_dev(kwargs["state"][1])
        self.temperature = kwargs["eps"]
        prob = self._prob(kwargs, len(view))
        if self.use_mf:
            assert len(prob) == len(view)
        if self._explore == "boltzmann":
            T = check_temperature(self.temperature)
            self._draws += 1
            if self.view_space == (13, 13, 7) and self.num_actions <= 32:
                return self._hip_current().act(view, feat, prob, temperature=T, seed=self.seed, step=self._draws)
            e_q = self.eval_net(view, feat, prob).float().contiguous()
            return mf.q_sample(e_q, T, self.seed, self._draws)
        if self.view_space == (13, 13, 7) and self.num_actions <= 32:
            return self._hip_current().act(view, feat, prob)
        e_q = self.eval_net(view, feat, prob)
        return torch.argmax(torch.softmax(e_q / self.temperature, dim=1), dim=1).to(torch.int32)

    def _hip_current(self):
        """The HIP forward (act_precision) holding the eval net's current weights: re-packed only when
        weights_key moved."""
        if getattr(self, "_hip", None) is None or self._hip.precision != self.act_precision:
            from ..policy import QNetHIP
            self._hip = QNetHIP(self.view_space, self.feature_space, self.num_actions, self.use_mf,
                                precision=self.act_precision)
            self._hip_key = None
        key = weights_key(self.eval_net, self._wgen)
        if key != self._hip_key:                     # the weights train() last left, packed once
            self._hip.load(self.eval_net)
            self._hip_key = key
        return self._hip

    @torch.no_grad()
    def act_rollout(self, eng, group, eps=None, prob_rows=None):
        """Greedy actions of group `group` of a BattleBatch's rollout from its observation buffers into its action
        buffer (mfrl_amd.policy.QNetHIP.act_rollout), with the eval net's current weights; nothing is read back.
        Streams: the weights -- however they moved: an optimiser step, load_state_dict, train_batches of either
        backend -- are packed and uploaded on the caller's current stream, which is where torch wrote them; the
        kernels run on the engine's.  The handle orders the two (mfrl_amd.policy.StreamOrder): every engine that acts
        with this model, on whatever stream, waits for the last upload once, the first time it acts after it.

        explore = "boltzmann": row j of env e is drawn from softmax(q / eps) with the uniform (self.seed, the count
        of acting calls, group, e * rowcap + j); eps None: self.temperature (the last eps, 0.1 at first).  With the
        default "greedy", eps is not used.

        prob_rows (None: the rollout's group mean): the mean action per agent, float32 [E, rowcap, A] on the device
        (mean_field = "neighbors": mfrl_amd.mf.NeighborMean.rows), handed to QNetHIP.act_rollout."""
        if not (self.view_space == (13, 13, 7) and self.num_actions <= 32):
            raise ValueError("act_rollout: the HIP forward takes the Battle view (13, 13, 7) and at most 32 actions")
        hip = self._hip_current()
        if self._explore == "boltzmann":
            if eps is not None:
                self.temperature = eps
            T = check_temperature(self.temperature)
            self._draws += 1
            hip.act_rollout(eng, group, temperature=T, seed=self.seed, step=self._draws, prob_rows=prob_rows)
            return
        hip.act_rollout(eng, group, prob_rows=prob_rows)

    def act(self, **kwargs):
        return self.act_dev(**kwargs).cpu().numpy().astype(np.int32)

    def train(self, **kwargs):
        """kwargs: state [obs, feature], target_q, prob, acts, masks -> (loss, {'Eval-Q', 'Target-Q'})."""
        obs, feat = as_dev(kwargs["state"][0]), as_dev(kwargs["state"][1])
        prob = self._prob(kwargs, len(obs))
        target = as_dev(kwargs["target_q"])
        mask = as_dev(kwargs["masks"])
        acts = as_dev(kwargs["acts"], torch.int64)
        e_q = self.eval_net(obs, feat, prob)
        e_q_max = e_q.gather(1, acts.reshape(-1, 1)).reshape(-1)
        loss = torch.sum(torch.square(target - e_q_max) * mask) / torch.sum(mask)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.optimizer.step()
        return loss.item(), {"Eval-Q": np.round(e_q_max.mean().item(), 6), "Target-Q": np.round(target.mean().item(), 6)}

    def _save(self, dir_path, prefix, step):
        import os
        os.makedirs(dir_path, exist_ok=True)
        path = os.path.join(dir_path, "{}_{}.pt".format(prefix, step))
        torch.save({"eval": self.eval_net.state_dict(), "target": self.target_net.state_dict()}, path)
        print("[*] Model saved at: {}".format(path))

    def _load(self, dir_path, prefix, step):
        import os
        path = os.path.join(dir_path, "{}_{}.pt".format(prefix, step))
        state = torch.load(path, map_location="cuda", weights_only=True)
        self.eval_net.load_state_dict(state["eval"])
        self.target_net.load_state_dict(state["target"])
        print("[*] Loaded model from {}".format(path))
