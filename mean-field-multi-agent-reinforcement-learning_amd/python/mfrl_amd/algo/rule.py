"""RulePolicy: the scripted opponents "rush" and "random" -- a fixed yardstick for the learned models, where self-play
and the tournament only compare one trained model with another.

The rule (mfrl_amd.policy.RuleHIP, csrc/rule_kernels.hip; restated in numpy in tests/rule_ref.py) gives one
action per observation row from that row alone: attack the first attackable enemy; else step toward the nearest enemy
in view; else toward the densest enemy bin of the minimap; else toward the centre of the map; a step whose destination
is taken goes to the next best free one.  With probability eps the action is uniform instead; "random" is eps = 1.  It
is this project's own deterministic rule, not the reference's rush_prey_infer_action.

A RulePolicy stands where a model stands: act / act_dev for play, play_batched and Runner, act_rollout for the device
rollout loops (battle_rollout, play_rollout*: it writes into the engine's action buffer like the networks).  It learns
nothing: train() raises, save() and load() do nothing.  It has no explore, mean_field or target_rule, so the loops
call it plainly, and the eps they pass -- the learned models' exploration -- is not the rule's: that is self.eps.
"""
import zlib

import numpy as np
import torch

RULES = ("rush", "random")


def check_supported(env, handle):
    """Refuse an env whose observation the rule would misread: it takes two groups, minimap mode on, no food / turn /
    goal mode, 1 x 1 bodies (the 7-channel view: wall, own, own hp, own minimap, enemy, enemy hp, enemy minimap)."""
    def refuse(why):
        raise ValueError("RulePolicy: unsupported config: %s (the rule reads the Battle shape: 2 groups, minimap on, 7 "
                         "channels, no turn / food mode, 1 x 1 bodies)" % why)
    if len(env.get_handles()) != 2:
        refuse("%d groups" % len(env.get_handles()))
    vs = tuple(env.get_view_space(handle))
    if len(vs) != 3 or vs[2] != 7:
        refuse("a view of shape %s" % (vs,))
    if vs[0] * vs[1] > 256:
        refuse("a view of %d x %d cells (at most 256)" % (vs[0], vs[1]))
    n_action = env.get_action_space(handle)[0]
    if not 2 <= n_action <= 64:
        refuse("%d actions (2..64)" % n_action)
    cfg = getattr(env, "_config", None)
    if cfg is not None:
        for key in ("turn_mode", "food_mode", "goal_mode"):
            if cfg.config_dict.get(key, False):
                refuse(key)
        if not cfg.config_dict.get("minimap_mode", False):
            refuse("minimap_mode off")
        for name in cfg.groups:
            t = cfg.agent_type_dict[name]
            if int(t.get("width", 1)) != 1 or int(t.get("length", 1)) != 1:
                refuse("type %s has a %d x %d body" % (name, t.get("width", 1), t.get("length", 1)))


class RulePolicy:
    def __init__(self, sess, name, handle, env, rule="rush", eps=0.0):
        if rule not in RULES:
            raise ValueError("RulePolicy: rule %r (one of %s)" % (rule, ", ".join(RULES)))
        eps = 1.0 if rule == "random" else float(eps)
        if not 0.0 <= eps <= 1.0:                     # (false for NaN)
            raise ValueError("RulePolicy: eps must be in [0, 1], got %r" % (eps,))
        check_supported(env, handle)
        from ..policy import RuleHIP
        self.env = env
        self.name = name
        self.name_scope = name
        self.handle = handle
        self.rule = rule
        self.eps = eps
        self.view_space = tuple(env.get_view_space(handle))
        self.feature_space = tuple(env.get_feature_space(handle))
        self.num_actions = env.get_action_space(handle)[0]
        self.group = handle.value if hasattr(handle, "value") else int(handle)
        attack_base, v2a = env.get_view2attack(handle)
        self._hip = RuleHIP(self.view_space, self.feature_space, self.num_actions, attack_base, v2a,
                            env.get_move_delta(handle))
        self._draws = 0             # acting calls: the step counter of the exploration draw
        # the draw's seed, made as the models make theirs: the run's torch seed mixed with the name
        self.seed = zlib.crc32(("rule/%s/%d" % (name, torch.initial_seed())).encode())

    @property
    def vars(self):
        return []

    @torch.no_grad()
    def act_dev(self, **kwargs):
        """Device in, device out: int32 actions of the rows of kwargs["state"] = [view, feature].  prob and eps (the
        learned models' inputs) are accepted and not read; the rule explores with self.eps."""
        from .base import as_dev
        view, feat = as_dev(kwargs["state"][0]), as_dev(kwargs["state"][1])
        self._draws += 1
        return self._hip.act(view, feat, eps=self.eps, seed=self.seed, step=self._draws, group=self.group)

    def act(self, **kwargs):
        return self.act_dev(**kwargs).cpu().numpy().astype(np.int32)

    def act_rollout(self, eng, group, prob_rows=None):
        """Actions of group `group` of a BattleBatch's rollout from its observation buffers into its action buffer;
        nothing is read back.  prob_rows is accepted and not read."""
        self._draws += 1
        self._hip.act_rollout(eng, group, eps=self.eps, seed=self.seed, step=self._draws)

    def flush_buffer(self, **kwargs):
        pass

    def train(self):
        raise TypeError("RulePolicy %r is a scripted opponent: it does not train" % self.name)

    def save(self, dir_path, step=0):
        pass

    def load(self, dir_path, step=0):
        print("[*] {} is the scripted rule '{}': nothing to load".format(self.name, self.rule))
