"""The neighbourhood mean action (include/magent_amd.h part 4b) restated in numpy: brute force over pairs,
(count / n) in float64, cast to float32.  Test infrastructure only.

    compact(pos, actions, n_action, radius)                      one compact list -> [n, n_action] float32
    rollout(actions, alive, prev_num, pos, n_action, radius, restart)   the rollout form's inputs -> the same
    positions(feature, map_w, map_h)                             the position decode of the rollout form
"""
import numpy as np


def compact(pos, actions, n_action, radius):
    """pos int [n, 2] (x, y), actions int [n] -> float32 [n, n_action]: row j = the mean of the one-hot actions of the
    members k with max(|x_k - x_j|, |y_k - y_j|) <= radius (j included); an action outside [0, n_action) is counted in
    no entry while the divisor stays."""
    pos = np.asarray(pos, dtype=np.int64).reshape(-1, 2)
    actions = np.asarray(actions, dtype=np.int64).reshape(-1)
    n = len(actions)
    assert len(pos) == n
    out = np.zeros((n, n_action), dtype=np.float32)
    for j in range(n):
        cnt = np.zeros(n_action, dtype=np.int64)
        members = 0
        for k in range(n):
            if max(abs(int(pos[k, 0]) - int(pos[j, 0])), abs(int(pos[k, 1]) - int(pos[j, 1]))) <= radius:
                members += 1
                if 0 <= actions[k] < n_action:
                    cnt[actions[k]] += 1
        out[j] = (cnt.astype(np.float64) / np.float64(members)).astype(np.float32)
    return out


def positions(feature, map_w, map_h):
    """feature float32 [n, F] -> int [n, 2]: x = rint(feat[F - 2] * W), y = rint(feat[F - 1] * H), in float32 as the
    kernel computes it."""
    f = np.asarray(feature, dtype=np.float32)
    x = np.rint(f[:, -2] * np.float32(map_w)).astype(np.int64)
    y = np.rint(f[:, -1] * np.float32(map_h)).astype(np.int64)
    return np.stack([x, y], axis=1)


def rollout(actions, alive, prev_num, pos, n_action, radius, restart):
    """The rollout form for one (env, group): actions int [>= prev_num] and alive [>= prev_num] in the order of before
    clear_dead, prev_num the group's size before the step, pos int [n, 2] the survivors' positions in the order of the
    new observation -> float32 [n, n_action].  Survivor j's action is that of the j-th row with alive != 0 among the
    first prev_num; restart: all zero."""
    pos = np.asarray(pos, dtype=np.int64).reshape(-1, 2)
    n = len(pos)
    if restart:
        return np.zeros((n, n_action), dtype=np.float32)
    alive = np.asarray(alive)[:prev_num] != 0
    acts = np.asarray(actions, dtype=np.int64)[:prev_num][alive]
    assert len(acts) == n, "%d survivors for %d rows of the new observation" % (len(acts), n)
    return compact(pos, acts, n_action, radius)


# ---- the inputs the CPU and GPU tests share
def checkerboard(map_w, map_h, side):
    """The cells of the central side x side block, (x + y) even to group 0 and odd to group 1: the two groups start
    interleaved, so attacks land from the first step on."""
    x0, y0 = (map_w - side) // 2, (map_h - side) // 2
    cells = [(x, y) for x in range(x0, x0 + side) for y in range(y0, y0 + side)]
    return ([[x, y, 0] for x, y in cells if (x + y) % 2 == 0], [[x, y, 0] for x, y in cells if (x + y) % 2 == 1])


def draw_actions(rng, n, n_action, attack_base, p_attack=0.6):
    """n actions from `rng`: with probability p_attack one of the attack ids [attack_base, n_action), else any id."""
    u = rng.random_sample(n)
    att = rng.randint(attack_base, n_action, size=n)
    other = rng.randint(0, n_action, size=n)
    return np.where(u < p_attack, att, other).astype(np.int32)
