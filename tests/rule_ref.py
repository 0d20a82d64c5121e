"""The scripted rush / random opponent (csrc/rule_kernels.hip), restated in numpy: the contract the kernel
k_rule_act and mfrl_amd.algo.rule.RulePolicy are tested against.  One action per observation row, from that row alone.

Row: view [VH][VW][7] float32 as get_observation gives it to the observing group (0 wall, 1 own group, 3 own minimap,
4 enemy, 6 enemy minimap; both minimap channels carry +1 at the agent's own bin), feature [F] float32 whose last two
entries are x / W and y / H.  Tables: view2attack [VH][VW] (-1: not attackable), attack_base, move [attack_base][2] =
(mx, my).  Comparisons are on float32 as written; the arithmetic is integer.

  A  attack       the first row-major cell with enemy > 0.5 and view2attack >= 0: attack_base + view2attack
  B  in view      else, if any cell has enemy > 0.5: the one minimising (r - cy)^2 + (c - cx)^2 (first row-major on
                  ties); d = (c - cx, r - cy); move
  C  out of view  own bin = the first row-major cell with own minimap > 1.0; D = enemy minimap, minus 1.0f at the own
                  bin; target = the first row-major cell among those holding the largest D > 0.  With an own bin, a
                  target and target != own bin: d = 64 (sign(c - bx), sign(r - by)) (C-minimap); else
                  d = 64 (sign(0.5f - fx), sign(0.5f - fy)) (C-centre); move
  move            candidate a < attack_base is free if move[a] == (0, 0), or if (cy + my, cx + mx) lies inside the
                  view and has wall, own and enemy all <= 0.5; the free a minimising (dx - mx)^2 + (dy - my)^2, first
                  index on ties (0 if none is free)
  exploration     u1 = ac_uniform(seed, step, group, row); if u1 < eps the action is min(int(u2 * n_action),
                  n_action - 1) with u2 = ac_uniform(seed ^ 0x68E31DA4, step, group, row), the product in float32
"""
import numpy as np

import acnet_ref

CH_WALL, CH_OWN, CH_OWN_MM, CH_ENEMY, CH_ENEMY_MM = 0, 1, 3, 4, 6
N_CH = 7
SEED2 = 0x68E31DA4
TAG_A, TAG_B, TAG_C_MINIMAP, TAG_C_CENTRE, TAG_RANDOM = 0, 1, 2, 3, 4
TAG_NAMES = ("A", "B", "C-minimap", "C-centre", "random")


def circle_moves(speed):
    """The move offsets (mx, my) of a type of that speed, in action order: Range.h's circle of radius `speed`
    scanned row-major (AgentType.cc: move_range = CircleRange(speed, 0, 1))."""
    eps = 1e-8
    width = 2 * int(speed + eps) + 1
    if width % 2 != 1:
        width += 1
    center = int(speed)
    out = []
    for i in range(width):
        for j in range(width):
            dis = np.sqrt(float((j - center) ** 2 + (i - center) ** 2))
            if dis < speed + eps and dis > -eps:
                out.append((j - center, i - center))
    return np.array(out, dtype=np.int32)


def _sign(v):
    return (v > 0) - (v < 0)


def choose_move(view, d, move):
    """(the chosen move, whether the best move of all -- blocked or not -- was refused)."""
    VH, VW = view.shape[:2]
    cy, cx = VH // 2, VW // 2
    half = np.float32(0.5)
    best = best_any = None
    for a, (mx, my) in enumerate(move):
        mx, my = int(mx), int(my)
        free = mx == 0 and my == 0
        r, c = cy + my, cx + mx
        if not free and 0 <= r < VH and 0 <= c < VW:
            cell = view[r, c]
            free = bool(cell[CH_WALL] <= half and cell[CH_OWN] <= half and cell[CH_ENEMY] <= half)
        key = ((d[0] - mx) ** 2 + (d[1] - my) ** 2, a)
        if best_any is None or key < best_any[0]:
            best_any = (key, free)
        if free and (best is None or key < best):
            best = key
    return (best[1] if best is not None else 0), (best_any is not None and not best_any[1])


def rule_row(view, feat, v2a, attack_base, move):
    """(action, tag, best move refused) of one row, before exploration."""
    view = np.asarray(view, dtype=np.float32)
    VH, VW = view.shape[:2]
    cy, cx = VH // 2, VW // 2
    half, one = np.float32(0.5), np.float32(1.0)
    enemy = view[:, :, CH_ENEMY] > half
    hit = np.argwhere(enemy & (v2a >= 0))                       # (row-major order)
    if len(hit):
        r, c = hit[0]
        return attack_base + int(v2a[r, c]), TAG_A, False
    if enemy.any():
        cells = np.argwhere(enemy)
        dist = (cells[:, 0] - cy) ** 2 + (cells[:, 1] - cx) ** 2
        r, c = cells[int(np.argmin(dist))]                      # (argmin: the first minimum)
        d, tag = (int(c - cx), int(r - cy)), TAG_B
    else:
        own = np.argwhere(view[:, :, CH_OWN_MM] > one)
        D = view[:, :, CH_ENEMY_MM].copy()
        d = None
        if len(own):
            by, bx = own[0]
            D[by, bx] = np.float32(D[by, bx] - one)
            pos = D > 0
            if pos.any():
                top = np.argwhere(pos & (D == D[pos].max()))[0]
                if (top[0], top[1]) != (by, bx):
                    d, tag = (64 * _sign(int(top[1] - bx)), 64 * _sign(int(top[0] - by))), TAG_C_MINIMAP
        if d is None:
            fx, fy = np.float32(feat[-2]), np.float32(feat[-1])
            d, tag = (64 * _sign(float(np.float32(half - fx))), 64 * _sign(float(np.float32(half - fy)))), TAG_C_CENTRE
    a, refused = choose_move(view, d, move)
    return a, tag, refused


def rule_actions(view, feat, v2a, attack_base, n_action, move, eps=0.0, seed=0, step=0, group=0, rows=None):
    """view [n, VH, VW, 7], feat [n, F] -> (actions int32 [n], tags int32 [n], refused bool [n]); rows: the row of each
    uniform (None: 0..n-1; e * rowcap + j on a rollout)."""
    view = np.asarray(view, dtype=np.float32)
    feat = np.asarray(feat, dtype=np.float32)
    n = len(view)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    act = np.zeros(n, dtype=np.int32)
    tag = np.zeros(n, dtype=np.int32)
    refused = np.zeros(n, dtype=bool)
    eps = np.float32(eps)
    u1 = acnet_ref.uniforms(seed, step, group, rows) if n else np.zeros(0, np.float32)
    u2 = acnet_ref.uniforms(seed ^ SEED2, step, group, rows) if n else np.zeros(0, np.float32)
    for i in range(n):
        if u1[i] < eps:
            act[i] = min(int(np.float32(u2[i] * np.float32(n_action))), n_action - 1)
            tag[i] = TAG_RANDOM
            continue
        act[i], tag[i], refused[i] = rule_row(view[i], feat[i], v2a, attack_base, move)
    return act, tag, refused
