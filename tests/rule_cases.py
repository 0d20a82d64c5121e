"""Test infrastructure: the synthetic tables and rows that the rule tests share (tests/test_rule_gpu.py,
tests/test_rule_shapes_gpu.py, tests/test_rowmap_gpu.py on the GPU; tests/test_rule_cpu.py pins their preconditions on
the restatement tests/rule_ref.py without one).  Everything is a function of its arguments and cached; nobody writes
to the arrays."""
import numpy as np

import rule_ref as rr

EPS, SEED = 0.2, 4242
NS = (1, 63, 65, 1000)

# (VH, VW) off the square view, and what each reaches in k_rule_act (cells = VH * VW, VF = 7 cells floats):
#   (9, 13), (13, 9)  non-square, both ways: every / VW, % VW and * VW differs from the same with VH
#   (16, 16)          256 cells: VF & 3 = 0 (no dword tail), four full ballot passes, atk[3] in use
#   (6, 7)            42 cells: one partial pass, tail 2
#   (3, 5)            15 cells: tail 1
#   (4, 64)           256 cells as a strip: cx = 32, a view row is one whole ballot pass
SHAPES = [(9, 13), (13, 9), (16, 16), (6, 7), (3, 5), (4, 64)]
# added to the generator's seed per shape: the first from 0 on at which the transposed view changes the restatement's
# action on at least 10 % of the 1000 rows (tests/test_rule_cpu.py::test_shape_rows_take_every_branch).  The non-square
# shapes change 40 .. 50 % with seed 0.  On the square one the transposed view is the same view, and only the attack
# table's transpose shows, on the rows that attack off the diagonal: 9.6 % with seed 0, 10.2 % with seed 1.
SHAPE_SEED = {(16, 16): 1}


def tables(VH, VW):
    """Synthetic tables of a VH x VW view: the 8 cells around the centre attack, the moves of speed 2 (speed 1 in a
    view under 7 cells high or wide, whose 13-move circle would leave the view)."""
    move = rr.circle_moves(1 if min(VH, VW) < 7 else 2)
    v2a = np.full((VH, VW), -1, dtype=np.int32)
    k = 0
    for r in range(VH // 2 - 1, VH // 2 + 2):
        for c in range(VW // 2 - 1, VW // 2 + 2):
            if (r, c) != (VH // 2, VW // 2):
                v2a[r, c] = k
                k += 1
    return v2a, len(move), len(move) + 8, move


_ROWS = {}


def synthetic(VH, VW, n=1000, seed=0, F=12):
    """n rows of a VH x VW x 7 view and F features, five kinds in turn so that every branch is taken: a sparse enemy
    fill (A or B), one far enemy among walls and own agents (B, moves refused), no enemy and a minimap with the own
    bin marked (C-minimap, moves refused), no enemy and an empty minimap (C-centre; x / W and y / H on either side
    of and exactly at 0.5), and every channel filled at random; a third of the minimap rows carry exactly 1.0 at the
    own bin, i.e. no own bin (> 1.0), which sends them to the centre.  Made once per shape, never modified."""
    key = (VH, VW, n, seed, F)
    if key in _ROWS:
        return _ROWS[key]
    rng = np.random.RandomState(1000 * VH + VW + seed)
    view = np.zeros((n, VH, VW, 7), dtype=np.float32)
    feat = rng.uniform(0, 1, size=(n, F)).astype(np.float32)
    feat[:, -2:] = rng.choice(np.array([0.25, 0.5, 0.75], dtype=np.float32), size=(n, 2))
    for i in range(n):
        kind, v = i % 5, view[i]
        v[VH // 2, VW // 2, rr.CH_OWN] = 1
        if kind == 0:
            v[:, :, rr.CH_ENEMY] = rng.uniform(size=(VH, VW)) < 0.04
            v[VH // 2, VW // 2, rr.CH_ENEMY] = 0
        elif kind == 1:
            edge = [(r, c) for r in range(VH) for c in range(VW) if r in (0, VH - 1) or c in (0, VW - 1)]
            r, c = edge[rng.randint(len(edge))]
            v[r, c, rr.CH_ENEMY] = 1
            v[:, :, rr.CH_WALL] = rng.uniform(size=(VH, VW)) < 0.3
            v[:, :, rr.CH_OWN] = rng.uniform(size=(VH, VW)) < 0.3
            v[r, c, rr.CH_WALL] = v[r, c, rr.CH_OWN] = 0
        elif kind in (2, 3):
            own = rng.randint(VH), rng.randint(VW)
            v[:, :, rr.CH_OWN_MM] = (rng.uniform(size=(VH, VW)) < 0.1) * np.float32(0.125)
            v[own[0], own[1], rr.CH_OWN_MM] += 1
            if i % 3:                                            # (else often exactly 1.0: a row without an own bin)
                v[own[0], own[1], rr.CH_OWN_MM] = np.float32(1.125)
            if kind == 2:
                v[:, :, rr.CH_ENEMY_MM] = rng.randint(0, 4, size=(VH, VW)) * (rng.uniform(size=(VH, VW)) < 0.2) * np.float32(0.0625)
                v[:, :, rr.CH_WALL] = rng.uniform(size=(VH, VW)) < 0.3
            elif i % 2:
                v[:, :, rr.CH_ENEMY_MM] = np.float32(0.25) * (rng.uniform() < 0.5)      # (flat: only the own bin's + 1 stands out)
            v[own[0], own[1], rr.CH_ENEMY_MM] += 1
        else:
            view[i] = (rng.uniform(size=(VH, VW, 7)) < 0.15) * rng.choice(np.array([0.5, 1.0, 2.0], np.float32), size=(VH, VW, 7))
    _ROWS[key] = (view, feat)
    return _ROWS[key]


def shape_rows(shape):
    """The 1000 rows of one of SHAPES (12 features, the shape's own seed)."""
    return synthetic(shape[0], shape[1], seed=SHAPE_SEED.get(tuple(shape), 0))


# ------------------------------------------------------------------------------------------------- the range's ends
def strip_tables():
    """(4, 64), all moves: attack_base = n_action = 64 (the move argmin runs over all 64 lanes; the random draw reaches
    action 63), no attack cell, and the handle is made with F = 2.  The moves, in action order: (0, 0), (+-16, 0),
    (+-8, +-1), then 57 more inside the view and the contract's 16 cells (|mx| <= 15, my in -2 .. 1), all distinct."""
    VH, VW = 4, 64
    move = [(0, 0), (16, 0), (-16, 0), (8, 1), (8, -1), (-8, 1), (-8, -1)]
    rest = [(mx, my) for my in (0, -1, 1, -2) for mx in (1, -1, 2, -2, 3, -3, 5, -5, 6, -6, 11, -11, 13, -13, 15, -15)]
    move += [m for m in rest if m not in move][:64 - len(move)]
    move = np.array(move, dtype=np.int32)
    assert len(move) == 64 and len({tuple(m) for m in move.tolist()}) == 64
    return np.full((VH, VW), -1, dtype=np.int32), 64, 64, move


def many_tables():
    """(16, 16), many actions: circle_moves(4) gives 49 moves, plus the 8 attacks around the centre: n_action = 57."""
    VH = VW = 16
    v2a = tables(VH, VW)[0]
    move = rr.circle_moves(4)
    assert len(move) == 49
    return v2a, 49, 57, move


HAND_MADE = {"strip": ((4, 64), 2, strip_tables), "many": ((16, 16), 12, many_tables)}


def hand_made(name):
    """-> ((VH, VW), F, (v2a, attack_base, n_action, move), (view, feat)) of a hand-made table; the rows are the
    synthetic generator's at that shape with F features."""
    shape, F, tab = HAND_MADE[name]
    return shape, F, tab(), synthetic(shape[0], shape[1], seed=SHAPE_SEED.get(shape, 0), F=F)


_WANT = {}


def restated(key, view, feat, tab, eps=EPS, seed=SEED, step=1000, group=0):
    """rule_ref.rule_actions of the whole row set, cached under `key` (the restatement is a Python loop per row)."""
    k = (key, eps, seed, step, group)
    if k not in _WANT:
        v2a, base, n_action, move = tab
        _WANT[k] = rr.rule_actions(view, feat, v2a, base, n_action, move, eps, seed, step, group)
    return _WANT[k]
