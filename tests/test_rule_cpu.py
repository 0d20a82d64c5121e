"""The scripted rush / random opponent without a GPU: the numpy restatement (tests/rule_ref.py) driven
on the C oracle, so that the restatement and the kernel cannot share one wrong idea of the geometry; the blocked-move
choice on hand-built rows; the exploration draw; RulePolicy's interface and the command-line refusals."""
import itertools

import numpy as np
import pytest

import acnet_ref
import common
import rule_cases as rc
import rule_ref as rr

MAP, CENTRE, STAY = 40, (20, 20), 6            # STAY: the move (0, 0) of a speed-2 type
MOVE = rr.circle_moves(2)


def _env(pos0, pos1):
    env, h = common.battle_env(common.ORACLE_LIB, MAP)
    env.reset()
    for g, pos in enumerate((pos0, pos1)):
        if pos:
            env.add_agents(h[g], method="custom", pos=[[x, y, 0] for x, y in pos])
    return env, h


def _tables(env, h):
    attack_base, v2a = env.get_view2attack(h[0])
    return v2a, attack_base, env.get_action_space(h[0])[0]


def _rule(env, h, g):
    """(action, tag) of the only agent of group g on its oracle observation."""
    v2a, base, n_action = _tables(env, h)
    view, feat = env.get_observation(h[g])
    act, tag, _ = rr.rule_actions(view, feat, v2a, base, n_action, MOVE)
    return int(act[0]), int(tag[0])


def _step(env, h, g, action):
    """The observer of group g takes `action`, everyone else stays."""
    for k in range(2):
        n = env.get_num(h[k])
        a = np.full(n, STAY, dtype=np.int32)
        if k == g:
            a[0] = action
        env.set_action(h[k], a)
    env.step()


def _dist2(a, b):
    return int((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2)


def test_move_table_is_the_engines():
    """rule_ref.circle_moves (the oracle has no move getter) equals env_get_info("move_delta") of the HIP engine,
    which answers it on the host, and both are the 13 moves of the Battle type in action order."""
    import magent
    env = magent.GridWorld("battle", map_size=MAP, lib=magent.load_library(common.HIP_LIB))
    h = env.get_handles()
    for g in range(2):
        got = env.get_move_delta(h[g])
        assert got.dtype == np.int32 and np.array_equal(got, MOVE)
    assert len(MOVE) == 13 and tuple(MOVE[STAY]) == (0, 0) and tuple(MOVE[0]) == (0, -2) and tuple(MOVE[8]) == (2, 0)
    assert env.get_view2attack(h[0])[0] == 13


@pytest.mark.parametrize("g", [0, 1])
def test_every_cell_of_the_view_on_the_oracle(g):
    """One observer of group g at the centre of a 40 x 40 map and one enemy on each cell of its view circle in turn:
    on an attack cell the action is that attack and the enemy's hp drops; on any other cell the rule takes branch B
    and the squared distance is strictly smaller after the step."""
    y, x = np.mgrid[-6:7, -6:7]
    cells = [(int(a), int(b)) for a, b in zip(x.ravel(), y.ravel()) if 0 < a * a + b * b <= 36]
    assert len(cells) == 112
    attacks = 0
    for dx, dy in cells:
        me, foe = CENTRE, (CENTRE[0] + dx, CENTRE[1] + dy)
        env, h = _env(*([me], [foe]) if g == 0 else ([foe], [me]))
        v2a, base, _ = _tables(env, h)
        action, tag = _rule(env, h, g)
        if v2a[6 + dy, 6 + dx] >= 0:
            attacks += 1
            assert tag == rr.TAG_A and action == base + v2a[6 + dy, 6 + dx], (dx, dy)
            _step(env, h, g, action)
            view, _ = env.get_observation(h[g])
            assert 0 < view[0, 6 + dy, 6 + dx, 5] < 1.0, (dx, dy)            # (the enemy's hp / its full hp)
            assert tuple(env.get_pos(h[g])[0]) == me
        else:
            assert tag == rr.TAG_B and action < base, (dx, dy)
            _step(env, h, g, action)
            assert _dist2(env.get_pos(h[g])[0], foe) < dx * dx + dy * dy, (dx, dy)
    assert attacks == 8


@pytest.mark.parametrize("g", [0, 1])
def test_enemy_out_of_view_on_the_oracle(g):
    """The enemy 15 cells away in each of the 8 directions: the minimap branch, and the distance shrinks."""
    for sx, sy in itertools.product((-1, 0, 1), repeat=2):
        if (sx, sy) == (0, 0):
            continue
        me, foe = CENTRE, (CENTRE[0] + 15 * sx, CENTRE[1] + 15 * sy)
        env, h = _env(*([me], [foe]) if g == 0 else ([foe], [me]))
        action, tag = _rule(env, h, g)
        assert tag == rr.TAG_C_MINIMAP, (sx, sy)
        _step(env, h, g, action)
        assert _dist2(env.get_pos(h[g])[0], foe) < 225 * (sx * sx + sy * sy), (sx, sy)


@pytest.mark.parametrize("g", [0, 1])
def test_no_enemy_goes_to_the_centre_on_the_oracle(g):
    """No enemy at all (its minimap is 0 / 0 there): off-centre the observer moves toward the centre, at the exact
    centre it stays."""
    for me in ((10, 30), (30, 10), (20, 5), (33, 20)):
        env, h = _env(*([me], []) if g == 0 else ([], [me]))
        action, tag = _rule(env, h, g)
        assert tag == rr.TAG_C_CENTRE
        _step(env, h, g, action)
        assert _dist2(env.get_pos(h[g])[0], CENTRE) < _dist2(me, CENTRE), me
    env, h = _env(*([CENTRE], []) if g == 0 else ([], [CENTRE]))
    action, tag = _rule(env, h, g)
    assert tag == rr.TAG_C_CENTRE and action == STAY
    _step(env, h, g, action)
    assert tuple(env.get_pos(h[g])[0]) == CENTRE


def test_blocked_move_on_the_oracle():
    """A wall and an own agent on the two best destinations toward an enemy in view: the chosen destination is free
    and the agent arrives there."""
    me, foe = CENTRE, (CENTRE[0] + 5, CENTRE[1])
    env, h = _env([me, (CENTRE[0] + 1, CENTRE[1])], [foe])                 # own agent on (+1, 0)
    env.add_walls(method="custom", pos=[[CENTRE[0] + 2, CENTRE[1]]])        # wall on (+2, 0), the best destination
    v2a, base, n_action = _tables(env, h)
    view, feat = env.get_observation(h[0])
    act, tag, refused = rr.rule_actions(view, feat, v2a, base, n_action, MOVE)
    assert tag[0] == rr.TAG_B and refused[0]
    mx, my = MOVE[act[0]]
    assert (mx, my) in ((1, -1), (1, 1)) and act[0] == 3                   # (the first of the two next-best moves)
    _step(env, h, 0, int(act[0]))
    assert tuple(env.get_pos(h[0])[0]) == (me[0] + mx, me[1] + my)


def test_blocked_patterns_on_hand_built_rows():
    """Every free / blocked pattern of the 13 move cells (walls and own agents as blockers), four targets: the chosen
    move is free, it is the nearest free one to the target (first index on ties), and `refused` says whether the
    nearest move of all was blocked."""
    v2a = np.full((13, 13), -1, dtype=np.int32)
    feat = np.zeros(34, dtype=np.float32)
    checked = refused_n = 0
    for target in ((0, 6), (12, 12), (6, 0), (9, 2)):                      # (row, col) of the enemy in view
        d = np.array([target[1] - 6, target[0] - 6])
        cost = ((d[None, :] - MOVE) ** 2).sum(1)
        for pattern in range(1 << 13):
            view = np.zeros((13, 13, 7), dtype=np.float32)
            view[target[0], target[1], rr.CH_ENEMY] = 1
            blocked = np.array([(pattern >> a) & 1 for a in range(13)], dtype=bool)
            for a in np.nonzero(blocked)[0]:
                view[6 + MOVE[a, 1], 6 + MOVE[a, 0], rr.CH_WALL if (a + pattern) % 2 else rr.CH_OWN] = 1
            free = ~blocked
            free[STAY] = True                                               # (standing still is always allowed)
            act, tag, refused = rr.rule_row(view, feat, v2a, 13, MOVE)
            assert tag == rr.TAG_B and free[act], (target, pattern)
            want = int(np.argmin(np.where(free, cost, 1 << 30)))
            assert act == want, (target, pattern)
            assert refused == bool(blocked[int(np.argmin(cost))] and int(np.argmin(cost)) != STAY), (target, pattern)
            checked += 1
            refused_n += refused
    assert checked == 4 << 13 and 0 < refused_n < checked


def test_exploration_draw():
    """eps = 0 never takes the random branch, eps = 1 always does; the uniforms are acnet_ref's restatement of
    ac_uniform; over 20,000 rows at eps = 1 every action occurs."""
    n, A = 20000, 21
    v2a = np.full((13, 13), -1, dtype=np.int32)
    view = np.zeros((n, 13, 13, 7), dtype=np.float32)
    feat = np.full((n, 34), 0.5, dtype=np.float32)
    rows = np.arange(n) * 3 + 1
    act, tag, _ = rr.rule_actions(view[:200], feat[:200], v2a, 13, A, MOVE, eps=0.0, seed=9, step=4, group=1, rows=rows[:200])
    assert (tag == rr.TAG_C_CENTRE).all() and (act == STAY).all()
    act, tag, _ = rr.rule_actions(view, feat, v2a, 13, A, MOVE, eps=1.0, seed=9, step=4, group=1, rows=rows)
    assert (tag == rr.TAG_RANDOM).all()
    u2 = acnet_ref.uniforms(9 ^ 0x68E31DA4, 4, 1, rows)
    want = np.minimum((u2 * np.float32(A)).astype(np.float32).astype(np.int32), A - 1)
    assert np.array_equal(act, want)
    assert np.array_equal(np.unique(act), np.arange(A))
    # a share in between: the rows whose first uniform is below eps, and only those
    act, tag, _ = rr.rule_actions(view[:2000], feat[:2000], v2a, 13, A, MOVE, eps=0.25, seed=9, step=4, group=1, rows=rows[:2000])
    u1 = acnet_ref.uniforms(9, 4, 1, rows[:2000])
    assert np.array_equal(tag == rr.TAG_RANDOM, u1 < np.float32(0.25)) and 400 < (tag == rr.TAG_RANDOM).sum() < 600
    assert np.array_equal(act[tag == rr.TAG_RANDOM], want[:2000][tag == rr.TAG_RANDOM])


def _play_restatement(left_id, eps, max_steps=100):
    """One 40 x 40 episode on the C oracle: group 0 on the rule at eps[0], group 1 at eps[1]; -> kills per group."""
    import battle_driver as bd
    _, left, right = bd.generate_map_positions(MAP, 0)
    pos = [None, None]
    pos[left_id], pos[1 - left_id] = left, right
    env, h = common.battle_env(common.ORACLE_LIB, MAP)
    env.reset()
    for g in range(2):
        env.add_agents(h[g], method="custom", pos=pos[g])
    v2a, base, n_action = _tables(env, h)
    start = [env.get_num(x) for x in h]
    nums = list(start)
    for t in range(max_steps):
        for g in range(2):
            view, feat = env.get_observation(h[g])
            act, _, _ = rr.rule_actions(view, feat, v2a, base, n_action, MOVE, eps=eps[g], seed=77 + g, step=t, group=g)
            env.set_action(h[g], act)
        done = env.step()
        nums = [int(env.get_alive(x).sum()) for x in h]
        env.clear_dead()
        if done:
            break
    return [start[1] - nums[1], start[0] - nums[0]]


def test_rush_out_kills_random_on_the_oracle():
    """The rule plays: over one episode per side of the map, rush (eps 0) kills more than random (eps 1) does."""
    kills = np.sum([_play_restatement(left_id, (0.0, 1.0)) for left_id in (0, 1)], axis=0)
    print("kills rush / random: %d / %d" % (kills[0], kills[1]))
    assert kills[0] > kills[1] and kills[0] > 0


# ------------------------------------------------------------------------------------------------- the interface
def test_spawn_ai_gives_a_rule_policy():
    import magent
    from mfrl_amd.algo import spawn_ai
    from mfrl_amd.algo.rule import RulePolicy
    env = magent.GridWorld("battle", map_size=MAP, lib=magent.load_library(common.HIP_LIB))
    h = env.get_handles()
    rush, rnd = spawn_ai("rush", None, env, h[0], "rush-me", 100), spawn_ai("random", None, env, h[1], "random-op", 100)
    assert isinstance(rush, RulePolicy) and isinstance(rnd, RulePolicy)
    assert (rush.rule, rush.eps, rnd.rule, rnd.eps) == ("rush", 0.0, "random", 1.0)
    assert rush.seed != rnd.seed and rush.num_actions == 21 and rush.view_space == (13, 13, 7)
    for m in (rush, rnd):
        with pytest.raises(TypeError):
            m.train()
        assert m.flush_buffer(state=None) is None and m.save("/nonexistent") is None and m.load("/nonexistent") is None
        assert not any(hasattr(m, a) for a in ("explore", "mean_field", "target_rule"))
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            RulePolicy(None, "x", h[0], env, eps=bad)
    with pytest.raises(ValueError):
        RulePolicy(None, "x", h[0], env, rule="gather")


def test_unsupported_configs_are_refused():
    """pursuit (no minimap, a 2 x 2 body) and a Battle-like config in turn mode are refused at construction."""
    import magent
    from mfrl_amd.algo.rule import RulePolicy
    lib = magent.load_library(common.HIP_LIB)
    env = magent.GridWorld("pursuit", map_size=MAP, lib=lib)
    for h in env.get_handles():
        with pytest.raises(ValueError, match="unsupported config"):
            RulePolicy(None, "x", h, env)
    gw = magent.gridworld
    for extra, body in (({"turn_mode": True}, 1), ({}, 3)):
        cfg = gw.Config()
        cfg.set(dict({"map_width": MAP, "map_height": MAP, "minimap_mode": True, "embedding_size": 10}, **extra))
        t = cfg.register_agent_type("t", dict(width=body, length=body, hp=10, speed=2, damage=2,
                                              view_range=gw.CircleRange(6), attack_range=gw.CircleRange(1.5)))
        cfg.add_group(t)
        cfg.add_group(t)
        env = magent.GridWorld(cfg, lib=lib)
        assert env.get_view_space(env.get_handles()[0])[2] == 7
        with pytest.raises(ValueError, match="unsupported config"):
            RulePolicy(None, "x", env.get_handles()[0], env)


def test_rule_create_refuses_on_the_host():
    """mfx_rule_create: a 17 x 17 view, other channel counts, action counts and tables out of range give -1 with a
    message, on the host."""
    import ctypes
    from mfrl_amd import lib
    from mfrl_amd.policy import RuleHIP
    from magent.c_lib import EngineError
    v2a = np.full((13, 13), -1, dtype=np.int32)
    RuleHIP((13, 13, 7), (34,), 21, 13, v2a, MOVE)
    RuleHIP((16, 16, 7), (34,), 21, 13, np.full((16, 16), -1, np.int32), MOVE)
    for vs, F, A, base, table, move in (((17, 17, 7), 34, 21, 13, np.full((17, 17), -1, np.int32), MOVE),
                                        ((13, 13, 5), 34, 21, 13, v2a, MOVE),
                                        ((13, 13, 7), 1, 21, 13, v2a, MOVE),
                                        ((13, 13, 7), 34, 65, 13, v2a, MOVE),
                                        ((13, 13, 7), 34, 1, 1, v2a, MOVE[:1]),
                                        ((13, 13, 7), 34, 21, 13, np.full((13, 13), 8, np.int32), MOVE),
                                        ((13, 13, 7), 34, 21, 13, v2a, MOVE * 9)):
        with pytest.raises(EngineError):
            RuleHIP(vs, (F,), A, base, table, move)
        assert lib().mfx_last_error()
    with pytest.raises(ValueError):
        RuleHIP((13, 13, 7), (34,), 21, 15, v2a, MOVE)                   # (turn mode: attack_base past the moves)
    L = lib()
    L.mfx_rule_create.restype = ctypes.c_int
    assert L.mfx_rule_create(None, 13, 21, None, None, None, None) == -1


@pytest.mark.parametrize("argv", [
    ["--algo", "mfq", "--oppo", "mfac", "--idx", "5"],                    # two learned sides: two steps
    ["--algo", "mfq", "--oppo", "rush", "--idx", "5", "6"],               # one learned side: one step
    ["--algo", "mfq", "--oppo", "rush"],
    ["--algo", "random", "--oppo", "ac", "--idx", "5", "6"],
    ["--algo", "rush", "--oppo", "random", "--idx", "5"],                 # none: no step
    ["--algo", "rush", "--rule_eps", "1.5"],
    ["--algo", "rush", "--rule_eps", "-0.1"],
    ["--algo", "rush", "--rule_eps", "nan"],
    ["--algo", "mfq", "--untrained", "--rule_eps", "0.1"],                # no rule side
    ["--algo", "random", "--rule_eps", "0.1"],                            # random is eps = 1
])
def test_battle_eval_refuses(argv, capsys):
    from mfrl_amd import battle_eval
    with pytest.raises(SystemExit) as ex:
        battle_eval.main(argv)
    assert ex.value.code == 2
    err = capsys.readouterr().err
    assert "--idx" in err or "--rule_eps" in err


@pytest.mark.parametrize("argv", [
    ["--algo", "mfq", "--eval_oppo", "rush"],
    ["--algo", "mfq", "--eval_eps", "0.1"],
    ["--algo", "mfq", "--eval_every", "-1"],
    ["--algo", "mfq", "--eval_every", "1", "--eval_eps", "2"],
    ["--algo", "mfq", "--eval_every", "1", "--eval_oppo", "random", "--eval_eps", "0.5"],
    ["--algo", "mfq", "--eval_every", "1", "--eval_envs", "0"],
])
def test_train_battle_refuses(argv, capsys):
    from mfrl_amd import train_battle
    with pytest.raises(SystemExit) as ex:
        train_battle.main(argv)
    assert ex.value.code == 2
    assert "--eval_" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------- the off-square shapes
# Preconditions of tests/test_rule_shapes_gpu.py and tests/test_rowmap_gpu.py: properties of the restatement on the
# shared rows (tests/rule_cases.py), so that a kernel that is wrong off the square view cannot pass there unseen.
def _transposed(view, v2a):
    """The same floats read as a (VW, VH) view, with the attack table transposed: what a kernel that takes VH for VW
    everywhere makes of the row."""
    n, VH, VW = view.shape[:3]
    return view.reshape(n, VW, VH, 7), np.ascontiguousarray(v2a.T)


@pytest.mark.parametrize("shape", rc.SHAPES)
def test_shape_rows_take_every_branch(shape):
    """On each shape's 1000 rows (eps 0.2) every branch tag occurs, at least one best move is refused, moves and
    attacks both occur; and the restatement on the transposed view differs on at least 10 % of the rows (a floor for
    the inputs: a shape that misses it gets another seed in rule_cases.SHAPE_SEED, never a lower floor)."""
    tab = rc.tables(*shape)
    v2a, base, n_action, move = tab
    view, feat = rc.shape_rows(shape)
    want, tag, refused = rc.restated(shape, view, feat, tab)
    counts = np.bincount(tag, minlength=5)
    print("%s: tags %s, refused %d" % (shape, dict(zip(rr.TAG_NAMES, counts.tolist())), int(refused.sum())))
    assert (counts >= 1).all() and refused.sum() >= 1
    assert 0 <= want.min() and want.max() < n_action and len(np.unique(want)) > base
    tv, tv2a = _transposed(view, v2a)
    other = rr.rule_actions(tv, feat, tv2a, base, n_action, move, rc.EPS, rc.SEED, 1000, 0)[0]
    differ = float((other != want).mean())
    print("%s: the transposed view changes %.1f %% of the rows" % (shape, 100 * differ))
    assert differ >= 0.10, differ


@pytest.mark.parametrize("name", sorted(rc.HAND_MADE))
def test_hand_made_tables_reach_the_ranges_ends(name):
    """(4, 64) with 64 moves and (16, 16) with 57 actions: more than attack_base / 2 distinct actions occur, the rule
    itself (not the random draw) chooses a move of more than 2 cells on at least one row, the draw reaches the last
    action, and the tables are what mfx_rule_create accepts (a host call)."""
    from mfrl_amd.policy import RuleHIP
    shape, F, tab, (view, feat) = rc.hand_made(name)
    v2a, base, n_action, move = tab
    assert feat.shape[1] == F and view.shape[1:3] == shape
    RuleHIP(shape + (7,), (F,), n_action, base, v2a, move)
    want, tag, refused = rc.restated(name, view, feat, tab)
    ruled = want[(tag != rr.TAG_RANDOM) & (want < base)]
    far = np.abs(move[ruled]).max(axis=1) > 2
    print("%s: %d distinct actions of %d, %d rule moves past 2 cells, refused %d" % (name, len(np.unique(want)), n_action,
                                                                                   int(far.sum()), int(refused.sum())))
    assert len(np.unique(want)) > base / 2
    assert far.any()
    assert want.max() == n_action - 1 and (want[tag == rr.TAG_RANDOM] == n_action - 1).any()
    cy, cx = shape[0] // 2, shape[1] // 2
    inside = (0 <= cy + move[:, 1]) & (cy + move[:, 1] < shape[0]) & (0 <= cx + move[:, 0]) & (cx + move[:, 0] < shape[1])
    if name == "strip":
        assert base == n_action == 64 and (v2a < 0).all() and F == 2 and inside.all()
        have = {tuple(m) for m in move.tolist()}
        assert {(0, 0), (16, 0), (-16, 0), (8, 1), (8, -1), (-8, 1), (-8, -1)} <= have
    else:
        assert (base, n_action) == (49, 57) and (v2a >= 0).sum() == 8
