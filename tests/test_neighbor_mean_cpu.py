"""The neighbourhood mean action without a GPU: the facts about the engine's buffers that the rollout form of the
kernel relies on, checked on the C oracle; the limits of the definition on the numpy restatement; the refusals of the
model layer, the host loops and the command lines."""
import numpy as np
import pytest

import common
import neighbor_mean_ref as nr

MAP, SIDE, STEPS = 40, 8, 30


def _oracle_run():
    """30 steps of the C oracle on the 40 x 40 map from the checkerboard block under RandomState(7) actions (60 %
    attacks): per step and group what the rollout buffers would hold (actions / ids / alive in the order of before
    clear_dead, the group's size before the step, the new feature rows) and the engine's own answers (get_agent_id
    and get_pos after clear_dead)."""
    env, h = common.battle_env(common.ORACLE_LIB, MAP)
    env.reset()
    for g, pos in enumerate(nr.checkerboard(MAP, MAP, SIDE)):
        env.add_agents(h[g], method="custom", pos=pos)
    n_action = env.get_action_space(h[0])[0]
    attack_base, _ = env.get_view2attack(h[0])
    rng = np.random.RandomState(7)
    steps = []
    for t in range(STEPS):
        ids = [env.get_agent_id(h[g]).copy() for g in range(2)]
        acts = [nr.draw_actions(rng, len(ids[g]), n_action, attack_base) for g in range(2)]
        for g in range(2):
            env.set_action(h[g], acts[g])
        done = env.step()
        alive = [env.get_alive(h[g]).copy() for g in range(2)]
        env.clear_dead()
        rec = []
        for g in range(2):
            rec.append({"ids": ids[g], "acts": acts[g], "alive": alive[g], "prev_num": len(ids[g]),
                        "ids_after": env.get_agent_id(h[g]).copy(), "pos_after": env.get_pos(h[g]).copy(),
                        "feat": env.get_observation(h[g])[1].copy()})
        steps.append(rec)
        assert not done, "the episode ended at step %d: the run is meant to last" % t
    return steps, n_action


@pytest.fixture(scope="module")
def oracle_run():
    return _oracle_run()


def _by_id(rec, n_action, radius):
    """The definition keyed by agent id, from the engine's own answers: the action of id i is the one it was given,
    its position what get_pos reports after clear_dead."""
    act_of = dict(zip(rec["ids"].tolist(), rec["acts"].tolist()))
    pos_of = dict(zip(rec["ids_after"].tolist(), rec["pos_after"].tolist()))
    out = np.zeros((len(rec["ids_after"]), n_action), dtype=np.float32)
    for j, i in enumerate(rec["ids_after"].tolist()):
        near = [k for k in pos_of if max(abs(pos_of[k][0] - pos_of[i][0]), abs(pos_of[k][1] - pos_of[i][1])) <= radius]
        cnt = np.bincount([act_of[k] for k in near], minlength=n_action)
        out[j] = (cnt / np.float64(len(near))).astype(np.float32)
    return out


def test_rollout_buffers_give_the_definition(oracle_run):
    """At every step: the survivors' ids in the order of before clear_dead are the next get_agent_id; rint(feature *
    map) is get_pos; the restatement fed the buffer-shaped inputs equals the computation keyed by agent id.  The run
    has deaths in many steps (a condition, not a measurement: the oracle alone fixes them)."""
    steps, n_action = oracle_run
    deaths, steps_with_death, moved = 0, 0, 0
    for t, rec2 in enumerate(steps):
        died = 0
        for g, rec in enumerate(rec2):
            live = rec["alive"] != 0
            assert np.array_equal(rec["ids"][live], rec["ids_after"]), (t, g, "survivor order")
            pos = nr.positions(rec["feat"], MAP, MAP)
            assert np.array_equal(pos, rec["pos_after"]), (t, g, "position decode")
            for radius in (1, 6):
                got = nr.rollout(rec["acts"], rec["alive"], rec["prev_num"], pos, n_action, radius, False)
                assert got.tobytes() == _by_id(rec, n_action, radius).tobytes(), (t, g, radius)
            died += int((~live).sum())
            moved += int((~live)[:-1].any())
        deaths += died
        steps_with_death += died > 0
    assert deaths >= 10 and steps_with_death >= 5 and moved >= 1, (deaths, steps_with_death, moved)


def test_radius_zero_is_the_own_action(oracle_run):
    steps, n_action = oracle_run
    for t, rec2 in enumerate(steps):
        for g, rec in enumerate(rec2):
            pos = nr.positions(rec["feat"], MAP, MAP)
            got = nr.rollout(rec["acts"], rec["alive"], rec["prev_num"], pos, n_action, 0, False)
            want = np.eye(n_action, dtype=np.float32)[rec["acts"][rec["alive"] != 0]]
            assert got.tobytes() == want.tobytes(), (t, g)


def test_radius_past_the_map_is_the_group_mean(oracle_run):
    """On the steps without a death, R >= map gives every row bincount / n, the reference's group mean cast to float."""
    steps, n_action = oracle_run
    checked = 0
    for t, rec2 in enumerate(steps):
        for g, rec in enumerate(rec2):
            if not (rec["alive"] != 0).all():
                continue
            pos = nr.positions(rec["feat"], MAP, MAP)
            got = nr.rollout(rec["acts"], rec["alive"], rec["prev_num"], pos, n_action, MAP, False)
            want = (np.bincount(rec["acts"], minlength=n_action) / np.float64(len(rec["acts"]))).astype(np.float32)
            assert got.tobytes() == np.tile(want, (len(pos), 1)).tobytes(), (t, g)
            checked += 1
    assert checked >= 5


def test_out_of_range_actions_and_restart():
    pos = [[0, 0], [1, 1], [5, 5]]
    got = nr.compact(pos, [2, -1, 7], 4, 1)
    assert got.tolist() == [[0, 0, 0.5, 0], [0, 0, 0.5, 0], [0, 0, 0, 0]]       # (the divisor stays: 2, 2, 1)
    got = nr.rollout([1, 2, 3], [1, 0, 1], 3, [[0, 0], [9, 9]], 4, 1, False)
    assert got.tolist() == [[0, 1, 0, 0], [0, 0, 0, 1]]                         # (the dead row's action is nobody's)
    assert not nr.rollout([1, 2, 3], [1, 0, 1], 3, [[0, 0], [9, 9]], 4, 1, True).any()


# ------------------------------------------------------------------------------------------------- the surface
def test_mean_field_setter_validates():
    from mfrl_amd.algo.ac import MFAC, ActorCritic
    from mfrl_amd.algo.base import ValueNet
    for cls, flag in ((ValueNet, "use_mf"), (MFAC, None)):
        m = cls.__new__(cls)
        if flag:
            setattr(m, flag, True)
        assert m.mean_field == "group" and m.mf_radius == 6
        m.mean_field = "neighbors"
        m.mf_radius = 0
        assert m.mean_field == "neighbors" and m.mf_radius == 0 and cls._mean_field == "group" and cls._mf_radius == 6
        for bad in ("neighbours", "", None, 1):
            with pytest.raises(ValueError):
                m.mean_field = bad
        for bad in (-1, 1.5, "6", True):
            with pytest.raises((ValueError, TypeError)):
                m.mf_radius = bad
        assert m.mean_field == "neighbors" and m.mf_radius == 0
        m.mean_field = "group"
    dqn = ValueNet.__new__(ValueNet)
    dqn.use_mf = False
    for m in (dqn, ActorCritic.__new__(ActorCritic)):
        m.mean_field = "group"
        with pytest.raises(ValueError, match="mean-field model"):
            m.mean_field = "neighbors"
        assert m.mean_field == "group"


@pytest.mark.parametrize("loop", ["play", "play_batched"])
def test_host_loops_refuse_a_neighbors_model(loop):
    from mfrl_amd.algo import play as pl
    from mfrl_amd.algo.base import ValueNet
    m = ValueNet.__new__(ValueNet)
    m.use_mf = True
    m.mean_field = "neighbors"
    other = ValueNet.__new__(ValueNet)
    with pytest.raises(ValueError, match="device rollout loops"):
        if loop == "play":
            pl.play(None, 0, 40, 10, [None, None], [other, m], 50)
        else:
            pl.play_batched(None, 0, 40, 10, [m, other])


@pytest.mark.parametrize("argv,msg", [
    (["--algo", "mfq", "--mean_field", "neighbors"], "--mean_field"),
    (["--algo", "mfq", "--envs", "4", "--mean_field", "neighbors"], "--mean_field"),
    (["--algo", "mfac", "--envs", "4", "--mean_field", "neighbors"], "--mean_field"),
    (["--algo", "ac", "--envs", "4", "--rollout_episodes", "--mean_field", "neighbors"], "--mean_field"),
    (["--algo", "il", "--envs", "4", "--rollout", "--mean_field", "neighbors"], "--mean_field"),
    (["--algo", "mfq", "--envs", "4", "--rollout", "--mean_field", "nearby"], "--mean_field"),
    (["--algo", "mfq", "--envs", "4", "--rollout", "--mf_radius", "3"], "--mf_radius"),
    (["--algo", "mfq", "--envs", "4", "--rollout", "--mean_field", "neighbors", "--mf_radius", "-1"], "--mf_radius"),
])
def test_train_battle_refuses(argv, msg, capsys):
    from mfrl_amd import train_battle
    with pytest.raises(SystemExit) as ex:
        train_battle.main(argv)
    assert ex.value.code == 2
    assert msg in capsys.readouterr().err


@pytest.mark.parametrize("argv,msg", [
    (["--algo", "mfq", "--untrained", "--mean_field", "neighbors"], "--mean_field"),
    (["--algo", "ac", "--oppo", "il", "--untrained", "--envs", "4", "--mean_field", "neighbors"], "--mean_field"),
    (["--algo", "mfq", "--untrained", "--envs", "4", "--mf_radius", "3"], "--mf_radius"),
    (["--algo", "mfq", "--untrained", "--envs", "4", "--mean_field", "neighbors", "--mf_radius", "-2"], "--mf_radius"),
])
def test_battle_eval_refuses(argv, msg, capsys):
    from mfrl_amd import battle_eval
    with pytest.raises(SystemExit) as ex:
        battle_eval.main(argv)
    assert ex.value.code == 2
    assert msg in capsys.readouterr().err
