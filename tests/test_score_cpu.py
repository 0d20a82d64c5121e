"""The scorekeeper's contract off the GPU: tests/score_ref.py's win rule is tools.Runner.run's, its guards and its
log cap behave as include/magent_amd.h part 7 states, battle_eval refuses conflicting arguments, and the scripted cases
of tests/score_cases.py hold what the GPU tests need -- asserted here on the C oracle alone."""
import numpy as np
import pytest

import score_cases as sc
import score_ref as sr


# ------------------------------------------------------------------------------------------------- the win rule
PAIRS = [   # (max_nums, nums): main win, opponent win, tie, and unequal armies (kills may be negative: the rule as is)
    ([64, 64], [60, 50]), ([64, 64], [50, 60]), ([64, 64], [57, 57]), ([64, 64], [64, 64]), ([64, 64], [0, 0]),
    ([2, 18], [1, 18]), ([18, 2], [18, 0]), ([2, 18], [2, 2]), ([10, 6], [8, 4]), ([6, 10], [5, 1]),
]


def test_win_rule_is_runner_run():
    from mfrl_amd.algo import tools
    seen = set()
    for max_nums, nums in PAIRS:
        def play_handle(**kw):
            return list(max_nums), list(nums), [0.0, 0.0], [0.0, 0.0]
        runner = tools.Runner(None, None, [0, 1], 40, 400, [None, None], play_handle, render_every=0, train=False)
        win_cnt = {"main": 0, "opponent": 0}
        info = runner.run(0.0, 0, win_cnt=win_cnt)
        win, kill = sr.winner(max_nums, nums)
        assert kill == [info["main"]["kill"], info["opponent"]["kill"]]
        want = {sr.MAIN: {"main": 1, "opponent": 0}, sr.OPPONENT: {"main": 0, "opponent": 1},
                sr.TIE: {"main": 1, "opponent": 1}}[win]
        assert win_cnt == want, (max_nums, nums)
        seen.add(win)
    assert seen == {sr.MAIN, sr.OPPONENT, sr.TIE}
    assert any(a != b for (a, b), _ in PAIRS)


# ------------------------------------------------------------------------------------------------- guards and cap
def _src(E=2, rowcap=8, n=(5, 6)):
    alive = np.ones((E, 2, rowcap), np.uint8)
    return {"group_num": np.tile(np.array(n, np.int32), (E, 1)), "alive": alive,
            "stats": np.zeros((E, 4), np.float64), "agent_steps": np.zeros(E, np.int64)}


def _step(src, e, end=False, new=None, ret=(0.5, 0.25), jump=1):
    """Env e steps: agent_steps moves by its group sizes; at an end the episode count and the return sums move."""
    src["agent_steps"][e] += int(src["group_num"][e].sum())
    if new is not None:
        src["group_num"][e] = new
    if end:
        src["stats"][e, 0] += jump
        src["stats"][e, 1:3] += ret


def test_ref_scores_an_episode():
    src = _src()
    b = sr.new_board(2, 2)
    sr.attach(b, src)
    src["alive"][0, 0, 1] = 0
    src["alive"][0, 0, 6] = 0                      # at and past n_cur: never counted
    _step(src, 0, new=(4, 6))
    _step(src, 1)
    sr.update(b, src)
    assert b["totals"].sum() == 0 and list(b["carry"][0, :4]) == [4, 6, 5, 6] and b["carry"][0, sr.LEN] == 1
    src["alive"][:] = 1
    src["alive"][0, 1, :2] = 0
    _step(src, 0, end=True, new=(5, 6))
    _step(src, 1)
    sr.update(b, src)
    r = b["log"][0, 0]
    assert r["len"] == 2 and list(r["nums"]) == [4, 6] and list(r["surv"]) == [4, 4]
    assert list(r["kill"]) == [5 - 6, 6 - 4] and r["winner"] == sr.OPPONENT and list(r["ret"]) == [0.5, 0.25]
    assert list(b["totals"][0]) == [1, 0, 1, 0, -1, 2, 2, 0] and b["totals"][1].sum() == 0
    assert list(b["state"]) == [1, 0]
    assert list(b["carry"][0]) == [5, 6, 5, 6, 1, 21, 0, 0]


def test_ref_step_guard():
    src = _src()
    b = sr.new_board(2, 2)
    sr.attach(b, src)
    _step(src, 0)
    _step(src, 0, end=True)                        # env 0 stepped twice for one update: the first was not scored
    _step(src, 1, end=True)
    sr.update(b, src)
    assert b["state"][1] == sr.ERR_STEP
    assert b["totals"][0].sum() == 0 and b["totals"][1, sr.EPISODES] == 1
    # the failed env was taken afresh: it is scored again from here on, the word stays
    assert b["carry"][0, sr.EP] == 1 and b["carry"][0, sr.STEPS0] == 22
    _step(src, 0, end=True)
    _step(src, 1)
    word = int(b["state"][1])
    sr.update(b, src)
    assert b["totals"][0, sr.EPISODES] == 1 and b["state"][1] == word
    # an update without a step is a step scored twice
    sr.update(b, src)
    assert b["state"][1] & sr.ERR_STEP and b["totals"][0, sr.EPISODES] == 1


def test_ref_episode_jump():
    src = _src()
    b = sr.new_board(2, 2)
    sr.attach(b, src)
    _step(src, 0, end=True, jump=2)
    _step(src, 1, end=True)
    sr.update(b, src)
    assert b["state"][1] == sr.ERR_EPISODE
    assert b["totals"][0].sum() == 0 and b["totals"][1, sr.EPISODES] == 1 and b["carry"][0, sr.EP] == 2


def test_ref_log_cap_and_target():
    src = _src(E=1)
    b = sr.new_board(1, 1)
    sr.attach(b, src, target=2)
    for k in range(3):
        _step(src, 0, end=True)
        sr.update(b, src)
        assert b["state"][0] == (1 if k >= 1 else 0)
    assert list(b["totals"][0, [sr.EPISODES, sr.DROPPED, sr.STEPS]]) == [3, 2, 3] and b["state"][1] == 0
    assert b["log"][0, 0]["len"] == 1


def test_ref_count_out_of_range():
    src = _src()
    src["group_num"][1, 0] = 9
    b = sr.new_board(2, 1)
    sr.attach(b, src)
    assert b["state"][1] == sr.ERR_COUNT
    _step(src, 0)
    _step(src, 1)
    sr.update(b, src)
    assert b["state"][1] == sr.ERR_COUNT and b["carry"][1, sr.LEN] == 0 and b["carry"][0, sr.LEN] == 1


# ------------------------------------------------------------------------------------------------- the CLI
@pytest.mark.parametrize("argv,msg", [
    (["--algo", "mfq", "--oppo", "mfac", "--untrained", "--envs", "2", "--render"], "--render"),
    (["--algo", "mfq", "--idx", "1"], "--idx"),
    (["--algo", "mfq"], "--idx"),
    (["--algo", "mfq", "--untrained", "--idx", "1", "2"], "--untrained"),
    (["--algo", "mfq", "--untrained", "--act_precision", "bf16"], "--act_precision"),
    (["--algo", "mfq", "--untrained", "--envs", "0"], "--envs"),
    (["--algo", "mfq", "--untrained", "--n_round", "0"], "--n_round"),
    (["--algo", "ppo", "--untrained"], "--algo"),
])
def test_battle_eval_refuses(argv, msg, capsys):
    from mfrl_amd import battle_eval
    with pytest.raises(SystemExit) as ex:
        battle_eval.main(argv)
    assert ex.value.code == 2
    assert msg in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------- the cases
def test_cases_hold_what_the_gpu_tests_need():
    eps = [(name, e, ep) for name in sc.PLANS for e, lst in enumerate(sc.oracle_run(name)["episodes"]) for ep in lst]
    winners = {ep["winner"] for _, _, ep in eps}
    assert winners == {sr.MAIN, sr.OPPONENT, sr.TIE}
    assert any(ep["done"] and ep["len"] < sc.MAX_STEPS for _, _, ep in eps)
    assert any(ep["nums"] != ep["surv"] for _, _, ep in eps)
    for name in sc.PLANS:
        run = sc.oracle_run(name)
        assert all(len(lst) >= 2 for lst in run["episodes"]), name          # every env restarts twice in 25 steps
        assert run["rowcap"] == sc.rowcap_of(run["placement"])
        n_min = min(n for row in run["steps"] for st in row for n in st["n"])
        assert n_min < run["rowcap"], name                                  # stale bytes past n_cur exist
    packed = sc.oracle_run("packed")
    assert any(ep["done"] for lst in packed["episodes"] for ep in lst)
    assert len(packed["placement"][0]) != len(packed["placement"][1])
