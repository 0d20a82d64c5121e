"""NumPy restatement of the scorekeeper's contract (include/magent_amd.h part 7, csrc/score_kernels.hip): attach and
update on plain arrays, one env at a time, with no cleverness.  The device buffers have exactly these dtypes and
layouts, so a test compares whole buffers byte for byte.

    src: dict of group_num int32 [E][2], alive uint8 [E][2][rowcap], stats float64 [E][4], agent_steps int64 [E]
    board: dict of carry int64 [E][8], ret0 float64 [E][2], totals int64 [E][8], log RECORD [E][ep_cap], state int64 [2]
"""
import numpy as np

RECORD = np.dtype([("len", np.int32), ("nums", np.int32, 2), ("surv", np.int32, 2), ("kill", np.int32, 2),
                   ("winner", np.int32), ("ret", np.float64, 2)])
assert RECORD.itemsize == 48
N_CUR, START, EP, STEPS0, LEN, CARRY = 0, 2, 4, 5, 6, 8
EPISODES, MAIN_WINS, OPPO_WINS, TIES, KILLS, STEPS, DROPPED, TOTALS = 0, 1, 2, 3, 4, 6, 7, 8
ERR_STEP, ERR_EPISODE, ERR_COUNT = 1, 2, 4
MAIN, OPPONENT, TIE = 0, 1, 2


def winner(max_nums, nums):
    """Runner.run's rule (algo/tools.py, train=False): kill[i] = max_nums[i] - nums[1 - i]; the larger kill wins, equal
    kills count for both.  nums: get_num after the step, before clear_dead."""
    kill = [int(max_nums[0]) - int(nums[1]), int(max_nums[1]) - int(nums[0])]
    return (MAIN if kill[0] > kill[1] else OPPONENT if kill[0] < kill[1] else TIE), kill


def new_board(n_envs, ep_cap):
    return {"carry": np.zeros((n_envs, CARRY), np.int64), "ret0": np.zeros((n_envs, 2), np.float64),
            "totals": np.zeros((n_envs, TOTALS), np.int64), "log": np.zeros((n_envs, ep_cap), RECORD),
            "state": np.zeros(2, np.int64), "ep_cap": int(ep_cap), "target": 1}


def _snapshot(board, src, e):
    c = board["carry"][e]
    c[N_CUR:N_CUR + 2] = src["group_num"][e]
    c[START:START + 2] = src["group_num"][e]
    c[EP] = np.int64(src["stats"][e, 0])
    c[STEPS0] = src["agent_steps"][e]
    c[LEN] = 0
    c[7] = 0
    board["ret0"][e] = src["stats"][e, 1:3]


def _count_ok(n, rowcap):
    return 0 <= n <= rowcap


def attach(board, src, target=1):
    E, rowcap = len(src["group_num"]), src["alive"].shape[2]
    board["target"] = int(target)
    board["state"][:] = 0
    board["totals"][:] = 0
    board["log"][:] = np.zeros((), RECORD)
    for e in range(E):
        _snapshot(board, src, e)
        if not all(_count_ok(int(n), rowcap) for n in src["group_num"][e]):
            board["state"][1] |= ERR_COUNT


def update(board, src):
    E, rowcap = len(src["group_num"]), src["alive"].shape[2]
    for e in range(E):
        c, t = board["carry"][e], board["totals"][e]
        n_cur = [int(c[N_CUR]), int(c[N_CUR + 1])]
        start = [int(c[START]), int(c[START + 1])]
        new = [int(src["group_num"][e, 0]), int(src["group_num"][e, 1])]
        ep_now, steps_now = int(np.int64(src["stats"][e, 0])), int(src["agent_steps"][e])
        err = 0
        if steps_now - int(c[STEPS0]) != n_cur[0] + n_cur[1]:
            err |= ERR_STEP
        if ep_now - int(c[EP]) not in (0, 1):
            err |= ERR_EPISODE
        if not all(_count_ok(n, rowcap) for n in n_cur + new):
            err |= ERR_COUNT
        if err:
            board["state"][1] |= err
            _snapshot(board, src, e)
            continue
        surv = [int(np.count_nonzero(src["alive"][e, g, :n_cur[g]])) for g in range(2)]
        c[LEN] += 1
        if ep_now == int(c[EP]) + 1:
            win, kill = winner(start, n_cur)
            idx = int(t[EPISODES])
            if idx < board["ep_cap"]:
                r = board["log"][e, idx]
                r["len"], r["nums"], r["surv"], r["kill"], r["winner"] = c[LEN], n_cur, surv, kill, win
                r["ret"] = src["stats"][e, 1:3] - board["ret0"][e]
            else:
                t[DROPPED] += 1
            t[EPISODES] += 1
            t[MAIN_WINS + win] += 1
            t[KILLS:KILLS + 2] += kill
            t[STEPS] += c[LEN]
            if int(t[EPISODES]) == board["target"]:
                board["state"][0] += 1
            c[LEN] = 0
            c[EP] += 1
            board["ret0"][e] = src["stats"][e, 1:3]
            c[START:START + 2] = new
        c[N_CUR:N_CUR + 2] = new
        c[STEPS0] = steps_now


def outcome(board):
    """The dict RolloutScoreboard.finish() returns, from a board."""
    t = board["totals"]
    out = {"totals": t.copy(), "log": board["log"].copy(), "reached": int(board["state"][0]),
           "error": int(board["state"][1])}
    for k, i in (("episodes", EPISODES), ("main_wins", MAIN_WINS), ("oppo_wins", OPPO_WINS), ("ties", TIES),
                 ("steps", STEPS), ("dropped", DROPPED)):
        out[k] = int(t[:, i].sum())
    out["kills"] = [int(t[:, KILLS].sum()), int(t[:, KILLS + 1].sum())]
    return out
