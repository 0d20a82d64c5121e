"""The scorekeeper kernels (mfx_score_attach / mfx_score_update, csrc/score_kernels.hip) on synthetic device buffers,
without an engine: torch tensors stand in for the rollout buffers, the kernels are called through the ctypes structs of
mfrl_amd.scoreboard, and after every call all five destination buffers -- a sentinel row at each end included -- are
compared byte for byte with tests/score_ref.py.

Shapes: rowcap 4 (a single dword), 12, 260 (a second pass of the wave, with a tail); envs 1, 5 (a partial workgroup),
1030 (hundreds of workgroups), and one more than the launch's grid holds (8 workgroups per CU, four envs each), where
waves take a second env in the grid-stride loop -- after a scored env and after one that failed its guard; group sizes
0, 1, 3, rowcap - 1, rowcap (the mask inside a dword), with every byte at and past the group size set to 1, so a
kernel that counts them cannot pass, and the live flags drawn from 0, 1, 2, 0x80, 0xff, so one that tests a single bit
cannot either.  The script: an episode end at the first step, two consecutive ends, a skipped update, a +2 episode jump, a log
overflow at ep_cap = 1, the target counter."""
import ctypes

import numpy as np
import pytest

import score_ref as sr

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p
SENT = 0xA5
NAMES = ("carry", "ret0", "totals", "log", "state")
ALIVE = np.array([0, 0, 0, 1, 2, 0x80, 0xFF], np.uint8)      # the contract counts non-zero bytes, whatever their bits


def _sizes(E, ep_cap):
    return {"carry": E * sr.CARRY * 8, "ret0": E * 16, "totals": E * sr.TOTALS * 8, "log": E * ep_cap * 48, "state": 16}


class Device:
    """The five destination buffers on the device, one sentinel row (an env's share; for state one word) before and
    after what the kernels are given."""

    def __init__(self, E, ep_cap, target):
        import torch
        from mfrl_amd.scoreboard import score_lib
        self.E, self.ep_cap, self.target = E, ep_cap, target
        self.L = score_lib()
        self.pad = {k: (8 if k == "state" else n // E) for k, n in _sizes(E, ep_cap).items()}
        self.bufs = {k: torch.full((n + 2 * self.pad[k],), SENT, dtype=torch.uint8, device="cuda")
                     for k, n in _sizes(E, ep_cap).items()}
        got = (ctypes.c_size_t * 5)()
        assert self.L.mfx_score_sizes(E, ctypes.c_int64(ep_cap), got) == 0
        assert list(got) == [_sizes(E, ep_cap)[k] for k in NAMES]
        self.st = P(torch.cuda.current_stream().cuda_stream)
        self.keep = None

    def structs(self, src, rowcap, n_groups=2):
        import torch
        from mfrl_amd.scoreboard import _ScoreDst, _ScoreSrc
        self.keep = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in src.items()}
        s = _ScoreSrc(*[self.keep[k].data_ptr() for k in ("group_num", "alive", "stats", "agent_steps")], self.E,
                      n_groups, rowcap)
        d = _ScoreDst(*[self.bufs[k].data_ptr() + self.pad[k] for k in NAMES], self.ep_cap, self.target)
        return s, d

    def call(self, fn, src, rowcap, **kw):
        s, d = self.structs(src, rowcap, **kw)
        return getattr(self.L, fn)(ctypes.byref(s), ctypes.byref(d), self.st)

    def check(self, board, tag):
        import torch
        torch.cuda.synchronize()
        for k in NAMES:
            got = self.bufs[k].cpu().numpy()
            want = np.concatenate([np.full(self.pad[k], SENT, np.uint8), np.ascontiguousarray(board[k]).view(np.uint8)
                                   .reshape(-1), np.full(self.pad[k], SENT, np.uint8)])
            assert got.shape == want.shape, (tag, k)
            bad = np.nonzero(got != want)[0]
            assert len(bad) == 0, (tag, k, "first differing bytes", bad[:8] - self.pad[k], len(bad))


def _sizes_cycle(rowcap):
    return [0, 1, 3, rowcap - 1, rowcap]


def _advance(src, rng, e, new, end=0, rowcap=4):
    """Env e steps once: the alive rows hold random flags below the group sizes the step ran with and 1 from there
    on; agent_steps moves by those sizes; then the group sizes become `new`."""
    for g in range(2):
        n = int(src["group_num"][e, g])
        src["alive"][e, g, :n] = rng.choice(ALIVE, size=n)
        src["alive"][e, g, n:] = 1
    src["agent_steps"][e] += int(src["group_num"][e].sum())
    src["group_num"][e] = new
    if end:
        src["stats"][e, 0] += end
        src["stats"][e, 1:3] += rng.random(2) * 8 - 4
    src["stats"][e, 3] += 1.0


def _script(E, rowcap, ep_cap, target, seed=0, steps=7):
    rng = np.random.default_rng(seed)
    cyc = _sizes_cycle(rowcap)
    pick = lambda t, e, g: cyc[(t + e + 2 * g) % 5]
    src = {"group_num": np.array([[pick(0, e, g) for g in range(2)] for e in range(E)], np.int32),
           "alive": np.ones((E, 2, rowcap), np.uint8), "stats": np.zeros((E, 4), np.float64),
           "agent_steps": rng.integers(0, 1 << 40, size=E).astype(np.int64)}
    src["stats"][:, 0] = rng.integers(0, 5, size=E)
    src["stats"][:, 1:3] = rng.random((E, 2))
    dev, board = Device(E, ep_cap, target), sr.new_board(E, ep_cap)
    assert dev.call("mfx_score_attach", src, rowcap) == 0
    sr.attach(board, src, target)
    dev.check(board, "attach")
    skipped, jumped = 1 % E, 2 % E
    want_err = 0
    for t in range(1, steps + 1):
        for e in range(E):
            new = [pick(t, e, g) for g in range(2)]
            end = {1: e % 3 == 0, 2: e % 3 != 2, 4: e % 2 == 0, 6: True, 7: e % 3 == 2}.get(t, False)
            if t == 3 and e == skipped:                  # stepped twice for one update
                _advance(src, rng, e, new, 0, rowcap)
                want_err |= sr.ERR_STEP
            if t == 5 and e == jumped:
                end = 2
                want_err |= sr.ERR_EPISODE
            _advance(src, rng, e, new, int(end), rowcap)
        before = board["totals"].copy()
        assert dev.call("mfx_score_update", src, rowcap) == 0, dev.L.mfx_last_error().decode()
        sr.update(board, src)
        dev.check(board, ("update", t))
        assert int(board["state"][1]) == want_err, t
        if t == 3:                                       # totals unchanged for the skipped env only
            assert np.array_equal(board["totals"][skipped], before[skipped])
        if t == 5:
            assert np.array_equal(board["totals"][jumped], before[jumped])
    return board


@pytest.mark.parametrize("E", [1, 5, 1030])
@pytest.mark.parametrize("rowcap", [4, 12, 260])
def test_score_shapes(rowcap, E):
    ep_cap, target = (1, 1) if E == 5 else (2, 2)
    board = _script(E, rowcap, ep_cap, target, seed=rowcap + E)
    t = board["totals"]
    # the script's own conditions, on the reference alone
    assert t[0, sr.EPISODES] >= 3                        # env 0: ends at the first step and at the next
    assert board["log"][0, 0]["len"] == 1 and (ep_cap < 2 or board["log"][0, 1]["len"] == 1)
    assert t[:, sr.DROPPED].sum() > 0 and (t[:, sr.EPISODES] - t[:, sr.DROPPED] <= ep_cap).all()
    assert 0 < board["state"][0] <= E and board["state"][0] == (t[:, sr.EPISODES] >= target).sum()
    if E > 1:
        seen = set(board["log"]["nums"].reshape(-1).tolist())
        assert {0, 1, 3, rowcap - 1, rowcap} <= seen | set(board["carry"][:, :2].reshape(-1).tolist())
        assert (board["log"]["surv"] < board["log"]["nums"]).any()


def test_grid_stride():
    """More envs than the launch's grid holds waves (mfx_score_update: at most 8 workgroups per CU, four envs each):
    every wave of the first workgroups takes a second env.  Env 1 fails the step guard at step 3 and env 2 the episode
    check at step 5, both in the first stride, so their waves go on to a second env through the not-scored branch."""
    import torch
    grid_envs = 4 * 8 * torch.cuda.get_device_properties(0).multi_processor_count
    E, rowcap = grid_envs + 37, 12
    board = _script(E, rowcap, 1, 1, seed=9, steps=5)
    t = board["totals"]
    assert board["state"][1] == sr.ERR_STEP | sr.ERR_EPISODE
    # the second stride was scored: episodes finished and logged there, later ones dropped, lengths carried
    tail = t[grid_envs:]
    assert (tail[:, sr.EPISODES] >= 2).any() and tail[:, sr.DROPPED].sum() > 0
    assert (board["log"][grid_envs:, 0]["len"] >= 1).any() and (board["carry"][grid_envs:, sr.LEN] >= 1).any()
    assert (board["log"][grid_envs:]["surv"] < board["log"][grid_envs:]["nums"]).any()


def test_three_groups_are_refused():
    E, rowcap = 2, 4
    src = {"group_num": np.ones((E, 3), np.int32), "alive": np.ones((E, 3, rowcap), np.uint8),
           "stats": np.zeros((E, 4), np.float64), "agent_steps": np.zeros(E, np.int64)}
    dev, board = Device(E, 1, 1), None
    for fn in ("mfx_score_attach", "mfx_score_update"):
        assert dev.call(fn, src, rowcap, n_groups=3) == -1
        assert "two groups only" in dev.L.mfx_last_error().decode()
    two = {k: (v[:, :2].copy() if k in ("group_num", "alive") else v) for k, v in src.items()}
    assert dev.call("mfx_score_update", two, 6) == -1
    assert "multiple of 4" in dev.L.mfx_last_error().decode()
    import torch
    torch.cuda.synchronize()
    for k in NAMES:                                      # nothing was launched
        assert bool((dev.bufs[k] == SENT).all()), k
    assert board is None
