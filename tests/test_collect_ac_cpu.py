"""The episode-chain path of the rollout collector (AC / MFAC), host side, without a GPU: the numpy restatements of
the link columns and of the chain returns, the link columns of _StepRows, the collector's reservation over an
EpisodesBuffer, the new C entry points, and train_battle's refusals around --rollout_episodes."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import common

sys.path.insert(0, os.path.join(common.REPO, "oracle"))
import mf_oracle  # noqa: E402

ENTRY = ("mfx_collect_end_linked", "mfx_collect_links_reset", "mfx_chain_returns")


def test_entry_points_declared_and_exported():
    header = open(os.path.join(common.REPO, "include", "magent_amd.h")).read()
    dll = ctypes.CDLL(common.HIP_LIB)
    for fn in ENTRY:
        assert re.search(r"\bint %s\(" % fn, header), fn
        assert hasattr(dll, fn), fn
    # the unlinked end keeps its signature
    assert re.search(r"int mfx_collect_end\(const mfx_collect_src \*src, const mfx_collect_dst \*dst, "
                     r"const int32_t \*d_rows,\s+const int32_t \*d_total, int64_t \*d_state, int64_t id_stride, "
                     r"void \*stream\);", header)


def test_chain_links_on_a_hand_written_sequence():
    """Keys A = 7 and B = 9 interleaved over three steps (B dies after two), key C = 4 with one row, then the id of
    A again in a later episode (another key, 107) for two steps."""
    from mfrl_amd.replay import chain_links
    #        row: 0  1  2  3  4  5  6    7    8
    keys = [7, 9, 7, 9, 4, 7, 107, 107, 9 + 100]
    prev, tail = chain_links(keys)
    assert prev.dtype == np.int64 and tail.dtype == bool
    assert prev.tolist() == [-1, -1, 0, 1, -1, 2, -1, 6, -1]
    assert tail.tolist() == [False, False, False, True, True, True, False, True, True]
    p0, t0 = chain_links(np.zeros(0, np.int64))
    assert len(p0) == 0 and len(t0) == 0


def _forest(rng, lens):
    """Interleaved chains of the given lengths over sum(lens) rows: prev, tails (in chain order), the rows of every
    chain in step order."""
    owner = np.repeat(np.arange(len(lens)), lens)
    rng.shuffle(owner)
    prev = np.full(len(owner), -1, np.int64)
    rows = [np.nonzero(owner == c)[0] for c in range(len(lens))]
    for r in rows:
        prev[r[1:]] = r[:-1]
    return prev, np.array([r[-1] for r in rows], np.int64), rows


@pytest.mark.parametrize("numpy1", [True, False])
def test_chain_returns_host_equals_the_oracle_per_chain(numpy1):
    from mfrl_amd.replay import chain_returns_host
    rng = np.random.default_rng(5)
    lens = np.concatenate([rng.integers(1, 30, size=40), [1, 1, 200]])
    prev, tails, rows = _forest(rng, lens)
    rew = rng.standard_normal(len(prev)).astype(np.float32)
    val = rng.standard_normal(len(tails)).astype(np.float32)
    keep = rew.copy()
    got = chain_returns_host(rew, prev, tails, val, 0.95, numpy1)
    assert got.dtype == np.float32 and rew.tobytes() == keep.tobytes()          # a new array
    for r, v in zip(rows, val):
        assert got[r].tobytes() == mf_oracle.mfac_returns(rew[r], v, 0.95, numpy1=numpy1).tobytes()
    other = chain_returns_host(rew, prev, tails, val, 0.95, not numpy1)
    assert (other != got).any()                                                 # the two modes are two results


def test_step_rows_columns():
    import torch
    from mfrl_amd.algo.tools import _StepRows
    base = ["ids", "obs", "feat", "act", "rew", "term"]
    for use_mean in (False, True):
        want = base + (["prob"] if use_mean else [])
        r = _StepRows((3, 3, 2), (5,), 4, use_mean, device="cpu")
        r._ensure(1)
        assert list(r.cols) == want and not r.links
        r = _StepRows((3, 3, 2), (5,), 4, use_mean, device="cpu", links=True)
        r._ensure(1)
        assert list(r.cols) == want + ["prev", "tail"] and r.links
        assert r.cols["prev"].dtype == torch.int64 and r.cols["tail"].dtype == torch.bool
        assert r.cols["prev"].shape == r.cols["tail"].shape == (1024,)
        # a grow carries marked values in the link columns like the rest
        r.cols["prev"][:700] = torch.arange(700) - 1
        r.cols["tail"][:700] = torch.arange(700) % 3 == 0
        r.cols["act"][:700] = torch.arange(700, dtype=torch.int32)
        r._ensure(3000, live=700)
        assert r.cap == 3000
        assert torch.equal(r.cols["prev"][:700], torch.arange(700) - 1)
        assert torch.equal(r.cols["tail"][:700], torch.arange(700) % 3 == 0)
        assert torch.equal(r.cols["act"][:700], torch.arange(700, dtype=torch.int32))


def test_episodes_buffer_prepare_and_clear():
    from mfrl_amd.algo.tools import EpisodesBuffer
    buf = EpisodesBuffer(use_mean=True, device="cpu")
    assert buf._rows is None
    rows = buf.prepare((13, 13, 7), (34,), 21)
    assert rows is buf._rows and rows.links and rows.use_mean and rows.act_n == 21 and rows.n == 0
    assert rows.obs_shape == (13, 13, 7) and rows.feat_shape == (34,)
    assert buf.prepare((13, 13, 7), (34,), 21) is rows               # kept
    rows._ensure(10)
    store = rows.cols["obs"]
    rows.n = 7
    buf.clear()
    assert buf._rows is rows and rows.n == 0 and rows.cols["obs"] is store
    assert buf.batch() is None


class _Eng:
    n_envs, rowcap, handles = 3, 8, (0, 1)


def test_reservation_over_an_episodes_buffer():
    """_reserve / bound / capacity of a collector over a device="cpu" EpisodesBuffer, as over a MemoryGroup; the
    link columns are carried by every grow."""
    import torch
    from mfrl_amd.algo.tools import EpisodesBuffer
    from mfrl_amd.replay import RolloutCollector
    buf = EpisodesBuffer(use_mean=False, device="cpu")
    with pytest.raises(ValueError, match="prepare"):
        RolloutCollector(_Eng(), buf, 0)
    rows = buf.prepare((13, 13, 7), (34,), 1)
    col = RolloutCollector(_Eng(), buf, 0)
    assert col.linked and "prob" not in rows.cols
    assert col.step_rows() == 24 and col.id_stride() == 16
    assert col.finish() == 0
    caps, bound = [], 0
    for k in range(100):
        cap = col._reserve()
        bound += 24
        assert col._bound == bound and cap == rows.cap >= bound
        if not caps or cap != caps[-1]:
            caps.append(cap)
        rows.cols["prev"][bound - 24:bound] = k                       # what the kernels would write
        rows.cols["tail"][bound - 24:bound] = bool(k & 1)
    assert caps[0] == 1024 and all(b >= 2 * a for a, b in zip(caps, caps[1:])) and len(caps) == 3
    assert torch.equal(rows.cols["prev"][:bound], torch.arange(100).repeat_interleave(24))
    assert torch.equal(rows.cols["tail"][:bound], (torch.arange(100) % 2 == 1).repeat_interleave(24))
    assert rows.n == 0
    col.discard()
    capped = RolloutCollector(_Eng(), buf, 0, capacity=30)
    assert capped._reserve() == 30 and capped._bound == 24
    assert capped._reserve() == 30 and capped._bound <= rows.cap
    # an unlinked owner still takes the unlinked path
    from mfrl_amd.algo.tools import MemoryGroup
    mg = MemoryGroup((13, 13, 7), (34,), 21, 64, 16, 8, use_mean=True, device="cpu")
    assert not RolloutCollector(_Eng(), mg, 0).linked


@pytest.mark.parametrize("argv, words", [
    (["--algo", "mfq", "--envs", "4", "--rollout_episodes"], ("--rollout_episodes", "ac or mfac")),
    (["--algo", "il", "--envs", "4", "--rollout_episodes"], ("--rollout_episodes", "ac or mfac")),
    (["--algo", "mfac", "--envs", "1", "--rollout_episodes"], ("--rollout_episodes", "--envs > 1")),
    (["--algo", "mfac", "--rollout_episodes"], ("--rollout_episodes", "--envs > 1")),
    (["--algo", "mfac", "--envs", "4", "--rollout_episodes", "--rollout"], ("--rollout_episodes and --rollout",)),
    (["--algo", "ac", "--envs", "4", "--rollout_episodes", "--train_backend", "hip"],
     ("--rollout_episodes", "--train_backend hip")),
    (["--algo", "ac", "--envs", "4", "--rollout"], ("--rollout collects", "--rollout_episodes")),
])
def test_train_battle_refusals(argv, words, capsys):
    from mfrl_amd import train_battle
    with pytest.raises(SystemExit) as ex:
        train_battle.main(argv)
    assert ex.value.code == 2
    err = capsys.readouterr().err
    assert "unrecognized arguments" not in err
    for w in words:
        assert w in err, (w, err)
