"""The rollout collector's host side, without a GPU: the C ABI is declared and exported, the agent key is injective,
train_battle refuses --rollout where it cannot work, and the collector's bound-based reservation on a device="cpu"
MemoryGroup grows geometrically and carries the rows up to the bound."""
import ctypes
import os
import re

import numpy as np
import pytest

import common

ENTRY = ("mfx_collect_reset", "mfx_collect_begin", "mfx_collect_end", "mfx_collect_key")


def test_collect_entry_points_declared_and_exported():
    header = open(os.path.join(common.REPO, "include", "magent_amd.h")).read()
    dll = ctypes.CDLL(common.HIP_LIB)
    for fn in ENTRY:
        assert re.search(r"\b(int|int64_t) %s\(" % fn, header), fn
        assert hasattr(dll, fn), fn
    for name in ("mfx_collect_src", "mfx_collect_dst"):
        assert re.search(r"typedef struct %s \{" % name, header), name
    assert re.search(r"names: [^*]*\bids, alive\b", header)
    assert "csrc/collect_kernels.hip" in open(os.path.join(common.PKG, "Makefile")).read()


def test_ctypes_structs_match_the_header_layout():
    """mfx_collect_src: nine pointers then eight int32; mfx_collect_dst: seven pointers then an int64."""
    from mfrl_amd.replay import _CollectDst, _CollectSrc
    assert ctypes.sizeof(_CollectSrc) == 9 * 8 + 8 * 4
    assert ctypes.sizeof(_CollectDst) == 7 * 8 + 8
    header = open(os.path.join(common.REPO, "include", "magent_amd.h")).read()
    body = re.search(r"typedef struct mfx_collect_src \{(.*?)\} mfx_collect_src;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\*?(\w+)\s*[,;]", body)
    assert names == [k for k, _ in _CollectSrc._fields_], names
    body = re.search(r"typedef struct mfx_collect_dst \{(.*?)\} mfx_collect_dst;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\*?(\w+)\s*[,;]", body)
    assert names == [k for k, _ in _CollectDst._fields_], names


def test_key_is_injective_and_matches_the_library():
    from mfrl_amd.replay import rollout_key
    E, stride = 5, 2 * 68
    env, ep, aid = np.meshgrid(np.arange(E), np.arange(7), np.arange(stride), indexing="ij")
    keys = rollout_key(env, ep, aid, E, stride).reshape(-1)
    assert len(np.unique(keys)) == keys.size
    assert keys.min() == 0 and keys.max() == 7 * E * stride - 1          # and dense: the grouping tables stay small
    dll = ctypes.CDLL(common.HIP_LIB)
    dll.mfx_collect_key.restype = ctypes.c_int64
    dll.mfx_collect_key.argtypes = [ctypes.c_int64] * 5
    for e, k, i in ((0, 0, 0), (4, 6, stride - 1), (3, 2, 17), (1, 1000000, 5)):
        assert dll.mfx_collect_key(e, k, i, E, stride) == rollout_key(e, k, i, E, stride)
    # the largest shape in use: 2048 envs of 2 x 2048 row slots, 400 episodes -- far inside int64
    assert rollout_key(2047, 400, 4095, 2048, 4096) < 2 ** 40


@pytest.mark.parametrize("argv", [["--algo", "mfq", "--rollout"],
                                  ["--algo", "mfq", "--envs", "1", "--rollout"],
                                  ["--algo", "ac", "--envs", "4", "--rollout"],
                                  ["--algo", "mfac", "--envs", "4", "--rollout"]])
def test_train_battle_refuses_rollout(argv, capsys):
    from mfrl_amd import train_battle
    with pytest.raises(SystemExit) as ex:
        train_battle.main(argv)
    assert ex.value.code == 2
    assert "--rollout" in capsys.readouterr().err


class _Eng:
    n_envs, rowcap, handles = 3, 8, (0, 1)


def _cpu_collector(capacity=None):
    from mfrl_amd.algo.tools import MemoryGroup
    from mfrl_amd.replay import RolloutCollector
    mg = MemoryGroup((13, 13, 7), (34,), 21, 64, 16, 8, use_mean=True, device="cpu")
    return mg, RolloutCollector(_Eng(), mg, 0, capacity=capacity)


def test_reservation_follows_the_bound():
    import torch
    mg, col = _cpu_collector()
    assert col.step_rows() == 24 and col.id_stride() == 16
    assert col.finish() == 0                       # no step since the last finish: nothing to read
    rows = mg._rows
    mg.push(ids=np.arange(5), state=[np.zeros((5, 13, 13, 7), np.float32), np.zeros((5, 34), np.float32)],
            acts=np.arange(5, dtype=np.int32), rewards=np.zeros(5, np.float32), alives=np.ones(5, bool),
            prob=np.zeros((5, 21), np.float32))
    caps, bound = [], 5
    for k in range(100):
        cap = col._reserve()
        bound += 24
        assert col._bound == bound and cap == rows.cap >= bound       # room for the worst case of this step
        if not caps or cap != caps[-1]:
            caps.append(cap)
        rows.cols["act"][bound - 24:bound] = k                        # what the kernels would write
    assert caps[0] == 1024 and all(b >= 2 * a for a, b in zip(caps, caps[1:])) and len(caps) == 3
    # every grow carried the rows up to the bound, the pushed ones included
    assert rows.cols["act"][:5].tolist() == list(range(5))
    assert torch.equal(rows.cols["act"][5:bound], torch.arange(100, dtype=torch.int32).repeat_interleave(24))
    assert rows.n == 5                              # the exact count is the device's: finish() sets it


def test_reservation_respects_the_capacity():
    mg, col = _cpu_collector(capacity=30)
    assert col._reserve() == 30 and col._bound == 24
    assert col._reserve() == 30 and col._bound <= mg._rows.cap
    mg._rows._ensure(4096)
    assert col._reserve() == 30
    col.discard()
    assert col._bound is None
