"""The mean-field kernels (csrc/mf_kernels.hip) off the Battle shape, bit for bit against tests/rows_ref.py:
k_mfq_target over action counts, batch sizes around a workgroup, hand-built NaN / infinity / signed-zero rows and every
done byte; k_mean_action over action counts and row capacities around a workgroup, actions outside the range, and
counts above the row capacity (capped, as the row-list kernels cap them); and the wrappers' dtype refusals
(mfrl_amd/mf.py), which need no kernel.  tests/test_rows_ref_cpu.py checks the inputs' own conditions."""
import numpy as np
import pytest

import rows_cases as rc
import rows_ref

gpu = pytest.mark.gpu


def _cuda(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


# ------------------------------------------------------------------------------------------------- k_mfq_target
@gpu
@pytest.mark.parametrize("A", [1, 2, 21, 33])
@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_mfq_target_shapes(M, A):
    from mfrl_amd.mf import mfq_target
    eq, tq, r, done = rc.mfq_inputs(M, A)
    for gamma in (0.95, 0.0, 1.0):
        got = mfq_target(*_cuda(eq, tq, r, done), gamma).cpu().numpy()
        assert got.dtype == np.float64
        assert got.tobytes() == rows_ref.mfq_target_ref(eq, tq, r, done, gamma).tobytes(), gamma


@gpu
@pytest.mark.parametrize("A", [1, 2, 21, 33])
def test_mfq_target_hand_built_rows(A):
    """Each hand-built row on its own, not done, with t_q = the column index: the target names the chosen action."""
    from mfrl_amd.mf import mfq_target
    rows = rc.mfq_rows(A)
    eq = np.stack(list(rows.values()))
    M = len(eq)
    tq = np.tile(np.arange(A, dtype=np.float32), (M, 1))
    r, done = np.zeros(M, np.float32), np.zeros(M, np.uint8)
    got = mfq_target(*_cuda(eq, tq, r, done), 1.0).cpu().numpy()
    want = rows_ref.mfq_target_ref(eq, tq, r, done, 1.0)
    assert dict(zip(rows, got.tolist())) == dict(zip(rows, want.tolist()))
    assert got.tobytes() == want.tobytes()
    assert want.tolist() == [float(np.argmax(v)) for v in rows.values()]


@gpu
def test_mfq_target_empty_batch_and_refusal():
    import torch
    from mfrl_amd import EngineError
    from mfrl_amd.mf import mfq_target
    z = torch.zeros((0, 3), device="cuda")
    assert mfq_target(z, z, z[:, 0], z[:, 0].to(torch.uint8)).shape == (0,)
    z = torch.zeros((4, 0), device="cuda")
    with pytest.raises(EngineError, match="A must be >= 1"):
        mfq_target(z, z, torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda", dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------- k_mean_action
@gpu
@pytest.mark.parametrize("n_action", [1, 2, 21, 255, 256])
@pytest.mark.parametrize("rowcap", [1, 255, 256, 257, 1000])
def test_mean_action_shapes(rowcap, n_action):
    from mfrl_amd.mf import mean_action
    acts, counts = rc.mean_action_inputs(n_action, rowcap)
    d_acts, d_counts = _cuda(acts, counts)
    got = mean_action(d_acts[:-1], d_counts, n_action).cpu().numpy()
    want = rows_ref.mean_action_ref(acts[:-1], counts, n_action)
    assert got.shape == want.shape and np.isnan(want[0]).all() and not np.isnan(want[2]).any()
    assert got.tobytes() == want.tobytes()


@gpu
@pytest.mark.parametrize("n_action,rowcap", [(21, 1), (21, 256), (2, 255), (256, 257), (1, 1000)])
def test_mean_action_caps_counts_at_rowcap(n_action, rowcap):
    """Counts in (rowcap, 2 rowcap] pool the row's rowcap slots and nothing of the next row (whose actions differ: the
    CPU test shows an uncapped reader would give another result).  B + 1 rows are allocated and B passed, so that a
    reader without the cap stays inside the allocation; negative counts read as 0."""
    from mfrl_amd.mf import mean_action
    acts, counts = rc.mean_action_inputs(n_action, rowcap, over=True)
    assert (counts > rowcap).sum() == 3 and counts.max() <= 2 * rowcap
    d_acts, d_counts = _cuda(acts, counts)
    got = mean_action(d_acts[:-1], d_counts, n_action).cpu().numpy()
    assert got.tobytes() == rows_ref.mean_action_ref(acts[:-1], counts, n_action).tobytes()
    counts[1], counts[4] = -1, -(1 << 31)
    got = mean_action(d_acts[:-1], _cuda(counts)[0], n_action).cpu().numpy()
    assert np.isnan(got[[0, 1, 4]]).all()
    assert got.tobytes() == rows_ref.mean_action_ref(acts[:-1], counts, n_action).tobytes()


@gpu
def test_mean_action_empty_batch_and_refusals():
    import torch
    from mfrl_amd import EngineError
    from mfrl_amd.mf import mean_action
    acts = torch.zeros((0, 5), dtype=torch.int32, device="cuda")
    assert mean_action(acts, torch.zeros(0, dtype=torch.int32, device="cuda"), 21).shape == (0, 21)
    acts = torch.zeros((2, 5), dtype=torch.int32, device="cuda")
    counts = torch.ones(2, dtype=torch.int32, device="cuda")
    for n_action in (0, 257):
        with pytest.raises(EngineError, match="1 <= n_action <= 256"):
            mean_action(acts, counts, n_action)


# ------------------------------------------------------------------------------------------------- dtype refusals
class _NoLibrary:
    def __call__(self):
        raise AssertionError("the library was reached")


@pytest.fixture
def no_library(monkeypatch):
    """The wrappers must refuse before any library call: lib() itself fails the test."""
    import mfrl_amd.mf as mf
    monkeypatch.setattr(mf, "lib", _NoLibrary())
    return mf


def test_mean_action_refuses_other_dtypes(no_library):
    import torch
    mf = no_library
    a32, c32 = torch.zeros((3, 4), dtype=torch.int32), torch.ones(3, dtype=torch.int32)
    with pytest.raises(TypeError, match="actions must be torch.int32"):
        mf.mean_action(a32.long(), c32, 5)                 # (once read as pairs of int32)
    with pytest.raises(TypeError, match="counts must be torch.int32"):
        mf.mean_action(a32, c32.long(), 5)
    with pytest.raises(TypeError):
        mf.mean_action(a32.float(), c32, 5)
    with pytest.raises(ValueError):
        mf.mean_action(a32, c32[:2], 5)
    with pytest.raises(AssertionError, match="the library was reached"):
        mf.mean_action(a32, c32, 5)


def test_mfq_target_refuses_other_dtypes(no_library):
    import torch
    mf = no_library
    q, r, d = torch.zeros((3, 4)), torch.zeros(3), torch.zeros(3, dtype=torch.uint8)
    for name, args in (("e_q", (q.double(), q, r, d)), ("t_q", (q, q.half(), r, d)), ("rewards", (q, q, r.double(), d))):
        with pytest.raises(TypeError, match="%s must be torch.float32" % name):
            mf.mfq_target(*args)
    with pytest.raises(ValueError):
        mf.mfq_target(q, q[:, :3], r, d)
    with pytest.raises(ValueError):
        mf.mfq_target(q, q, r[:2], d)
    with pytest.raises(AssertionError, match="the library was reached"):
        mf.mfq_target(q, q, r, d.bool())


def test_mfac_returns_refuses_other_dtypes_and_lengths(no_library):
    import torch
    mf = no_library
    rew, off, val = torch.zeros(6), torch.tensor([0, 2, 6]), torch.zeros(2)
    assert off.dtype == torch.int64
    with pytest.raises(TypeError, match="rewards must be torch.float32"):
        mf.mfac_returns(rew.double(), off, val)
    with pytest.raises(TypeError, match="offsets must be torch.int64"):
        mf.mfac_returns(rew, off.int(), val)
    with pytest.raises(TypeError, match="values must be torch.float32"):
        mf.mfac_returns(rew, off, val.double())
    with pytest.raises(ValueError, match="contiguous"):
        mf.mfac_returns(torch.zeros(12)[::2], off, val)
    with pytest.raises(ValueError, match="3 offsets for 3 values"):
        mf.mfac_returns(rew, off, torch.zeros(3))
    with pytest.raises(ValueError, match="2 offsets for 2 values"):
        mf.mfac_returns(rew, off[:2], val)
    with pytest.raises(AssertionError, match="the library was reached"):
        mf.mfac_returns(rew, off, val)
