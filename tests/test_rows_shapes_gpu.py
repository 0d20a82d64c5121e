"""The replay rows' mover (mfx_rows_copy_shift: k_rows_copy, k_rows_pipe<NW, NU>; csrc/replay_kernels.hip) off the
Battle row shape, bit for bit against tests/rows_ref.py::rows_copy_ref: every width path and tail of a wide column,
the limits of the pipelined form, narrow columns in dword and byte units, the template boundaries, indices above 2^32
and below zero under a modulo, shifts, the ring, the refusals.  Columns are views into uint8 buffers at a byte offset;
every buffer has a spare row at each end, destinations are filled with a sentinel and compared whole.  Each case
asserts the launch form it was written for (replay.rows_plan); tests/test_rows_ref_cpu.py checks the cases' own
conditions."""
import ctypes

import numpy as np
import pytest

import rows_cases as rc
import rows_ref

pytestmark = pytest.mark.gpu


def _device(arrays, cols):
    """Per column a uint8 tensor [rows + 2, bytes] at its byte offset inside a buffer of its own."""
    import torch
    out = []
    for a, (b, off) in zip(arrays, cols):
        buf = torch.empty(off + a.size + 16, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        buf.fill_(0x3C)
        view = buf[off:off + a.size].view(a.shape)
        view.copy_(torch.from_numpy(a))
        out.append((buf, view))
    return out


def _run(case, pipe, monkeypatch):
    import torch
    from mfrl_amd import replay
    monkeypatch.setenv("MFX_ROWS_PIPE", pipe)
    src, dst = case.buffers()
    d_src, d_dst = _device(src, case.cols), _device(dst, case.cols)
    s_in, d_in = [v[1:-1] for _, v in d_src], [v[1:-1] for _, v in d_dst]
    for k, (b, off) in enumerate(case.cols):
        assert s_in[k].data_ptr() % 16 == d_in[k].data_ptr() % 16 == (off + b) % 16
    assert replay.rows_plan(d_in, s_in, case.shift_mask) == case.expected_plan(pipe)
    a = case.args()
    bad = rows_ref.rows_copy_ref([x[1:-1] for x in dst], [x[1:-1] for x in src], **a)
    idx = None if a["idx"] is None else torch.from_numpy(a["idx"]).cuda()
    replay.rows_copy(d_in, s_in, idx, a["src_mod"], a["dst_start"], a["dst_cap"], a["n"], a["shift_mask"], a["shift"])
    torch.cuda.synchronize()
    for k in range(len(case.cols)):
        got = d_dst[k][1].cpu().numpy()
        assert (got[0] == rc.SENT).all() and (got[-1] == rc.SENT).all(), ("spare rows of column", k)
        assert np.array_equal(got, dst[k]), ("column", k)
        assert np.array_equal(d_src[k][1].cpu().numpy(), src[k]), ("source column", k)
        off, size = case.cols[k][1], dst[k].size
        pad = d_dst[k][0].cpu().numpy()
        assert (pad[:off] == 0x3C).all() and (pad[off + size:] == 0x3C).all(), ("around column", k)
    return bad


def _cases(cases):
    return [pytest.param(c, p, id="%s-pipe%s" % (c.name, p)) for c in cases for p in c.pipes]


@pytest.mark.parametrize("case,pipe", _cases(rc.SMALL_CASES))
def test_rows_copy_case(case, pipe, monkeypatch):
    from mfrl_amd.replay import check_errors
    assert _run(case, pipe, monkeypatch) == []
    check_errors()


@pytest.mark.parametrize("case,bad", rc.OOB_CASES, ids=lambda x: getattr(x, "name", None))
@pytest.mark.parametrize("pipe", ["1", "0"])
def test_out_of_range_row_is_skipped_and_reported(case, bad, pipe, monkeypatch):
    from mfrl_amd.replay import check_errors
    assert _run(case, pipe, monkeypatch) == [bad]
    with pytest.raises(IndexError, match="index %d out of range" % bad):
        check_errors()
    check_errors()


def test_more_rows_than_four_rounds_of_the_persistent_grid(monkeypatch):
    import torch
    from mfrl_amd.replay import check_errors
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = rc.big_grid_case(cus)
    assert case.n > 4 * rc.pipe_rows_per_round(cus)
    assert _run(case, "1", monkeypatch) == []
    check_errors()


def test_grid_stride_of_the_one_row_per_wave_form(monkeypatch):
    from mfrl_amd.replay import check_errors
    case = rc.stride_case()
    assert case.n > rc.COPY_GRID_ROWS
    assert _run(case, "0", monkeypatch) == []
    check_errors()


# ------------------------------------------------------------------------------------------------------- refusals
def _raw(dst, src, row_bytes, n_cols=None, idx=None, src_mod=0, src_rows=None, dst_start=0, dst_cap=0, n=0, mask=0):
    import torch
    from mfrl_amd import lib
    L = lib()
    L.mfx_rows_copy_shift.restype = ctypes.c_int
    k = len(dst)
    P = ctypes.c_void_p * max(k, 1)
    rb = (ctypes.c_int64 * max(k, 1))(*row_bytes)
    ret = L.mfx_rows_copy_shift(k if n_cols is None else n_cols, P(*[d.data_ptr() if d is not None else 0 for d in dst]),
                                P(*[s.data_ptr() for s in src]), rb,
                                ctypes.c_void_p(idx.data_ptr() if idx is not None else 0), ctypes.c_int64(src_mod),
                                ctypes.c_int64(src_rows), ctypes.c_int64(dst_start), ctypes.c_int64(dst_cap),
                                ctypes.c_int64(n), ctypes.c_uint32(mask), ctypes.c_int64(1),
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return ret, L.mfx_last_error().decode()


REFUSALS = [
    ("no_columns", dict(n_cols=0, n=4), "1..12 columns, got 0"),
    ("thirteen_columns", dict(n_cols=13, n=4), "1..12 columns, got 13"),
    ("mask_past_the_last", dict(n=4, mask=1 << 2), "names columns past 2"),
    ("modulo_over_source", dict(n=4, src_mod=11), "modulo 11 over 10"),
    ("no_list_n_over_source", dict(n=11), "11 rows from 10 source rows"),
    ("n_over_ring", dict(n=5, dst_cap=4, idx=True), "5 rows into a ring of 4"),
    ("negative_n", dict(n=-1), "-1 rows into a ring"),
    ("zero_byte_column", dict(n=4, zero=True), "column 1 is empty"),
    ("null_column", dict(n=4, null=True), "column 0 is empty"),
]


@pytest.mark.parametrize("name,kw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_store_nothing(name, kw, msg):
    import torch
    kw = dict(kw)
    src = [torch.arange(10 * 129, device="cuda", dtype=torch.int32).view(10, 129), torch.arange(10, device="cuda")]
    dst = [torch.full((12, 129), -3, device="cuda", dtype=torch.int32), torch.full((12,), -3, device="cuda")]
    rb = [516, 0 if kw.pop("zero", False) else 8]
    idx = torch.arange(5, device="cuda") if kw.pop("idx", None) else None
    d = [None, dst[1]] if kw.pop("null", False) else dst
    ret, err = _raw(d, src, rb, idx=idx, src_rows=10, **kw)
    torch.cuda.synchronize()
    assert ret != 0 and msg in err, err
    assert (dst[0] == -3).all() and (dst[1] == -3).all()


def test_zero_rows_succeed_and_store_nothing():
    import torch
    src = [torch.arange(10 * 129, device="cuda", dtype=torch.int32).view(10, 129)]
    dst = [torch.full((12, 129), -3, device="cuda", dtype=torch.int32)]
    ret, _ = _raw(dst, src, [516], src_rows=10, n=0)
    torch.cuda.synchronize()
    assert ret == 0 and (dst[0] == -3).all()


def test_plan_honours_the_environment_and_refuses_like_the_launcher(monkeypatch):
    import torch
    from mfrl_amd import EngineError, lib, replay
    x = torch.zeros((8, 129), device="cuda")
    monkeypatch.delenv("MFX_ROWS_PIPE", raising=False)
    assert replay.rows_plan([x], [x]) == {"form": 1, "nw": 1, "nu": 1, "units": 0, "cols": [2]}
    monkeypatch.setenv("MFX_ROWS_PIPE", "0")
    assert replay.rows_plan([x], [x]) == {"form": 0, "nw": 0, "nu": 0, "units": 0, "cols": [2]}
    with pytest.raises(EngineError, match="names columns past 1"):
        replay.rows_plan([x], [x], shift_mask=2)
    L = lib()
    L.mfx_rows_copy_plan.restype = ctypes.c_int
    out = (ctypes.c_int32 * 5)()
    P = ctypes.c_void_p * 1
    assert L.mfx_rows_copy_plan(13, P(x.data_ptr()), P(x.data_ptr()), (ctypes.c_int64 * 1)(516), 0, out) != 0
    assert L.mfx_rows_copy_plan(1, P(x.data_ptr()), P(x.data_ptr()), (ctypes.c_int64 * 1)(0), 0, out) != 0
    assert L.mfx_rows_copy_plan(1, P(x.data_ptr()), P(x.data_ptr()), (ctypes.c_int64 * 1)(516), 0, None) != 0
