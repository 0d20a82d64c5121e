"""The rollout collector (mfx_collect_begin / _end / _end_linked, csrc/collect_kernels.hip), the compact row list
(mfx_rollout_rows) and the two return kernels (k_chain_returns, k_mfac_returns) on synthetic rollout buffers, off the
Battle shape: torch tensors stand in for an engine, the kernels are called through the ctypes structs of
mfrl_amd.replay, and every destination column -- one spare sentinel row at each end included -- is compared byte for
byte with tests/rows_ref.py::collect_ref.  tests/test_rows_ref_cpu.py checks the cases' own conditions."""
import ctypes

import numpy as np
import pytest

import rows_cases as rc
import rows_ref

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p
DST = {"obs": np.float32, "feat": np.float32, "act": np.int32, "rew": np.float32, "term": np.uint8, "prob": np.float32,
       "key": np.int64, "prev": np.int64, "tail": np.uint8}


def _sent(shape, dtype):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.full(n, rc.SENT, dtype=np.uint8).view(dtype).reshape(shape)


def _lib():
    from mfrl_amd import lib
    L = lib()
    for fn in ("mfx_collect_reset", "mfx_collect_begin", "mfx_collect_end", "mfx_collect_end_linked",
               "mfx_collect_links_reset", "mfx_rollout_rows"):
        getattr(L, fn).restype = ctypes.c_int
    return L


class Collector:
    """One collector over torch tensors: sentinel-filled destination columns of capacity + 2 rows (the kernels see row
    1 on), the device state, and the expected columns kept beside them in numpy."""

    def __init__(self, shape, capacity, n0=0, prob=True, linked=False):
        import torch
        self.shape, self.capacity, self.prob, self.linked = shape, capacity, prob, linked
        E, G, g, rowcap, V, F, A, ms = shape
        self.stride = G * rowcap
        widths = {"obs": (V,), "feat": (F,), "prob": (A,)}
        self.names = [k for k in DST if (prob or k != "prob") and (linked or k not in ("prev", "tail"))]
        self.want = {k: _sent((capacity + 2,) + widths.get(k, ()), DST[k]) for k in self.names}
        self.cols = {k: torch.from_numpy(v.copy()).cuda() for k, v in self.want.items()}
        self.state = torch.zeros(2, dtype=torch.int64, device="cuda")
        self.scratch = torch.full((E * rowcap + 1 + (E + 63) // 64,), -7, dtype=torch.int32, device="cuda")
        self.n, self.err = n0, 0
        self.L = _lib()
        self.st = P(torch.cuda.current_stream().cuda_stream)
        assert self.L.mfx_collect_reset(P(self.state.data_ptr()), ctypes.c_int64(n0), self.st) == 0
        if linked:
            self.links = rows_ref.links_state(E, self.stride)
            self.links["key"] = np.zeros(n0, np.int64)
            self.links["tail"] = self.want["tail"][1:1 + n0].copy()
            self.links["prev"] = self.want["prev"][1:1 + n0].copy()
            self.last = torch.full((E * self.stride + 2,), 77, dtype=torch.int64, device="cuda")
            assert self.L.mfx_collect_links_reset(P(self.last.data_ptr() + 8), ctypes.c_int64(E * self.stride),
                                                  self.st) == 0

    def structs(self, src, **over):
        from mfrl_amd.replay import _CollectDst, _CollectSrc
        E, G, g, rowcap, V, F, A, ms = self.shape
        f = dict(n_envs=E, n_groups=G, group=g, rowcap=rowcap, view_floats=V, feat_floats=F, n_action=A, mean_stride=ms)
        f.update({k: src[k].data_ptr() for k in rc.COLLECT_NAMES})
        d = {k: self.cols[k][1:].data_ptr() for k in ("obs", "feat", "act", "rew", "term", "key")}
        d["prob"] = self.cols["prob"][1:].data_ptr() if self.prob else None
        d["capacity"] = self.capacity
        for k, v in over.items():
            (f if k in f else d)[k] = v
        return _CollectSrc(**f), _CollectDst(**d)

    def calls(self, s, d):
        """(name, thunk) of begin and the end this collector uses."""
        rows, total = P(self.scratch.data_ptr()), P(self.scratch.data_ptr() + 4 * self.shape[0] * self.shape[3])
        a = (ctypes.byref(s), ctypes.byref(d), rows, total, P(self.state.data_ptr()))
        out = [("begin", lambda: self.L.mfx_collect_begin(*a, self.st))]
        if self.linked:
            out.append(("end_linked", lambda: self.L.mfx_collect_end_linked(
                *a, ctypes.c_int64(self.stride), P(self.last.data_ptr() + 8), P(self.cols["prev"][1:].data_ptr()),
                P(self.cols["tail"][1:].data_ptr()), self.st)))
        else:
            out.append(("end", lambda: self.L.mfx_collect_end(*a, ctypes.c_int64(self.stride), self.st)))
        return out

    def step(self, arrays):
        """One begin + end pair on the device and in the reference; returns the reference's result."""
        import torch
        src = {k: torch.from_numpy(np.ascontiguousarray(arrays[k])).cuda() for k in rc.COLLECT_NAMES}
        s, d = self.structs(src)
        for name, call in self.calls(s, d):
            assert call() == 0, (name, self.L.mfx_last_error().decode())
        torch.cuda.synchronize()
        res = rows_ref.collect_ref(arrays, self.shape, self.n, self.capacity, self.stride,
                                   self.links if self.linked else None, prob=self.prob)
        if res["fits"]:
            for k, v in res["cols"].items():
                self.want[k][1 + self.n:1 + res["n"]] = v
            if self.linked:
                self.links = res["state"]
                self.want["prev"][1:1 + res["n"]] = self.links["prev"]
                self.want["tail"][1:1 + res["n"]] = self.links["tail"]
        self.n, self.err = res["n"], self.err | res["err"]
        return res

    def check(self):
        assert self.state.cpu().tolist() == [self.n, self.err]
        for k in self.names:
            got = self.cols[k].cpu().numpy()
            assert got[0].tobytes() == self.want[k][0].tobytes() and got[-1].tobytes() == self.want[k][-1].tobytes(), k
            assert got.tobytes() == self.want[k].tobytes(), k
        if self.linked:
            last = self.last.cpu().numpy()
            assert last[0] == 77 and last[-1] == 77 and np.array_equal(last[1:-1], self.links["last"])


# ------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("shape", rc.COLLECT_SHAPES, ids=str)
@pytest.mark.parametrize("prob", [True, False], ids=["prob", "noprob"])
def test_collect_shapes(shape, prob):
    for linked in (False, True):
        col = Collector(shape, capacity=shape[0] * shape[3] + 9, n0=3, prob=prob, linked=linked)
        res = col.step(rc.collect_inputs(shape))
        assert res["fits"] and res["count"] > 0
        col.check()


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_begin_refills_both_pipeline_slots():
    """8,000 rows: more than two rounds of k_collect_begin's grid (3 workgroups per CU, four waves each)."""
    shape = rc.LONG_BEGIN
    assert shape[0] * shape[3] > 2 * rc.begin_grid_waves(_cus(), shape)
    col = Collector(shape, capacity=shape[0] * shape[3] + 5, n0=2)
    assert col.step(rc.collect_inputs(shape, full=True))["count"] == shape[0] * shape[3]
    col.check()


def test_end_takes_its_grid_stride():
    """Just more rows than k_collect_end's grid has lanes (8 workgroups per CU)."""
    shape = rc.long_end_shape(_cus())
    assert shape[0] * shape[3] > rc.end_grid_lanes(_cus(), shape)
    col = Collector(shape, capacity=shape[0] * shape[3] + 1, n0=1)
    assert col.step(rc.collect_inputs(shape, full=True))["count"] == shape[0] * shape[3]
    col.check()


# ------------------------------------------------------------------------------------------------- steps in a row
@pytest.mark.parametrize("linked", [True, False], ids=["linked", "unlinked"])
def test_three_steps_in_a_row(linked):
    import torch
    from mfrl_amd.replay import chain_returns, chain_returns_host
    shape = (4, 2, 1, 9, 4, 33, 2, 24)
    col = Collector(shape, capacity=3 * shape[0] * shape[3], linked=linked)
    ns = []
    for arrays in rc.three_steps(shape):
        res = col.step(arrays)
        assert res["fits"]
        col.check()                                       # prev / tail / last after every step
        ns.append(col.n)
    assert 0 < ns[0] < ns[1] < ns[2] and col.err == 2     # the two ids outside [0, id_stride)
    if not linked:
        return
    n = col.n
    prev, tail = col.links["prev"], col.links["tail"]
    assert (prev >= 0).sum() > 10
    tails = np.flatnonzero(tail)
    values = np.random.RandomState(9).standard_normal(len(tails)).astype(np.float32)
    rew = col.want["rew"][1:1 + n].copy()
    for numpy1 in (True, False):
        got = chain_returns(col.cols["rew"][1:1 + n].clone(), col.cols["prev"][1:1 + n].contiguous(),
                            torch.from_numpy(tails).cuda(), torch.from_numpy(values).cuda(), 0.95, numpy1=numpy1)
        assert got.cpu().numpy().tobytes() == chain_returns_host(rew, prev, tails, values, 0.95, numpy1).tobytes()


# ------------------------------------------------------------------------------------------------- capacity
@pytest.mark.parametrize("linked", [True, False], ids=["linked", "unlinked"])
def test_capacity_is_exact(linked):
    shape = (4, 2, 1, 9, 4, 33, 2, 24)
    arrays = rc.collect_inputs(shape)
    count = rows_ref.rollout_rows_ref(arrays["counts"], shape[2], shape[3])[1]
    fit = Collector(shape, capacity=5 + count, n0=5, linked=linked)
    assert fit.step(arrays)["fits"] and fit.n == 5 + count and fit.err == 0
    fit.check()
    full = Collector(shape, capacity=5 + count - 1, n0=5, linked=linked)
    res = full.step(arrays)
    assert not res["fits"] and full.n == 5 and full.err == 1
    full.check()                                          # no column, link or table entry was written
    for k in full.names:
        assert (full.cols[k].cpu().numpy().view(np.uint8) == rc.SENT).all(), k


# ------------------------------------------------------------------------------------------------- refusals
BASE = (2, 2, 0, 6, 8, 34, 21, 24)
REFUSALS = [("V_0", dict(view_floats=0), "view rows of 1..1283 floats"),
            ("V_1284", dict(view_floats=1284), "view rows of 1..1283 floats"),
            ("V_5124", dict(view_floats=5124), "view rows of 1..1283 floats"),
            ("F_0", dict(feat_floats=0), "feature rows of 1..64 floats"),
            ("F_65", dict(feat_floats=65), "feature rows of 1..64 floats"),
            ("A_65_with_prob", dict(n_action=65, mean_stride=80), "mean actions of 1..64 entries"),
            ("A_over_mean_stride", dict(n_action=21, mean_stride=20), "within the stride"),
            ("group_is_n_groups", dict(group=2), "bad batch shape"),
            ("view_at_2_bytes", dict(view=2), "4-byte aligned"),
            ("null_column", dict(rew=None), "destination column is missing")] + \
           [("V_%d" % s[4], dict(shape=s), "view rows of 1..1283 floats") for s in rc.COLLECT_TOO_WIDE]


@pytest.mark.parametrize("name,over,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_store_nothing(name, over, msg):
    import torch
    over = dict(over)
    shape = over.pop("shape", BASE)
    for linked in (False, True):
        col = Collector(shape, capacity=40, linked=linked)
        src = {k: torch.from_numpy(v).cuda() for k, v in rc.collect_inputs(shape).items()}
        o = dict(over)
        if "view" in o:
            o["view"] = src["view"].data_ptr() + o["view"]
        s, d = col.structs(src, **o)
        for call_name, call in col.calls(s, d):
            assert call() != 0, call_name
            assert msg in col.L.mfx_last_error().decode(), (call_name, col.L.mfx_last_error().decode())
        torch.cuda.synchronize()
        col.check()
        assert (col.scratch == -7).all()


# ------------------------------------------------------------------------------------------------- the row list
@pytest.mark.parametrize("G,g", [(1, 0), (3, 0), (3, 1), (3, 2)])
@pytest.mark.parametrize("E,rowcap", [(70, 1), (70, 300), (5, 2048), (0, 300)])
def test_rollout_rows(E, rowcap, G, g):
    import torch
    rng = np.random.RandomState(E + rowcap + G + g)
    counts = rng.randint(0, rowcap + 3, size=(E, G)).astype(np.int32)
    if E:
        counts[0, g], counts[E // 2, g], counts[-1, g] = rowcap + 2, 0, rowcap
    d_counts = torch.from_numpy(counts).cuda()
    buf = torch.full((E * rowcap + 1 + (E + 63) // 64 + 1,), -7, dtype=torch.int32, device="cuda")
    L = _lib()
    assert L.mfx_rollout_rows(P(d_counts.data_ptr()), E, G, g, rowcap, P(buf.data_ptr()),
                              P(buf.data_ptr() + 4 * E * rowcap), P(torch.cuda.current_stream().cuda_stream)) == 0
    got = buf.cpu().numpy()
    want, n = rows_ref.rollout_rows_ref(counts, g, rowcap)
    assert got[E * rowcap] == n and np.array_equal(got[:n], want)
    assert (got[n:E * rowcap] == -7).all() and got[-1] == -7


# ------------------------------------------------------------------------------------------------- chains, returns
@pytest.mark.parametrize("numpy1", [True, False], ids=["numpy1", "nep50"])
@pytest.mark.parametrize("n", rc.COUNTS)
def test_chain_returns_counts(n, numpy1):
    import torch
    from mfrl_amd.replay import chain_returns, chain_returns_host
    for ones in (False, True):
        rew, prev, tails, values = rc.chains(n, ones=ones)
        for gamma in rc.GAMMAS:
            got = chain_returns(*(torch.from_numpy(x).cuda() for x in (rew, prev, tails, values)), gamma, numpy1=numpy1)
            assert got.cpu().numpy().tobytes() == chain_returns_host(rew, prev, tails, values, gamma, numpy1).tobytes()


@pytest.mark.parametrize("numpy1", [True, False], ids=["numpy1", "nep50"])
@pytest.mark.parametrize("n", rc.COUNTS)
def test_mfac_returns_counts(n, numpy1):
    import torch
    from mfrl_amd.mf import mfac_returns
    rew, offsets, values = rc.episodes(n)
    for gamma in rc.GAMMAS:
        t = torch.from_numpy(np.concatenate([rew, np.float32([123.0])])).cuda()       # one spare entry past the rows
        got = mfac_returns(t[:len(rew)], torch.from_numpy(offsets).cuda(), torch.from_numpy(values).cuda(), gamma,
                           numpy1=numpy1)
        assert got.cpu().numpy().tobytes() == rows_ref.mfac_returns_ref(rew, offsets, values, gamma, numpy1).tobytes()
        assert float(t[-1]) == 123.0
