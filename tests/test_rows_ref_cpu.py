"""The NumPy references of tests/rows_ref.py against independent forms, and every input condition the GPU cases of
tests/test_rows_shapes_gpu.py, test_collect_shapes_gpu.py and test_mf_shapes_gpu.py rely on (tests/rows_cases.py), so
that no case quietly degenerates.  No GPU, no engine library."""
import os

import numpy as np
import pytest

import common
import rows_cases as rc
import rows_ref

MI355X_CUS = 256
ALL_ROW_CASES = rc.SMALL_CASES + [c for c, _ in rc.OOB_CASES] + [rc.big_grid_case(MI355X_CUS)]


def _fancy(case, src, dst):
    """rows_copy by vectorised fancy indexing: dst[d] = src[s] over the rows whose indices are in range."""
    n, n_src = case.n, case.n_src
    raw = (case.idx if case.idx is not None else np.arange(n, dtype=np.int64)).astype(object)   # exact integers

    def rows(x):
        if case.src_mod:
            s = x % case.src_mod
        else:
            s = np.array([v + n_src if v < 0 else v for v in x], dtype=object)
        ok = np.array([0 <= v < n_src for v in s], dtype=bool)
        return np.where(ok, s, 0).astype(np.int64), ok
    s0, ok0 = rows(raw)
    s1, ok1 = rows(raw + case.shift) if case.shift_mask else (s0, ok0)
    ok = ok0 & ok1
    d = case.dst_start + np.arange(n)
    if case.dst_cap:
        d = np.where(d >= case.dst_cap, d % case.dst_cap, d)
    for k, (a, b) in enumerate(zip(dst, src)):
        a[d[ok]] = b[(s1 if case.shift_mask >> k & 1 else s0)[ok]]
    bad = [int(raw[i]) if not ok0[i] else int(raw[i]) + case.shift for i in np.flatnonzero(~ok)]
    return bad, s0, s1, d


@pytest.mark.parametrize("case", ALL_ROW_CASES + [rc.stride_case()], ids=repr)
def test_rows_copy_ref_matches_fancy_indexing(case):
    src, dst = case.buffers()
    want = [x.copy() for x in dst]
    bad = rows_ref.rows_copy_ref([x[1:-1] for x in dst], [x[1:-1] for x in src], **case.args())
    bad2, _, _, d = _fancy(case, [x[1:-1] for x in src], [x[1:-1] for x in want])
    assert bad == bad2
    for a, b in zip(dst, want):
        assert np.array_equal(a, b)
        assert (a[0] == rc.SENT).all() and (a[-1] == rc.SENT).all()          # the spare rows
    assert len(set(d.tolist())) == case.n                                     # distinct destination rows
    assert any((a[1:-1] != rc.SENT).any() for a in dst)


@pytest.mark.parametrize("case", ALL_ROW_CASES + [rc.stride_case()], ids=repr)
def test_row_case_plans_follow_from_the_columns(case):
    """The plan a case states against the launcher's documented rule, restated here from the column sizes and offsets
    alone (an aligned base is the GPU test's own assertion)."""
    units, codes, n_wide, wide_ok = 0, [], 0, True
    for b, off in case.cols:
        a4 = ((off + b) | b) & 3 == 0
        if b >= rc.BIG_ROW:
            codes.append(2)
            n_wide += 1
            wide_ok = wide_ok and a4 and b // 4 <= rc.PIPE_MAX_DW
        else:
            codes.append(0 if a4 else 1)
            units += b // 4 if a4 else b
    pipe = n_wide <= 2 and wide_ok and units <= 128
    want = (1, 2 if n_wide == 2 else 1, 2 if units > 64 else 1) if pipe else (0, 0, 0)
    assert case.plan == want + (units, tuple(codes))
    assert len(case.cols) <= 12 and case.expected_plan("0")["form"] == 0
    if "0" not in case.pipes:
        assert case.plan[0] == 1
    for k, (b, off) in enumerate(case.cols):
        if case.wide is not None and b >= rc.BIG_ROW:
            assert case.wide_path(k) == case.wide


def _by_name(name):
    return next(c for c in ALL_ROW_CASES if c.name == name)


def test_row_cases_cover_what_they_claim():
    names = [c.name for c in ALL_ROW_CASES]
    assert len(set(names)) == len(names)
    # wide widths: every path, every tail, the limits of the pipelined form, more than one round of both copy loops
    paths = {(c.cols[0][0], c.cols[0][1]): c.wide for c in rc.WIDE_CASES}
    assert paths[(512, 0)] == paths[(528, 0)] == 16 and paths[(528, 4)] == 4 and paths[(516, 0)] == 4
    assert paths[(515, 0)] == paths[(1027, 0)] == 1
    assert [(b // 4) & 3 for b in (1280, 1284, 1288, 1292)] == [0, 1, 2, 3] and 1280 // 16 == 80
    assert 5120 // 16 == 320 and 5132 // 4 == rc.PIPE_MAX_DW and 5136 // 4 == rc.PIPE_MAX_DW + 1
    assert _by_name("wide_5132_at0").plan[0] == 1 and _by_name("wide_5136_at0").plan[0] == 0
    assert _by_name("wide_5124_at4").plan[0] == 1 and 512 // 16 < 64
    assert 20480 > rc.COPY16_ROUND and 20484 > rc.COPY4_ROUND
    assert rc.COPY16_ROUND < 7696 < 2 * rc.COPY16_ROUND and rc.COPY4_ROUND < 7700 < 2 * rc.COPY4_ROUND
    # narrow: unit totals at the template boundaries, a wide column whose ustart is in the middle
    assert [_by_name("units_%d" % u).plan[:4] for u in (64, 65, 128, 129)] == \
        [(1, 1, 1, 64), (1, 1, 2, 65), (1, 1, 2, 128), (0, 0, 0, 129)]
    assert all(c.plan[4].count(2) == 0 for c in rc.NARROW_CASES[:9]) and len(_by_name("twelve_columns").cols) == 12
    assert _by_name("narrow_wide_narrow").plan[4] == (0, 2, 0) and _by_name("narrow_4_at1").plan[4] == (1, 0)
    assert {b for c in rc.NARROW_CASES for b, _ in c.cols} >= {1, 2, 3, 6, 7, 508}
    assert _by_name("one_wide_100_units").plan[:3] == (1, 1, 2) and _by_name("two_wide").plan[:3] == (1, 2, 1)
    assert _by_name("three_wide").plan[0] == 0 and _by_name("two_wide_one_misaligned").plan[0] == 0
    # indices
    c = _by_name("mod_big_indices")
    assert c.src_mod == c.n_src == 599 and (1 << 32) % 599 != 0
    assert (c.idx >= 1 << 32).sum() > 100 and (c.idx < 0).sum() > 50 and c.idx.max() < 1 << 40
    assert any(int(v) % 599 != (int(v) & 0xffffffff) % 599 for v in c.idx if v >= 1 << 32)   # 32 bits are not enough
    assert _by_name("mod_below_src_rows").src_mod < _by_name("mod_below_src_rows").n_src
    assert _by_name("mod_1").src_mod == 1
    mod = 250
    assert [c.shift for c in ALL_ROW_CASES if c.name.startswith("mod_shift_")] == [0, -1, mod - 1, mod, mod + 3]
    for c in ALL_ROW_CASES:
        if c.name.startswith("mod_shift_"):
            assert c.src_mod == mod and c.shift_mask and (c.idx % mod == mod - 1).any() and (c.idx < 0).any()
    up, down = _by_name("shift_+2_no_mod"), _by_name("shift_-1_no_mod")
    assert ((up.idx < 0) & (up.idx + 2 >= 0)).any() and ((down.idx >= 0) & (down.idx - 1 < 0)).any()
    assert not up.src_mod and not down.src_mod
    assert [_by_name("n_%d" % n).n for n in (1, 3, 4, 5)] == [1, 3, 4, 5] and _by_name("no_index_list").idx is None
    big = rc.big_grid_case(MI355X_CUS)
    assert big.n > 4 * MI355X_CUS * 3 * 4 and big.plan[:3] == (1, 1, 1) and big.pipes == ("1",)
    st = rc.stride_case()
    assert st.n == 300001 > rc.COPY_GRID_ROWS and st.pipes == ("0",) and st.cols == [(4, 0)]
    assert st.n * 4 * 2 + st.n * 8 < 100e6 and big.n * 516 * 2 < 100e6
    # the ring: rows on both sides of the wrap; a start at and beyond the cap; n == cap; an end exactly on the cap
    w = _by_name("ring_wrap")
    assert w.dst_start < w.dst_cap < w.dst_start + w.n
    assert _by_name("ring_start_at_cap").dst_start == 300 == _by_name("ring_start_at_cap").dst_cap
    assert _by_name("ring_start_beyond_cap").dst_start > 2 * 300
    assert _by_name("ring_n_equals_cap").n == _by_name("ring_n_equals_cap").dst_cap
    e = _by_name("ring_ends_on_cap")
    assert e.dst_start + e.n == e.dst_cap
    # all valid but in the two out-of-range cases, which hold exactly one bad index each
    for c in rc.SMALL_CASES + [big, st]:
        src, dst = c.buffers()
        assert rows_ref.rows_copy_ref([x[1:-1] for x in dst], [x[1:-1] for x in src], **c.args()) == []
    for c, bad in rc.OOB_CASES:
        src, dst = c.buffers()
        assert rows_ref.rows_copy_ref([x[1:-1] for x in dst], [x[1:-1] for x in src], **c.args()) == [bad]
    assert rc.OOB_CASES[0][0].plan[4] == (2,) and 2 not in rc.OOB_CASES[1][0].plan[4]


def test_rows_copy_ref_shift_is_applied_before_the_index_rule():
    src = [np.arange(10)[:, None]]
    dst = [np.full((4, 1), -1)]
    bad = rows_ref.rows_copy_ref(dst, src, np.array([-1, 0, 9, -10]), 0, 0, 0, 4, 1, 2)
    assert dst[0][:, 0].tolist() == [1, 2, -1, 2] and bad == [11]          # -1 + 2 = row 1, not row 9 + 2
    dst = [np.full((3, 1), -1)]
    bad = rows_ref.rows_copy_ref(dst, src, np.array([0, -10, 5]), 0, 0, 0, 3, 1, -1)
    assert dst[0][:, 0].tolist() == [9, -1, 4] and bad == [-11]


# ------------------------------------------------------------------------------------------------- the collector
def _collect_loop(src, shape, id_stride, prob):
    """collect_ref's columns by a plain loop over envs and rows, with replay.rollout_key."""
    from mfrl_amd.replay import rollout_key
    E, G, g, rowcap, V, F, A, ms = shape
    out = {k: [] for k in ("obs", "feat", "act", "prob", "rew", "term", "key")}
    for e in range(E):
        for j in range(min(int(src["counts"][e, g]), rowcap)):
            out["obs"].append(src["view"][e, j])
            out["feat"].append(src["feat"][e, j])
            out["act"].append(src["actions"][e, g, j])
            out["prob"].append(np.array([np.float32(x) for x in src["mean"][e, g, :A]]))
            out["rew"].append(src["rewards"][e, g, j])
            out["term"].append(0 if src["alive"][e, g, j] else 1)
            out["key"].append(rollout_key(e, int(src["stats"][e, 0]), int(src["ids"][e, g, j]), E, id_stride))
    if not prob:
        del out["prob"]
    return out


@pytest.mark.parametrize("shape", rc.COLLECT_SHAPES, ids=str)
@pytest.mark.parametrize("prob", [True, False])
def test_collect_ref_matches_a_plain_loop(shape, prob):
    E, G, g, rowcap, V, F, A, ms = shape
    src = rc.collect_inputs(shape)
    assert (src["counts"][:, g] > rowcap).any() and (E == 1 or (src["counts"][:, g] == 0).any())
    assert set(src["stats"][:, 0].tolist()) == set(rc.EPISODES[:min(E, 3)])
    for e in range(E):
        assert sorted(src["ids"][e].reshape(-1).tolist()) == list(range(G * rowcap))
    res = rows_ref.collect_ref(src, shape, 3, 10 ** 6, G * rowcap, prob=prob)
    want = _collect_loop(src, shape, G * rowcap, prob)
    assert res["fits"] and res["err"] == 0 and res["n"] == 3 + res["count"] == 3 + len(want["key"]) > 3
    assert set(res["cols"]) == set(want)
    for k, v in want.items():
        got = res["cols"][k]
        assert got.tobytes() == np.asarray(v, dtype=got.dtype).reshape(got.shape).tobytes(), k
    assert V >= 1 and V // 4 <= 320 and F <= 64 and A <= ms


def test_collect_shapes_reach_the_limits():
    V = [s[4] for s in rc.COLLECT_SHAPES]
    assert {v & 3 for v in V} == {0, 1, 2, 3} and max(V) == rc.VIEW_MAX == 64 * 4 * 5 + 3 and min(V) == 1
    assert 1280 in V and 1280 // 4 == 64 * 5 and all(s[4] > rc.VIEW_MAX for s in rc.COLLECT_TOO_WIDE)
    assert {v // 4 < 64 for v in V} == {True, False}
    assert max(s[5] for s in rc.COLLECT_SHAPES) == 64 and max(s[6] for s in rc.COLLECT_SHAPES) == 64
    assert any(s[7] > s[6] for s in rc.COLLECT_SHAPES) and any(s[2] > 0 for s in rc.COLLECT_SHAPES)
    # the long lists at the MI355X's CU count (the GPU test sizes them from the device's own)
    assert 40 * 200 == rc.LONG_BEGIN[0] * rc.LONG_BEGIN[3] > 2 * rc.begin_grid_waves(MI355X_CUS, rc.LONG_BEGIN)
    assert rc.begin_grid_waves(MI355X_CUS, rc.LONG_BEGIN) == 4 * 3 * MI355X_CUS
    sh = rc.long_end_shape(MI355X_CUS)
    assert sh[0] * sh[3] > rc.end_grid_lanes(MI355X_CUS, sh) == 256 * 8 * MI355X_CUS
    assert sh[0] * sh[3] < 1.01 * 256 * 8 * MI355X_CUS
    assert sh[0] * sh[3] * (2 * (sh[4] + sh[5]) * 4 + 40) < 100e6


def test_collect_ref_links_match_chain_links_over_three_steps():
    from mfrl_amd.replay import chain_links
    shape = (4, 2, 1, 9, 4, 33, 2, 24)
    E, G, g, rowcap = shape[:4]
    stride = G * rowcap
    steps = rc.three_steps(shape)
    assert steps[2]["stats"][1, 0] == steps[1]["stats"][1, 0] + 1 and steps[1]["stats"][1, 0] == steps[0]["stats"][1, 0]
    assert not np.array_equal(steps[0]["ids"], steps[1]["ids"]) and not np.array_equal(steps[1]["ids"], steps[2]["ids"])
    state, n, errs = rows_ref.links_state(E, stride), 0, []
    for s in steps:
        res = rows_ref.collect_ref(s, shape, n, 10 ** 6, stride, state)
        assert res["n"] == n + res["count"] > n
        n, state = res["n"], res["state"]
        errs.append(res["err"])
    assert errs == [0, 2, 0]
    key = state["key"]
    # the two rows with an id outside [0, stride) start chains of their own; every other row follows chain_links
    first = rows_ref.collect_ref(steps[0], shape, 0, 10 ** 6, stride)["count"]
    rows1, _ = rows_ref.rollout_rows_ref(steps[1]["counts"], g, rowcap)
    odd = [first + int(np.flatnonzero(rows1 == e * rowcap + j)[0]) for e, j in ((0, 0), (2, 1))]    # ids stride and -1
    assert state["prev"][odd].tolist() == [-1, -1] and state["tail"][odd].tolist() == [1, 1]
    keep = np.setdiff1d(np.arange(n), odd)
    prev, tail = chain_links(key[keep])
    assert np.array_equal(np.where(prev >= 0, keep[np.maximum(prev, 0)], -1), state["prev"][keep])
    assert np.array_equal(tail, state["tail"][keep].astype(bool))
    assert (state["prev"] >= 0).sum() > 10                                    # chains do run across the steps
    # env 1's third-step rows link to nothing although `last` still holds their ids' rows of the earlier episode
    third = np.arange(n - res["count"], n)
    env1 = third[(key[third] // stride) % E == 1]
    assert len(env1) and (state["prev"][env1] == -1).all()
    # a step that does not fit changes nothing
    res = rows_ref.collect_ref(steps[0], shape, n, n + 1, stride, state)
    assert not res["fits"] and res["err"] == 1 and res["n"] == n and res["state"] is state and res["cols"] is None


# ------------------------------------------------------------------------------------------------- mean field
@pytest.mark.parametrize("numpy1", [True, False])
def test_mfac_returns_ref_matches_reference_vectors(numpy1):
    fx = np.load(os.path.join(common.GOLDEN, "algo_mfac_returns.npz"))
    offs = np.concatenate([[0], np.cumsum(fx["lens"])]).astype(np.int64)
    got = rows_ref.mfac_returns_ref(fx["rewards"], offs, fx["value"], 0.95, numpy1=numpy1)
    assert got.tobytes() == fx["returns_numpy1" if numpy1 else "returns_nep50"].tobytes()


@pytest.mark.parametrize("numpy1", [True, False])
def test_returns_cases_and_chain_form_agree(numpy1):
    """The episode and chain generators hold what the GPU cases need, and contiguous episodes written as chains give
    the same returns through replay.chain_returns_host."""
    from mfrl_amd.replay import chain_returns_host
    assert rc.COUNTS == (1, 256, 257, 1000) and 0.95 in rc.GAMMAS and float(np.float32(0.95)) != 0.95
    for n_ep in rc.COUNTS:
        rew, offs, val = rc.episodes(n_ep)
        lens = np.diff(offs)
        assert (n_ep < 3 or (lens == 0).any()) and len(val) == n_ep and (n_ep < 3 or (lens > 1).any())
        assert lens[-1] > 1                                  # the last episode is not empty: 257 needs a second workgroup
        prev = np.arange(len(rew), dtype=np.int64) - 1
        prev[offs[:-1][lens > 0]] = -1
        live = np.flatnonzero(lens > 0)
        for gamma in rc.GAMMAS:
            want = rows_ref.mfac_returns_ref(rew, offs, val, gamma, numpy1=numpy1)
            got = chain_returns_host(rew, prev, offs[1:][live] - 1, val[live], gamma, numpy1=numpy1)
            assert got.tobytes() == want.tobytes()
        rew, prev, tails, val = rc.chains(n_ep)
        assert len(tails) == n_ep and prev[tails[0]] == -1 and (prev < np.arange(len(prev))).all()
        assert len(set(tails.tolist())) == n_ep and (n_ep == 1 or (prev >= 0).any())
    rew, prev, tails, val = rc.chains(257, ones=True)
    assert (prev == -1).all() and len(rew) == 257


def test_mean_action_ref_rules():
    acts = np.array([[0, 2, 2, 9], [1, 1, -1, 5], [3, 3, 3, 3]], dtype=np.int32)
    out = rows_ref.mean_action_ref(acts, np.array([3, 7, 0]), 4)
    assert out[0].tolist() == [1 / 3, 0, 2 / 3, 0]                 # the oracle's expression
    assert out[1].tolist() == [0, 0.5, 0, 0]                       # capped at 4 slots; -1 and 5 counted nowhere
    assert np.isnan(out[2]).all()
    assert np.isnan(rows_ref.mean_action_ref(acts, np.array([-2, -1, 0]), 4)).all()
    for n_action in (1, 2, 21, 255, 256):
        for rowcap in (1, 255, 256, 257, 1000):
            for over in (False, True):
                a, c = rc.mean_action_inputs(n_action, rowcap, over=over)
                assert a.shape == (len(c) + 1, rowcap) and c[:3].tolist() == [0, 1, rowcap]
                assert ((a < 0) | (a >= n_action)).any() or rowcap == 1
                assert over == bool((c > rowcap).any()) and c.max() <= 2 * rowcap
                if over:                   # a reader without the cap would give another result, inside the buffer
                    flat = a.reshape(-1)
                    b = int(np.flatnonzero(c > rowcap)[0])
                    uncapped = np.bincount(flat[b * rowcap:b * rowcap + c[b]].clip(-1, n_action) + 1,
                                           minlength=n_action + 2)[1:-1] / c[b]
                    assert b * rowcap + c[b] <= flat.size
                    assert not np.array_equal(uncapped, rows_ref.mean_action_ref(a[:-1], c, n_action)[b])


def test_mfq_target_ref_rules():
    for A in (1, 2, 21, 33):
        rows = rc.mfq_rows(A)
        am = {k: int(np.argmax(v)) for k, v in rows.items()}
        assert am["nan_first"] == 0 and am["nan_last"] == A - 1 and am["all_-inf"] == 0 and am["all_equal"] == 0
        assert am["max_last"] == A - 1
        if A >= 2:
            assert am["two_nans"] == 0 and np.isnan(rows["two_nans"][[0, -1]]).all()
            assert am["-0_then_+0"] == 0 and am["+0_then_-0"] == 0 and am["nan_after_inf"] == A - 1
            assert np.isinf(rows["nan_after_inf"][0])
        if A >= 3:
            assert am["two_nans_inside"] == 1
        for M in (1, 255, 256, 257):
            eq, tq, r, done = rc.mfq_inputs(M, A)
            assert M < 255 or set(done.tolist()) == {0, 1, 2, 255}
            assert (done[:len(rows)] == 0).all() and (M < 255 or (eq[:len(rows)].tobytes() ==
                                                                  np.stack(list(rows.values())).tobytes()))
            if M >= 255:                   # t_q tells the hand-built rows' choices apart
                assert all(len(set(tq[m].tolist())) == A for m in range(len(rows)))
            out = rows_ref.mfq_target_ref(eq, tq, r, done, 0.95)
            assert out.dtype == np.float64 and np.isfinite(out).all()
            assert out[done != 0].tobytes() == r[done != 0].astype(np.float64).tobytes()      # any non-zero byte is done
            want = r.astype(np.float64) + ((done == 0) * tq[np.arange(M), np.argmax(eq, 1)].astype(np.float64)) * 0.95
            assert out.tobytes() == want.tobytes()
