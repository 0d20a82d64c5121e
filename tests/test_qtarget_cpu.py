"""The opt-in Boltzmann mean-field value target on the CPU: the numpy restatement tests/qtarget_ref.py in
its two limits against the reference-pinned fixture, on non-finite rows, and the Python surface refusing what it
should (no GPU)."""
import os

import numpy as np
import pytest

import common
import qsample_ref as qs
import qtarget_ref as qt

GAMMA = 0.95
LOW_T = 2.5e-5
FINITE_BATCHES = (0, 2, 3)        # b1 holds the NaN / 1e30 / tie rows


def fixture():
    return np.load(os.path.join(common.GOLDEN, "algo_mfq_target.npz"))


def batch(fx, b):
    return [fx["b%d_%s" % (b, k)] for k in ("eq", "tq", "r", "done")]


def seq_mean(t_q):
    """The sequential float64 mean of each row, in ascending action order."""
    out = np.zeros(len(t_q))
    for i, row in enumerate(np.asarray(t_q, dtype=np.float32)):
        s = 0.0
        for x in row:
            s += float(x)
        out[i] = s / float(len(row))
    return out


def test_low_temperature_limit_is_the_max_rule():
    """192 finite rows without tied maxima: at T = 2.5e-5 every non-maximal weight underflows to exactly 0 (the
    smallest argmax gap 0.003446 gives an exponent of -137.8; float32 expf reaches 0 near -103.3), so v = t_q[argmax]
    exactly and the target is the reference's, bit for bit."""
    fx = fixture()
    gaps = []
    for b in FINITE_BATCHES:
        eq, tq, r, done = batch(fx, b)
        assert np.isfinite(eq).all() and np.isfinite(tq).all()
        s = np.sort(eq, axis=1)
        gaps.append(float((s[:, -1] - s[:, -2]).min()))
        w = qt.weights(eq, LOW_T)
        assert ((w == 0) | (w == 1)).all() and (w.sum(1) == 1).all()
        assert (np.argmax(w, axis=1) == np.argmax(eq, axis=1)).all()
        got = qt.target(eq, tq, r, done, GAMMA, LOW_T)
        assert got.dtype == np.float64 and got.tobytes() == fx["b%d_target" % b].tobytes(), b
    assert min(gaps) > 0.0034 and min(gaps) / LOW_T > 104.0


def test_high_temperature_limit_is_the_mean():
    """At T = 1e30 every weight is exactly 1 and v is the sequential float64 mean of t_q."""
    fx = fixture()
    for b in FINITE_BATCHES:
        eq, tq, r, done = batch(fx, b)
        w = qt.weights(eq, 1e30)
        assert (w == 1).all()
        want = r.astype(np.float64) + ((1.0 - done.astype(np.float64)) * seq_mean(tq)) * GAMMA
        assert qt.target(eq, tq, r, done, GAMMA, 1e30).tobytes() == want.tobytes(), b
    eq, tq, r, done = batch(fx, 0)
    assert np.abs(qt.target(eq, tq, r, done, GAMMA, 1e30) - fx["b0_target"]).max() > 0.1      # (and not the max rule)


def test_non_finite_rows_follow_the_acting_policy():
    nan, inf = np.nan, np.inf
    eq = np.array([[0.0, nan, 2.0, 1.0], [nan, nan, nan, nan], [0.0, inf, inf, 1.0], [-inf, -inf, -inf, -inf],
                   [nan, -inf, -inf, 0.5], [nan, -inf, -inf, -inf], [1.0, 3.0, 3.0, 2.0]], dtype=np.float32)
    tq = np.arange(28, dtype=np.float32).reshape(7, 4) + 0.5
    r = np.linspace(-1, 1, 7).astype(np.float32)
    done = np.array([0, 0, 0, 0, 1, 0, 0], dtype=np.uint8)
    greedy = [2, 0, 1, 0, 3, 1]
    for T in (0.5, 1e-3, 1e30):
        w = qt.weights(eq, T)
        for i, g in enumerate(greedy):
            assert list(w[i]) == [1.0 if a == g else 0.0 for a in range(4)], (T, i)
        got = qt.target(eq, tq, r, done, GAMMA, T)
        for i, g in enumerate(greedy):
            want = float(r[i]) + ((1.0 - float(done[i] != 0)) * float(tq[i, g])) * GAMMA
            assert got[i] == want, (T, i)
    # the tied finite row: both maxima weigh 1, the rest expf(-1 / T)
    w = qt.weights(eq, 0.5)[6].astype(np.float64)
    assert w[1] == w[2] == 1.0 and 0 < w[0] < w[3] < 1
    assert qt.target(eq, tq, r, done, GAMMA, 0.5)[6] == float(r[6]) + (w @ tq[6].astype(np.float64) / w.sum()) * GAMMA
    # the max rule differs on row 0: np.argmax lets the first NaN win (index 1); the acting policy never takes a NaN
    assert int(np.argmax(eq[0])) == 1 and greedy[0] == 2
    # the fixture's NaN / 1e30 / tie batch: non-finite rows are one-hot at the greedy action, whatever T
    fx = fixture()
    eq1 = fx["b1_eq"]
    bad = ~qs.finite_rows(eq1)
    assert bad.any() and not bad.all()
    w1 = qt.weights(eq1, 0.1)
    hot = np.zeros_like(w1[bad])
    hot[np.arange(len(hot)), qs.greedy(eq1[bad])] = 1.0
    assert w1[bad].tobytes() == hot.tobytes()
    # a done flag is any non-zero byte
    a = qt.target(eq[6:], tq[6:], r[6:], np.array([255], dtype=np.uint8), GAMMA, 0.5)
    assert a[0] == float(r[6])


def test_refusals():
    import torch
    from mfrl_amd import mf
    from mfrl_amd.algo.base import ValueNet
    rs = np.random.RandomState(0)
    for A in (1, 33):
        with pytest.raises(ValueError):
            qt.weights(rs.randn(4, A).astype(np.float32), 0.1)
    for T in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            qt.target(rs.randn(4, 5), rs.randn(4, 5), rs.randn(4), np.zeros(4), GAMMA, T)
    # the wrapper refuses before it reaches the library
    f = lambda *s: torch.zeros(*s, dtype=torch.float32)
    ok = dict(e_q=f(4, 5), t_q=f(4, 5), rewards=f(4), dones=torch.zeros(4, dtype=torch.uint8), gamma=GAMMA, temperature=0.1)
    for key, bad, err in (("e_q", f(4, 5).double(), TypeError), ("t_q", f(4, 5).half(), TypeError),
                          ("rewards", f(4).double(), TypeError), ("t_q", f(4, 6), ValueError), ("rewards", f(5), ValueError),
                          ("dones", torch.zeros(3, dtype=torch.uint8), ValueError), ("temperature", 0.0, ValueError),
                          ("temperature", -1.0, ValueError), ("temperature", float("inf"), ValueError),
                          ("temperature", float("nan"), ValueError), ("temperature", f(1).double(), TypeError),
                          ("temperature", f(2), ValueError), ("temperature", f(1), ValueError)):     # (f(1): not on the device)
        with pytest.raises(err):
            mf.mfq_target_boltzmann(**dict(ok, **{key: bad}))
    for A in (1, 33):
        with pytest.raises(ValueError):
            mf.mfq_target_boltzmann(**dict(ok, e_q=f(4, A), t_q=f(4, A)))
    # ValueNet.target_rule
    assert ValueNet.target_rule.fget(ValueNet) == "max" and ValueNet.target_temperature is None
    m = ValueNet.__new__(ValueNet)
    m._graph = "a captured graph"
    m.target_rule = "max"
    assert m._graph == "a captured graph"                      # unchanged rule: the graph stays
    m.target_rule = "boltzmann"
    assert m.target_rule == "boltzmann" and m._graph is None and ValueNet._target_rule == "max"
    for bad in ("soft", "", None, "Boltzmann", 1):
        with pytest.raises(ValueError):
            m.target_rule = bad
    assert m.target_rule == "boltzmann"
    m.temperature = 0.25
    assert m._target_T() == 0.25
    m.target_temperature = 0.5
    assert m._target_T() == 0.5
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        m.target_temperature = bad
        with pytest.raises(ValueError):
            m._target_T()


@pytest.mark.parametrize("argv", [
    ["--algo", "mfac", "--target", "boltzmann"],
    ["--algo", "ac", "--target", "boltzmann"],
    ["--algo", "mfq", "--target", "soft"],
])
def test_train_battle_refuses(argv, capsys):
    from mfrl_amd import train_battle
    with pytest.raises(SystemExit) as ex:
        train_battle.main(argv)
    assert ex.value.code == 2
    assert "--target" in capsys.readouterr().err
