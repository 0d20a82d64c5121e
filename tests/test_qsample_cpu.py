"""The Boltzmann draw of the Q models' opt-in acting mode (csrc/qsample.h) on the CPU: the numpy
restatement (tests/qsample_ref.py) against the actor-critic draw's hash, on hand-made weight rows, and in the
frequency check the GPU test repeats on the kernel; the Python surface refusing what it should (no GPU)."""
import numpy as np
import pytest

import acnet_ref
import qsample_ref as qs


def test_uniform_is_the_actor_critic_uniform():
    table = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (4242, 7, 1, 131),
             (0xFFFFFFFF, 0xFFFFFFFF, 1, 0x7FFFFFFF), (123456789, 1000, 0, 65535), (3, 99, 1, 8 * 324 + 17)]
    for seed, step, g, row in table:
        rows = np.array([row, row + 1, row + 2], dtype=np.int64) & 0x7FFFFFFF
        got, want = qs.uniforms(seed, step, g, rows), acnet_ref.uniforms(seed, step, g, rows)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (seed, step, g, row)
        assert ((got >= 0) & (got < 1)).all()
    u = qs.uniforms(5, 1, 0, np.arange(4096))
    assert len(np.unique(u)) > 4000 and 0.45 < u.mean() < 0.55


def test_draw_on_hand_made_rows():
    f = np.float32
    top = f(1.0) - f(2.0 ** -24)                       # the largest uniform the hash gives
    one_hot = np.array([[0, 0, 1, 0, 0]], dtype=f)
    for u in (0.0, 0.3, top):
        assert qs.draw(one_hot, [u])[0] == 2
    eq = np.ones((1, 4), dtype=f)
    assert [int(qs.draw(eq, [u])[0]) for u in (0.0, 0.2499, 0.25, 0.5, 0.74, 0.75, top)] == [0, 0, 1, 2, 2, 3, 3]
    tail = np.array([[0.5, 0.5, 0, 0, 0]], dtype=f)    # a zero tail is never drawn: run reaches tot at action 1
    assert [int(qs.draw(tail, [u])[0]) for u in (0.0, 0.49, 0.5, top)] == [0, 0, 1, 1]
    # u at the very top: the last action with weight, A - 1 when every weight is positive -- the threshold
    # (1 - 2^-24) tot rounds below tot for every float32 tot, so the last running sum always exceeds it ...
    rng = np.random.RandomState(1)
    w = (rng.rand(64, 21) + 0.01).astype(f)
    assert (qs.draw(w, np.full(64, top, dtype=f)) == 20).all()
    # ... and where no running sum exceeds the threshold (u = 1, which the hash cannot give) the rule answers A - 1
    assert qs.draw(np.array([[1.0, 0.0, 0.0]], dtype=f), [f(1.0)])[0] == 2
    assert qs.draw(np.zeros((1, 3), dtype=f), [f(0.0)])[0] == 2


def test_non_finite_rows_take_the_greedy_action():
    nan, inf = np.nan, np.inf
    q = np.array([[0.0, nan, 2.0, 1.0], [nan, nan, nan, nan], [0.0, inf, inf, 1.0], [-inf, -inf, -inf, -inf],
                  [nan, -inf, -inf, 0.5], [nan, -inf, -inf, -inf], [1.0, 3.0, 3.0, 2.0]], dtype=np.float32)
    assert list(qs.greedy(q)) == [2, 0, 1, 0, 3, 1, 1]
    fin = qs.finite_rows(q)
    assert list(fin) == [False] * 6 + [True]
    for step in range(20):
        act = qs.sample(q, 0.5, 9, step, 0, np.arange(len(q)))
        assert list(act[:6]) == [2, 0, 1, 0, 3, 1]
        assert act[6] in (0, 1, 2, 3)


def test_weights_follow_the_softmax():
    rng = np.random.RandomState(0)
    for T in (1e-3, 0.1, 1.0):
        q = (rng.randn(200, 21) * 3 * T).astype(np.float32)
        w = qs.weights(q, T).astype(np.float64)
        p = w / w.sum(1, keepdims=True)
        assert np.abs(p - qs.softmax64(q, T)).max() <= 1e-5
    # past (m - q) / T > 104 the f32 weight is exactly 0
    q = np.array([[0.0, -104.5, -200.0, -1e30]], dtype=np.float32)
    assert list(qs.weights(q, 1.0)[0]) == [1.0, 0.0, 0.0, 0.0]


FREQ_Q = (np.arange(21, dtype=np.float64) * 8 % 21 * (3.0 / 20.0)).astype(np.float32)[None, :]   # gaps spread over 0..3
FREQ_N = 65536


def freq_check(actions, seed):
    """|c_a - N p_a| <= 5 sqrt(N p_a (1 - p_a)) + 1 for every action (the + 1: the 24-bit granularity of u)."""
    p = qs.softmax64(FREQ_Q, 1.0)[0]
    c = np.bincount(actions, minlength=21).astype(np.float64)
    assert c.sum() == FREQ_N
    dev = np.abs(c - FREQ_N * p)
    bound = 5.0 * np.sqrt(FREQ_N * p * (1.0 - p)) + 1.0
    assert (dev <= bound).all(), (seed, np.round(dev / bound, 3))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_frequencies_follow_the_softmax(seed):
    assert FREQ_Q.min() == 0.0 and FREQ_Q.max() == 3.0 and len(np.unique(FREQ_Q)) == 21
    q = np.repeat(FREQ_Q, FREQ_N, axis=0)
    freq_check(qs.sample(q, 1.0, seed, 0, 0, np.arange(FREQ_N)), seed)


# ------------------------------------------------------------------------------------------------- the surface
def test_explore_setter_validates():
    from mfrl_amd.algo.base import ValueNet, check_temperature
    assert ValueNet.explore.fget(ValueNet) == "greedy"          # the class default
    m = ValueNet.__new__(ValueNet)
    assert m.explore == "greedy"
    m.explore = "boltzmann"
    assert m.explore == "boltzmann" and ValueNet._explore == "greedy"
    m.explore = "greedy"
    for bad in ("eps", "", None, "Boltzmann", 1):
        with pytest.raises(ValueError):
            m.explore = bad
    assert m.explore == "greedy"
    assert check_temperature(0.5) == 0.5
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            check_temperature(bad)


@pytest.mark.parametrize("argv,msg", [
    (["--algo", "ac", "--explore", "boltzmann"], "--explore"),
    (["--algo", "mfac", "--envs", "4", "--rollout_episodes", "--explore", "boltzmann"], "--explore"),
    (["--algo", "mfq", "--explore", "softmax"], "--explore"),
])
def test_train_battle_refuses(argv, msg, capsys):
    from mfrl_amd import train_battle
    with pytest.raises(SystemExit) as ex:
        train_battle.main(argv)
    assert ex.value.code == 2
    assert msg in capsys.readouterr().err


@pytest.mark.parametrize("argv,msg", [
    (["--algo", "mfac", "--oppo", "ac", "--untrained", "--explore", "boltzmann"], "--explore"),
    (["--algo", "mfq", "--untrained", "--explore", "softmax"], "--explore"),
    (["--algo", "mfq", "--untrained", "--temperature", "0.5"], "--temperature"),
    (["--algo", "mfq", "--untrained", "--explore", "boltzmann", "--temperature", "0"], "--temperature"),
    (["--algo", "mfq", "--untrained", "--explore", "boltzmann", "--temperature", "-1"], "--temperature"),
    (["--algo", "mfq", "--untrained", "--explore", "boltzmann", "--temperature", "nan"], "--temperature"),
    (["--algo", "mfq", "--untrained", "--explore", "boltzmann", "--temperature", "inf"], "--temperature"),
])
def test_battle_eval_refuses(argv, msg, capsys):
    from mfrl_amd import battle_eval
    with pytest.raises(SystemExit) as ex:
        battle_eval.main(argv)
    assert ex.value.code == 2
    assert msg in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------- the off-shape cases
def test_shape_cases_are_decisive():
    """The precondition of tests/test_qsample_shapes_gpu.py, from the references alone: at each case's temperature at
    least MIN_ROWS of the 131 reference rows do not draw the argmax, and at A = 32 at least MIN_ROWS draw an action
    >= 24 (the lanes A = 21 leaves empty); the temperature is the first of the list that gives both."""
    import qsample_cases as qc
    assert len(qc.CASES) == 18 and {c[:2] for c in qc.CASES} == set(qc.FA)
    for case in qc.CASES:
        T = qc.temperature(case)
        off, high = qc.decisive(case, T)
        print("%s: T %g, %d rows off the argmax, %d rows >= %d" % (qc.case_id(case), T, off, high, qc.HIGH))
        assert off >= qc.MIN_ROWS, (case, off)
        assert case[1] <= qc.HIGH or high >= qc.MIN_ROWS, (case, high)
        assert np.isfinite(qc.reference_q(case)).all()
