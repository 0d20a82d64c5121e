"""The trace / sweep variants of the fused MF-Q kernels and the Metropolis kernel (csrc/ising_kernels.hip
k_ising_mfq<.., true>, k_ising_mfq_big<.., true>; csrc/ising_mc_kernels.hip k_ising_mc), bit for bit against the
numpy restatements of tests/ising_trace_ref.py, which tests/test_ising_sweep_cpu.py pins to episodes recorded from
the reference scenario.

Shapes (the smallest at which each branch can go wrong):
    N 16,   view 1, K 4   one partial wave
    N 100,  view 1, K 4   two waves, the second partial: the cross-wave mse order
    N 36,   view 2, K 8   the general target formula, the <16> instantiation
    N 1156, view 1, K 4   34 x 34: k_ising_mfq_big, some lanes own two agents; even side, so k_ising_mc takes it too
T = 200 with decay_gap 7, decay_rate 0.8 (the clamp is reached), act_rate 1.0 and 0.5.

The device exp() is not bit-pinned, so every restatement-compared case first asserts that no draw came within GAP
of its threshold (as tests/test_ising_shapes_gpu.py does)."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import common
import ising_trace_ref as ref

pytestmark = pytest.mark.gpu

GAP = 1e-12
SHAPES = [(16, 1, 4), (100, 1, 4), (36, 2, 8), (1156, 1, 4)]
T, DG, DR = 200, 7, 0.8
ANNEAL = dict(decay_rate=DR, decay_gap=DG)
ARMS = [(1.0, 0.02), (0.5, 0.8)]                       # (act_rate, temperature)


@functools.lru_cache(maxsize=None)
def restated(n, view, tau, act, seed, steps=T):
    """One restated episode, computed once and shared (never modified)."""
    out = ref.trace(n, tau, steps, act_rate=act, seed=seed, view=view, **ANNEAL)
    print("N %d view %d tau %g act %g seed %d: min|u-c0| = %.3e, %d steps" % (n, view, tau, act, seed, out["min_gap"],
                                                                            out["steps"]))
    assert out["min_gap"] > GAP
    return out


def same_run(a, b, keys=("q", "order", "n_up", "steps", "spins"), rows=None):
    for k in keys:
        x, y = a[k], b[k]
        if rows is not None and k in ("order", "n_up"):
            for r in range(len(rows)):
                assert x[r, :rows[r]].tobytes() == y[r, :rows[r]].tobytes(), (k, r)
        else:
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


def same_as_restated(got, r, want, tag):
    S = want["steps"]
    assert int(got["steps"][r]) == S, tag
    for k in ("order", "rsum", "mse"):
        assert got[k][r, :S].tobytes() == want[k].tobytes(), (tag, k)
        assert np.isnan(got[k][r, S:]).all(), (tag, k, "rows past the stop step")
    np.testing.assert_array_equal(got["n_up"][r, :S], want["n_up"], err_msg=str(tag))
    assert got["q"][r].tobytes() == want["q"].tobytes(), tag
    np.testing.assert_array_equal(got["spins"][r], want["spins"], err_msg=str(tag))


# ------------------------------------------------------------------ 1. unchanged without temps
@pytest.mark.parametrize("n,view,K", SHAPES)
@pytest.mark.parametrize("act,tau", ARMS)
def test_trace_variant_leaves_the_episode_unchanged(n, view, K, act, tau):
    """temps null and temps all equal to tau give today's q, order, n_up, steps and spins: host draws, the device's
    numpy stream, Philox."""
    from mfrl_amd.ising import IsingLattice, reference_stream
    R, seed = 2, 13
    lat = IsingLattice(n, R, view=view)
    assert lat.K == K
    streams = [reference_stream(seed + r, n, T, act) for r in range(R)]
    spins0 = np.stack([s[0] for s in streams])
    u = np.stack([s[1] for s in streams])
    mask = np.stack([s[2] for s in streams]) if act != 1.0 else None
    same = np.full(R, tau)
    # host draws
    lat.set_spins(spins0)
    base = lat.run_mfq(T, tau, u=u, mask=mask, **ANNEAL)
    lat.set_spins(spins0)
    a = lat.run_mfq_trace(T, tau, u=u, mask=mask, **ANNEAL)
    lat.set_spins(spins0)
    b = lat.run_mfq_trace(T, 77.0, u=u, mask=mask, temps=same, **ANNEAL)
    rows = [int(s) for s in base["steps"]]
    same_run(a, base, rows=rows)
    same_run(b, base, rows=rows)
    assert a["rsum"].tobytes() == b["rsum"].tobytes() and a["mse"].tobytes() == b["mse"].tobytes()
    # the device's numpy stream: today's run_mfq_stream against the sweep with one stream per replica
    base_s = lat.run_mfq_stream(T, tau, act_rate=act, seed=seed, **ANNEAL)[0]
    base_s["spins"] = lat.get_spins()
    c = lat.run_mfq_sweep(T, same, act_rate=act, seed=seed, **ANNEAL)
    same_run(c, base_s, rows=rows)
    same_run(c, base, rows=rows)                              # (and the host stream is the device stream)
    assert c["rsum"].tobytes() == a["rsum"].tobytes() and c["mse"].tobytes() == a["mse"].tobytes()
    # Philox (act_rate 1 only: no act_group draws in that mode)
    if act == 1.0:
        lat.set_spins(spins0)
        base_p = lat.run_mfq(T, tau, seed=99, **ANNEAL)
        lat.set_spins(spins0)
        d = lat.run_mfq_trace(T, tau, seed=99, **ANNEAL)
        lat.set_spins(spins0)
        e = lat.run_mfq_trace(T, 77.0, seed=99, temps=same, **ANNEAL)
        rows_p = [int(s) for s in base_p["steps"]]
        same_run(d, base_p, rows=rows_p)
        same_run(e, base_p, rows=rows_p)
        assert d["q"].tobytes() != base["q"].tobytes()


# ------------------------------------------------------------------ 2. restatement parity
@pytest.mark.parametrize("n,view,K", SHAPES)
@pytest.mark.parametrize("act,tau", ARMS)
def test_trace_equals_restatement(n, view, K, act, tau):
    """rsum and mse (and the episode) of two replicas of one sweep launch against the restatement, bit for bit."""
    from mfrl_amd.ising import IsingLattice
    R, seed = 2, 13
    wants = [restated(n, view, tau, act, seed + r) for r in range(R)]
    for w in wants:
        assert w["mse"].max() > 0.0 and len(np.unique(w["rsum"])) > 1
    lat = IsingLattice(n, R, view=view)
    got = lat.run_mfq_sweep(T, np.full(R, tau), act_rate=act, seed=seed, **ANNEAL)
    for r in range(R):
        same_as_restated(got, r, wants[r], (n, view, act, r))


@pytest.mark.parametrize("name", ["n16_t08", "n16_t002_act05", "n100_t002", "n100_t08_act05"])
def test_trace_against_recorded_reference_episode(name):
    """The device against the episode recorded from the reference scenario under the script's loop: everything bit
    for bit but the mse, whose terms the script adds in act_group order -- within 2 N 2^-53 mse_ref, the first-order
    bound for two summation orders of N non-negative float64 terms."""
    from mfrl_amd.ising import IsingLattice
    fx = np.load(os.path.join(common.GOLDEN, "ising_sweep_%s.npz" % name))
    n, S = int(fx["arg_n_agents"]), int(fx["stop"])
    lat = IsingLattice(n, 1)
    got = lat.run_mfq_sweep(int(fx["arg_steps"]), [float(fx["arg_temperature"])], lr=float(fx["arg_lr"]),
                            decay_rate=float(fx["arg_decay_rate"]), decay_gap=int(fx["arg_decay_gap"]),
                            act_rate=float(fx["arg_act_rate"]), seed=int(fx["arg_seed"]))
    assert int(got["steps"][0]) == S
    assert got["rsum"][0, :S].tobytes() == fx["reward_sum"].tobytes()
    assert got["order"][0, :S].tobytes() == fx["order"].tobytes()
    assert got["q"][0].tobytes() == fx["q_final"].tobytes()
    bound = 2.0 * n * 2.0 ** -53 * fx["mse"]
    err = np.abs(got["mse"][0, :S] - fx["mse"])
    print("%s: max |mse - mse_ref| / bound = %.3g" % (name, np.max(err / np.where(bound > 0, bound, 1.0))))
    assert (err <= bound).all()


# ------------------------------------------------------------------ 3, 4. the sweep equals single runs
def test_sweep_equals_single_runs_and_feels_its_temperatures():
    """R = 6: three temperatures x two seeds sharing two streams through stream_of.  Replica (g, s) is the single
    run at temps[g] on seed seed0 + s, q included; some replicas stop early, some run to the cap, and rows past the
    stop step stay NaN.  The restatement first shows that the temperatures matter: a kernel that ignored temps (or
    stream_of) could not pass."""
    from mfrl_amd.ising import IsingLattice
    n, steps, seed0 = 16, 600, 13
    temps, S = [0.02, 0.8, 2.5], 2
    wants = {(g, s): restated(n, 1, temps[g], 1.0, seed0 + s, steps) for g in range(3) for s in range(S)}
    stops = [w["steps"] for w in wants.values()]
    assert min(stops) < steps and max(stops) == steps, stops
    for s in range(S):                                       # swapping two replicas' temperatures changes their rows
        for g, h in ((0, 1), (1, 2), (0, 2)):
            k = min(wants[g, s]["steps"], wants[h, s]["steps"])
            assert wants[g, s]["order"][:k].tobytes() != wants[h, s]["order"][:k].tobytes()
    for g in range(3):                                       # and so does swapping their streams
        k = min(wants[g, 0]["steps"], wants[g, 1]["steps"])
        assert wants[g, 0]["order"][:k].tobytes() != wants[g, 1]["order"][:k].tobytes()
    lat = IsingLattice(n, 6)
    got = lat.run_mfq_sweep(steps, np.repeat(temps, S), np.tile(np.arange(S), 3), S, seed=seed0, **ANNEAL)
    one = IsingLattice(n, 1)
    for g in range(3):
        for s in range(S):
            r = g * S + s
            same_as_restated(got, r, wants[g, s], (g, s))
            single = one.run_mfq_stream(steps, temps[g], seed=seed0 + s, **ANNEAL)[0]
            k = int(single["steps"][0])
            assert int(got["steps"][r]) == k
            assert got["q"][r].tobytes() == single["q"][0].tobytes()
            assert got["order"][r, :k].tobytes() == single["order"][0, :k].tobytes()
            np.testing.assert_array_equal(got["n_up"][r, :k], single["n_up"][0, :k])
            np.testing.assert_array_equal(got["spins"][r], one.get_spins()[0])


def test_sweep_function_layout():
    """sweep(): temperature-major [n_temps][n_seeds][...], NaN / -1 past the stop step, the Metropolis arm beside."""
    from mfrl_amd.ising import sweep
    n, steps = 16, 600
    temps = [0.02, 2.5]
    out = sweep(n, temps, 2, steps, seed=13, mcmc_sweeps=10, **ANNEAL)
    assert out["order"].shape == out["rsum"].shape == out["mse"].shape == out["n_up"].shape == (2, 2, steps)
    assert out["q"].shape == (2, 2, n, 5, 2) and out["steps"].shape == (2, 2) and out["mc_order"].shape == (2, 2, 10)
    for g in range(2):
        for s in range(2):
            w = restated(n, 1, temps[g], 1.0, 13 + s, steps)
            k = w["steps"]
            assert int(out["steps"][g, s]) == k
            assert out["mse"][g, s, :k].tobytes() == w["mse"].tobytes()
            assert np.isnan(out["order"][g, s, k:]).all() and (out["n_up"][g, s, k:] == -1).all()
            assert out["order_final"][g, s] == w["order"][-1]
            m = ref.metropolis(n, 10, ref.metropolis_table(temps[g]), seed=0, rep=g * 2 + s)
            assert out["mc_order"][g, s].tobytes() == m["order"].tobytes()
    assert out["steps"][0].max() < steps


def test_sweep_abi_refusals():
    from mfrl_amd.ising import IsingLattice
    lat = IsingLattice(16, 3)
    for temps in ([0.8, 0.0, 0.8], [0.8, float("nan"), 0.8], [float("inf"), 0.8, 0.8], [0.8, 0.8, -2.0]):
        with pytest.raises(RuntimeError, match="temperature"):
            lat.run_mfq_sweep(10, temps)
    for so, ns in (([0, 1, 2], 2), ([0, -1, 0], 2)):
        with pytest.raises(RuntimeError, match="stream_of"):
            lat.run_mfq_sweep(10, [0.8] * 3, so, ns)
    with pytest.raises(RuntimeError, match="n_streams"):     # no stream_of: one stream per replica of the handle
        lat.run_mfq_sweep(10, [0.8] * 3, None, 2)
    with pytest.raises(ValueError):                          # R differing from the handle's
        lat.run_mfq_sweep(10, [0.8] * 4)
    with pytest.raises(RuntimeError, match="temperature"):
        lat.run_mfq_trace(10, 0.8, temps=[0.8, 0.0, 0.8])


# ------------------------------------------------------------------ 5. Metropolis
@pytest.mark.parametrize("n", [16, 100, 1156])
def test_metropolis_equals_restatement(n):
    from mfrl_amd.ising import IsingLattice, metropolis_table
    R, sweeps, seed = 4, 50, 11
    acc = np.stack([metropolis_table(t) for t in (0.4, 1.0, 1.5, 4.0)])
    spins0 = np.random.RandomState(n).randint(0, 2, size=(R, n)).astype(np.uint8)
    spins0[3] = 1
    lat = IsingLattice(n, R)
    lat.set_spins(spins0)
    got = lat.run_mc(sweeps, acc, seed)
    finals = []
    for r in range(R):
        want = ref.metropolis(n, sweeps, acc[r], seed=seed, rep=r, spins0=spins0[r])
        assert got["order"][r].tobytes() == want["order"].tobytes(), r
        np.testing.assert_array_equal(got["n_up"][r], want["n_up"])
        np.testing.assert_array_equal(got["spins"][r], want["spins"])
        finals.append(want["n_up"][-1])
    assert not np.array_equal(got["spins"], spins0) and len(set(finals)) > 1


@pytest.mark.parametrize("n,view", [(25, 1), (16, 2), (36, 2)])
def test_metropolis_refuses_other_shapes(n, view):
    """Odd side, view 2, and the N 36 / view 2 shape: python refuses, and so does the ABI itself."""
    from mfrl_amd import lib
    from mfrl_amd.ising import IsingLattice
    lat = IsingLattice(n, 1, view=view)
    with pytest.raises(ValueError):
        lat.run_mc(5, np.ones(5))
    acc, order, nup = np.ones(5), np.zeros(5), np.zeros(5, np.int32)
    P = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    before = lat.get_spins()
    assert lib().mfx_ising_mc_run(lat._h, 5, P(acc), ctypes.c_uint(0), P(order), P(nup)) == -1
    assert b"ising mc" in lib().mfx_last_error()
    np.testing.assert_array_equal(lat.get_spins(), before)


# ------------------------------------------------------------------ 6. the command line
def test_cli_writes_the_sweep(tmp_path):
    from mfrl_amd.ising import sweep
    out_dir = str(tmp_path / "figs")
    env = dict(os.environ, PYTHONPATH=common.PY_DIR)
    run = subprocess.run([sys.executable, "-m", "mfrl_amd.main_MFQ_Ising", "-n", "16", "-t", "0.5", "2.0", "--seeds",
                          "2", "-ts", "120", "--mcmc", "20", "--out", out_dir], capture_output=True, text=True,
                         env=env, timeout=120)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("T = 0.500000: MF-Q Order = ") and "MCMC Order = " in lines[1]
    got = np.load(os.path.join(out_dir, "sweep.npz"))
    want = sweep(16, [0.5, 2.0], 2, 120, mcmc_sweeps=20)
    assert sorted(got.files) == sorted(want)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)        # (NaN rows equal NaN rows)
    assert "%f" % want["order_final"][0].mean() in lines[0] and "%f" % want["mc_order_final"][1].mean() in lines[1]


def test_cli_single_run_prints_the_scripts_lines(tmp_path, capsys):
    """One temperature, one seed: the script's "+++" marks, per-step lines and "Episode:" line (:138-169), figures
    from the restatement."""
    from mfrl_amd import main_MFQ_Ising as cli
    n, steps = 16, 30
    w = ref.trace(n, 0.8, steps, seed=13)
    assert w["min_gap"] > GAP and w["steps"] == steps
    want, max_order, at, ups_at = [], 0.0, 0, 0
    for t in range(steps):
        if w["order"][t] > max_order:
            max_order, at, ups_at = w["order"][t], t, int(w["n_up"][t])
            want.append("+++++++++++++++++++++++++++++")
        want.append('E: %d/%d, reward = %f, mse = %f, Order = %f, Up = %d, Down = %d' %
                    (0, t, w["rsum"][t], w["mse"][t], w["order"][t], w["n_up"][t], n - w["n_up"][t]))
    want.append('Episode: %d, MaxO = %f at %d (%d/%d)' % (0, max_order, at, ups_at, n - ups_at))
    assert cli.main(["-n", str(n), "-t", "0.8", "-ts", str(steps), "--out", str(tmp_path)]) == 0
    assert capsys.readouterr().out.splitlines() == want
    assert os.path.exists(os.path.join(str(tmp_path), "sweep.npz"))
