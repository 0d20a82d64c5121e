"""The numpy restatements of the Ising trace / sweep / Metropolis contract (tests/ising_trace_ref.py) against the
episodes recorded from the reference scenario (tests/golden/ising_sweep_*.npz, make_ising_sweep_fixtures.py), and
the refusals of sweep() and the command line.  No GPU."""
import glob
import os

import numpy as np
import pytest

import common
import ising_trace_ref as ref

FIXTURES = sorted(os.path.basename(p)[len("ising_sweep_"):-len(".npz")]
                  for p in glob.glob(os.path.join(common.GOLDEN, "ising_sweep_*.npz")))


def load(name):
    fx = np.load(os.path.join(common.GOLDEN, "ising_sweep_%s.npz" % name))
    kw = dict(n_agents=int(fx["arg_n_agents"]), temperature=float(fx["arg_temperature"]), steps=int(fx["arg_steps"]),
              lr=float(fx["arg_lr"]), act_rate=float(fx["arg_act_rate"]), decay_rate=float(fx["arg_decay_rate"]),
              decay_gap=int(fx["arg_decay_gap"]), seed=int(fx["arg_seed"]))
    return fx, kw


def mse_bound(n_agents, mse_ref):
    """Two summation orders of N non-negative float64 terms differ by at most (N - 1) u sum each from the exact sum,
    u = 2^-53, to first order: |a - b| <= 2 N 2^-53 mse_ref."""
    return 2.0 * n_agents * 2.0 ** -53 * mse_ref


def test_fixture_set():
    assert FIXTURES == ["n100_t002", "n100_t08_act05", "n16_t002_act05", "n16_t08"]


@pytest.mark.parametrize("name", ["n100_t002", "n100_t08_act05", "n16_t002_act05", "n16_t08"])
def test_restatement_equals_recorded_reference_episode(name):
    fx, kw = load(name)
    got = ref.trace(**kw)
    S = int(fx["stop"])
    assert got["steps"] == S
    assert got["rsum"].tobytes() == fx["reward_sum"].tobytes()
    assert got["order"].tobytes() == fx["order"].tobytes()
    np.testing.assert_array_equal(got["n_up"], fx["n_up"])
    assert got["q"].tobytes() == fx["q_final"].tobytes()
    np.testing.assert_array_equal(got["spins"], fx["spins_final"])
    # the device's summation order against the script's act_group order
    bound = mse_bound(kw["n_agents"], fx["mse"])
    err = np.abs(got["mse"] - fx["mse"])
    print("%s: max |mse - mse_ref| / bound = %.3g" % (name, np.max(err / np.where(bound > 0, bound, 1.0))))
    assert (err <= bound).all()
    assert (np.abs(got["mse_script"] - fx["mse"]) <= bound).all()
    assert fx["mse"].max() > 0.0


def test_target_formula_is_the_scripts_table_at_k4():
    table = np.array([[2, -2], [1, -1], [0, 0], [-1, 1], [-2, 2]], dtype=np.float64)   # main_MFQ_Ising.py:77-81
    np.testing.assert_array_equal(ref.target(4), table)
    t8 = ref.target(8)
    assert t8.shape == (9, 2) and t8[0, 0] == 4.0 and t8[8, 1] == 4.0 and t8[4, 0] == 0.0
    np.testing.assert_array_equal(t8[:, 0], -t8[:, 1])


def test_device_mse_order_is_not_the_plain_sum():
    """The contract's order matters: on 100 terms of mixed size it differs from numpy's left-to-right sum in the
    last bits (else the bit-for-bit GPU comparison would not pin the order), and stays within the bound."""
    rs = np.random.RandomState(5)
    differs = 0
    for n in (100, 1156):
        terms = rs.random_sample(n) ** 8
        a = ref.device_mse(terms, n)
        b = 0.0
        for x in terms:
            b += x
        b /= n
        assert abs(a - b) <= mse_bound(n, b)
        differs += a != b
    assert differs


def test_metropolis_table_matches_the_package():
    from mfrl_amd.ising import metropolis_table
    for tau in (0.4, 1.0, 4.0):
        assert metropolis_table(tau).tobytes() == ref.metropolis_table(tau).tobytes()
    acc = metropolis_table(0.5)
    assert acc[0] == 1.0 and acc[1] == 1.0 and acc[2] == 1.0 and acc[3] == np.exp(-2 / 0.5) and acc[4] == np.exp(-4 / 0.5)
    assert metropolis_table(0.5, coupling=2.0)[4] == np.exp(-8 / 0.5)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_metropolis_orders_below_and_disorders_above(seed):
    """L = 16, 400 sweeps from all up: ordered at tau 0.4, disordered at tau 4.0 (the chain's critical point is
    tau = 2 / ln(1 + sqrt 2) / 2 ~ 1.13: its exponent is half the textbook Delta E / T at J = 1)."""
    cold = ref.metropolis(256, 400, ref.metropolis_table(0.4), seed=seed)
    hot = ref.metropolis(256, 400, ref.metropolis_table(4.0), seed=seed)
    print("seed %d: order %.3f at 0.4, %.3f at 4.0" % (seed, cold["order"][-1], hot["order"][-1]))
    assert cold["order"][-1] >= 0.9
    assert hot["order"][-1] <= 0.4


def test_metropolis_replicas_and_sweeps_draw_apart():
    u = ref.mc_uniform(3, np.arange(2)[:, None, None], np.arange(3)[None, :, None], np.arange(16)[None, None, :])
    assert len(np.unique(u)) == u.size and (u >= 0).all() and (u < 1).all()
    import ising_oracle
    assert not np.array_equal(u[0, 0], ising_oracle.philox_uniform(3, 0, 0, np.arange(16))), "its own domain"


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kw", [dict(temperatures=[0.8, 0.0]), dict(temperatures=[float("nan")]),
                                dict(temperatures=[float("inf")]), dict(temperatures=[-1.0]), dict(temperatures=[]),
                                dict(seeds=0), dict(steps=0), dict(n_agents=10), dict(mcmc_sweeps=-1),
                                dict(n_agents=25, mcmc_sweeps=5)])
def test_sweep_refuses(kw):
    from mfrl_amd.ising import sweep
    args = dict(n_agents=16, temperatures=[0.8], seeds=1, steps=10)
    args.update(kw)
    with pytest.raises(ValueError):
        sweep(**args)


@pytest.mark.parametrize("n,K", [(25, 4), (36, 8), (16, 6), (4, 2)])
def test_metropolis_shape_refusals(n, K):
    from mfrl_amd.ising import check_mc_shape
    with pytest.raises(ValueError):
        check_mc_shape(n, K)
    check_mc_shape(16, 4)
    check_mc_shape(1156, 4)


@pytest.mark.parametrize("argv,word", [(["-p", "1"], "matplotlib"), (["-epi", "2"], "-epi"), (["-ns", "8"], "-ns"),
                                       (["-n", "10"], "square"), (["-t", "0.5", "-1"], "temperature"),
                                       (["-s", "Other.py"], "scenario"), (["--seeds", "0"], "--seeds"),
                                       (["-ac", "1.5"], "act rate"), (["-n", "25", "--mcmc", "10"], "even")])
def test_cli_refuses(argv, word):
    from mfrl_amd import main_MFQ_Ising as cli
    with pytest.raises(SystemExit) as ex:
        cli.main(argv)
    assert word in str(ex.value), str(ex.value)


def test_cli_takes_the_scripts_arguments():
    from mfrl_amd import main_MFQ_Ising as cli
    a = cli.parser().parse_args("-n 400 -t 0.5 0.8 -epi 1 -ts 50 -lr 0.2 -dr 0.9 -dg 7 -ac 0.5 -ns 4 --seeds 3 "
                                "--mcmc 20".split())
    assert (a.num_agents, a.temperature, a.time_steps, a.learning_rate, a.decay_rate, a.decay_gap, a.act_rate,
            a.neighbor_size, a.seeds, a.mcmc) == (400, [0.5, 0.8], 50, 0.2, 0.9, 7, 0.5, 4, 3, 20)
    d = cli.parser().parse_args([])
    assert (d.num_agents, d.temperature, d.episode, d.time_steps, d.learning_rate, d.decay_rate, d.decay_gap,
            d.act_rate, d.neighbor_size, d.plot) == (100, [1.0], 1, 10000, 0.1, 0.99, 2000, 1.0, 4, 0)
    cli.check_args(a)


def test_cli_prints_the_scripts_lines(capsys):
    """print_episode on a made-up two-step result: the script's format strings (:147, :158, :168)."""
    from mfrl_amd import main_MFQ_Ising as cli
    res = {"steps": np.array([[2]]), "q": np.zeros((1, 1, 16, 5, 2)), "order": np.array([[[0.25, 0.5]]]),
           "n_up": np.array([[[10, 12]]]), "rsum": np.array([[[4.0, -2.5]]]), "mse": np.array([[[1.5, 0.125]]])}
    cli.print_episode(res)
    out = capsys.readouterr().out.splitlines()
    assert out == ["+++++++++++++++++++++++++++++",
                   "E: 0/0, reward = 4.000000, mse = 1.500000, Order = 0.250000, Up = 10, Down = 6",
                   "+++++++++++++++++++++++++++++",
                   "E: 0/1, reward = -2.500000, mse = 0.125000, Order = 0.500000, Up = 12, Down = 4",
                   "Episode: 0, MaxO = 0.500000 at 1 (12/4)"]
