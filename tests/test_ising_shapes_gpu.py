"""The Ising kernels off the 4-neighbour, fixed-temperature line (csrc/ising_kernels.hip), bit for bit.

Every device result is compared with float64 numpy in the reference's own operation order (oracle/ising_oracle.py),
which tests/test_ising_cpu.py pins to fixtures recorded from the reference's Ising.py / core.py -- no tolerances.

The kernel each case runs: K <= 4 takes the <4> instantiations, K > 4 the <16> ones (17 Q rows in registers, chosen
by `if (s == st)` chains); N <= 1024 takes k_ising_mfq (one lane per agent), N > 1024 k_ising_mfq_big.

The device exp() is not bit-pinned, so every oracle-compared case first asserts, from the oracle alone, that no draw
came within GAP of its threshold: min |u - c0| > 1e-12, about 10^3 times what a libm exp a few ulp off can move c0
(c0 is a quotient of two exps in [0, 1]: an ulp of either is ~1e-16 of it)."""
import json
import os
import sys

import numpy as np
import pytest

import common

sys.path.insert(0, os.path.join(common.REPO, "oracle"))
import ising_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

GAP = 1e-12
U_MAX = 1.0 - 2.0 ** -53                    # the largest double random_sample can return

with open(os.path.join(common.GOLDEN, "ising_manifest.json")) as f:
    SHAPE_CASES = json.load(f)["shape_cases"]


def _clear(ref, tag=""):
    """The precondition: the oracle's closest draw stands clear of its threshold."""
    print("%s min|u-c0| = %.3e over %d steps" % (tag, ref["min_gap"], ref["steps"]))
    assert ref["min_gap"] > GAP, (tag, ref["min_gap"])


def _same(got, r, ref, spins=True, tag=""):
    """Replica r of a device result against one oracle episode: stop step, order, n_up, Q bytes, final spins."""
    S = ref["steps"]
    assert int(got["steps"][r]) == S, (tag, r, int(got["steps"][r]), S)
    assert got["order"][r, :S].tobytes() == ref["order"].tobytes(), (tag, r)
    np.testing.assert_array_equal(got["n_up"][r, :S], ref["n_up"], err_msg=str((tag, r)))
    assert got["q"][r].shape == ref["q"].shape, (tag, r)
    assert got["q"][r].tobytes() == ref["q"].tobytes(), (tag, r)
    if spins:
        np.testing.assert_array_equal(got["spins"][r], ref["spins"], err_msg=str((tag, r)))


def _stream(n, view, steps, temperature, replicas=1, **kw):
    """Reference mode (numpy's stream generated on the device) at any view: replica r = the script with seed + r."""
    from mfrl_amd.ising import IsingLattice
    lat = IsingLattice(n, replicas, view=view)
    return lat, lat.run_mfq_stream(steps, temperature, **kw)[0]


# ------------------------------------------------------------------ views
@pytest.mark.parametrize("name", ["ising7_v3", "ising4_v2"])
def test_views_reference_mode_matches_fixture(name):
    """k_ising_mfq<16> at K 12 (49 agents, view 3) and K 6 (16 agents, view 2: the wrap-collapsed mask) against the
    trajectories recorded from the reference scenario."""
    c = SHAPE_CASES[name]
    fx = np.load(os.path.join(common.GOLDEN, name + ".npz"))
    ref = ising_oracle.mfq(c["n_agents"], c["temperature"], c["steps"], seed=c["seed"], view=c["view"])
    _clear(ref, name)
    lat, out = _stream(c["n_agents"], c["view"], c["steps"], c["temperature"], seed=c["seed"])
    assert lat.K == c["K"]
    T = c["stopped_after"]
    assert int(out["steps"][0]) == T
    assert out["order"][0, :T].tobytes() == fx["order"].tobytes()
    np.testing.assert_array_equal(out["n_up"][0, :T], fx["n_up"])
    np.testing.assert_array_equal(out["spins"][0], fx["spins_final"])
    assert out["q"][0].shape == fx["q_final"].shape == (c["n_agents"], c["K"] + 1, 2)
    assert out["q"][0].tobytes() == fx["q_final"].tobytes()


@pytest.mark.parametrize("n,view,K,steps", [(81, 4, 16, 60), (64, 4, 14, 60), (1089, 2, 8, 30)])
def test_views_reference_mode_matches_oracle(n, view, K, steps):
    """K 16 (the last register row), K 14 (mask-scan neighbourhood, 2 view >= L) and the big kernel's <16>
    instantiation at K 8."""
    ref = ising_oracle.mfq(n, 0.8, steps, seed=21, view=view)
    _clear(ref, (n, view))
    assert ref["q"].shape[1] == K + 1
    assert ref["q"][:, K].any(), "the case must reach the last Q row (every neighbour up)"
    lat, out = _stream(n, view, steps, 0.8, seed=21)
    assert lat.K == K
    _same(out, 0, ref)


@pytest.mark.parametrize("n,view,K", [(16, 2, 6), (49, 3, 12), (81, 4, 16)])
def test_env_step_views_and_signed_actions(n, view, K):
    """k_ising_step at K != 4, three replicas, actions from {-3 .. 3}: a non-positive action is spin 0."""
    from mfrl_amd.ising import IsingLattice
    rs = np.random.RandomState(100 + K)
    R = 3
    lat = IsingLattice(n, replicas=R, view=view)
    assert lat.K == K
    nbr = ising_oracle.neighbours(n, view)
    lat.set_spins(rs.randint(0, 2, size=(R, n)))
    acts = rs.randint(-3, 4, size=(R, n))
    assert (acts < 0).any() and (acts == 0).any() and (acts > 1).any()
    rew, obs, nup, order = lat.step(acts)
    for r in range(R):
        s, rw, ob, nu, od = ising_oracle.env_step(None, nbr, acts[r])
        assert rew[r].tobytes() == rw.tobytes(), r
        np.testing.assert_array_equal(obs[r], ob)
        assert nup[r] == nu and order[r] == od
        np.testing.assert_array_equal(lat.get_spins()[r], s)


def test_dropin_env_agent_view_2_under_the_reference_loop():
    """main_MFQ_Ising.py's loop on the drop-in env with agent_view=2 on 25 agents (K 8, Q sized K + 1) against the
    oracle: every action and the float64 Q table."""
    from examples.ising_model.multiagent.environment import IsingMultiAgentEnv
    import examples.ising_model as ising_model
    n, T, tau, lr, seed = 25, 60, 0.8, 0.1, 13
    ref = ising_oracle.mfq(n, tau, T, lr=lr, seed=seed, view=2)
    _clear(ref, "dropin")
    state = np.random.get_state()
    try:
        np.random.seed(seed)
        scen = ising_model.load("Ising.py").Scenario()
        env = IsingMultiAgentEnv(world=scen.make_world(num_agents=n, agent_view=2), reset_callback=scen.reset_world,
                                 reward_callback=scen.reward, observation_callback=scen.observation,
                                 done_callback=scen.done)
        n_actions = env.action_space[0].n
        assert env.observation_space[0].n == 8
        obs = np.stack(env.reset())
        K = obs.shape[1]
        assert K == 8
        Q = np.zeros((env.n, K + 1, n_actions))
        current_t = 0.3
        acts, orders = [], []
        for t in range(T):
            action = np.zeros(env.n, dtype=np.int32)
            if t % 2000 == 0:
                current_t *= 0.99
            if current_t < tau:
                current_t = tau
            for i in range(env.n):
                s = np.count_nonzero(obs[i] == 1)
                vals = [np.exp(Q[i, s, k] / current_t) for k in range(n_actions)]
                denom = 0
                for v in vals:
                    denom += v
                action[i] = np.random.choice(n_actions, 1, p=[v / denom for v in vals])[0]
            obs_, reward, done, order, ups, downs = env.step(np.expand_dims(action, axis=1))
            obs_ = np.stack(obs_)
            for i in np.random.choice(env.n, env.n, replace=False):
                s = np.count_nonzero(obs[i] == 1)
                Q[i, s, action[i]] = Q[i, s, action[i]] + lr * (reward[i][0] - Q[i, s, action[i]])
            obs = obs_
            acts.append(action.copy())
            orders.append(order)
    finally:
        np.random.set_state(state)
    np.testing.assert_array_equal(np.stack(acts), ref["actions"])
    assert np.array(orders).tobytes() == ref["order"].tobytes()
    assert Q.tobytes() == ref["q"].tobytes()


# ------------------------------------------------------------------ annealing
def test_anneal_reference_mode_matches_fixture():
    """The temperature decays every 7 steps (x 0.8) from 0.3 into its clamp at 0.02, then the order parameter stays
    flat and the episode stops at step 547 of 1200 (k_ising_mfq<4>)."""
    from mfrl_amd.ising import run_mfq
    c = SHAPE_CASES["ising10_anneal"]
    fx = np.load(os.path.join(common.GOLDEN, "ising10_anneal.npz"))
    kw = dict(lr=c["lr"], decay_rate=c["decay_rate"], decay_gap=c["decay_gap"], seed=c["seed"])
    ref = ising_oracle.mfq(c["n_agents"], c["temperature"], c["steps"], **kw)
    _clear(ref, "ising10_anneal")
    out = run_mfq(c["n_agents"], c["temperature"], c["steps"], **kw)
    T = c["stopped_after"]
    assert T == 547 and int(out["steps"][0]) == T
    assert out["order"][0, :T].tobytes() == fx["order"].tobytes()
    np.testing.assert_array_equal(out["n_up"][0, :T], fx["n_up"])
    np.testing.assert_array_equal(out["spins"][0], fx["spins_final"])
    assert out["q"][0].tobytes() == fx["q_final"].tobytes()


def test_anneal_big_kernel_matches_oracle():
    """The same schedule in k_ising_mfq_big<4> (1089 agents) with lr 0.25."""
    from mfrl_amd.ising import run_mfq
    kw = dict(lr=0.25, decay_rate=0.8, decay_gap=7, seed=21)
    ref = ising_oracle.mfq(1089, 0.02, 60, **kw)
    _clear(ref, "anneal 1089")
    _same(run_mfq(1089, 0.02, 60, **kw), 0, ref)


# ------------------------------------------------------------------ Philox
@pytest.mark.parametrize("n,view,R,T", [(100, 1, 3, 50), (1089, 1, 2, 20), (25, 2, 2, 40)])
def test_philox_mode_equals_supplied_philox_draws(n, view, R, T):
    """The kernel's Philox draws are philox_uniform(seed, replica, step, agent) of the oracle (pinned to Random123's
    known answers in tests/test_ising_cpu.py): Philox mode equals the run from those draws uploaded, and the oracle
    fed them -- Q, order, n_up, stop step and spins."""
    from mfrl_amd.ising import IsingLattice
    seed, tau = 0x9E3779B1, 0.8
    spins0 = np.random.RandomState(7).randint(0, 2, size=(R, n)).astype(np.uint8)
    spins0[:] = spins0[0]                                       # the replicas differ by their draws alone
    u = np.stack([ising_oracle.philox_uniform(seed, r, np.arange(T)[:, None], np.arange(n)[None, :])
                  for r in range(R)])
    refs = [ising_oracle.mfq_given(spins0[r], u[r], None, view, temperature=tau) for r in range(R)]
    for r in range(R):
        _clear(refs[r], ("philox", n, r))
    lat = IsingLattice(n, R, view=view)
    lat.set_spins(spins0)
    dev = lat.run_mfq(T, tau, seed=seed)
    lat.set_spins(spins0)
    host = lat.run_mfq(T, tau, u=u)
    np.testing.assert_array_equal(dev["steps"], host["steps"])
    np.testing.assert_array_equal(dev["n_up"], host["n_up"])
    assert dev["order"].tobytes() == host["order"].tobytes()
    assert dev["q"].tobytes() == host["q"].tobytes()
    np.testing.assert_array_equal(dev["spins"], host["spins"])
    for r in range(R):
        _same(dev, r, refs[r], tag="philox")
        _same(host, r, refs[r], tag="uploaded")
    for r in range(1, R):
        assert not np.array_equal(dev["n_up"][r], dev["n_up"][0]), "replicas must draw apart"
        assert dev["q"][r].tobytes() != dev["q"][0].tobytes()


# ------------------------------------------------------------------ early stop from supplied draws
@pytest.mark.parametrize("n", [1089, 1024])
def test_early_stop_per_replica_in_one_launch(n):
    """Three replicas of one launch (1089: k_ising_mfq_big; 1024: k_ising_mfq with all 1024 lanes): u == 0 makes every
    action 0 and u == 1 - 2^-53 every action 1, so the order parameter is 1.0 from step 0 and replicas 0 and 2 leave
    the step loop at 500 of 520, while replica 1, on random draws, runs to the cap."""
    from mfrl_amd.ising import IsingLattice
    T, tau = 520, 0.8
    rs = np.random.RandomState(n)
    spins0 = rs.randint(0, 2, size=(3, n)).astype(np.uint8)
    u = np.empty((3, T, n))
    u[0], u[1], u[2] = 0.0, rs.random_sample((T, n)), U_MAX
    refs = [ising_oracle.mfq_given(spins0[r], u[r], temperature=tau) for r in range(3)]
    for r in range(3):
        _clear(refs[r], ("early stop", n, r))
    assert [ref["steps"] for ref in refs] == [500, T, 500]
    lat = IsingLattice(n, 3)
    lat.set_spins(spins0)
    out = lat.run_mfq(T, tau, u=u)
    assert list(out["steps"]) == [500, T, 500]
    assert (out["order"][0, :500] == 1.0).all() and (out["n_up"][0, :500] == 0).all()
    assert (out["order"][2, :500] == 1.0).all() and (out["n_up"][2, :500] == n).all()
    assert not out["spins"][0].any() and out["spins"][2].all()
    for r in range(3):
        _same(out, r, refs[r], tag=("early stop", n))


@pytest.mark.parametrize("n", [100, 1089])
def test_action_threshold_at_equality(n):
    """searchsorted(side='right') is u >= c0.  At step 0 Q is zero and c0 = (1/2) / (1/2 + 1/2) = 0.5 exactly
    (exp(0) = 1): a draw of 0.5 acts 1, the double just below acts 0.  Step 0 sits on the threshold by construction,
    so the clearance precondition applies from step 1 on."""
    from mfrl_amd.ising import IsingLattice
    T, tau = 8, 0.8
    rs = np.random.RandomState(3)
    half = rs.permutation(n) < n // 2
    u = rs.random_sample((T, n))
    u[0] = np.where(half, 0.5, np.nextafter(0.5, 0.0))
    spins0 = rs.randint(0, 2, size=n).astype(np.uint8)
    ref = ising_oracle.mfq_given(spins0, u, temperature=tau)
    assert ref["gaps"][0] == 0.0 and ref["gaps"][1:].min() > GAP
    np.testing.assert_array_equal(ref["actions"][0], half.astype(np.int64))
    lat = IsingLattice(n, 1)
    lat.set_spins(spins0[None])
    one = lat.run_mfq(1, tau, u=u[None, :1])
    np.testing.assert_array_equal(one["spins"][0], half.astype(np.uint8))
    assert int(one["n_up"][0, 0]) == n // 2
    lat.set_spins(spins0[None])
    _same(lat.run_mfq(T, tau, u=u[None]), 0, ref, tag="equality")


# ------------------------------------------------------------------ stream mode, replicas stopping apart
def test_stream_episodes_with_replicas_stopping_apart():
    """Three episodes on each replica's stream, four replicas (seed 13 + r) in one launch per episode: the replicas
    stop at different steps, so every replica's next episode starts at its own offset prev_off[r][prev_steps[r]]."""
    from mfrl_amd.ising import IsingLattice
    R, E, T = 4, 3, 2000
    refs = [ising_oracle.mfq_episodes(16, 0.1, T, E, seed=13 + r) for r in range(R)]
    for k in range(E - 1):
        assert len({refs[r][k]["steps"] for r in range(R)}) > 1, "the replicas must stop apart"
    assert any(refs[r][k]["steps"] < T for r in range(R) for k in range(E - 1))
    got = IsingLattice(16, R).run_mfq_stream(T, 0.1, seed=13, episodes=E)
    for r in range(R):
        for k in range(E):
            _clear(refs[r][k], ("stream", r, k))
            _same(got[k], r, refs[r][k], spins=(k == E - 1), tag=("stream", k))


# ------------------------------------------------------------------ sizes
@pytest.mark.parametrize("n,steps", [(1024, 40), (1089, 40), (32761, 3)])
def test_sizes_reference_mode_matches_oracle(n, steps):
    """Both sides of the kernel hand-over (1024: the register kernel's full workgroup; 1089: the big kernel's first
    size) and the largest lattice (181 x 181: 98,283 B of dynamic LDS)."""
    from mfrl_amd.ising import run_mfq
    ref = ising_oracle.mfq(n, 0.8, steps, seed=21)
    _clear(ref, n)
    _same(run_mfq(n, 0.8, steps, seed=21), 0, ref)


def test_act_rate_half_on_the_big_kernel():
    """act_rate 0.5 above 1024 agents: the scan's permutation and act_group bits, the big kernel's mask read -- the
    device stream against the host stream, and both against the oracle."""
    from mfrl_amd.ising import run_mfq
    n, R, T = 1089, 2, 40
    dev = run_mfq(n, 0.8, T, act_rate=0.5, seed=13, replicas=R)
    host = run_mfq(n, 0.8, T, act_rate=0.5, seed=13, replicas=R, mode="host")
    assert dev["q"].tobytes() == host["q"].tobytes()
    assert dev["order"].tobytes() == host["order"].tobytes()
    np.testing.assert_array_equal(dev["steps"], host["steps"])
    np.testing.assert_array_equal(dev["n_up"], host["n_up"])
    np.testing.assert_array_equal(dev["spins"], host["spins"])
    for r in range(R):
        ref = ising_oracle.mfq(n, 0.8, T, act_rate=0.5, seed=13 + r)
        _clear(ref, ("act 0.5", r))
        _same(dev, r, ref)


def test_act_rate_truncates_like_int():
    """int(0.29 * 100) is 28, not 29: 28 agents update at every step (the host stream's act_group bits), and the
    device stream, which counts them itself, gives the same run as the host stream and the oracle."""
    from mfrl_amd.ising import reference_stream, run_mfq
    n, T = 100, 60
    assert int(0.29 * n) == 28
    _, _, mask = reference_stream(13, n, T, 0.29)
    bits = (mask[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    assert (bits.reshape(T, -1).sum(axis=1) == 28).all()
    ref = ising_oracle.mfq(n, 0.8, T, act_rate=0.29, seed=13)
    _clear(ref, "act 0.29")
    # one step with lr 1: Q holds the reward wherever an agent updated, so at most 28 agents carry a non-zero row
    first = ising_oracle.mfq(n, 0.8, 1, lr=1.0, act_rate=0.29, seed=13)
    touched = int(first["q"].reshape(n, -1).any(axis=1).sum())
    assert 0 < touched <= 28
    for mode in ("reference", "host"):
        _same(run_mfq(n, 0.8, T, act_rate=0.29, seed=13, mode=mode), 0, ref, tag=mode)
        one = run_mfq(n, 0.8, 1, lr=1.0, act_rate=0.29, seed=13, mode=mode)
        assert int(one["q"][0].reshape(n, -1).any(axis=1).sum()) == touched
        assert one["q"][0].tobytes() == first["q"].tobytes()


def test_act_rate_zero_updates_nothing():
    """act_rate 0: the permutation is still drawn (the stream moves on), no agent updates, Q stays zero."""
    from mfrl_amd.ising import run_mfq
    n, T = 36, 60
    ref = ising_oracle.mfq(n, 0.8, T, act_rate=0.0, seed=13)
    _clear(ref, "act 0")
    assert not ref["q"].any()
    for mode in ("reference", "host"):
        out = run_mfq(n, 0.8, T, act_rate=0.0, seed=13, mode=mode)
        assert out["q"].tobytes() == bytes(out["q"].nbytes), mode       # all +0.0
        _same(out, 0, ref, tag=mode)


# ------------------------------------------------------------------ seed wrap
def test_replica_seeds_wrap_at_32_bits():
    """Replica r runs RandomState((seed + r) mod 2^32): seed 2^32 - 2 gives replicas 2 and 3 the seeds 0 and 1."""
    from mfrl_amd.ising import run_mfq
    seed, R, T = 2 ** 32 - 2, 4, 30
    out = run_mfq(16, 0.8, T, seed=seed, replicas=R)
    for r in range(R):
        ref = ising_oracle.mfq(16, 0.8, T, seed=(seed + r) % 2 ** 32)
        _clear(ref, ("wrap", r))
        _same(out, r, ref, tag="wrap")
