"""The GAE(lambda) mode of the actor-critic models without a GPU: the properties of the numpy restatement
(tests/gae_ref.py) on the synthetic forest -- lambda = 0 is the one-step TD error, lambda = 1 the reference's
bootstrapped return -- and the refusals of the surface: the setters, train() on a "gae" model, train_battle's flags."""
import numpy as np
import pytest

import common  # noqa: F401  (the package path)
import gae_ref

GAMMA = 0.95


@pytest.mark.parametrize("scale", [1.0, 100.0])
def test_lambda_0_is_the_one_step_td_error(scale):
    """adv = (rew + gamma V[succ]) - V in float64, rounded once, bit for bit; a tail is its own successor.  And the
    reward column is then adv + V."""
    f = gae_ref.forest(scale)
    rew, adv, bad = gae_ref.chain_gae(f["rew"], f["prev"], f["tails"], f["V"], GAMMA, 0.0)
    assert bad is None
    succ = gae_ref.successors(f["prev"], f["tails"])
    V = f["V"].astype(np.float64)
    want = (f["rew"].astype(np.float64) + np.float64(GAMMA) * V[succ]) - V
    assert adv.tobytes() == want.astype(np.float32).tobytes()
    assert rew.tobytes() == (want + V).astype(np.float32).tobytes()


@pytest.mark.parametrize("scale", [1.0, 100.0])
def test_lambda_1_is_the_bootstrapped_return(scale):
    """rew = replay.chain_returns_host(numpy1=True) bootstrapped from V[tails], to within one float32 spacing per row
    (the walk forms the return as (return - V) + V: two more roundings in float64 before the one to float32; in numpy
    0 of the 6,384 rows differ at either value scale -- the bound is the spacing, not zero), and adv = return - V."""
    from mfrl_amd.replay import chain_returns_host
    f = gae_ref.forest(scale)
    rew, adv, bad = gae_ref.chain_gae(f["rew"], f["prev"], f["tails"], f["V"], GAMMA, 1.0)
    assert bad is None
    want = chain_returns_host(f["rew"], f["prev"], f["tails"], f["V"][f["tails"]], GAMMA, numpy1=True)
    assert want.dtype == np.float32 and len(want) == gae_ref.FOREST_ROWS
    diff = np.abs(rew.astype(np.float64) - want.astype(np.float64))
    print("rows that differ:", int((diff > 0).sum()), "of", len(want))
    assert (diff <= np.spacing(np.abs(want)).astype(np.float64)).all()
    # adv + V is the return again, to the rounding of the two float32 columns
    back = adv.astype(np.float64) + f["V"].astype(np.float64)
    tol = np.spacing(np.abs(want)) + np.spacing(np.abs(adv)) + np.spacing(np.abs(f["V"]))
    assert (np.abs(back - want) <= tol).all()


def test_the_walk_stops_at_a_bad_link():
    prev = np.array([-1, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9], np.int64)
    rew = np.arange(1, 13, dtype=np.float32)
    V = np.linspace(-1, 1, 12).astype(np.float32)
    prev[5] = 7
    out, adv, bad = gae_ref.chain_gae(rew, prev, [10, 11], V, GAMMA, 0.5, adv=np.full(12, -7, np.float32))
    assert bad == 7
    assert (adv[[1, 3]] == -7).all() and out[[1, 3]].tobytes() == rew[[1, 3]].tobytes()
    assert (adv[[5, 7, 9, 11]] != -7).all() and (adv[0::2] != -7).all()


def test_normalise_restatement():
    a = np.random.default_rng(3).standard_normal(1000).astype(np.float32)
    z = gae_ref.adv_normalize(a)
    assert abs(z.mean()) < 1e-12 and abs(z.std() - 1.0) < 1e-6
    assert not gae_ref.adv_normalize(np.full(7, 2.5, np.float32)).any()
    assert not gae_ref.adv_normalize(np.array([3.0], np.float32)).any()


# ------------------------------------------------------------------------------------------------- the surface
def _models():
    from mfrl_amd.algo.ac import MFAC, ActorCritic
    return [cls.__new__(cls) for cls in (ActorCritic, MFAC)]


def test_setters_validate():
    from mfrl_amd.algo.ac import ActorCritic
    for m in _models():
        assert m.advantage == "returns" and m.gae_lambda == 0.95 and m.adv_norm is False
        for bad in ("gae ", "GAE", "", None, 1):
            with pytest.raises(ValueError):
                m.advantage = bad
        for bad in (-0.01, 1.01, float("nan"), "0.9", None, True):
            with pytest.raises(ValueError):
                m.gae_lambda = bad
        assert m.gae_lambda == 0.95
        with pytest.raises(ValueError, match="gae"):
            m.adv_norm = True                                   # requires "gae"
        for bad in (1, "yes", None):
            with pytest.raises(ValueError):
                m.adv_norm = bad
        m.advantage = "gae"
        m.gae_lambda = 0
        assert m.gae_lambda == 0.0
        m.gae_lambda = 1
        m.gae_lambda = 0.5
        m.adv_norm = True
        assert (m.advantage, m.gae_lambda, m.adv_norm) == ("gae", 0.5, True)
        with pytest.raises(ValueError, match="adv_norm"):
            m.advantage = "returns"                             # not while adv_norm is set
        m.adv_norm = False
        m.advantage = "returns"
        assert m.advantage == "returns"
    assert (ActorCritic._advantage, ActorCritic._gae_lambda, ActorCritic._adv_norm) == ("returns", 0.95, False)


def test_train_refuses_a_gae_model():
    for m in _models():
        m.advantage = "gae"
        with pytest.raises(ValueError, match="device rollout loop"):
            m.train()


def test_chain_gae_wrapper_refuses_gamma_and_lambda_before_anything_else():
    from mfrl_amd import replay
    for gamma, lam in ((1.5, 0.5), (0.9, -0.1), (float("nan"), 0.5), (0.9, float("nan"))):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            replay.chain_gae(None, None, None, None, None, gamma, lam)


@pytest.mark.parametrize("argv,msg", [
    (["--algo", "mfq", "--envs", "4", "--rollout", "--advantage", "gae"], "--advantage"),
    (["--algo", "il", "--envs", "4", "--rollout", "--advantage", "gae"], "--advantage"),
    (["--algo", "mfac", "--advantage", "gae"], "--rollout_episodes"),
    (["--algo", "ac", "--envs", "4", "--advantage", "gae"], "--rollout_episodes"),
    (["--algo", "mfac", "--envs", "4", "--rollout_episodes", "--gae_lambda", "0.9"], "--gae_lambda"),
    (["--algo", "mfac", "--envs", "4", "--rollout_episodes", "--adv_norm"], "--adv_norm"),
    (["--algo", "mfac", "--envs", "4", "--rollout_episodes", "--advantage", "returns", "--adv_norm"], "--adv_norm"),
    (["--algo", "mfac", "--envs", "4", "--rollout_episodes", "--advantage", "gae", "--gae_lambda", "1.5"], "[0, 1]"),
    (["--algo", "ac", "--envs", "4", "--rollout_episodes", "--advantage", "gae", "--gae_lambda", "-0.1"], "[0, 1]"),
    (["--algo", "ac", "--envs", "4", "--rollout_episodes", "--advantage", "gae", "--gae_lambda", "nan"], "[0, 1]"),
    (["--algo", "ac", "--envs", "4", "--rollout_episodes", "--advantage", "lambda"], "--advantage"),
])
def test_train_battle_refuses(argv, msg, capsys, monkeypatch):
    """Every refusal is parser.error (exit status 2), before the env is made."""
    import magent
    from mfrl_amd import train_battle

    def no_env(*a, **k):
        raise AssertionError("the env was made before the refusal")
    monkeypatch.setattr(magent, "GridWorld", no_env)
    with pytest.raises(SystemExit) as ex:
        train_battle.main(argv)
    assert ex.value.code == 2
    assert msg in capsys.readouterr().err
