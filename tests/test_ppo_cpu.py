"""The PPO objective of the actor-critic models without a GPU: the float64 restatement of the loss head (tests/ppo_ref.py)
against finite differences of its own loss and against the advantage-column head it extends, replay.ppo_order, and
the refusals of the surface: the setters, train() on a "ppo" model, ACTrainHIP's column checks, train_battle's flags,
and the three prototypes as ctypes sees them."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import actrain_ref as ar
import common  # noqa: F401  (the package path)
import gae_ref
import ppo_ref

V, F, A = ar.BATTLE
CLIP = 0.2


def _small(seed=5, n=8, A3=3):
    """A = 3, 8 rows, float64: logits, values, actions, returns, advantages of both signs, and lp_old = lp - log(t)
    with t alternating between the inside of the clip range and far outside it on either side."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, A3))
    v, ret = rng.standard_normal(n), 2.5 * rng.standard_normal(n)
    act = rng.integers(0, A3, size=n)
    adv = np.array([1.5, -0.7, 2.0, -1.1, 0.4, -2.2, 0.9, -0.3])
    t = np.array([1.05, 0.95, 1.6, 0.5, 0.45, 1.7, 1.08, 0.93])     # rows 2, 3 clipped; 4, 5 outside on the harmless side
    e = np.exp(z - z.max(1, keepdims=True))
    lp_old = ppo_ref.logp(e / e.sum(1, keepdims=True), act) - np.log(t)
    return z, v, act, ret, adv, lp_old, t


def test_dz_is_the_finite_difference_of_the_loss():
    """dL/dz and dL/dv of the restatement against central differences of its own loss (h = 1e-6, float64: the
    truncation error is h^2 times a third derivative of order 1, the rounding error 1e-16 / h -- 1e-9 covers both by
    an order of magnitude), with no row within 0.05 of a clip bound: the loss has a kink there."""
    z, v, act, ret, adv, lp_old, t = _small()
    got = ppo_ref.head(z, v, act, ret, adv, lp_old, CLIP)
    lo, hi = ppo_ref.bounds(CLIP)
    assert np.allclose(got["r"], t, rtol=1e-12)
    assert min(np.abs(got["r"] - lo).min(), np.abs(got["r"] - hi).min()) > 0.05
    assert got["clipped"].tolist() == [False, False, True, True, False, False, False, False]
    assert got["clip_frac"] == 2 / 8 and got["approx_kl"] > 0
    h = 1e-6
    loss = lambda zz, vv: sum(ppo_ref.loss_terms(zz, vv, act, ret, adv, lp_old, CLIP))
    assert abs(loss(z, v) - sum(got["stats"][:3])) < 1e-15
    for i in range(z.shape[0]):
        for k in range(z.shape[1]):
            zp, zm = z.copy(), z.copy()
            zp[i, k] += h
            zm[i, k] -= h
            fd = (loss(zp, v) - loss(zm, v)) / (2 * h)
            assert abs(fd - got["dz"][i, k]) < 1e-9, (i, k, fd, got["dz"][i, k])
        vp, vm = v.copy(), v.copy()
        vp[i] += h
        vm[i] -= h
        assert abs((loss(z, vp) - loss(z, vm)) / (2 * h) - got["dv"][i]) < 1e-9


@pytest.mark.parametrize("use_mf", [False, True])
def test_ratio_one_is_the_advantage_column_head(use_mf):
    """lp_old = the rows' own lp (r = 1 everywhere, nothing clipped): the head is actrain_ref's with adv = ret - v --
    its policy-bias and value-bias gradients are the column sums of dz and dv -- and torch's float64 gradient of the
    whole network is gae_ref.torch_gradient's on the same advantage column; clip_frac and approx_kl are 0."""
    n = 40
    blob, (nb, off) = ar.packed(V, F, A, use_mf, 11)
    rows = ar.rows(V, F, A, use_mf, 11, n)
    g, stats = ar.gradient(blob, off, V, F, A, use_mf, rows)
    k = ar.forward_keep(blob.astype(np.float64), off, V, F, A, use_mf, rows["obs"], rows["feat"], rows.get("prob"))
    lp = ppo_ref.logp(k["s"], rows["act"])
    adv = rows["ret"].astype(np.float64) - k["v"]
    got = ppo_ref.head(k["z"], k["v"], rows["act"], rows["ret"], adv, lp, CLIP)
    assert got["clip_frac"] == 0.0 and abs(got["approx_kl"]) < 1e-15 and np.abs(got["r"] - 1).max() < 1e-15
    assert np.allclose(got["dz"].sum(0), g[off[8]:off[8] + A], rtol=1e-10, atol=1e-14)
    vb = 18 if use_mf else 10
    assert np.allclose(got["dv"].sum(), g[off[vb]], rtol=1e-10, atol=1e-14)
    # the pg stat is -mean(adv r) = -mean(adv) here, no longer -mean(adv lp); the other three are the head's
    assert abs(got["stats"][0] + adv.mean()) < 1e-14
    assert np.allclose(got["stats"][1:], stats[1:], rtol=1e-12)
    col = (2.5 * np.random.RandomState(77).randn(n)).astype(np.float32)
    net = ar.net(V, F, A, use_mf, 11)
    want, _ = gae_ref.torch_gradient(net, rows, col, torch.float64)
    named, _, extra = ppo_ref.torch_gradient(net, rows, col, lp, CLIP, torch.float64)
    assert extra[0] == 0.0 and abs(extra[1]) < 1e-14
    for name in want:
        scale = np.abs(want[name]).max()
        assert scale > 0 and np.abs(named[name] - want[name]).max() <= 1e-10 * scale, name


def test_every_row_clipped_leaves_no_policy_gradient():
    """adv > 0 and lp_old = lp - 1 (r = e > 1 + clip): dz is the entropy term's alone -- the head's with adv = 0 --
    clip_frac is 1, and the policy loss is the constant -mean(adv) hi."""
    z, v, act, ret, adv, lp_old, t = _small()
    adv = np.abs(adv)
    lp = lp_old + np.log(t)
    got = ppo_ref.head(z, v, act, ret, adv, lp - 1.0, CLIP)
    none = ppo_ref.head(z, v, act, ret, np.zeros_like(adv), lp, CLIP)
    assert got["clipped"].all() and got["clip_frac"] == 1.0
    assert got["dz"].tobytes() == none["dz"].tobytes() and np.abs(got["dz"]).max() > 0
    assert abs(got["stats"][0] + adv.mean() * ppo_ref.bounds(CLIP)[1]) < 1e-15
    # and with adv < 0 on the other side
    got = ppo_ref.head(z, v, act, ret, -adv, lp + 1.0, CLIP)
    assert got["clipped"].all() and got["dz"].tobytes() == none["dz"].tobytes()


def test_a_row_on_the_bound_is_not_clipped():
    lo, hi = ppo_ref.bounds(CLIP)
    r = np.array([hi, np.nextafter(hi, 2.0), lo, np.nextafter(lo, 0.0), hi, lo])
    adv = np.array([1.0, 1.0, -1.0, -1.0, -1.0, 1.0])
    assert ppo_ref.clipped_mask(adv, r, CLIP).tolist() == [False, True, False, True, False, False]


def test_model_losses_is_the_restatement():
    """ActorCritic.losses with logp_old and clip (the model's own code, float64 on the CPU) gives ppo_ref.torch_gradient's
    loss terms and (clip_frac, approx_kl) sums on rows of all three kinds; without them its ops are the default's."""
    from mfrl_amd.algo.ac import ActorCritic
    n = 30
    net = copy.deepcopy(ar.net(V, F, A, True, 11)).double()     # (ar.net is shared: .double() converts in place)
    rows = ar.rows(V, F, A, True, 11, n)
    blob, (nb, off) = ar.packed(V, F, A, True, 11)
    k = ar.forward_keep(blob.astype(np.float64), off, V, F, A, True, rows["obs"], rows["feat"], rows["prob"])
    t = np.tile([1.05, 1.6, 0.5], n // 3)
    lp_old = ppo_ref.logp(k["s"], rows["act"]) - np.log(t)
    adv = 2.5 * np.random.RandomState(77).randn(n)

    class M:
        num_actions, value_coef, ent_coef = A, ar.VALUE_COEF, ar.ENT_COEF
    M.net = net
    m = M()
    T = lambda x: torch.as_tensor(np.array(x, dtype=np.float64))
    pg, vf, ent, value, sums = ActorCritic.losses(m, T(rows["obs"]), T(rows["feat"]), torch.as_tensor(np.array(rows["act"])),
                                            T(rows["ret"]), T(rows["prob"]), adv=T(adv), logp_old=T(lp_old), clip=CLIP)
    _, s, extra = ppo_ref.torch_gradient(ar.net(V, F, A, True, 11), rows, adv, lp_old, CLIP, torch.float64)
    got = tuple(float(x.detach()) for x in (pg, vf, ent, value.mean()))
    # (the model adds the double 1e-6 inside the log, the restatement its float32 value: 3e-14 / p apart per row)
    assert np.allclose(got, s, rtol=1e-9, atol=1e-12), (got, s)
    assert sums.dtype == torch.float64 and not sums.requires_grad
    terms = (sums / n).tolist()
    assert len(ActorCritic.losses(m, T(rows["obs"]), T(rows["feat"]), torch.as_tensor(np.array(rows["act"])),
                                  T(rows["ret"]), T(rows["prob"]), adv=T(adv))) == 4
    assert terms[0] == extra[0] and 0 < extra[0] < 1 and abs(terms[1] - extra[1]) < 1e-9
    ref = ppo_ref.head(k["z"], k["v"], rows["act"], rows["ret"], adv, lp_old, CLIP)
    assert np.allclose(got, ref["stats"], rtol=1e-10) and extra[0] == ref["clip_frac"]
    assert abs(extra[1] - ref["approx_kl"]) < 1e-12


# ------------------------------------------------------------------------------------------------- ppo_order
def test_ppo_order():
    from mfrl_amd.replay import ppo_order
    state = np.random.get_state()
    orders = [ppo_order(1234, 7, e, 8) for e in range(8)]
    again = [ppo_order(1234, 7, e, 8) for e in range(8)]
    other = ppo_order(1234, 8, 0, 8)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    assert orders == again
    for o in orders:
        assert sorted(o) == list(range(8)) and o != list(range(8)) and all(type(k) is int for k in o)
    assert len({tuple(o) for o in orders}) > 1 and other != orders[0]
    assert ppo_order(1, 2, 3, 1) == [0]
    assert sorted(ppo_order(2 ** 32 - 1, 10 ** 6, 3, 5)) == list(range(5))          # a crc32 seed, a late round


# ------------------------------------------------------------------------------------------------- the surface
def _models():
    from mfrl_amd.algo.ac import MFAC, ActorCritic
    return [cls.__new__(cls) for cls in (ActorCritic, MFAC)]


def test_setters_validate():
    from mfrl_amd.algo.ac import ActorCritic
    for m in _models():
        assert (m.objective, m.ppo_clip, m.ppo_epochs, m.ppo_minibatches, m.ppo_target_kl) == ("pg", 0.2, 4, 4, None)
        for bad in ("PPO", "ppo ", "", None, 1):
            with pytest.raises(ValueError):
                m.objective = bad
        with pytest.raises(ValueError, match="gae"):
            m.objective = "ppo"                                 # requires "gae"
        for bad in (0, 0.0, -0.1, float("nan"), float("inf"), "0.2", None, True):
            with pytest.raises(ValueError):
                m.ppo_clip = bad
        for name in ("ppo_epochs", "ppo_minibatches"):
            for bad in (0, -1, 1.0, 2.5, "4", None, True, float("nan")):
                with pytest.raises(ValueError):
                    setattr(m, name, bad)
        for bad in (-1e-9, float("nan"), float("inf"), "0.01", True):
            with pytest.raises(ValueError):
                m.ppo_target_kl = bad
        assert (m.objective, m.ppo_clip, m.ppo_epochs, m.ppo_minibatches, m.ppo_target_kl) == ("pg", 0.2, 4, 4, None)
        m.advantage = "gae"
        m.objective = "ppo"
        m.ppo_clip, m.ppo_epochs, m.ppo_minibatches, m.ppo_target_kl = 0.1, 2, np.int64(3), 0
        assert (m.ppo_clip, m.ppo_epochs, m.ppo_minibatches, m.ppo_target_kl) == (0.1, 2, 3, 0.0)
        assert type(m.ppo_minibatches) is int
        m.ppo_target_kl = 0.015
        m.ppo_target_kl = None
        assert m.ppo_target_kl is None
        with pytest.raises(ValueError, match="ppo"):
            m.advantage = "returns"                             # not while "ppo" is set
        assert m.advantage == "gae"
        m.objective = "pg"
        m.advantage = "returns"
        assert (m.objective, m.advantage) == ("pg", "returns")
        assert m.ppo_rounds == 0
        for bad in (-1, 1.0, "1", None, True):
            with pytest.raises(ValueError):
                m.ppo_rounds = bad
        m.ppo_rounds = 7
        assert m.ppo_rounds == 7
    assert (ActorCritic._objective, ActorCritic._ppo_clip, ActorCritic._ppo_epochs, ActorCritic._ppo_minibatches,
            ActorCritic._ppo_target_kl) == ("pg", 0.2, 4, 4, None)


def test_train_refuses_a_ppo_model():
    for m in _models():
        m.advantage = "gae"
        m.objective = "ppo"
        with pytest.raises(ValueError, match="objective 'ppo'.*device rollout loop"):
            m.train()


def test_actrain_refuses_clip_and_logp_new_without_logp_old():
    """ACTrainHIP._set_ppo's host checks, before the library is reached (a handle is not needed for them)."""
    from mfrl_amd.actrain import ACTrainHIP
    tr = ACTrainHIP.__new__(ACTrainHIP)
    tr.handle = None
    with pytest.raises(ValueError, match="logp_old"):
        tr._set_ppo({}, 4, 0.2)
    with pytest.raises(ValueError, match="logp_old"):
        tr._set_ppo({"logp_new": torch.zeros(4)}, 4, None)
    with pytest.raises(ValueError, match="clip"):
        tr._set_ppo({"logp_old": torch.zeros(4)}, 4, None)
    with pytest.raises(AssertionError, match="logp_old"):
        tr._set_ppo({"logp_old": torch.zeros(4)}, 4, 0.2)       # not a CUDA tensor


@pytest.mark.parametrize("argv,msg", [
    (["--algo", "mfq", "--envs", "4", "--rollout", "--objective", "ppo"], "--objective"),
    (["--algo", "il", "--envs", "4", "--rollout", "--objective", "ppo"], "--objective"),
    (["--algo", "mfac", "--advantage", "gae", "--objective", "ppo"], "--rollout_episodes"),
    (["--algo", "ac", "--envs", "4", "--objective", "ppo"], "--rollout_episodes"),
    (["--algo", "mfac", "--envs", "4", "--rollout_episodes", "--objective", "ppo"], "--advantage gae"),
    (["--algo", "ac", "--envs", "4", "--rollout_episodes", "--advantage", "returns", "--objective", "ppo"],
     "--advantage gae"),
    (["--algo", "mfac", "--envs", "4", "--rollout_episodes", "--advantage", "gae", "--ppo_clip", "0.1"], "--ppo_clip"),
    (["--algo", "mfac", "--envs", "4", "--rollout_episodes", "--advantage", "gae", "--ppo_epochs", "2"], "--ppo_epochs"),
    (["--algo", "mfac", "--envs", "4", "--rollout_episodes", "--advantage", "gae", "--ppo_minibatches", "2"],
     "--ppo_minibatches"),
    (["--algo", "mfac", "--envs", "4", "--rollout_episodes", "--advantage", "gae", "--ppo_target_kl", "0.01"],
     "--ppo_target_kl"),
    (["--algo", "mfac", "--envs", "4", "--rollout_episodes", "--advantage", "gae", "--objective", "ppo", "--ppo_clip", "0"],
     "--ppo_clip"),
    (["--algo", "mfac", "--envs", "4", "--rollout_episodes", "--advantage", "gae", "--objective", "ppo", "--ppo_clip",
      "nan"], "--ppo_clip"),
    (["--algo", "mfac", "--envs", "4", "--rollout_episodes", "--advantage", "gae", "--objective", "ppo", "--ppo_clip",
      "inf"], "--ppo_clip"),
    (["--algo", "ac", "--envs", "4", "--rollout_episodes", "--advantage", "gae", "--objective", "ppo", "--ppo_epochs", "0"],
     "--ppo_epochs"),
    (["--algo", "ac", "--envs", "4", "--rollout_episodes", "--advantage", "gae", "--objective", "ppo", "--ppo_minibatches",
      "0"], "--ppo_minibatches"),
    (["--algo", "ac", "--envs", "4", "--rollout_episodes", "--advantage", "gae", "--objective", "ppo", "--ppo_target_kl",
      "-0.5"], "--ppo_target_kl"),
    (["--algo", "ac", "--envs", "4", "--rollout_episodes", "--advantage", "gae", "--objective", "ppo", "--ppo_target_kl",
      "nan"], "--ppo_target_kl"),
    (["--algo", "ac", "--envs", "4", "--rollout_episodes", "--advantage", "gae", "--objective", "trpo"], "--objective"),
])
def test_train_battle_refuses(argv, msg, capsys, monkeypatch):
    """Every refusal is parser.error (exit status 2), before the env -- and so any model -- is made."""
    import magent
    from mfrl_amd import train_battle

    def no_env(*a, **k):
        raise AssertionError("the env was made before the refusal")
    monkeypatch.setattr(magent, "GridWorld", no_env)
    with pytest.raises(SystemExit) as ex:
        train_battle.main(argv)
    assert ex.value.code == 2
    assert msg in capsys.readouterr().err


def test_the_header_declares_the_three_entry_points():
    from mfrl_amd import abi
    protos = abi.prototypes()
    VP = ctypes.c_void_p
    assert protos["mfx_actrain_set_ppo"] == (ctypes.c_int, [VP, VP, ctypes.c_double, VP])
    assert protos["mfx_actrain_ppo_stats"] == (ctypes.c_int, [VP, VP, VP])
    assert protos["mfx_policy_logp"] == (ctypes.c_int, [VP, VP, ctypes.c_longlong, ctypes.c_int, VP, VP])
    assert len(abi.fields(abi._header()[1]["mfx_actrain_rows"], abi._header()[1], "mfx_actrain_rows")) == 5
