"""The float64 restatement of the actor-critic training step (tests/actrain_ref.py) against torch's float64 autograd,
the preconditions of the inputs the GPU tests use (tests/test_actrain_gpu.py), pack / unpack, and the CLI refusal.
No GPU."""
import numpy as np
import pytest
import torch

import actrain_ref as ar

V, F, A = ar.BATTLE
OFF_SHAPE = [(47, 37, 2, True), (1196, 1, 32, True), (4096, 256, 20, False), (17, 36, 21, False)]
# (V, F, A, use_mf, seed, n, policy_scale) of every input set the GPU tests take a gradient of
GPU_CASES = ([(V, F, A, mf, seed, n, 1.0) for mf in (False, True) for seed in (11, 12) for n in (1, 20, 272)] +
             [(V, F, A, mf, 11, 700, 1.0) for mf in (False, True)] +
             [(V, F, A, mf, ar.CLAMP_SEED, ar.CLAMP_N, ar.POLICY_SCALE) for mf in (False, True)] +
             [c + (11, 20, 1.0) for c in OFF_SHAPE])
FLOOR = 1e-3


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("scale", [1.0, ar.POLICY_SCALE])
@pytest.mark.parametrize("use_mf", [False, True])
def test_restatement_is_torch_float64(use_mf, scale):
    """Per block of the blob, the numpy gradient equals torch's float64 autograd of ActorCritic.losses' formula to
    1e-10 relative; the stats likewise."""
    n = 40
    blob, (nb, off) = ar.packed(V, F, A, use_mf, 11, scale)
    rows = ar.rows(V, F, A, use_mf, 11, n)
    g, stats = ar.gradient(blob, off, V, F, A, use_mf, rows)
    named, t_stats = ar.torch_gradient(ar.net(V, F, A, use_mf, 11, scale), rows, torch.float64)
    g_t = ar.pack64(named, V, F, A, use_mf, off, nb)
    ends = list(off[1:]) + [nb]
    for k, (o, e) in enumerate(zip(off, ends)):
        if k in ar.empty_blocks(use_mf):
            assert e == o
            continue
        assert np.abs(g_t[o:e]).max() > 0, k
        assert _rel(g[o:e], g_t[o:e]) <= 1e-10, (k, _rel(g[o:e], g_t[o:e]))
    for x, y in zip(stats, t_stats):
        assert abs(x - y) <= 1e-10 * max(1.0, abs(y))
    pad = ar.padding_mask(off, V, F, A, use_mf, nb)
    assert np.all(g[pad] == 0) and np.all(blob[pad] == 0) and pad.sum() > 0


def test_chunk_formula_matches_model_losses():
    """torch_gradient's formula is ActorCritic.losses' (the model's own code, float32 on the CPU) on the same rows."""
    from mfrl_amd.algo.ac import ActorCritic
    net = ar.net(V, F, A, True, 11)
    rows = ar.rows(V, F, A, True, 11, 20)

    class M:
        num_actions, value_coef, ent_coef = A, ar.VALUE_COEF, ar.ENT_COEF
    M.net = net
    t = lambda x: torch.as_tensor(np.array(x))
    pg, vf, ent, value = ActorCritic.losses(M, t(rows["obs"]), t(rows["feat"]), t(rows["act"]), t(rows["ret"]),
                                            t(rows["prob"]))
    _, s = ar.torch_gradient(net, rows, torch.float32)
    got = tuple(float(x.detach()) for x in (pg, vf, ent, value.mean()))
    assert np.allclose(got, s, rtol=1e-5, atol=1e-6), (got, s)


@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_input_preconditions(case):
    """On the float64 forward: every non-empty block's max |g64| is at least FLOOR (the relative error of a block means
    something); no softmax entry lies within 1 % of the clamp's bound (f32 and f64 agree on the mask); the
    clamp-heavy case has at least 10 % of its entries on either side; the actions cover 0 and A - 1."""
    Vc, Fc, Ac, mf, seed, n, scale = case
    g, _, k = ar.reference(*case)
    _, (nb, off) = ar.packed(Vc, Fc, Ac, mf, seed, scale)
    for kk, (e, ref) in enumerate(ar.block_errors(g, g, off, nb)):
        if kk in ar.empty_blocks(mf):
            continue
        assert ref >= FLOOR, (kk, ref)
    assert ar.clamp_margin(k["s"]) > 0.01
    below = float((k["s"] < ar.LO).mean())
    if scale != 1.0:
        assert 0.1 <= below <= 0.9, below
    act = ar.rows(Vc, Fc, Ac, mf, seed, n)["act"]
    if n > 1:
        assert act.min() == 0 and act.max() == Ac - 1


@pytest.mark.parametrize("case", [(V, F, A, False), (V, F, A, True)] + OFF_SHAPE)
def test_unpack_is_the_inverse_of_pack(case):
    from mfrl_amd.algo.nets import ACNet
    from mfrl_amd.policy import pack_acnet, unpack_acnet
    Vc, Fc, Ac, mf = case
    src = ar.net(Vc, Fc, Ac, mf)
    blob = pack_acnet(src, Vc, Fc, Ac, mf)
    dst = ACNet((Vc,), (Fc,), Ac, use_mf=mf)
    unpack_acnet(blob, dst)
    for (ka, a), (kb, b) in zip(src.named_parameters(), dst.named_parameters()):
        assert ka == kb and a.detach().numpy().tobytes() == b.detach().numpy().tobytes(), ka
    assert pack_acnet(dst, Vc, Fc, Ac, mf).numpy().tobytes() == blob.numpy().tobytes()
    into = [torch.zeros_like(p) for p in src.parameters()]
    unpack_acnet(blob, src, into=into)
    for p, t in zip(src.parameters(), into):
        assert p.detach().numpy().tobytes() == t.numpy().tobytes()


def test_cli_refuses_ac_backend_for_q_models(capsys):
    from mfrl_amd import train_battle
    for algo in ("mfq", "il"):
        with pytest.raises(SystemExit):
            train_battle.main(["--algo", algo, "--ac_train_backend", "hip"])
        err = capsys.readouterr().err
        assert "--ac_train_backend hip trains the actor-critic network: --algo ac or mfac" in err
        assert "--train_backend hip" in err
