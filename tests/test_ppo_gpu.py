"""The PPO objective of the actor-critic models on the GPU (csrc/ppo_kernels.hip, the PPO loss head k_at_loss_ppo of
csrc/actrain_kernels.hip, ActorCritic.objective = "ppo").

mfx_policy_logp straight through the C ABI against float64.  The loss head with logp_old / clip against torch in
float64 on rows of all three kinds (inside the clip range, clipped, outside on the harmless side), torch's own f32
error as the yardstick (tests/test_actrain_gpu.py's margin); its exact reductions on one handle (ratio 1: the
advantage-column head; every row clipped: that head with a zero column; null: the default head); the refusals.  End to
end on rows a linked collector left ("few" plan, 25 scripted steps): train_rollout under "ppo" on both backends --
step=False against float64, a full round against a manual loop of the same steps bit for bit, ppo_target_kl, what the
round leaves behind, and a model set to "ppo" and back.  Driver: play_rollout_episodes under "ppo".

ACTRAIN_ERROR_OUT=<path>: the loss-head tests append their measured figures there (profiles/ppo_error.jsonl is such a
run)."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest

import actrain_ref as ar
import common
import ppo_ref

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p
CLIP = 0.2


# ------------------------------------------------------------------------------------------------- mfx_policy_logp
def _abi():
    dll = ctypes.CDLL(common.HIP_LIB)
    dll.mfx_policy_logp.restype = ctypes.c_int
    dll.mfx_policy_logp.argtypes = [P, P, ctypes.c_longlong, ctypes.c_int, P, P]
    dll.mfx_last_error.restype = ctypes.c_char_p
    return dll


def _policy(n, A, seed):
    """A clamped f32 policy [n, A] as the forward leaves it (some rows nearly one-hot: entries at the clamp's floor)
    and actions covering 0 and A - 1."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, A)) * rng.choice([1.0, 30.0], size=(n, 1))
    e = np.exp(z - z.max(1, keepdims=True))
    p = np.clip((e / e.sum(1, keepdims=True)).astype(np.float32), np.float32(ar.LO), np.float32(ar.HI))
    act = rng.integers(0, A, size=n).astype(np.int32)
    act[0], act[-1] = 0, A - 1
    return np.ascontiguousarray(p), act


@pytest.mark.parametrize("A", [2, 21, 32])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_policy_logp(n, A):
    """|lp - lp64| <= 4 x 2^-24 x max(1, |lp64|): the 3-ulp bound of OpenCL's log plus the one rounding of p + 1e-6f;
    two calls give the same bits.  n = 1 .. 257: one lane, one workgroup short of full, full, one lane in a second;
    70001: 274 workgroups, the last ragged."""
    import torch
    dll = _abi()
    st = P(torch.cuda.current_stream().cuda_stream)
    p, act = _policy(n, A, 1000 * A + n)
    d_p, d_a = torch.from_numpy(p).cuda(), torch.from_numpy(act).cuda()
    outs = []
    for _ in range(2):
        out = torch.full((n + 1,), -7.0, dtype=torch.float32, device="cuda")
        assert dll.mfx_policy_logp(P(d_p.data_ptr()), P(d_a.data_ptr()), n, A, P(out.data_ptr()), st) == 0
        outs.append(out.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes() and outs[0][n] == -7.0
    lp64 = np.log(p[np.arange(n), act].astype(np.float64) + ar.EPS)
    err = np.abs(outs[0][:n].astype(np.float64) - lp64)
    bound = 4.0 * 2.0 ** -24 * np.maximum(1.0, np.abs(lp64))
    print("n", n, "A", A, "max err / bound", float((err / bound).max()), "min lp", float(lp64.min()))
    assert (err <= bound).all()


def test_policy_logp_bad_actions_and_arguments():
    """A row whose action is outside [0, A) gets +0, its neighbours their values; n = 0 does nothing; n_action outside
    2..32 is refused."""
    import torch
    dll = _abi()
    st = P(torch.cuda.current_stream().cuda_stream)
    n, A = 257, 21
    p, act = _policy(n, A, 5)
    good = act.copy()
    bad_rows = [0, 3, 255, 256]
    act[bad_rows] = [-1, A, 2 ** 31 - 1, -2 ** 31]
    d_p = torch.from_numpy(p).cuda()
    got = []
    for a in (act, good):
        d_a = torch.from_numpy(a).cuda()
        out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
        assert dll.mfx_policy_logp(P(d_p.data_ptr()), P(d_a.data_ptr()), n, A, P(out.data_ptr()), st) == 0
        got.append(out.cpu().numpy())
    assert not got[0][bad_rows].view(np.uint32).any()                       # +0 exactly
    keep = np.setdiff1d(np.arange(n), bad_rows)
    # (a good row is never 0: p = 1 gives log(1 + 1e-6) > 0)
    assert got[0][keep].tobytes() == got[1][keep].tobytes() and np.isfinite(got[1]).all() and (got[1] != 0).all()
    out = torch.full((4,), -7.0, dtype=torch.float32, device="cuda")
    assert dll.mfx_policy_logp(P(d_p.data_ptr()), P(d_a.data_ptr()), 0, A, P(out.data_ptr()), st) == 0
    for bad_A in (1, 33, 0, -3):
        assert dll.mfx_policy_logp(P(d_p.data_ptr()), P(d_a.data_ptr()), 4, bad_A, P(out.data_ptr()), st) == -1
        assert b"n_action" in dll.mfx_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all()


def test_the_wrapper():
    import torch
    from mfrl_amd import replay
    p, act = _policy(300, 21, 9)
    out = torch.zeros(300, dtype=torch.float32, device="cuda")
    back = replay.policy_logp(torch.from_numpy(p).cuda(), torch.from_numpy(act).cuda(), out)
    assert back.data_ptr() == out.data_ptr()
    lp64 = np.log(p[np.arange(300), act].astype(np.float64) + ar.EPS)
    assert np.abs(out.cpu().numpy() - lp64).max() <= 4.0 * 2.0 ** -24 * np.abs(lp64).max()


# ------------------------------------------------------------------------------------------------- the loss head
def _head_inputs(case, seed, n):
    """rows, the non-zero random advantage column, and lp_old = f32(lp64 - log t): t per row from U(1 - clip / 2, 1 +
    clip / 2), U(1 + 2 clip, 1 + 4 clip), U(1 - 4 clip, 1 - 2 clip), a third of the rows each.  The preconditions are
    asserted on the float64 reference: no ratio within 1e-3 of a bound (the head is discontinuous there), and clipped
    and unclipped rows of either sign."""
    V, F, A, use_mf = case
    rows = ar.rows(V, F, A, use_mf, seed, n)
    adv = (2.5 * np.random.RandomState(77).randn(n)).astype(np.float32)
    assert (adv != 0).all()
    k = ar.reference(V, F, A, use_mf, seed, n)[2]
    lp64 = ppo_ref.logp(k["s"], rows["act"])
    rng = np.random.default_rng(100 + n)
    kind = np.arange(n) % 3
    t = np.where(kind == 0, rng.uniform(1 - CLIP / 2, 1 + CLIP / 2, n),
                 np.where(kind == 1, rng.uniform(1 + 2 * CLIP, 1 + 4 * CLIP, n), rng.uniform(1 - 4 * CLIP, 1 - 2 * CLIP, n)))
    lp_old = (lp64 - np.log(t)).astype(np.float32)
    r64 = np.exp(lp64 - lp_old.astype(np.float64))
    lo, hi = ppo_ref.bounds(CLIP)
    assert min(np.abs(r64 - lo).min(), np.abs(r64 - hi).min()) >= 1e-3
    cl = ppo_ref.clipped_mask(adv, r64, CLIP)
    for sign in (adv > 0, adv < 0):
        assert (cl & sign).any() and (~cl & sign).any()
    return rows, adv, lp_old, k, cl, r64


def _ppo_head(case, seed, n, chunk):
    """Per block of the blob e = max |g - g64| / max |g64| of ACTrainHIP.grads with adv, logp_old and clip against the
    same loss in torch float64; e_hip <= 4 e_torch, torch's own f32 gradient of that loss.  The stats within 1e-4
    max(1, |x64|), approx_kl likewise, clip_frac the reference's count exactly, logp_new the reference's log-prob to the
    f32 forward's error, padding +0."""
    import torch
    from test_actrain_gpu import dev_rows, handle
    V, F, A, use_mf = case
    rows, adv, lp_old, k, cl, r64 = _head_inputs(case, seed, n)
    _, (nb, off) = ar.packed(V, F, A, use_mf, seed)
    net = ar.net(V, F, A, use_mf, seed)
    named64, stats64, extra64 = ppo_ref.torch_gradient(net, rows, adv, lp_old, CLIP, torch.float64, "cuda")
    named32, _, _ = ppo_ref.torch_gradient(net, rows, adv, lp_old, CLIP, torch.float32, "cuda")
    g64, g32 = (ar.pack64(x, V, F, A, use_mf, off, nb) for x in (named64, named32))
    ref = ppo_ref.head(k["z"], k["v"], rows["act"], rows["ret"], adv, lp_old, CLIP)
    assert np.array_equal(ref["clipped"], cl) and abs(ref["approx_kl"] - extra64[1]) <= 1e-9
    assert abs(extra64[0] * n - cl.sum()) < 1e-6
    tr = handle(case, seed, chunk_rows=chunk)
    cols = dev_rows(rows)
    cols["adv"] = torch.from_numpy(adv).cuda()
    cols["logp_old"] = torch.from_numpy(lp_old).cuda()
    cols["logp_new"] = torch.full((n + 1,), -7.0, dtype=torch.float32, device="cuda")
    g, stats = tr.grads(cols, n, clip=CLIP)
    extra = tr.ppo_stats().cpu().numpy()
    tr.check_error()
    g, stats = g.cpu().numpy(), stats.cpu().numpy()
    e_hip, e_torch = ar.block_errors(g, g64, off, nb), ar.block_errors(g32, g64, off, nb)
    rec = {"tag": "ppo-head", "V": V, "F": F, "A": A, "use_mf": use_mf, "n": n, "e_hip": [e[0] for e in e_hip],
           "e_torch": [e[0] for e in e_torch], "stats": [float(x) for x in stats], "stats64": list(stats64),
           "clip_frac": float(extra[0]), "approx_kl": float(extra[1]), "clipped": int(cl.sum()), "approx_kl64": extra64[1],
           "max_ratio": max(e_hip[j][0] / e_torch[j][0] for j in range(19) if e_torch[j][0] > 0)}
    print(json.dumps(rec))
    if os.environ.get("ACTRAIN_ERROR_OUT"):
        with open(os.environ["ACTRAIN_ERROR_OUT"], "a") as f:
            f.write(json.dumps(rec) + "\n")
    pad = ar.padding_mask(off, V, F, A, use_mf, nb)
    assert np.all(g[pad].view(np.uint32) == 0)
    for j in range(19):
        if j in ar.empty_blocks(use_mf):
            continue
        assert e_hip[j][1] > 0, j
        assert e_hip[j][0] <= 4.0 * e_torch[j][0], (j, e_hip[j][0], e_torch[j][0])
    for x, x64 in zip(stats, stats64):
        assert abs(float(x) - x64) <= 1e-4 * max(1.0, abs(x64)), (stats, stats64)
    assert abs(float(extra[0]) * n - cl.sum()) < 1e-3 and round(float(extra[0]) * n) == int(cl.sum())
    assert float(extra[0]) == float(np.float32(cl.sum() / n))
    assert abs(float(extra[1]) - extra64[1]) <= 1e-4 * max(1.0, abs(extra64[1])), (extra, extra64)
    lp_new = cols["logp_new"].cpu().numpy()
    assert lp_new[n] == -7.0
    assert np.abs(lp_new[:n] - ref["lp"]).max() <= 1e-4 * max(1.0, np.abs(ref["lp"]).max())
    return tr, cols, rows, adv, g, stats


@pytest.mark.parametrize("use_mf", [False, True], ids=["ac", "mfac"])
def test_ppo_head(use_mf):
    """At the Battle shape: 300 rows at chunk_rows = 128 -- three chunks, the last ragged (44 rows), so the three columns
    are read (and logp_new written) at each chunk's row offset and both partial buffers add up over the workgroups of
    several launches.  Then, on the same handle, the head's exact reductions:
    (a) logp_old := the logp_new column the head wrote: d = 0 and r = 1 in every row, so the gradient and the value,
        entropy and mean-value stats are bitwise the advantage-column head's, and (clip_frac, approx_kl) is exactly
        (0, 0).  The policy stat is the mean of -adv r = -adv now, not of -adv lp: it is judged against float64.
    (b) logp_old := logp_new - 1 with adv > 0 everywhere: every row is clipped (r = e), the gradient is bitwise the
        advantage-column head's on an all-zero column, clip_frac is exactly 1.
    (c) logp_old := None restores the fresh handle's default gradient bit for bit."""
    import torch
    from test_actrain_gpu import dev_rows, handle, same_bits
    case = tuple(ar.BATTLE) + (use_mf,)
    n, chunk = 300, 128
    tr, cols, rows, adv, g_ppo, _ = _ppo_head(case, 11, n, chunk)
    plain = {k: v for k, v in cols.items() if k not in ("logp_old", "logp_new")}
    g_adv, s_adv = (x.cpu().numpy() for x in tr.grads(plain, n))
    assert not same_bits(g_adv, g_ppo)
    # (a)
    lp_self = cols["logp_new"][:n].clone()
    again = dict(plain, logp_old=lp_self, logp_new=torch.empty(n, dtype=torch.float32, device="cuda"))
    g_a, s_a = (x.cpu().numpy() for x in tr.grads(again, n, clip=CLIP))
    assert same_bits(g_a, g_adv) and same_bits(s_a[1:], s_adv[1:])
    assert torch.equal(again["logp_new"], lp_self)
    assert not tr.ppo_stats().cpu().numpy().view(np.uint32).any()           # (+0, +0)
    want_pg = -float(adv.astype(np.float64).mean())
    assert abs(float(s_a[0]) - want_pg) <= 1e-4 * max(1.0, abs(want_pg))
    # (b)
    up = dict(plain, adv=cols["adv"].abs(), logp_old=lp_self - 1.0)
    g_b = tr.grads(up, n, clip=CLIP)[0].cpu().numpy()
    frac, kl = tr.ppo_stats().cpu().tolist()
    g_zero = tr.grads(dict(plain, adv=torch.zeros_like(cols["adv"])), n)[0].cpu().numpy()
    assert same_bits(g_b, g_zero) and frac == 1.0 and abs(kl - (np.e - 2.0)) < 1e-4
    # (c)
    g_back = tr.grads(dict(plain, adv=None), n)[0].cpu().numpy()
    g_fresh = handle(case, 11, chunk_rows=chunk).grads(dev_rows(rows), n)[0].cpu().numpy()
    assert same_bits(g_back, g_fresh) and not same_bits(g_back, g_adv)
    tr.check_error()


@pytest.mark.parametrize("case", [(47, 37, 2, True), (4096, 256, 20, False)], ids=["47-37-2-mf", "4096-256-20"])
def test_ppo_head_off_the_battle_shape(case):
    """The same head at two of test_actrain_gpu.OFF_SHAPE's shapes, 20 rows (one chunk)."""
    from test_actrain_gpu import OFF_SHAPE
    assert case in OFF_SHAPE
    _ppo_head(case, 11, 20, None)


@pytest.mark.parametrize("clip", [0.0, -0.1, float("nan"), float("inf")])
def test_a_bad_clip_is_refused_before_any_launch(clip):
    import torch
    from mfrl_amd import EngineError, lib
    from test_actrain_gpu import dev_rows, handle, same_bits, states
    case = tuple(ar.BATTLE) + (False,)
    rows = ar.rows(*case, 11, 20)
    tr = handle(case, 11)
    cols = dev_rows(rows)
    cols["adv"] = torch.ones(20, device="cuda")
    cols["logp_old"] = torch.zeros(20, device="cuda")
    before = states(tr)
    with pytest.raises(EngineError, match="clip"):
        tr.step(cols, 20, clip=clip)
    assert b"clip" in lib().mfx_last_error()
    torch.cuda.synchronize()
    assert same_bits(states(tr), before) and tr.step_count() == 0
    tr.check_error()


def test_ppo_without_an_advantage_column_is_refused_before_any_launch():
    import torch
    from mfrl_amd import EngineError, lib
    from test_actrain_gpu import dev_rows, handle, same_bits, states
    case = tuple(ar.BATTLE) + (True,)
    rows = ar.rows(*case, 11, 20)
    tr = handle(case, 11)
    cols = dev_rows(rows)
    cols["logp_old"] = torch.zeros(20, device="cuda")
    before = states(tr)
    for call in (tr.step, tr.grads):
        with pytest.raises(EngineError, match="advantage"):
            call(cols, 20, clip=CLIP)
        assert b"advantage" in lib().mfx_last_error() and b"d_logp_old" in lib().mfx_last_error()
    torch.cuda.synchronize()
    assert same_bits(states(tr), before) and tr.step_count() == 0
    # ... and the next call without the column is the default head's, as if nothing had been set
    del cols["logp_old"]
    g = tr.grads(cols, 20)[0].cpu().numpy()
    assert same_bits(g, handle(case, 11).grads(dev_rows(rows), 20)[0].cpu().numpy())


# ------------------------------------------------------------------------------------------------- end to end
_STATE0 = {}


class _Ppo:
    """test_gae_gpu's collected rows and model (shared with its tests), set to "gae" + "ppo" with two passes of three
    segments; leave() puts the model back as it was found: weights, optimiser, trainer, modes."""

    def __init__(self, algo):
        import torch
        from test_gae_gpu import _collected
        self.s = s = _collected(algo)
        self.m = m = s.model
        if algo not in _STATE0:
            _STATE0[algo] = copy.deepcopy(m.net.state_dict())
        self.reset()
        m.advantage = "gae"
        m.objective = "ppo"
        m.ppo_clip, m.ppo_epochs, m.ppo_minibatches, m.ppo_target_kl = CLIP, 2, 3, None
        self.eng = m._rollout_collector.eng
        self.torch = torch

    def reset(self):
        """The collected weights, a fresh torch optimiser, and no HIP trainer (the next one starts at step 0 with zero
        moments, like a manual handle made beside it)."""
        m = self.m
        m.net.load_state_dict(_STATE0[self.s.algo])
        m.reset_optimizer()
        self.s.restore()

    def leave(self):
        m = self.m
        m.objective = "pg"
        m.ppo_clip, m.ppo_epochs, m.ppo_minibatches, m.ppo_target_kl = 0.2, 4, 4, None
        m.adv_norm = False
        m.advantage = "returns"
        m.gae_lambda = 0.95
        self.reset()

    def prepared(self, backend):
        """One step=False round: -> (gradients, the reward / advantage / logp_old columns the preparation left)."""
        m, n = self.m, self.s.n
        g, ret = self.s.run(backend, chunk_rows=600 if backend == "hip" else None)
        return g, ret, m._gae_adv[:n].clone(), m._ppo_logp[:n].clone()

    def segments(self):
        from mfrl_amd.replay import ppo_order
        m, n = self.m, self.s.n
        M = min(m.ppo_minibatches, n)
        return [(k * n // M, (k + 1) * n // M) for e in range(m.ppo_epochs) for k in ppo_order(m.seed, m.ppo_rounds, e, M)]


def _losses64(p, ret, adv, logp):
    """_Collected.losses64 with the PPO columns: (g64, g32) of ActorCritic.losses on the collected rows in one piece."""
    import torch
    s, m = p.s, p.m
    c, n = s.c, s.n
    prob = c["prob"][:n] if s.use_mf else None
    net32 = m.net
    total = sum(m.losses(c["obs"][:n], c["feat"][:n], c["act"][:n], ret, prob, adv=adv, logp_old=logp, clip=CLIP)[:3])
    g32 = [g.detach().clone() for g in torch.autograd.grad(total, list(net32.parameters()))]
    m.net = copy.deepcopy(net32).double()
    try:
        total64 = sum(m.losses(c["obs"][:n].double(), c["feat"][:n].double(), c["act"][:n], ret.double(),
                               prob.double() if s.use_mf else None, adv=adv.double(), logp_old=logp.double(),
                               clip=CLIP)[:3])
        g64 = [g.detach().clone() for g in torch.autograd.grad(total64, list(m.net.parameters()))]
    finally:
        m.net = net32
    return g64, g32


@pytest.mark.parametrize("algo", ["ac", "mfac"])
def test_train_rollout_step_false_under_ppo(algo, capsys):
    """step=False on both backends: the gradient of the whole round as one minibatch at the unchanged weights, against
    the float64 gradient of losses(..., logp_old = the column the model built, clip), e <= 4 e_torch.  The column is
    replay.policy_logp of the f32 forward's policy on the collected rows, bit for bit; the reward and advantage columns
    are GAE's; the printed line carries the new fields and 0 steps."""
    import torch
    from mfrl_amd import replay
    p = _Ppo(algo)
    try:
        s, m, n, c = p.s, p.m, p.s.n, p.s.c
        m.objective = "pg"
        _, ret_gae = s.run("hip")
        adv_gae = m._gae_adv[:n].clone()
        m.objective = "ppo"
        rounds = m.ppo_rounds
        got = {b: p.prepared(b) for b in ("torch", "hip")}
        out = capsys.readouterr().out
        assert out.count("/ CLIP_FRAC: 0.0 / KL:") == 2 and out.count("chains, 0 steps)") == 2
        (g_t, ret, adv, logp), (g_h, ret_h, adv_h, logp_h) = got["torch"], got["hip"]
        assert torch.equal(ret, ret_h) and torch.equal(adv, adv_h) and torch.equal(logp, logp_h)
        assert torch.equal(ret, ret_gae) and torch.equal(adv, adv_gae)
        with torch.no_grad():
            pol, _, _ = m._hip_net().forward(c["obs"][:n], c["feat"][:n], c["prob"][:n] if s.use_mf else None,
                                             want_policy=True, want_value=True, want_act=False)
            want = replay.policy_logp(pol, c["act"][:n], torch.empty(n, dtype=torch.float32, device="cuda"))
        assert torch.equal(want, logp) and bool(torch.isfinite(logp).all()) and bool((logp != 0).all())
        g64, g32 = _losses64(p, ret, adv, logp)
        s.judge(g_t, g64, g32, "ppo-step-false-torch")
        s.judge(g_h, g64, g32, "ppo-step-false-hip")
        assert m.ppo_rounds == rounds                           # (a gradient is no round: the order's key is not advanced)
    finally:
        p.leave()


@pytest.mark.parametrize("algo", ["ac", "mfac"])
def test_a_full_round_on_the_hip_backend(algo, capsys):
    """ppo_epochs = 2, ppo_minibatches = 3: the trainer's final parameters are bitwise those of a manual loop of
    ACTrainHIP.step over the same slices in ppo_order's order from the same state, and its step count advanced by 6;
    ppo_target_kl = 0 stops after the first pass (3 steps).  After the round: the buffer is cleared, the reward column
    is GAE's adv + value, the network holds the trainer's parameters, the acting handle's policy on 64 of the rows is
    bitwise a fresh ACNetHIP's loaded from model.net, and np.random was not drawn from."""
    import torch
    from mfrl_amd import actrain
    from mfrl_amd.policy import ACNetHIP
    p = _Ppo(algo)
    try:
        s, m, n, c = p.s, p.m, p.s.n, p.s.c
        _, ret, adv, logp = p.prepared("hip")
        cols = {"obs": c["obs"], "feat": c["feat"], "act": c["act"], "ret": ret, "prob": c["prob"] if s.use_mf else None,
                "adv": adv, "logp_old": logp}
        segs = p.segments()
        assert len(segs) == 6 and sorted(segs[:3]) == sorted(segs[3:]) == [(0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)]

        def manual(steps):
            tr = actrain.ACTrainHIP(m.view_space, m.feature_space, m.num_actions, s.use_mf, lr=m.learning_rate,
                                    value_coef=m.value_coef, ent_coef=m.ent_coef)
            tr.load(m.net)
            tr.set_input_support(p.eng.view_support(0))
            kls = []
            for a, b in segs[:steps]:
                tr.step({k: (t[a:b] if t is not None else None) for k, t in cols.items()}, b - a, clip=CLIP)
                kls.append(tr.ppo_stats())
            tr.check_error()
            return tr.get_state(actrain.PARAMS), torch.stack(kls).cpu().numpy()

        want6, st6 = manual(6)
        want3, _ = manual(3)
        assert not torch.equal(want6, want3)
        assert (st6[3:, 1] > 0).all() and st6[0, 0] == 0.0     # the first step is at ratio 1; later ones have moved
        for target, steps, want in ((None, 6, want6), (0.0, 3, want3)):
            p.reset()
            m.ppo_target_kl = target
            m.train_backend = "hip"
            rounds, np_state = m.ppo_rounds, np.random.get_state()
            capsys.readouterr()
            assert m.train_rollout() is None
            out = capsys.readouterr().out
            assert "/ CLIP_FRAC:" in out and "/ KL:" in out and "chains, %d steps)" % steps in out
            assert m.ppo_rounds == rounds + 1
            m.ppo_rounds = rounds                              # (the manual loops above used this round's orders)
            after = np.random.get_state()
            assert np_state[0] == after[0] and np.array_equal(np_state[1], after[1]) and np_state[2:] == after[2:]
            tr = m._hip_trainer()
            assert tr.step_count() == steps
            assert torch.equal(tr.get_state(actrain.PARAMS), want), (target, steps)
            assert s.rows.n == 0
            assert torch.equal(c["rew"][:n], ret)
            fresh = copy.deepcopy(m.net)
            tr.export(fresh)
            assert all(torch.equal(a, b) for a, b in zip(fresh.parameters(), m.net.parameters()))
            assert any(not torch.equal(a, b) for a, b in zip(m.net.parameters(), _STATE0[algo].values()))
            prob = c["prob"][:64] if s.use_mf else None
            with torch.no_grad():
                key = m._hip_key
                got_pol = m._hip_net().forward(c["obs"][:64], c["feat"][:64], prob, want_policy=True, want_act=False)[0]
                assert m._hip_key == key                       # (nothing was re-packed: the blob came device to device)
                ref_net = ACNetHIP(m.view_space, m.feature_space, m.num_actions, s.use_mf)
                ref_net.load(m.net)
                want_pol = ref_net.forward(c["obs"][:64], c["feat"][:64], prob, want_policy=True, want_act=False)[0]
            assert torch.equal(got_pol, want_pol)
    finally:
        p.leave()


@pytest.mark.parametrize("algo", ["ac", "mfac"])
def test_a_full_round_on_the_torch_backend(algo, capsys):
    """The same round on torch autograd: the parameters are bitwise those of a manual loop over model.losses with a
    copied net and a fresh Adam (the manual loop, run twice, repeats itself bit for bit first); ppo_target_kl = 0
    takes 3 of the 6 steps."""
    import torch
    p = _Ppo(algo)
    try:
        s, m, n, c = p.s, p.m, p.s.n, p.s.c
        _, ret, adv, logp = p.prepared("torch")
        segs = p.segments()
        prob = c["prob"] if s.use_mf else None

        def manual(steps):
            keep = m.net
            m.net = net = copy.deepcopy(keep)
            opt = torch.optim.Adam(net.parameters(), lr=m.learning_rate)
            try:
                for a, b in segs[:steps]:
                    opt.zero_grad(set_to_none=True)
                    pg, vf, ent = m.losses(c["obs"][a:b], c["feat"][a:b], c["act"][a:b], ret[a:b],
                                              prob[a:b] if prob is not None else None, total_rows=b - a, adv=adv[a:b],
                                              logp_old=logp[a:b], clip=CLIP)[:3]
                    (pg + vf + ent).backward()
                    opt.step()
            finally:
                m.net = keep
            return [q.detach().clone() for q in net.parameters()]

        want6, again6, want3 = manual(6), manual(6), manual(3)
        assert all(torch.equal(a, b) for a, b in zip(want6, again6))
        for target, steps, want in ((None, 6, want6), (0.0, 3, want3)):
            p.reset()
            m.ppo_target_kl = target
            m.train_backend = "torch"
            rounds, np_state = m.ppo_rounds, np.random.get_state()
            capsys.readouterr()
            assert m.train_rollout() is None
            out = capsys.readouterr().out
            assert "/ CLIP_FRAC:" in out and "/ KL:" in out and "chains, %d steps)" % steps in out
            m.ppo_rounds = rounds
            after = np.random.get_state()
            assert np_state[0] == after[0] and np.array_equal(np_state[1], after[1]) and np_state[2:] == after[2:]
            assert all(torch.equal(a, b) for a, b in zip(m.net.parameters(), want)), (target, steps)
            assert int(m.optimizer.state[next(m.net.parameters())]["step"]) == steps
            assert s.rows.n == 0 and torch.equal(c["rew"][:n], ret)
            assert all(q.grad is None for q in m.net.parameters())
    finally:
        p.leave()


@pytest.mark.parametrize("algo", ["ac", "mfac"])
def test_ppo_and_back_leaves_no_trace(algo):
    """A model set to "ppo" (a gradient taken and a full round trained on both backends) and back to "pg" / "returns"
    at its old weights: the reward column and the gradients are the untouched model's, bit for bit (torch's when torch
    itself repeats its gradient on these rows, as in test_gae_gpu)."""
    import torch
    p = _Ppo(algo)
    try:
        s, m = p.s, p.m
        for backend in ("torch", "hip"):
            p.prepared(backend)
            p.reset()
            m.train_backend = backend
            m.train_rollout()
        p.leave()
        assert (m.objective, m.advantage) == ("pg", "returns")
        for backend in ("torch", "hip"):
            g, ret = s.run(backend)
            g0, ret0 = s.base[backend]
            assert torch.equal(ret, ret0), backend
            same = all(torch.equal(a, b) for a, b in zip(g, g0))
            if backend == "hip":
                assert same
            else:
                repeats = all(torch.equal(a, b) for a, b in zip(s.base["torch"][0], s.base["torch2"][0]))
                print("torch repeats its own gradient bit for bit:", repeats)
                assert same or not repeats
    finally:
        p.leave()


# ------------------------------------------------------------------------------------------------- the driver
@pytest.mark.parametrize("backend", ["torch", "hip"])
@pytest.mark.parametrize("algo", ["mfac", "ac"])
def test_play_rollout_episodes_trains_under_ppo(algo, backend, capsys):
    """Two rounds of play_rollout_episodes (40x40, 2 envs, 10 steps, train) under "gae" + adv_norm + "ppo" (2 x 2
    steps): it prints the new line once per round, the main model's parameters moved and are finite, the opponent's did
    not move, the rows are empty afterwards and round two runs on the same storage."""
    import torch
    import test_collect_ac_gpu as tc
    from mfrl_amd.algo import spawn_ai
    from mfrl_amd.algo.play import play_rollout_episodes
    from mfrl_amd.battle import BattleBatch
    map_size, E, max_steps = 40, 2, 10
    me, env = tc._model(algo, algo + "-0", max_steps)
    other = spawn_ai(algo, None, env, env.get_handles()[1], algo + "-1", max_steps)
    for m in (me, other):
        m.train_backend = backend
        m.advantage = "gae"
        m.adv_norm = True
        m.objective = "ppo"
        m.ppo_epochs = m.ppo_minibatches = 2
    eng = BattleBatch(map_size, E, stream=torch.cuda.current_stream())
    before = [q.detach().clone() for q in me.net.parameters()]
    oppo = [q.detach().clone() for q in other.net.parameters()]
    buf = me.replay_buffer
    seen = []
    for k in range(2):
        play_rollout_episodes(eng, k, map_size, max_steps, [me, other], eps=1.0, train=True, left_id=0)
        assert me.replay_buffer is buf and buf._rows.n == 0
        seen.append((buf._rows.cap, me._gae_value.data_ptr(), me._gae_adv.data_ptr(), me._ppo_logp.data_ptr(),
                     me._ppo_logp.numel()))
        if k == 0:
            mid = [q.detach().clone() for q in me.net.parameters()]
    assert seen[0][4] >= seen[0][0] >= E * 64 * max_steps and seen[1] == seen[0]
    after = list(me.net.parameters())
    assert all(bool(torch.isfinite(q).all()) for q in after)
    assert any(not torch.equal(a, b) for a, b in zip(mid, before))
    assert any(not torch.equal(a, b) for a, b in zip(after, mid))
    assert all(torch.equal(a, b) for a, b in zip(other.net.parameters(), oppo))
    out = capsys.readouterr().out
    assert out.count("[*] PG_LOSS:") == 2 and out.count("/ CLIP_FRAC:") == 2 and out.count("chains, 4 steps)") == 2
    assert me.ppo_rounds == 2 and other.ppo_rounds == 0
