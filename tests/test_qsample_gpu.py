"""The opt-in Boltzmann acting mode of the Q models on the GPU (csrc/qsample.h): the stand-alone
k_q_sample on synthetic Q tables against the numpy restatement (tests/qsample_ref.py); the draw fused into the
epilogues of k_qnet_head / k_qb16_head against k_q_sample on the Q values they write; a sampled rollout replayed on
the C oracle; ValueNet.explore and the train_battle switch."""
import numpy as np
import pytest

import battle_driver as bd
import common
import qsample_ref as qs
from test_qsample_cpu import FREQ_N, FREQ_Q, freq_check

pytestmark = pytest.mark.gpu
VS, FS, NA = (13, 13, 7), (34,), 21


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ------------------------------------------------------------------------------------------------- 1: k_q_sample
def _table(n, A, T, seed):
    """n Q rows: the even rows decisive ((m - second) / T > 104: every weight but the maximum's is exactly 0), the odd
    ones cycling through ties, gaps of 0 / 1e-3 / 200, Q values on the scale of T, and the non-finite kinds."""
    rng = np.random.RandomState(seed)
    f = np.float32
    q = np.zeros((n, A), dtype=f)
    for i in range(n):
        if i % 2 == 0:
            top = rng.randint(A)
            q[i] = f(rng.uniform(-1, 1)) - f(T) * f(rng.uniform(110, 400, size=A))
            q[i, top] = q[i].max() + f(T) * f(rng.uniform(110, 130))
            continue
        k = (i // 2) % 11
        if k == 0:
            q[i] = f(rng.uniform(-2, 2))                             # every action tied
        elif k == 1:
            q[i] = f(rng.uniform(-2, 2)) - f(T) * rng.uniform(0.5, 3, size=A).astype(f)
            a, b = rng.choice(A, 2, replace=False)
            q[i, a] = q[i, b] = q[i].max() + f(T)                    # two tied maxima
        elif k in (2, 3, 4):
            gap = (0.0, 1e-3, 200.0)[k - 2]
            q[i] = f(rng.uniform(-1, 1)) + f(gap) * rng.permutation(A).astype(f)
        elif k in (5, 6):
            q[i] = (rng.randn(A) * T * (1.0, 4.0)[k - 5]).astype(f)
        elif k == 7:
            q[i] = rng.randn(A).astype(f)
            q[i, rng.randint(A)] = np.nan
        elif k == 8:
            q[i] = rng.randn(A).astype(f)
            q[i, rng.choice(A, 2, replace=False)] = np.inf           # two +inf: the first is the greedy action
        elif k == 9:
            q[i] = rng.randn(A).astype(f)
            q[i, rng.randint(A)] = -np.inf
        else:
            q[i] = np.nan                                            # all NaN: action 0
            if i % 4 == 1:
                q[i, 1:] = -np.inf                                   # NaN, then -inf everywhere: action 1
    return q


@pytest.mark.parametrize("T", [1e-3, 0.1, 1.0])
@pytest.mark.parametrize("n", [1, 63, 65, 1000])
@pytest.mark.parametrize("A", [2, 5, 21, 32])
def test_q_sample_matches_restatement(A, n, T):
    import torch
    from mfrl_amd import mf
    q = _table(n, A, T, 1000 * A + n)
    seed, step, group = 77 + A, 3 + n, n % 2
    act, w = mf.q_sample(_cuda(q), T, seed, step, group, want_w=True)
    torch.cuda.synchronize()
    act, w = act.cpu().numpy(), w.cpu().numpy()
    rows = np.arange(n)
    fin = qs.finite_rows(q)
    # every row: the restatement's draw on the kernel's own weights (non-finite rows: the greedy rule)
    assert np.array_equal(act, qs.sample(q, T, seed, step, group, rows, w=w))
    assert act.min() >= 0 and act.max() < A
    # finite rows: w / tot within 1e-5 of the float64 softmax
    p = w[fin].astype(np.float64)
    p /= p.sum(1, keepdims=True)
    err = np.abs(p - qs.softmax64(q[fin], T)).max()
    print("A %d n %d T %g: max |w / tot - softmax64| = %.3e" % (A, n, T, err))
    assert err <= 1e-5, err
    # non-finite rows: the first maximum, one-hot weights
    g = qs.greedy(q)
    assert np.array_equal(act[~fin], g[~fin])
    assert np.array_equal(w[~fin], np.eye(A, dtype=np.float32)[g[~fin]])
    # decisive rows take the argmax; at least half of the table is decisive
    with np.errstate(invalid="ignore", over="ignore"):
        srt = np.sort(q, axis=1)
        ratio = ((srt[:, -1] - srt[:, -2]).astype(np.float32) / np.float32(T)).astype(np.float32)
    dec = fin & (ratio > 104)
    assert dec.sum() * 2 >= n and dec[::2].all()
    assert np.array_equal(act[dec], np.argmax(q[dec], axis=1))
    assert np.array_equal(w[dec], np.eye(A, dtype=np.float32)[act[dec]])
    if n >= 63:
        assert (~fin).sum() >= 8 and (fin & ~dec).sum() >= 14        # (every kind of row is there)
    # the row map: row i drawn with the uniform of rows[i]
    rmap = (rows * 7 + 5).astype(np.int32)
    act2 = mf.q_sample(_cuda(q), T, seed, step, group, rows=_cuda(rmap)).cpu().numpy()
    assert np.array_equal(act2, qs.sample(q, T, seed, step, group, rmap, w=w))


def test_q_sample_refuses_bad_arguments():
    import torch
    from magent.c_lib import EngineError
    from mfrl_amd import mf
    q = torch.zeros((4, 5), device="cuda")
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(EngineError):
            mf.q_sample(q, bad, 1, 1)
    for A in (1, 33):
        with pytest.raises(EngineError):
            mf.q_sample(torch.zeros((4, A), device="cuda"), 1.0, 1, 1)
    with pytest.raises(TypeError):
        mf.q_sample(q.double(), 1.0, 1, 1)
    assert mf.q_sample(torch.zeros((0, 5), device="cuda"), 1.0, 1, 1).shape == (0,)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_q_sample_frequencies(seed):
    """The CPU frequency check on the kernel: its 65,536 actions are the restatement's, and follow the softmax."""
    import torch
    from mfrl_amd import mf
    q = np.repeat(FREQ_Q, FREQ_N, axis=0)
    act, w = mf.q_sample(_cuda(q), 1.0, seed, 0, want_w=True)
    torch.cuda.synchronize()
    act, w = act.cpu().numpy(), w.cpu().numpy()
    assert (w == w[0]).all()
    ulp = np.abs(w[0].view(np.int32) - qs.weights(FREQ_Q, 1.0)[0].view(np.int32)).max()
    print("seed %d: device expf against the rounded float64 exp: %d ulp at most" % (seed, ulp))
    freq_check(act, seed)
    assert np.array_equal(act, qs.sample(q, 1.0, seed, 0, 0, np.arange(FREQ_N), w=w))
    assert np.array_equal(act, qs.sample(q, 1.0, seed, 0, 0, np.arange(FREQ_N)))


# ------------------------------------------------------------------------------------------------- 2: the epilogues
def _net(use_mf, seed):
    import torch
    from mfrl_amd.algo.nets import QNet
    torch.manual_seed(seed)
    net = QNet(VS, FS, NA, use_mf).cuda()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return net


_OBS = {}


def _rollout_obs(E=256, steps=30):
    """Live-agent rows (views, features, per-row group-0 mean action) of a 64x64 rush rollout after `steps` steps
    (the helper of tests/test_policy_gpu.py); made once, never modified."""
    import torch
    from mfrl_amd.battle import BattleBatch
    if (E, steps) in _OBS:
        return _OBS[(E, steps)]
    left, right = bd.block_positions(64, 128)
    eng = BattleBatch(64, E, stream=torch.cuda.current_stream())
    eng.rollout_init([left, right], max_steps=400, eps=0.2, seed=5, stagger=True)
    eng.rollout_step(steps)
    rc = eng.rowcap
    view = torch.empty((E, rc, 1183), dtype=torch.float32, device="cuda")
    feat = torch.empty((E, rc, 34), dtype=torch.float32, device="cuda")
    num = torch.empty((E, 2), dtype=torch.int32, device="cuda")
    mean = torch.empty((E, 2, NA), dtype=torch.float64, device="cuda")
    eng.rollout_copy("view", view, group=0)
    eng.rollout_copy("feature", feat, group=0)
    eng.rollout_copy("group_num", num)
    eng.rollout_copy("mean_action", mean)
    eng.sync()
    live = torch.arange(rc, device="cuda")[None, :] < num[:, 0:1]
    prob = mean[:, 0:1, :].expand(E, rc, NA).float()
    _OBS[(E, steps)] = (view[live].reshape(-1, 13, 13, 7)[:512].clone(), feat[live][:512].clone(),
                        prob[live][:512].clone())
    return _OBS[(E, steps)]


@pytest.mark.parametrize("use_mf", [False, True])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_fused_epilogue_is_q_sample_on_the_forwards_q(precision, use_mf):
    """forward(temperature=...): d_q is the greedy forward's bit for bit, (d_act, d_w) are mfx_q_sample's on that
    d_q with the same (T, seed, step) bit for bit, at ragged batch sizes; another step draws other actions, the same
    step the same ones."""
    import torch
    from mfrl_amd import mf
    from mfrl_amd.policy import QNetHIP
    view, feat, prob = _rollout_obs()
    hip = QNetHIP(VS, FS, NA, use_mf, precision=precision).load(_net(use_mf, 70 + use_mf))
    pr = prob if use_mf else None
    T, seed = 0.05, 991
    for n in (1, 15, 17, 63, 65, 200):
        a = (view[:n], feat[:n], pr[:n] if use_mf else None)
        q_g, a_g = hip.forward(*a)
        q_s, a_s, w_s = hip.forward(*a, temperature=T, seed=seed, step=n, want_w=True)
        a_k, w_k = mf.q_sample(q_g, T, seed, n, want_w=True)
        a_only = hip.act(*a, temperature=T, seed=seed, step=n)
        torch.cuda.synchronize()
        assert torch.equal(q_s, q_g), n
        assert torch.equal(a_s, a_k) and torch.equal(w_s, w_k), n
        assert torch.equal(a_only, a_k), n
    again = hip.forward(*a, temperature=T, seed=seed, step=200)[1]
    other = hip.forward(*a, temperature=T, seed=seed, step=201)[1]
    torch.cuda.synchronize()
    assert torch.equal(again, a_s)
    changed = int((other != a_s).sum())
    assert 0 < changed, changed
    assert int((a_s != a_g).sum()) > 0                     # (the draw is not the argmax everywhere)
    from magent.c_lib import EngineError
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(EngineError):
            hip.forward(*a, temperature=bad)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_fused_epilogue_past_one_pass(precision):
    """2^18 + 17 rows: the forward runs two conv -> head passes; the second pass draws with the rows of the whole
    batch (the uniform's row and the weights' offset move with the pass), so the result is still q_sample's."""
    import torch
    from mfrl_amd import mf
    from mfrl_amd.policy import QNetHIP
    view, feat, prob = _rollout_obs()
    n = (1 << 18) + 17
    idx = (torch.arange(n, device="cuda") * 7 + 3) % view.shape[0]
    v, f, p = view[idx], feat[idx], prob[idx]
    hip = QNetHIP(VS, FS, NA, True, precision=precision).load(_net(True, 90))
    q_g, _ = hip.forward(v, f, p)
    q_s, a_s, w_s = hip.forward(v, f, p, temperature=0.05, seed=5, step=9, want_w=True)
    a_k, w_k = mf.q_sample(q_g, 0.05, 5, 9, want_w=True)
    torch.cuda.synchronize()
    assert torch.equal(q_s, q_g) and torch.equal(a_s, a_k) and torch.equal(w_s, w_k)
    assert len(torch.unique(a_s[1 << 18:])) > 1            # (the second pass's 17 rows are not one action)


# ------------------------------------------------------------------------------------------------- 3: the rollout
@pytest.mark.parametrize("E,small_e,steps,plan", [(3, "0", 12, "k_rollout"), (8, None, 5, None)])
def test_sampled_rollout_matches_oracle(E, small_e, steps, plan, monkeypatch):
    """Two mean-field QNets sampling at T = 0.5 drive a rollout (act_rollout(temperature=...) + rollout_policy_step),
    3 envs on the fused plan and 8 envs on the few-env plan, max_steps 5 so every env restarts.  Per step the action
    buffer's live rows are q_sample on the forward's Q for those rows with row = e * rowcap + j, the rows past each
    group's count are untouched, and every env is replayed on the C oracle with the device's actions: rewards,
    views, features and mean actions bit for bit."""
    import torch
    from mfrl_amd import mf
    from mfrl_amd.battle import BattleBatch
    from mfrl_amd.policy import QNetHIP
    if small_e is not None:
        monkeypatch.setenv("MFX_SMALL_E", small_e)
    max_steps, VF, F, T, seed = 5, 1183, 34, 0.5, 31337
    left, right = bd.block_positions(64, 128)
    eng = BattleBatch(64, E, stream=torch.cuda.current_stream())
    eng.rollout_init([left, right], max_steps=max_steps, eps=0.0, seed=1, stagger=False)
    if plan:
        assert eng.rollout_path() == plan
    else:
        assert eng.rollout_path() != "k_rollout"                       # (the few-env plan: another step kernel)
    pols = [QNetHIP(VS, FS, NA, True).load(_net(True, 21 + g)) for g in range(2)]
    rc = eng.rowcap
    oracles = []
    for e in range(E):
        env, h = common.battle_env(common.ORACLE_LIB, 64)
        env.reset()
        env.add_agents(h[0], method="custom", pos=left)
        env.add_agents(h[1], method="custom", pos=right)
        oracles.append([env, h, 0])
    eng.rollout_policy_observe()

    def grab():
        out = {}
        for g in range(2):
            out["view%d" % g] = torch.empty((E, rc, VF), dtype=torch.float32, device="cuda")
            out["feat%d" % g] = torch.empty((E, rc, F), dtype=torch.float32, device="cuda")
            eng.rollout_copy("view", out["view%d" % g], group=g)
            eng.rollout_copy("feature", out["feat%d" % g], group=g)
        out["mean"] = torch.empty((E, 2, NA), dtype=torch.float64, device="cuda")
        eng.rollout_copy("mean_action", out["mean"])
        eng.sync()
        return out

    obs = grab()
    slot = torch.arange(E * rc, dtype=torch.int32, device="cuda").reshape(E, rc)      # e * rowcap + j
    restarts, kinds, not_greedy = 0, set(), 0
    for t in range(steps):
        eng.rollout_write("actions", torch.full((E, 2, rc), -7, dtype=torch.int32, device="cuda"))
        for g in range(2):
            pols[g].act_rollout(eng, g, temperature=T, seed=seed, step=t)
        act = torch.empty((E, 2, rc), dtype=torch.int32, device="cuda")
        eng.rollout_copy("actions", act)
        eng.sync()
        for g in range(2):
            n_g = torch.tensor([len(o[0].get_agent_id(o[1][g])) for o in oracles], device="cuda")
            live = torch.arange(rc, device="cuda")[None, :] < n_g[:, None]
            prob = obs["mean"][:, g:g + 1, :].expand(E, rc, NA)[live].float()
            q, greedy = pols[g].forward(obs["view%d" % g][live].reshape(-1, 13, 13, 7), obs["feat%d" % g][live], prob)
            want = mf.q_sample(q, T, seed, t, group=g, rows=slot[live].contiguous())
            torch.cuda.synchronize()
            assert torch.equal(act[:, g][live], want), (t, g)
            assert bool((act[:, g][~live] == -7).all()), (t, g)
            not_greedy += int((want != greedy).sum())
        actn = act.cpu().numpy()
        eng.rollout_write("actions", torch.clamp(act, min=0))          # (the sentinel out of the dead rows again)
        eng.rollout_policy_step()
        nxt = grab()
        rew = torch.empty((E, 2, rc), dtype=torch.float32, device="cuda")
        eng.rollout_copy("rewards", rew)
        eng.sync()
        for e, st in enumerate(oracles):
            env, h, _ = st
            acts = [np.ascontiguousarray(actn[e, g, :len(env.get_agent_id(h[g]))]) for g in range(2)]
            for g in range(2):
                kinds.update(acts[g].tolist())
                env.set_action(h[g], acts[g])
            done = env.step()
            for g in range(2):
                rw = env.get_reward(h[g])
                assert rew[e, g, :len(rw)].cpu().numpy().tobytes() == rw.tobytes(), (t, e, g, "reward")
            env.clear_dead()
            st[2] += 1
            restart = done or st[2] >= max_steps
            for g in range(2):
                n = len(acts[g])
                want = np.bincount(acts[g], minlength=NA) / n if n else np.full(NA, np.nan)
                got = nxt["mean"][e, g].cpu().numpy()
                if restart:
                    assert not got.any(), (t, e, g, "mean reset")
                else:
                    assert np.array_equal(got, want, equal_nan=True), (t, e, g, "mean")
            if restart:
                st[2] = 0
                restarts += 1
                env.reset()
                env.add_agents(h[0], method="custom", pos=left)
                env.add_agents(h[1], method="custom", pos=right)
            for g in range(2):
                v, f = env.get_observation(h[g])
                n = len(v)
                assert nxt["view%d" % g][e, :n].cpu().numpy().tobytes() == v.reshape(n, VF).tobytes(), (t, e, g)
                assert nxt["feat%d" % g][e, :n].cpu().numpy().tobytes() == f.tobytes(), (t, e, g)
        obs = nxt
    eng.rollout_check()
    assert restarts >= E * (steps // max_steps) and len(kinds) > 3 and not_greedy > 0


# ------------------------------------------------------------------------------------------------- 4: ValueNet
def _model(name):
    import magent
    from mfrl_amd.algo import spawn_ai
    env = magent.GridWorld("battle", map_size=20)
    return spawn_ai("mfq", None, env, env.get_handles()[0], name, 50)


def test_valuenet_explore_act():
    """explore = "boltzmann": act(eps=T) gives the restatement's actions for (self.seed, the call count) on the Q
    values of the HIP forward; the default gives what it gives today (the HIP forward's argmax), eps unused."""
    import torch
    from mfrl_amd import mf
    from mfrl_amd.algo.base import ValueNet
    from mfrl_amd.policy import QNetHIP
    torch.manual_seed(12)
    m = _model("mfq-explore")
    assert isinstance(m, ValueNet) and m.explore == "greedy" and m._draws == 0
    view, feat, prob = (x[:300] for x in _rollout_obs())
    hip = QNetHIP(VS, FS, NA, True).load(m.eval_net)
    q, greedy = hip.forward(view, feat, prob)
    for eps in (1.0, 0.1):
        got = m.act(state=[view, feat], prob=prob, eps=eps)
        assert got.dtype == np.int32 and np.array_equal(got, greedy.cpu().numpy())
    assert m._draws == 0
    m.explore = "boltzmann"
    for call, T in ((1, 0.7), (2, 0.02)):
        got = m.act(state=[view, feat], prob=prob, eps=T)
        _, w = mf.q_sample(q, T, 0, 0, want_w=True)
        want = qs.sample(q.cpu().numpy(), T, m.seed, call, 0, np.arange(300), w=w.cpu().numpy())
        assert m._draws == call and got.dtype == np.int32 and np.array_equal(got, want), call
    assert not np.array_equal(got, greedy.cpu().numpy())
    with pytest.raises(ValueError):
        m.act(state=[view, feat], prob=prob, eps=0.0)
    # the seed: the model's name and the run's torch seed, as ActorCritic's
    torch.manual_seed(12)
    assert _model("mfq-explore").seed == m.seed
    assert _model("mfq-other").seed != m.seed
    torch.manual_seed(13)
    assert _model("mfq-explore").seed != m.seed
    m.explore = "greedy"
    assert np.array_equal(m.act(state=[view, feat], prob=prob, eps=0.3), greedy.cpu().numpy())


def test_valuenet_explore_act_rollout():
    """act_rollout with explore = "boltzmann" draws with (self.seed, the call count, group, e * rowcap + j) at eps (or
    self.temperature); the default writes QNetHIP.act_rollout's greedy actions, as today."""
    import torch
    from mfrl_amd import mf
    from mfrl_amd.battle import BattleBatch
    from mfrl_amd.policy import QNetHIP
    E = 4
    m = _model("mfq-rollout")
    left, right = bd.block_positions(64, 128)
    eng = BattleBatch(64, E, stream=torch.cuda.current_stream())
    eng.rollout_init([left, right], max_steps=50, eps=0.0, seed=2, stagger=False)
    eng.rollout_policy_observe()
    rc = eng.rowcap
    hip = QNetHIP(VS, FS, NA, True).load(m.eval_net)

    def acts(fn):
        eng.rollout_write("actions", torch.full((E, 2, rc), -7, dtype=torch.int32, device="cuda"))
        fn()
        out = torch.empty((E, 2, rc), dtype=torch.int32, device="cuda")
        eng.rollout_copy("actions", out)
        eng.sync()
        return out

    base = acts(lambda: hip.act_rollout(eng, 1))
    assert torch.equal(acts(lambda: m.act_rollout(eng, 1)), base)
    assert torch.equal(acts(lambda: m.act_rollout(eng, 1, eps=0.3)), base) and m._draws == 0
    m.explore = "boltzmann"
    got = acts(lambda: m.act_rollout(eng, 1, eps=0.4))
    assert m._draws == 1 and m.temperature == 0.4
    assert torch.equal(got, acts(lambda: hip.act_rollout(eng, 1, temperature=0.4, seed=m.seed, step=1)))
    got2 = acts(lambda: m.act_rollout(eng, 1))                          # eps None: self.temperature
    assert torch.equal(got2, acts(lambda: hip.act_rollout(eng, 1, temperature=0.4, seed=m.seed, step=2)))
    # ... which are the restatement's actions on the forward's Q
    view = torch.empty((E, rc, 1183), dtype=torch.float32, device="cuda")
    feat = torch.empty((E, rc, 34), dtype=torch.float32, device="cuda")
    num = torch.empty((E, 2), dtype=torch.int32, device="cuda")
    mean = torch.empty((E, 2, NA), dtype=torch.float64, device="cuda")
    eng.rollout_copy("view", view, group=1)
    eng.rollout_copy("feature", feat, group=1)
    eng.rollout_copy("group_num", num)
    eng.rollout_copy("mean_action", mean)
    eng.sync()
    live = torch.arange(rc, device="cuda")[None, :] < num[:, 1:2]
    q = hip.forward(view[live].reshape(-1, 13, 13, 7), feat[live], mean[:, 1:2, :].expand(E, rc, NA)[live].float())[0]
    _, w = mf.q_sample(q, 0.4, 0, 0, want_w=True)
    rows = torch.arange(E * rc, device="cuda").reshape(E, rc)[live].cpu().numpy()
    want = qs.sample(q.cpu().numpy(), 0.4, m.seed, 1, 1, rows, w=w.cpu().numpy())
    assert np.array_equal(got[:, 1][live].cpu().numpy(), want)
    assert bool((got[:, 1][~live] == -7).all()) and bool((got[:, 0] == -7).all())
    assert not torch.equal(got, base) and not torch.equal(got, got2)


def test_train_battle_explore_runs(tmp_path, capsys):
    from mfrl_amd import train_battle
    train_battle.main(["--algo", "mfq", "--envs", "4", "--rollout", "--explore", "boltzmann", "--n_round", "1",
                       "--max_steps", "8", "--map_size", "40", "--base_dir", str(tmp_path)])
    out = capsys.readouterr().out
    assert "device rollout" in out and "[TIME] round 0" in out
