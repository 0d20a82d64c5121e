"""The bf16 acting mode of the Q network on the GPU: QNetHIP(precision="bf16") = mfx_qnet_set_precision(1) =
csrc/qnet_bf16_kernels.hip (k_qb16_conv + k_qb16_head on v_mfma_f32_16x16x32_bf16).

The contract is the numpy restatement tests/qnet_bf16_ref.py; tests/test_policy_bf16_cpu.py pins that reference and the
conditions used here (e_q = the reference's own quantisation error against the exact float64 forward; clear rows =
rows decided by more than 2 e_q).  The bounds: |q - reference| <= e_q and |q - exact| <= 2 e_q.  Both come from a CPU
estimate, not from the kernels: re-running the reference with f32 accumulation in another order moved it by at most
0.57 e_q through flipped roundings of intermediates, while a layout or permutation mistake gives errors of the order of
the Q scale, a hundred times e_q."""
import ctypes
import os
import re

import numpy as np
import pytest

import battle_driver as bd
import common
import qnet_bf16_ref as ref
import rollout_check as rck

pytestmark = pytest.mark.gpu
VS, FS, NA = (13, 13, 7), (34,), 21


def _hip(net, use_mf, precision="bf16"):
    from mfrl_amd.policy import QNetHIP
    return QNetHIP(VS, FS, NA, use_mf, precision=precision).load(net)


def _header_constant(name):
    src = open(os.path.join(common.PKG, "csrc", "qnet_bf16.h")).read()
    return int(re.search(r"\b%s = (\d+)" % name, src).group(1))


@pytest.fixture(scope="module")
def rows():
    """2,304 distinct rows on the device: the 256 fixture views in a strided order, the fixture features scaled per
    row, a drawn mean action per row."""
    import torch
    view, feat, _ = ref.fixture_rows()
    n = 2304
    i = np.arange(n)
    rng = np.random.RandomState(23)
    v = view[(7 * i) % 256]
    f = (feat[i % 256] * (1.0 + (i // 256)[:, None] / 16.0)).astype(np.float32)
    p = rng.dirichlet(np.ones(NA), n).astype(np.float32)
    return torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(p).cuda()


@pytest.fixture(scope="module")
def full(rows):
    """A mean-field bf16 net and its forward of all 2,304 rows (computed once, never modified)."""
    import torch
    net = ref.net(True, 5).cuda()
    hip = _hip(net, True)
    q, a = hip.forward(*rows)
    torch.cuda.synchronize()
    return hip, q.clone(), a.clone()


# ------------------------------------------------------------------------------------------------- 1: the reference
@pytest.mark.parametrize("use_mf,seed", [(False, 11), (False, 12), (True, 11), (True, 12)])
def test_bf16_forward_matches_reference(use_mf, seed):
    import torch
    view, feat, prob = ref.fixture_rows()
    net = ref.net(use_mf, seed)
    exact, quant, e_q, scale = ref.quantisation(net, use_mf, view, feat, prob)
    hip = _hip(net.cuda(), use_mf)
    q, act = hip.forward(torch.from_numpy(view).cuda(), torch.from_numpy(feat).cuda(),
                         torch.from_numpy(prob).cuda() if use_mf else None)
    torch.cuda.synchronize()
    q, act = q.cpu().double().numpy(), act.cpu().numpy()
    d_exact, d_ref = float(np.abs(q - exact).max()), float(np.abs(q - quant).max())
    clear = ref.clear_rows(exact, e_q)
    print("bf16 forward use_mf %d seed %d: e_q %.4e scale %.3f |q-exact|/e_q %.3f |q-ref|/e_q %.3f clear %.3f"
          % (use_mf, seed, e_q, scale, d_exact / e_q, d_ref / e_q, clear.mean()))
    assert d_exact <= 2.0 * e_q, (d_exact, e_q)
    assert d_ref <= e_q, (d_ref, e_q)
    assert np.array_equal(act[clear], np.argmax(exact, 1)[clear])
    assert np.array_equal(act, np.argmax(q, 1))          # (the kernel's own argmax: first maximum)


# ------------------------------------------------------------------------------------------------- 2: partial tiles
def test_every_partial_tile(rows, full):
    """n = 1 .. 65 (partial agent tiles, waves and workgroups of both kernels) and n = conv grid cap x agents per conv
    pass + 1 (the conv's grid-stride loop wraps once) give, bit for bit, the rows the 2,304-row batch gives."""
    import torch
    hip, q_all, a_all = full
    wrap = _header_constant("kB16ConvMaxGrid") * _header_constant("kB16ConvAgents") + 1
    assert 200 <= wrap <= q_all.shape[0]
    for n in (1, 15, 16, 17, 63, 64, 65, wrap):
        q, a = hip.forward(rows[0][:n], rows[1][:n], rows[2][:n])
        torch.cuda.synchronize()
        assert torch.equal(q, q_all[:n]) and torch.equal(a, a_all[:n]), n


# ------------------------------------------------------------------------------------------------- 3: the pass split
def test_pass_split(rows, full):
    """One forward of 2^18 + 17 rows (two conv -> head passes) of a repeated 1,024-row block equals the block's
    result tiled."""
    import torch
    hip, q_all, a_all = full
    n, b = (1 << 18) + 17, 1024
    rep = (n + b - 1) // b
    view = rows[0][:b].repeat(rep, 1, 1, 1)[:n]
    feat = rows[1][:b].repeat(rep, 1)[:n]
    prob = rows[2][:b].repeat(rep, 1)[:n]
    q, a = hip.forward(view, feat, prob)
    torch.cuda.synchronize()
    assert torch.equal(q, q_all[:b].repeat(rep, 1)[:n])
    assert torch.equal(a, a_all[:b].repeat(rep)[:n])


# ------------------------------------------------------------------------------------------------- 4: modes
def test_determinism_and_mode_switching(rows):
    import torch
    from mfrl_amd import check
    view, feat, prob = (x[:300] for x in rows)
    net = ref.net(True, 12).cuda()
    never = _hip(net, True, "f32")
    q_never, a_never = never.forward(view, feat, prob)
    hip = _hip(net, True, "f32")
    L, mode = hip._L, ctypes.c_int(-1)

    def precision():
        check(L.mfx_qnet_precision(hip.handle, ctypes.byref(mode)), "mfx_qnet_precision")
        return mode.value

    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert precision() == 0
    q0, a0 = hip.forward(view, feat, prob)
    check(L.mfx_qnet_set_precision(hip.handle, 1, stream), "mfx_qnet_set_precision")     # images built from the kept blob
    assert precision() == 1
    q1, a1 = hip.forward(view, feat, prob)
    q2, a2 = hip.forward(view, feat, prob)
    assert L.mfx_qnet_set_precision(hip.handle, 2, stream) != 0 and precision() == 1     # refused, the mode stays
    check(L.mfx_qnet_set_precision(hip.handle, 0, stream), "mfx_qnet_set_precision")
    assert precision() == 0
    q3, a3 = hip.forward(view, feat, prob)
    born = _hip(net, True, "bf16")                                                     # images built by set_weights
    qb, ab = born.forward(view, feat, prob)
    torch.cuda.synchronize()
    assert torch.equal(q1, q2) and torch.equal(a1, a2)
    assert torch.equal(q1, qb) and torch.equal(a1, ab)
    assert torch.equal(q0, q3) and torch.equal(a0, a3)
    assert torch.equal(q0, q_never) and torch.equal(a0, a_never)
    d = float((q1 - q0).abs().max())
    assert 0.0 < d < 0.1 * max(1.0, float(q0.abs().max())), d        # another mode, the same network
    header = open(os.path.join(common.REPO, "include", "magent_amd.h")).read()
    dll = ctypes.CDLL(common.HIP_LIB)
    for fn in ("mfx_qnet_set_precision", "mfx_qnet_precision"):
        assert re.search(r"\bint %s\(" % fn, header), fn
        assert hasattr(dll, fn), fn


# ------------------------------------------------------------------------------------------------- 5: the row map
def test_act_rollout_bf16_matches_dense_forward():
    """64 envs of 64x64 after 30 rollout steps: act_rollout (row list, float64 mean action, the rollout's action
    buffer) writes for every live row the action the dense bf16 forward gives on that row's view, feature and env
    mean action gathered by hand; dead rows of the action buffer are untouched."""
    import torch
    from mfrl_amd.battle import BattleBatch
    E = 64
    left, right = bd.block_positions(64, 128)
    eng = BattleBatch(64, E, stream=torch.cuda.current_stream())
    eng.rollout_init([left, right], max_steps=400, eps=0.2, seed=5, stagger=True)
    eng.rollout_step(30)
    eng.rollout_policy_observe()
    rc = eng.rowcap
    pols = [_hip(ref.net(True, 31 + g).cuda(), True) for g in range(2)]
    eng.rollout_write("actions", torch.full((E, 2, rc), -7, dtype=torch.int32, device="cuda"))
    for g in range(2):
        pols[g].act_rollout(eng, g)
    act = torch.empty((E, 2, rc), dtype=torch.int32, device="cuda")
    num = torch.empty((E, 2), dtype=torch.int32, device="cuda")
    mean = torch.empty((E, 2, NA), dtype=torch.float64, device="cuda")
    eng.rollout_copy("actions", act)
    eng.rollout_copy("group_num", num)
    eng.rollout_copy("mean_action", mean)
    live_n = 0
    for g in range(2):
        view = torch.empty((E, rc, 1183), dtype=torch.float32, device="cuda")
        feat = torch.empty((E, rc, 34), dtype=torch.float32, device="cuda")
        eng.rollout_copy("view", view, group=g)
        eng.rollout_copy("feature", feat, group=g)
        eng.sync()
        live = torch.arange(rc, device="cuda")[None, :] < num[:, g:g + 1]
        prob = mean[:, g:g + 1, :].expand(E, rc, NA)[live].float()       # f64 -> f32 here, f32 -> bf16 in the kernel
        want = pols[g].act(view[live].reshape(-1, 13, 13, 7), feat[live], prob)
        torch.cuda.synchronize()
        assert torch.equal(act[:, g][live], want), g
        assert bool((act[:, g][~live] == -7).all()), g
        live_n += int(live.sum())
        assert len(torch.unique(want)) > 3                 # (not one action everywhere)
    assert live_n > 4000 and bool((mean != 0).any())      # (of at most 64 x 2 x 128 rows)
    assert float((mean.float().double() - mean).abs().max()) > 0         # the f64 -> f32 rounding is a real one


# ------------------------------------------------------------------------------------------------- 6: in the loop
def _loop_and_replay(map_size, E, placement, T, max_steps, path=None, policy_path=None):
    """Two mean-field bf16 QNets drive a rollout for T steps (act_rollout + rollout_policy_step); the sampled envs are
    then replayed on the C oracle from rollout_init with the actions the device recorded at every step, and the final
    views, features, rewards, mean actions and group sizes must agree bit for bit."""
    import torch
    from mfrl_amd.battle import BattleBatch
    eng = BattleBatch(map_size, E, stream=torch.cuda.current_stream())
    eng.rollout_init(placement, max_steps=max_steps, eps=0.2, seed=7, stagger=True)
    if path:
        assert eng.rollout_path() == path
    if policy_path:
        assert eng.rollout_policy_path() == policy_path
    rc = eng.rowcap
    pols = [_hip(ref.net(True, 41 + g).cuda(), True) for g in range(2)]
    picks = rck.sample_envs(E, 3)
    log = torch.empty((T, len(picks), 2, rc), dtype=torch.int32, device="cuda")
    eng.rollout_policy_observe()
    for t in range(T):
        for g in range(2):
            pols[g].act_rollout(eng, g)
        for j, e in enumerate(picks):
            eng.rollout_copy_at("actions", log[t, j], e * 2 * rc * 4)
        eng.rollout_policy_step()
    eng.sync()
    eng.rollout_check()
    dev = rck.device_records(eng, picks)
    acts = log.cpu().numpy()
    restarts, kinds = 0, set()
    for j, e in enumerate(picks):
        o, h = common.battle_env(common.ORACLE_LIB, map_size)

        def reset():
            o.reset()
            for g in range(2):
                o.add_agents(h[g], method="custom", pos=placement[g])

        reset()
        ep_len, last = e * max_steps // E, None
        for t in range(T):
            n = [len(o.get_agent_id(h[g])) for g in range(2)]
            act = [np.ascontiguousarray(acts[t, j, g, :n[g]]) for g in range(2)]
            for g in range(2):
                assert act[g].min() >= 0 and act[g].max() < NA, (e, t, g)
                kinds.update(act[g].tolist())
                o.set_action(h[g], act[g])
            done = o.step()
            rew = [o.get_reward(h[g]).copy() for g in range(2)]
            o.clear_dead()
            ep_len += 1
            restart = bool(done) or ep_len >= max_steps
            if restart:
                ep_len = 0
                restarts += 1
                reset()
            last = (n, act, rew, restart)
        n, act, rew, restart = last
        for g in range(2):
            v, f = o.get_observation(h[g])
            m = len(v)
            assert int(dev["group_num"][j, g]) == m, (e, g, "size")
            assert dev["view"][g][j, :m].tobytes() == v.reshape(m, -1).tobytes(), (e, g, "view")
            assert dev["feature"][g][j, :m].tobytes() == f.tobytes(), (e, g, "feature")
            assert dev["rewards"][j, g, :n[g]].tobytes() == rew[g].tobytes(), (e, g, "rewards")
            want = (np.zeros(NA) if restart else np.bincount(act[g], minlength=NA) / n[g] if n[g] else np.full(NA, np.nan))
            assert np.array_equal(dev["mean"][j, g, :NA], want, equal_nan=True), (e, g, "mean action")
    assert len(kinds) > 3                                  # (the nets chose among several actions)
    return restarts


def test_bf16_policy_in_the_loop_fused_plan(monkeypatch):
    monkeypatch.setenv("MFX_SMALL_E", "0")               # 3 envs on the fused path, as tests/test_policy_gpu.py
    restarts = _loop_and_replay(64, 3, list(bd.block_positions(64, 128)), T=25, max_steps=30, path="k_rollout")
    assert restarts >= 2


def test_bf16_policy_in_the_loop_large_env_plan():
    _loop_and_replay(200, 2, list(bd.block_positions(200, 1250)), T=20, max_steps=400, path="k_rollout_bigq",
                     policy_path="k_observe_items+k_rollout_big")


# ------------------------------------------------------------------------------------------------- 7: ValueNet
def test_valuenet_act_precision(rows):
    """ValueNet.act_precision = "bf16": act_dev returns what a bf16 QNetHIP loaded from the eval net returns, before
    and after a train() step (the weights_key path re-packs the weights)."""
    import magent
    import torch
    from mfrl_amd.algo import spawn_ai
    from mfrl_amd.algo.base import ValueNet
    assert ValueNet.act_precision == "f32"
    env = magent.GridWorld("battle", map_size=20)
    m = spawn_ai("mfq", None, env, env.get_handles()[0], "mfq-bf16", 50)
    assert isinstance(m, ValueNet) and m.use_mf
    m.act_precision = "bf16"
    view, feat, prob = (x[:500] for x in rows)
    got = m.act_dev(state=[view, feat], prob=prob, eps=1.0)
    assert m._hip.precision == "bf16"
    want = _hip(m.eval_net, True).act(view, feat, prob)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    for grp in m.optimizer.param_groups:                 # one large step: the new weights act differently
        grp["lr"] = 0.05
    ValueNet.train(m, state=[view, feat], target_q=torch.randn(500, device="cuda"), prob=prob,
                   acts=torch.randint(0, NA, (500,), device="cuda"), masks=torch.ones(500, device="cuda"))
    got2 = m.act_dev(state=[view, feat], prob=prob, eps=1.0)
    want2 = _hip(m.eval_net, True).act(view, feat, prob)
    torch.cuda.synchronize()
    assert torch.equal(got2, want2)
    assert not torch.equal(got2, got)
