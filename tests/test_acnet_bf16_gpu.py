"""The bf16 acting mode of the actor-critic network on the GPU: ACNetHIP(precision="bf16") =
mfx_acnet_set_precision(1) = csrc/acnet_bf16_kernels.hip (k_acb16 on v_mfma_f32_16x16x32_bf16).

The contract is the numpy restatement tests/acnet_bf16_ref.py; tests/test_acnet_bf16_cpu.py pins that reference and the
conditions used here (e_p = the reference's own quantisation error against the exact float64 policy; clear rows = rows
whose uniform lies more than 2 e_c from every boundary of the exact cumulative policy).  The bounds: |p - reference|
<= e_p and |p - exact| <= 2 e_p.  Both come from the CPU, not from the kernel: re-running the reference with f32
accumulation in three other orders moved the policy by at most 0.17 e_p, while a layout or permutation mistake moves
it by the policy scale, 10 - 40 times e_p."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

import acnet_bf16_ref as ref
import acnet_ref
import battle_driver as bd
import common
import net_shapes as ns
import rollout_check as rck
from test_acnet_bf16_cpu import BATTLE_CASES, SHAPE_CASES

pytestmark = pytest.mark.gpu
VS, FS, NA = (13, 13, 7), (34,), 21
SEED, STEP = 4242, 5


def _hip(net, use_mf=True, precision="bf16", shape=(VS, FS, NA)):
    from mfrl_amd.policy import ACNetHIP
    return ACNetHIP(shape[0], shape[1], shape[2], use_mf, precision=precision).load(net)


def _header_constant(name):
    src = open(os.path.join(common.PKG, "csrc", "acnet_bf16.h")).read()
    return int(re.search(r"\b%s = (\d+)" % name, src).group(1))


def _bounds(tag, pol, act, exact, quant, e_p, seed, step):
    """The reference bounds (ratios printed first) and the draw, on one forward's policy and actions."""
    n = len(exact)
    d_exact, d_ref = float(np.abs(pol - exact).max()), float(np.abs(pol - quant).max())
    u = acnet_ref.uniforms(seed, step, 0, np.arange(n))
    clear, e_c = ref.clear_rows(exact, quant, u)
    print("bf16 acnet %s: e_p %.4e |p-ref|/e_p %.3f |p-exact|/e_p %.3f e_c %.3e clear %.3f"
          % (tag, e_p, d_ref / e_p, d_exact / e_p, e_c, clear.mean()))
    assert d_ref <= e_p, (d_ref, e_p)
    assert d_exact <= 2.0 * e_p, (d_exact, e_p)
    return clear


def _draws(pol32, act, exact, clear, seed, step):
    n = len(exact)
    assert np.array_equal(act, acnet_ref.draw(pol32, seed, step, 0, np.arange(n)))          # the kernel's own rows
    want = acnet_ref.draw(exact.astype(np.float32), seed, step, 0, np.arange(n))
    assert clear.mean() >= 0.5
    assert np.array_equal(act[clear], want[clear])
    assert len(np.unique(act)) > 1


@pytest.fixture(scope="module")
def battle():
    """Per (use_mf, seed): the kernel's policy (float32) and actions on the 256 fixture rows, and the CPU references
    (computed once, never modified)."""
    import torch
    view, feat = ref.fixture_rows()
    out = {}
    for use_mf, seed in BATTLE_CASES:
        net = ref.net(use_mf, seed)
        exact, quant, e_p = ref.quantisation(net, use_mf, (view, feat))
        hip = _hip(net.cuda(), use_mf)
        pol, _, act = hip.forward(torch.from_numpy(view).cuda(), torch.from_numpy(feat).cuda(), seed=SEED, step=STEP)
        torch.cuda.synchronize()
        out[(use_mf, seed)] = (pol.cpu().numpy(), act.cpu().numpy(), exact, quant, e_p)
    return out


# ------------------------------------------------------------------------------------------------- 1: the reference
@pytest.mark.parametrize("use_mf,seed", BATTLE_CASES)
def test_bf16_policy_matches_reference(battle, use_mf, seed):
    pol, act, exact, quant, e_p = battle[(use_mf, seed)]
    assert pol.dtype == np.float32 and pol.shape == (256, NA)
    _bounds("use_mf %d seed %d" % (use_mf, seed), pol.astype(np.float64), act, exact, quant, e_p, SEED, STEP)
    assert pol.min() >= np.float32(1e-10) and abs(float(pol.sum(1).mean()) - 1.0) < 1e-5


# ------------------------------------------------------------------------------------------------- 2: the draw
@pytest.mark.parametrize("use_mf,seed", BATTLE_CASES)
def test_bf16_draw(battle, use_mf, seed):
    pol, act, exact, quant, e_p = battle[(use_mf, seed)]
    clear, _ = ref.clear_rows(exact, quant, acnet_ref.uniforms(SEED, STEP, 0, np.arange(256)))
    _draws(pol, act, exact, clear, SEED, STEP)


# ------------------------------------------------------------------------------------------------- 3: partial tiles
def _rows(n=2304):
    """n distinct rows on the device: the 256 fixture views in a strided order, the fixture features scaled per row
    (as tests/test_policy_bf16_gpu.py's rows fixture)."""
    import torch
    view, feat = ref.fixture_rows()
    i = np.arange(n)
    v = view[(7 * i) % 256]
    f = (feat[i % 256] * (1.0 + (i // 256)[:, None] / 16.0)).astype(np.float32)
    return torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()


@pytest.fixture(scope="module")
def rows():
    return _rows()


@pytest.fixture(scope="module")
def full(rows):
    """A bf16 MFAC net and its forward of all 2,304 rows (computed once, never modified)."""
    import torch
    hip = _hip(ref.net(True, 5).cuda())
    pol, _, act = hip.forward(rows[0], rows[1], seed=SEED, step=STEP)
    torch.cuda.synchronize()
    return hip, pol.clone(), act.clone()


def test_every_partial_tile(rows, full):
    import torch
    hip, p_all, a_all = full
    per_wg = _header_constant("kAB16Rows")
    assert 16 <= per_wg and per_wg + 1 <= p_all.shape[0]
    assert len(torch.unique(a_all)) > 3 and float((p_all[1:] - p_all[:-1]).abs().max()) > 0
    for n in (1, 15, 16, 17, 63, 64, 65, per_wg + 1):
        pol, _, act = hip.forward(rows[0][:n], rows[1][:n], seed=SEED, step=STEP)
        torch.cuda.synchronize()
        assert torch.equal(pol, p_all[:n]) and torch.equal(act, a_all[:n]), n


# ------------------------------------------------------------------------------------------------- 4: other shapes
@pytest.mark.parametrize("case", SHAPE_CASES, ids=ns.case_id)
def test_off_the_battle_shape(case):
    import torch
    V, F, A, mf = case
    r = ns.acnet_case(*case)
    exact, quant, e_p = ref.quantisation_blob(r.blob, r.layout[1], V, F, A, mf, r.view, r.feat)
    for name, (v, f) in (("view", (0 * r.view, r.feat)), ("feat", (r.view, 0 * r.feat))):     # the precondition
        moved = float(np.median(np.abs(ref.forward(r.blob, r.layout[1], V, F, A, mf, v, f) - quant).max(1)))
        assert moved > 2.0 * e_p, (name, moved, e_p)
    hip = _hip(copy.deepcopy(r.net).cuda(), mf, shape=((V,), (F,), A))      # (r is cached: its CPU net stays put)
    pol, _, act = hip.forward(torch.from_numpy(r.view).cuda(), torch.from_numpy(r.feat).cuda(), seed=SEED, step=STEP)
    torch.cuda.synchronize()
    pol, act = pol.cpu().numpy(), act.cpu().numpy()
    assert pol.shape == (ns.N, A)
    clear = _bounds(ns.case_id(case), pol.astype(np.float64), act, exact, quant, e_p, SEED, STEP)
    _draws(pol, act, exact, clear, SEED, STEP)


# ------------------------------------------------------------------------------------------------- 5: modes
def test_determinism_and_mode_switching(rows):
    import torch
    from mfrl_amd import check
    view, feat = (x[:300] for x in rows)
    prob = torch.full((300, NA), 1.0 / NA, device="cuda")
    net = ref.net(True, 12).cuda()
    fwd = lambda h: h.forward(view, feat, seed=SEED, step=STEP)                         # noqa: E731
    fwd_v = lambda h: h.forward(view, feat, prob, want_value=True, seed=SEED, step=STEP)  # noqa: E731
    never = fwd_v(_hip(net, precision="f32"))
    hip = _hip(net, precision="f32")
    L, mode = hip._L, ctypes.c_int(-1)

    def precision():
        check(L.mfx_acnet_precision(hip.handle, ctypes.byref(mode)), "mfx_acnet_precision")
        return mode.value

    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert precision() == 0
    r0 = fwd_v(hip)
    hip.set_precision("bf16")                                                          # images built from the kept blob
    assert precision() == 1 and hip.precision == "bf16"
    r1, r2 = fwd(hip), fwd(hip)
    assert L.mfx_acnet_set_precision(hip.handle, 2, stream) != 0 and precision() == 1    # refused, the mode stays
    # the value is refused: the C call with d_value, and the wrapper before any call
    val = torch.full((300,), -3.0, device="cuda")
    act = torch.full((300,), -7, dtype=torch.int32, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())                                        # noqa: E731
    rc = L.mfx_acnet_forward(hip.handle, P(view.reshape(300, -1).contiguous()), P(feat), P(prob), 300, None, P(val), P(act),
                             ctypes.c_uint32(SEED), ctypes.c_uint32(STEP), stream)
    assert rc != 0 and "bf16 is acting only" in L.mfx_last_error().decode()
    torch.cuda.synchronize()
    assert bool((val == -3.0).all()) and bool((act == -7).all())                       # nothing was launched
    with pytest.raises(ValueError):
        fwd_v(hip)
    # a support mask set and cleared: the same results, on views that are zero outside it
    mask = ns.support_mask(1183)
    vm = view.reshape(300, -1) * torch.from_numpy(mask).cuda().float()
    dense = hip.forward(vm, feat, seed=SEED, step=STEP)
    hip.set_input_support(mask)
    packed = hip.forward(vm, feat, seed=SEED, step=STEP)
    hip.set_input_support(None)
    cleared = hip.forward(vm, feat, seed=SEED, step=STEP)
    hip.set_precision("f32")
    assert precision() == 0
    r3 = fwd_v(hip)
    born = _hip(net)                                                                   # images built by set_weights
    rb = fwd(born)
    # new weights in bf16 mode: a fresh bf16 handle's results
    net2 = ref.net(True, 13).cuda()
    born.load(net2)
    rn, rf = fwd(born), fwd(_hip(net2))
    torch.cuda.synchronize()
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b) if x is not None)   # noqa: E731
    assert same(r1, r2) and same(r1, rb)
    assert same(r0, r3) and same(r0, never) and r0[1] is not None
    assert same(dense, packed) and same(dense, cleared)
    assert same(rn, rf) and not torch.equal(rn[0], r1[0])
    d = float((r1[0] - r0[0]).abs().max())
    assert 0.0 < d < 0.1, d                                                            # another mode, the same network


# ------------------------------------------------------------------------------------------------- 6: the row map
def _engine(E=8, map_size=40, n_side=40, max_steps=400, seed=5):
    import torch
    from mfrl_amd.battle import BattleBatch
    placement = list(bd.block_positions(map_size, n_side))
    eng = BattleBatch(map_size, E, stream=torch.cuda.current_stream())
    eng.rollout_init(placement, max_steps=max_steps, eps=0.2, seed=seed, stagger=True)
    return eng, placement


def test_act_rollout_bf16_matches_dense_forward():
    """8 staggered envs of 40 x 40 after 12 rollout steps: act_rollout writes for every live row e * rowcap + j of
    group g the draw (seed, step, g, e * rowcap + j) on the policy the dense bf16 forward gives on that row's view and
    features gathered by hand; rows past the live count are untouched."""
    import torch
    E = 8
    eng, _ = _engine(E)
    eng.rollout_step(12)
    eng.rollout_policy_observe()
    rc = eng.rowcap
    pols = [_hip(ref.net(True, 31 + g).cuda()) for g in range(2)]
    eng.rollout_write("actions", torch.full((E, 2, rc), -7, dtype=torch.int32, device="cuda"))
    for g in range(2):
        pols[g].act_rollout(eng, g, seed=SEED, step=STEP)
    act = torch.empty((E, 2, rc), dtype=torch.int32, device="cuda")
    num = torch.empty((E, 2), dtype=torch.int32, device="cuda")
    eng.rollout_copy("actions", act)
    eng.rollout_copy("group_num", num)
    live_n = 0
    for g in range(2):
        view = torch.empty((E, rc, 1183), dtype=torch.float32, device="cuda")
        feat = torch.empty((E, rc, 34), dtype=torch.float32, device="cuda")
        eng.rollout_copy("view", view, group=g)
        eng.rollout_copy("feature", feat, group=g)
        eng.sync()
        live = torch.arange(rc, device="cuda")[None, :] < num[:, g:g + 1]
        pol = pols[g].forward(view[live], feat[live], want_act=False)[0]
        torch.cuda.synchronize()
        rows = live.reshape(-1).nonzero().reshape(-1).cpu().numpy()                     # e * rowcap + j
        want = acnet_ref.draw(pol.cpu().numpy(), SEED, STEP, g, rows)
        assert np.array_equal(act[:, g][live].cpu().numpy(), want), g
        assert bool((act[:, g][~live] == -7).all()), g
        live_n += int(live.sum())
        assert int(live.sum()) > _header_constant("kAB16Rows")            # (more than one workgroup's rows)
        assert len(np.unique(want)) > 3
    assert live_n < E * 2 * rc                                            # (and some rows are not live)


# ------------------------------------------------------------------------------------------------- 7: in the loop
def test_bf16_policy_in_the_loop():
    """Two bf16 MFAC networks drive rollout_policy_step for 30 steps on 8 envs of 40 x 40; the sampled envs are then
    replayed on the C oracle from rollout_init with the actions the device recorded at every step, and the final
    views, features, rewards, mean actions and group sizes must agree bit for bit (scripts/bench_policy_env.py)."""
    import torch
    E, T, max_steps, map_size = 8, 30, 20, 40
    eng, placement = _engine(E, max_steps=max_steps, seed=7)
    rc = eng.rowcap
    pols = [_hip(ref.net(True, 41 + g).cuda()) for g in range(2)]
    picks = rck.sample_envs(E, 3)
    log = torch.empty((T, len(picks), 2, rc), dtype=torch.int32, device="cuda")
    eng.rollout_policy_observe()
    for t in range(T):
        for g in range(2):
            pols[g].act_rollout(eng, g, seed=SEED, step=t)
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
    assert len(kinds) > 3 and restarts >= 2


# ------------------------------------------------------------------------------------------------- 8: ActorCritic
def test_actor_critic_act_precision(rows):
    """ActorCritic.act_precision = "bf16": act_dev returns what a bf16 ACNetHIP loaded from the net returns with the
    model's seed and draw count; the gradients of train_rollout(step=False) on the same collected rows are bitwise
    equal under both settings (the bootstrap value stays on the f32 forward)."""
    import torch
    from mfrl_amd.algo.ac import ActorCritic
    from test_collect_ac_gpu import _engine as collect_engine, _model, _scripted
    assert ActorCritic.act_precision == "f32"
    view, feat = (x[:500] for x in rows)
    grads = {}
    for precision in ("f32", "bf16"):
        m, _ = _model("mfac", "mfac-" + precision)
        m.seed = 99                                     # (the name is part of the seed: the same draws for both)
        m.act_precision = precision
        got = m.act_dev(state=[view.reshape(-1, 13, 13, 7), feat])
        assert m._hip.precision == precision and m._draws == 1
        want = _hip(m.net, precision=precision).act(view, feat, seed=99, step=1)
        torch.cuda.synchronize()
        assert torch.equal(got, want)
        grads[precision] = got
        eng = collect_engine("few")
        n = _scripted(eng, m.rollout_collector(eng, 0))
        assert n > 1000
        grads[precision + "-g"] = m.train_rollout(step=False)
        assert m._hip.precision == "f32"                # the bootstrap value came from the f32 forward
        m.act_dev(state=[view.reshape(-1, 13, 13, 7), feat])
        assert m._hip.precision == precision
    assert float((grads["f32"] == grads["bf16"]).float().mean()) > 0.9
    for a, b in zip(grads["f32-g"], grads["bf16-g"]):
        assert (a is None) == (b is None)
        assert a is None or torch.equal(a, b)
