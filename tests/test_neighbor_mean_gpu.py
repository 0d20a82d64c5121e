"""The opt-in neighbourhood mean action on the GPU (csrc/neighbor_kernels.hip): the stand-alone kernel on
synthetic lists and the rollout form on three rollout plans against the numpy restatement (tests/neighbor_mean_ref.py)
with the C oracle in lockstep, bit for bit; the per-row mean through the Q forward's rollout form and the collector;
the models, the rollout loops and the train_battle switch."""
import os

import numpy as np
import pytest

import common
import neighbor_mean_ref as nr

pytestmark = pytest.mark.gpu
VS, FS, NA, VF, F = (13, 13, 7), (34,), 21, 13 * 13 * 7, 34
SENTINEL = -3.0


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ------------------------------------------------------------------------------------------------- 1: the kernel
def _cells(rng, W, H, n):
    """n distinct cells of the W x H map: the four corners and border cells first (the window clamps there), the
    rest a seeded sample; then shuffled, so that the corners sit at any row."""
    corners = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    border = [(x, y) for x in range(W) for y in range(H) if x in (0, W - 1) or y in (0, H - 1)]
    border = [border[i] for i in rng.permutation(len(border))[:8]]
    rest = [(int(i) % W, int(i) // W) for i in rng.permutation(W * H)]
    seen, out = set(), []
    for c in corners + border + rest:
        if c not in seen:
            seen.add(c)
            out.append(c)
        if len(out) == n:
            break
    return np.asarray([out[i] for i in rng.permutation(n)], dtype=np.int32).reshape(n, 2)


def _counts(B, rowcap):
    mid = max(rowcap // 2, 1)
    if B == 1:
        return [[c] for c in sorted({0, 1, rowcap, mid})]
    return [[rowcap, mid, 0], [1, rowcap, mid]]


@pytest.mark.parametrize("W,H", [(16, 16), (40, 23)])
@pytest.mark.parametrize("n_action", [2, 21, 64])
def test_kernel_equals_the_restatement(W, H, n_action):
    """B in {1, 3}, rowcap in {1, 63, 64, 65, 130}, counts 0 / 1 / rowcap / one between, R in {0, 1, 6, 100}, on a
    square and a non-square map with cells on the borders and in the corners; n_action = 21 also carries actions
    outside [0, n_action).  Bit for bit the restatement; rows past the count keep the sentinel."""
    import torch
    from mfrl_amd import mf
    rng = np.random.RandomState(W * 1000 + n_action)
    for B in (1, 3):
        for rowcap in (1, 63, 64, 65, 130):
            for counts in _counts(B, rowcap):
                pos = np.stack([_cells(rng, W, H, rowcap) for _ in range(B)])
                act = rng.randint(0, n_action, size=(B, rowcap)).astype(np.int32)
                if n_action == 21:
                    bad = rng.random_sample((B, rowcap)) < 0.1
                    act[bad] = rng.choice([-1, 21, 63], size=int(bad.sum()))
                    if rowcap > 1:
                        act[:, 0], act[:, 1] = -1, 63
                d_pos, d_act, d_cnt = _cuda(pos), _cuda(act), _cuda(np.asarray(counts, dtype=np.int32))
                for R in (0, 1, 6, 100):
                    out = torch.full((B, rowcap, n_action), SENTINEL, dtype=torch.float32, device="cuda")
                    got = mf.neighbor_mean(d_pos, d_act, d_cnt, n_action, R, W, H, out=out).cpu().numpy()
                    for b, n in enumerate(counts):
                        want = nr.compact(pos[b, :n], act[b, :n], n_action, R)
                        assert got[b, :n].tobytes() == want.tobytes(), (B, rowcap, counts, R, b)
                        assert (got[b, n:] == SENTINEL).all(), (B, rowcap, counts, R, b)
                        if R == 0:
                            ok = (act[b, :n] >= 0) & (act[b, :n] < n_action)
                            one_hot = np.zeros((n, n_action), dtype=np.float32)
                            one_hot[np.nonzero(ok)[0], act[b, :n][ok]] = 1
                            assert got[b, :n].tobytes() == one_hot.tobytes()


def test_kernel_refusals():
    import torch
    from magent.c_lib import EngineError
    from mfrl_amd import mf
    pos = torch.zeros((2, 4, 2), dtype=torch.int32, device="cuda")
    act = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
    cnt = torch.ones(2, dtype=torch.int32, device="cuda")
    assert mf.neighbor_mean(pos, act, cnt, 3, 1, 8, 8).shape == (2, 4, 3)
    for args in ((pos.long(), act, cnt), (pos.float(), act, cnt), (pos, act.long(), cnt), (pos, act, cnt.long())):
        with pytest.raises(TypeError):
            mf.neighbor_mean(*args, 3, 1, 8, 8)
    with pytest.raises(TypeError):
        mf.neighbor_mean(pos, act, cnt, 3, 1, 8, 8, out=torch.zeros((2, 4, 3), dtype=torch.float64, device="cuda"))
    for args in ((pos[:, :3], act, cnt), (pos, act, cnt[:1]), (pos[..., :1], act, cnt), (pos, act.reshape(-1), cnt)):
        with pytest.raises(ValueError):
            mf.neighbor_mean(*args, 3, 1, 8, 8)
    with pytest.raises(ValueError):
        mf.neighbor_mean(pos, act, cnt, 3, 1, 8, 8, out=torch.zeros((2, 4, 4), device="cuda"))
    for n_action in (0, 65):
        with pytest.raises(EngineError, match="n_action"):
            mf.neighbor_mean(pos, act, cnt, n_action, 1, 8, 8)
    with pytest.raises(EngineError, match="radius"):
        mf.neighbor_mean(pos, act, cnt, 3, -1, 8, 8)
    with pytest.raises(EngineError, match="limit"):
        mf.neighbor_mean(pos, act, cnt, 3, 1, 512, 512)
    assert mf.neighbor_mean(pos, act, cnt, 3, 1, 256, 256).shape == (2, 4, 3)      # (64 KB of grid fits)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- 2: the rollout form
def _engine(map_size, E, small_e, placement, max_steps):
    import torch
    from mfrl_amd.battle import BattleBatch
    old = os.environ.get("MFX_SMALL_E")
    if small_e is not None:
        os.environ["MFX_SMALL_E"] = small_e
    try:
        eng = BattleBatch(map_size, E, stream=torch.cuda.current_stream())
        eng.rollout_init(placement, max_steps=max_steps, eps=0.0, seed=1, stagger=False)
    finally:
        if small_e is not None:
            if old is None:
                del os.environ["MFX_SMALL_E"]
            else:
                os.environ["MFX_SMALL_E"] = old
    return eng


# name: (map size, envs, MFX_SMALL_E, steps, rollout_policy_path, radii compared with the restatement, the radius
# compared with the rollout's mean_action on the steps without a death or None).  "large": 288 is the first multiple of
# 32 whose cell array alone (2 bytes per cell) is past the 160 KiB of LDS, so the env takes the large-env plan, whose
# clear_dead renumbers the slots, whatever the agent count.
ROLLOUTS = {
    "fused": (40, 3, "0", 30, "k_rollout", (1, 6), 64),
    "few": (40, 8, None, 30, "k_observe_items+k_rollout_big", (1, 6), 64),
    "large": (288, 2, None, 15, "k_observe_items+k_rollout_big", (6,), None),
}
MAX_STEPS = 12


@pytest.mark.parametrize("plan", list(ROLLOUTS))
def test_rollout_form_equals_the_restatement(plan):
    """The checkerboard block, the test's own actions (RandomState(7 + e), 60 % attacks) and every env replayed in
    lockstep on the C oracle, which alone fixes who dies.  After every step, for both groups: NeighborMean.rows equal
    the restatement on the oracle's positions and alive flags bit for bit -- the rows of the survivors, zero at a
    restart, the rows past the count as they were --, and with R = 64 on the steps without a death every row is the
    rollout's mean_action cast to float."""
    import torch
    from mfrl_amd import mf
    map_size, E, small_e, steps, path, radii, r_all = ROLLOUTS[plan]
    placement = nr.checkerboard(map_size, map_size, 8)
    eng = _engine(map_size, E, small_e, placement, MAX_STEPS)
    assert eng.rollout_policy_path() == path
    if plan == "fused":
        assert eng.rollout_path() == "k_rollout"
    rc = eng.rowcap
    all_r = list(radii) + ([r_all] if r_all is not None else [])
    nms = {(g, R): mf.NeighborMean(eng, g, R) for g in range(2) for R in all_r}
    want = {k: np.full((E, rc, NA), SENTINEL, dtype=np.float32) for k in nms}
    for nm in nms.values():
        assert nm.rows.shape == (E, rc, NA) and nm.rows.dtype == torch.float32
        nm.rows.fill_(SENTINEL)
    oracles, rngs, ep_len = [], [np.random.RandomState(7 + e) for e in range(E)], [0] * E
    for e in range(E):
        env, h = common.battle_env(common.ORACLE_LIB, map_size)
        env.reset()
        for g in range(2):
            env.add_agents(h[g], method="custom", pos=placement[g])
        oracles.append((env, h))
    attack_base = oracles[0][0].get_view2attack(oracles[0][1][0])[0]
    eng.rollout_policy_observe()
    for k, nm in nms.items():
        nm.reset()
        want[k][:, :len(placement[k[0]])] = 0
    eng.sync()
    for k, nm in nms.items():
        assert nm.rows.cpu().numpy().tobytes() == want[k].tobytes(), ("reset", k)
    deaths, restarts, moved, plain_steps = 0, [0] * E, 0, 0
    keep = []
    for t in range(steps):
        actn = np.zeros((E, 2, rc), dtype=np.int32)
        prev = np.zeros((E, 2), dtype=np.int64)
        for e, (env, h) in enumerate(oracles):
            for g in range(2):
                prev[e, g] = len(env.get_agent_id(h[g]))
                actn[e, g, :prev[e, g]] = nr.draw_actions(rngs[e], prev[e, g], NA, attack_base)
        keep.append(_cuda(actn))                     # (kept: the engine's stream copies it asynchronously)
        eng.rollout_write("actions", keep[-1])
        eng.rollout_policy_step()
        for nm in nms.values():
            nm.update()
        mean = torch.empty((E, 2, eng.mean_stride()), dtype=torch.float64, device="cuda")
        eng.rollout_copy("mean_action", mean)
        eng.sync()
        mean = mean.cpu().numpy()
        got = {k: nm.rows.cpu().numpy() for k, nm in nms.items()}
        for e, (env, h) in enumerate(oracles):
            for g in range(2):
                env.set_action(h[g], np.ascontiguousarray(actn[e, g, :prev[e, g]]))
            done = env.step()
            alive = [env.get_alive(h[g]).copy() for g in range(2)]
            env.clear_dead()
            ep_len[e] += 1
            restart = bool(done) or ep_len[e] >= MAX_STEPS
            if restart:
                ep_len[e] = 0
                restarts[e] += 1
                env.reset()
                for g in range(2):
                    env.add_agents(h[g], method="custom", pos=placement[g])
            for g in range(2):
                pos = env.get_pos(h[g])
                n = len(pos)
                dead = alive[g] == 0
                if not restart:
                    deaths += int(dead.sum())
                    moved += int(dead[:-1].any())
                for R in all_r:
                    want[(g, R)][e, :n] = nr.rollout(actn[e, g], alive[g], int(prev[e, g]), pos, NA, R, restart)
                    assert got[(g, R)][e].tobytes() == want[(g, R)][e].tobytes(), (t, e, g, R, restart)
                    if restart:
                        assert not got[(g, R)][e, :n].any()
                if r_all is not None and not dead.any():
                    group_mean = mean[e, g, :NA].astype(np.float32)
                    assert got[(g, r_all)][e, :n].tobytes() == np.tile(group_mean, (n, 1)).tobytes(), (t, e, g)
                    plain_steps += 1
    eng.rollout_check()
    assert deaths >= 10 and moved >= 1, (deaths, moved)
    if steps > MAX_STEPS:
        assert min(restarts) >= 1, restarts
    if r_all is not None:
        assert plain_steps >= 5


def test_rollout_form_refusals():
    """A group whose features carry no position (minimap_mode off) is refused by both calls; a negative radius by the
    constructor."""
    import magent
    import torch
    from magent.c_lib import EngineError
    from mfrl_amd import mf
    from mfrl_amd.battle import BattleBatch
    gw = magent.gridworld
    cfg = gw.Config()
    cfg.set({"map_width": 40, "map_height": 40, "minimap_mode": False, "embedding_size": 10})
    small = cfg.register_agent_type("small", dict(width=1, length=1, hp=10, speed=2, damage=2, step_recover=0.1,
                                                  step_reward=-0.005, kill_reward=5, dead_penalty=-0.1,
                                                  attack_penalty=-0.1, view_range=gw.CircleRange(6),
                                                  attack_range=gw.CircleRange(1.5)))
    armies = [cfg.add_group(small), cfg.add_group(small)]
    a, b = (gw.AgentSymbol(g, index="any") for g in armies)
    cfg.add_reward_rule(gw.Event(a, "attack", b), receiver=a, value=0.2)
    cfg.add_reward_rule(gw.Event(b, "attack", a), receiver=b, value=0.2)
    eng = BattleBatch(40, 2, config=cfg, stream=torch.cuda.current_stream())
    eng.rollout_init(nr.checkerboard(40, 40, 4), max_steps=5, eps=0.0, seed=1, stagger=False)
    nm = mf.NeighborMean(eng, 0, 2)
    with pytest.raises(EngineError, match="minimap_mode"):
        nm.reset()
    with pytest.raises(EngineError, match="minimap_mode"):
        nm.update()
    with pytest.raises(ValueError):
        mf.NeighborMean(eng, 0, -1)
    eng.sync()


# ------------------------------------------------------------------------------------------------- 3: the forward
def _net(use_mf, seed):
    import torch
    from mfrl_amd.algo.nets import QNet
    torch.manual_seed(seed)
    net = QNet(VS, FS, NA, use_mf).cuda()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return net


_STATE = {}


def _mid_rollout():
    """4 envs of 40 x 40 from a 16 x 16 checkerboard block (128 agents per side), six steps of seeded actions (60 %
    attacks) in: the engine, its observation buffers, group sizes and mean actions (device tensors; made once, never
    modified)."""
    import torch
    if _STATE:
        return _STATE
    E = 4
    eng = _engine(40, E, None, nr.checkerboard(40, 40, 16), 400)
    eng.rollout_policy_observe()
    rng = np.random.RandomState(9)
    keep = []
    for _ in range(6):
        keep.append(_cuda(nr.draw_actions(rng, E * 2 * eng.rowcap, NA, 13).reshape(E, 2, eng.rowcap)))
        eng.rollout_write("actions", keep[-1])
        eng.rollout_policy_step()
    rc = eng.rowcap
    st = {"eng": eng, "E": E, "rc": rc}
    for g in range(2):
        st["view%d" % g] = torch.empty((E, rc, VF), dtype=torch.float32, device="cuda")
        st["feat%d" % g] = torch.empty((E, rc, F), dtype=torch.float32, device="cuda")
        eng.rollout_copy("view", st["view%d" % g], group=g)
        eng.rollout_copy("feature", st["feat%d" % g], group=g)
    st["num"] = torch.empty((E, 2), dtype=torch.int32, device="cuda")
    st["mean"] = torch.empty((E, 2, eng.mean_stride()), dtype=torch.float64, device="cuda")
    eng.rollout_copy("group_num", st["num"])
    eng.rollout_copy("mean_action", st["mean"])
    eng.sync()
    assert 0 < int(st["num"].min()) and int(st["num"].min()) < rc            # (rows past the count exist)
    _STATE.update(st)
    return _STATE


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_act_rollout_reads_the_rows_own_mean(precision):
    """act_rollout(prob_rows=P), P random: the live rows' actions are the dense forward's on (view, feature, P) of
    those rows bit for bit, greedy and sampled (row index e * rowcap + j); rows past the count are untouched.  The
    default guard: without prob_rows the actions are the dense forward's on the env's mean, and P = that mean
    expanded gives the same actions."""
    import torch
    from mfrl_amd import mf
    from mfrl_amd.policy import QNetHIP
    st = _mid_rollout()
    eng, E, rc = st["eng"], st["E"], st["rc"]
    T, seed = 0.5, 4242
    slot = torch.arange(E * rc, dtype=torch.int32, device="cuda").reshape(E, rc)
    torch.manual_seed(11)
    P = torch.rand((E, rc, NA), dtype=torch.float32, device="cuda")
    P /= P.sum(-1, keepdim=True)
    differ = 0
    for g in range(2):
        hip = QNetHIP(VS, FS, NA, True, precision=precision).load(_net(True, 40 + g))
        live = torch.arange(rc, device="cuda")[None, :] < st["num"][:, g:g + 1]
        view, feat = st["view%d" % g][live].reshape(-1, 13, 13, 7), st["feat%d" % g][live]
        group_mean = st["mean"][:, g:g + 1, :NA].expand(E, rc, NA).float().contiguous()

        def run(**kw):
            eng.rollout_write("actions", torch.full((E, 2, rc), -7, dtype=torch.int32, device="cuda"))
            hip.act_rollout(eng, g, **kw)
            act = torch.empty((E, 2, rc), dtype=torch.int32, device="cuda")
            eng.rollout_copy("actions", act)
            eng.sync()
            assert bool((act[:, g][~live] == -7).all()) and bool((act[:, 1 - g] == -7).all())
            return act[:, g][live]

        q, greedy = hip.forward(view, feat, P[live])
        assert torch.equal(run(prob_rows=P), greedy), (g, "greedy")
        sampled = mf.q_sample(q, T, seed, 3, group=g, rows=slot[live].contiguous())
        assert torch.equal(run(prob_rows=P, temperature=T, seed=seed, step=3), sampled), (g, "sampled")
        q0, greedy0 = hip.forward(view, feat, group_mean[live])
        sampled0 = mf.q_sample(q0, T, seed, 3, group=g, rows=slot[live].contiguous())
        assert torch.equal(run(), greedy0) and torch.equal(run(prob_rows=group_mean), greedy0), (g, "default")
        assert torch.equal(run(temperature=T, seed=seed, step=3), sampled0), (g, "default sampled")
        assert torch.equal(run(prob_rows=group_mean, temperature=T, seed=seed, step=3), sampled0)
        differ += int((q != q0).any(1).sum())
        for bad in (P.double(), P[:, :-1], P[..., :-1], P.cpu()):
            with pytest.raises(ValueError):
                hip.act_rollout(eng, g, prob_rows=bad)
    assert differ > 0                                # (the per-row mean reaches the Q values)


# ------------------------------------------------------------------------------------------------- 4: the collector
def _collect_once(linked, P):
    """One scripted step of a fresh 40 x 40 / 3-env rollout collected with prob_rows=P (None: the default): the
    columns of the new rows (host copies) and the (env, row) of each."""
    import torch
    from mfrl_amd.algo.tools import EpisodesBuffer, MemoryGroup
    from mfrl_amd.replay import RolloutCollector
    E = 3
    placement = nr.checkerboard(40, 40, 8)
    eng = _engine(40, E, None, placement, 50)
    rc = eng.rowcap
    if linked:
        buf = EpisodesBuffer(use_mean=True)
        buf.prepare(VS, FS, NA)
    else:
        buf = MemoryGroup(VS, FS, NA, 1000, 64, 8, use_mean=True)
    eng.rollout_policy_observe()
    rng = np.random.RandomState(5)
    acts = [_cuda(rng.randint(0, NA, size=(E, 2, rc)).astype(np.int32)) for _ in range(2)]
    eng.rollout_write("actions", acts[0])
    eng.rollout_policy_step()                        # (one step first: the env's mean action is no longer zero)
    num = torch.empty((E, 2), dtype=torch.int32, device="cuda")
    eng.rollout_copy("group_num", num)
    col = RolloutCollector(eng, buf, 0, prob_rows=P(E, rc) if P is not None else None)
    assert col.linked == linked
    eng.rollout_write("actions", acts[1])
    col.begin()
    eng.rollout_policy_step()
    col.end()
    n = col.finish()
    eng.rollout_check()
    num = num.cpu().numpy()
    where = [(e, j) for e in range(E) for j in range(num[e, 0])]
    assert n == len(where)
    return {k: v[:n].cpu().numpy() for k, v in buf._rows.cols.items()}, where, col


@pytest.mark.parametrize("linked", [False, True])
def test_collector_takes_the_rows_own_mean(linked):
    """One step collected with prob_rows=P: the prob column of row (e, j) is P[e, j] byte for byte and every other
    column is that of a collector without prob_rows, whose prob column is the env's mean; on the unlinked and the
    linked path."""
    import torch
    torch.manual_seed(3)
    held = {}

    def P(E, rc):
        held["P"] = torch.rand((E, rc, NA), dtype=torch.float32, device="cuda")
        return held["P"]

    got, where, col = _collect_once(linked, P)
    ref, where0, _ = _collect_once(linked, None)
    assert where == where0 and set(got) == set(ref)
    Ph = held["P"].cpu().numpy()
    want = np.stack([Ph[e, j] for e, j in where])
    assert got["prob"].tobytes() == want.tobytes()
    for k in ref:
        if k != "prob":
            assert got[k].tobytes() == ref[k].tobytes(), k
    env_of = np.asarray([e for e, _ in where])
    for e in set(env_of.tolist()):                   # the default: one mean per env, not zero after a step
        rows = ref["prob"][env_of == e]
        assert (rows == rows[0]).all() and rows[0].any() and abs(float(rows[0].sum()) - 1) < 1e-5
    col.prob_rows = held["P"][:, :-1]
    with pytest.raises(ValueError):
        col.begin()


# ------------------------------------------------------------------------------------------------- 5: models, loops, CLI
def _models(algo, max_steps):
    import magent
    import torch
    from mfrl_amd.algo import spawn_ai
    env = magent.GridWorld("battle", map_size=40)
    h = env.get_handles()
    torch.manual_seed(3)
    return [spawn_ai(algo, None, env, h[g], "%s-%d" % (algo, g), max_steps, memory_size=4000) for g in range(2)]


@pytest.mark.parametrize("algo", ["mfq", "mfac"])
def test_rollout_round_stores_the_neighbourhood_mean(algo, monkeypatch):
    """One short training round of 4 envs of 40 x 40 with mean_field = "neighbors" (MFQ through play_rollout, MFAC
    through play_rollout_episodes): the prob column of the collected rows is NeighborMean.rows as it stood at each
    step's begin(), row for row, and the rows of one step differ from each other -- what one mean per env cannot
    give.  A model left at "group" makes no NeighborMean."""
    import torch
    from mfrl_amd.algo.play import play_rollout, play_rollout_episodes
    from mfrl_amd.battle import BattleBatch
    from mfrl_amd.replay import RolloutCollector
    E, max_steps = 4, 8
    models = _models(algo, max_steps)
    models[0].mean_field = "neighbors"
    models[0].mf_radius = 2
    if algo == "mfq":
        for m in models:
            m.explore = "boltzmann"                  # (an untrained greedy net picks one action for everybody)
    eng = BattleBatch(40, E, stream=torch.cuda.current_stream())
    snaps, held = [], {}
    real_begin = RolloutCollector.begin

    def begin(self):
        num = torch.empty((E, 2), dtype=torch.int32, device="cuda")
        self.eng.rollout_copy("group_num", num)
        assert self.prob_rows is models[0]._neighbor_means[0].rows
        snaps.append((self.prob_rows.clone(), num))
        real_begin(self)

    def train():                                     # (the rows stay where the collector put them)
        rows = models[0].replay_buffer._rows
        held.update({k: v[:rows.n].clone() for k, v in rows.cols.items()})

    monkeypatch.setattr(RolloutCollector, "begin", begin)
    monkeypatch.setattr(models[0], "train" if algo == "mfq" else "train_rollout", train, raising=True)
    loop = play_rollout if algo == "mfq" else play_rollout_episodes
    loop(eng, 0, 40, max_steps, models, eps=1.0, train=True, left_id=0)
    assert len(snaps) == max_steps and "_neighbor_means" not in models[1].__dict__
    want, varied = [], 0
    for t, (rows, num) in enumerate(snaps):
        rows, num = rows.cpu().numpy(), num.cpu().numpy()
        for e in range(E):
            want.append(rows[e, :num[e, 0]])
            varied += t > 0 and bool((rows[e, :num[e, 0]] != rows[e, 0]).any())
        if t == 0:
            assert not rows[:, :64].any()            # (an episode starts from a zero mean)
    want = np.concatenate(want)
    got = held["prob"].cpu().numpy()
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
    assert varied >= E


def test_train_battle_mean_field_runs(tmp_path, capsys):
    from mfrl_amd import train_battle
    train_battle.main(["--algo", "mfq", "--rollout", "--envs", "4", "--mean_field", "neighbors", "--mf_radius", "2",
                       "--n_round", "1", "--max_steps", "10", "--map_size", "40", "--base_dir", str(tmp_path)])
    out = capsys.readouterr().out
    assert "device rollout" in out and "replay rows" in out and "[TIME] round 0" in out


def test_battle_rollout_with_a_neighbors_model():
    """battle_rollout takes the mode: an evaluation round of an MFQ "neighbors" model against an MFAC one runs and
    scores its E episodes."""
    import torch
    from mfrl_amd.algo.play import battle_rollout
    from mfrl_amd.battle import BattleBatch
    E, max_steps = 3, 12
    models = [_models("mfq", max_steps)[0], _models("mfac", max_steps)[1]]
    for m in models:
        m.mean_field = "neighbors"
    eng = BattleBatch(40, E, stream=torch.cuda.current_stream())
    out = battle_rollout(eng, 0, 40, max_steps, models, eps=0.0, left_id=0)
    assert int(out[4]["totals"][:, 0].sum()) >= E
    assert models[0]._neighbor_means[0].radius == 6 and models[1]._neighbor_means[1].group == 1
