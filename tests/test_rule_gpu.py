"""The scripted rush / random opponent on the GPU (csrc/rule_kernels.hip): k_rule_act on synthetic and real
rows against the numpy restatement (tests/rule_ref.py); two rule policies driving a rollout that is replayed on the C
oracle; RulePolicy on the host loop; battle_eval and train_battle --eval_every with a rule side; the refusals.
Everything is integer equality."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import battle_driver as bd
import common
import rule_cases as rc
import rule_ref as rr

pytestmark = pytest.mark.gpu
VS, FS, NA = (13, 13, 7), (34,), 21
MOVE2 = rr.circle_moves(2)


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ------------------------------------------------------------------------------------------------- 1: the compact form
_tables, _synthetic = rc.tables, rc.synthetic          # (shared with tests/test_rule_shapes_gpu.py)


@pytest.mark.parametrize("shape", [(5, 5), (13, 13), (15, 15)])
def test_compact_form_matches_restatement(shape):
    """Synthetic rows of three view sizes, n = 1, 63, 65, 1000: the kernel's actions are the restatement's; among the
    1000 rows every branch tag and a refused best move occur; another step draws other random rows, the same step the
    same ones."""
    import torch
    from mfrl_amd.policy import RuleHIP
    VH, VW = shape
    v2a, base, n_action, move = _tables(VH, VW)
    view, feat = _synthetic(VH, VW)
    hip = RuleHIP((VH, VW, 7), (12,), n_action, base, v2a, move)
    dv, df = _cuda(view), _cuda(feat)
    eps, seed = 0.2, 4242
    for n in (1, 63, 65, 1000):
        got = hip.act(dv[:n], df[:n], eps=eps, seed=seed, step=n, group=n % 2)
        torch.cuda.synchronize()
        want, tag, refused = rr.rule_actions(view[:n], feat[:n], v2a, base, n_action, move, eps, seed, n, n % 2)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (shape, n)
    counts = np.bincount(tag, minlength=5)
    print("%s: tags %s, refused %d" % (shape, dict(zip(rr.TAG_NAMES, counts.tolist())), int(refused.sum())))
    assert (counts >= 1).all() and refused.sum() >= 1
    assert 0 <= want.min() and want.max() < n_action and len(np.unique(want)) > base        # moves and attacks
    again = hip.act(dv, df, eps=eps, seed=seed, step=1000, group=0).cpu().numpy()
    other = hip.act(dv, df, eps=eps, seed=seed, step=1001, group=0).cpu().numpy()
    assert np.array_equal(again, want)
    w2, t2, _ = rr.rule_actions(view, feat, v2a, base, n_action, move, eps, seed, 1001, 0)
    assert np.array_equal(other, w2) and not np.array_equal(t2 == rr.TAG_RANDOM, tag == rr.TAG_RANDOM)
    # eps 0 draws nothing, eps 1 is the random opponent
    for e, kind in ((0.0, False), (1.0, True)):
        got = hip.act(dv, df, eps=e, seed=seed, step=3).cpu().numpy()
        want, tag, _ = rr.rule_actions(view, feat, v2a, base, n_action, move, e, seed, 3, 0)
        assert np.array_equal(got, want) and ((tag == rr.TAG_RANDOM) == kind).all()
    assert hip.act(dv[:0], df[:0]).shape == (0,)


_OBS = {}


def _rollout_obs(E=64, steps=30):
    """Live-agent rows (views, features) of both groups of a 64 x 64 rush rollout after `steps` steps (the helper
    pattern of tests/test_qsample_gpu.py); made once, never modified."""
    import torch
    from mfrl_amd.battle import BattleBatch
    if (E, steps) in _OBS:
        return _OBS[(E, steps)]
    left, right = bd.block_positions(64, 128)
    eng = BattleBatch(64, E, stream=torch.cuda.current_stream())
    eng.rollout_init([left, right], max_steps=400, eps=0.2, seed=5, stagger=True)
    eng.rollout_step(steps)
    rc = eng.rowcap
    num = torch.empty((E, 2), dtype=torch.int32, device="cuda")
    eng.rollout_copy("group_num", num)
    out = []
    for g in range(2):
        view = torch.empty((E, rc, 1183), dtype=torch.float32, device="cuda")
        feat = torch.empty((E, rc, 34), dtype=torch.float32, device="cuda")
        eng.rollout_copy("view", view, group=g)
        eng.rollout_copy("feature", feat, group=g)
        eng.sync()
        live = torch.arange(rc, device="cuda")[None, :] < num[:, g:g + 1]
        out.append((view[live].reshape(-1, 13, 13, 7)[:600].clone(), feat[live][:600].clone()))
    _OBS[(E, steps)] = out
    return out


def _battle_tables():
    import magent
    env = magent.GridWorld("battle", map_size=64)
    h = env.get_handles()
    base, v2a = env.get_view2attack(h[0])
    move = env.get_move_delta(h[0])
    assert np.array_equal(move, MOVE2)
    return env, h, v2a, base, move


def test_real_rows_match_restatement():
    import torch
    from mfrl_amd.policy import RuleHIP
    _, _, v2a, base, move = _battle_tables()
    hip = RuleHIP(VS, FS, NA, base, v2a, move)
    seen = np.zeros(5, dtype=np.int64)
    for g, (view, feat) in enumerate(_rollout_obs()):
        got = hip.act(view, feat, eps=0.1, seed=7, step=2, group=g)
        torch.cuda.synchronize()
        want, tag, _ = rr.rule_actions(view.cpu().numpy(), feat.cpu().numpy(), v2a, base, NA, move, 0.1, 7, 2, g)
        assert len(want) == 600 and np.array_equal(got.cpu().numpy(), want), g
        seen += np.bincount(tag, minlength=5)
    print("real rows: tags %s" % dict(zip(rr.TAG_NAMES, seen.tolist())))
    assert seen[rr.TAG_A] and seen[rr.TAG_B] and seen[rr.TAG_RANDOM]


# ------------------------------------------------------------------------------------------------- 2: the rollout
def _columns():
    """Two columns of four, 3 cells apart, and one straggler per side that sees nobody: A, B and C from the start."""
    left = [[29, y, 0] for y in (28, 30, 32, 34)] + [[6, 6, 0]]
    right = [[32, y, 0] for y in (28, 30, 32, 34)] + [[57, 57, 0]]
    return left, right


@pytest.mark.parametrize("E,small_e,steps,plan", [(3, "0", 12, "k_rollout"), (8, None, 5, None)])
def test_rule_rollout_matches_oracle(E, small_e, steps, plan, monkeypatch):
    """Two rule policies at eps = 0.1 drive both groups of a rollout (act_rollout + rollout_policy_step), 3 envs on
    the fused plan and 8 on the few-env plan, max_steps 5 so every env restarts.  Per step the live action rows are the
    restatement's on the oracle's own observations with row = e * rowcap + j, the rows past each count keep the -7
    sentinel, and every env is replayed on the C oracle: rewards, views, features and mean actions bit for bit."""
    import torch
    from mfrl_amd.battle import BattleBatch
    from mfrl_amd.policy import RuleHIP
    if small_e is not None:
        monkeypatch.setenv("MFX_SMALL_E", small_e)
    max_steps, VF, F, eps, seed = 5, 1183, 34, 0.1, 2024
    left, right = _columns()
    eng = BattleBatch(64, E, stream=torch.cuda.current_stream())
    eng.rollout_init([left, right], max_steps=max_steps, eps=0.0, seed=1, stagger=False)
    if plan:
        assert eng.rollout_path() == plan
    else:
        assert eng.rollout_path() != "k_rollout"                       # (the few-env plan: another step kernel)
    _, _, v2a, base, move = _battle_tables()
    pols = [RuleHIP(VS, FS, NA, base, v2a, move) for _ in range(2)]
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

    restarts, tags = 0, np.zeros(5, dtype=np.int64)
    for t in range(steps):
        eng.rollout_write("actions", torch.full((E, 2, rc), -7, dtype=torch.int32, device="cuda"))
        for g in range(2):
            pols[g].act_rollout(eng, g, eps=eps, seed=seed + g, step=t)
        act = torch.empty((E, 2, rc), dtype=torch.int32, device="cuda")
        eng.rollout_copy("actions", act)
        eng.sync()
        actn = act.cpu().numpy()
        for e, (env, h, _) in enumerate(oracles):
            for g in range(2):
                view, feat = env.get_observation(h[g])
                n = len(view)
                want, tag, _ = rr.rule_actions(view, feat, v2a, base, NA, move, eps, seed + g, t, g,
                                               rows=e * rc + np.arange(n))
                assert np.array_equal(actn[e, g, :n], want), (t, e, g)
                assert (actn[e, g, n:] == -7).all(), (t, e, g)
                tags += np.bincount(tag, minlength=5)
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
    eng.rollout_check()
    print("E %d: tags %s, %d restarts" % (E, dict(zip(rr.TAG_NAMES, tags.tolist())), restarts))
    assert restarts >= E * (steps // max_steps)
    assert tags[rr.TAG_A] and tags[rr.TAG_B] and tags[rr.TAG_C_MINIMAP] and tags[rr.TAG_RANDOM]


# ------------------------------------------------------------------------------------------------- 3: RulePolicy
def test_rule_policy_on_the_host_loop():
    """RulePolicy.act(state=...) on an oracle observation is the restatement with (policy.seed, the call count, the
    policy's group); prob and eps are not read."""
    import torch
    from mfrl_amd.algo import spawn_ai
    torch.manual_seed(3)
    env, h, v2a, base, move = _battle_tables()
    left, right = bd.block_positions(64, 128)
    orc, oh = common.battle_env(common.ORACLE_LIB, 64)
    orc.reset()
    orc.add_agents(oh[0], method="custom", pos=left)
    orc.add_agents(oh[1], method="custom", pos=right)
    for g in range(2):
        m = spawn_ai("rush", None, env, h[g], "rush-%d" % g, 100)
        m.eps = 0.3
        view, feat = orc.get_observation(oh[g])
        for call in (1, 2):
            got = m.act(state=[view, feat], prob=np.zeros((len(view), NA)), eps=1.0)
            want, tag, _ = rr.rule_actions(view, feat, v2a, base, NA, move, 0.3, m.seed, call, g)
            assert got.dtype == np.int32 and np.array_equal(got, want), (g, call)
            assert 0 < (tag == rr.TAG_RANDOM).sum() < len(tag)
        assert m._draws == 2
    torch.manual_seed(3)
    assert spawn_ai("rush", None, env, h[1], "rush-1", 100).seed == m.seed
    assert spawn_ai("rush", None, env, h[1], "rush-x", 100).seed != m.seed


def test_rush_beats_random_in_battle_eval(tmp_path, capsys):
    from mfrl_amd import battle_eval
    win = battle_eval.main(["--algo", "rush", "--oppo", "random", "--envs", "8", "--map_size", "40", "--max_steps", "100",
                            "--n_round", "1", "--base_dir", str(tmp_path)])
    out = capsys.readouterr().out
    m = re.search(r"'kills': \[(\d+), (\d+)\]", out)
    assert m, out[-600:]
    kills = int(m.group(1)), int(m.group(2))
    print("rush vs random, 8 envs: kills %s, wins %s" % (kills, win))
    assert kills[0] > kills[1]
    # win counts a tie for both sides: main wins + ties = win["main"], opponent wins = 8 - win["main"]
    assert win["main"] + win["opponent"] >= 8 and win["main"] >= 8 - win["main"]
    assert re.search(r"WIN_RATE: \[rush\] \S+ / \[random\] \S+", out)
    assert "nothing to load" not in out and not os.path.exists(tmp_path / "data")


def test_battle_eval_learned_against_rush(tmp_path, capsys):
    from mfrl_amd import battle_eval
    battle_eval.main(["--algo", "mfq", "--oppo", "rush", "--untrained", "--envs", "4", "--max_steps", "10", "--n_round", "1",
                      "--rule_eps", "0.05", "--base_dir", str(tmp_path)])
    assert re.search(r"WIN_RATE: \[mfq\] \S+ / \[rush\] \S+", capsys.readouterr().out)


def test_train_battle_eval_every(tmp_path, capsys, monkeypatch):
    """--eval_every 1: two [EVAL] lines and two JSON lines; the weights after the run, and every file it saved, are
    bit for bit those of the same run without the flag, which prints no [EVAL] and writes no eval file."""
    import random
    import torch
    from mfrl_amd import train_battle
    real = train_battle.spawn_ai
    made = []

    def recording(*a, **kw):
        made.append(real(*a, **kw))
        return made[-1]

    monkeypatch.setattr(train_battle, "spawn_ai", recording)
    argv = ["--algo", "mfq", "--rollout", "--train_backend", "hip", "--envs", "4", "--n_round", "2", "--max_steps", "10"]
    runs = {}
    for name, extra in (("eval", ["--eval_every", "1", "--eval_envs", "4"]), ("plain", [])):
        torch.manual_seed(11)
        np.random.seed(11)
        random.seed(11)
        del made[:]
        train_battle.main(argv + extra + ["--base_dir", str(tmp_path / name)])
        torch.cuda.synchronize()
        weights = [[p.detach().cpu().numpy().copy() for p in m.eval_net.parameters()] for m in made[:2]]
        saved = {}
        for root, _, files in os.walk(tmp_path / name / "data" / "models"):
            for f in files:
                sd = torch.load(os.path.join(root, f), map_location="cpu", weights_only=True)
                saved[os.path.relpath(os.path.join(root, f), tmp_path / name)] = sd
        runs[name] = (capsys.readouterr().out, weights, saved, len(made))
    out, weights, saved, n_made = runs["eval"]
    assert n_made == 3 and runs["plain"][3] == 2                          # (the rule is made only with the flag)
    lines = [x for x in out.splitlines() if x.startswith("[EVAL]")]
    assert len(lines) == 2 and all(re.fullmatch(r"\[EVAL\] round \d vs rush: WIN_RATE \S+ / \S+, kills \d+ / \d+", x)
                                   for x in lines), lines
    recs = [json.loads(x) for x in open(tmp_path / "eval" / "data" / "eval_mfq.jsonl")]
    assert [r["round"] for r in recs] == [0, 1] and all(r["oppo"] == "rush" and r["envs"] == 4 for r in recs)
    assert "[EVAL]" not in runs["plain"][0] and not os.path.exists(tmp_path / "plain" / "data" / "eval_mfq.jsonl")
    for a, b in zip(weights, runs["plain"][1]):
        assert len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert sorted(saved) == sorted(runs["plain"][2])
    def same(x, y):
        if isinstance(x, dict):
            return isinstance(y, dict) and sorted(x) == sorted(y) and all(same(x[n], y[n]) for n in x)
        if isinstance(x, (list, tuple)):
            return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
        return torch.equal(x, y) if torch.is_tensor(x) else x == y

    print("files saved by the run: %s" % sorted(saved))                  # (the Runner saves when the main side wins)
    for k, sd in saved.items():
        assert same(sd, runs["plain"][2][k]), k


# ------------------------------------------------------------------------------------------------- 4: refusals
def test_rule_refusals_launch_nothing():
    """Null pointers, n < 0, eps NaN / < 0 / > 1 and a 17 x 17 view each give -1 with a message; the action buffer
    keeps its sentinel."""
    import torch
    from mfrl_amd import lib
    from mfrl_amd.policy import RuleHIP
    from magent.c_lib import EngineError
    _, _, v2a, base, move = _battle_tables()
    hip = RuleHIP(VS, FS, NA, base, v2a, move)
    view, feat = _rollout_obs()[0]
    n = 64
    act = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    L, P = lib(), ctypes.c_void_p
    L.mfx_rule_act.restype = ctypes.c_int
    v, f, a = P(view.data_ptr()), P(feat.data_ptr()), P(act.data_ptr())
    u = ctypes.c_uint32

    def call(handle, v, f, n, eps, a):
        L.mfx_rule_act.restype = ctypes.c_int
        return L.mfx_rule_act(handle, v, f, n, ctypes.c_float(eps), u(1), u(1), 0, a, P())

    for args in ((P(), v, f, n, 0.0, a), (hip.handle, P(), f, n, 0.0, a), (hip.handle, v, P(), n, 0.0, a),
                 (hip.handle, v, f, n, 0.0, P()), (hip.handle, v, f, -1, 0.0, a), (hip.handle, v, f, n, float("nan"), a),
                 (hip.handle, v, f, n, -0.01, a), (hip.handle, v, f, n, 1.01, a)):
        assert call(*args) == -1
        assert L.mfx_last_error()
    with pytest.raises(EngineError):
        RuleHIP((17, 17, 7), FS, NA, base, np.full((17, 17), -1, np.int32), move)
    with pytest.raises(ValueError):
        hip.act(view[:n], feat[:n], eps=2.0)
    torch.cuda.synchronize()
    assert bool((act == -7).all())
    # the rollout form: the same refusals, through the engine's own buffers
    from mfrl_amd.battle import BattleBatch
    left, right = _columns()
    eng = BattleBatch(64, 2, stream=torch.cuda.current_stream())
    eng.rollout_init([left, right], max_steps=5, eps=0.0, seed=1, stagger=False)
    eng.rollout_policy_observe()
    eng.rollout_write("actions", torch.full((2, 2, eng.rowcap), -7, dtype=torch.int32, device="cuda"))
    for bad in (float("nan"), -1.0, 1.5):
        with pytest.raises(EngineError):
            hip.act_rollout(eng, 0, eps=bad)
    got = torch.empty((2, 2, eng.rowcap), dtype=torch.int32, device="cuda")
    eng.rollout_copy("actions", got)
    eng.sync()
    assert bool((got == -7).all())
    assert call(hip.handle, v, f, n, 1.0, a) == 0                      # (and a good call still runs)
    torch.cuda.synchronize()
    assert bool(((act >= 0) & (act < NA)).all())
