"""The recorder of the device rollout loop (mfrl_amd.recorder, csrc/trace_kernels.hip) on the GPU.

* The kernels on synthetic device arrays against tests/trace_ref.py, all nine destination buffers compared byte for
  byte after every call, a sentinel block at each end included: watched envs unsorted with the first and the last env
  among them, rowcap 4 (below a wave), 68 (no multiple of 64) and 260 (more than a workgroup's lanes hold dwords; the
  alive row goes as dwords at 4, 68 and 260 and as 16-byte vectors at 16), 1 and 16 watched envs, a group of 0 and one of
  rowcap members, a step past cap_steps, a skipped and a doubled update.
* The scripted cases of tests/score_cases.py on the rollout loop (k_rollout; k_observe_items + k_rollout_big) with the
  recorder around every policy step: the trace is the C oracle lockstep's, and the replay on the product engine writes
  the frame files the reference build writes for the same actions.
* battle_rollout with an untrained MF-Q against an untrained MF-AC: the replay passes, final state included, and the
  scoreboard's outcome is the same with and without the recorder."""
import ctypes
import os

import numpy as np
import pytest

import common
import score_cases as sc
import trace_ref as tr

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p
SENT, PAD = 0xA5, 256


class Device:
    """The nine destination buffers on the device, PAD sentinel bytes before and after what the kernels are given."""

    def __init__(self, K, rowcap, cap):
        import torch
        from mfrl_amd.recorder import trace_lib
        self.K, self.rowcap, self.cap = K, rowcap, cap
        self.L = trace_lib()
        self.sizes = tr.sizes(K, rowcap, cap)
        got = (ctypes.c_size_t * 9)()
        assert self.L.mfx_trace_sizes(K, rowcap, ctypes.c_int64(cap), got) == 0
        assert list(got) == [self.sizes[k] for k in tr.NAMES]
        self.bufs = {k: torch.full((n + 2 * PAD,), SENT, dtype=torch.uint8, device="cuda")
                     for k, n in self.sizes.items()}
        self.st = P(torch.cuda.current_stream().cuda_stream)
        self.keep = None

    def structs(self, src, n_groups=2, rowcap=None):
        import torch
        from mfrl_amd.recorder import SRC_NAMES, _TraceDst, _TraceSrc
        self.keep = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in src.items()}
        s = _TraceSrc(*[self.keep[k].data_ptr() for k in SRC_NAMES], len(src["agent_steps"]), n_groups,
                      rowcap or self.rowcap)
        d = _TraceDst(*[self.bufs[k].data_ptr() + PAD for k in tr.NAMES], self.cap, self.K)
        return s, d

    def attach(self, src, envs, **kw):
        s, d = self.structs(src, **kw)
        return self.L.mfx_trace_attach(ctypes.byref(s), ctypes.byref(d), (ctypes.c_int32 * len(envs))(*envs), self.st)

    def update(self, src, step, **kw):
        s, d = self.structs(src, **kw)
        return self.L.mfx_trace_update(ctypes.byref(s), ctypes.byref(d), ctypes.c_int64(step), self.st)

    def check(self, rec, tag):
        import torch
        torch.cuda.synchronize()
        for k in tr.NAMES:
            got = self.bufs[k].cpu().numpy()
            pad = np.full(PAD, SENT, np.uint8)
            want = np.concatenate([pad, np.ascontiguousarray(rec[k]).view(np.uint8).reshape(-1), pad])
            assert got.shape == want.shape, (tag, k)
            bad = np.nonzero(got != want)[0]
            assert len(bad) == 0, (tag, k, "first differing bytes", bad[:8] - PAD, len(bad))


def _sources(E, rowcap, rng):
    cyc = [0, rowcap, 1, rowcap - 1, 3 % (rowcap + 1)]
    src = {"group_num": np.array([[cyc[(e + 2 * g) % 5] for g in range(2)] for e in range(E)], np.int32),
           "alive": rng.integers(0, 256, size=(E, 2, rowcap)).astype(np.uint8),
           "stats": np.zeros((E, 4), np.float64), "agent_steps": rng.integers(0, 1 << 40, size=E).astype(np.int64),
           "actions": rng.integers(0, 21, size=(E, 2, rowcap)).astype(np.int32),
           "ids": rng.integers(0, 1 << 20, size=(E, 2, rowcap)).astype(np.int32),
           "rewards": rng.standard_normal((E, 2, rowcap)).astype(np.float32),
           "rng": rng.integers(1, 2147483647, size=E).astype(np.uint32)}
    src["stats"][:, 0] = rng.integers(0, 5, size=E)
    src["stats"][:, 1:] = rng.random((E, 3))
    return src, cyc


def _advance(src, rng, e, new, end=0):
    """Env e steps once: every row is rewritten (stale entries behind the group sizes too: the record keeps them),
    agent_steps moves by the sizes the step ran with, then the sizes become `new`."""
    E, _, rowcap = src["alive"].shape
    src["alive"][e] = rng.integers(0, 256, size=(2, rowcap))
    src["actions"][e] = rng.integers(0, 21, size=(2, rowcap))
    src["ids"][e] = rng.integers(0, 1 << 20, size=(2, rowcap))
    src["rewards"][e] = rng.standard_normal((2, rowcap))
    src["agent_steps"][e] += int(src["group_num"][e].sum())
    src["group_num"][e] = new
    src["stats"][e, 0] += end


def _script(E, envs, rowcap, seed):
    """cap_steps 3 and five updates: step 1 is skipped for one watched env (it steps twice), step 2 comes without a
    step of another (a doubled update), steps 3 and 4 are past the cap.  Returns the record and the error words."""
    rng = np.random.default_rng(seed)
    src, cyc = _sources(E, rowcap, rng)
    K, cap = len(envs), 3
    dev, rec = Device(K, rowcap, cap), tr.new_record(K, rowcap, cap, fill=SENT)
    assert dev.attach(src, envs) == 0, dev.L.mfx_last_error().decode()
    tr.attach(rec, src, envs)
    dev.check(rec, "attach")
    words = []
    for t in range(5):
        for e in range(E):
            new = [cyc[(t + 1 + e + 2 * g) % 5] for g in range(2)]
            if t == 2 and e == envs[0]:
                continue                                 # no step of this env: its update is a doubled one
            if t == 1 and e == envs[-1]:
                _advance(src, rng, e, new)               # stepped twice for one update
            _advance(src, rng, e, new, end=int((t + e) % 2 == 0))
        assert dev.update(src, t) == 0, dev.L.mfx_last_error().decode()
        tr.update(rec, src, t)
        dev.check(rec, ("update", t))
        words.append(int(rec["state"][1]))
    return rec, words


@pytest.mark.parametrize("rowcap", [4, 16, 68, 260])
@pytest.mark.parametrize("E,envs", [(5, [4, 0, 2]), (5, [3]), (20, [19, 3, 0, 7, 1, 12, 5, 18, 2, 9, 4, 16, 6, 11, 8, 10])])
def test_kernels_equal_the_restatement(rowcap, E, envs):
    rec, words = _script(E, envs, rowcap, seed=rowcap + E)
    K = len(envs)
    # the script's own conditions, on the restatement alone
    assert words[0] == 0 and rec["head"][0, :, tr.VALID].all()
    assert words[1] == tr.ERR_STEP and rec["head"][1, K - 1, tr.VALID] == 0
    assert rec["head"][2, 0, tr.VALID] == 0 and (K == 1 or rec["head"][2, 1:K - 1, tr.VALID].all())
    assert words[3] == words[4] == tr.ERR_STEP | tr.FULL and rec["state"][0] == 3
    sizes = set(rec["head"][:, :, 1:3].reshape(-1).tolist())
    assert ({0, rowcap} <= sizes) if K > 1 else (sizes & {0, rowcap})
    assert (rec["head"][:, :, tr.EP_AFTER] - rec["head"][:, :, tr.EP_BEFORE] == 1).any()


def test_bad_arguments_are_refused():
    import torch
    rng = np.random.default_rng(1)
    src, _ = _sources(4, 8, rng)
    dev = Device(2, 8, 2)
    for envs, msg in (([0, 4], "outside"), ([-1, 0], "outside"), ([2, 2], "twice")):
        assert dev.attach(src, envs) == -1
        assert msg in dev.L.mfx_last_error().decode()
    three = {k: (np.concatenate([v, v[:, :1]], axis=1) if v.ndim > 1 and v.shape[1] == 2 else v) for k, v in src.items()}
    assert dev.attach(three, [0, 1], n_groups=3) == -1 and "two groups only" in dev.L.mfx_last_error().decode()
    assert dev.update(src, 0, rowcap=6) == -1 and "multiple of 4" in dev.L.mfx_last_error().decode()
    got = (ctypes.c_size_t * 9)()
    assert dev.L.mfx_trace_sizes(17, 8, ctypes.c_int64(2), got) == -1
    torch.cuda.synchronize()
    for k in tr.NAMES:                                   # nothing was launched or copied
        assert bool((dev.bufs[k] == SENT).all()), k


class _Arrays:
    """What RolloutRecorder needs of an engine, over synthetic device arrays."""
    handles = (0, 1)

    def __init__(self, src):
        import torch
        self.n_envs, _, self.rowcap = src["alive"].shape
        self.src = src
        self.dev = {k: torch.from_numpy(v).cuda() for k, v in src.items()}

    def push(self):
        import torch
        for k, v in self.src.items():
            self.dev[k].copy_(torch.from_numpy(v))

    def stream_handle(self):
        import torch
        return torch.cuda.current_stream().cuda_stream

    def torch_stream(self):
        import torch
        return torch.cuda.current_stream()


def _recorder(eng, envs, cap):
    from mfrl_amd.recorder import RolloutRecorder

    class Synthetic(RolloutRecorder):
        def _buffer(self, name):
            return self.eng.dev[name].data_ptr()

    return Synthetic(eng, envs, cap)


@pytest.mark.parametrize("fault,bit", [("skipped", "not recorded"), ("doubled", "not recorded"), ("full", "full")])
def test_finish_raises_on_the_error_word(fault, bit):
    from mfrl_amd.recorder import TraceError
    rng = np.random.default_rng(5)
    src, _ = _sources(5, 12, rng)
    eng = _Arrays(src)
    rec = _recorder(eng, [4, 0, 2], 3)
    rec.attach(40, 12, [np.zeros((1, 2), np.int32)] * 2)
    for t in range(4 if fault == "full" else 3):
        for e in range(5):
            if not (fault == "doubled" and t == 1 and e == 0):
                _advance(src, rng, e, [3, 4])
            if fault == "skipped" and t == 1 and e == 2:
                _advance(src, rng, e, [3, 4])
        eng.push()
        rec.update()
    with pytest.raises(TraceError, match=bit):
        rec.finish(final=False)


def test_finish_returns_the_recorded_rows():
    rng = np.random.default_rng(6)
    src, _ = _sources(5, 12, rng)
    eng = _Arrays(src)
    rec = _recorder(eng, [4, 0, 2], 3)
    want = tr.new_record(3, 12, 3)
    for rnd in range(2):                                 # the buffers are reused from round to round
        rec.attach(40, 12, [np.zeros((1, 2), np.int32)] * 2)
        bufs = [b.data_ptr() for b in rec._bufs]
        tr.attach(want, src, [4, 0, 2])
        for t in range(2 + rnd):
            for e in range(5):
                _advance(src, rng, e, [int(rng.integers(0, 13)), 4], end=int(e == t))
            eng.push()
            rec.update()
            tr.update(want, src, t)
        trace = rec.finish(final=False)
        assert trace["steps"] == 2 + rnd and trace["valid"].all() and list(trace["envs"]) == [4, 0, 2]
        assert trace["n"].tobytes() == want["head"][:2 + rnd, :, 1:3].astype(np.int32).tobytes()
        assert trace["ep_after"].tobytes() == np.ascontiguousarray(want["head"][:2 + rnd, :, tr.EP_AFTER]).tobytes()
        for name, _ in tr.ROWS:
            assert trace[name].tobytes() == want[name][:2 + rnd].tobytes(), name
    assert bufs == [b.data_ptr() for b in rec._bufs]


# ------------------------------------------------------------------------------------------------- the scripted cases
_CACHE = {}


def _run(name):
    if name in _CACHE:
        return _CACHE[name]
    import torch
    from mfrl_amd.battle import BattleBatch
    from mfrl_amd.recorder import RolloutRecorder
    plan, run = sc.PLANS[name], sc.oracle_run(name)
    old = os.environ.get("MFX_SMALL_E")
    if plan["small_e"] is not None:
        os.environ["MFX_SMALL_E"] = plan["small_e"]
    try:
        eng = BattleBatch(plan["map_size"], plan["envs"], stream=torch.cuda.current_stream())
        eng.rollout_init(run["placement"], max_steps=sc.MAX_STEPS, eps=0.2, seed=3, stagger=False)
    finally:
        if plan["small_e"] is not None:
            if old is None:
                del os.environ["MFX_SMALL_E"]
            else:
                os.environ["MFX_SMALL_E"] = old
    assert eng.rollout_policy_path() == plan["path"]
    assert eng.rowcap == run["rowcap"]
    watch = list(range(plan["envs"]))[::-1]
    rec, keep = RolloutRecorder(eng, watch, sc.STEPS), []
    eng.rollout_policy_observe()
    rec.attach(plan["map_size"], sc.MAX_STEPS, run["placement"])
    for t in range(sc.STEPS):
        keep.append(torch.from_numpy(run["actions"][t]).cuda())
        eng.rollout_write("actions", keep[-1])
        eng.rollout_policy_step()
        rec.update()
    trace = rec.finish()
    eng.rollout_check()
    _CACHE[name] = {"trace": trace, "want": tr.lockstep(name, watch)["trace"], "run": run}
    return _CACHE[name]


@pytest.mark.parametrize("name", list(sc.PLANS))
def test_trace_equals_the_oracle_lockstep(name):
    from mfrl_amd.recorder import replay
    res = _run(name)
    got, want = res["trace"], res["want"]
    assert got["steps"] == want["steps"] == sc.STEPS and got["valid"].all()
    assert list(got["envs"]) == list(want["envs"]) and got["rowcap"] == want["rowcap"]
    assert got["n"].tobytes() == want["n"].tobytes()
    assert np.array_equal(got["ep_after"] - got["ep_before"], want["ep_after"] - want["ep_before"])
    assert np.array_equal(got["agent_steps"] - got["agent_steps"][0], want["agent_steps"] - want["agent_steps"][0])
    assert got["actions"].tobytes() == want["actions"].tobytes()          # whole rows, behind the group sizes too
    for t in range(sc.STEPS):
        for k in range(len(got["envs"])):
            for g in range(2):
                n = int(want["n"][t, k, g])
                assert got["ids"][t, k, g, :n].tobytes() == want["ids"][t, k, g, :n].tobytes(), (t, k, g)
                assert np.array_equal(got["alive"][t, k, g, :n] != 0, want["alive"][t, k, g, :n] != 0), (t, k, g)
                assert got["rewards"][t, k, g, :n].tobytes() == want["rewards"][t, k, g, :n].tobytes(), (t, k, g)
    # the replay on the product engine passes its own comparison, the state the round ended in included
    assert got["final"] is not None
    for k in range(len(got["envs"])):
        out = replay(got, k)
        assert out["steps"] == sc.STEPS and out["episodes"] == len(res["run"]["episodes"][int(got["envs"][k])])


@pytest.mark.parametrize("name", list(sc.PLANS))
def test_replay_writes_the_reference_frames(name, tmp_path):
    if not os.path.exists(common.REF_LIB):
        pytest.skip("reference build absent")
    from mfrl_amd.recorder import replay
    from test_trace_cpu import direct_frames, frame_conditions, same_files
    trace = _run(name)["trace"]
    events = died = False
    for k, e in enumerate(trace["envs"]):
        e = int(e)
        out = replay(trace, k, render_dir=str(tmp_path / "replay"))
        direct_frames(common.REF_LIB, name, e, tmp_path / "ref" / ("env_%d" % e))
        files = same_files(out["dir"], str(tmp_path / "ref" / ("env_%d" % e)))
        assert len([f for f in files if f.startswith("video_")]) >= 2
        ev, dd = frame_conditions(out["dir"], trace, k)
        events |= ev
        died |= dd
    if name == "packed":
        assert events and died


def test_a_later_round_replays_from_its_shuffle_state():
    """Two rounds of the packed case on one engine: the second starts with the shuffle engines where the first left
    them (a reset does not re-seed them), and its replay on a new one-env engine still passes."""
    import torch
    from mfrl_amd.battle import BattleBatch
    from mfrl_amd.recorder import RolloutRecorder, TraceMismatch, replay
    plan, run = sc.PLANS["packed"], sc.oracle_run("packed")
    eng = BattleBatch(plan["map_size"], plan["envs"], stream=torch.cuda.current_stream())
    rec, keep, traces = RolloutRecorder(eng, [0, 1], sc.STEPS), [], []
    for rnd in range(2):
        eng.reset()
        eng.rollout_init(run["placement"], max_steps=sc.MAX_STEPS, eps=0.0, seed=rnd, stagger=False)
        eng.rollout_policy_observe()
        rec.attach(plan["map_size"], sc.MAX_STEPS, run["placement"])
        for t in range(sc.STEPS):
            keep.append(torch.from_numpy(run["actions"][t]).cuda())
            eng.rollout_write("actions", keep[-1])
            eng.rollout_policy_step()
            rec.update()
        traces.append(rec.finish())
        eng.rollout_check()
    first, second = traces
    assert list(first["seed"]) == [1, 1] and all(int(s) not in (0, 1) for s in second["seed"])
    assert first["n"].tobytes() == tr.lockstep("packed", [0, 1])["trace"]["n"].tobytes()
    for k in range(2):
        assert replay(second, k)["steps"] == sc.STEPS
    # the same rows from a new engine's state are another game: the shuffle state is what makes the replay right
    differs = 0
    for k in range(2):
        bad = dict(second, seed=np.ones(2, np.uint32))
        try:
            replay(bad, k)
        except TraceMismatch:
            differs += 1
    assert differs >= 1


# ------------------------------------------------------------------------------------------------- with networks
def _models(map_size, max_steps, seed=3):
    import torch
    import magent
    from mfrl_amd.algo import spawn_ai
    env = magent.GridWorld("battle", map_size=map_size)
    h = env.get_handles()
    torch.manual_seed(seed)
    return [spawn_ai("mfq", None, env, h[0], "mfq-me", max_steps, memory_size=1024),
            spawn_ai("mfac", None, env, h[1], "mfac-opponent", max_steps)]


def test_battle_rollout_with_the_recorder():
    import torch
    from mfrl_amd.algo.play import battle_rollout
    from mfrl_amd.battle import BattleBatch
    from mfrl_amd.recorder import RolloutRecorder, replay
    map_size, E, max_steps = 40, 2, 30
    outs = []
    for with_rec in (False, True):
        models = _models(map_size, max_steps)
        eng = BattleBatch(map_size, E, stream=torch.cuda.current_stream())
        rec = RolloutRecorder(eng, [1, 0], max_steps) if with_rec else None
        outs.append(battle_rollout(eng, 0, map_size, max_steps, models, left_id=0, recorder=rec)[4])
    plain, watched = outs
    assert "trace" not in plain
    assert plain["totals"].tobytes() == watched["totals"].tobytes()
    assert plain["log"].tobytes() == watched["log"].tobytes()
    for key in ("episodes", "main_wins", "oppo_wins", "ties", "kills", "steps", "agent_steps", "steps_run", "first"):
        assert plain[key] == watched[key], key
    trace = watched["trace"]
    assert trace["steps"] == watched["steps_run"] == max_steps and trace["valid"].all()
    assert list(trace["envs"]) == [1, 0] and trace["final"] is not None
    for k in range(2):
        out = replay(trace, k)
        assert out["steps"] == max_steps and out["episodes"] == 1
        assert int(trace["agent_steps"][-1, k] - trace["agent_steps"][0, k]) == int(trace["n"][1:, k].sum())
    assert int(trace["n"][:, :, :].sum()) == watched["agent_steps"]


def _videos(d):
    return sorted(f for f in os.listdir(d) if f.startswith("video_"))


def test_training_loops_take_a_recorder(tmp_path, capsys):
    """play_rollout and play_rollout_episodes with recorder=: the round's trace is on the recorder and replays, every
    episode of the round in a file of its own; without one they return what they returned."""
    import torch
    from mfrl_amd.algo.play import play_rollout, play_rollout_episodes
    from mfrl_amd.battle import BattleBatch
    from mfrl_amd.recorder import RolloutRecorder, replay
    map_size, E, max_steps = 40, 2, 12
    for loop, order in ((play_rollout, (0, 1)), (play_rollout_episodes, (1, 0))):
        res = []
        for with_rec in (False, True):
            models = _models(map_size, max_steps)
            models = [models[order[0]], models[order[1]]]
            eng = BattleBatch(map_size, E, stream=torch.cuda.current_stream())
            rec = RolloutRecorder(eng, [1], max_steps) if with_rec else None
            res.append(loop(eng, 0, map_size, max_steps, models, left_id=1, **({"recorder": rec} if with_rec else {})))
        assert res[0] == res[1], loop.__name__
        trace = rec.trace
        assert trace["steps"] == max_steps and list(trace["envs"]) == [1] and trace["final"] is not None
        out = replay(trace, 0, render_dir=str(tmp_path / loop.__name__))
        assert out["steps"] == max_steps and out["episodes"] == 1
        assert "config.json" in os.listdir(out["dir"]) and len(_videos(out["dir"])) == 1
    capsys.readouterr()


def test_train_battle_watch(tmp_path, capsys):
    """train_battle --rollout --render --watch: the rounds the Runner marks for rendering (it passes
    (round + 1) % save_every, the reference's expression) leave the watched env's frames, the others nothing."""
    from mfrl_amd import train_battle
    train_battle.main(["--algo", "mfq", "--envs", "2", "--rollout", "--render", "--watch", "1", "--n_round", "2",
                       "--save_every", "2", "--map_size", "40", "--max_steps", "12", "--base_dir", str(tmp_path)])
    out = capsys.readouterr().out
    assert out.count("[WATCH] round 0 env 1: 12 steps, 1 episodes") == 1 and "[WATCH] round 1" not in out
    render = tmp_path / "examples/battle_model" / "build/render"
    assert sorted(os.listdir(render)) == ["round_0"] and os.listdir(render / "round_0") == ["env_1"]
    d = render / "round_0" / "env_1"
    assert "config.json" in os.listdir(d) and len(_videos(d)) == 1


def test_battle_eval_watch(tmp_path, capsys):
    from mfrl_amd import battle_eval
    argv = ["--algo", "mfq", "--oppo", "mfac", "--untrained", "--envs", "3", "--n_round", "2", "--map_size", "40",
            "--max_steps", "12", "--seed", "4"]
    plain = battle_eval.main(argv + ["--base_dir", str(tmp_path / "plain")])
    watched = battle_eval.main(argv + ["--base_dir", str(tmp_path / "watched"), "--watch", "2", "0"])
    out = capsys.readouterr().out
    assert plain == watched                                      # the recorder changes no game
    assert out.count("[WATCH] round 0 env") == 2 and "[WATCH] round 1" not in out
    render = tmp_path / "watched" / "examples/battle_model" / "build/render"
    assert sorted(os.listdir(render)) == ["round_0"] and sorted(os.listdir(render / "round_0")) == ["env_0", "env_2"]
    for e in (0, 2):
        d = render / "round_0" / ("env_%d" % e)
        assert "config.json" in os.listdir(d) and len(_videos(d)) == 1       # the first episode only
    assert not os.path.exists(tmp_path / "plain" / "examples/battle_model" / "build/render" / "round_0")
