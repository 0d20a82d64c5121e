"""The recorder's contract off the GPU: tests/trace_ref.py's guards, cap and verbatim rows behave as
include/magent_amd.h part 8 states; a trace built by lockstep on the C oracle over the scripted cases of
tests/score_cases.py replays clean (mfrl_amd.recorder.replay), a changed action or a flipped reward bit is caught at its
step, and on the reference build the replay writes the very frame files a direct run writes; the --watch refusals."""
import os

import numpy as np
import pytest

import common
import score_cases as sc
import trace_ref as tr


# ------------------------------------------------------------------------------------------------- guards and cap
def _src(E=3, rowcap=8, n=(5, 6), seed=0):
    rng = np.random.default_rng(seed)
    return {"group_num": np.tile(np.array(n, np.int32), (E, 1)),
            "alive": rng.integers(0, 3, size=(E, 2, rowcap)).astype(np.uint8),
            "stats": np.zeros((E, 4), np.float64), "agent_steps": rng.integers(0, 1 << 40, size=E).astype(np.int64),
            "actions": rng.integers(0, 21, size=(E, 2, rowcap)).astype(np.int32),
            "ids": rng.integers(0, 99, size=(E, 2, rowcap)).astype(np.int32),
            "rewards": rng.random((E, 2, rowcap)).astype(np.float32),
            "rng": rng.integers(1, 2147483647, size=E).astype(np.uint32)}


def _step(src, e, new=None, end=0):
    src["agent_steps"][e] += int(src["group_num"][e].sum())
    if new is not None:
        src["group_num"][e] = new
    src["stats"][e, 0] += end


def test_ref_records_verbatim_rows():
    src = _src()
    rec = tr.new_record(2, 8, 3, fill=0xA5)
    tr.attach(rec, src, [2, 0])
    assert list(rec["state"]) == [0, 0] and list(rec["envs"]) == [2, 0]
    assert list(rec["seeds"]) == [src["rng"][2], src["rng"][0]]
    assert list(rec["carry"][0, 0]) == [5, 6, 0, int(src["agent_steps"][2])] and not rec["carry"][1].any()
    before = {k: src[k].copy() for k in ("actions", "ids", "rewards", "alive")}
    for e in range(3):
        _step(src, e, new=(4, 6), end=int(e == 2))
    tr.update(rec, src, 0)
    assert list(rec["state"]) == [1, 0]
    # whole rows, the stale entries at and past the group sizes included
    for k, e in enumerate([2, 0]):
        for name in before:
            assert rec[name][0, k].tobytes() == before[name][e].tobytes(), name
        assert list(rec["head"][0, k]) == [1, 5, 6, 0, int(e == 2), int(src["agent_steps"][e])]
        assert list(rec["carry"][1, k]) == [4, 6, int(e == 2), int(src["agent_steps"][e])]
    # nothing behind step 0 was touched
    assert (rec["head"][1:].view(np.uint8) == 0xA5).all() and (rec["alive"][1:] == 0xA5).all()


def test_ref_guards():
    src = _src()
    rec = tr.new_record(2, 8, 6)
    tr.attach(rec, src, [2, 0])
    _step(src, 0)
    _step(src, 0)                                   # env 0 stepped twice for one update
    _step(src, 2)
    tr.update(rec, src, 0)
    assert rec["state"][1] == tr.ERR_STEP
    assert rec["head"][0, 1, tr.VALID] == 0 and rec["head"][0, 0, tr.VALID] == 1
    # the carry was taken afresh: the next step of env 0 is valid again, the word stays
    _step(src, 0)
    _step(src, 2)
    tr.update(rec, src, 1)
    assert rec["head"][1, 1, tr.VALID] == 1 and rec["state"][1] == tr.ERR_STEP
    # an update without a step is a step recorded twice
    tr.update(rec, src, 2)
    assert not rec["head"][2, :, tr.VALID].any()
    # an episode count that jumps by two
    rec["state"][1] = 0
    _step(src, 0, end=2)
    _step(src, 2, end=1)
    tr.update(rec, src, 3)
    assert rec["state"][1] == tr.ERR_EPISODE and list(rec["head"][3, :, tr.VALID]) == [1, 0]
    # a group size outside [0, rowcap]: flagged, recorded as it is, and no address depends on it
    rec["state"][1] = 0
    _step(src, 0, new=(9, 1))
    _step(src, 2)
    tr.update(rec, src, 4)
    assert rec["state"][1] == tr.ERR_COUNT and rec["head"][4, 1, tr.VALID] == 0
    _step(src, 0, new=(8, 0))
    _step(src, 2)
    rec["state"][1] = 0
    tr.update(rec, src, 5)
    assert rec["state"][1] == tr.ERR_COUNT and list(rec["head"][5, 1, 1:3]) == [9, 1]
    assert list(rec["state"]) == [6, tr.ERR_COUNT]


def test_ref_full_writes_nothing():
    src = _src()
    rec = tr.new_record(1, 8, 3, fill=0x5A)
    tr.attach(rec, src, [1])
    for t in range(3):
        _step(src, 1)
        tr.update(rec, src, t)
    keep = {k: rec[k].copy() for k in tr.NAMES}
    _step(src, 1)
    tr.update(rec, src, 3)
    assert rec["state"][1] == tr.FULL and rec["state"][0] == 3
    rec["state"][1] = 0
    for k in tr.NAMES:
        assert rec[k].tobytes() == keep[k].tobytes(), k


def test_ref_bad_env_index():
    src = _src()
    rec = tr.new_record(2, 8, 2, fill=0x11)
    tr.attach(rec, src, [1, 3])
    assert rec["state"][1] == tr.ERR_ENV and not rec["carry"][:, 1].any()
    _step(src, 1)
    tr.update(rec, src, 0)
    assert rec["head"][0, 0, tr.VALID] == 1 and not rec["head"][0, 1].any()
    assert (rec["actions"][0, 1].view(np.uint8) == 0x11).all()


def test_recorder_refuses_a_bad_watch_list():
    from mfrl_amd.recorder import check_watch
    assert check_watch([4, 0, 2], 5) == [4, 0, 2]
    for envs, msg in (([], "1 to 16"), (list(range(17)), "1 to 16"), ([5], "outside"), ([-1], "outside"),
                      ([1, 2, 1], "twice")):
        with pytest.raises(ValueError, match=msg):
            check_watch(envs, 5 if len(envs) < 17 else 40)


# ------------------------------------------------------------------------------------------------- the replay
def _oracle():
    import magent
    return magent.load_library(common.ORACLE_LIB)


@pytest.mark.parametrize("name", list(sc.PLANS))
def test_lockstep_trace_replays_on_the_oracle(name):
    from mfrl_amd.recorder import replay
    res = tr.lockstep(name)
    trace, run = res["trace"], res["run"]
    E = sc.PLANS[name]["envs"]
    assert trace["steps"] == sc.STEPS and trace["valid"].all() and list(trace["envs"]) == list(range(E))[::-1]
    for k, e in enumerate(trace["envs"]):
        # the trace is the oracle run's: group sizes and alive flags before clear_dead, the scripted action rows whole
        for t, row in enumerate(run["steps"]):
            assert list(trace["n"][t, k]) == row[e]["n"]
            for g in range(2):
                n = row[e]["n"][g]
                assert np.array_equal(trace["alive"][t, k, g, :n].astype(bool), row[e]["alive"][g])
            assert trace["actions"][t, k].tobytes() == run["actions"][t][e].tobytes()
        ends = trace["ep_after"][:, k] - trace["ep_before"][:, k]
        assert int(ends.sum()) == len(run["episodes"][e]) >= 2
        out = replay(trace, k, lib=_oracle())
        assert out == {"steps": sc.STEPS, "episodes": len(run["episodes"][e]), "dir": None}
        one = replay(trace, k, lib=_oracle(), episodes=1)
        assert one["episodes"] == 1 and one["steps"] == run["episodes"][e][0]["len"]
    assert (trace["n"] < trace["rowcap"]).any()          # stale entries behind a group's size exist and were kept


def test_replay_starts_from_the_recorded_shuffle_state():
    """A reset does not re-seed an env's shuffle engine, so a round's attack order depends on the state the engine came
    with; the trace carries it and the replay starts from it."""
    from mfrl_amd.recorder import TraceMismatch, replay
    seeds = [20261020, 977]
    res = tr.lockstep("packed", seeds=seeds)
    trace = res["trace"]
    assert list(trace["seed"]) == seeds[::-1]
    plain = tr.lockstep("packed")["trace"]
    assert list(plain["seed"]) == [1, 1]
    # the case's own condition: the state matters to this plan (the same actions, another game)
    assert any(trace[f].tobytes() != plain[f].tobytes() for f in ("rewards", "alive", "n"))
    for k in range(2):
        assert replay(trace, k, lib=_oracle())["steps"] == sc.STEPS
    differs = 0
    for k in range(2):
        bad = _copy(trace)
        bad["seed"][k] = 1
        try:
            replay(bad, k, lib=_oracle())
        except TraceMismatch:
            differs += 1
    assert differs >= 1


def _copy(trace):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in trace.items()}


def test_replay_catches_a_changed_action_and_a_flipped_reward_bit():
    from mfrl_amd.recorder import TraceMismatch, replay
    trace = tr.lockstep("packed")["trace"]
    k = 0
    # an attack that landed (its target died in that step, so the step's rewards and alive flags depend on it) ...
    hit = [(t, g, i) for t in range(3, sc.STEPS) for g in range(2) for i in range(int(trace["n"][t, k, g]))
           if trace["actions"][t, k, g, i] >= 13 and trace["rewards"][t, k, g, i] > 1.0]
    assert hit, "the packed plan has kills"
    t, g, i = hit[0]
    bad = _copy(trace)
    bad["actions"][t, k, g, i] = 6                       # ... replaced by another id
    with pytest.raises(TraceMismatch) as ex:
        replay(bad, k, lib=_oracle())
    assert ex.value.step == t and ex.value.env == int(trace["envs"][k])
    # one reward bit
    t2, g2 = 7, 1
    bad = _copy(trace)
    bad["rewards"][t2, k, g2, 0] = (bad["rewards"][t2, k, g2, :1].view(np.uint32) ^ np.uint32(1)).view(np.float32)[0]
    with pytest.raises(TraceMismatch) as ex:
        replay(bad, k, lib=_oracle())
    assert (ex.value.step, ex.value.group, ex.value.field) == (t2, g2, "rewards")
    # a stale entry behind the group's size is not the game's: changing it changes nothing
    t3 = next(t for t in range(sc.STEPS) if trace["n"][t, k, 0] < trace["rowcap"])
    ok = _copy(trace)
    ok["rewards"][t3, k, 0, -1] += 1.0
    ok["actions"][t3, k, 0, -1] ^= 1
    assert replay(ok, k, lib=_oracle())["steps"] == sc.STEPS
    # a record that failed a guard on the device is refused
    bad = _copy(trace)
    bad["valid"][4, k] = False
    with pytest.raises(TraceMismatch) as ex:
        replay(bad, k, lib=_oracle())
    assert (ex.value.step, ex.value.field) == (4, "valid")


# ------------------------------------------------------------------------------------------------- frames
def direct_frames(lib_path, name, e, out_dir):
    """The frame files of env e of the scripted case, written by a direct run on the build at lib_path: the calls the
    replay makes, spelled out here with the case's own actions."""
    plan, run = sc.PLANS[name], sc.oracle_run(name)
    env, h = common.battle_env(lib_path, plan["map_size"])
    env.set_render_dir(str(out_dir))

    def place():
        env.reset()
        for g, pos in enumerate(run["placement"]):
            env.add_agents(h[g], method="custom", pos=pos)

    place()
    env.render()
    ep_len = 0
    for t in range(sc.STEPS):
        for g in range(2):
            env.set_action(h[g], np.ascontiguousarray(run["actions"][t][e, g, :env.get_num(h[g])]))
        done = env.step()
        env.render()
        env.clear_dead()
        ep_len += 1
        if done or ep_len >= sc.MAX_STEPS:
            ep_len = 0
            place()
            if t + 1 < sc.STEPS:
                env.render()
    del env


def frames(path):
    """[(n_agents, n_events, {id: hp%})] of a video_<n>.txt."""
    out, lines = [], open(path).read().split("\n")
    i = 0
    while i < len(lines):
        p = lines[i].split()
        if p and p[0] == "W":
            i += 1 + int(p[1])
        elif p and p[0] == "F":
            na, ne = int(p[1]), int(p[2])
            agents = {int(x.split()[0]): int(x.split()[1]) for x in lines[i + 1:i + 1 + na]}
            out.append((na, ne, agents))
            i += 1 + na + ne
        else:
            i += 1
    return out


def same_files(a, b):
    files = sorted(os.listdir(a))
    assert files == sorted(os.listdir(b)) and "config.json" in files
    for f in files:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f
    return files


def frame_conditions(d, trace, k):
    """The case's own conditions on the frame files of watched env k in directory d."""
    videos = sorted((f for f in os.listdir(d) if f.startswith("video_")), key=lambda f: int(f[6:-4]))
    assert len(videos) >= 2
    fr = [f for v in videos for f in frames(os.path.join(d, v))]
    ends = trace["ep_after"][:, k] - trace["ep_before"][:, k]
    assert len(fr) == trace["steps"] + 1 + int(ends[:-1].sum())      # one per step, one per placement
    events, died = any(ne > 0 for _, ne, _ in fr), False
    at = 1                                                           # frame of step t (the placement frames skipped)
    for t in range(trace["steps"]):
        for g in range(2):
            n = int(trace["n"][t, k, g])
            for i in np.nonzero(trace["alive"][t, k, g, :n] == 0)[0]:
                died |= fr[at][2].get(int(trace["ids"][t, k, g, i])) == 0
        at += 2 if ends[t] else 1
    return events, died


def test_replay_on_the_reference_writes_the_reference_frames(tmp_path):
    if not os.path.exists(common.REF_LIB):
        pytest.skip("reference build absent")
    import magent
    from mfrl_amd.recorder import replay
    trace = tr.lockstep("packed")["trace"]
    common.pin_ref_threads()
    events = died = False
    for k, e in enumerate(trace["envs"]):
        e = int(e)
        out = replay(trace, k, lib=magent.load_library(common.REF_LIB), render_dir=str(tmp_path / "replay"))
        assert out["dir"] == str(tmp_path / "replay" / ("env_%d" % e)) and out["steps"] == sc.STEPS
        direct_frames(common.REF_LIB, "packed", e, tmp_path / "direct" / ("env_%d" % e))
        same_files(out["dir"], str(tmp_path / "direct" / ("env_%d" % e)))
        ev, dd = frame_conditions(out["dir"], trace, k)
        events |= ev
        died |= dd
    assert events and died


# ------------------------------------------------------------------------------------------------- the CLI
EVAL = ["--algo", "mfq", "--oppo", "mfac", "--untrained"]
TRAIN = ["--algo", "mfq"]


@pytest.mark.parametrize("mod,argv,msg", [
    ("battle_eval", EVAL + ["--watch", "0"], "--watch"),
    ("battle_eval", EVAL + ["--envs", "4", "--watch", "4"], "--watch"),
    ("battle_eval", EVAL + ["--envs", "4", "--watch", "1", "3", "1"], "--watch"),
    ("battle_eval", EVAL + ["--envs", "64", "--watch"] + [str(i) for i in range(17)], "--watch"),
    ("battle_eval", EVAL + ["--envs", "4", "--watch", "1", "--watch_rounds", "0"], "--watch_rounds"),
    ("train_battle", TRAIN + ["--envs", "4", "--watch", "1"], "--watch"),
    ("train_battle", TRAIN + ["--watch", "0", "--rollout"], "--rollout"),
    ("train_battle", TRAIN + ["--envs", "4", "--rollout", "--watch", "4"], "--watch"),
    ("train_battle", TRAIN + ["--envs", "4", "--rollout", "--watch", "2", "2"], "--watch"),
    ("train_battle", TRAIN + ["--envs", "4", "--rollout", "--watch", "2"], "--render"),
    ("train_battle", TRAIN + ["--envs", "64", "--rollout", "--watch"] + [str(i) for i in range(17)], "--watch"),
])
def test_watch_refusals(mod, argv, msg, capsys):
    import importlib
    m = importlib.import_module("mfrl_amd." + mod)
    with pytest.raises(SystemExit) as ex:
        m.main(argv)
    assert ex.value.code == 2
    assert msg in capsys.readouterr().err


class _Parsed(Exception):
    pass


@pytest.mark.parametrize("mod,argv", [
    ("battle_eval", EVAL + ["--render"]),
    ("battle_eval", EVAL + ["--envs", "4", "--watch", "3", "0"]),
    ("train_battle", TRAIN + ["--render"]),
    ("train_battle", TRAIN + ["--render", "--envs", "64", "--rollout"]),
    ("train_battle", TRAIN + ["--render", "--envs", "64", "--rollout", "--watch", "63", "0"]),
])
def test_arguments_that_parse(mod, argv, monkeypatch):
    """--render without --watch is accepted as before, and a good --watch list is: main() gets as far as making the
    env (which this test stops)."""
    import importlib
    m = importlib.import_module("mfrl_amd." + mod)

    def stop(*a, **kw):
        raise _Parsed()

    monkeypatch.setattr(m.magent, "GridWorld", stop)
    with pytest.raises(_Parsed):
        m.main(argv)
