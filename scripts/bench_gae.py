"""Measurements of the GAE(lambda) mode of AC / MFAC (ActorCritic.advantage = "gae"), appended as JSON lines
to --out (profiles/gae_ab.jsonl is such a run).  One round of rows is collected on the device rollout loop (MF-AC, 64
envs of 40x40, 100 steps by default: about 409,600 rows); every measure then runs on those same rows, the arms
alternating, --runs times after one warm-up pass, and ends with a summary line per arm: median (min-max), and
"resolved": false against the first arm when the two ranges overlap.

  prepare  round preparation, tails known -> columns ready (device events on the engine's stream):
             returns    gather of the tail rows + value forward (k_acnet) + mfx_chain_returns
             gae        value forward over all rows + mfx_chain_gae
             gae_norm   gae + mfx_adv_normalize
  train    the whole train_rollout() call (wall clock around it, the device idle before and after), backend x mode:
             torch / hip  x  returns / gae / gae_norm
  parent   the default mode against the parent commit's package: child processes of this script (measure "child": one
           collected round, --runs train_rollout() calls, their median), alternating between this tree and --parent_pkg
           (a checkout of the parent commit with its library built: <parent_pkg>/python and <parent_pkg>/build/libmagent.so),
           per backend.

    python scripts/bench_gae.py --out profiles/gae_ab.jsonl prepare train
    python scripts/bench_gae.py --out profiles/gae_ab.jsonl --parent_pkg <dir> parent
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("BENCH_GAE_PKG") or os.path.join(REPO, "mean-field-multi-agent-reinforcement-learning_amd")
if os.environ.get("BENCH_GAE_PKG"):
    os.environ["MAGENT_LIB"] = os.path.join(PKG, "build", "libmagent.so")
sys.path.insert(0, os.path.join(PKG, "python"))


def emit(args, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def summarise(args, measure, unit, samples, extra):
    """One line per arm: median (min-max); resolved = its range does not overlap the first arm's."""
    names = list(samples)
    lo0, hi0 = min(samples[names[0]]), max(samples[names[0]])
    for name in names:
        x = samples[name]
        rec = dict(extra, measure=measure, summary=True, arm=name, runs=len(x), unit=unit,
                   median=statistics.median(x), min=min(x), max=max(x))
        if name != names[0]:
            rec["against"] = names[0]
            rec["resolved"] = bool(min(x) > hi0 or max(x) < lo0)
            rec["delta_of_medians"] = statistics.median(x) - statistics.median(samples[names[0]])
        emit(args, rec)


def collect(args):
    """-> (model, rows, n, snapshot of the reward column): one round collected into models[0]'s buffer."""
    import magent
    import torch
    from mfrl_amd.algo import spawn_ai
    from mfrl_amd.algo.play import block_positions
    from mfrl_amd.battle import BattleBatch
    env = magent.GridWorld("battle", map_size=args.map_size)
    h = env.get_handles()
    torch.manual_seed(3)
    models = [spawn_ai(args.algo, None, env, h[g], "%s-%d" % (args.algo, g), args.max_steps) for g in range(2)]
    eng = BattleBatch(args.map_size, args.envs, stream=torch.cuda.current_stream())
    me = models[0]
    col = me.rollout_collector(eng, 0)
    left, right = block_positions(args.map_size)
    eng.reset()
    eng.rollout_init([left, right], max_steps=args.max_steps, eps=0.0, seed=0, stagger=False)
    eng.rollout_policy_observe()
    for _ in range(args.max_steps):
        for g in range(2):
            models[g].act_rollout(eng, g)
        col.begin()
        eng.rollout_policy_step()
        col.end()
    n = col.finish()
    eng.rollout_check()
    rows = me.replay_buffer._rows
    return me, rows, n, rows.cols["rew"][:n].clone()


def shape(args, n):
    return {"algo": args.algo, "map_size": args.map_size, "envs": args.envs, "max_steps": args.max_steps, "rows": n}


def do_prepare(args):
    import torch
    from mfrl_amd import replay
    me, rows, n, snap = collect(args)
    c = rows.cols
    use_mf = "prob" in c
    hip = me._hip_net()
    tails = c["tail"][:n].nonzero().reshape(-1)
    value = torch.empty(n, dtype=torch.float32, device="cuda")
    adv = torch.empty(n, dtype=torch.float32, device="cuda")

    def returns(rew):
        _, keep, _ = hip.forward(c["obs"][tails], c["feat"][tails], c["prob"][tails] if use_mf else None,
                                 want_policy=False, want_value=True, want_act=False)
        replay.chain_returns(rew, c["prev"], tails, keep, me.gamma)

    def gae(rew, norm=False):
        _, v, _ = hip.forward(c["obs"][:n], c["feat"][:n], c["prob"][:n] if use_mf else None, want_policy=False,
                              want_value=True, want_act=False)
        value.copy_(v.reshape(-1))
        replay.chain_gae(rew, adv, c["prev"], tails, value, me.gamma, 0.95)
        if norm:
            replay.adv_normalize(adv)

    arms = {"returns": returns, "gae": gae, "gae_norm": lambda rew: gae(rew, True)}
    samples = {k: [] for k in arms}
    with torch.no_grad():
        for run in range(-1, args.runs):                 # run -1: warm-up, not reported
            for name, fn in arms.items():
                rew = snap.clone()                       # the walks work in place: a fresh copy, off the clock
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                a.record()
                fn(rew)
                b.record()
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                if run >= 0:
                    samples[name].append(a.elapsed_time(b))
                    emit(args, dict(shape(args, n), measure="prepare", arm=name, run=run, chains=len(tails),
                                    device_ms=a.elapsed_time(b), wall_ms=wall))
    summarise(args, "prepare", "device_ms", samples, dict(shape(args, n), chains=len(tails)))


def timed_train(me, rows, n, snap):
    import torch
    rows.cols["rew"][:n].copy_(snap)
    rows.n = n
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    me.train_rollout()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def quiet(fn, *a):
    """fn(*a) with the training print of train_rollout kept off the JSON stream."""
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a)


def do_train(args):
    me, rows, n, snap = collect(args)
    arms = [(b, m) for b in ("torch", "hip") for m in ("returns", "gae", "gae_norm")]
    samples = {"%s/%s" % a: [] for a in arms}
    for run in range(-1, args.runs):
        for backend, mode in arms:
            me.train_backend = backend
            me.adv_norm = False
            me.advantage = "returns" if mode == "returns" else "gae"
            me.adv_norm = mode == "gae_norm"
            ms = quiet(timed_train, me, rows, n, snap)
            if run >= 0:
                samples["%s/%s" % (backend, mode)].append(ms)
                emit(args, dict(shape(args, n), measure="train", backend=backend, mode=mode, run=run, wall_ms=ms))
    for backend in ("torch", "hip"):
        summarise(args, "train", "wall_ms", {k: v for k, v in samples.items() if k.startswith(backend + "/")},
                  dict(shape(args, n), backend=backend))


def do_child(args):
    """The default mode only (nothing of the GAE surface is touched: the parent commit's package runs this too)."""
    me, rows, n, snap = collect(args)
    me.train_backend = args.backend
    quiet(timed_train, me, rows, n, snap)
    ms = [quiet(timed_train, me, rows, n, snap) for _ in range(args.runs)]
    print(json.dumps(dict(shape(args, n), backend=args.backend, wall_ms=ms, median_ms=statistics.median(ms))), flush=True)


def do_parent(args):
    if not args.parent_pkg or not os.path.exists(os.path.join(args.parent_pkg, "build", "libmagent.so")):
        raise SystemExit("parent: --parent_pkg <dir> with python/ and build/libmagent.so of the parent commit")
    base = [sys.executable, os.path.abspath(__file__), "child", "--algo", args.algo, "--map_size", str(args.map_size),
            "--envs", str(args.envs), "--max_steps", str(args.max_steps), "--runs", str(args.runs)]
    for backend in ("torch", "hip"):
        samples = {"parent": [], "new": []}
        for run in range(args.runs):
            for arm in ("parent", "new"):
                env = dict(os.environ)
                env.pop("BENCH_GAE_PKG", None)
                env.pop("MAGENT_LIB", None)
                if arm == "parent":
                    env["BENCH_GAE_PKG"] = os.path.abspath(args.parent_pkg)
                p = subprocess.run(["timeout", "-k", "10", str(args.limit)] + base + ["--backend", backend], env=env,
                                   capture_output=True, text=True)
                if p.returncode != 0:
                    print(p.stdout[-2000:], p.stderr[-3000:])
                    raise SystemExit("child (%s, %s) exited with %d" % (arm, backend, p.returncode))
                res = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")][-1]
                samples[arm].append(res["median_ms"])
                emit(args, dict(res, measure="parent", arm=arm, run=run))
        summarise(args, "parent", "median wall_ms of a child's train_rollout calls", samples,
                  {"backend": backend, "mode": "returns"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="+", choices=["prepare", "train", "parent", "child"])
    ap.add_argument("--algo", default="mfac", choices=["ac", "mfac"])
    ap.add_argument("--map_size", type=int, default=40)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--max_steps", type=int, default=100)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--backend", default="torch", choices=["torch", "hip"], help="child: the training backend")
    ap.add_argument("--parent_pkg", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if "parent" in args.what:                            # children first: this process has not opened the GPU yet
        do_parent(args)
    if "child" in args.what:
        do_child(args)
    if "prepare" in args.what:
        do_prepare(args)
    if "train" in args.what:
        do_train(args)


if __name__ == "__main__":
    main()
