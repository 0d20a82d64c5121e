"""Measurements of the PPO objective of AC / MFAC (ActorCritic.objective = "ppo"), appended as JSON lines to
--out (profiles/ppo_ab.jsonl is such a run).  The frame is scripts/bench_gae.py's: one round of rows is collected on the
device rollout loop (MF-AC, 64 envs of 40x40, 100 steps by default: about 409,600 rows); every measure then runs on
those same rows, the arms alternating, --runs times after one warm-up pass, and ends with a summary line per arm: median
(min-max), and "resolved": false against the first arm when the two ranges overlap.

  prepare  round preparation, tails known -> columns ready (device events on the engine's stream):
             gae        value forward over all rows + mfx_chain_gae
             ppo        policy + value forward over all rows (sliced) + mfx_policy_logp + mfx_chain_gae
  train    the whole train_rollout() call (wall clock around it, the device idle before and after), backend x mode:
             torch / hip  x  gae (one step) / ppo (ppo_epochs x ppo_minibatches steps, the default 4 x 4)
           the weights are put back before every call, so every call trains from the same state
  head     ACTrainHIP.grads on the same rows with the advantage column (k_at_loss<true>) and with logp_old + clip
           (k_at_loss_ppo): device events around the call; the two differ in the loss head alone
  parent   the modes that exist in the parent commit ("returns", "gae") against the parent commit's package: child
           processes of this script (measure "child": one collected round, --runs train_rollout() calls, their median),
           alternating between this tree and --parent_pkg (<parent_pkg>/python and <parent_pkg>/build/libmagent.so of the
           parent commit, its include/magent_amd.h two levels above python/), per backend and mode.

    python scripts/bench_ppo.py --out profiles/ppo_ab.jsonl prepare train head
    python scripts/bench_ppo.py --out profiles/ppo_ab.jsonl --parent_pkg <dir> parent
"""
import argparse
import copy
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_gae as bg  # noqa: E402  (the frame: emit, summarise, collect, quiet; BENCH_GAE_PKG selects the package)


def do_prepare(args):
    import torch
    from mfrl_amd import replay
    me, rows, n, snap = bg.collect(args)
    c = rows.cols
    use_mf = "prob" in c
    hip = me._hip_net()
    tails = c["tail"][:n].nonzero().reshape(-1)
    value = torch.empty(n, dtype=torch.float32, device="cuda")
    adv = torch.empty(n, dtype=torch.float32, device="cuda")
    logp = torch.empty(n, dtype=torch.float32, device="cuda")
    S = me.PPO_FORWARD_ROWS

    def gae(rew):
        _, v, _ = hip.forward(c["obs"][:n], c["feat"][:n], c["prob"][:n] if use_mf else None, want_policy=False,
                              want_value=True, want_act=False)
        value.copy_(v.reshape(-1))
        replay.chain_gae(rew, adv, c["prev"], tails, value, me.gamma, 0.95)

    def ppo(rew):
        for a in range(0, n, S):
            b = min(a + S, n)
            pol, v, _ = hip.forward(c["obs"][a:b], c["feat"][a:b], c["prob"][a:b] if use_mf else None, want_policy=True,
                                    want_value=True, want_act=False)
            value[a:b].copy_(v.reshape(-1))
            replay.policy_logp(pol, c["act"][a:b], logp[a:b])
        replay.chain_gae(rew, adv, c["prev"], tails, value, me.gamma, 0.95)

    arms = {"gae": gae, "ppo": ppo}
    samples = {k: [] for k in arms}
    with torch.no_grad():
        for run in range(-1, args.runs):                 # run -1: warm-up, not reported
            for name, fn in arms.items():
                rew = snap.clone()                       # the walk works in place: a fresh copy, off the clock
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn(rew)
                b.record()
                torch.cuda.synchronize()
                if run >= 0:
                    samples[name].append(a.elapsed_time(b))
                    bg.emit(args, dict(bg.shape(args, n), measure="prepare", arm=name, run=run, chains=len(tails),
                                       device_ms=a.elapsed_time(b)))
    bg.summarise(args, "prepare", "device_ms", samples, dict(bg.shape(args, n), chains=len(tails)))


def do_train(args):
    import torch
    me, rows, n, snap = bg.collect(args)
    state0 = copy.deepcopy(me.net.state_dict())
    me.advantage = "gae"
    arms = [(b, m) for b in ("torch", "hip") for m in ("gae", "ppo")]
    samples = {"%s/%s" % a: [] for a in arms}
    for run in range(-1, args.runs):
        for backend, mode in arms:
            me.net.load_state_dict(state0)
            me.train_backend = backend
            me.objective = "pg" if mode == "gae" else "ppo"
            ms = bg.quiet(bg.timed_train, me, rows, n, snap)
            if run >= 0:
                samples["%s/%s" % (backend, mode)].append(ms)
                bg.emit(args, dict(bg.shape(args, n), measure="train", backend=backend, mode=mode, run=run, wall_ms=ms,
                                   steps=1 if mode == "gae" else me.ppo_epochs * min(me.ppo_minibatches, n)))
    for backend in ("torch", "hip"):
        bg.summarise(args, "train", "wall_ms", {k: v for k, v in samples.items() if k.startswith(backend + "/")},
                     dict(bg.shape(args, n), backend=backend, ppo_epochs=me.ppo_epochs, ppo_minibatches=me.ppo_minibatches))


def do_head(args):
    import torch
    from mfrl_amd import replay
    me, rows, n, snap = bg.collect(args)
    c = rows.cols
    use_mf = "prob" in c
    tr = me._hip_trainer()
    with torch.no_grad():
        pol, _, _ = me._hip_net().forward(c["obs"][:n], c["feat"][:n], c["prob"][:n] if use_mf else None,
                                          want_policy=True, want_value=True, want_act=False)
        logp = replay.policy_logp(pol, c["act"][:n], torch.empty(n, dtype=torch.float32, device="cuda"))
    del pol
    adv = torch.randn(n, device="cuda")
    base = {"obs": c["obs"], "feat": c["feat"], "act": c["act"], "ret": c["rew"], "prob": c["prob"] if use_mf else None,
            "adv": adv}
    arms = {"adv": (base, None), "ppo": (dict(base, logp_old=logp), me.ppo_clip)}
    samples = {k: [] for k in arms}
    for run in range(-1, args.runs):
        for name, (cols, clip) in arms.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            tr.grads(cols, n, clip=clip)
            b.record()
            torch.cuda.synchronize()
            if run >= 0:
                samples[name].append(a.elapsed_time(b))
                bg.emit(args, dict(bg.shape(args, n), measure="head", arm=name, run=run, device_ms=a.elapsed_time(b)))
    tr.check_error()
    bg.summarise(args, "head", "device_ms of ACTrainHIP.grads", samples, bg.shape(args, n))


def do_child(args):
    """Modes of the parent commit only (nothing of the PPO surface is touched: the parent's package runs this too)."""
    me, rows, n, snap = bg.collect(args)
    me.train_backend = args.backend
    me.advantage = args.mode
    bg.quiet(bg.timed_train, me, rows, n, snap)
    ms = [bg.quiet(bg.timed_train, me, rows, n, snap) for _ in range(args.runs)]
    print(json.dumps(dict(bg.shape(args, n), backend=args.backend, mode=args.mode, wall_ms=ms,
                          median_ms=statistics.median(ms))), flush=True)


def do_parent(args):
    if not args.parent_pkg or not os.path.exists(os.path.join(args.parent_pkg, "build", "libmagent.so")):
        raise SystemExit("parent: --parent_pkg <dir> with python/ and build/libmagent.so of the parent commit")
    base = [sys.executable, os.path.abspath(__file__), "child", "--algo", args.algo, "--map_size", str(args.map_size),
            "--envs", str(args.envs), "--max_steps", str(args.max_steps), "--runs", str(args.runs)]
    for backend in ("torch", "hip"):
        for mode in ("returns", "gae"):
            samples = {"parent": [], "new": []}
            for run in range(args.runs):
                for arm in ("parent", "new"):
                    env = dict(os.environ)
                    env.pop("BENCH_GAE_PKG", None)
                    env.pop("MAGENT_LIB", None)
                    if arm == "parent":
                        env["BENCH_GAE_PKG"] = os.path.abspath(args.parent_pkg)
                    p = subprocess.run(["timeout", "-k", "10", str(args.limit)] + base + ["--backend", backend, "--mode", mode],
                                       env=env, capture_output=True, text=True)
                    if p.returncode != 0:
                        print(p.stdout[-2000:], p.stderr[-3000:])
                        raise SystemExit("child (%s, %s, %s) exited with %d" % (arm, backend, mode, p.returncode))
                    res = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")][-1]
                    samples[arm].append(res["median_ms"])
                    bg.emit(args, dict(res, measure="parent", arm=arm, run=run))
            bg.summarise(args, "parent", "median wall_ms of a child's train_rollout calls", samples,
                         {"backend": backend, "mode": mode})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="+", choices=["prepare", "train", "head", "parent", "child"])
    ap.add_argument("--algo", default="mfac", choices=["ac", "mfac"])
    ap.add_argument("--map_size", type=int, default=40)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--max_steps", type=int, default=100)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--backend", default="torch", choices=["torch", "hip"], help="child: the training backend")
    ap.add_argument("--mode", default="returns", choices=["returns", "gae"], help="child: the advantage")
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
    if "head" in args.what:
        do_head(args)


if __name__ == "__main__":
    main()
