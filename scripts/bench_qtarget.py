"""What the opt-in Boltzmann value target (ValueNet.target_rule = "boltzmann") costs, and that the default
"max" rule costs what it did, on bench_qtrain.py's synthetic replay ring, in one process.

    python scripts/bench_qtarget.py [--rows 80000] [--batches 2000] [--reps 5] [--parent_lib build/libmagent_parent.so]
                                    [--out profiles/qtarget_ab.jsonl]

  arm a   QTrainHIP.run under "max" on this build against the same call on --parent_lib (the library of the commit
          before the rule existed, built by `make` in a checkout of it; skipped when the file is not given), and under
          "boltzmann" at T = 0.1: --batches minibatches of 64 rows per timed call, the arms alternating, --reps runs
  arm b   ValueNet.train_batches, "max" against "boltzmann", for both backends ("torch": the captured graph; "hip": the
          hand-written step with the pack / unpack of the weights), MF-Q and DQN
  arm c   the stand-alone kernels: mf.mfq_target against mf.mfq_target_boltzmann at M = 4,096 and 262,144 rows, A = 21

Every timed call sits between two HIP events; one JSON line per timed call and one summary line (median, min, max) per
arm are appended to --out."""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mean-field-multi-agent-reinforcement-learning_amd", "python"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import magent  # noqa: E402
from bench_qtrain import fill  # noqa: E402
from mfrl_amd import mf, qtrain  # noqa: E402
from mfrl_amd.algo import spawn_ai  # noqa: E402

T_SOFT = 0.1


class _Missing:
    restype = None


class _OlderLib:
    """A library from before mfx_qtrain_set_target: QTrainHIP's constructor may name the entry point, nothing calls it."""

    def __init__(self, path):
        self._dll = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)

    def __getattr__(self, name):
        try:
            return getattr(self._dll, name)
        except AttributeError:
            return _Missing()


def handle_on(library, model):
    """A QTrainHIP on `library` (None: this build's) holding `model`'s weights."""
    keep = qtrain.lib
    if library is not None:
        qtrain.lib = lambda: library
    try:
        tr = qtrain.QTrainHIP(model.view_space, model.feature_space, model.num_actions, model.use_mf, lr=model.lr,
                              tau=model.tau, gamma=model.gamma)
    finally:
        qtrain.lib = keep
    tr.load(model.eval_net, model.target_net)
    return tr


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def summary(arm, ms, **extra):
    out = dict(extra, arm=arm, summary=True, device=torch.cuda.get_device_name(0))
    for k, v in ms.items():
        out[k] = {"median": round(float(np.median(v)), 5), "min": round(float(min(v)), 5), "max": round(float(max(v)), 5)}
    return out


def arm_a(args, env, h, emit):
    model = spawn_ai("mfq", None, env, h[0], "mfq-a", 400, memory_size=args.rows)
    buf = model.replay_buffer
    fill(buf, args.rows, 1, True)
    cols = {"obs0": buf.obs0.data, "feat0": buf.feat0.data, "actions": buf.actions.data, "rewards": buf.rewards.data,
            "terminals": buf.terminals.data, "masks": buf.masks.data, "prob": buf.prob.data}
    idx = torch.as_tensor(np.random.RandomState(2).randint(args.rows, size=(args.batches, buf.batch_size)), device="cuda")
    arms = {"max": handle_on(None, model), "boltzmann": handle_on(None, model)}
    arms["boltzmann"].set_target("boltzmann", T_SOFT)
    if args.parent_lib:
        arms["max_parent"] = handle_on(_OlderLib(args.parent_lib), model)
    for tr in arms.values():
        tr.run(cols, args.rows, idx[:8])
        tr.check_error()
    ms = {k: [] for k in arms}
    for rep in range(args.reps):
        for k, tr in arms.items():
            x = event_ms(lambda: tr.run(cols, args.rows, idx)) / args.batches
            tr.check_error()
            ms[k].append(x)
            emit({"arm": "a", "rule": k, "rep": rep, "rows": args.rows, "batch_size": buf.batch_size,
                  "minibatches": args.batches, "ms_per_minibatch": round(x, 5)})
    emit(summary("a", ms, unit="ms_per_minibatch", launches_per_minibatch=13))


def timed_train(model, buf, batches, use_mean):
    with contextlib.redirect_stdout(io.StringIO()):
        return event_ms(lambda: model.train_batches(buf, batches, use_mean)) / batches


def arm_b(args, env, h, emit):
    for algo, use_mean in (("mfq", True), ("il", False)):
        np.random.seed(0)
        torch.manual_seed(0)
        keys = [(b, r) for b in ("torch", "hip") for r in ("max", "boltzmann")]
        models = {}
        for b, r in keys:
            m = spawn_ai(algo, None, env, h[0], "%s-%s-%s" % (algo, b, r), 400, memory_size=args.rows)
            if models:
                first = models[keys[0]]
                m.eval_net.load_state_dict(first.eval_net.state_dict())
                m.target_net.load_state_dict(first.target_net.state_dict())
            if b == "hip":
                m.train_backend = "hip"
            m.target_rule, m.temperature = r, T_SOFT
            models[(b, r)] = m
        buf = models[keys[0]].replay_buffer
        fill(buf, args.rows, 1, use_mean)
        for k in keys:
            timed_train(models[k], buf, 8, use_mean)                 # warm-up: graph capture, allocations
        ms = {"%s/%s" % k: [] for k in keys}
        for rep in range(args.reps):
            for k in keys:
                x = timed_train(models[k], buf, args.batches, use_mean)
                ms["%s/%s" % k].append(x)
                emit({"arm": "b", "algo": algo, "backend": k[0], "rule": k[1], "rep": rep, "rows": args.rows,
                      "batch_size": buf.batch_size, "minibatches": args.batches, "ms_per_minibatch": round(x, 5)})
        emit(summary("b", ms, algo=algo, unit="ms_per_minibatch", temperature=T_SOFT))
        del models, buf
        torch.cuda.empty_cache()


def arm_c(args, emit):
    g = torch.Generator(device="cuda").manual_seed(3)
    calls = 200
    for M in (4096, 262144):
        eq = torch.rand(M, 21, device="cuda", generator=g) * 6 - 3
        tq = torch.rand(M, 21, device="cuda", generator=g) * 20 - 10
        r = torch.randn(M, device="cuda", generator=g)
        d = (torch.rand(M, device="cuda", generator=g) < 0.1).to(torch.uint8)
        fns = {"max": lambda: mf.mfq_target(eq, tq, r, d, 0.95),
               "boltzmann": lambda: mf.mfq_target_boltzmann(eq, tq, r, d, 0.95, T_SOFT)}
        for fn in fns.values():
            fn()
        ms = {k: [] for k in fns}
        for rep in range(args.reps):
            for k, fn in fns.items():
                x = event_ms(lambda: [fn() for _ in range(calls)]) / calls
                ms[k].append(x)
                emit({"arm": "c", "rule": k, "rep": rep, "M": M, "A": 21, "calls": calls, "ms_per_call": round(x, 6)})
        emit(summary("c", ms, M=M, A=21, unit="ms_per_call (wrapper included)"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=80000)
    ap.add_argument("--batches", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "qtarget_ab.jsonl"))
    args = ap.parse_args()
    env = magent.GridWorld("battle", map_size=40)
    h = env.get_handles()
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    arm_a(args, env, h, emit)
    torch.cuda.empty_cache()
    arm_b(args, env, h, emit)
    arm_c(args, emit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
