"""A/B of ValueNet.train_batches' two backends -- "torch" (autograd + Adam replayed as a HIP graph) and "hip" (the
hand-written training step, csrc/qtrain_kernels.hip) -- on one synthetic replay ring, in one process.

    python scripts/bench_qtrain.py [--rows 80000] [--batches 2000] [--reps 3] [--out profiles/qtrain_ab.jsonl]

Per algorithm (MF-Q, DQN): a seeded ring of --rows entries (uniform views / features / mean actions, uniform actions,
rewards 0.5 randn, 10 % terminals, 80 % masks), two models with the same initial weights, batch size 64.  After a
warm-up call of each backend (graph capture, allocations), --reps alternating pairs of train_batches(buf, --batches)
timed by HIP events around the whole call: index upload, the minibatch loop, and for "hip" the pack / unpack of the
weights.  One JSON line per timed call and one summary line per algorithm are appended to --out."""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mean-field-multi-agent-reinforcement-learning_amd", "python"))

import magent  # noqa: E402
from mfrl_amd.algo import spawn_ai  # noqa: E402


def fill(buf, rows, seed, use_mean):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.rand(*s, device="cuda", generator=g)
    cols = {"obs0": r(rows, 13, 13, 7), "feat0": r(rows, buf.feat0.data.shape[1]),
            "actions": torch.randint(0, buf.act_n, (rows,), device="cuda", generator=g, dtype=torch.int32),
            "rewards": 0.5 * torch.randn(rows, device="cuda", generator=g), "terminals": r(rows) < 0.1,
            "masks": r(rows) < 0.8}
    if use_mean:
        p = r(rows, buf.act_n)
        cols["prob"] = p / p.sum(1, keepdim=True)
    for k, t in cols.items():
        mb = getattr(buf, k)
        mb.data[:rows] = t
        mb.length = rows


def timed(model, buf, batches, use_mean):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with contextlib.redirect_stdout(io.StringIO()):
        a.record()
        model.train_batches(buf, batches, use_mean)
        b.record()
        torch.cuda.synchronize()
    return a.elapsed_time(b) / batches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=80000)
    ap.add_argument("--batches", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "qtrain_ab.jsonl"))
    args = ap.parse_args()
    env = magent.GridWorld("battle", map_size=40)
    h = env.get_handles()
    lines = []
    for algo, use_mean in (("mfq", True), ("il", False)):
        np.random.seed(0)
        torch.manual_seed(0)
        models = {k: spawn_ai(algo, None, env, h[0], algo + "-" + k, 400, memory_size=args.rows) for k in ("torch", "hip")}
        models["hip"].eval_net.load_state_dict(models["torch"].eval_net.state_dict())
        models["hip"].target_net.load_state_dict(models["torch"].target_net.state_dict())
        models["hip"].train_backend = "hip"
        buf = models["torch"].replay_buffer
        fill(buf, args.rows, 1, use_mean)
        for k in ("torch", "hip"):
            timed(models[k], buf, 8, use_mean)                    # warm-up: graph capture, allocations
        ms = {"torch": [], "hip": []}
        for rep in range(args.reps):
            for k in ("hip", "torch"):
                x = timed(models[k], buf, args.batches, use_mean)
                ms[k].append(x)
                lines.append({"algo": algo, "backend": k, "rep": rep, "rows": args.rows, "batch_size": buf.batch_size,
                              "minibatches": args.batches, "ms_per_minibatch": round(x, 5)})
                print(json.dumps(lines[-1]), flush=True)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        lines.append({"algo": algo, "summary": True, "ms_per_minibatch_torch": round(med["torch"], 5),
                      "ms_per_minibatch_hip": round(med["hip"], 5), "torch_over_hip": round(med["torch"] / med["hip"], 3),
                      "launches_per_minibatch_hip": 13, "device": torch.cuda.get_device_name(0)})
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
