"""A/B of the two training backends of ActorCritic / MFAC -- "torch" (autograd per 65,536-row chunk + torch.optim.Adam,
as train_rollout runs it) and "hip" (the hand-written training step, csrc/actrain_kernels.hip, as _hip_train runs it:
the step, the export into the torch module and the hand-over to the acting forward) -- on one set of synthetic rows, in
one process.

    python scripts/bench_actrain.py [--algo mfac] [--reps 3] [--rows 409600,6400] [--out profiles/actrain_ab.jsonl]

Rows: 409,600 = one MF-AC round at 64 envs of 40 x 40 over 100 steps; 6,400 = a small round (1 env).  Views are 30 %
dense uniform, features uniform, mean actions Dirichlet-like, actions uniform, returns randn.  Two models with the same
initial weights.  After a warm-up call of each backend (allocations), --reps alternating pairs, timed by HIP events
around the whole training call.  One JSON line per timed call and one summary line per row count are appended to --out.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mean-field-multi-agent-reinforcement-learning_amd", "python"))

import magent  # noqa: E402
from mfrl_amd.algo import spawn_ai  # noqa: E402


def make_rows(n, A, F, use_mf, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.rand(*s, device="cuda", generator=g)
    cols = {"obs": (r(n, 13 * 13 * 7) < 0.3).float() * r(n, 13 * 13 * 7), "feat": r(n, F),
            "act": torch.randint(0, A, (n,), device="cuda", generator=g, dtype=torch.int32),
            "ret": torch.randn(n, device="cuda", generator=g), "prob": None}
    if use_mf:
        p = r(n, A)
        cols["prob"] = (p / p.sum(1, keepdim=True)).contiguous()
    return cols


def train_torch(model, cols, n):
    """The training part of ActorCritic.train_rollout, "torch" backend."""
    chunk = model.ROLLOUT_CHUNK_ROWS
    model.optimizer.zero_grad(set_to_none=True)
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        pg, vf, ent, _ = model.losses(cols["obs"][a:b], cols["feat"][a:b], cols["act"][a:b], cols["ret"][a:b],
                                      cols["prob"][a:b] if cols["prob"] is not None else None, total_rows=n)
        (pg + vf + ent).backward()
    model.optimizer.step()


def train_hip(model, cols, n):
    model._hip_train(cols, n)


def timed(fn, model, cols, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(model, cols, n)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", default="mfac", choices=["ac", "mfac"])
    ap.add_argument("--rows", default="409600,6400")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "actrain_ab.jsonl"))
    args = ap.parse_args()
    env = magent.GridWorld("battle", map_size=40)
    h = env.get_handles()
    use_mf = args.algo == "mfac"
    lines = []
    for n in [int(x) for x in args.rows.split(",")]:
        np.random.seed(0)
        torch.manual_seed(0)
        models = {k: spawn_ai(args.algo, None, env, h[0], args.algo + "-" + k, 400) for k in ("torch", "hip")}
        models["hip"].net.load_state_dict(models["torch"].net.state_dict())
        models["hip"].train_backend = "hip"
        fns = {"torch": train_torch, "hip": train_hip}
        cols = make_rows(n, models["hip"].num_actions, models["hip"].feature_space[0], use_mf, 1)
        for k in ("torch", "hip"):
            timed(fns[k], models[k], cols, n)                     # warm-up: allocations, kernel loading
        ms = {"torch": [], "hip": []}
        for rep in range(args.reps):
            for k in ("hip", "torch"):
                x = timed(fns[k], models[k], cols, n)
                ms[k].append(x)
                lines.append({"algo": args.algo, "backend": k, "rep": rep, "rows": n, "ms": round(x, 3)})
                print(json.dumps(lines[-1]), flush=True)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        flop = n * (1.87e6 if use_mf else 1.50e6) * 2
        lines.append({"algo": args.algo, "summary": True, "rows": n, "ms_torch": round(med["torch"], 3),
                      "ms_hip": round(med["hip"], 3), "torch_over_hip": round(med["torch"] / med["hip"], 3),
                      "hip_tflops": round(flop / med["hip"] / 1e9, 2), "device": torch.cuda.get_device_name(0)})
        print(json.dumps(lines[-1]), flush=True)
        del cols, models
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
