"""The Q network's acting forward, greedy against the Boltzmann draw (QNetHIP.act with temperature=None / T), f32 and
bf16, on --rows observation rows (default 262,144: live agents of a 64x64 rush rollout, tiled), mean-field net.

    python scripts/bench_qsample.py --out profiles/qsample_ab.jsonl
    MAGENT_LIB=<an older build> python scripts/bench_qsample.py --arms greedy      # the untouched greedy kernels

Every timing is a device-event pair on the current stream around --iters forwards; the arms alternate inside one
process (rep 0: every arm, rep 1: every arm, ...), --reps of each.  One JSON line per (precision, arm): median, min
and max of the per-forward milliseconds.  The sampled arm's actions are checked against mfrl_amd.mf.q_sample on the
greedy forward's Q values before the clock (bit for bit)."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mean-field-multi-agent-reinforcement-learning_amd", "python"))
sys.path.insert(0, os.path.join(REPO, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=262144)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--temperature", type=float, default=0.1)
ap.add_argument("--arms", nargs="+", choices=["greedy", "boltzmann"], default=["greedy", "boltzmann"])
ap.add_argument("--precisions", nargs="+", choices=["f32", "bf16"], default=["f32", "bf16"])
ap.add_argument("--out", type=str, default=None, help="append the JSON lines to this file too")
a = ap.parse_args()

import torch  # noqa: E402

import battle_driver as bd  # noqa: E402
from mfrl_amd import mf  # noqa: E402
from mfrl_amd.algo.nets import QNet  # noqa: E402
from mfrl_amd.battle import BattleBatch  # noqa: E402
from mfrl_amd.policy import QNetHIP  # noqa: E402

assert torch.cuda.is_available(), "bench_qsample.py measures on the GPU"
torch.cuda.set_device(0)
VS, FS, NA = (13, 13, 7), (34,), 21


def observation_rows(n):
    E = 1024
    left, right = bd.block_positions(64, 128)
    eng = BattleBatch(64, E, stream=torch.cuda.current_stream())
    eng.rollout_init([left, right], max_steps=400, eps=0.2, seed=5, stagger=True)
    eng.rollout_step(40)
    rc = eng.rowcap
    view = torch.empty((E, rc, 1183), dtype=torch.float32, device="cuda")
    feat = torch.empty((E, rc, 34), dtype=torch.float32, device="cuda")
    num = torch.empty((E, 2), dtype=torch.int32, device="cuda")
    mean = torch.empty((E, 2, NA), dtype=torch.float64, device="cuda")
    eng.rollout_copy("view", view, group=0)
    eng.rollout_copy("feature", feat, group=0)
    eng.rollout_copy("group_num", num)
    eng.rollout_copy("mean_action", mean)
    eng.sync()
    live = torch.arange(rc, device="cuda")[None, :] < num[:, 0:1]
    v, f, p = view[live], feat[live], mean[:, 0:1, :].expand(E, rc, NA)[live].float()
    idx = torch.arange(n, device="cuda") % v.shape[0]
    return v[idx].contiguous(), f[idx].contiguous(), p[idx].contiguous()


torch.manual_seed(3)
net = QNet(VS, FS, NA, True).cuda()
with torch.no_grad():
    for prm in net.parameters():
        prm.add_(0.05 * torch.randn_like(prm))
view, feat, prob = observation_rows(a.rows)
lib = os.path.basename(os.environ.get("MAGENT_LIB") or "libmagent.so")
lines = []
for precision in a.precisions:
    hip = QNetHIP(VS, FS, NA, True, precision=precision).load(net)
    kw = {"greedy": {}, "boltzmann": {"temperature": a.temperature, "seed": 11, "step": 1}}
    if "boltzmann" in a.arms:
        q, _ = hip.forward(view, feat, prob)
        got = hip.act(view, feat, prob, **kw["boltzmann"])
        want = mf.q_sample(q, a.temperature, 11, 1)
        torch.cuda.synchronize()
        assert torch.equal(got, want), "the fused draw differs from q_sample on the forward's Q"
        del q
    ms = {arm: [] for arm in a.arms}
    for arm in a.arms:
        for _ in range(a.warmup):
            hip.act(view, feat, prob, **kw[arm])
    torch.cuda.synchronize()
    for rep in range(a.reps):
        for arm in a.arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                hip.act(view, feat, prob, **kw[arm])
            e1.record()
            e1.synchronize()
            ms[arm].append(e0.elapsed_time(e1) / a.iters)
    for arm in a.arms:
        x = ms[arm]
        lines.append({"script": "bench_qsample.py", "lib": lib, "precision": precision, "arm": arm, "rows": a.rows,
                      "temperature": a.temperature if arm == "boltzmann" else None, "reps": a.reps, "iters": a.iters,
                      "ms_median": round(statistics.median(x), 4), "ms_min": round(min(x), 4),
                      "ms_max": round(max(x), 4), "rows_per_s": round(a.rows / (statistics.median(x) * 1e-3), 1)})
for ln in lines:
    print(json.dumps(ln))
if a.out:
    with open(a.out, "a") as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + "\n")
