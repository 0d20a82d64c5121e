"""Ising temperature sweep: what one launch buys, and what the trace costs.  Appends JSON lines to
profiles/ising_sweep.jsonl (--out).

    python scripts/bench_ising_sweep.py [--temps 16] [--seeds 64] [--steps 2000] [--replicas 16384] [--reps 5]

1. sweep_vs_per_temperature: the (temps x seeds) episodes of a 20 x 20 lattice as ONE mfx_ising_mfq_run_sweep call
   (seeds streams generated once, shared through stream_of) against the same episodes as `temps` calls of
   mfx_ising_mfq_run_stream on a `seeds`-replica handle, in the same process, arms alternating.  Each figure is an
   event pair on the engine's stream around the arm (mfx_ising_mark): generation, walk, episode kernels, read-backs
   and, for the per-temperature arm, the host's turn-around between its calls.  The Q tables of the two arms are
   compared bit for bit.
2. trace_cost: mfx_ising_mfq_run (today's kernel) next to mfx_ising_mfq_run_trace on `replicas` replicas in Philox
   mode, the same event pairs, arms alternating; both calls read back Q only (the per-step arrays stay on the
   device), so the difference is the kernels'.
Medians over --reps with the min and max beside them: the spread is part of the result."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mean-field-multi-agent-reinforcement-learning_amd", "python"))

ap = argparse.ArgumentParser()
ap.add_argument("--temps", type=int, default=16)
ap.add_argument("--seeds", type=int, default=64)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--replicas", type=int, default=16384)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ising_sweep.jsonl"))
a = ap.parse_args()

import numpy as np  # noqa: E402
from mfrl_amd import check, lib  # noqa: E402
from mfrl_amd.ising import IsingLattice  # noqa: E402

N, T, G, S = 400, a.steps, a.temps, a.seeds
temps = np.linspace(0.2, 3.2, G)
P = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None  # noqa: E731


def stat(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "runs": len(xs)}


def emit(line):
    line["when"] = time.strftime("%Y-%m-%d %H:%M:%S")
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line), flush=True)


# ------------------------------------------------------------------ 1. one launch against one launch per temperature
big, small = IsingLattice(N, G * S), IsingLattice(N, S)
rep_t, rep_s = np.repeat(temps, S), np.tile(np.arange(S, dtype=np.int32), G)


def arm_sweep():
    big.mark(0)
    res = big.run_mfq_sweep(T, rep_t, rep_s, S, seed=13)
    big.mark(1)
    return big.marked_ms(), res


def arm_per_temperature():
    small.mark(0)
    res = [small.run_mfq_stream(T, float(t), seed=13)[0] for t in temps]
    small.mark(1)
    return small.marked_ms(), res


arm_sweep(), arm_per_temperature()                      # warm-up: code objects, the engines' buffers at these shapes
ms_sweep, ms_per = [], []
for _ in range(a.reps):
    m, sw = arm_sweep()
    ms_sweep.append(m)
    m, per = arm_per_temperature()
    ms_per.append(m)
same = all(sw["q"][g * S:(g + 1) * S].tobytes() == per[g]["q"].tobytes()
           and np.array_equal(sw["steps"][g * S:(g + 1) * S], per[g]["steps"]) for g in range(G))
spin_steps = int(sw["steps"].sum()) * N
emit({"metric": "Ising 20x20 temperature sweep, one launch vs one launch per temperature", "temps": G, "seeds": S,
      "steps_cap": T, "episodes": G * S, "spin_steps": spin_steps, "sweep_one_launch": stat(ms_sweep),
      "per_temperature_launches": stat(ms_per),
      "ratio_per_temperature_over_sweep": statistics.median(ms_per) / statistics.median(ms_sweep),
      "sweep_spin_steps_per_s": spin_steps / (statistics.median(ms_sweep) * 1e-3),
      "timed": "event pair on the engine's stream around the whole arm (generation, walk, kernels, read-backs)",
      "q_and_steps_equal_bit_for_bit": bool(same)})
del big, small, sw, per

# ------------------------------------------------------------------ 2. the cost of the trace (Philox mode)
R = a.replicas
lat = IsingLattice(N, R)
spins0 = np.random.RandomState(7).randint(0, 2, size=(R, N)).astype(np.uint8)
q = np.empty((R, N, 5, 2))
steps = np.empty(R, np.int32)
L = lib()


def arm_plain():
    lat.set_spins(spins0)
    lat.mark(0)
    check(L.mfx_ising_mfq_run(lat._h, T, ctypes.c_double(0.8), ctypes.c_double(0.1), ctypes.c_double(0.99), 2000,
                              None, None, ctypes.c_uint(7), P(q), None, None, P(steps)), "mfx_ising_mfq_run")
    lat.mark(1)
    return lat.marked_ms(), q.tobytes(), int(steps.sum())


def arm_trace():
    lat.set_spins(spins0)
    lat.mark(0)
    check(L.mfx_ising_mfq_run_trace(lat._h, T, ctypes.c_double(0.8), None, ctypes.c_double(0.1),
                                    ctypes.c_double(0.99), 2000, None, None, ctypes.c_uint(7), P(q), None, None,
                                    P(steps), None, None), "mfx_ising_mfq_run_trace")
    lat.mark(1)
    return lat.marked_ms(), q.tobytes(), int(steps.sum())


arm_plain(), arm_trace()
ms_plain, ms_trace = [], []
for _ in range(a.reps):
    m, q_plain, done = arm_plain()
    ms_plain.append(m)
    m, q_trace, done_t = arm_trace()
    ms_trace.append(m)
emit({"metric": "Ising 20x20 MF-Q, cost of the per-step trace (Philox mode)", "replicas": R, "steps_cap": T,
      "spin_steps": done * N, "k_ising_mfq<4>": stat(ms_plain), "k_ising_mfq<4, trace>": stat(ms_trace),
      "ratio_trace_over_plain": statistics.median(ms_trace) / statistics.median(ms_plain),
      "plain_spin_steps_per_s": done * N / (statistics.median(ms_plain) * 1e-3),
      "trace_spin_steps_per_s": done_t * N / (statistics.median(ms_trace) * 1e-3),
      "timed": "event pair on the engine's stream around the call: the kernel and the read-back of Q and steps "
               "(the same in both arms; the per-step arrays are not read back)",
      "q_equal_bit_for_bit": q_plain == q_trace and done == done_t})
