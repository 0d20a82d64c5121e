"""main_MFQ_Ising.py on the device, as a command line:

    python -m mfrl_amd.main_MFQ_Ising -n 400 -t 0.8 -ts 10000
    python -m mfrl_amd.main_MFQ_Ising -n 400 -t 0.5 0.8 1.2 2.0 --seeds 8 --mcmc 2000

The script's arguments under the script's names (-n -t -epi -ts -lr -dr -dg -ac -ns -s -p); -t takes several
temperatures; new: --seeds S (the numpy seeds 13 .. 13 + S - 1; --seed moves the first), --mcmc SWEEPS (a Metropolis
baseline from an all-up start at the same temperatures, --coupling its exponent's factor) and --out DIR (instead of
the script's ./ising_figs/<time>-<n>-<t>-<lr>-<ac>/ folder).  Every (temperature, seed) episode runs in one launch
(mfrl_amd.ising.sweep), each bit for bit the script run with that seed at that -t.

One temperature and one seed: the script's per-step line, its "+++" marks and its "Episode:" line, in its format.
Several: one line per temperature -- the final order parameter averaged over the seeds, MF-Q and MCMC side by side.
sweep.npz in the folder holds every array of sweep().

Refused with a message: -p (no matplotlib here), -epi other than 1 (mfrl_amd.ising.run_mfq_episodes runs -epi),
-ns other than 4 and a scenario other than Ising.py (the script builds its world with agent_view=1).
"""
import argparse
import os
import sys
import time

import numpy as np


def parser():
    ap = argparse.ArgumentParser(prog="python -m mfrl_amd.main_MFQ_Ising", description=None)
    ap.add_argument('-n', '--num_agents', default=100, type=int)
    ap.add_argument('-t', '--temperature', default=[1.0], type=float, nargs='+')
    ap.add_argument('-epi', '--episode', default=1, type=int)
    ap.add_argument('-ts', '--time_steps', default=10000, type=int)
    ap.add_argument('-lr', '--learning_rate', default=0.1, type=float)
    ap.add_argument('-dr', '--decay_rate', default=0.99, type=float)
    ap.add_argument('-dg', '--decay_gap', default=2000, type=int)
    ap.add_argument('-ac', '--act_rate', default=1.0, type=float)
    ap.add_argument('-ns', '--neighbor_size', default=4, type=int)
    ap.add_argument('-s', '--scenario', default='Ising.py', help='Path of the scenario Python script.')
    ap.add_argument('-p', '--plot', default=0, type=int)
    ap.add_argument('--seeds', default=1, type=int, help='episodes per temperature, on numpy seeds seed .. seed + S - 1')
    ap.add_argument('--seed', default=13, type=int, help="the first numpy seed (the script's is 13)")
    ap.add_argument('--mcmc', default=0, type=int, metavar='SWEEPS', help='Metropolis sweeps of the baseline (0: none)')
    ap.add_argument('--coupling', default=1.0, type=float, help="factor of the Metropolis exponent (DESIGN.md)")
    ap.add_argument('--out', default=None, help="folder for sweep.npz (default: the script's ./ising_figs/...)")
    return ap


def check_args(a):
    """The refusals; raises SystemExit with the message (before anything touches the GPU)."""
    def refuse(msg):
        raise SystemExit("main_MFQ_Ising: " + msg)
    if a.plot:
        refuse("-p is not available: this build has no matplotlib; sweep.npz holds every curve")
    if a.episode != 1:
        refuse("-epi %d: the sweep runs one episode per (temperature, seed); mfrl_amd.ising.run_mfq_episodes runs -epi"
               % a.episode)
    if a.neighbor_size != 4:
        refuse("-ns %d: the script's world has agent_view=1, four neighbours" % a.neighbor_size)
    if os.path.basename(a.scenario) != 'Ising.py':
        refuse("-s %s: only the Ising.py scenario exists" % a.scenario)
    L = int(round(a.num_agents ** 0.5))
    if a.num_agents < 1 or L * L != a.num_agents:
        refuse("-n %d: the lattice needs a square number of agents" % a.num_agents)
    if any(not (np.isfinite(t) and t > 0) for t in a.temperature):
        refuse("-t: every temperature must be a finite value above zero")
    if a.time_steps < 1 or a.seeds < 1 or a.decay_gap < 1 or a.mcmc < 0:
        refuse("-ts, --seeds and -dg must be at least 1 and --mcmc at least 0")
    if not 0.0 <= a.act_rate <= 1.0:
        refuse("-ac %g: the act rate lies in [0, 1]" % a.act_rate)
    if a.mcmc and (L % 2 or L < 4):
        refuse("--mcmc: the Metropolis checkerboard needs an even lattice side >= 4, not %d" % L)


def print_episode(res, i_episode=0):
    """The script's prints (:138-169) of replica (0, 0)."""
    steps = int(res["steps"][0, 0])
    max_order, max_order_step, o_up, o_down = 0.0, 0, 0, 0
    n = res["q"].shape[2]
    done_ = 0
    for t in range(steps):
        order = res["order"][0, 0, t]
        ups = int(res["n_up"][0, 0, t])
        if order > max_order:
            max_order, max_order_step, o_up, o_down = order, t, ups, n - ups
            print("+++++++++++++++++++++++++++++")
        done_ = done_ + 1 if abs(max_order - order) < 0.001 else 0
        if done_ == 500:
            break                                                  # the early stop leaves before its print (:154-159)
        print('E: %d/%d, reward = %f, mse = %f, Order = %f, Up = %d, Down = %d' %
              (i_episode, t, res["rsum"][0, 0, t], res["mse"][0, 0, t], order, ups, n - ups))
    print('Episode: %d, MaxO = %f at %d (%d/%d)' % (i_episode, max_order, max_order_step, o_up, o_down))


def main(argv=None):
    a = parser().parse_args(argv)
    check_args(a)
    from .ising import sweep
    temps = [float(t) for t in a.temperature]
    folder = a.out or ("./ising_figs/" + time.strftime("%Y%m%d-%H%M%S") + "-" + str(a.num_agents) + "-"
                       + "_".join(str(t) for t in temps) + "-" + str(a.learning_rate) + "-" + str(a.act_rate) + "/")
    os.makedirs(folder, exist_ok=True)
    res = sweep(a.num_agents, temps, a.seeds, a.time_steps, lr=a.learning_rate, act_rate=a.act_rate,
                decay_rate=a.decay_rate, decay_gap=a.decay_gap, seed=a.seed, mcmc_sweeps=a.mcmc, coupling=a.coupling)
    if len(temps) == 1 and a.seeds == 1:
        print_episode(res)
        if a.mcmc:
            print('MCMC: Order = %f after %d sweeps' % (res["mc_order_final"][0, 0], a.mcmc))
    else:
        for g, t in enumerate(temps):
            mc = ('%f' % res["mc_order_final"][g].mean()) if a.mcmc else 'n/a'
            print('T = %f: MF-Q Order = %f, MCMC Order = %s (%d seeds, mean steps %.1f)' %
                  (t, res["order_final"][g].mean(), mc, a.seeds, res["steps"][g].mean()))
    np.savez_compressed(os.path.join(folder, "sweep.npz"), **res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
