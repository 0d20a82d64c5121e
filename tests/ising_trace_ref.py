"""TEST ORACLE ONLY -- numpy restatements of part 3b of include/magent_amd.h (the trace / sweep variants of the fused
MF-Q kernels and the Metropolis baseline).  The product never imports this.

  * target(K)                    -- reward_target of main_MFQ_Ising.py:77-81 for any K
  * device_mse(terms, n)         -- the mse of one step in the DEVICE's summation order
  * trace() / trace_given()      -- the episode of oracle/ising_oracle.py (mfq / mfq_given) with the per-step
                                    sum(reward) and mse added
  * metropolis()                 -- the chain of k_ising_mc

Summation order of the mse (the contract): the workgroup has B lanes, B = 64 * ceil(N / 64) up to 1024; lane l adds
the terms of its own agents l, l + B, ... in ascending index (from 0.0; an agent outside act_group adds nothing); an
xor butterfly with masks 1, 2, 4, 8, 16, 32 runs over each wave's 64 lanes (v = v + v[lane ^ m]); lane 0 adds the
waves' partials in wave order; the sum is divided by float(N).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import ising_oracle  # noqa: E402

MC_DOMAIN = 0x5EED2                 # the fourth Philox counter word of k_ising_mc's draws (the MF-Q draws: 0x5EED1)
_LANE = np.arange(64)


def target(K):
    """[K + 1][2]: target[s][a] = (a ? 1 : -1) (2 s - K) / 2."""
    s = np.arange(K + 1, dtype=np.float64)[:, None]
    sign = np.array([-1.0, 1.0])[None, :]
    return sign * (2.0 * s - K) / 2.0


def device_mse(terms, n_agents):
    """terms [N] float64, 0.0 where the agent did not update -> the step's mse as the kernels add it."""
    B = 1024 if n_agents > 1024 else (n_agents + 63) // 64 * 64
    lanes = np.zeros(B)
    for c in range(0, n_agents, B):
        part = terms[c:c + B]
        lanes[:len(part)] = lanes[:len(part)] + part
    v = lanes.reshape(-1, 64)
    for m in (1, 2, 4, 8, 16, 32):
        v = v + v[:, _LANE ^ m]
    s = v[0, 0]
    for w in range(1, v.shape[0]):
        s = s + v[w, 0]
    return s / float(n_agents)


def _run(spins, nbr, steps, temperature, lr, decay_rate, decay_gap, draw_u, draw_grp):
    """ising_oracle._run with "rsum" (sum(reward), exact: every reward is a multiple of 0.5), "mse" (device order)
    and "mse_script" (the terms added in act_group order, as main_MFQ_Ising.py:125-133 adds them)."""
    n = len(spins)
    K = nbr.shape[1]
    tg = target(K)
    Q = np.zeros((n, K + 1, 2))
    current_t, max_order, done_ = 0.3, 0.0, 0
    orders, nups, acts, rsum, mse, mse_script, gaps = [], [], [], [], [], [], []
    ar = np.arange(n)
    for t in range(steps):
        if t % decay_gap == 0:
            current_t *= decay_rate
        if current_t < temperature:
            current_t = temperature
        st = spins[nbr].sum(axis=1)
        e0 = np.exp(Q[ar, st, 0] / current_t)
        e1 = np.exp(Q[ar, st, 1] / current_t)
        denom = e0 + e1
        p0, p1 = e0 / denom, e1 / denom
        c0 = p0 / (p0 + p1)
        u = draw_u(t)
        gaps.append(float(np.abs(u - c0).min()))
        action = (u >= c0).astype(np.int64)
        spins, reward, _obs, n_up, order = ising_oracle.env_step(spins, nbr, action)
        grp = np.asarray(draw_grp(t))
        qn = Q[grp, st[grp], action[grp]] + lr * (reward[grp] - Q[grp, st[grp], action[grp]])
        Q[grp, st[grp], action[grp]] = qn
        d = qn - tg[st[grp], action[grp]]
        terms = np.zeros(n)
        terms[grp] = d * d
        mse.append(device_mse(terms, n))
        acc = 0.0
        for x in d * d:                                        # act_group order
            acc += x
        mse_script.append(acc / n)
        rsum.append(float(reward.sum()))
        orders.append(order)
        nups.append(n_up)
        acts.append(action)
        if order > max_order:
            max_order = order
        if abs(max_order - order) < 0.001:
            done_ += 1
        else:
            done_ = 0
        if done_ == 500:
            break
    return {"q": Q, "order": np.array(orders), "n_up": np.array(nups), "actions": np.stack(acts), "spins": spins,
            "steps": len(orders), "rsum": np.array(rsum), "mse": np.array(mse), "mse_script": np.array(mse_script),
            "gaps": np.array(gaps), "min_gap": min(gaps)}


def trace(n_agents, temperature, steps, lr=0.1, act_rate=1.0, decay_rate=0.99, decay_gap=2000, seed=13, view=1):
    """main_MFQ_Ising.py (one episode) on RandomState(seed), as ising_oracle.mfq draws it."""
    rs = np.random.RandomState(seed)
    for _ in range(n_agents):                  # make_world -> reset_world
        rs.choice(2)
    spins = np.array([rs.choice(2) for _ in range(n_agents)], dtype=np.int64)   # env.reset()
    n_upd = int(act_rate * n_agents)
    return _run(spins, ising_oracle.neighbours(n_agents, view), steps, temperature, lr, decay_rate, decay_gap,
                lambda t: rs.random_sample(n_agents), lambda t: rs.choice(n_agents, n_upd, replace=False))


def trace_given(spins0, u, mask=None, view=1, *, temperature, lr=0.1, decay_rate=0.99, decay_gap=2000):
    """The same episode from supplied draws (ising_oracle.mfq_given's arguments)."""
    spins = np.asarray(spins0).astype(np.int64).reshape(-1)
    n = len(spins)
    u = np.asarray(u, dtype=np.float64).reshape(-1, n)
    ar = np.arange(n)
    if mask is None:
        grp = lambda t: ar                                                        # noqa: E731
    else:
        mask = np.asarray(mask, dtype=np.uint32).reshape(len(u), -1)
        grp = lambda t: np.nonzero((mask[t][ar >> 5] >> (ar & 31).astype(np.uint32)) & 1)[0]   # noqa: E731
    return _run(spins, ising_oracle.neighbours(n, view), len(u), temperature, lr, decay_rate, decay_gap,
                lambda t: u[t], grp)


def mc_uniform(seed, rep, sweep, i):
    """k_ising_mc's draw of replica rep, sweep `sweep`, site i: Philox counter (i, sweep, rep, MC_DOMAIN), key
    (seed, 0xA511E9B3), 53 bits of words 0 and 1 like ising_oracle.philox_uniform."""
    i, sweep, rep = np.broadcast_arrays(np.asarray(i, dtype=np.uint64), np.asarray(sweep, dtype=np.uint64),
                                        np.asarray(rep, dtype=np.uint64))
    w0, w1, _, _ = ising_oracle.philox((i, sweep, rep, np.uint64(MC_DOMAIN)), seed, 0xA511E9B3)
    bits = ((w0 >> np.uint64(5)) << np.uint64(26)) | (w1 >> np.uint64(6))
    return bits.astype(np.float64) * (1.0 / 9007199254740992.0)


def metropolis_table(temperature, K=4, coupling=1.0):
    """acc[a] = min(1, exp(-coupling (2 a - K) / temperature)), a = the neighbours equal to the site."""
    a = np.arange(K + 1, dtype=np.float64)
    with np.errstate(over="ignore"):
        return np.minimum(1.0, np.exp(-(coupling * (2.0 * a - K)) / temperature))


def metropolis(n_agents, sweeps, acc, seed=0, rep=0, spins0=None):
    """The checkerboard Metropolis chain of k_ising_mc for one replica: per sweep the sites of even row + column,
    then the odd ones; site i with `a` neighbours equal to it flips when mc_uniform(seed, rep, sweep, i) < acc[a].
    spins0 None: all up.  4 neighbours, even side."""
    L = int(round(n_agents ** 0.5))
    assert L * L == n_agents and L % 2 == 0 and L >= 4
    nbr = ising_oracle.neighbours(n_agents, 1)
    assert nbr.shape[1] == 4
    acc = np.asarray(acc, dtype=np.float64).reshape(5)
    s = np.ones(n_agents, np.int64) if spins0 is None else np.asarray(spins0).astype(np.int64).reshape(-1).copy()
    idx = np.arange(n_agents)
    parity = (idx // L + idx % L) & 1
    orders, nups = [], []
    for t in range(sweeps):
        u = mc_uniform(seed, rep, t, idx)
        for par in (0, 1):
            same = (s[nbr] == s[:, None]).sum(axis=1)
            flip = (parity == par) & (u < acc[same])
            s = np.where(flip, 1 - s, s)
        n_up = int(s.sum())
        nups.append(n_up)
        orders.append(abs(n_up - (n_agents - n_up)) / (n_agents + 0.0))
    return {"order": np.array(orders), "n_up": np.array(nups, dtype=np.int32), "spins": s.astype(np.uint8)}
