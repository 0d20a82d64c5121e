"""Test infrastructure: the GAE(lambda) estimator of the device rollout loop (csrc/gae_kernels.hip; the contract is
mfx_chain_gae / mfx_adv_normalize in include/magent_amd.h) restated in numpy float64, one rounded operation per line as
the kernel has them; the synthetic forest the chain tests share; and torch's gradient of ActorCritic.losses' formula
with an advantage column (actrain_ref.torch_gradient's, with adv given instead of formed).

    nxt = V[t]; g = 0                                  t: the chain's tail row -- its value stands for the state after it
    per row r = t, prev[r], ... to -1:
        delta = (rew[r] + gamma * nxt) - V[r];  g = delta + (gamma * lambda) * g
        adv[r] = f32(g);  rew[r] = f32(g + V[r]);  nxt = V[r]
"""
import numpy as np

import actrain_ref as ar

FOREST_SEED, FOREST_ROWS = 23, 6384


def chain_gae(rew, prev, tails, values, gamma, lam, adv=None):
    """-> (rew float32, adv float32, bad): new arrays (adv starts as the given column, or zeros); bad = the first
    index that ended a walk (a tail outside [0, n), a predecessor that is neither -1 nor in [0, its row)), or None.
    A walk that meets one stops before touching anything more, as the kernel's does."""
    out = np.array(rew, dtype=np.float32)
    n = len(out)
    adv = np.zeros(n, np.float32) if adv is None else np.array(adv, dtype=np.float32)
    prev = np.asarray(prev, dtype=np.int64)
    V = np.asarray(values, dtype=np.float32)
    gamma = np.float64(gamma)
    gl = np.float64(gamma * np.float64(lam))
    bad = None
    for t in np.asarray(tails, dtype=np.int64).tolist():
        r, above, nxt, g, first = t, n, np.float64(0.0), np.float64(0.0), True
        while r != -1:
            if r < 0 or r >= above:
                bad = r if bad is None else bad
                break
            x, v = np.float64(out[r]), np.float64(V[r])
            if first:
                nxt, first = v, False
            t1 = np.float64(gamma * nxt)
            delta = np.float64(np.float64(x + t1) - v)
            g = np.float64(delta + np.float64(gl * g))
            adv[r] = np.float32(g)
            out[r] = np.float32(np.float64(g + v))
            nxt = v
            above, r = r, int(prev[r])
    return out, adv, bad


def adv_normalize(adv):
    """(adv - mean) / (std + 1e-8) in float64 (population deviation, two passes), as float64."""
    a = np.asarray(adv, dtype=np.float64)
    mean = a.sum() / len(a)
    std = np.sqrt(((a - mean) ** 2).sum() / len(a))
    return (a - mean) / (std + 1e-8)


def successors(prev, tails):
    """succ[r] = the row whose predecessor is r; a tail is its own successor."""
    prev = np.asarray(prev, dtype=np.int64)
    succ = np.full(len(prev), -1, np.int64)
    has = prev >= 0
    succ[prev[has]] = np.nonzero(has)[0]
    succ[np.asarray(tails, dtype=np.int64)] = tails
    assert (succ >= 0).all()
    return succ


def _forest(rng, lens):
    owner = np.repeat(np.arange(len(lens)), lens)
    rng.shuffle(owner)
    prev = np.full(len(owner), -1, np.int64)
    rows = [np.nonzero(owner == k)[0] for k in range(len(lens))]
    for r in rows:
        prev[r[1:]] = r[:-1]
    return prev, np.array([r[-1] for r in rows], np.int64), rows


_FOREST = {}


def forest(value_scale=1.0):
    """test_collect_ac_gpu.test_synthetic_forest's forest, drawn straight from seed 23 (the lengths, the interleaving,
    the rewards, the values, in that order): 300 interleaved chains of 1..40 rows plus one of 400 (more tails than a
    workgroup; a chain at the episode cap), 6,384 rows; one value per row, value_scale x randn.
    -> dict rew, prev, tails, rows (per chain, ascending), V; shared, read-only."""
    if value_scale in _FOREST:
        return _FOREST[value_scale]
    rng = np.random.default_rng(FOREST_SEED)
    lens = np.concatenate([rng.integers(1, 41, size=300), [400]])
    prev, tails, rows = _forest(rng, lens)
    rew = rng.standard_normal(len(prev)).astype(np.float32)
    V = (value_scale * rng.standard_normal(len(prev))).astype(np.float32)
    assert len(prev) == FOREST_ROWS and len(tails) == 301 > 256 and max(len(r) for r in rows) == 400
    assert min(len(r) for r in rows) == 1
    out = {"rew": rew, "prev": prev, "tails": tails, "rows": rows, "V": V}
    for k in ("rew", "prev", "tails", "V"):
        out[k].setflags(write=False)
    _FOREST[value_scale] = out
    return out


def _made(key, prev, tails, rows, rng, value_scale=1.0):
    out = {"rew": rng.standard_normal(len(prev)).astype(np.float32), "prev": prev, "tails": tails, "rows": rows,
           "V": (value_scale * rng.standard_normal(len(prev))).astype(np.float32)}
    for k in ("rew", "prev", "tails", "V"):
        out[k].setflags(write=False)
    _FOREST[key] = out
    return out


def short_forest(n_tails):
    """n_tails interleaved chains of 1..3 rows, every length present (256 tails: k_chain_gae's one full workgroup; 257:
    one lane in a second).  Shared, read-only."""
    key = ("short", n_tails)
    if key in _FOREST:
        return _FOREST[key]
    rng = np.random.default_rng(FOREST_SEED + n_tails)
    lens = rng.integers(1, 4, size=n_tails)
    prev, tails, rows = _forest(rng, lens)
    assert len(tails) == n_tails and set(lens.tolist()) == {1, 2, 3}
    return _made(key, prev, tails, rows, rng)


def long_chain(n=5000):
    """One chain over all n rows (prev[r] = r - 1), for the walk at gamma = lambda = 1.  Shared, read-only."""
    key = ("long", n)
    if key in _FOREST:
        return _FOREST[key]
    rng = np.random.default_rng(FOREST_SEED + n)
    prev = np.arange(-1, n - 1, dtype=np.int64)
    return _made(key, prev, np.array([n - 1], np.int64), [np.arange(n)], rng)


def torch_gradient(net, rows, adv, dtype, device="cpu", value_coef=ar.VALUE_COEF, ent_coef=ar.ENT_COEF):
    """actrain_ref.torch_gradient with the policy term's advantage taken from the column `adv` (None: ret - value,
    detached -- the default loss): (named gradients as float64 numpy, (pg, vf, ent, mean value))."""
    import copy
    import torch
    import torch.nn.functional as Fn
    m = copy.deepcopy(net).to(device=device, dtype=dtype)
    t = lambda x, dt=dtype: torch.as_tensor(np.array(x), device=device).to(dt)
    view, feat, ret = t(rows["obs"]), t(rows["feat"]), t(rows["ret"])
    concat = torch.cat([Fn.relu(m.h_view(view.reshape(view.shape[0], -1))), Fn.relu(m.h_emb(feat))], dim=1)
    dense = Fn.relu(m.dense(concat))
    policy = torch.clamp(torch.softmax(m.policy(dense / 0.1), dim=1), ar.LO, ar.HI)
    if m.use_mf:
        p = Fn.relu(m.dense_prob(Fn.relu(m.emb_prob(t(rows["prob"])))))
        value = m.value(Fn.relu(m.value_dense(torch.cat([concat, p], dim=1)))).reshape(-1)
    else:
        value = m.value(dense).reshape(-1)
    mask = Fn.one_hot(t(rows["act"], torch.int64), policy.shape[1]).to(dtype)
    a = (ret - value).detach() if adv is None else t(adv)
    lp = torch.log(policy + ar.EPS)
    pg = -torch.mean(a * torch.sum(lp * mask, dim=1))
    vf = value_coef * torch.mean(torch.square(ret - value))
    ent = ent_coef * torch.mean(torch.sum(policy * lp, dim=1))
    (pg + vf + ent).backward()
    named = {k: (q.grad.detach().double().cpu().numpy() if q.grad is not None else np.zeros(tuple(q.shape)))
             for k, q in m.named_parameters()}
    return named, (float(pg.detach()), float(vf.detach()), float(ent.detach()), float(value.detach().mean()))
