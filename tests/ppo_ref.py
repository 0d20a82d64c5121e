"""Test infrastructure: the PPO loss head of csrc/actrain_kernels.hip (k_at_loss_ppo; the contract is
mfx_actrain_set_ppo's in include/magent_amd.h) restated in float64 numpy on the logits and values actrain_ref.forward_keep
gives, and torch's gradient of the same loss over the whole network (gae_ref.torch_gradient's, with the clipped
surrogate as its policy term).

    lp = log(p_a + EPS);  d = lp - lp_old;  r = exp(d);  lo = f32(1 - clip);  hi = f32(1 + clip)
    clipped = (adv > 0 and r > hi) or (adv < 0 and r < lo)                    (strict: a row on the bound is not clipped)
    row policy loss  clipped: -adv (hi if adv > 0 else lo), a constant;  else -adv r
    dL/dp_a          gets -(adv r) / (p_a + EPS) / n unless clipped; everything else is actrain_ref's head
    clip_frac = mean(clipped);  approx_kl = mean((r - 1) - d)
"""
import numpy as np

import actrain_ref as ar


def bounds(clip):
    """(lo, hi) as the head forms them: float32 values of 1 - clip and 1 + clip."""
    return float(np.float32(1.0 - clip)), float(np.float32(1.0 + clip))


def logp(s, act):
    """lp[i] = log(clamp(s[i, act[i]]) + EPS) of softmax outputs s [n, A]."""
    p = np.clip(np.asarray(s, dtype=np.float64), ar.LO, ar.HI)
    return np.log(p[np.arange(len(p)), np.asarray(act).astype(np.int64)] + ar.EPS)


def ratio(s, act, lp_old):
    """(d, r) of the rows."""
    d = logp(s, act) - np.asarray(lp_old, dtype=np.float64)
    return d, np.exp(d)


def clipped_mask(adv, r, clip):
    lo, hi = bounds(clip)
    adv = np.asarray(adv, dtype=np.float64)
    return ((adv > 0) & (r > hi)) | ((adv < 0) & (r < lo))


def loss_terms(z, v, act, ret, adv, lp_old, clip, value_coef=ar.VALUE_COEF, ent_coef=ar.ENT_COEF):
    """The head's loss on logits z [n, A] and values v [n]: (pg, vf, ent) with their coefficients, as the stats have
    them.  adv and lp_old are constants of the loss."""
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    s = e / e.sum(1, keepdims=True)
    p = np.clip(s, ar.LO, ar.HI)
    lp = np.log(p + ar.EPS)
    adv, ret, v = (np.asarray(x, dtype=np.float64) for x in (adv, ret, v))
    d, r = ratio(s, act, lp_old)
    lo, hi = bounds(clip)
    cl = clipped_mask(adv, r, clip)
    row = np.where(cl, -adv * np.where(adv > 0, hi, lo), -adv * r)
    return (float(row.mean()), float(value_coef * np.mean((ret - v) ** 2)),
            float(ent_coef * np.mean(np.sum(p * lp, axis=1))))


def head(z, v, act, ret, adv, lp_old, clip, value_coef=ar.VALUE_COEF, ent_coef=ar.ENT_COEF):
    """-> dict: dz [n, A] = dL/dz and dv [n] = dL/dv of L = pg + vf + ent (means over the n rows), stats (pg, vf, ent,
    mean value), clip_frac, approx_kl, and the per-row lp, d, r, clipped."""
    z = np.asarray(z, dtype=np.float64)
    n = len(z)
    rows = np.arange(n)
    act = np.asarray(act).astype(np.int64)
    adv, ret, v = (np.asarray(x, dtype=np.float64) for x in (adv, ret, v))
    e = np.exp(z - z.max(1, keepdims=True))
    s = e / e.sum(1, keepdims=True)
    p = np.clip(s, ar.LO, ar.HI)
    lp = np.log(p + ar.EPS)
    d, r = ratio(s, act, lp_old)
    cl = clipped_mask(adv, r, clip)
    pg, vf, ent = loss_terms(z, v, act, ret, adv, lp_old, clip, value_coef, ent_coef)
    gp = ent_coef * (lp + p / (p + ar.EPS))
    gp[rows, act] += np.where(cl, 0.0, -(adv * r) / (p[rows, act] + ar.EPS))
    gp /= n
    gp[~((s >= ar.LO) & (s <= ar.HI))] = 0.0
    dz = s * (gp - np.sum(s * gp, axis=1, keepdims=True))
    return {"dz": dz, "dv": -2.0 * value_coef * (ret - v) / n, "stats": (pg, vf, ent, float(v.mean())),
            "clip_frac": float(cl.sum()) / n, "approx_kl": float(np.mean((r - 1.0) - d)), "lp": lp[rows, act], "d": d,
            "r": r, "clipped": cl}


def torch_gradient(net, rows, adv, logp_old, clip, dtype, device="cpu", value_coef=ar.VALUE_COEF, ent_coef=ar.ENT_COEF):
    """gae_ref.torch_gradient with the policy term the head's clipped surrogate, written with the explicit mask:
    (named gradients as float64 numpy, (pg, vf, ent, mean value), (clip_frac, approx_kl))."""
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
    a = t(adv)
    lp = torch.log(policy + ar.EPS)
    d = torch.sum(lp * mask, dim=1) - t(logp_old)
    r = torch.exp(d)
    lo, hi = bounds(clip)
    cl = ((a > 0) & (r > hi)) | ((a < 0) & (r < lo))
    bound = torch.where(a > 0, torch.full_like(r, hi), torch.full_like(r, lo))
    pg = -torch.mean(torch.where(cl, (a * bound).detach(), a * r))
    vf = value_coef * torch.mean(torch.square(ret - value))
    ent = ent_coef * torch.mean(torch.sum(policy * lp, dim=1))
    (pg + vf + ent).backward()
    named = {k: (q.grad.detach().double().cpu().numpy() if q.grad is not None else np.zeros(tuple(q.shape)))
             for k, q in m.named_parameters()}
    extra = (float(cl.double().mean()), float(((r - 1.0) - d).detach().double().mean()))
    return named, (float(pg.detach()), float(vf.detach()), float(ent.detach()), float(value.detach().mean())), extra
