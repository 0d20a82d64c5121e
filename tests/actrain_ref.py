"""Test infrastructure: one training step of ActorCritic / MFAC (algo/ac.py; mfrl_amd.algo.ac.ActorCritic.losses)
restated in float64 numpy on the packed weight blob -- tests/acnet_ref.forward extended with kept activations, the
backward pass and Adam.  The contract of csrc/actrain_kernels.hip (include/magent_amd.h, mfx_actrain_*):

    forward:  acnet_ref.forward;  s = softmax(z), z = Wp (d / 0.1) + bp;  p = clamp(s, LO, HI);  lp = log(p + EPS)
    loss:     adv = ret - v (a constant);  L = -mean(adv lp[a]) + value_coef mean((ret - v)^2) + ent_coef mean(sum p lp)
    backward: dL/dv = -2 value_coef (ret - v) / n;  dL/dp_k = (-adv [k = a] / (p_a + EPS) + ent_coef (lp_k + p_k / (p_k +
              EPS))) / n where LO <= s_k <= HI, else 0 (torch's clamp backward);  dL/dz = s (dL/dp - sum_j s_j dL/dp_j)
    Adam:     torch defaults, bias-corrected by the step count t

LO, HI and EPS are the float32 values of 1e-10, 1 - 1e-10 (= 1) and 1e-6, as the f32 code on either side has them.
Gradients come back as a blob in the same layout, padding entries zero.  Also the inputs the actrain tests share."""
import functools

import numpy as np

import acnet_ref
import net_shapes as ns
import qnet_bf16_ref as qb

LO = float(np.float32(1e-10))
HI = float(np.float32(1.0) - np.float32(1e-10))          # 1.0
EPS = float(np.float32(1e-6))
BATTLE = (1183, 34, 21)
VALUE_COEF, ENT_COEF = 0.1, 0.08


def padding_mask(offsets, V, F, A, use_mf, n):
    """bool [n]: the blob's padding entries (K rows past V / F / A, policy columns past A, value columns 1..15, and
    whatever lies between a block's last entry and the next block)."""
    Vp, Fp, Ap = (V + 3) & ~3, (F + 3) & ~3, (A + 3) & ~3
    pad = np.ones(n, dtype=bool)

    def real(k, rows, cols, ld):
        m = np.zeros((rows if ld else 1, ld or cols), dtype=bool)
        if ld:
            m[:, :cols] = True
        else:
            m[:] = True
        o = offsets[k]
        pad[o:o + m.size] = ~m.reshape(-1)

    real(0, V, 256, 256); real(1, 1, 256, 0)
    real(2, F, 256, 256); real(3, 1, 256, 0)
    real(4, 512, 256, 256); real(5, 512, 256, 256); real(6, 1, 512, 0)
    real(7, 512, A, 32); real(8, 1, A, 0)
    if use_mf:
        real(11, A, 64, 64); real(12, 1, 64, 0)
        real(13, 64, 32, 32); real(14, 1, 32, 0)
        real(15, 544, 256, 256); real(16, 1, 256, 0)
        real(17, 256, 1, 16); real(18, 1, 1, 0)
    else:
        real(9, 512, 1, 16); real(10, 1, 1, 0)
    assert Vp >= V and Fp >= F and Ap >= A
    return pad


def forward_keep(blob, offsets, V, F, A, use_mf, view, feat, prob=None):
    """acnet_ref.forward with every activation kept: a dict."""
    W = acnet_ref.blocks(blob, offsets, V, F, A, use_mf)
    wv, bv, we, be, wd0, wd1, bd, wp, bp, wval, bval, wep, bep, wdp, bdp, wvd, bvd, wvo, bvo = W
    relu = lambda x: np.maximum(x, 0.0)
    x = np.asarray(view, dtype=np.float64).reshape(len(view), -1)
    n = x.shape[0]
    k = {"W": W}
    k["xv"] = xv = np.zeros((n, wv.shape[0]))
    xv[:, :V] = x
    k["f"] = f = np.zeros((n, we.shape[0]))
    f[:, :F] = feat
    k["concat"] = concat = np.concatenate([relu(xv @ wv + bv), relu(f @ we + be)], axis=1)
    k["d"] = d = relu(concat @ np.concatenate([wd0, wd1], axis=1) + bd)
    k["z"] = z = ((d / 0.1) @ wp + bp)[:, :A]
    e = np.exp(z - z.max(1, keepdims=True))
    k["s"] = s = e / e.sum(1, keepdims=True)
    k["p"] = np.clip(s, LO, HI)
    if use_mf:
        k["pp"] = pp = np.zeros((n, wep.shape[0]))
        pp[:, :A] = prob
        k["p1"] = p1 = relu(pp @ wep + bep)
        k["p2"] = p2 = relu(p1 @ wdp + bdp)
        k["cat"] = cat = np.concatenate([concat, p2], axis=1)
        k["vd"] = vd = relu(cat @ wvd + bvd)
        k["v"] = (vd @ wvo + bvo)[:, 0]
    else:
        k["v"] = (d @ wval + bval)[:, 0]
    return k


def gradient(blob, offsets, V, F, A, use_mf, rows, value_coef=VALUE_COEF, ent_coef=ENT_COEF):
    """-> (gradient blob float64, (pg_loss, vf_loss, ent_loss, mean value)).  rows: dict obs, feat, act, ret, prob."""
    blob = np.asarray(blob, dtype=np.float64)
    k = forward_keep(blob, offsets, V, F, A, use_mf, rows["obs"], rows["feat"], rows.get("prob"))
    wv, bv, we, be, wd0, wd1, bd, wp, bp, wval, bval, wep, bep, wdp, bdp, wvd, bvd, wvo, bvo = k["W"]
    act = np.asarray(rows["act"]).astype(np.int64)
    ret = np.asarray(rows["ret"], dtype=np.float64)
    n = len(act)
    ar = np.arange(n)
    s, p, v, d, concat = k["s"], k["p"], k["v"], k["d"], k["concat"]
    adv = ret - v
    lp = np.log(p + EPS)
    stats = (float(-np.mean(adv * lp[ar, act])), float(value_coef * np.mean((ret - v) ** 2)),
             float(ent_coef * np.mean(np.sum(p * lp, axis=1))), float(v.mean()))
    dv = -2.0 * value_coef * (ret - v) / n
    gp = ent_coef * (lp + p / (p + EPS))
    gp[ar, act] += -adv / (p[ar, act] + EPS)
    gp /= n
    gp[~((s >= LO) & (s <= HI))] = 0.0
    dz = s * (gp - np.sum(s * gp, axis=1, keepdims=True))
    g = np.zeros_like(blob)

    def put(kk, mat):
        mat = np.asarray(mat, dtype=np.float64)
        g[offsets[kk]:offsets[kk] + mat.size] = mat.reshape(-1)

    def cols(mat, width):
        full = np.zeros((mat.shape[0], width))
        full[:, :mat.shape[1]] = mat
        return full

    put(7, cols((d / 0.1).T @ dz, 32))
    put(8, dz.sum(0))
    dd = (dz @ wp[:, :A].T) / 0.1
    if not use_mf:
        dd = dd + dv[:, None] * wval[:, 0][None, :]
        put(9, cols((d.T @ dv)[:, None], 16))
        put(10, [dv.sum()])
    dd = dd * (d > 0)
    dcat = dd @ np.concatenate([wd0, wd1], axis=1).T
    if use_mf:
        vd, cat, p1, p2, pp = k["vd"], k["cat"], k["p1"], k["p2"], k["pp"]
        dvd = (vd > 0) * (dv[:, None] * wvo[:, 0][None, :])
        put(17, cols((vd.T @ dv)[:, None], 16))
        put(18, [dv.sum()])
        put(15, cat.T @ dvd)
        put(16, dvd.sum(0))
        dc2 = dvd @ wvd.T
        dcat = dcat + dc2[:, :512]
        dp2 = dc2[:, 512:] * (p2 > 0)
        put(13, p1.T @ dp2)
        put(14, dp2.sum(0))
        dp1 = (dp2 @ wdp.T) * (p1 > 0)
        put(11, pp.T @ dp1)
        put(12, dp1.sum(0))
    dcat = dcat * (concat > 0)
    put(4, concat.T @ dd[:, :256])
    put(5, concat.T @ dd[:, 256:])
    put(6, dd.sum(0))
    put(0, k["xv"].T @ dcat[:, :256])
    put(1, dcat[:, :256].sum(0))
    put(2, k["f"].T @ dcat[:, 256:])
    put(3, dcat[:, 256:].sum(0))
    return g, stats


def adam(p, m, v, g, t, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam's step number t (1-based), float64 -> (p, m, v)."""
    p, m, v, g = (np.asarray(x, dtype=np.float64) for x in (p, m, v, g))
    m2 = beta1 * m + (1.0 - beta1) * g
    v2 = beta2 * v + (1.0 - beta2) * g * g
    p2 = p - (lr / (1.0 - beta1 ** t)) * (m2 / (np.sqrt(v2) / np.sqrt(1.0 - beta2 ** t) + eps))
    return p2, m2, v2


def torch_gradient(net, rows, dtype, device="cpu", value_coef=VALUE_COEF, ent_coef=ENT_COEF):
    """torch autograd's gradient of ActorCritic.losses' formula (the clamp and the log with LO, HI, EPS) with the
    module cast to `dtype` on `device`: (named gradients as float64 numpy, (pg, vf, ent, mean value))."""
    import copy
    import torch
    import torch.nn.functional as Fn
    m = copy.deepcopy(net).to(device=device, dtype=dtype)
    t = lambda x, dt=dtype: torch.as_tensor(np.array(x), device=device).to(dt)
    view, feat, ret = t(rows["obs"]), t(rows["feat"]), t(rows["ret"])
    concat = torch.cat([Fn.relu(m.h_view(view.reshape(view.shape[0], -1))), Fn.relu(m.h_emb(feat))], dim=1)
    dense = Fn.relu(m.dense(concat))
    policy = torch.clamp(torch.softmax(m.policy(dense / 0.1), dim=1), LO, HI)
    if m.use_mf:
        p = Fn.relu(m.dense_prob(Fn.relu(m.emb_prob(t(rows["prob"])))))
        value = m.value(Fn.relu(m.value_dense(torch.cat([concat, p], dim=1)))).reshape(-1)
    else:
        value = m.value(dense).reshape(-1)
    mask = Fn.one_hot(t(rows["act"], torch.int64), policy.shape[1]).to(dtype)
    adv = (ret - value).detach()
    lp = torch.log(policy + EPS)
    pg = -torch.mean(adv * torch.sum(lp * mask, dim=1))
    vf = value_coef * torch.mean(torch.square(ret - value))
    ent = ent_coef * torch.mean(torch.sum(policy * lp, dim=1))
    (pg + vf + ent).backward()
    named = {k: (q.grad.detach().double().cpu().numpy() if q.grad is not None else np.zeros(tuple(q.shape)))
             for k, q in m.named_parameters()}
    return named, (float(pg.detach()), float(vf.detach()), float(ent.detach()), float(value.detach().mean()))


def pack64(named, V, F, A, use_mf, offsets, n):
    """pack_acnet's layout in float64 numpy from `named`: parameter name -> array in torch's parameter shape."""
    blob = np.zeros(n)

    def put(k, mat):
        mat = np.asarray(mat, dtype=np.float64)
        blob[offsets[k]:offsets[k] + mat.size] = mat.reshape(-1)

    def dense(k, name, rows=None, cols=None):
        w = named[name + ".weight"].T
        full = np.zeros((rows or w.shape[0], cols or w.shape[1]))
        full[:w.shape[0], :w.shape[1]] = w
        put(k, full)
        put(k + 1, named[name + ".bias"])

    dense(0, "h_view", rows=(V + 3) & ~3)
    dense(2, "h_emb", rows=(F + 3) & ~3)
    wd = named["dense.weight"].T
    put(4, wd[:, :256])
    put(5, wd[:, 256:])
    put(6, named["dense.bias"])
    dense(7, "policy", cols=32)
    if use_mf:
        dense(11, "emb_prob", rows=(A + 3) & ~3)
        dense(13, "dense_prob")
        dense(15, "value_dense")
        dense(17, "value", cols=16)
    else:
        dense(9, "value", cols=16)
    return blob


def block_errors(g, g64, offsets, n):
    """Per block: (max |g - g64| / max |g64|, max |g64|); an empty or all-zero block reports its absolute error."""
    ends = list(offsets[1:]) + [n]
    out = []
    for o, e in zip(offsets, ends):
        if e == o:
            out.append((0.0, 0.0))
            continue
        ref = np.abs(g64[o:e]).max()
        err = np.abs(np.asarray(g[o:e], dtype=np.float64) - g64[o:e]).max()
        out.append((float(err / ref) if ref > 0 else float(err), float(ref)))
    return out


def empty_blocks(use_mf):
    return range(9, 11) if use_mf else range(11, 19)


# ------------------------------------------------------------------------------------------------- shared inputs
POLICY_SCALE = 4.0            # the clamp-heavy case: the policy layer scaled up
# ... on 64 rows of seed 12: of the seeds 11..16 at 64 / 100 / 272 rows the first pair whose softmax keeps 1 % clear of
# the clamp's bound for both networks (measured on the float64 forward alone; tests/test_actrain_cpu.py asserts it)
CLAMP_SEED, CLAMP_N = 12, 64


@functools.lru_cache(maxsize=None)
def net(V, F, A, use_mf, seed=0, policy_scale=1.0):
    """net_shapes.acnet(V, F, A, use_mf) on the CPU; seed > 0 adds 0.02 randn from that seed once more (another net of
    the same shape); policy_scale multiplies the policy layer."""
    import torch
    m = ns.acnet(V, F, A, use_mf)
    with torch.no_grad():
        if seed:
            gen = torch.Generator().manual_seed(1000 + seed)
            for q in m.parameters():
                q.add_(0.02 * torch.randn(q.shape, generator=gen))
        if policy_scale != 1.0:
            m.policy.weight.mul_(policy_scale)
            m.policy.bias.mul_(policy_scale)
    return m


@functools.lru_cache(maxsize=None)
def rows(V, F, A, use_mf, seed, n):
    """n rows: at the Battle shape the fixture observation rows (qnet_bf16_ref.fixture_rows, 256 of them, rolled by
    7 seed and repeated past 256; the mean action 8 x the fixture's), elsewhere net_shapes.acnet_inputs' first n;
    returns 2.5 randn and actions uniform from RandomState(500 + seed), the first action 0 (seed even: the last row's
    when n = 1) and the last A - 1."""
    if (V, F, A) == BATTLE:
        fv, ff, fp = qb.fixture_rows()
        sel = (np.arange(n) + 7 * seed) % len(fv)
        obs, feat, prob = fv[sel].reshape(n, -1), ff[sel], 8.0 * fp[sel]
    else:
        view, feat, prob = ns.acnet_inputs(V, F, A, use_mf)
        assert n <= ns.N
        obs, feat, prob = view[:n], feat[:n], prob[:n]
    rng = np.random.RandomState(500 + seed)
    act = rng.randint(A, size=n).astype(np.int32)
    act[-1] = A - 1
    if n > 1 or seed % 2 == 0:
        act[0] = 0
    out = {"obs": np.ascontiguousarray(obs, dtype=np.float32), "feat": np.ascontiguousarray(feat, dtype=np.float32),
           "act": act, "ret": (2.5 * rng.randn(n)).astype(np.float32)}
    if use_mf:
        out["prob"] = np.ascontiguousarray(prob, dtype=np.float32)
    for x in out.values():
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def packed(V, F, A, use_mf, seed=0, policy_scale=1.0):
    """(blob float32 numpy, (n floats, offsets)) of net(...)."""
    from mfrl_amd.policy import acnet_layout, pack_acnet
    layout = acnet_layout(V, F, A, use_mf)
    blob = pack_acnet(net(V, F, A, use_mf, seed, policy_scale), V, F, A, use_mf, layout).numpy()
    blob.setflags(write=False)
    return blob, layout


@functools.lru_cache(maxsize=None)
def reference(V, F, A, use_mf, seed, n, policy_scale=1.0):
    """(g64, stats64, kept) of the case: computed once, shared, never written."""
    blob, (_, off) = packed(V, F, A, use_mf, seed, policy_scale)
    r = rows(V, F, A, use_mf, seed, n)
    g, stats = gradient(blob, off, V, F, A, use_mf, r)
    g.setflags(write=False)
    k = forward_keep(blob.astype(np.float64), off, V, F, A, use_mf, r["obs"], r["feat"], r.get("prob"))
    return g, stats, k


def clamp_margin(s):
    """min over entries of |s / LO - 1|: how far the softmax stays from the clamp's lower bound."""
    return float(np.abs(np.asarray(s) / LO - 1.0).min())
