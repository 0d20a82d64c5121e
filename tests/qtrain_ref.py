"""Test infrastructure: one minibatch of ValueNet's training step (algo/base.py:192-279, algo/q_learning.py:42-54,
:110-131) restated in float64 numpy on the packed weight blob -- tests/qnet_ref.forward extended with kept
activations, the backward pass, Adam and the soft update.  The contract of csrc/qtrain_kernels.hip:

    next rows (idx + 1) % n:  q_t = target(next), q_e = eval(next), best = argmax q_e (first maximum),
                              y = r + ((1 - done) q_t[best]) gamma
    current rows idx:         d = y - q[a];  loss = sum d^2 m / sum m;  dL/dq[a] = -2 d m / sum m;  backward
    Adam (torch defaults, bias-corrected by the step count t), then target <- (1 - tau) target + tau eval_new

Gradients come back as a blob in the same layout, padding entries zero.  Also the inputs the qtrain tests share."""
import numpy as np

import qnet_bf16_ref as qb
import qnet_ref

F, A = qb.F, qb.A
N_RING, RING_ROWS = 200, 256


def padding_mask(offsets, F, A, use_mf, n):
    """bool [n]: the blob's padding entries (conv1's 64th K row, `we` rows past F, `wp1` rows past A, `wq` / `bq`
    columns past A)."""
    Fp, Ap = (F + 3) & ~3, (A + 3) & ~3
    pad = np.zeros(n, dtype=bool)
    pad[offsets[0] + 63 * 32:offsets[0] + 64 * 32] = True
    pad[offsets[6] + F * 32:offsets[6] + Fp * 32] = True
    pad[offsets[8] + A * 64:offsets[8] + Ap * 64] = True
    wq = np.zeros((64, 32), dtype=bool)
    wq[:, A:] = True
    pad[offsets[16]:offsets[16] + 64 * 32] = wq.reshape(-1)
    pad[offsets[17] + A:offsets[17] + 32] = True
    if not use_mf:                                   # the mean-field blocks of a DQN blob: unused, zero
        pad[offsets[8]:offsets[12]] = True
    return pad


def forward_keep(blob, offsets, F, A, use_mf, view, feat, prob=None):
    """qnet_ref.forward with every activation kept (float64)."""
    w1, b1, w2, b2, wd, bd, we, be, wp1, bp1, wp2, bp2, w2d, b2d, wo, bo, wq, bq = qnet_ref.blocks(blob, offsets, F, A, use_mf)
    relu = lambda x: np.maximum(x, 0.0)
    v = np.asarray(view, dtype=np.float64)
    n = v.shape[0]
    k = {}
    k["cols1"] = np.stack([v[:, ky:ky + 11, kx:kx + 11, :] for ky in range(3) for kx in range(3)], axis=3).reshape(n, 11, 11, 63)
    k["c1"] = relu(k["cols1"] @ w1[:63] + b1)
    k["cols2"] = np.stack([k["c1"][:, ky:ky + 9, kx:kx + 9, :] for ky in range(3) for kx in range(3)], axis=3).reshape(n, 9, 9, 288)
    k["c2"] = relu(k["cols2"] @ w2 + b2).reshape(n, 2592)
    k["hobs"] = relu(k["c2"] @ wd + bd)
    k["f"] = np.zeros((n, we.shape[0]))
    k["f"][:, :F] = feat
    k["hemb"] = relu(k["f"] @ we + be)
    h = [k["hobs"], k["hemb"]]
    if use_mf:
        k["p"] = np.zeros((n, wp1.shape[0]))
        k["p"][:, :A] = prob
        k["p1"] = relu(k["p"] @ wp1 + bp1)
        k["p2"] = relu(k["p1"] @ wp2 + bp2)
        h.append(k["p2"])
    k["cat"] = np.concatenate(h, axis=1)
    k["x2"] = relu(k["cat"] @ w2d + b2d)
    k["x3"] = relu(k["x2"] @ wo + bo)
    k["q"] = (k["x3"] @ wq + bq)[:, :A]
    return k


def targets(eval_blob, target_blob, offsets, F, A, use_mf, ring, n, idx, gamma):
    """y [B] (float64) of the minibatch at idx, and the eval net's next-state Q (for the argmax-gap precondition)."""
    nxt = (np.asarray(idx) + 1) % n
    pn = ring["prob"][nxt] if use_mf else None
    q_t = qnet_ref.forward(target_blob, offsets, F, A, use_mf, ring["obs"][nxt], ring["feat"][nxt], pn)
    q_e = qnet_ref.forward(eval_blob, offsets, F, A, use_mf, ring["obs"][nxt], ring["feat"][nxt], pn)
    best = np.argmax(q_e, axis=1)
    done = ring["term"][idx].astype(np.float64)
    y = ring["rew"][idx].astype(np.float64) + ((1.0 - done) * q_t[np.arange(len(idx)), best]) * gamma
    return y, q_e


def gradient(eval_blob, target_blob, offsets, F, A, use_mf, ring, n, idx, gamma, y=None):
    """(gradient blob float64, loss, mean q[a]) of the minibatch at idx over ring rows [0, n)."""
    idx = np.asarray(idx)
    blob = np.asarray(eval_blob, dtype=np.float64)
    if y is None:
        y, _ = targets(blob, np.asarray(target_blob, dtype=np.float64), offsets, F, A, use_mf, ring, n, idx, gamma)
    w1, b1, w2, b2, wd, bd, we, be, wp1, bp1, wp2, bp2, w2d, b2d, wo, bo, wq, bq = qnet_ref.blocks(blob, offsets, F, A, use_mf)
    B = len(idx)
    k = forward_keep(blob, offsets, F, A, use_mf, ring["obs"][idx], ring["feat"][idx], ring["prob"][idx] if use_mf else None)
    a = ring["act"][idx].astype(np.int64)
    m = ring["mask"][idx].astype(np.float64)
    qa = k["q"][np.arange(B), a]
    d = y - qa
    loss = float(np.sum(d * d * m) / np.sum(m))
    g = np.zeros_like(blob)
    gb = qnet_ref.blocks(g, offsets, F, A, use_mf)        # views into g
    dq = np.zeros((B, 32))
    dq[np.arange(B), a] = -2.0 * d * m / np.sum(m)
    gb[16][:] = k["x3"].T @ dq
    gb[17][:] = dq.sum(0)
    dx3 = (dq @ wq.T) * (k["x3"] > 0)
    gb[14][:] = k["x2"].T @ dx3
    gb[15][:] = dx3.sum(0)
    dx2 = (dx3 @ wo.T) * (k["x2"] > 0)
    gb[12][:] = k["cat"].T @ dx2
    gb[13][:] = dx2.sum(0)
    dcat = dx2 @ w2d.T
    dhobs = dcat[:, :256] * (k["hobs"] > 0)
    demb = dcat[:, 256:288] * (k["hemb"] > 0)
    gb[6][:F] = k["f"][:, :F].T @ demb
    gb[7][:] = demb.sum(0)
    if use_mf:
        dp2 = dcat[:, 288:] * (k["p2"] > 0)
        gb[10][:] = k["p1"].T @ dp2
        gb[11][:] = dp2.sum(0)
        dp1 = (dp2 @ wp2.T) * (k["p1"] > 0)
        gb[8][:A] = k["p"][:, :A].T @ dp1
        gb[9][:] = dp1.sum(0)
    gb[4][:] = k["c2"].T @ dhobs
    gb[5][:] = dhobs.sum(0)
    dc2 = ((dhobs @ wd.T) * (k["c2"] > 0)).reshape(B, 9, 9, 32)
    gb[2][:] = k["cols2"].reshape(-1, 288).T @ dc2.reshape(-1, 32)
    gb[3][:] = dc2.reshape(-1, 32).sum(0)
    dcols2 = (dc2 @ w2.T).reshape(B, 9, 9, 9, 32)
    dc1 = np.zeros((B, 11, 11, 32))
    for ky in range(3):
        for kx in range(3):
            dc1[:, ky:ky + 9, kx:kx + 9, :] += dcols2[:, :, :, ky * 3 + kx, :]
    dc1 *= k["c1"] > 0
    gb[0][:63] = k["cols1"].reshape(-1, 63).T @ dc1.reshape(-1, 32)
    gb[1][:] = dc1.reshape(-1, 32).sum(0)
    g[padding_mask(offsets, F, A, use_mf, g.size)] = 0.0      # (wq / bq columns past A: dq is zero there anyway)
    return g, loss, float(qa.mean())


def adam(p, tgt, m, v, g, t, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, tau=0.005):
    """torch.optim.Adam's step number t (1-based) and the soft update, float64 -> (p, target, m, v)."""
    p, tgt, m, v, g = (np.asarray(x, dtype=np.float64) for x in (p, tgt, m, v, g))
    m2 = beta1 * m + (1.0 - beta1) * g
    v2 = beta2 * v + (1.0 - beta2) * g * g
    step = lr / (1.0 - beta1 ** t)
    p2 = p - step * (m2 / (np.sqrt(v2) / np.sqrt(1.0 - beta2 ** t) + eps))
    return p2, (1.0 - tau) * tgt + tau * p2, m2, v2


# ------------------------------------------------------------------------------------------------- shared inputs
def ring(seed, F=F, A=A):
    """The ring the tests share: the 256 fixture rows, n = 200 live; columns from RandomState(100 + seed).  Other
    widths than the fixture's (F = 34, A = 21): the features uniform in [0, 1), the mean actions Dirichlet(1), from
    RandomState(200 + seed) -- the columns' stream stays the default shape's."""
    view, feat, prob = qb.fixture_rows()
    wide = np.random.RandomState(200 + seed)
    if F != qb.F:
        feat = wide.rand(RING_ROWS, F).astype(np.float32)
    if A != qb.A:
        prob = wide.dirichlet(np.ones(A), RING_ROWS).astype(np.float32)
    rng = np.random.RandomState(100 + seed)
    return {"obs": view, "feat": feat, "prob": prob,
            "act": rng.randint(A, size=RING_ROWS).astype(np.int32),
            "rew": (0.5 * rng.randn(RING_ROWS)).astype(np.float32),
            "term": rng.rand(RING_ROWS) < 0.1,
            "mask": rng.rand(RING_ROWS) < 0.8}


def index_list(seed, B, n=N_RING):
    """B indices from RandomState(300 + seed), forced to contain n - 1 (the wrap to row 0) and a repeated index."""
    idx = np.random.RandomState(300 + seed).randint(n, size=B).astype(np.int64)
    idx[0] = n - 1
    if B > 2:
        idx[2] = idx[1]
    return idx


def nets(use_mf, seed, F=F, A=A):
    """(eval, target) torch QNets on the CPU: qnet_bf16_ref.net(use_mf, seed) and net(use_mf, seed + 100)."""
    return qb.net(use_mf, seed, F, A), qb.net(use_mf, seed + 100, F, A)


def pack64(named, F, A, use_mf, offsets, n):
    """pack_qnet's layout in float64 numpy from `named`: parameter name -> array in torch's parameter shape (e.g.
    the gradients of a float64 module)."""
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

    w = np.zeros((64, 32))
    w[:63] = np.transpose(named["conv1.weight"], (2, 3, 1, 0)).reshape(-1, 32)
    put(0, w)
    put(1, named["conv1.bias"])
    put(2, np.transpose(named["conv2.weight"], (2, 3, 1, 0)).reshape(-1, 32))
    put(3, named["conv2.bias"])
    dense(4, "dense_obs")
    dense(6, "dense_emb", rows=(F + 3) & ~3)
    if use_mf:
        dense(8, "prob_emb", rows=(A + 3) & ~3)
        dense(10, "dense_act_prob")
    dense(12, "dense2")
    dense(14, "dense_out")
    dense(16, "q_value", cols=32)
    return blob


def torch_gradient(net, use_mf, ring, idx, y, dtype, device="cpu"):
    """torch autograd's gradient of the masked-MSE loss against the fixed targets y, as named arrays (float64 numpy),
    with the module cast to `dtype` on `device`; also (loss, mean q[a])."""
    import copy
    import torch
    m = copy.deepcopy(net).to(device=device, dtype=dtype)
    t = lambda x, dt=dtype: torch.as_tensor(np.asarray(x), device=device).to(dt)
    q = m(t(ring["obs"][idx]), t(ring["feat"][idx]), t(ring["prob"][idx]) if use_mf else None)
    qa = q.gather(1, t(ring["act"][idx], torch.int64).reshape(-1, 1)).reshape(-1)
    mask = t(ring["mask"][idx])
    loss = torch.sum(torch.square(t(y) - qa) * mask) / torch.sum(mask)
    loss.backward()
    named = {k: p.grad.detach().double().cpu().numpy() for k, p in m.named_parameters()}
    return named, float(loss.detach()), float(qa.detach().mean())


def block_errors(g, g64, offsets, n):
    """Per block: (max |g - g64| / max |g64|, max |g64|); blocks whose reference is all zero report 0 error when g is too."""
    ends = list(offsets[1:]) + [n]
    out = []
    for o, e in zip(offsets, ends):
        ref = np.abs(g64[o:e]).max()
        err = np.abs(np.asarray(g[o:e], dtype=np.float64) - g64[o:e]).max()
        out.append((float(err / ref) if ref > 0 else float(err), float(ref)))
    return out
