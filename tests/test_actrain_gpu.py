"""The HIP training step of the actor-critic network (csrc/actrain_kernels.hip, mfrl_amd.actrain.ACTrainHIP) on the GPU
against the float64 restatement tests/actrain_ref.py: gradient accuracy with torch's own f32 autograd as the yardstick,
the clamp-heavy inputs, shapes off Battle's, padding, one step = Adam on its own gradient, determinism, the input
support, the device guard, and the "hip" backend of ActorCritic / MFAC.

Inputs (actrain_ref): nets net_shapes.acnet + 0.02 randn of the seed, the fixture observation rows, returns 2.5 randn,
actions covering 0 and A - 1; tests/test_actrain_cpu.py asserts their preconditions on the float64 forward.

ACTRAIN_ERROR_OUT=<path>: the gradient tests append their measured figures per case there (profiles/actrain_error.jsonl
is such a run)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import actrain_ref as ar
import net_shapes as ns

pytestmark = pytest.mark.gpu

V, F, A = ar.BATTLE
LR = 1e-4
FLOOR = 1e-3                       # every non-empty block's max |g64| (measured on the CPU: test_actrain_cpu.py)
OFF_SHAPE = [(47, 37, 2, True), (1196, 1, 32, True), (4096, 256, 20, False), (17, 36, 21, False)]


def dev_rows(rows):
    """The rows as contiguous CUDA columns."""
    out = {}
    for k, x in rows.items():
        t = torch.as_tensor(np.array(x), device="cuda")
        out[k] = t.contiguous()
    return out


def handle(case, seed=0, scale=1.0, chunk_rows=None):
    from mfrl_amd import actrain
    Vc, Fc, Ac, mf = case
    tr = actrain.ACTrainHIP((Vc,), (Fc,), Ac, mf, lr=LR, value_coef=ar.VALUE_COEF, ent_coef=ar.ENT_COEF,
                            chunk_rows=chunk_rows)
    tr.set_state(actrain.PARAMS, torch.as_tensor(np.array(ar.packed(Vc, Fc, Ac, mf, seed, scale)[0])))
    return tr


def states(tr):
    """(parameters, m, v) as numpy float32."""
    return [tr.get_state(k).cpu().numpy() for k in range(3)]


def same_bits(a, b):
    if isinstance(a, (list, tuple)):
        return all(same_bits(x, y) for x, y in zip(a, b))
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def check_gradient(case, seed, n, scale=1.0, chunk_rows=None, tag=""):
    """Per block of the blob, e = max |g - g64| / max |g64| against the float64 restatement; torch's f32 autograd on
    the GPU over the same rows is the yardstick: e_hip <= 4 e_torch (another summation order of the same f32 products;
    a layout, transposition or masking mistake gives errors of order 1).  Every non-empty block's max |g64| >= 1e-3
    (measured on the CPU from the restatement: the smallest over all cases is 1.0e-3 .. 2e-3, the MF emb_prob weights),
    padding entries zero bits, the empty blocks empty, the stats within 1e-4 max(1, |x64|)."""
    Vc, Fc, Ac, mf = case
    g64, stats64, _ = ar.reference(Vc, Fc, Ac, mf, seed, n, scale)
    blob, (nb, off) = ar.packed(Vc, Fc, Ac, mf, seed, scale)
    rows = ar.rows(Vc, Fc, Ac, mf, seed, n)
    tr = handle(case, seed, scale, chunk_rows)
    before = states(tr)
    g, stats = tr.grads(dev_rows(rows), n)
    tr.check_error()
    assert same_bits(states(tr), before)                          # grads changes no state
    g, stats = g.cpu().numpy(), stats.cpu().numpy()
    named, t_stats = ar.torch_gradient(ar.net(Vc, Fc, Ac, mf, seed, scale), rows, torch.float32, "cuda")
    g_t = ar.pack64(named, Vc, Fc, Ac, mf, off, nb)
    e_hip, e_torch = ar.block_errors(g, g64, off, nb), ar.block_errors(g_t, g64, off, nb)
    rec = {"case": list(case), "seed": seed, "n": n, "chunk_rows": chunk_rows, "policy_scale": scale, "tag": tag,
           "e_hip": [e[0] for e in e_hip], "e_torch": [e[0] for e in e_torch], "max_g64": [e[1] for e in e_hip],
           "stats": [float(x) for x in stats], "stats64": list(stats64), "torch_stats": list(t_stats)}
    print(json.dumps(rec))
    if os.environ.get("ACTRAIN_ERROR_OUT"):
        with open(os.environ["ACTRAIN_ERROR_OUT"], "a") as f:
            f.write(json.dumps(rec) + "\n")
    pad = ar.padding_mask(off, Vc, Fc, Ac, mf, nb)
    assert np.all(g[pad].view(np.uint32) == 0)
    ends = list(off[1:]) + [nb]
    for k in range(19):
        if k in ar.empty_blocks(mf):
            assert ends[k] == off[k], k
            continue
        assert e_hip[k][1] >= FLOOR, (k, e_hip[k])
        assert e_hip[k][0] <= 4.0 * e_torch[k][0], (k, e_hip[k][0], e_torch[k][0])
    for x, x64 in zip(stats, stats64):
        assert abs(float(x) - x64) <= 1e-4 * max(1.0, abs(x64)), (stats, stats64)


# ------------------------------------------------------------------------------------------------- 1: gradient
@pytest.mark.parametrize("n,chunk", [(1, None), (20, None), (272, None), (272, 80)])
@pytest.mark.parametrize("seed", [11, 12])
@pytest.mark.parametrize("use_mf", [False, True])
def test_gradient_accuracy(use_mf, seed, n, chunk):
    """n = 272 at chunk_rows = 80: three full chunks and a 32-row tail -- the chunk-order accumulation."""
    check_gradient((V, F, A, use_mf), seed, n, chunk_rows=chunk)


@pytest.mark.parametrize("use_mf", [False, True])
def test_gradient_over_two_k_slices(use_mf):
    """700 rows in one chunk: the weight gradients' K dimension in two slices (512 rows and a 188-row tail)."""
    check_gradient((V, F, A, use_mf), 11, 700, tag="k-slices")


# ------------------------------------------------------------------------------------------------- 2: clamp-heavy
@pytest.mark.parametrize("use_mf", [False, True])
def test_gradient_with_clamped_policy(use_mf):
    """The policy layer x 4: between 10 % and 90 % of the softmax entries lie below 1e-10 and none within 1 % of it
    (test_actrain_cpu.py), so both sides of the clamp's mask carry entries."""
    check_gradient((V, F, A, use_mf), ar.CLAMP_SEED, ar.CLAMP_N, scale=ar.POLICY_SCALE, tag="clamp")


# ------------------------------------------------------------------------------------------------- 3: other shapes
@pytest.mark.parametrize("case", OFF_SHAPE, ids=ns.case_id)
def test_gradient_off_the_battle_shape(case):
    check_gradient(case, 11, 20, tag="shape")


# ------------------------------------------------------------------------------------------------- 4: padding
@pytest.mark.parametrize("use_mf", [False, True])
def test_padding_stays_zero(use_mf):
    case = (V, F, A, use_mf)
    tr = handle(case, 11)
    cols = dev_rows(ar.rows(V, F, A, use_mf, 11, 272))
    for _ in range(10):
        tr.step(cols, 272)
    tr.check_error()
    assert tr.step_count() == 10
    _, (nb, off) = ar.packed(V, F, A, use_mf, 11)
    pad = ar.padding_mask(off, V, F, A, use_mf, nb)
    for k, s in enumerate(states(tr)):
        assert np.all(s[pad].view(np.uint32) == 0), k
        assert np.any(s[~pad] != 0), k


# ------------------------------------------------------------------------------------------------- 5: one step
@pytest.mark.parametrize("use_mf", [False, True])
def test_step_is_adam_on_its_gradient(use_mf):
    """Ten consecutive steps; each: read the state, grads, step, read the state again.  The after-state must be the
    float64 restatement (actrain_ref.adam, step number t) applied to the before-state and that gradient, per element
    within test_qtrain_gpu.py's bounds: parameters 2^-23 |p| + lr 2^-16; m 2^-22 (|b1 m| + |(1 - b1) g|); v 2^-22 v."""
    tr = handle((V, F, A, use_mf), 12)
    cols = dev_rows(ar.rows(V, F, A, use_mf, 12, 272))
    start = states(tr)[0]
    for t in range(1, 11):
        before = states(tr)
        g, _ = tr.grads(cols, 272)
        g = g.cpu().numpy().astype(np.float64)
        assert same_bits(states(tr), before)
        tr.step(cols, 272)
        tr.check_error()
        assert tr.step_count() == t
        after = states(tr)
        p, m, v = ar.adam(*before, g, t, lr=LR)
        for name, got, want, bound in (
                ("p", after[0], p, 2.0 ** -23 * np.abs(p) + LR * 2.0 ** -16),
                ("m", after[1], m, 2.0 ** -22 * (np.abs(0.9 * before[1].astype(np.float64)) + np.abs(0.1 * g))),
                ("v", after[2], v, 2.0 ** -22 * v)):
            err = np.abs(got.astype(np.float64) - want)
            worst = int(np.argmax(err - bound))
            assert np.all(err <= bound), (t, name, worst, err[worst], bound[worst])
    assert np.abs(after[0] - start).max() > 5 * LR                # ten steps moved the weights


# ------------------------------------------------------------------------------------------------- 6: determinism
@pytest.mark.parametrize("use_mf", [False, True])
def test_bitwise_deterministic(use_mf):
    case = (V, F, A, use_mf)
    cols = dev_rows(ar.rows(V, F, A, use_mf, 11, 700))
    a, b = handle(case, 11, chunk_rows=300), handle(case, 11, chunk_rows=300)
    for _ in range(3):
        sa, sb = a.step(cols, 700), b.step(cols, 700)
    a.check_error()
    b.check_error()
    assert same_bits(sa.cpu().numpy(), sb.cpu().numpy()) and bool(torch.isfinite(sa).all())
    assert same_bits(states(a), states(b))
    # grads is the gradient step applies: from equal state, m after one step from zero moments is (1 - b1) g
    c = handle(case, 11, chunk_rows=300)
    g1 = c.grads(cols, 700)[0].cpu().numpy()
    g2 = c.grads(cols, 700)[0].cpu().numpy()
    assert same_bits(g1, g2)
    c.step(cols, 700)
    c.check_error()
    m = states(c)[1]
    want = (np.float32(1.0 - 0.9) * g1).astype(np.float32)       # fma(1 - b1, g - 0, 0): one rounded product
    assert same_bits(m, want)


# ------------------------------------------------------------------------------------------------- 7: input support
@pytest.mark.parametrize("use_mf", [False, True])
def test_input_support_is_bit_identical(use_mf):
    case = (V, F, A, use_mf)
    n = 272
    mask = ns.support_mask(V)
    rows = dict(ar.rows(V, F, A, use_mf, 11, n))
    rows["obs"] = rows["obs"] * mask[None, :].astype(np.float32)
    cols = dev_rows(rows)
    dense, sup = handle(case, 11), handle(case, 11)
    sup.set_input_support(mask)
    gd = dense.grads(cols, n)[0].cpu().numpy()
    gs = sup.grads(cols, n)[0].cpu().numpy()
    assert same_bits(gd, gs)
    _, (nb, off) = ar.packed(V, F, A, use_mf, 11)
    wv = gs[off[0]:off[0] + V * 256].reshape(V, 256)
    assert np.all(wv[mask == 0].view(np.uint32) == 0) and np.any(wv[mask == 1] != 0)
    for _ in range(2):
        dense.step(cols, n)
        sup.step(cols, n)
    dense.check_error()
    sup.check_error()
    assert same_bits(states(dense), states(sup))
    sup.set_input_support(None)                                   # back to the dense order: the same again
    assert same_bits(sup.grads(cols, n)[0].cpu().numpy(), dense.grads(cols, n)[0].cpu().numpy())


# ------------------------------------------------------------------------------------------------- 8: the guard
def test_guard():
    """One action equal to A: the kernel checks it before anything it selects, so nothing is read out of bounds; the
    step applies nothing."""
    from mfrl_amd import actrain
    case = (V, F, A, True)
    n = 272
    rows = ar.rows(V, F, A, True, 11, n)
    cols = dev_rows(rows)
    tr = handle(case, 11)
    tr.step(cols, n)
    tr.check_error()
    before = states(tr)
    for bad in (A, -3):
        bad_cols = dict(cols)
        bad_cols["act"] = cols["act"].clone()
        bad_cols["act"][100] = bad
        tr.step(bad_cols, n)
        assert tr.error() == (1, bad)
        assert tr.error() == (0, 0)                               # cleared
        assert tr.step_count() == 1 and same_bits(states(tr), before)
    bad_cols["act"][100] = A
    tr.step(bad_cols, n)
    with pytest.raises(actrain.ACTrainError):
        tr.check_error()
    assert tr.step_count() == 1 and same_bits(states(tr), before)
    with pytest.raises(ValueError):
        tr.step(cols, 0)
    tr.step(cols, n)                                              # the next clean step applies
    tr.check_error()
    assert tr.step_count() == 2 and not same_bits(states(tr)[0], before[0])


# ------------------------------------------------------------------------------------------------- 9: the backend
def _collect(algo, name):
    import test_collect_ac_gpu as tc
    model, _ = tc._model(algo, name)
    eng = tc._engine("few")
    col = model.rollout_collector(eng, 0)
    n = tc._scripted(eng, col)
    return model, n


@pytest.mark.parametrize("algo", ["ac", "mfac"])
def test_backend_gradient_of_train_rollout(algo):
    """The same collected rows ("few", 25 scripted steps) and the same weights under both backends:
    train_rollout(step=False) per parameter against the loss evaluated by torch in float64 on the batch()-ordered
    copy (test_collect_ac_gpu.py's reference), e_hip <= 4 e_torch."""
    import test_collect_ac_gpu as tc
    from mfrl_amd import mf
    use_mf = algo == "mfac"
    m_t, n = _collect(algo, algo + "-t")
    m_h, n_h = _collect(algo, algo + "-h")
    with torch.no_grad():
        for a, b in zip(m_h.net.parameters(), m_t.net.parameters()):
            a.copy_(b)
    assert n == n_h and n > 1000
    ct, ch = m_t.replay_buffer._rows.cols, m_h.replay_buffer._rows.cols
    assert all(torch.equal(ct[k][:n], ch[k][:n]) for k in ("obs", "feat", "act", "rew", "prev", "tail"))
    rows, counts = m_t.replay_buffer.batch()
    prob = rows.get("prob")
    last = torch.cumsum(counts, 0) - 1
    with torch.no_grad():
        _, keep, _ = m_t._hip_net().forward(rows["obs"][last], rows["feat"][last], prob[last] if use_mf else None,
                                            want_policy=False, want_value=True, want_act=False)
    offsets = torch.zeros(len(counts) + 1, dtype=torch.int64, device="cuda")
    offsets[1:] = torch.cumsum(counts, 0)
    ret = mf.mfac_returns(rows["rew"].clone(), offsets, keep.float().contiguous(), m_t.gamma)
    net32 = m_t.net
    m_t.net = copy.deepcopy(net32).double()
    try:
        total64 = sum(m_t.losses(rows["obs"].double(), rows["feat"].double(), rows["act"], ret.double(),
                                 prob.double() if use_mf else None)[:3])
        g64 = [g.detach().clone() for g in torch.autograd.grad(total64, list(m_t.net.parameters()))]
    finally:
        m_t.net = net32
    with pytest.raises(ValueError):
        m_h.train_backend = "cuda"
    m_h.train_backend = "hip"
    assert m_t.train_backend == "torch" and m_h.train_backend == "hip"
    before = [p.detach().clone() for p in m_h.net.parameters()]
    g_t = m_t.train_rollout(step=False)
    g_h = m_h.train_rollout(step=False)
    assert all(torch.equal(a, b) for a, b in zip(before, m_h.net.parameters()))
    assert m_h.replay_buffer._rows.n == 0
    e_h, e_t = tc._block_errors(g_h, g64), tc._block_errors(g_t, g64)
    names = [k for k, _ in m_h.net.named_parameters()]
    rec = {"algo": algo, "rows": n, "tag": "backend", "blocks": names, "e_hip": [e[0] for e in e_h],
           "e_torch": [e[0] for e in e_t], "max_g64": [e[1] for e in e_h]}
    print(json.dumps(rec))
    if os.environ.get("ACTRAIN_ERROR_OUT"):
        with open(os.environ["ACTRAIN_ERROR_OUT"], "a") as f:
            f.write(json.dumps(rec) + "\n")
    for k, name in enumerate(names):
        assert e_h[k][1] > 0, name
        assert e_h[k][0] <= 4.0 * e_t[k][0], (name, e_h[k][0], e_t[k][0])


@pytest.mark.parametrize("algo", ["mfac", "ac"])
def test_backend_trains(algo, capsys):
    """Two rounds of play_rollout_episodes(train=True) under "hip": the parameters moved and are finite, self.net is
    the handle's blob, and the acting handle holds the same weights without a re-pack; then train() on a
    batch()-ordered buffer."""
    import test_collect_ac_gpu as tc
    from mfrl_amd import actrain
    from mfrl_amd.algo import spawn_ai
    from mfrl_amd.algo.base import weights_key
    from mfrl_amd.algo.play import play_rollout_episodes
    from mfrl_amd.battle import BattleBatch
    from mfrl_amd.policy import pack_acnet
    map_size, E, max_steps = 40, 2, 10
    me, env = tc._model(algo, algo + "-0", max_steps)
    other = spawn_ai(algo, None, env, env.get_handles()[1], algo + "-1", max_steps)
    for m in (me, other):
        m.train_backend = "hip"
    eng = BattleBatch(map_size, E, stream=torch.cuda.current_stream())
    before = [p.detach().clone() for p in me.net.parameters()]
    opt_state = copy.deepcopy(me.optimizer.state_dict()["state"])
    for k in range(2):
        play_rollout_episodes(eng, k, map_size, max_steps, [me, other], eps=1.0, train=True, left_id=0)
        if k == 0:
            mid = [p.detach().clone() for p in me.net.parameters()]
    out = capsys.readouterr().out
    assert out.count("[*] PG_LOSS:") == 2 and "/ VF_LOSS:" in out and "/ ENT_LOSS:" in out and "/ VALUE:" in out
    after = list(me.net.parameters())
    assert all(bool(torch.isfinite(p).all()) for p in after)
    assert any(not torch.equal(a, b) for a, b in zip(mid, before))
    assert any(not torch.equal(a, b) for a, b in zip(after, mid))
    assert me._trainer.step_count() == 2 and me.optimizer.state_dict()["state"] == opt_state == {}
    blob = me._trainer.get_state(actrain.PARAMS)
    assert torch.equal(pack_acnet(me.net, me._trainer.V, me._trainer.F, me._trainer.A, me._use_mf), blob)
    key = weights_key(me.net)
    assert me._hip_key == key and me._trainer_key == key         # neither handle re-packs at its next use
    assert torch.equal(me._hip._blob, blob)
    # train() on pushed rows (batch() order) under the same backend
    from mfrl_amd.algo import tools
    rows = ar.rows(V, F, A, algo == "mfac", 11, 40)
    ids = np.arange(40) % 8
    snap = [p.detach().clone() for p in me.net.parameters()]
    me.replay_buffer = tools.EpisodesBuffer(use_mean=me._use_mf)
    me.flush_buffer(state=(rows["obs"].reshape(-1, 13, 13, 7), rows["feat"]), acts=rows["act"], rewards=rows["ret"],
                    alives=np.ones(40, dtype=bool), ids=ids, prob=rows.get("prob"))
    me.train()
    assert me._trainer.step_count() == 3
    assert any(not torch.equal(a.detach(), b) for a, b in zip(me.net.parameters(), snap))
    assert me._hip_key == weights_key(me.net)
    assert "[*] PG_LOSS:" in capsys.readouterr().out
