"""The GAE(lambda) mode of the actor-critic models on the GPU (csrc/gae_kernels.hip, the advantage column of
csrc/actrain_kernels.hip's loss head, ActorCritic.advantage = "gae").

The walk and the normalisation straight through the C ABI against tests/gae_ref.py -- the walk bitwise; the guards on
valid memory.  The loss head with an advantage column against torch in float64, torch's own f32 error as the yardstick
(tests/test_actrain_gpu.py's margin).  End to end on rows a linked collector left ("few" plan, 25 scripted steps):
train_rollout under "gae" on both backends, lambda = 1 against the default loss, and a model set to "gae" and back.
Driver: two rounds of play_rollout_episodes under "gae" + adv_norm.

ACTRAIN_ERROR_OUT=<path>: test_adv_normalize and the loss-head tests append their measured figures there
(profiles/gae_shapes_error.jsonl is such a run)."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest

import common
import gae_ref

pytestmark = pytest.mark.gpu
GAMMA = 0.95
LAMBDAS = [0.0, 0.5, 0.95, 1.0]
P = ctypes.c_void_p


def _abi():
    dll = ctypes.CDLL(common.HIP_LIB)
    dll.mfx_chain_gae.restype = ctypes.c_int
    dll.mfx_chain_gae.argtypes = [P] * 5 + [ctypes.c_int64, ctypes.c_int64, ctypes.c_double, ctypes.c_double, P]
    dll.mfx_adv_normalize.restype = ctypes.c_int
    dll.mfx_adv_normalize.argtypes = [P, ctypes.c_int64, P]
    dll.mfx_last_error.restype = ctypes.c_char_p
    return dll


def _gae_call(dll, rew, adv, prev, tails, V, lam, gamma=GAMMA):
    """-> (rc, rew, adv) after the call on device copies; every pointer is valid memory, empty arrays included."""
    import torch
    d = [torch.from_numpy(np.array(x)).cuda() for x in (rew, adv, prev, tails, V)]      # (copies: the forest is read-only)
    pad = torch.zeros(8, dtype=torch.int64, device="cuda")
    ptr = [P(t.data_ptr() if t.numel() else pad.data_ptr()) for t in d]
    rc = dll.mfx_chain_gae(*ptr, len(tails), len(rew), gamma, lam, P(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, d[0].cpu().numpy(), d[1].cpu().numpy()


# ------------------------------------------------------------------------------------------------- the walk
@pytest.mark.parametrize("lam", LAMBDAS)
def test_chain_gae_equals_the_restatement(lam):
    """Zero tails: nothing is written; one chain of one row; the forest (301 tails: two workgroups; a chain of 400);
    forests of exactly 256 and 257 tails with chains of 1..3 rows (one full workgroup; one lane in a second); at
    lambda = 1 one chain of 5000 rows with gamma = 1 (gl = 1: nothing decays over the whole walk)."""
    dll = _abi()
    rng = np.random.default_rng(29)
    rew = rng.standard_normal(5).astype(np.float32)
    sent = np.full(5, -7, np.float32)
    rc, out, adv = _gae_call(dll, rew, sent, np.full(5, -1, np.int64), np.zeros(0, np.int64),
                             rng.standard_normal(5).astype(np.float32), lam)
    assert rc == 0 and out.tobytes() == rew.tobytes() and adv.tobytes() == sent.tobytes()
    one = {"rew": np.array([0.75], np.float32), "prev": np.array([-1], np.int64), "tails": np.array([0], np.int64),
           "V": np.array([-1.25], np.float32)}
    cases = [(f, GAMMA) for f in (one, gae_ref.forest(1.0), gae_ref.forest(100.0), gae_ref.short_forest(256),
                                  gae_ref.short_forest(257))]
    if lam == 1.0:
        cases.append((gae_ref.long_chain(), 1.0))
    for f, gamma in cases:
        sent = np.full(len(f["rew"]), -7, np.float32)
        want_rew, want_adv, bad = gae_ref.chain_gae(f["rew"], f["prev"], f["tails"], f["V"], gamma, lam, adv=sent)
        assert bad is None
        rc, out, adv = _gae_call(dll, f["rew"], sent, f["prev"], f["tails"], f["V"], lam, gamma=gamma)
        assert rc == 0
        assert adv.tobytes() == want_adv.tobytes() and out.tobytes() == want_rew.tobytes(), len(f["rew"])
        assert (adv != -7).all()                               # every row of the forest is on a chain


@pytest.mark.parametrize("bad", [1000, -2, 7])
def test_a_prev_outside_the_rows_is_reported(bad):
    """test_collect_ac_gpu's cases, argument checks on valid memory: a predecessor outside the rows (1000 of 12; -2;
    7, which is not below its row 5) ends the walk there -- the rows walked before it hold their adv / rew, nothing is
    stored past it in either column, the call returns -1 with the index in its message -- and the next call is clean;
    then a tail outside the rows."""
    dll = _abi()
    prev = np.array([-1, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9], np.int64)      # two chains: even rows, odd rows
    tails = np.array([10, 11], np.int64)
    rew = np.arange(1, 13, dtype=np.float32)
    V = np.linspace(-1.0, 1.0, 12).astype(np.float32)
    sent = np.full(12, -7, np.float32)
    broken = prev.copy()
    broken[5] = bad                                                        # the odd chain: 11, 9, 7, 5 | 3, 1
    want_rew, want_adv, want_bad = gae_ref.chain_gae(rew, broken, tails, V, GAMMA, 0.95, adv=sent)
    assert want_bad == bad and (want_adv[[1, 3]] == -7).all() and (want_adv[[5, 7, 9, 11]] != -7).all()
    rc, out, adv = _gae_call(dll, rew, sent, broken, tails, V, 0.95)
    msg = dll.mfx_last_error()
    assert rc == -1 and b"chain_gae" in msg and str(bad).encode() in msg
    assert out.tobytes() == want_rew.tobytes() and adv.tobytes() == want_adv.tobytes()
    assert out[[1, 3]].tobytes() == rew[[1, 3]].tobytes() and adv[[1, 3]].tobytes() == sent[[1, 3]].tobytes()
    good_rew, good_adv, none = gae_ref.chain_gae(rew, prev, tails, V, GAMMA, 0.95, adv=sent)
    assert none is None
    rc, out, adv = _gae_call(dll, rew, sent, prev, tails, V, 0.95)         # the error word was cleared
    assert rc == 0 and out.tobytes() == good_rew.tobytes() and adv.tobytes() == good_adv.tobytes()
    t_bad = np.array([10, 12], np.int64)                                   # a tail outside the rows
    want_rew, want_adv, want_bad = gae_ref.chain_gae(rew, prev, t_bad, V, GAMMA, 0.95, adv=sent)
    rc, out, adv = _gae_call(dll, rew, sent, prev, t_bad, V, 0.95)
    assert rc == -1 and want_bad == 12 and b"12" in dll.mfx_last_error()
    assert out.tobytes() == want_rew.tobytes() and adv.tobytes() == want_adv.tobytes()
    assert (adv[1::2] == -7).all()
    rc, _, _ = _gae_call(dll, rew, sent, prev, tails, V, 0.95)
    assert rc == 0


@pytest.mark.parametrize("gamma,lam", [(1.5, 0.5), (-0.1, 0.5), (0.9, 1.01), (0.9, -1e-9), (float("nan"), 0.5),
                                       (0.9, float("nan"))])
def test_gamma_and_lambda_outside_0_1_are_refused_before_any_launch(gamma, lam):
    dll = _abi()
    f = gae_ref.forest(1.0)
    sent = np.full(len(f["rew"]), -7, np.float32)
    rc, out, adv = _gae_call(dll, f["rew"], sent, f["prev"], f["tails"], f["V"], lam, gamma=gamma)
    assert rc == -1 and b"[0, 1]" in dll.mfx_last_error()
    assert out.tobytes() == f["rew"].tobytes() and adv.tobytes() == sent.tobytes()


def test_the_wrapper_raises_index_error():
    import torch
    from mfrl_amd import replay
    prev = torch.tensor([-1, 0, 5], dtype=torch.int64, device="cuda")
    rew, adv, V = (torch.zeros(3, device="cuda") for _ in range(3))
    with pytest.raises(IndexError, match="chain_gae.* 5 "):
        replay.chain_gae(rew, adv, prev, torch.tensor([2], device="cuda"), V, 0.95, 0.95)
    prev[2] = 1
    r, a = replay.chain_gae(rew, adv, prev, torch.tensor([2], device="cuda"), V, 0.95, 0.95)
    assert r.data_ptr() == rew.data_ptr() and a.data_ptr() == adv.data_ptr()


# ------------------------------------------------------------------------------------------------- the normalisation
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001, 4096, 4097, 4194304, 4194305])
def test_adv_normalize(n):
    """Two calls on equal input: bitwise equal output; within one float32 spacing of the numpy float64 result (whose
    summation order is another: the difference before the rounding to float32 is of the order of n 2^-53); a constant
    column becomes zeros.  The partition's edges: 4096 is one part, 4097 two parts of 2049, 4194304 the full 1024 parts
    of 4096 and 4194305 the cap, 1024 parts of 4097 (n 2^-53 is 5e-10 there, still far inside one spacing).
    ACTRAIN_ERROR_OUT=<path>: the measured max err / spacing is appended there."""
    import torch
    dll = _abi()
    st = P(torch.cuda.current_stream().cuda_stream)
    a = (3.0 * np.random.default_rng(n).standard_normal(n) + 0.5).astype(np.float32)
    outs = []
    for _ in range(2):
        d = torch.from_numpy(a).cuda()
        assert dll.mfx_adv_normalize(P(d.data_ptr()), n, st) == 0
        outs.append(d.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    want = gae_ref.adv_normalize(a)
    w32 = want.astype(np.float32)
    err = np.abs(outs[0].astype(np.float64) - want)
    worst = float((err / np.spacing(np.abs(w32)).astype(np.float64)).max()) if n > 1 else 0.0
    print("n", n, "max err / spacing", worst)
    if os.environ.get("ACTRAIN_ERROR_OUT"):
        with open(os.environ["ACTRAIN_ERROR_OUT"], "a") as f:
            f.write(json.dumps({"tag": "adv_normalize", "n": n, "max_err_over_spacing": worst}) + "\n")
    assert (err <= np.spacing(np.abs(w32)).astype(np.float64)).all()
    if n > 1:
        assert abs(float(outs[0].astype(np.float64).mean())) < 1e-6 and abs(float(outs[0].astype(np.float64).std()) - 1) < 1e-5
    d = torch.full((n,), 2.5, dtype=torch.float32, device="cuda")
    assert dll.mfx_adv_normalize(P(d.data_ptr()), n, st) == 0
    assert not d.cpu().numpy().view(np.uint32).any()             # +0 exactly


# ------------------------------------------------------------------------------------------------- the loss head
def _loss_head(case, seed, n, chunk):
    """Per block of the blob e = max |g - g64| / max |g64| of ACTrainHIP.grads with an adv column against the same loss
    in torch float64; e_hip <= 4 e_torch, torch's own f32 gradient of that loss.  Then adv = None on the same handle:
    bitwise a fresh handle's default gradient.  ACTRAIN_ERROR_OUT=<path>: the figures are appended there."""
    import torch
    import actrain_ref as ar
    from test_actrain_gpu import dev_rows, handle, same_bits
    V, F, A, use_mf = case
    rows = ar.rows(V, F, A, use_mf, seed, n)
    adv = (2.5 * np.random.RandomState(77).randn(n)).astype(np.float32)
    _, (nb, off) = ar.packed(V, F, A, use_mf, seed)
    net = ar.net(V, F, A, use_mf, seed)
    named64, stats64 = gae_ref.torch_gradient(net, rows, adv, torch.float64, "cuda")
    named32, _ = gae_ref.torch_gradient(net, rows, adv, torch.float32, "cuda")
    g64, g32 = (ar.pack64(x, V, F, A, use_mf, off, nb) for x in (named64, named32))
    tr = handle(case, seed, chunk_rows=chunk)
    cols = dev_rows(rows)
    cols["adv"] = torch.from_numpy(adv).cuda()
    g, stats = tr.grads(cols, n)
    tr.check_error()
    g, stats = g.cpu().numpy(), stats.cpu().numpy()
    e_hip, e_torch = ar.block_errors(g, g64, off, nb), ar.block_errors(g32, g64, off, nb)
    rec = {"tag": "adv-column", "V": V, "F": F, "A": A, "use_mf": use_mf, "n": n, "e_hip": [e[0] for e in e_hip],
           "e_torch": [e[0] for e in e_torch], "stats": [float(x) for x in stats], "stats64": list(stats64),
           "max_ratio": max(e_hip[k][0] / e_torch[k][0] for k in range(19) if e_torch[k][0] > 0)}
    print(json.dumps(rec))
    if os.environ.get("ACTRAIN_ERROR_OUT"):
        with open(os.environ["ACTRAIN_ERROR_OUT"], "a") as f:
            f.write(json.dumps(rec) + "\n")
    pad = ar.padding_mask(off, V, F, A, use_mf, nb)
    assert np.all(g[pad].view(np.uint32) == 0)
    for k in range(19):
        if k in ar.empty_blocks(use_mf):
            continue
        assert e_hip[k][1] > 0, k
        assert e_hip[k][0] <= 4.0 * e_torch[k][0], (k, e_hip[k][0], e_torch[k][0])
    for x, x64 in zip(stats, stats64):
        assert abs(float(x) - x64) <= 1e-4 * max(1.0, abs(x64)), (stats, stats64)
    # the column changed the gradient, and None restores the default head bit for bit
    cols["adv"] = None
    g_back = tr.grads(cols, n)[0].cpu().numpy()
    g_fresh = handle(case, seed, chunk_rows=chunk).grads(dev_rows(rows), n)[0].cpu().numpy()
    assert same_bits(g_back, g_fresh) and not same_bits(g_back, g)


@pytest.mark.parametrize("use_mf", [False, True], ids=["ac", "mfac"])
def test_loss_head_with_an_advantage_column(use_mf):
    """ACTrainHIP.grads with an adv column at the Battle shape: 300 rows at chunk_rows = 128 -- three chunks, the last
    ragged (44 rows), so the column is read at each chunk's row offset and the stats add up over the workgroups of
    several k_at_loss launches; 300 rows are more than one workgroup's 256.  The checks are _loss_head's."""
    import actrain_ref as ar
    _loss_head(tuple(ar.BATTLE) + (use_mf,), 11, 300, 128)


@pytest.mark.parametrize("case", [(47, 37, 2, True), (4096, 256, 20, False)], ids=["47-37-2-mf", "4096-256-20"])
def test_loss_head_with_an_advantage_column_off_the_battle_shape(case):
    """The same at two of test_actrain_gpu.OFF_SHAPE's shapes, 20 rows (one chunk): two actions under a mean-field value
    head with h_emb in registers; the widest view and feature rows without one."""
    from test_actrain_gpu import OFF_SHAPE
    assert case in OFF_SHAPE
    _loss_head(case, 11, 20, None)


# ------------------------------------------------------------------------------------------------- end to end
_E2E = {}


class _Collected:
    """One model per algo with the rows of the "few" plan's 25 scripted steps left in its buffer, the reward column
    snapshotted; restore() puts the rows back as collected (train_rollout writes the reward column and empties the
    rows).  `base`: rew column and gradients of the model before it was ever set to "gae", per backend (torch twice)."""

    def __init__(self, algo):
        import test_collect_ac_gpu as tc
        self.tc = tc
        self.algo, self.use_mf = algo, algo == "mfac"
        self.model, _ = tc._model(algo, algo + "-gae")
        eng = tc._engine("few")
        col = self.model.rollout_collector(eng, 0)
        self.n = tc._scripted(eng, col)
        self.rows = self.model.replay_buffer._rows
        self.c = self.rows.cols
        self.snap = self.c["rew"][:self.n].clone()
        assert self.n > 1000 and int(self.c["tail"][:self.n].sum()) > 256
        self.base = {"torch": self.run("torch"), "torch2": self.run("torch"), "hip": self.run("hip")}

    def restore(self):
        self.c["rew"][:self.n].copy_(self.snap)
        self.rows.n = self.n

    def run(self, backend, chunk_rows=None):
        """-> (gradients, the reward column after the round preparation), rows restored afterwards."""
        self.restore()
        self.model.train_backend = backend
        g = self.model.train_rollout(chunk_rows=chunk_rows, step=False)
        rew = self.c["rew"][:self.n].clone()
        self.restore()
        return g, rew

    def losses64(self, ret, adv):
        """(g64, g32): the gradient of ActorCritic.losses on the collected rows in one piece, in float64 and in
        float32 (torch's own error: the yardstick), with `ret` as the reward column and `adv` (or None: the default)."""
        import torch
        m, c, n = self.model, self.c, self.n
        prob = c["prob"][:n] if self.use_mf else None
        net32 = m.net
        total = sum(m.losses(c["obs"][:n], c["feat"][:n], c["act"][:n], ret, prob, adv=adv)[:3])
        g32 = [g.detach().clone() for g in torch.autograd.grad(total, list(net32.parameters()))]
        m.net = copy.deepcopy(net32).double()
        try:
            total64 = sum(m.losses(c["obs"][:n].double(), c["feat"][:n].double(), c["act"][:n], ret.double(),
                                   prob.double() if self.use_mf else None,
                                   adv=adv.double() if adv is not None else None)[:3])
            g64 = [g.detach().clone() for g in torch.autograd.grad(total64, list(m.net.parameters()))]
        finally:
            m.net = net32
        return g64, g32

    def judge(self, g, g64, g32, tag):
        e, e_t = self.tc._block_errors(g, g64), self.tc._block_errors(g32, g64)
        names = [k for k, _ in self.model.net.named_parameters()]
        print(json.dumps({"algo": self.algo, "tag": tag, "rows": self.n, "blocks": names, "e": [x[0] for x in e],
                          "e_torch": [x[0] for x in e_t], "max_g64": [x[1] for x in e]}))
        for k, name in enumerate(names):
            assert e[k][1] > 0, name
            assert e[k][0] <= 4.0 * e_t[k][0], (tag, name, e[k][0], e_t[k][0])


def _collected(algo):
    if algo not in _E2E:
        _E2E[algo] = _Collected(algo)
    s = _E2E[algo]
    s.restore()
    m = s.model
    m._adv_norm, m._advantage, m._gae_lambda = False, "returns", 0.95
    return s


@pytest.mark.parametrize("algo", ["ac", "mfac"])
def test_train_rollout_under_gae(algo):
    """lambda = 0.95 on both backends: train_rollout(step=False) against float64 torch on the same adv / ret columns
    (the columns the round preparation left: the two backends get the same bits), e <= 4 e_torch.  The value column is
    the f32 forward's over all rows, the columns are gae_ref's walk of it, bit for bit."""
    import torch
    s = _collected(algo)
    m = s.model
    m.advantage = "gae"
    m.gae_lambda = 0.95
    got = {}
    for backend in ("torch", "hip"):
        g, ret = s.run(backend, chunk_rows=600 if backend == "hip" else None)
        got[backend] = (g, ret, m._gae_adv[:s.n].clone(), m._gae_value[:s.n].clone())
    (g_t, ret, adv, val), (g_h, ret_h, adv_h, val_h) = got["torch"], got["hip"]
    assert torch.equal(ret, ret_h) and torch.equal(adv, adv_h) and torch.equal(val, val_h)
    assert not torch.equal(ret, s.snap) and not torch.equal(ret, s.base["hip"][1])
    tails = np.nonzero(s.c["tail"][:s.n].cpu().numpy())[0]
    w_rew, w_adv, bad = gae_ref.chain_gae(s.snap.cpu().numpy(), s.c["prev"][:s.n].cpu().numpy(), tails,
                                          val.cpu().numpy(), m.gamma, 0.95)
    assert bad is None and ret.cpu().numpy().tobytes() == w_rew.tobytes() and adv.cpu().numpy().tobytes() == w_adv.tobytes()
    with torch.no_grad():
        c = s.c
        _, v_all, _ = m._hip_net().forward(c["obs"][:s.n], c["feat"][:s.n], c["prob"][:s.n] if s.use_mf else None,
                                           want_policy=False, want_value=True, want_act=False)
    assert torch.equal(v_all.reshape(-1), val)
    g64, g32 = s.losses64(ret, adv)
    s.judge(g_t, g64, g32, "gae-0.95-torch")
    s.judge(g_h, g64, g32, "gae-0.95-hip")
    # adv_norm: the column is normalised before either backend reads it
    m.adv_norm = True
    g_n, ret_n = s.run("hip", chunk_rows=600)
    adv_n = m._gae_adv[:s.n].clone()
    assert torch.equal(ret_n, ret)
    want = gae_ref.adv_normalize(adv.cpu().numpy())
    err = np.abs(adv_n.cpu().numpy().astype(np.float64) - want)
    assert (err <= np.spacing(np.abs(want.astype(np.float32))).astype(np.float64)).all()
    g64n, g32n = s.losses64(ret, adv_n)
    s.judge(g_n, g64n, g32n, "gae-0.95-norm-hip")


@pytest.mark.parametrize("algo", ["ac", "mfac"])
def test_lambda_1_reduces_to_the_default_loss(algo):
    """lambda = 1, adv_norm off, both backends: the gradient against the float64 gradient of the default "returns"
    loss on those rows and weights (the reward column the untouched model's round preparation left), e <= 4 e_torch
    with torch's f32 gradient of that default loss as the yardstick."""
    s = _collected(algo)
    m = s.model
    ret_def = s.base["hip"][1]
    g64, g32 = s.losses64(ret_def, None)
    m.advantage = "gae"
    m.gae_lambda = 1.0
    for backend in ("torch", "hip"):
        g, ret = s.run(backend, chunk_rows=600 if backend == "hip" else None)
        d = (ret.double() - ret_def.double()).abs().cpu().numpy()
        sp = np.spacing(np.abs(ret_def.cpu().numpy())).astype(np.float64)
        print("lambda 1, %s: %d of %d return rows differ, max %.3g spacings" % (backend, int((d > 0).sum()), s.n,
                                                                             float((d / sp).max())))
        assert (d <= sp).all()
        s.judge(g, g64, g32, "gae-1-" + backend)


@pytest.mark.parametrize("algo", ["ac", "mfac"])
def test_gae_and_back_leaves_no_trace(algo):
    """A model set to "gae" (with adv_norm, a round prepared and its gradient taken on both backends) and back to
    "returns": the reward column and the gradients are the untouched model's, bit for bit.  The HIP backend has one
    summation order, so its gradient is compared unconditionally; torch autograd's is compared when torch itself
    repeats its gradient bit for bit on these rows (two runs of the untouched model)."""
    import torch
    s = _collected(algo)
    m = s.model
    m.advantage = "gae"
    m.adv_norm = True
    for backend in ("torch", "hip"):
        s.run(backend)
    m.adv_norm = False
    m.advantage = "returns"
    assert torch.equal(s.base["torch"][1], s.base["hip"][1])
    for backend in ("torch", "hip"):
        g, ret = s.run(backend)
        g0, ret0 = s.base[backend]
        assert torch.equal(ret, ret0), backend
        same = all(torch.equal(a, b) for a, b in zip(g, g0))
        if backend == "hip":
            assert same
        else:
            repeats = all(torch.equal(a, b) for a, b in zip(s.base["torch"][0], s.base["torch2"][0]))
            print("torch repeats its own gradient bit for bit:", repeats)
            assert same or not repeats


# ------------------------------------------------------------------------------------------------- the driver
@pytest.mark.parametrize("backend", ["torch", "hip"])
@pytest.mark.parametrize("algo", ["mfac", "ac"])
def test_play_rollout_episodes_trains_under_gae(algo, backend, capsys):
    """Two rounds of play_rollout_episodes (40x40, 2 envs, 10 steps, train) under "gae" + adv_norm: the parameters
    moved and are finite, the rows are empty afterwards, round two runs on the same storage -- the buffer's columns
    and the model's value / advantage tensors."""
    import torch
    import test_collect_ac_gpu as tc
    from mfrl_amd.algo import spawn_ai
    from mfrl_amd.algo.play import play_rollout_episodes
    from mfrl_amd.battle import BattleBatch
    map_size, E, max_steps = 40, 2, 10
    me, env = tc._model(algo, algo + "-0", max_steps)
    other = spawn_ai(algo, None, env, env.get_handles()[1], algo + "-1", max_steps)
    for m in (me, other):
        m.train_backend = backend
        m.advantage = "gae"
        m.adv_norm = True
    eng = BattleBatch(map_size, E, stream=torch.cuda.current_stream())
    before = [p.detach().clone() for p in me.net.parameters()]
    buf = me.replay_buffer
    seen = []
    for k in range(2):
        play_rollout_episodes(eng, k, map_size, max_steps, [me, other], eps=1.0, train=True, left_id=0)
        assert me.replay_buffer is buf and buf._rows.n == 0
        seen.append((buf._rows.cap, {n: c.data_ptr() for n, c in buf._rows.cols.items()}, me._gae_value.data_ptr(),
                     me._gae_adv.data_ptr(), me._gae_value.numel()))
        if k == 0:
            mid = [p.detach().clone() for p in me.net.parameters()]
    assert seen[0][0] >= E * 64 * max_steps and seen[0][4] >= seen[0][0]
    assert seen[1] == seen[0]
    after = list(me.net.parameters())
    assert all(bool(torch.isfinite(p).all()) for p in after)
    assert any(not torch.equal(a, b) for a, b in zip(mid, before))
    assert any(not torch.equal(a, b) for a, b in zip(after, mid))
    assert capsys.readouterr().out.count("[*] PG_LOSS:") == 2              # models[0] trains, once per round
    n = me._rollout_collector.last_rows
    adv = me._gae_adv[:n].double()
    assert abs(float(adv.mean())) < 1e-5 and abs(float(adv.std(unbiased=False)) - 1.0) < 1e-4
