"""Test infrastructure: the shapes, networks, inputs and float64 references that tests/test_net_shapes_cpu.py and
tests/test_net_shapes_gpu.py share -- the four network paths off the Battle shape (view 13 x 13 x 7, F = 34, A = 21),
over the ranges include/magent_amd.h documents.

One batch size everywhere: N = 131 rows (two full 64-agent tiles and a 3-row tail).  Networks as the Battle-shape
tests build them (ACNet: default init + 0.02 randn; QNet: + 0.05 randn), on the CPU in float32, fixed seeds.  Inputs:
view = (rand < 0.3) * rand (dense rand for ACNet views of fewer than 16 floats), feat = rand, prob = Dirichlet(1).

The references are functions of (case) alone and cached, so every test of a case sees the same arrays; nobody writes
to them.

The sensitivity precondition (a condition on the float64 reference, checked on the CPU and again where the GPU tests
use it): zeroing one operand -- the view, the features, the mean action -- moves every output that operand feeds by at
least 1000 x the output's tolerance on the median row.  A kernel that ignores an operand (reads zeros for it) then misses
its bound on at least half the rows, by three orders of magnitude."""
import functools

import numpy as np

import acnet_ref
import qnet_bf16_ref as qb
import qnet_ref

N = 131
TOL = 1e-5                 # the policy, value / max(1, max |value|) and q / max(1, max |q|) bounds of the f32 kernels
SENSITIVITY = 1000.0

# ------------------------------------------------------------------------------------------------- ACNet: (V, F, A, use_mf)
_F_SWEEP = [(1, (True,)), (32, (True,)), (33, (True,)), (35, (False, True)), (36, (False, True)), (37, (False, True)),
            (40, (False, True)), (48, (True,)), (256, (False, True))]
ACNET_F_SWEEP = [(1188, F, 21, mf) for F, mfs in _F_SWEEP for mf in mfs]
ACNET_V_SWEEP = ([(V, 34, 21, True) for V in (1, 3, 16, 17, 47, 1184, 1192, 1196, 4096)] +
                 [(V, 40, 21, True) for V in (17, 1196)])
ACNET_A_SWEEP = [(1188, F, A, True) for F in (34, 40) for A in (2, 20, 32)]
ACNET_CASES = ACNET_F_SWEEP + ACNET_V_SWEEP + ACNET_A_SWEEP
ACNET_SUPPORT_CASES = [(1188, 34, 21, True), (1188, 40, 21, True)]

# ------------------------------------------------------------------------------------------------- Q-net: (F, A, use_mf)
_QNET_FA = [(1, 21), (4, 21), (33, 21), (37, 2), (256, 32), (34, 1), (34, 2), (34, 20), (34, 32)]
QNET_CASES = [(F, A, mf) for F, A in _QNET_FA for mf in (False, True)]
BF16_CASES = [(F, A, mf) for F, A in _QNET_FA if (F, A) not in ((4, 21), (34, 20)) for mf in (False, True)]
# (F, A, use_mf, seed): the seeds chosen on the CPU from the float64 restatement alone (test_net_shapes_cpu.py)
QTRAIN_CASES = [(37, 32, True, 11), (1, 2, True, 11), (256, 20, False, 11)]
QTRAIN_B = 20


def case_id(case):
    return "-".join(str(int(x)) for x in case)


def _seed(*case):
    """A fixed seed per case (no hash(): stable across processes)."""
    s = 17
    for x in case:
        s = (s * 1000003 + int(x)) % 2147483629
    return s


# ------------------------------------------------------------------------------------------------- ACNet
_SALT = {(1188, 34, 2, True): 2}          # added to the case's seeds (acnet_inputs)


def acnet(V, F, A, use_mf):
    """The case's torch ACNet on the CPU (float32): tests/test_policy_gpu.py::_acnet at another shape."""
    import torch
    from mfrl_amd.algo.nets import ACNet
    torch.manual_seed(_seed(V, F, A, use_mf) % 100000 + _SALT.get((V, F, A, bool(use_mf)), 0))
    net = ACNet((V,), (F,), A, use_mf=bool(use_mf))
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.02 * torch.randn_like(p))
    return net


def acnet_inputs(V, F, A, use_mf):
    """(view [N, V], feat [N, F], prob [N, A]) float32.  Where the stated inputs miss the sensitivity precondition
    (measured on the float64 reference, in tolerances on the median row) the input is scaled, never the factor:
    views of fewer than 16 floats are dense and x 4 (V = 1: 667 on the value), a single feature is x 4 (937 on the
    value), and the mean action is 8 x a Dirichlet(1) row (at unit mass the value head's 64 -> 32 branch, 32 of the
    544 inputs of its dense layer, moves the value by 260 .. 800 tolerances only).  With two actions the softmax at
    temperature 0.1 is nearly saturated (mean top probability 0.97), larger inputs only saturate it further, and
    (1188, 34, 2) takes the first later seed that meets the precondition instead (_SALT; the features moved the policy
    by 961 with the case's own seed and by 534 with the next)."""
    rng = np.random.RandomState(_seed(V, F, A, use_mf) % 100000 + 1 + _SALT.get((V, F, A, bool(use_mf)), 0))
    view = rng.rand(N, V)
    view = (rng.rand(N, V) < 0.3) * view if V >= 16 else 4.0 * view
    feat = rng.rand(N, F) * (4.0 if F == 1 else 1.0)
    prob = 8.0 * rng.dirichlet(np.ones(A), N)
    return view.astype(np.float32), feat.astype(np.float32), prob.astype(np.float32)


class ACRef:
    """net, the packed blob (float32 numpy) and its offsets, the inputs, and the float64 forward on the blob."""

    def __init__(self, V, F, A, use_mf):
        from mfrl_amd.policy import acnet_layout, pack_acnet
        self.case = (V, F, A, bool(use_mf))
        self.net = acnet(V, F, A, use_mf)
        self.layout = acnet_layout(V, F, A, use_mf)
        self.blob = pack_acnet(self.net, V, F, A, use_mf, self.layout).numpy()
        self.view, self.feat, self.prob = acnet_inputs(V, F, A, use_mf)
        self.policy, self.value = self.forward(self.view, self.feat, self.prob)
        self.vscale = max(1.0, float(np.abs(self.value).max()))

    def forward(self, view, feat, prob):
        V, F, A, mf = self.case
        return acnet_ref.forward(self.blob.astype(np.float64), self.layout[1], V, F, A, mf, view, feat, prob)

    def sensitivity(self):
        """{(operand, output): median over rows of the output's change when the operand is zeroed, in units of the
        output's tolerance} for every operand that feeds the output."""
        out = {}
        for name, args in (("view", (0 * self.view, self.feat, self.prob)), ("feat", (self.view, 0 * self.feat, self.prob)),
                           ("prob", (self.view, self.feat, 0 * self.prob))):
            p, v = self.forward(*args)
            if name != "prob":
                out[(name, "policy")] = float(np.median(np.abs(p - self.policy).max(1))) / TOL
            if name != "prob" or self.case[3]:
                out[(name, "value")] = float(np.median(np.abs(v - self.value))) / (TOL * self.vscale)
        return out


@functools.lru_cache(maxsize=None)
def acnet_case(V, F, A, use_mf):
    return ACRef(V, F, A, use_mf)


def support_mask(V, density=0.55, seed=3):
    return (np.random.RandomState(seed).rand(V) < density).astype(np.uint8)


def sparse_mask(V, every=20):
    """One supported input in every `every` floats: 16 packed inputs span more than 255 view floats."""
    m = np.zeros(V, dtype=np.uint8)
    m[::every] = 1
    return m


# ------------------------------------------------------------------------------------------------- Q-net
def qnet_inputs(F, A, use_mf, fixture_views=False):
    """(view [N, 13, 13, 7], feat [N, F], prob [N, A]) float32.  fixture_views (the bf16 cases): the first N fixture
    rows of qnet_bf16_ref.fixture_rows, with the fixture's features at F = 34 and its mean actions at A = 21."""
    rng = np.random.RandomState(_seed(F, A, use_mf) % 100000 + 2)
    view = ((rng.rand(N, 13, 13, 7) < 0.3) * rng.rand(N, 13, 13, 7)).astype(np.float32)
    feat = rng.rand(N, F).astype(np.float32)
    prob = rng.dirichlet(np.ones(A), N).astype(np.float32)
    if fixture_views:
        fv, ff, fp = qb.fixture_rows()
        view = fv[:N]
        if F == qb.F:
            feat = ff[:N]
        if A == qb.A:
            prob = fp[:N]
    return view, feat, prob


class QRef:
    """net (qnet_bf16_ref.net: Glorot + 0.05 randn), its blob, the inputs, the float64 forward; bf16: the quantised
    reference and its self-calibrating bound e_q too."""

    def __init__(self, F, A, use_mf, bf16=False):
        self.case = (F, A, bool(use_mf))
        self.net = qb.net(bool(use_mf), _seed(F, A, use_mf) % 100000, F, A)
        self.blob, self.off = qb.packed(self.net, use_mf, F, A)
        self.view, self.feat, self.prob = qnet_inputs(F, A, use_mf, fixture_views=bf16)
        self.q = self.forward(self.view, self.feat, self.prob)
        self.scale = max(1.0, float(np.abs(self.q).max()))
        if bf16:
            self.quant = qb.forward(self.blob, self.off, F, A, use_mf, self.view, self.feat, self.prob if use_mf else None)
            self.e_q = float(np.abs(self.quant - self.q).max())

    def forward(self, view, feat, prob):
        F, A, mf = self.case
        return qnet_ref.forward(self.blob.astype(np.float64), self.off, F, A, mf, view, feat, prob if mf else None)

    def sensitivity(self):
        """{operand: median over rows of max |q - q(operand zeroed)|} (absolute) for every operand the net reads."""
        out = {}
        for name, args in (("view", (0 * self.view, self.feat, self.prob)), ("feat", (self.view, 0 * self.feat, self.prob)),
                           ("prob", (self.view, self.feat, 0 * self.prob))):
            if name == "prob" and not self.case[2]:
                continue
            out[name] = float(np.median(np.abs(self.forward(*args) - self.q).max(1)))
        return out

    def sensitivity_bf16(self):
        """The same on the bf16 reference.  The bf16 bound is |q - reference| <= e_q: a kernel that ignores an operand
        computes the contract of the zeroed operand, so at best it lies within e_q of reference(zeroed) and misses
        the bound wherever |reference(zeroed) - reference| > 2 e_q."""
        F, A, mf = self.case
        out = {}
        for name, args in (("view", (0 * self.view, self.feat, self.prob)), ("feat", (self.view, 0 * self.feat, self.prob)),
                           ("prob", (self.view, self.feat, 0 * self.prob))):
            if name == "prob" and not mf:
                continue
            z = qb.forward(self.blob, self.off, F, A, mf, args[0], args[1], args[2] if mf else None)
            out[name] = float(np.median(np.abs(z - self.quant).max(1)))
        return out

    def clear(self, bound):
        """Rows whose float64 top-two gap exceeds bound (one action: every row)."""
        if self.q.shape[1] < 2:
            return np.ones(N, dtype=bool)
        s = np.sort(self.q, axis=1)
        return (s[:, -1] - s[:, -2]) > bound


@functools.lru_cache(maxsize=None)
def qnet_case(F, A, use_mf, bf16=False):
    return QRef(F, A, use_mf, bf16)


# ------------------------------------------------------------------------------------------------- the Boltzmann target
QTRAIN_SOFT_T = (1.0, 0.1)


def qtrain_soft_target64(eb64, tb64, off, F, A, use_mf, ring, n_ring, idx, gamma, T):
    """The float64 Boltzmann target (qtarget_ref.target64) of ring rows idx from the float64 forwards of both nets on
    the next rows: tests/test_qtarget_gpu.py's yardstick at another (F, A).  -> (y, eval Q, target Q of the next rows)."""
    import qtarget_ref as qt
    qt.check(A, T)
    nxt = (np.asarray(idx) + 1) % n_ring
    pn = ring["prob"][nxt] if use_mf else None
    q_e = qnet_ref.forward(eb64, off, F, A, use_mf, ring["obs"][nxt], ring["feat"][nxt], pn)
    q_t = qnet_ref.forward(tb64, off, F, A, use_mf, ring["obs"][nxt], ring["feat"][nxt], pn)
    return qt.target64(q_e, q_t, ring["rew"][idx], ring["term"][idx], gamma, T), q_e, q_t
