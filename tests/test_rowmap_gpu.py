"""The row map of a rollout batch (QRowMap, csrc/policy_act.h: row = rows[i], slot = (row / rowcap) * act_env +
act_off + row % rowcap, prob row = row / rowcap or the row itself) on made-up batches (tests/fake_batch.py), at the
layouts no engine makes: G = 1 and G = 3 (with G = 2, act_off = g * rowcap and (G - 1 - g) * rowcap differ only by
which group is written), counts past rowcap inside an acting call, a mean_stride wider than n_action with NaN in the
extra columns, 65 envs (two chunks of the row list), and, for the actor-critic and rule kernels, view shapes other than
13 x 13 x 7.

Every call is made for every group in turn on a buffer full of sentinels, and the whole action buffer is compared:
the expected action in the live slots of the group, the sentinel in every other slot.  Expected actions come from the
dense forms on the gathered live rows -- bit for bit, the equality the engine-based tests assert -- with the uniform of
row e * rowcap + j and group g."""
import copy

import numpy as np
import pytest
import torch

import acnet_ref
import fake_batch as fb
import net_shapes as ns
import qnet_bf16_ref as qb
import rule_cases as rc
import rule_ref as rr

pytestmark = pytest.mark.gpu
SEED, STEP, T = 4242, 9, 0.2


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _same(b, g, e, j, act, what):
    got, want = b.actions(), b.expected(g, e, j, act)
    live = np.zeros(got.shape, dtype=bool)
    live[e, g, j] = True
    assert np.array_equal(got[live], want[live]), (what, g, "live rows", int((got[live] != want[live]).sum()))
    assert np.array_equal(got, want), (what, g, "slots outside the group's live rows", np.argwhere(got != want)[:5].tolist())


# ------------------------------------------------------------------------------------------------- the Q network
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("FA", [(34, 21), (37, 32)], ids=lambda x: "F%d-A%d" % x)
@pytest.mark.parametrize("layout", fb.LAYOUTS, ids=fb.layout_id)
def test_qnet_act_rollout_on_a_made_up_batch(layout, FA, precision):
    """QNetHIP.act_rollout, mean field: greedy, temperature=, prob_rows= and both, against the dense forward on the
    gathered live rows with the env's mean cast to float32 (prob_rows: the row's own) and mf.q_sample on its Q values
    with rows e * rowcap + j, group g."""
    from mfrl_amd import mf
    from mfrl_amd.policy import QNetHIP
    F, A = FA
    E, G, rowcap = layout
    b = fb.FakeBatch(layout, 1183, F, A, seed=100 * F + E)
    hip = QNetHIP((13, 13, 7), (F,), A, True, precision=precision).load(qb.net(True, 7 + F, F, A).cuda())
    prob_rows = _dev(np.random.RandomState(5).dirichlet(np.ones(A), size=(E, rowcap)).astype(np.float32))
    mean32 = _dev(b.mean_np[:, :, :A]).float()
    seen, off = set(), 0
    for g in range(G):
        e, j = b.live(g)
        assert len(e) > 0
        te, tj = _dev(e), _dev(j)
        view, feat = b.buf[("view", g)][te, tj], b.buf[("feature", g)][te, tj]
        rows = _dev((e * rowcap + j).astype(np.int32))
        for by_row in (False, True):
            prob = prob_rows[te, tj] if by_row else mean32[te, g]
            q, greedy = hip.forward(view, feat, prob)
            drawn = mf.q_sample(q, T, SEED, STEP, group=g, rows=rows)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(q).all())
            for temperature, want in ((None, greedy), (T, drawn)):
                b.reset_actions()
                kw = {"prob_rows": prob_rows} if by_row else {}
                if temperature is not None:
                    kw.update(temperature=temperature, seed=SEED, step=STEP)
                hip.act_rollout(b, g, **kw)
                want = want.cpu().numpy()
                _same(b, g, e, j, want, ("qnet", layout, FA, precision, by_row, temperature))
                seen.update(want.tolist())
            off += int((drawn != greedy).sum())
    assert off > 0 and len(seen) > 1                               # (the draw is not the argmax everywhere)


# ------------------------------------------------------------------------------------------------- the actor-critic network
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("case", [(47, 37, 2, True), (1196, 40, 32, True), (1188, 34, 21, False)], ids=ns.case_id)
@pytest.mark.parametrize("layout", fb.LAYOUTS, ids=fb.layout_id)
def test_acnet_act_rollout_on_a_made_up_batch(layout, case, precision):
    """ACNetHIP.act_rollout(support=False) against acnet_ref.draw on the policy the dense forward returns for the
    gathered live rows (a row's policy does not depend on its place in the batch: tests/test_policy_gpu.py and
    tests/test_acnet_bf16_gpu.py assert that bitwise), rows e * rowcap + j, group g."""
    from mfrl_amd.policy import ACNetHIP
    V, F, A, use_mf = case
    E, G, rowcap = layout
    b = fb.FakeBatch(layout, V, F, A, seed=100 * F + E)
    hip = ACNetHIP((V,), (F,), A, use_mf, precision=precision).load(copy.deepcopy(ns.acnet(*case)).cuda())
    seen = set()
    for g in range(G):
        e, j = b.live(g)
        te, tj = _dev(e), _dev(j)
        pol = hip.forward(b.buf[("view", g)][te, tj], b.buf[("feature", g)][te, tj], want_act=False)[0]
        torch.cuda.synchronize()
        want = acnet_ref.draw(pol.cpu().numpy(), SEED, STEP, g, e * rowcap + j)
        b.reset_actions()
        hip.act_rollout(b, g, SEED, STEP, support=False)
        _same(b, g, e, j, want, ("acnet", layout, case, precision))
        seen.update(want.tolist())
    assert len(seen) > 1


# ------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("shape", [(9, 13), (16, 16)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("layout", fb.LAYOUTS, ids=fb.layout_id)
def test_rule_act_rollout_on_a_made_up_batch(layout, shape):
    """RuleHIP.act_rollout at two of tests/rule_cases.py's view shapes and their rows, eps = 0.2, against
    rule_ref.rule_actions with rows e * rowcap + j and group g."""
    from mfrl_amd.policy import RuleHIP
    E, G, rowcap = layout
    v2a, base, n_action, move = rc.tables(*shape)
    view, feat = rc.shape_rows(shape)
    V, F = shape[0] * shape[1] * 7, feat.shape[1]
    b = fb.FakeBatch(layout, V, F, n_action, seed=E, rows=(view, feat))
    hip = RuleHIP(shape + (7,), (F,), n_action, base, v2a, move)
    tags = np.zeros(5, dtype=np.int64)
    for g in range(G):
        e, j = b.live(g)
        want, tag, _ = rr.rule_actions(b.view_np[g][e, j].reshape(-1, shape[0], shape[1], 7), b.feat_np[g][e, j], v2a, base,
                                       n_action, move, rc.EPS, SEED, STEP, g, rows=e * rowcap + j)
        b.reset_actions()
        hip.act_rollout(b, g, eps=rc.EPS, seed=SEED, step=STEP)
        _same(b, g, e, j, want, ("rule", layout, shape))
        tags += np.bincount(tag, minlength=5)
    assert (tags >= 1).all(), tags
