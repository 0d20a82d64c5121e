"""k_rule_act (csrc/rule_kernels.hip) off the square view: the kernel's actions against the numpy restatement
(tests/rule_ref.py) by integer equality, at the view shapes and tables of tests/rule_cases.py.

What the shapes reach that 5 x 5, 13 x 13 and 15 x 15 never ran: VH != VW both ways (the kernel divides or multiplies
by VW in seven places); VF & 3 = 0, 1, 2 (the three tested sizes all leave a dword tail of 3); 256 cells, square and as
a 4 x 64 strip (four full ballot passes, the fourth attack word in use, cx = 32); one partial pass.  Two hand-made
tables sit at the ends of the contract's ranges: 64 moves of up to 16 cells with F = 2, and 57 actions with moves of up
to 4 cells.

tests/test_rule_cpu.py asserts, without a GPU, what makes these rows decisive: every branch is taken and a best move
is refused on each shape, the view read with VH and VW swapped gives other actions on at least 10 % of the rows, and
the hand-made tables' far moves and last actions are chosen."""
import numpy as np
import pytest
import torch

import rule_cases as rc
import rule_ref as rr

pytestmark = pytest.mark.gpu


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _check(key, shape, F, tab, view, feat):
    """n = 1, 63, 65, 1000 at eps = 0.2 (step n, group n % 2), then eps = 0 and eps = 1 on all rows: the restatement's
    actions, integer for integer."""
    from mfrl_amd.policy import RuleHIP
    v2a, base, n_action, move = tab
    hip = RuleHIP(shape + (7,), (F,), n_action, base, v2a, move)
    dv, df = _cuda(view), _cuda(feat)
    for n in rc.NS:
        got = hip.act(dv[:n], df[:n], eps=rc.EPS, seed=rc.SEED, step=n, group=n % 2)
        torch.cuda.synchronize()
        if n == 1000:
            want = rc.restated(key, view, feat, tab, step=n, group=n % 2)[0]
        else:
            want = rr.rule_actions(view[:n], feat[:n], v2a, base, n_action, move, rc.EPS, rc.SEED, n, n % 2)[0]
        got = got.cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, want), (key, n, int((got != want).sum()))
    for e, kind in ((0.0, False), (1.0, True)):
        got = hip.act(dv, df, eps=e, seed=rc.SEED, step=3).cpu().numpy()
        want, tag, _ = rr.rule_actions(view, feat, v2a, base, n_action, move, e, rc.SEED, 3, 0)
        assert np.array_equal(got, want) and ((tag == rr.TAG_RANDOM) == kind).all(), (key, e)
    return want


@pytest.mark.parametrize("shape", rc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_off_square_views_match_restatement(shape):
    view, feat = rc.shape_rows(shape)
    _check(shape, shape, 12, rc.tables(*shape), view, feat)


@pytest.mark.parametrize("name", sorted(rc.HAND_MADE))
def test_hand_made_tables_match_restatement(name):
    """The 4 x 64 strip with 64 moves (the move argmin over all 64 lanes, moves of 16 cells landing inside the view,
    the draw reaching action 63, F = 2: the feature row is x / W, y / H alone) and 16 x 16 with 57 actions."""
    shape, F, tab, (view, feat) = rc.hand_made(name)
    drawn = _check(name, shape, F, tab, view, feat)               # (the eps = 1 run: the uniform draw alone)
    assert drawn.max() == tab[2] - 1 and drawn.min() == 0
