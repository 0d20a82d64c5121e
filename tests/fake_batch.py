"""Test infrastructure: a stand-in for BattleBatch with exactly the members the act_rollout wrappers of
mfrl_amd.policy read (n_envs, rowcap, handles, rollout_buffer, mean_stride, stream_handle, torch_stream), backed by torch
tensors the test fills -- so that the row map (QRowMap, csrc/policy_act.h) runs at layouts no engine makes: G = 1 or 3,
counts past rowcap, a mean_stride wider than n_action.

Buffers, as the engine lays them out:
    view [E][rowcap][V], feature [E][rowcap][F] float32 per group   (every row filled, live or not: a kernel that acts
                                                                     on a dead row writes a real action over the sentinel)
    group_num [E][G] int32           drawn in [0, rowcap + 3]; per group one env has 0 and one has more than rowcap
    mean_action [E][G][stride] f64   Dirichlet(1) in the first A columns, NaN in the stride's other columns
    actions [E][G][rowcap] int32     SENTINEL everywhere"""
import numpy as np
import torch

SENTINEL = -7
LAYOUTS = [(65, 3, 5), (3, 1, 130), (7, 3, 64)]            # (E, G, rowcap); 65 envs: two 64-env chunks of the row list
EXTRA = 3                                                  # mean_stride = A + EXTRA


def layout_id(layout):
    return "E%d-G%d-rc%d" % layout


def counts(E, G, rowcap, seed):
    """group_num [E][G] int32 in [0, rowcap + 3]: per group g env g % E has no live row and env (g + 1) % E has
    rowcap + 1 + g % 3 (capped at rowcap by the row list); with more than two envs some other env is not full."""
    rng = np.random.RandomState(seed)
    c = rng.randint(0, rowcap + 4, size=(E, G)).astype(np.int32)
    for g in range(G):
        c[g % E, g] = 0
        c[(g + 1) % E, g] = rowcap + 1 + g % 3
        c[(g + 2) % E, g] = 1 + (rowcap - 1) // 2
    assert c.min() == 0 and c.max() <= rowcap + 3 and (c > rowcap).any(axis=0).all() and (c == 0).any(axis=0).all()
    return c


class FakeBatch:
    def __init__(self, layout, V, F, A, seed=0, rows=None):
        """rows: None -- views (rand < 0.3) * rand, features rand; or (view [n, V], feat [n, F]) numpy rows that the
        buffers cycle through, each group from another offset."""
        E, G, rc = layout
        self.n_envs, self.rowcap, self.handles = E, rc, list(range(G))
        self.G, self.V, self.F, self.A, self.stride = G, V, F, A, A + EXTRA
        rng = np.random.RandomState(seed)
        self.view_np, self.feat_np = [], []
        for g in range(G):
            if rows is None:
                v = ((rng.rand(E, rc, V) < 0.3) * rng.rand(E, rc, V)).astype(np.float32)
                f = rng.rand(E, rc, F).astype(np.float32)
            else:
                k = (np.arange(E * rc) + 331 * g) % len(rows[0])
                v = np.ascontiguousarray(rows[0].reshape(len(rows[0]), V)[k].reshape(E, rc, V), dtype=np.float32)
                f = np.ascontiguousarray(rows[1][k].reshape(E, rc, F), dtype=np.float32)
            self.view_np.append(v)
            self.feat_np.append(f)
        self.counts_np = counts(E, G, rc, seed + 1)
        mean = np.full((E, G, self.stride), np.nan)
        mean[:, :, :A] = rng.dirichlet(np.ones(A), size=(E, G))
        self.mean_np = mean
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        self.buf = {("view", g): dev(self.view_np[g]) for g in range(G)}
        self.buf.update({("feature", g): dev(self.feat_np[g]) for g in range(G)})
        self.buf[("group_num", 0)] = dev(self.counts_np)
        self.buf[("mean_action", 0)] = dev(mean)
        self.buf[("actions", 0)] = torch.full((E, G, rc), SENTINEL, dtype=torch.int32, device="cuda")

    # ---- what the wrappers read
    def rollout_buffer(self, name, group=0):
        return self.buf[(name, group)].data_ptr()

    def mean_stride(self):
        return self.stride

    def stream_handle(self):
        return torch.cuda.current_stream().cuda_stream

    def torch_stream(self):
        return torch.cuda.current_stream()

    # ---- what the tests read
    def live(self, g):
        """(e, j) int arrays of group g's live rows in the row list's order: env-major, j < min(count, rowcap)."""
        n = np.minimum(self.counts_np[:, g], self.rowcap)
        e = np.repeat(np.arange(self.n_envs), n)
        j = np.concatenate([np.arange(k) for k in n]) if n.sum() else np.zeros(0, np.int64)
        return e, j.astype(np.int64)

    def reset_actions(self):
        self.buf[("actions", 0)].fill_(SENTINEL)

    def actions(self):
        torch.cuda.synchronize()
        return self.buf[("actions", 0)].cpu().numpy()

    def expected(self, g, e, j, act):
        """The whole action buffer after one call for group g: `act` in the live slots, SENTINEL in every other slot --
        the other groups, the rows past each count, the rows past rowcap of a capped env."""
        want = np.full((self.n_envs, self.G, self.rowcap), SENTINEL, dtype=np.int32)
        want[e, g, j] = act
        return want
