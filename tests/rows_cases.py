"""The case tables of tests/test_rows_shapes_gpu.py (NumPy only, so tests/test_rows_ref_cpu.py can check on the CPU
every input condition a case depends on).  A column is (row bytes, byte offset of its buffer from an aligned base);
src and dst buffers carry one spare sentinel row at each end; the pointer a kernel sees is that of row 1."""
import numpy as np

SENT = 0xA5                     # destination fill (never zero: a stray store of zeros must show)
PIPE_MAX_DW = 64 * 4 * 5 + 3    # k_rows_pipe's limit per wide row, in dwords (csrc/replay_kernels.hip)
BIG_ROW = 512                   # columns at least this wide are "wide"


class Case:
    def __init__(self, name, cols, plan, n_src=300, n=257, idx="perm", src_mod=0, dst_start=0, dst_cap=0,
                 shift_mask=0, shift=0, pipes=("1", "0"), wide=None, seed=0):
        self.name, self.cols, self.plan = name, cols, plan
        self.n_src, self.n, self.src_mod = n_src, n, src_mod
        self.dst_start, self.dst_cap, self.shift_mask, self.shift = dst_start, dst_cap, shift_mask, shift
        self.pipes, self.wide, self.seed = pipes, wide, seed
        self.n_dst = dst_cap if dst_cap else dst_start + n
        rng = np.random.RandomState(1000 + seed + len(name))
        if isinstance(idx, str) and idx == "perm":          # distinct rows, a tenth of them numpy's negative indices
            idx = rng.permutation(n_src)[:n].astype(np.int64) if n <= n_src else rng.randint(0, n_src, n).astype(np.int64)
            if not src_mod:
                neg = rng.rand(n) < 0.1
                idx[neg] -= n_src
            else:
                idx = idx + src_mod * rng.randint(-3, 4, n)
        self.idx = None if idx is None else np.asarray(idx, dtype=np.int64)

    def __repr__(self):
        return self.name

    def expected_plan(self, pipe):
        """{form, nw, nu, units, cols} as replay.rows_plan reports it under MFX_ROWS_PIPE = pipe."""
        form, nw, nu, units, codes = self.plan
        if pipe == "0":
            form, nw, nu = 0, 0, 0
        return {"form": form, "nw": nw, "nu": nu, "units": units, "cols": list(codes)}

    def wide_path(self, k):
        """k_rows_copy's path of wide column k from the alignment of (row pointer | row bytes): 16, 4 or 1."""
        b, off = self.cols[k]
        a = (off + b) | b                   # row 1 of a buffer at `off` from a 16-B aligned base
        return 16 if a & 15 == 0 else 4 if a & 3 == 0 else 1

    def buffers(self):
        """(src, dst): per column a uint8 array [rows + 2, bytes] -- random source rows, sentinel-filled destination."""
        rng = np.random.RandomState(7 + self.seed)
        src = [rng.randint(0, 256, size=(self.n_src + 2, b), dtype=np.uint8) for b, _ in self.cols]
        dst = [np.full((self.n_dst + 2, b), SENT, dtype=np.uint8) for b, _ in self.cols]
        return src, dst

    def args(self):
        return dict(idx=self.idx, src_mod=self.src_mod, dst_start=self.dst_start, dst_cap=self.dst_cap, n=self.n,
                    shift_mask=self.shift_mask, shift=self.shift)


I32 = (4, 0)
ONE_WIDE = (1, 1, 1, 1, (2, 0))            # k_rows_pipe<1, 1>, one narrow dword unit
COPY_1W = (0, 0, 0, 1, (2, 0))


def _wide(b, off=0, plan=ONE_WIDE, path=None, **kw):
    return Case("wide_%d_at%d" % (b, off), [(b, off), I32], plan, wide=path, **kw)


WIDE_CASES = [
    _wide(512, path=16), _wide(528, path=16), _wide(528, 4, path=4), _wide(516, path=4),
    _wide(515, plan=COPY_1W, path=1), _wide(1027, plan=COPY_1W, path=1),
    _wide(1280, path=16), _wide(1284, path=4), _wide(1288, path=4), _wide(1292, path=4),
    _wide(5120, path=16, n_src=80, n=67), _wide(5132, path=4, n_src=80, n=67),
    _wide(5136, plan=COPY_1W, path=16, n_src=80, n=67), _wide(5124, 4, path=4, n_src=80, n=67),
    _wide(20480, plan=COPY_1W, path=16, n_src=40, n=33), _wide(20484, plan=COPY_1W, path=4, n_src=40, n=33),
    # (20,480 B is four full rounds of row_copy16, 20,484 B four full rounds of row_copy4 and one dword; these two
    # end in the middle of their second round)
    _wide(7696, plan=COPY_1W, path=16, n_src=40, n=33), _wide(7700, plan=COPY_1W, path=4, n_src=40, n=33),
]
COPY16_ROUND, COPY4_ROUND = 64 * 5 * 16, 64 * 20 * 4      # bytes one `base` round of row_copy16 / row_copy4 moves

NARROW_CASES = [
    Case("narrow_only", [(4, 0), (8, 0), (1, 0)], (1, 1, 1, 4, (0, 0, 1))),
    Case("narrow_1_2_3_6_7", [(1, 0), (2, 0), (3, 0), (6, 0), (7, 0)], (1, 1, 1, 19, (1, 1, 1, 1, 1))),
    Case("narrow_508", [(508, 0)], (1, 1, 2, 127, (0,))),
    Case("narrow_508_bytes", [(508, 1)], (0, 0, 0, 508, (1,))),
    Case("narrow_4_at1", [(4, 1), I32], (1, 1, 1, 5, (1, 0))),
    Case("units_64", [(256, 0)], (1, 1, 1, 64, (0,))),
    Case("units_65", [(256, 0), I32], (1, 1, 2, 65, (0, 0))),
    Case("units_128", [(508, 0), I32], (1, 1, 2, 128, (0, 0))),
    Case("units_129", [(508, 0), (8, 0)], (0, 0, 0, 129, (0, 0))),
    Case("narrow_wide_narrow", [(8, 0), (1028, 0), (12, 0)], (1, 1, 1, 5, (0, 2, 0))),
    Case("twelve_columns", [(4, 0), (1, 0), (8, 0), (516, 0), (2, 0), (16, 0), (3, 0), (4, 0), (12, 0), (1, 0), (4, 0),
                            (24, 0)], (1, 1, 1, 25, (0, 1, 0, 2, 1, 0, 1, 0, 0, 1, 0, 0))),
]

WIDE_COUNT_CASES = [
    Case("one_wide_100_units", [(1028, 0), (400, 0)], (1, 1, 2, 100, (2, 0))),
    Case("two_wide", [(516, 0), (1284, 0), I32], (1, 2, 1, 1, (2, 2, 0))),
    Case("two_wide_100_units", [(516, 0), (1284, 0), (400, 0)], (1, 2, 2, 100, (2, 2, 0))),
    Case("three_wide", [(516, 0), (520, 0), (524, 0), I32], (0, 0, 0, 1, (2, 2, 2, 0))),
    Case("two_wide_one_misaligned", [(516, 0), (517, 0), I32], (0, 0, 0, 1, (2, 2, 0))),
]

# ---- indices: two wide columns and three narrow ones; columns 3 and 4 are the shifted ones where a case shifts
ICOLS = [(516, 0), I32, (1, 0), (520, 0), (8, 0)]
IPLAN = (1, 2, 1, 4, (2, 0, 1, 2, 0))
SHIFTED = (1 << 3) | (1 << 4)


def _big_mod_idx(n, seed=5):
    rng = np.random.RandomState(seed)
    idx = rng.randint(1 << 32, 1 << 40, size=n, dtype=np.int64)
    idx[1::3] = -rng.randint(1, 1 << 40, size=len(idx[1::3]), dtype=np.int64)
    idx[0], idx[2] = (1 << 32), (1 << 40) - 1
    return idx


def _idx_cases():
    out = [Case("mod_big_indices", ICOLS, IPLAN, n_src=599, n=257, idx=_big_mod_idx(257), src_mod=599),
           Case("mod_below_src_rows", ICOLS, IPLAN, n_src=300, n=257, src_mod=123),
           Case("mod_1", ICOLS, IPLAN, n_src=300, n=50, src_mod=1)]
    mod = 250
    for sh in (0, -1, mod - 1, mod, mod + 3):
        out.append(Case("mod_shift_%d" % sh, ICOLS, IPLAN, n_src=300, n=257, src_mod=mod, shift_mask=SHIFTED, shift=sh,
                        seed=sh % 7))
    out.append(Case("mod_big_indices_shift_-1", ICOLS, IPLAN, n_src=599, n=257, idx=_big_mod_idx(257, 6), src_mod=599,
                    shift_mask=SHIFTED, shift=-1))
    # without a modulo the shifted index is idx + shift, then numpy's rule: -1 + 2 is row 1, 0 - 1 the last row
    n_src = 300
    rng = np.random.RandomState(11)
    up = np.concatenate([[-1, -2, -n_src, n_src - 3, 0], rng.randint(-n_src, n_src - 2, 200)]).astype(np.int64)
    down = np.concatenate([[0, -1, -n_src + 1, n_src - 1, 1], rng.randint(-n_src + 1, n_src, 200)]).astype(np.int64)
    out.append(Case("shift_+2_no_mod", ICOLS, IPLAN, n_src=n_src, n=len(up), idx=up, shift_mask=SHIFTED, shift=2))
    out.append(Case("shift_-1_no_mod", ICOLS, IPLAN, n_src=n_src, n=len(down), idx=down, shift_mask=SHIFTED, shift=-1))
    for n in (1, 3, 4, 5):
        out.append(Case("n_%d" % n, ICOLS, IPLAN, n_src=40, n=n, seed=n))
    out.append(Case("no_index_list", ICOLS, IPLAN, n_src=300, n=300, idx=None))
    return out


INDEX_CASES = _idx_cases()

RING_CASES = [
    Case("ring_wrap", ICOLS, IPLAN, dst_cap=300, dst_start=250),
    Case("ring_start_at_cap", ICOLS, IPLAN, dst_cap=300, dst_start=300),
    Case("ring_start_beyond_cap", ICOLS, IPLAN, dst_cap=300, dst_start=617),
    Case("ring_n_equals_cap", ICOLS, IPLAN, n_src=300, n=300, dst_cap=300, dst_start=5),
    Case("ring_ends_on_cap", ICOLS, IPLAN, dst_cap=300, dst_start=43),
]

SMALL_CASES = WIDE_CASES + NARROW_CASES + WIDE_COUNT_CASES + INDEX_CASES + RING_CASES

# ---- out-of-range rows: one bad index each, so "the first" is defined
OOB_CASES = [
    (Case("oob_wide_only", [(516, 0)], (1, 1, 1, 0, (2,)), n_src=64, n=6,
          idx=np.array([5, 63, 64, -64, 7, 0], dtype=np.int64)), 64),
    (Case("oob_narrow_only", [I32, (1, 0)], (1, 1, 1, 2, (0, 1)), n_src=64, n=6,
          idx=np.array([5, -1, 3, -65, 7, 0], dtype=np.int64)), -65),
]


def pipe_rows_per_round(cus, n_wide=1):
    """Rows one round of the pipelined form's persistent grid takes: (2 or 3 workgroups per CU) x 4 waves."""
    return cus * (2 if n_wide == 2 else 3) * 4


def big_grid_case(cus):
    """More rows than four rounds of the persistent grid (every wave refills both of its slots twice)."""
    n = 4 * pipe_rows_per_round(cus) + 7
    rng = np.random.RandomState(3)
    return Case("pipe_four_rounds", [(512, 0), I32], ONE_WIDE, n_src=600, n=n,
                idx=rng.randint(-600, 600, n).astype(np.int64), pipes=("1",))


COPY_GRID_ROWS = 65536 * 4      # rows one pass of k_rows_copy's largest grid takes


def stride_case():
    """One int32 column, 300,001 rows in reverse order: k_rows_copy's grid-stride loop."""
    n = 300001
    return Case("copy_grid_stride", [I32], (1, 1, 1, 1, (0,)), n_src=n, n=n, idx=np.arange(n - 1, -1, -1, dtype=np.int64),
                pipes=("0",))


# ------------------------------------------------------------------------------------------------- the collector
# (E, G, g, rowcap, V, F, A, mean_stride)
COLLECT_SHAPES = [(3, 1, 0, 5, 1, 1, 1, 1), (5, 3, 1, 7, 3, 64, 64, 64), (4, 2, 1, 9, 4, 33, 2, 24),
                  (2, 2, 0, 6, 255, 34, 21, 24), (2, 2, 0, 6, 1180, 34, 21, 24), (2, 2, 0, 6, 1181, 34, 21, 24),
                  (2, 2, 0, 6, 1182, 34, 21, 24), (2, 2, 0, 6, 1280, 34, 21, 24), (1, 2, 1, 3, 1283, 34, 21, 24)]
VIEW_MAX = 64 * 4 * 5 + 3       # floats of a view row k_collect_begin takes: 320 16-B units and a tail of 3 (5,132 B)
# View rows past that limit are refused, not collected: 5120 and 5123 floats (the limit's byte count read as floats)
COLLECT_TOO_WIDE = [(2, 2, 0, 6, 5120, 34, 21, 24), (1, 2, 1, 3, 5123, 34, 21, 24)]
EPISODES = (0, 3, 1 << 20)
COLLECT_NAMES = ("view", "feat", "actions", "rewards", "mean", "stats", "counts", "ids", "alive")


def collect_inputs(shape, seed=0, full=False, episodes=None):
    """Synthetic rollout buffers of one step: random counts (one env above rowcap, one empty where there are two),
    a random permutation of the G * rowcap ids per env, episode numbers 0, 3 and 2^20 in turn."""
    E, G, g, rowcap, V, F, A, ms = shape
    rng = np.random.RandomState(100 + seed)
    counts = rng.randint(0, rowcap + 4, size=(E, G)).astype(np.int32)
    counts[0, g] = rowcap + 2
    if E > 1:
        counts[1, g] = 0
    if full:
        counts[:] = rowcap
    stats = rng.rand(E, 4)
    stats[:, 0] = [EPISODES[e % 3] for e in range(E)] if episodes is None else episodes
    return {"view": rng.standard_normal((E, rowcap, V)).astype(np.float32),
            "feat": rng.standard_normal((E, rowcap, F)).astype(np.float32),
            "actions": rng.randint(0, A, size=(E, G, rowcap)).astype(np.int32),
            "rewards": rng.standard_normal((E, G, rowcap)).astype(np.float32),
            "mean": rng.rand(E, G, ms), "stats": stats, "counts": counts,
            "ids": np.stack([rng.permutation(G * rowcap).reshape(G, rowcap) for _ in range(E)]).astype(np.int32),
            "alive": (rng.rand(E, G, rowcap) < 0.7).astype(np.uint8)}


def begin_grid_waves(cus, shape):
    """Waves of k_collect_begin's grid (one row each per round): min(ceil(E * rowcap / 4), 3 per CU) workgroups x 4."""
    return min((shape[0] * shape[3] + 3) // 4, 3 * cus) * 4


def end_grid_lanes(cus, shape):
    """Lanes of k_collect_end's grid (one row each per pass): min(ceil(E * rowcap / 256), 8 per CU) workgroups x 256."""
    return min((shape[0] * shape[3] + 255) // 256, 8 * cus) * 256


LONG_BEGIN = (40, 1, 0, 200, 4, 1, 1, 1)       # 8,000 rows with full counts


def long_end_shape(cus):
    """E x rowcap just above 256 x 8 x CUs."""
    return (cus + 1, 1, 0, 2048, 4, 1, 1, 1)


def three_steps(shape, seed=40):
    """Three steps' inputs for one collector: new ids every step, env 1's episode number rises before the third step
    (so its `last` entries are stale), and in the second step one live id is id_stride and one is -1."""
    E, G, g, rowcap = shape[:4]
    episodes = [[EPISODES[e % 3] for e in range(E)] for _ in range(3)]
    episodes[2][1] += 1
    steps = [collect_inputs(shape, seed + t, episodes=episodes[t]) for t in range(3)]
    for s in steps:                             # every env live, so ids recur from step to step
        s["counts"][:, g] = np.maximum(s["counts"][:, g], rowcap - 2)
    steps[1]["ids"][0, g, 0] = G * rowcap
    steps[1]["ids"][2, g, 1] = -1
    return steps


# ------------------------------------------------------------------------------------------------- chains / returns
def chains(n_chains, seed=0, max_len=6, ones=False):
    """n_chains interleaved chains over step-major rows: (rew, prev, tails, values)."""
    rng = np.random.RandomState(200 + seed)
    lens = np.ones(n_chains, dtype=np.int64) if ones else rng.randint(1, max_len + 1, size=n_chains)
    lens[0] = 1
    owner = rng.permutation(np.repeat(np.arange(n_chains), lens))
    prev = np.full(len(owner), -1, dtype=np.int64)
    last = {}
    for r, c in enumerate(owner.tolist()):
        prev[r] = last.get(c, -1)
        last[c] = r
    tails = np.array([last[c] for c in range(n_chains)], dtype=np.int64)
    return (rng.standard_normal(len(owner)).astype(np.float32), prev, tails,
            rng.standard_normal(n_chains).astype(np.float32))


def episodes(n_ep, seed=0, max_len=6):
    """n_ep episodes, some of them empty (equal offsets) where there are more than two: (rewards, offsets, values)."""
    rng = np.random.RandomState(300 + seed)
    lens = rng.randint(0, max_len + 1, size=n_ep)
    lens[-1] = max_len                         # the last episode has rows: a launch that stops short of it shows
    if n_ep > 2:
        lens[0], lens[1], lens[n_ep // 2] = 0, 1, 0
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rng.standard_normal(int(offsets[-1])).astype(np.float32), offsets, rng.standard_normal(n_ep).astype(np.float32)


COUNTS = (1, 256, 257, 1000)
GAMMAS = (0.95, 1.0, 0.0)


# ------------------------------------------------------------------------------------------------- mean field
def mfq_rows(A):
    """Hand-built e_q rows of A entries (those that need more entries than A are left out): name -> row."""
    rows = {"all_equal": np.full(A, 0.25), "all_-inf": np.full(A, -np.inf), "max_last": np.arange(A, dtype=np.float64),
            "nan_first": np.r_[np.nan, np.arange(A - 1)], "nan_last": np.r_[np.arange(A - 1), np.nan]}
    if A >= 2:
        rows["two_nans"] = np.r_[np.nan, np.arange(A - 2, dtype=np.float64), np.nan]    # index 0 wins over the later one
        rows["-0_then_+0"] = np.r_[-0.0, 0.0, np.full(A - 2, -1.0)]
        rows["+0_then_-0"] = np.r_[0.0, -0.0, np.full(A - 2, -1.0)]
        rows["nan_after_inf"] = np.r_[np.full(A - 1, -2.0), np.nan]
        rows["nan_after_inf"][0] = np.inf
    if A >= 3:
        rows["two_nans_inside"] = np.r_[1.0, np.nan, np.full(A - 3, 5.0), np.nan]
    return {k: v.astype(np.float32) for k, v in rows.items()}


def mfq_inputs(M, A, seed=0):
    """(e_q, t_q, r, done bytes): random rows, the hand-built ones first (as many as fit, none of them done), then
    done bytes 0 / 1 / 2 / 255."""
    rng = np.random.RandomState(400 + seed + 7 * A + M)
    eq = rng.standard_normal((M, A)).astype(np.float32)
    for m, row in enumerate(list(mfq_rows(A).values())[:M]):
        eq[m] = row
    done = rng.choice(np.array([0, 0, 1, 2, 255], dtype=np.uint8), size=M)
    done[:len(mfq_rows(A))] = 0                # the hand-built rows are not done: their argmax reaches the target
    return eq, rng.standard_normal((M, A)).astype(np.float32), rng.standard_normal(M).astype(np.float32), done


def mean_action_inputs(n_action, rowcap, B=7, seed=0, over=False):
    """(acts [B + 1, rowcap], counts [B]): counts 0, 1 and rowcap first, then random; a fifth of the actions outside
    [0, n_action).  over: some counts in (rowcap, 2 rowcap] -- the spare row B keeps an uncapped reader in bounds."""
    rng = np.random.RandomState(500 + seed + n_action + rowcap)
    acts = rng.randint(0, n_action, size=(B + 1, rowcap)).astype(np.int32)
    wild = rng.rand(B + 1, rowcap) < 0.2
    acts[wild] = rng.choice(np.array([-1, -7, n_action, n_action + 5, 1 << 30], dtype=np.int32), size=int(wild.sum()))
    counts = rng.randint(0, rowcap + 1, size=B).astype(np.int32)
    counts[:3] = [0, 1, rowcap]
    if over:
        counts[3:6] = [rowcap + 1, 2 * rowcap, rowcap + (rowcap + 1) // 2]
    return acts, counts
