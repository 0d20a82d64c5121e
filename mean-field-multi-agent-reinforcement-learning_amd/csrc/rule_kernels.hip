// rule_kernels.hip -- k_rule_act: the scripted rush / random opponent of the device rollout loop.  One
// action per observation row, computed from that row alone, so it runs wherever a learned policy does: on a compact
// batch of rows (the host loops) and on the live rows of a rollout batch (QRowMap, policy_act.h).  It is the project's
// own deterministic rule, not the reference's rush_prey_infer_action.
//
// CONTRACT (include/magent_amd.h; tests/rule_ref.py restates it in numpy).  Row: view [VH][VW][7] f32 (0 wall, 1 own
// group, 3 own minimap, 4 enemy, 6 enemy minimap; both minimaps carry +1 at the agent's own bin), feature [F] f32 whose
// last two entries are x / W, y / H.  cy = VH / 2, cx = VW / 2.  Comparisons on f32 as written, arithmetic integer.
//   A  attack       the first row-major cell with enemy > 0.5 and view2attack >= 0: attack_base + view2attack
//   B  in view      else, if a cell has enemy > 0.5: the one minimising (r - cy)^2 + (c - cx)^2, first row-major on
//                   ties; d = (c - cx, r - cy)
//   C  out of view  own bin: the first row-major cell with own minimap > 1.0; D = enemy minimap, minus 1.0f at the own
//                   bin; target: the first row-major cell among those of the largest D > 0.  With an own bin, a target
//                   and target != own bin, d = 64 (sign(c - bx), sign(r - by)); else
//                   d = 64 (sign(0.5f - fx), sign(0.5f - fy))
//   move            a < attack_base is free if move[a] == (0, 0), or if (cy + my, cx + mx) is inside the view with wall,
//                   own and enemy all <= 0.5; the free a minimising (dx - mx)^2 + (dy - my)^2, first index on ties
//                   (0 if none is free)
//   exploration     u1 = ac_uniform(seed, step, group, row); u1 < eps: min(int(u2 * n_action), n_action - 1) with
//                   u2 = ac_uniform(seed ^ 0x68E31DA4, step, group, row), one f32 multiply.  Such a row is not read.
//
// One wave per row, grid-stride over the compact row list.  The row (4,732 B at the Battle shape, dword aligned) is
// read once in 16-B units into the wave's LDS slab and the scans run from there: a ballot per 64-cell pass (A, the own
// bin), packed-key wave reductions (B, the density argmax, the move).  The branches are wave-uniform; lane 0 stores the
// action.  No atomics, no scratch; nothing is written but the action slot of a live row.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <new>

#include "mfx_common.h"
#include "policy_act.h"
#include "../../include/magent_amd.h"

namespace mfx {

constexpr int kRuleCh = 7;               // channels of the supported view
constexpr int kRuleMaxCells = 256;       // VH * VW
constexpr int kRuleMaxA = 64;            // actions (the move candidates sit on the lanes of one wave)
constexpr int kRuleWaves = 4;            // waves (rows in flight) per workgroup
constexpr int kRuleSlab = kRuleMaxCells * kRuleCh;          // floats of one wave's slab
constexpr int kRuleUnits = kRuleSlab / 4 / 64;              // 16-B units per lane of the largest row
constexpr uint32_t kRuleSeed2 = 0x68E31DA4u;
typedef uint32_t r32x4a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t r32x4 __attribute__((ext_vector_type(4)));

struct RuleTab {                         // a kernel argument: pure data, made on the host by mfx_rule_create
    int VH, VW, F, n_action, attack_base;
    unsigned long long atk[kRuleMaxCells / 64];              // bit c % 64 of word c / 64: cell c is attackable
    int8_t v2a[kRuleMaxCells];                               // view2attack per cell (-1: none)
    int8_t mdx[kRuleMaxA], mdy[kRuleMaxA];                   // move[a]
};

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = (unsigned long long)__shfl_xor((long long)v, o);
        v = w > v ? w : v;
    }
    return v;
}

__device__ __forceinline__ int rule_sign(int v) { return (v > 0) - (v < 0); }
__device__ __forceinline__ int rule_signf(float v) { return (v > 0.f) - (v < 0.f); }

// n: the upper bound of the row count, d_n: the count on the device (null: n).
__global__ void __launch_bounds__(64 * kRuleWaves) k_rule_act(RuleTab t, const float* __restrict__ view,
                                                              const float* __restrict__ feat, QRowMap rm, int n,
                                                              const int32_t* __restrict__ d_n, float eps, uint32_t seed,
                                                              uint32_t step, int group, int32_t* __restrict__ act) {
    __shared__ __attribute__((aligned(16))) float slabs[kRuleWaves][kRuleSlab];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float* slab = slabs[wid];
    const int count = d_n ? min(*d_n, n) : n;
    const int cells = t.VH * t.VW, VF = cells * kRuleCh;
    const int nq = VF >> 2, nt = VF & 3, passes = (cells + 63) >> 6;
    const int cy = t.VH / 2, cx = t.VW / 2;
    const int W = (int)gridDim.x * kRuleWaves;
    for (int i = (int)blockIdx.x * kRuleWaves + wid; i < count; i += W) {
        const int row = rm.row(i);                           // wave-uniform
        int action;
        if (ac_uniform(seed, step, group, row) < eps) {      // exploration: the row is not read
            const float u2 = ac_uniform(seed ^ kRuleSeed2, step, group, row);
            action = min((int)(u2 * (float)t.n_action), t.n_action - 1);
        } else {
            // the row into the slab, 16-B units at the row's dword alignment
            const uint32_t* vp = reinterpret_cast<const uint32_t*>(view + (size_t)row * VF);
#pragma unroll
            for (int u = 0; u < kRuleUnits; ++u) {
                const int q = lane + 64 * u;
                if (q < nq) reinterpret_cast<r32x4*>(slab)[q] = reinterpret_cast<const r32x4a4*>(vp)[q];
            }
            if (lane < nt) reinterpret_cast<uint32_t*>(slab)[4 * nq + lane] = vp[4 * nq + lane];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the wave's LDS operations keep this order
            // A: the first attackable cell holding an enemy;  B: the nearest enemy cell
            action = -1;
            bool any = false;
            uint32_t near = 0xFFFFFFFFu;
            for (int p = 0; p < passes; ++p) {
                const int c = 64 * p + lane;
                const bool e = c < cells && slab[c * kRuleCh + 4] > 0.5f;
                const unsigned long long em = __ballot(e);
                if (em & t.atk[p]) {
                    action = t.attack_base + t.v2a[64 * p + __builtin_ctzll(em & t.atk[p])];
                    break;
                }
                any = any || em != 0;
                if (e) {
                    const int r = c / t.VW, dy = r - cy, dx = c - r * t.VW - cx;
                    near = min(near, ((uint32_t)(dx * dx + dy * dy) << 8) | (uint32_t)c);
                }
            }
            if (action < 0) {
                int dx, dy;
                if (any) {
                    const int c = (int)(wave_min_u32(near) & 0xFFu), r = c / t.VW;
                    dx = c - r * t.VW - cx;
                    dy = r - cy;
                } else {
                    // C: the own bin, then the densest enemy bin
                    int own = -1;
                    for (int p = 0; p < passes && own < 0; ++p) {
                        const int c = 64 * p + lane;
                        const unsigned long long om = __ballot(c < cells && slab[c * kRuleCh + 3] > 1.0f);
                        if (om) own = 64 * p + __builtin_ctzll(om);
                    }
                    unsigned long long top = 0;
                    for (int p = 0; p < passes; ++p) {
                        const int c = 64 * p + lane;
                        if (c < cells) {
                            float v = slab[c * kRuleCh + 6];
                            if (c == own) v -= 1.0f;
                            // (positive f32 bit patterns order as unsigned; the inverted cell: first on ties)
                            if (v > 0.f) top = max(top, ((unsigned long long)__float_as_uint(v) << 8) | (unsigned)(255 - c));
                        }
                    }
                    top = wave_max_u64(top);
                    const int tc = 255 - (int)(top & 0xFFu);
                    if (own >= 0 && top != 0 && tc != own) {
                        dx = 64 * rule_sign(tc % t.VW - own % t.VW);
                        dy = 64 * rule_sign(tc / t.VW - own / t.VW);
                    } else {
                        const float* fr = feat + (size_t)row * t.F + (t.F - 2);
                        dx = 64 * rule_signf(0.5f - fr[0]);
                        dy = 64 * rule_signf(0.5f - fr[1]);
                    }
                }
                // move: the candidates on the low lanes, one packed min
                uint32_t key = 0xFFFFFFFFu;
                if (lane < t.attack_base) {
                    const int mx = t.mdx[lane], my = t.mdy[lane];
                    const int r = cy + my, c = cx + mx;
                    bool free = mx == 0 && my == 0;
                    if (!free && r >= 0 && r < t.VH && c >= 0 && c < t.VW) {
                        const float* cell = slab + (r * t.VW + c) * kRuleCh;
                        free = cell[0] <= 0.5f && cell[1] <= 0.5f && cell[4] <= 0.5f;
                    }
                    if (free) key = ((uint32_t)((dx - mx) * (dx - mx) + (dy - my) * (dy - my)) << 8) | (uint32_t)lane;
                }
                key = wave_min_u32(key);
                action = key == 0xFFFFFFFFu ? 0 : (int)(key & 0xFFu);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (the next row's units come behind these reads)
        }
        if (lane == 0) act[rm.slot(row, i)] = action;
    }
}

}  // namespace mfx

// ------------------------------------------------------------------------------------------ C ABI
using namespace mfx;

namespace {
struct RuleHandle {
    RuleTab tab{};
};

int rule_eps(const char* who, float eps) {
    if (eps >= 0.f && eps <= 1.f) return 0;                  // (false for NaN)
    return fail("%s: eps must be in [0, 1]; got %g", who, (double)eps);
}

hipError_t rule_launch(const RuleTab& t, const float* view, const float* feat, QRowMap rm, int n, const int32_t* d_n,
                       float eps, uint32_t seed, uint32_t step, int group, int32_t* act, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    // (28 KB of LDS per workgroup: five of them fit a CU)
    const int grid = std::min((n + kRuleWaves - 1) / kRuleWaves, device_cus() * 5);
    k_rule_act<<<grid, 64 * kRuleWaves, 0, st>>>(t, view, feat, rm, n, d_n, eps, seed, step, group, act);
    return hipGetLastError();
}
}  // namespace

extern "C" {

// shape: {view_h, view_w, channels, feature}.  Host only: no device memory, no launch.
MFX_API int mfx_rule_create(const int32_t* shape, int attack_base, int n_action, const int32_t* view2attack,
                            const int32_t* move_dx, const int32_t* move_dy, void** handle) {
    if (!shape || !view2attack || !move_dx || !move_dy || !handle) return fail("rule_create: null argument");
    const int VH = shape[0], VW = shape[1], C = shape[2], F = shape[3];
    if (C != kRuleCh)
        return fail("rule_create: the rule reads the 7-channel view of two groups with a minimap; got %d channels", C);
    if (VH < 1 || VW < 1 || (long long)VH * VW > kRuleMaxCells)
        return fail("rule_create: the view must have 1..%d cells; got %d x %d", kRuleMaxCells, VH, VW);
    if (F < 2) return fail("rule_create: the feature row ends in x / W, y / H; got %d features", F);
    if (n_action < 2 || n_action > kRuleMaxA) return fail("rule_create: 2 <= n_action <= %d; got %d", kRuleMaxA, n_action);
    if (attack_base < 1 || attack_base > n_action)
        return fail("rule_create: 1 <= attack_base <= n_action; got %d of %d", attack_base, n_action);
    auto* h = new (std::nothrow) RuleHandle();
    if (!h) return fail("rule_create: out of memory");
    RuleTab& t = h->tab;
    t.VH = VH; t.VW = VW; t.F = F; t.n_action = n_action; t.attack_base = attack_base;
    for (int c = 0; c < kRuleMaxCells; ++c) t.v2a[c] = -1;
    for (int c = 0; c < VH * VW; ++c) {
        const int a = view2attack[c];
        if (a < -1 || a >= n_action - attack_base) {
            delete h;
            return fail("rule_create: view2attack[%d] = %d, outside -1..%d", c, a, n_action - attack_base - 1);
        }
        t.v2a[c] = (int8_t)a;
        if (a >= 0) t.atk[c >> 6] |= 1ull << (c & 63);
    }
    for (int a = 0; a < attack_base; ++a) {
        if (std::abs(move_dx[a]) > 16 || std::abs(move_dy[a]) > 16) {
            delete h;
            return fail("rule_create: move[%d] = (%d, %d), beyond 16 cells", a, move_dx[a], move_dy[a]);
        }
        t.mdx[a] = (int8_t)move_dx[a];
        t.mdy[a] = (int8_t)move_dy[a];
    }
    *handle = h;
    return 0;
}

MFX_API int mfx_rule_destroy(void* handle) {
    delete static_cast<RuleHandle*>(handle);
    return 0;
}

// n rows, dense: view [n][VH * VW * 7], feature [n][F] -> act [n]; row i drawn with (seed, step, group, i).
MFX_API int mfx_rule_act(void* handle, const float* d_view, const float* d_feat, int n, float eps, uint32_t seed,
                         uint32_t step, int group, int32_t* d_act, void* stream) {
    if (!handle) return fail("rule_act: no handle");
    if (n < 0) return fail("rule_act: n >= 0; got %d", n);
    MFX_CHECK(rule_eps("rule_act", eps));
    if (!d_view || !d_feat || !d_act) return fail("rule_act: null view, feature or action pointer");
    const QRowMap rm{nullptr, 1, 0, 0, 0};
    MFX_HIP(rule_launch(static_cast<RuleHandle*>(handle)->tab, d_view, d_feat, rm, n, nullptr, eps, seed, step, group,
                        d_act, (hipStream_t)stream));
    return 0;
}

// Group g of a rollout batch (the conventions of mfx_qnet_act_rollout_sample): actions of the group's live rows into
// d_act [E][G][rowcap]; row j of env e drawn with (seed, step, g, e * rowcap + j).
MFX_API int mfx_rule_act_rollout(void* handle, const float* d_view, const float* d_feat, const int32_t* d_counts, int E,
                                 int G, int g, int rowcap, int32_t* d_rows, int32_t* d_total, int32_t* d_act, float eps,
                                 uint32_t seed, uint32_t step, void* stream) {
    if (!handle) return fail("rule_act_rollout: no handle");
    if (E < 0 || G < 1 || g < 0 || g >= G || rowcap < 1 || (long long)E * rowcap > 0x7FFFFFFFll)
        return fail("rule_act_rollout: bad shape (E %d, G %d, g %d, rowcap %d)", E, G, g, rowcap);
    MFX_CHECK(rule_eps("rule_act_rollout", eps));
    if (!d_view || !d_feat || !d_counts || !d_rows || !d_total || !d_act)
        return fail("rule_act_rollout: null buffer pointer");
    hipStream_t st = (hipStream_t)stream;
    MFX_HIP(launch_rollout_rows(d_counts, E, G, g, rowcap, d_rows, d_total, st));
    const QRowMap rm{d_rows, rowcap, G * rowcap, g * rowcap, 0};
    MFX_HIP(rule_launch(static_cast<RuleHandle*>(handle)->tab, d_view, d_feat, rm, E * rowcap, d_total, eps, seed, step,
                        g, d_act, st));
    return 0;
}

}  // extern "C"
