// neighbor_kernels.hip -- the opt-in neighbourhood mean action of the MF-Q / MF-AC rollouts.
//
// The paper's mean action of agent j is the average over j's neighbours, a_bar_j = 1 / |N(j)| sum_{k in N(j)} a_k; the
// reference (senario_battle.py:141), k_rollout's mean buffer and mfx_mean_action feed every agent of a group the
// group-wide mean instead.  These kernels give every survivor of a step its own row: the mean of the one-hot actions
// of the survivors of its own group within Chebyshev distance R of it, itself included (include/magent_amd.h part 4b
// states the contract; tests/neighbor_mean_ref.py restates it in numpy).
//
// One workgroup per (env, group) item of a persistent grid; the map is a W x H byte grid in LDS (0 empty, action + 1,
// or kNbBad for an occupied cell whose action is outside [0, n_action)), so a survivor's neighbourhood is a window
// scan of (2 R + 1)^2 cells -- 64 at a time, one wave per survivor -- and not a test against every other member.
// Integer counts and one float64 division per entry: no floating-point atomics, bitwise reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "battle_engine.h"
#include "mfx_common.h"
#include "../../include/magent_amd.h"

namespace mfx {

constexpr int kNbMaxA = 64;                 // actions: one histogram bin per lane
constexpr int kNbWaves = 4;
constexpr uint8_t kNbBad = 255;             // an occupied cell that counts in the divisor only
constexpr size_t kNbLdsMax = 160 * 1024;    // LDS of one CU (one workgroup may take all of it)

struct NbArgs {
    int B, rowcap, n_action, radius, W, H;
    float* out;                             // [B][rowcap][n_action]
    // stand-alone loader: a compact row list
    const int32_t* pos;                     // [B][rowcap][2]
    const int32_t* acts;                    // [B][rowcap]   (rollout: [E][G][rowcap], group offset applied)
    const int32_t* counts;                  // [B]           (rollout: group_num [E][G], group offset applied)
    // rollout loader
    const float* feat;                      // [E][rowcap][F] of the group: x / W, y / H in the last two floats
    const uint8_t* alive;                   // [E][G][rowcap], group offset applied
    const double* stats;                    // [E][4]: [0] the episode number
    int32_t* state;                         // [2][E]: prev_num, prev_episode
    int F, G;
};

// LDS of one workgroup: the byte grid, the survivors' packed positions and action codes, one histogram per wave.
__host__ __device__ inline size_t nb_grid_bytes(int W, int H) { return ((size_t)W * H + 15) & ~(size_t)15; }
__host__ __device__ inline size_t nb_lds_bytes(int W, int H, int rowcap) {
    return nb_grid_bytes(W, H) + (size_t)rowcap * 4 + (((size_t)rowcap + 15) & ~(size_t)15) + kNbWaves * kNbMaxA * 4;
}

__device__ __forceinline__ uint8_t nb_code(int a, int n_action) {
    return a >= 0 && a < n_action ? (uint8_t)(a + 1) : kNbBad;
}

// kRollout: the survivors come from the rollout buffers after a policy step (compaction of the pre-clear_dead action
// rows by the alive flags, positions decoded from the new feature rows, the restart rule, the carried state);
// else from a compact (pos, action) row list.  Everything behind the loader is the same code.
template <bool kRollout>
__global__ void __launch_bounds__(64 * kNbWaves) k_neighbor_mean(NbArgs p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t nsm[];
    uint8_t* grid = nsm;
    uint32_t* spos = reinterpret_cast<uint32_t*>(nsm + nb_grid_bytes(p.W, p.H));
    uint8_t* sact = reinterpret_cast<uint8_t*>(spos + p.rowcap);
    int* hist = reinterpret_cast<int*>(nsm + nb_lds_bytes(p.W, p.H, p.rowcap)) - kNbWaves * kNbMaxA;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int A = p.n_action, W = p.W, H = p.H, R = p.radius;
    {   // the grid is zeroed once; every item clears the cells it filled
        uint4* g4 = reinterpret_cast<uint4*>(grid);
        for (int i = tid; i < (int)(nb_grid_bytes(W, H) >> 4); i += blockDim.x) g4[i] = uint4{0u, 0u, 0u, 0u};
    }
    __syncthreads();
    for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
        int n;
        bool restart = false;
        if constexpr (kRollout) {
            const size_t eg = (size_t)b * p.G;
            n = min(max(p.counts[eg], 0), p.rowcap);
            const int prev_n = min(max(p.state[b], 0), p.rowcap);
            const int ep = (int)p.stats[(size_t)b * 4];
            restart = ep != p.state[p.B + b];
            __syncthreads();                          // every lane has read the carried state
            if (tid == 0) {
                p.state[b] = n;
                p.state[p.B + b] = ep;
            }
            if (!restart) {
                // survivor j = the j-th row with alive != 0 among the first prev_n rows: its action code
                if (wid == 0) {
                    int base = 0;
                    for (int i0 = 0; i0 < prev_n; i0 += 64) {
                        const int i = i0 + lane;
                        const bool live = i < prev_n && p.alive[eg * p.rowcap + i] != 0;
                        const unsigned long long m = __ballot(live);
                        const int j = base + __popcll(m & ((1ull << lane) - 1ull));
                        if (live && j < n) sact[j] = nb_code(p.acts[eg * p.rowcap + i], A);
                        base += __popcll(m);
                    }
                    for (int j = base + lane; j < n; j += 64) sact[j] = kNbBad;    // (fewer survivors than rows: never)
                }
                const float* fr = p.feat + (size_t)b * p.rowcap * p.F + (p.F - 2);
                for (int j = tid; j < n; j += blockDim.x) {
                    const int x = (int)rintf(fr[(size_t)j * p.F] * (float)W), y = (int)rintf(fr[(size_t)j * p.F + 1] * (float)H);
                    spos[j] = (uint32_t)(x & 0xFFFF) | ((uint32_t)(y & 0xFFFF) << 16);
                }
            }
        } else {
            n = min(max(p.counts[b], 0), p.rowcap);
            for (int j = tid; j < n; j += blockDim.x) {
                const size_t r = (size_t)b * p.rowcap + j;
                spos[j] = (uint32_t)(p.pos[2 * r] & 0xFFFF) | ((uint32_t)(p.pos[2 * r + 1] & 0xFFFF) << 16);
                sact[j] = nb_code(p.acts[r], A);
            }
        }
        float* orow = p.out + (size_t)b * p.rowcap * A;
        if (restart) {                                // senario_battle.py:89, per row
            for (int i = tid; i < n * A; i += blockDim.x) orow[i] = 0.f;
            continue;
        }
        __syncthreads();
        for (int j = tid; j < n; j += blockDim.x) {
            const int x = (int)(spos[j] & 0xFFFFu), y = (int)(spos[j] >> 16);
            if (x < W && y < H) grid[y * W + x] = sact[j];
        }
        __syncthreads();
        int* h = hist + wid * kNbMaxA;
        for (int j = wid; j < n; j += kNbWaves) {
            const int x = (int)(spos[j] & 0xFFFFu), y = (int)(spos[j] >> 16);
            const int x0 = max(x - R, 0), x1 = min(x + R, W - 1), y0 = max(y - R, 0), y1 = min(y + R, H - 1);
            const int ww = x1 - x0 + 1, cells = x0 <= x1 && y0 <= y1 ? ww * (y1 - y0 + 1) : 0;
            __atomic_store_n(&h[lane], 0, __ATOMIC_RELAXED);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // the wave's LDS operations keep this order
            int cnt = 0;
            for (int c0 = 0; c0 < cells; c0 += 64) {
                const int c = c0 + lane;
                uint8_t v = 0;
                if (c < cells) {
                    const int dy = c / ww;
                    v = grid[(y0 + dy) * W + x0 + (c - dy * ww)];
                }
                cnt += __popcll(__ballot(v != 0));
                if (v != 0 && v != kNbBad) atomicAdd(&h[v - 1], 1);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            const int k = __atomic_load_n(&h[lane], __ATOMIC_RELAXED);
            if (lane < A) orow[(size_t)j * A + lane] = cnt ? (float)((double)k / (double)cnt) : 0.f;
        }
        __syncthreads();
        for (int j = tid; j < n; j += blockDim.x) {
            const int x = (int)(spos[j] & 0xFFFFu), y = (int)(spos[j] >> 16);
            if (x < W && y < H) grid[y * W + x] = 0;
        }
        __syncthreads();
    }
}

// The reset form of the rollout state: the rows of the live agents zero, prev_num = group_num, prev_episode = the
// episode number.  One workgroup per env.
__global__ void __launch_bounds__(256) k_neighbor_reset(NbArgs p) {
    const int b = blockIdx.x;
    const int n = min(max(p.counts[(size_t)b * p.G], 0), p.rowcap);
    float* orow = p.out + (size_t)b * p.rowcap * p.n_action;
    for (int i = threadIdx.x; i < n * p.n_action; i += blockDim.x) orow[i] = 0.f;
    if (threadIdx.x == 0) {
        p.state[b] = n;
        p.state[p.B + b] = (int)p.stats[(size_t)b * 4];
    }
}

static int nb_shape(const char* who, int B, int rowcap, int n_action, int radius, int W, int H) {
    if (B < 0 || rowcap < 1) return fail("%s: B >= 0 and rowcap >= 1; got B %d, rowcap %d", who, B, rowcap);
    if (n_action < 1 || n_action > kNbMaxA) return fail("%s: 1 <= n_action <= %d; got %d", who, kNbMaxA, n_action);
    if (radius < 0) return fail("%s: the radius must be >= 0; got %d", who, radius);
    if (W < 1 || H < 1 || W > 65535 || H > 65535) return fail("%s: a map of %d x %d", who, W, H);
    const size_t need = nb_lds_bytes(W, H, rowcap);
    if (need > kNbLdsMax)
        return fail("%s: a %d x %d map with %d rows per env needs %zu bytes of LDS (one byte per cell, five per row); "
                    "the limit is %zu", who, W, H, rowcap, need, kNbLdsMax);
    return 0;
}

template <bool kRollout>
static int nb_launch(NbArgs p, hipStream_t st) {
    if (p.B == 0) return 0;
    p.radius = std::min(p.radius, std::max(p.W, p.H));                 // (the window is clamped to the map anyway)
    const size_t lds = nb_lds_bytes(p.W, p.H, p.rowcap);
    const int per_cu = (int)std::min<size_t>(std::max<size_t>(kNbLdsMax / lds, 1), 8);
    const int grid = (int)std::min<int64_t>(p.B, (int64_t)device_cus() * per_cu);
    k_neighbor_mean<kRollout><<<grid, 64 * kNbWaves, lds, st>>>(p);
    MFX_HIP(hipGetLastError());
    return 0;
}

// The rollout buffers of group `group` of an engine behind rollout_init, as the loader's arguments.
static int nb_rollout_args(BattleEngine* e, const char* who, int group, int radius, float* d_out, int32_t* d_state,
                           NbArgs* p) {
    if (!e) return fail("%s: null engine", who);
    if (!e->rollout_ready) return fail("%s before rollout_init", who);
    const int G = e->n_groups();
    if (group < 0 || group >= G) return fail("%s: bad group %d", who, group);
    if (!d_out || !d_state) return fail("%s: null argument", who);
    if (!e->gp.minimap || e->gp.feat_size[group] < 2)
        return fail("%s: the features of group %d carry no position (minimap_mode is off)", who, group);
    const int rc = e->ra.rowcap;
    MFX_CHECK(nb_shape(who, e->E, rc, e->gp.type[group].n_action, radius, e->gp.W, e->gp.H));
    *p = NbArgs{};
    p->B = e->E; p->rowcap = rc; p->n_action = e->gp.type[group].n_action; p->radius = radius;
    p->W = e->gp.W; p->H = e->gp.H; p->out = d_out;
    p->acts = e->ra.actions + (size_t)group * rc;
    p->counts = e->s.grp_n + group;
    p->feat = e->ra.feat[group];
    p->alive = e->ra.alive + (size_t)group * rc;
    p->stats = e->ra.stats;
    p->state = d_state;
    p->F = e->gp.feat_size[group]; p->G = G;
    return 0;
}

}  // namespace mfx

using namespace mfx;

extern "C" {

MFX_API int mfx_neighbor_mean(const int32_t* d_pos, const int32_t* d_actions, const int32_t* d_counts, int B, int rowcap,
                              int n_action, int radius, int W, int H, float* d_out, void* stream) {
    MFX_CHECK(nb_shape("neighbor_mean", B, rowcap, n_action, radius, W, H));
    if (B == 0) return 0;
    if (!d_pos || !d_actions || !d_counts || !d_out) return fail("neighbor_mean: null argument");
    NbArgs p{};
    p.B = B; p.rowcap = rowcap; p.n_action = n_action; p.radius = radius; p.W = W; p.H = H; p.out = d_out;
    p.pos = d_pos; p.acts = d_actions; p.counts = d_counts;
    return nb_launch<false>(p, (hipStream_t)stream);
}

MFX_API int mfx_neighbor_mean_reset(void* game, int group, float* d_out, int32_t* d_state) {
    auto* e = static_cast<BattleEngine*>(game);
    NbArgs p;
    MFX_CHECK(nb_rollout_args(e, "neighbor_mean_reset", group, 0, d_out, d_state, &p));
    k_neighbor_reset<<<p.B, 256, 0, e->stream>>>(p);
    MFX_HIP(hipGetLastError());
    return 0;
}

MFX_API int mfx_neighbor_mean_rollout(void* game, int group, int radius, float* d_out, int32_t* d_state) {
    auto* e = static_cast<BattleEngine*>(game);
    NbArgs p;
    MFX_CHECK(nb_rollout_args(e, "neighbor_mean_rollout", group, radius, d_out, d_state, &p));
    return nb_launch<true>(p, e->stream);
}

}  // extern "C"
