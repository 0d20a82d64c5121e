// collect_kernels.hip -- replay rows straight from the device rollout loop (mfrl_amd.replay.RolloutCollector):
// one row of MemoryGroup's step rows (algo/tools.py _StepRows: view, feature, action, reward, terminal, former mean
// action, agent key) per live agent of one group for every mfx_battle_rollout_policy_step, with no host work per
// step.  A step is collected in two halves around the policy step, because neither half of a row survives it:
//
//   mfx_collect_begin  (the policy's actions are in the action buffer; before the step)
//       the compact live-row list of the group (launch_rollout_rows, in the collector's own scratch), then for list
//       entry k = row j of env e -> step row n + k: the view row, the feature row, the action, the env's former mean
//       action as float32, and the env's episode number (stats[e][0]) parked in the key column;
//   mfx_collect_end    (after the step, same list)
//       the reward, terminal = !alive and the key (collect_key of env, parked episode number, id) from the rollout's
//       rewards / alive / ids buffers, which hold the members as they were before clear_dead; then one thread advances
//       the row counter n by the list length, behind the row writes on the same stream.
//
// n and the error word live on the device (state[0], state[1]); the host reads them once, in finish().  Both halves
// check n + count against the destination capacity before any store: a step that does not fit writes nothing, sets
// bit 0 of the error word (sticky) and leaves n where it was.
//
// For the actor-critic models (EpisodesBuffer rows: algo/ac.py train_rollout) mfx_collect_end_linked also records,
// in the same launch, which row precedes each row in its agent's episode (prev) and which rows end a chain so far
// (tail); mfx_chain_returns then turns the reward column into discounted returns in place by walking those chains,
// so the step-major rows are never sorted or regrouped.
//
// The view move is the HBM-bound part (4,732 B read + written per row, up to 40 GB per step at 256x256 x 2048 envs)
// and follows k_rows_pipe (replay_kernels.hip): one wave per row, 16-B units at the rows' dword alignment, two rows in
// flight per wave -- row k + W's loads are issued before row k's stores --, the list entry through a scalar load (the
// row is wave-uniform), every slot index a constant so the rows stay in registers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfx_common.h"
#include "policy_gemm.h"
#include "../../include/magent_amd.h"

namespace mfx {

constexpr int kColQ = 5;                 // 16-B units per lane of a view row: up to 64 x 4 x 5 + 3 floats
constexpr int kColNarrow = 64;           // feature floats / actions per row moved by one lane each
typedef uint32_t c32x4a4 __attribute__((ext_vector_type(4), aligned(4)));

// The agent key of a collected row: injective over (env < n_envs, episode >= 0, id < id_stride).  Ids restart at 0
// in every episode, so the episode number keeps an agent of the next episode out of its predecessor's sequence.
// (mfrl_amd.replay.rollout_key restates it.)
__host__ __device__ inline int64_t collect_key(int64_t env, int64_t episode, int64_t id, int64_t n_envs,
                                               int64_t id_stride) {
    return (episode * n_envs + env) * id_stride + id;
}

__device__ __forceinline__ void collect_flag(int64_t* state, unsigned long long bit) {
    atomicOr(reinterpret_cast<unsigned long long*>(state + 1), bit);
}

struct CollectRow {
    bool ok;
    int64_t d;                 // destination row
    c32x4a4 q[kColQ];          // this lane's 16-B units of the view row
    uint32_t t;                //   and tail dword
    uint32_t f;                // this lane's feature dword
    float p;                   // this lane's mean-action entry
    int32_t a;                 // lane 0: the action
    int64_t ep;                //         the episode number
};

// kProb: 0 no prob column, 1 the env's mean action (s.mean, float64), 2 the row's own (prob_rows [E][rowcap][n_action]
// float32: the neighbourhood mean, neighbor_kernels.hip).
template <int kProb>
__global__ void __launch_bounds__(256) k_collect_begin(mfx_collect_src s, mfx_collect_dst d,
                                                       const int32_t* __restrict__ rows,
                                                       const int32_t* __restrict__ total, int64_t* state,
                                                       const float* __restrict__ prob_rows) {
    const int lane = threadIdx.x & 63;
    const int count = *total;
    const int64_t n = state[0];
    if (n + count > d.capacity) {                    // the step does not fit: nothing is written
        if (blockIdx.x == 0 && threadIdx.x == 0) collect_flag(state, 1ull);
        return;
    }
    const int W = (int)gridDim.x * 4;
    const int first = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int nq = s.view_floats >> 2, nt = s.view_floats & 3;
    auto fetch = [&](int k, CollectRow& r) {
        r.ok = k < count;
        if (!r.ok) return;
        const int row = rows[k];                     // wave-uniform: a scalar load
        const int e = row / s.rowcap, j = row - e * s.rowcap;
        const size_t eg = (size_t)e * s.n_groups + s.group;
        r.d = n + k;
        const uint32_t* vp = reinterpret_cast<const uint32_t*>(s.view + (size_t)row * s.view_floats);
#pragma unroll
        for (int u = 0; u < kColQ; ++u) {
            const int q = lane + 64 * u;
            if (q < nq) r.q[u] = reinterpret_cast<const c32x4a4*>(vp)[q];
        }
        if (lane < nt) r.t = vp[4 * nq + lane];
        if (lane < s.feat_floats)
            r.f = reinterpret_cast<const uint32_t*>(s.feat)[(size_t)row * s.feat_floats + lane];
        if (kProb == 1 && lane < s.n_action) r.p = (float)s.mean[eg * s.mean_stride + lane];
        if (kProb == 2 && lane < s.n_action) r.p = prob_rows[(size_t)row * s.n_action + lane];
        if (lane == 0) {
            r.a = s.actions[eg * s.rowcap + j];
            r.ep = (int64_t)s.stats[(size_t)e * 4];
        }
    };
    auto put = [&](const CollectRow& r) {
        if (!r.ok) return;
        uint32_t* op = reinterpret_cast<uint32_t*>(d.obs + (size_t)r.d * s.view_floats);
#pragma unroll
        for (int u = 0; u < kColQ; ++u) {
            const int q = lane + 64 * u;
            if (q < nq) reinterpret_cast<c32x4a4*>(op)[q] = r.q[u];
        }
        if (lane < nt) op[4 * nq + lane] = r.t;
        if (lane < s.feat_floats)
            reinterpret_cast<uint32_t*>(d.feat)[(size_t)r.d * s.feat_floats + lane] = r.f;
        if (kProb && lane < s.n_action) d.prob[(size_t)r.d * s.n_action + lane] = r.p;
        if (lane == 0) {
            d.act[r.d] = r.a;
            d.key[r.d] = r.ep;                       // parked until k_collect_end knows the id
        }
    };
    CollectRow r[2];
    fetch(first, r[0]);
    int k = first;
    while (k < count) {
        fetch(k + W, r[1]);                          // row k + W in flight ...
        put(r[0]);                                   // ... while row k drains
        k += W;
        if (k >= count) break;
        fetch(k + W, r[0]);
        put(r[1]);
        k += W;
    }
}

// The link columns of a linked collection (mfx_collect_end_linked); all null in the unlinked kernel.
struct CollectLinks {
    int64_t* last;             // [n_envs * id_stride]: the newest row of (env, id), -1 when empty
    int64_t* prev;             // [capacity]
    uint8_t* tail;             // [capacity]
};

// One lane per list entry: reward, terminal and key of step row n + k.  kLink: also the row's place in its agent's
// episode chain -- prev[r] = the row of the same key one step earlier (or -1), tail[r] = 1 and the predecessor's
// tail = 0 --, found through the table `last` of the newest row per (env, id).
template <bool kLink>
__global__ void __launch_bounds__(256) k_collect_end(mfx_collect_src s, mfx_collect_dst d,
                                                     const int32_t* __restrict__ rows,
                                                     const int32_t* __restrict__ total, int64_t* state,
                                                     int64_t id_stride, CollectLinks lk) {
    const int count = *total;
    const int64_t n = state[0];
    if (n + count > d.capacity) {
        if (blockIdx.x == 0 && threadIdx.x == 0) collect_flag(state, 1ull);
        return;
    }
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const int row = rows[k];
        const int e = row / s.rowcap, j = row - e * s.rowcap;
        const size_t slot = ((size_t)e * s.n_groups + s.group) * s.rowcap + j;
        const int64_t id = s.ids[slot];
        if (id < 0 || id >= id_stride) collect_flag(state, 2ull);      // the key would not be injective
        d.rew[n + k] = s.rewards[slot];
        d.term[n + k] = (uint8_t)(s.alive[slot] == 0);
        const int64_t key = collect_key(e, d.key[n + k], id, s.n_envs, id_stride);
        d.key[n + k] = key;
        if constexpr (kLink) {
            // No atomic and no race: a live id occurs once per env and step, so this lane is the only one of the
            // launch that touches last[e][id], and the only one that clears tail[p] (p is that slot's row of an
            // earlier step, below n; every store of this step is at or above n).  A stale entry -- the id's row of
            // an earlier episode -- fails the key comparison, the episode number being part of the key.  An id the
            // check above flagged has no table entry and starts a chain of its own.
            int64_t p = -1;
            if (id >= 0 && id < id_stride) {
                int64_t* slot_last = lk.last + (size_t)e * id_stride + id;
                p = *slot_last;
                if (p < 0 || p >= n || d.key[p] != key) p = -1;
                *slot_last = n + k;
            }
            if (p >= 0) lk.tail[p] = 0;
            lk.prev[n + k] = p;
            lk.tail[n + k] = 1;
        }
    }
}

__global__ void __launch_bounds__(256) k_fill_i64(int64_t* __restrict__ p, int64_t n, int64_t v) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        p[i] = v;
}

// Discounted returns in place on step-major rows (mfx_chain_returns): one lane per chain, from its tail row back
// along prev, keep = keep * gamma + rew[r]; rew[r] = keep -- k_mfac_returns' recursion (mf_kernels.hip) and its two
// arithmetic forms (numpy1: float64 keep; else float32 keep and gamma; -ffp-contract=off keeps the multiply and the
// add apart), over a linked list instead of a contiguous run.  Latency-bound like it: every step of a chain is a
// load that depends on the one before.  Rows are step-major, so a predecessor lies strictly below its row: a tail
// outside [0, n_rows) or a prev that is neither -1 nor in [0, r) ends the walk there (nothing is stored past it, and
// no walk can cycle) and sets err[0] = 1, err[1] = an offending index.
__device__ int64_t g_chain_err[2];       // zero at load; read, and cleared when set, by mfx_chain_returns

template <typename T>
__global__ void __launch_bounds__(256) k_chain_returns(float* __restrict__ rew, const int64_t* __restrict__ prev,
                                                       const int64_t* __restrict__ tails,
                                                       const float* __restrict__ value, int64_t n_tails,
                                                       int64_t n_rows, T gamma, int64_t* err) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tails) return;
    T keep = (T)value[i];
    int64_t r = tails[i], above = n_rows;
    do {
        if (r < 0 || r >= above) {
            err[1] = r;                              // (any offender: lanes may race here, each with a bad index)
            err[0] = 1;
            return;
        }
        const T t = keep * gamma;
        keep = t + (T)rew[r];
        rew[r] = (float)keep;
        above = r;
        r = prev[r];
    } while (r != -1);
}

// Behind the row writes of its step on the same stream: n += count when the step fitted.
__global__ void k_collect_advance(const int32_t* __restrict__ total, int64_t* state, int64_t capacity) {
    const int64_t n = state[0];
    const int count = *total;
    if (n + count <= capacity) state[0] = n + count;
}

__global__ void k_collect_reset(int64_t* state, int64_t n) {
    state[0] = n;
    state[1] = 0;
}

static int collect_shape(const mfx_collect_src* s, const mfx_collect_dst* d, const void* rows, const void* total,
                         const void* state, const float* prob_rows = nullptr) {
    if (!s || !d || !rows || !total || !state) return fail("collect: null argument");
    if (s->n_envs < 1 || s->n_groups < 1 || s->group < 0 || s->group >= s->n_groups || s->rowcap < 1)
        return fail("collect: bad batch shape");
    if (s->view_floats < 1 || (s->view_floats >> 2) > 64 * kColQ)
        return fail("collect: view rows of 1..%d floats, got %d", 64 * 4 * kColQ + 3, s->view_floats);
    if (s->feat_floats < 1 || s->feat_floats > kColNarrow)
        return fail("collect: feature rows of 1..%d floats, got %d", kColNarrow, s->feat_floats);
    if (d->prob && !prob_rows && (s->n_action < 1 || s->n_action > kColNarrow || s->n_action > s->mean_stride || !s->mean))
        return fail("collect: mean actions of 1..%d entries within the stride, got %d", kColNarrow, s->n_action);
    if (prob_rows && (!d->prob || s->n_action < 1 || s->n_action > kColNarrow))
        return fail("collect: per-row mean actions need a prob column and 1..%d entries, got %d", kColNarrow, s->n_action);
    if (!s->view || !s->feat || !s->actions || !s->rewards || !s->stats || !s->counts || !s->ids || !s->alive)
        return fail("collect: a rollout buffer is missing");
    if (!d->obs || !d->feat || !d->act || !d->rew || !d->term || !d->key || d->capacity < 0)
        return fail("collect: a destination column is missing");
    if ((((uintptr_t)s->view | (uintptr_t)d->obs | (uintptr_t)s->feat | (uintptr_t)d->feat) & 3) != 0)
        return fail("collect: rows must be 4-byte aligned");
    return 0;
}

}  // namespace mfx

using namespace mfx;

extern "C" {

MFX_API int mfx_collect_reset(int64_t* d_state, int64_t n, void* stream) {
    if (!d_state || n < 0) return fail("collect_reset: bad argument");
    k_collect_reset<<<1, 1, 0, (hipStream_t)stream>>>(d_state, n);
    MFX_HIP(hipGetLastError());
    return 0;
}

static int collect_begin(const mfx_collect_src* src, const mfx_collect_dst* dst, const float* d_prob_rows, int32_t* d_rows,
                         int32_t* d_total, int64_t* d_state, void* stream) {
    MFX_CHECK(collect_shape(src, dst, d_rows, d_total, d_state, d_prob_rows));
    hipStream_t st = (hipStream_t)stream;
    MFX_HIP(launch_rollout_rows(src->counts, src->n_envs, src->n_groups, src->group, src->rowcap, d_rows, d_total, st));
    // persistent-sized grid for the upper bound of the list (the count stays on the device): three workgroups per
    // CU, k_rows_pipe's best for one wide column (profiles/r06_replay_ab.txt)
    const int64_t wgs = ((int64_t)src->n_envs * src->rowcap + 3) / 4, cap = (int64_t)device_cus() * 3;
    const int grid = (int)(wgs < cap ? wgs : cap);
    if (d_prob_rows) k_collect_begin<2><<<grid, 256, 0, st>>>(*src, *dst, d_rows, d_total, d_state, d_prob_rows);
    else if (dst->prob) k_collect_begin<1><<<grid, 256, 0, st>>>(*src, *dst, d_rows, d_total, d_state, nullptr);
    else k_collect_begin<0><<<grid, 256, 0, st>>>(*src, *dst, d_rows, d_total, d_state, nullptr);
    MFX_HIP(hipGetLastError());
    return 0;
}

MFX_API int mfx_collect_begin(const mfx_collect_src* src, const mfx_collect_dst* dst, int32_t* d_rows, int32_t* d_total,
                              int64_t* d_state, void* stream) {
    return collect_begin(src, dst, nullptr, d_rows, d_total, d_state, stream);
}

// mfx_collect_begin with the prob of a row taken from its own entry of d_prob_rows [E][rowcap][n_action] float32.
MFX_API int mfx_collect_begin_rows(const mfx_collect_src* src, const mfx_collect_dst* dst, const float* d_prob_rows,
                                   int32_t* d_rows, int32_t* d_total, int64_t* d_state, void* stream) {
    if (!d_prob_rows) return fail("collect_begin_rows: null prob rows");
    return collect_begin(src, dst, d_prob_rows, d_rows, d_total, d_state, stream);
}

MFX_API int mfx_collect_end(const mfx_collect_src* src, const mfx_collect_dst* dst, const int32_t* d_rows,
                            const int32_t* d_total, int64_t* d_state, int64_t id_stride, void* stream) {
    MFX_CHECK(collect_shape(src, dst, d_rows, d_total, d_state));
    if (id_stride < 1) return fail("collect_end: id stride %lld", (long long)id_stride);
    hipStream_t st = (hipStream_t)stream;
    const int64_t wgs = ((int64_t)src->n_envs * src->rowcap + 255) / 256, cap = (int64_t)device_cus() * 8;
    k_collect_end<false><<<(int)(wgs < cap ? wgs : cap), 256, 0, st>>>(*src, *dst, d_rows, d_total, d_state, id_stride,
                                                                       CollectLinks{nullptr, nullptr, nullptr});
    MFX_HIP(hipGetLastError());
    k_collect_advance<<<1, 1, 0, st>>>(d_total, d_state, dst->capacity);
    MFX_HIP(hipGetLastError());
    return 0;
}

MFX_API int mfx_collect_end_linked(const mfx_collect_src* src, const mfx_collect_dst* dst, const int32_t* d_rows,
                                   const int32_t* d_total, int64_t* d_state, int64_t id_stride, int64_t* d_last,
                                   int64_t* d_prev, uint8_t* d_tail, void* stream) {
    MFX_CHECK(collect_shape(src, dst, d_rows, d_total, d_state));
    if (id_stride < 1) return fail("collect_end_linked: id stride %lld", (long long)id_stride);
    if (!d_last || !d_prev || !d_tail) return fail("collect_end_linked: a link column is missing");
    hipStream_t st = (hipStream_t)stream;
    const int64_t wgs = ((int64_t)src->n_envs * src->rowcap + 255) / 256, cap = (int64_t)device_cus() * 8;
    k_collect_end<true><<<(int)(wgs < cap ? wgs : cap), 256, 0, st>>>(*src, *dst, d_rows, d_total, d_state, id_stride,
                                                                      CollectLinks{d_last, d_prev, d_tail});
    MFX_HIP(hipGetLastError());
    k_collect_advance<<<1, 1, 0, st>>>(d_total, d_state, dst->capacity);
    MFX_HIP(hipGetLastError());
    return 0;
}

MFX_API int mfx_collect_links_reset(int64_t* d_last, int64_t n, void* stream) {
    if (n < 0 || (n > 0 && !d_last)) return fail("collect_links_reset: bad argument");
    if (n == 0) return 0;
    const int64_t wgs = (n + 255) / 256, cap = (int64_t)device_cus() * 8;
    k_fill_i64<<<(int)(wgs < cap ? wgs : cap), 256, 0, (hipStream_t)stream>>>(d_last, n, -1);
    MFX_HIP(hipGetLastError());
    return 0;
}

MFX_API int mfx_chain_returns(float* d_rew, const int64_t* d_prev, const int64_t* d_tails, const float* d_value,
                              int64_t n_tails, int64_t n_rows, double gamma, int numpy1, void* stream) {
    if (n_tails < 0 || n_rows < 0) return fail("chain_returns: n_tails and n_rows must be >= 0");
    if (n_tails == 0) return 0;
    if (!d_rew || !d_prev || !d_tails || !d_value) return fail("chain_returns: null argument");
    if (n_tails > n_rows) return fail("chain_returns: %lld tails for %lld rows", (long long)n_tails, (long long)n_rows);
    hipStream_t st = (hipStream_t)stream;
    int64_t* err = nullptr;
    MFX_HIP(hipGetSymbolAddress((void**)&err, HIP_SYMBOL(g_chain_err)));
    const unsigned grid = (unsigned)((n_tails + 255) / 256);
    if (numpy1) k_chain_returns<double><<<grid, 256, 0, st>>>(d_rew, d_prev, d_tails, d_value, n_tails, n_rows, gamma, err);
    else k_chain_returns<float><<<grid, 256, 0, st>>>(d_rew, d_prev, d_tails, d_value, n_tails, n_rows, (float)gamma, err);
    MFX_HIP(hipGetLastError());
    int64_t h[2] = {0, 0};
    MFX_HIP(hipMemcpyAsync(h, err, sizeof h, hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    if (h[0]) {
        const int64_t z[2] = {0, 0};
        MFX_HIP(hipMemcpyAsync(err, z, sizeof z, hipMemcpyHostToDevice, st));
        MFX_HIP(hipStreamSynchronize(st));
        return fail("chain_returns: row index %lld is outside its chain's rows (tails in [0, %lld), a predecessor in "
                    "[0, its row))", (long long)h[1], (long long)n_rows);
    }
    return 0;
}

MFX_API int64_t mfx_collect_key(int64_t env, int64_t episode, int64_t id, int64_t n_envs, int64_t id_stride) {
    return collect_key(env, episode, id, n_envs, id_stride);
}

}  // extern "C"
