// score_kernels.hip -- per-episode outcomes of the device rollout loop (mfrl_amd.scoreboard.RolloutScoreboard): the
// scorekeeper of an evaluation round (the reference's battle.py through Runner.run(train=False)), beside the collector.
//
// The rollout restarts a finished env inside its step and keeps only sums (stats[e] = episodes finished, the two return
// sums, kills), so an episode's outcome has to be taken at the step that ends it.  One launch after every
// mfx_battle_rollout_policy_step does that from four rollout buffers (group_num, alive, stats, agent_steps) and a few
// words of state carried per env; include/magent_amd.h part 7 states the contract, tests/score_ref.py restates it in
// NumPy.  The win rule is Runner.run's: kill[i] = max_nums[i] - nums[1 - i] with nums read after the step and before
// clear_dead (senario_battle.py:258), i.e. the members of the last step, those that died in it included -- the group
// sizes this kernel carried over from before the step, not the survivor count.
//
// Shape: launch- and latency-bound (2 x rowcap bytes per env).  One wave per env, four envs per workgroup, grid-stride
// over envs.  Everything the wave reads is wave-uniform except the alive rows, which lanes read as dwords (rowcap is a
// multiple of 4, so every [e][g] row is dword aligned) with the last partial dword masked; non-zero bytes are counted
// by one ballot per byte position, whose popcount is already the wave's sum in a scalar.  Lane 0 stores.  The carried
// group sizes are checked against rowcap before any alive byte is addressed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfx_common.h"
#include "../../include/magent_amd.h"

namespace mfx {

static_assert(sizeof(mfx_score_record) == 48, "mfx_score_record is 48 bytes");

__device__ __forceinline__ bool score_count_ok(int64_t n, int rowcap) { return n >= 0 && n <= rowcap; }

// An env's carry taken afresh from the buffers: attach, and update after a failed guard.
__device__ __forceinline__ void score_snapshot(const mfx_score_src& s, const mfx_score_dst& d, int e) {
    int64_t* c = d.carry + (size_t)e * MFX_SCORE_CARRY;
    const int64_t n0 = s.group_num[(size_t)e * 2], n1 = s.group_num[(size_t)e * 2 + 1];
    c[MFX_SCORE_N_CUR] = n0;
    c[MFX_SCORE_N_CUR + 1] = n1;
    c[MFX_SCORE_START] = n0;
    c[MFX_SCORE_START + 1] = n1;
    c[MFX_SCORE_EP] = (int64_t)s.stats[(size_t)e * 4];
    c[MFX_SCORE_STEPS0] = s.agent_steps[e];
    c[MFX_SCORE_LEN] = 0;
    c[7] = 0;
    d.ret0[(size_t)e * 2] = s.stats[(size_t)e * 4 + 1];
    d.ret0[(size_t)e * 2 + 1] = s.stats[(size_t)e * 4 + 2];
}

__device__ __forceinline__ void score_flag(int64_t* state, unsigned long long bits) {
    atomicOr(reinterpret_cast<unsigned long long*>(state + 1), bits);
}

__global__ void __launch_bounds__(256) k_score_attach(mfx_score_src s, mfx_score_dst d) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
    if (tid < 2) d.state[tid] = 0;
    for (int64_t e = tid; e < s.n_envs; e += nt) {
        score_snapshot(s, d, (int)e);
        for (int k = 0; k < MFX_SCORE_TOTALS; ++k) d.totals[e * MFX_SCORE_TOTALS + k] = 0;
    }
    int64_t* lw = reinterpret_cast<int64_t*>(d.log);
    const int64_t words = (int64_t)s.n_envs * d.ep_cap * (int64_t)(sizeof(mfx_score_record) / 8);
    for (int64_t i = tid; i < words; i += nt) lw[i] = 0;
}

// A group size outside [0, rowcap] at attach: the word is cleared by the stores above, so a kernel of its own, behind.
__global__ void __launch_bounds__(256) k_score_attach_check(mfx_score_src s, mfx_score_dst d) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = tid; e < s.n_envs; e += nt)
        if (!score_count_ok(s.group_num[e * 2], s.rowcap) || !score_count_ok(s.group_num[e * 2 + 1], s.rowcap))
            score_flag(d.state, MFX_SCORE_ERR_COUNT);
}

// Non-zero bytes among row[0 .. n) of a dword-aligned row; n in [0, rowcap], wave-uniform.  The result is wave-uniform.
__device__ __forceinline__ int score_survivors(const uint8_t* row, int n, int lane) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(row);
    const int nd = (n + 3) >> 2;
    int cnt = 0;
    for (int base = 0; base < nd; base += 64) {
        const int i = base + lane;
        uint32_t v = 0;
        if (i < nd) {
            v = p[i];
            const int rem = n - 4 * i;                   // >= 1
            if (rem < 4) v &= (1u << (8 * rem)) - 1u;    // bytes at and past n are stale rows of earlier steps
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) cnt += __popcll(__ballot(((v >> (8 * b)) & 0xffu) != 0));
    }
    return cnt;
}

__global__ void __launch_bounds__(256) k_score_update(mfx_score_src s, mfx_score_dst d) {
    const int lane = threadIdx.x & 63;
    const int W = (int)gridDim.x * 4;
    for (int e = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6))); e < s.n_envs; e += W) {
        int64_t* c = d.carry + (size_t)e * MFX_SCORE_CARRY;
        const int64_t n0 = c[MFX_SCORE_N_CUR], n1 = c[MFX_SCORE_N_CUR + 1];
        const int64_t st0 = c[MFX_SCORE_START], st1 = c[MFX_SCORE_START + 1];
        const int64_t ep = c[MFX_SCORE_EP], steps0 = c[MFX_SCORE_STEPS0];
        int64_t len = c[MFX_SCORE_LEN];
        const int64_t g0 = s.group_num[(size_t)e * 2], g1 = s.group_num[(size_t)e * 2 + 1];
        const double* stats = s.stats + (size_t)e * 4;
        const int64_t ep_now = (int64_t)stats[0], steps_now = s.agent_steps[e];
        unsigned long long err = 0;
        if (steps_now - steps0 != n0 + n1) err |= MFX_SCORE_ERR_STEP;
        if (ep_now != ep && ep_now != ep + 1) err |= MFX_SCORE_ERR_EPISODE;
        if (!score_count_ok(n0, s.rowcap) || !score_count_ok(n1, s.rowcap) || !score_count_ok(g0, s.rowcap) ||
            !score_count_ok(g1, s.rowcap))
            err |= MFX_SCORE_ERR_COUNT;
        if (err) {                                       // not scored: no alive byte is read, totals and log stay
            if (lane == 0) {
                score_flag(d.state, err);
                score_snapshot(s, d, e);
            }
            continue;
        }
        const uint8_t* alive = s.alive + (size_t)e * 2 * s.rowcap;
        const int surv0 = score_survivors(alive, (int)n0, lane);
        const int surv1 = score_survivors(alive + s.rowcap, (int)n1, lane);
        if (lane == 0) {                                 // the values are wave-uniform; one lane stores
            len += 1;
            if (ep_now == ep + 1) {
                const int64_t kill0 = st0 - n1, kill1 = st1 - n0;
                const int winner = kill0 > kill1 ? 0 : kill0 < kill1 ? 1 : 2;
                const double now0 = stats[1], now1 = stats[2];
                int64_t* t = d.totals + (size_t)e * MFX_SCORE_TOTALS;
                const int64_t idx = t[MFX_SCORE_EPISODES];
                if (idx >= 0 && idx < d.ep_cap) {
                    mfx_score_record r;
                    r.len = (int32_t)len;
                    r.nums[0] = (int32_t)n0;
                    r.nums[1] = (int32_t)n1;
                    r.surv[0] = surv0;
                    r.surv[1] = surv1;
                    r.kill[0] = (int32_t)kill0;
                    r.kill[1] = (int32_t)kill1;
                    r.winner = winner;
                    r.ret[0] = now0 - d.ret0[(size_t)e * 2];
                    r.ret[1] = now1 - d.ret0[(size_t)e * 2 + 1];
                    d.log[(size_t)e * d.ep_cap + idx] = r;
                } else {
                    t[MFX_SCORE_DROPPED] += 1;
                }
                t[MFX_SCORE_EPISODES] = idx + 1;
                t[MFX_SCORE_MAIN_WINS + winner] += 1;
                t[MFX_SCORE_KILLS] += kill0;
                t[MFX_SCORE_KILLS + 1] += kill1;
                t[MFX_SCORE_STEPS] += len;
                if (idx + 1 == d.target) atomicAdd(reinterpret_cast<unsigned long long*>(d.state), 1ull);
                len = 0;
                c[MFX_SCORE_EP] = ep + 1;
                d.ret0[(size_t)e * 2] = now0;
                d.ret0[(size_t)e * 2 + 1] = now1;
                c[MFX_SCORE_START] = g0;
                c[MFX_SCORE_START + 1] = g1;
            }
            c[MFX_SCORE_N_CUR] = g0;
            c[MFX_SCORE_N_CUR + 1] = g1;
            c[MFX_SCORE_STEPS0] = steps_now;
            c[MFX_SCORE_LEN] = len;
        }
    }
}

static int score_shape(const char* who, const mfx_score_src* s, const mfx_score_dst* d) {
    if (!s || !d) return fail("%s: null argument", who);
    if (s->n_groups != 2)
        return fail("%s: two groups only (main and opponent), got n_groups = %d", who, s->n_groups);
    if (s->n_envs < 1) return fail("%s: n_envs = %d", who, s->n_envs);
    if (s->rowcap < 4 || (s->rowcap & 3) != 0)
        return fail("%s: rowcap must be a multiple of 4, got %d", who, s->rowcap);
    if (!s->group_num || !s->alive || !s->stats || !s->agent_steps) return fail("%s: a rollout buffer is missing", who);
    if (((uintptr_t)s->alive & 3) != 0) return fail("%s: the alive rows must be 4-byte aligned", who);
    if (d->ep_cap < 0 || d->target < 1)
        return fail("%s: ep_cap >= 0 and target >= 1, got %lld and %lld", who, (long long)d->ep_cap,
                    (long long)d->target);
    if (!d->carry || !d->ret0 || !d->totals || !d->state || (d->ep_cap > 0 && !d->log))
        return fail("%s: a destination buffer is missing", who);
    if (((uintptr_t)d->log & 7) != 0) return fail("%s: the log must be 8-byte aligned", who);
    return 0;
}

}  // namespace mfx

using namespace mfx;

extern "C" {

MFX_API int mfx_score_sizes(int n_envs, int64_t ep_cap, size_t bytes[5]) {
    if (n_envs < 1 || ep_cap < 0 || !bytes) return fail("score_sizes: bad argument");
    bytes[0] = (size_t)n_envs * MFX_SCORE_CARRY * 8;
    bytes[1] = (size_t)n_envs * 2 * 8;
    bytes[2] = (size_t)n_envs * MFX_SCORE_TOTALS * 8;
    bytes[3] = (size_t)n_envs * (size_t)ep_cap * sizeof(mfx_score_record);
    bytes[4] = 2 * 8;
    return 0;
}

MFX_API int mfx_score_attach(const mfx_score_src* src, const mfx_score_dst* dst, void* stream) {
    MFX_CHECK(score_shape("score_attach", src, dst));
    hipStream_t st = (hipStream_t)stream;
    const int64_t items = (int64_t)src->n_envs * (dst->ep_cap * 6 > 1 ? dst->ep_cap * 6 : 1);
    const int64_t wgs = (items + 255) / 256, cap = (int64_t)device_cus() * 8;
    k_score_attach<<<(int)(wgs < cap ? wgs : cap), 256, 0, st>>>(*src, *dst);
    MFX_HIP(hipGetLastError());
    const int64_t w2 = ((int64_t)src->n_envs + 255) / 256;
    k_score_attach_check<<<(int)(w2 < cap ? w2 : cap), 256, 0, st>>>(*src, *dst);
    MFX_HIP(hipGetLastError());
    return 0;
}

MFX_API int mfx_score_update(const mfx_score_src* src, const mfx_score_dst* dst, void* stream) {
    MFX_CHECK(score_shape("score_update", src, dst));
    const int64_t wgs = ((int64_t)src->n_envs + 3) / 4, cap = (int64_t)device_cus() * 8;
    k_score_update<<<(int)(wgs < cap ? wgs : cap), 256, 0, (hipStream_t)stream>>>(*src, *dst);
    MFX_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
