// trace_kernels.hip -- the recorder of the device rollout loop (mfrl_amd.recorder.RolloutRecorder): per step, the rows of
// a few watched envs that let a one-env engine re-run them from the round's start and prove the re-run right, beside the
// collector and the scorekeeper.  include/magent_amd.h part 8 states the contract, tests/trace_ref.py restates it in
// NumPy.
//
// One launch per step, behind mfx_battle_rollout_policy_step: a learned policy's step only reads the action buffer
// (kExt in csrc/battle/rollout.inc and rollout_big.inc), so the actions it acted with are still there; the group sizes
// of before the step are not (clear_dead and a restart rewrite group_num inside the step) and are carried from the
// previous launch, as the scorekeeper carries them.  Attach also takes each watched env's shuffle-engine state (rng[e]):
// no reset re-seeds it, so a round's attack order depends on it and the re-run has to start from it.
//
// Shape: launch-bound (13 x rowcap bytes per watched env and group).  One workgroup per (watched env, group): both
// workgroups of an env read the carry of the step's parity and evaluate the same guards; the group-0 one writes the
// head and the carry of the other parity, which nobody reads in this launch, so nothing depends on the launch order.
// Rows move verbatim as 16-byte vectors (rowcap is a multiple of 4; the byte-wide alive row as dwords unless rowcap is a
// multiple of 16).  No address depends on a group size, only on step < cap_steps, k < K, g < 2 and the row index.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfx_common.h"
#include "../../include/magent_amd.h"

namespace mfx {

__device__ __forceinline__ bool trace_count_ok(int64_t n, int rowcap) { return n >= 0 && n <= rowcap; }

__device__ __forceinline__ void trace_flag(int64_t* state, unsigned long long bits) {
    atomicOr(reinterpret_cast<unsigned long long*>(state + 1), bits);
}

// One wave: lane k takes watched env k's carry (parity 0) and seed; lane 0 stores the two state words.
__global__ void __launch_bounds__(64) k_trace_attach(mfx_trace_src s, mfx_trace_dst d) {
    const int k = threadIdx.x;
    unsigned long long err = 0;
    if (k < d.n_watch) {
        const int e = d.envs[k];
        int64_t c[MFX_TRACE_CARRY] = {0, 0, 0, 0};
        uint32_t seed = 0;
        if (e < 0 || e >= s.n_envs) {
            err = MFX_TRACE_ERR_ENV;
        } else {
            c[0] = s.group_num[(size_t)e * 2];
            c[1] = s.group_num[(size_t)e * 2 + 1];
            c[2] = (int64_t)s.stats[(size_t)e * 4];
            c[3] = s.agent_steps[e];
            seed = s.rng[e];
            if (!trace_count_ok(c[0], s.rowcap) || !trace_count_ok(c[1], s.rowcap)) err = MFX_TRACE_ERR_COUNT;
        }
        for (int p = 0; p < 2; ++p)
            for (int i = 0; i < MFX_TRACE_CARRY; ++i)
                d.carry[((size_t)p * d.n_watch + k) * MFX_TRACE_CARRY + i] = p == 0 ? c[i] : 0;
        d.seeds[k] = seed;
    }
    const bool env_bad = __ballot(err == MFX_TRACE_ERR_ENV) != 0, count_bad = __ballot(err == MFX_TRACE_ERR_COUNT) != 0;
    if (k == 0) {
        d.state[0] = 0;
        d.state[1] = (env_bad ? MFX_TRACE_ERR_ENV : 0) | (count_bad ? MFX_TRACE_ERR_COUNT : 0);
    }
}

template <class V>
__device__ __forceinline__ void trace_copy(void* dst, const void* src, int n_vec) {
    V* o = reinterpret_cast<V*>(dst);
    const V* i = reinterpret_cast<const V*>(src);
    for (int j = threadIdx.x; j < n_vec; j += blockDim.x) o[j] = i[j];
}

__global__ void __launch_bounds__(256) k_trace_update(mfx_trace_src s, mfx_trace_dst d, int64_t step) {
    const int k = blockIdx.x >> 1, g = blockIdx.x & 1;     // grid = 2 K
    const bool lead = g == 0 && threadIdx.x == 0;
    if (step < 0 || step >= d.cap_steps) {                 // full: nothing but the bit
        if (lead && k == 0) trace_flag(d.state, MFX_TRACE_FULL);
        return;
    }
    const int K = d.n_watch, rc = s.rowcap;
    const int e = d.envs[k];
    int64_t* head = d.head + ((size_t)step * K + k) * MFX_TRACE_HEAD;
    if (e < 0 || e >= s.n_envs) {                          // (the host refuses such a list: a corrupted one)
        if (lead) {
            trace_flag(d.state, MFX_TRACE_ERR_ENV);
            for (int i = 0; i < MFX_TRACE_HEAD; ++i) head[i] = 0;
            if (k == 0) d.state[0] = step + 1;
        }
        return;
    }
    const size_t row = ((size_t)e * 2 + g) * rc, out = (((size_t)step * K + k) * 2 + g) * rc;
    trace_copy<uint4>(d.actions + out, s.actions + row, rc >> 2);
    trace_copy<uint4>(d.ids + out, s.ids + row, rc >> 2);
    trace_copy<uint4>(d.rewards + out, s.rewards + row, rc >> 2);
    if ((rc & 15) == 0) trace_copy<uint4>(d.alive + out, s.alive + row, rc >> 4);
    else trace_copy<uint32_t>(d.alive + out, s.alive + row, rc >> 2);
    if (!lead) return;
    const int64_t* c = d.carry + ((size_t)(step & 1) * K + k) * MFX_TRACE_CARRY;
    const int64_t n0 = c[0], n1 = c[1], ep = c[2], steps0 = c[3];
    const int64_t g0 = s.group_num[(size_t)e * 2], g1 = s.group_num[(size_t)e * 2 + 1];
    const int64_t ep_now = (int64_t)s.stats[(size_t)e * 4], steps_now = s.agent_steps[e];
    unsigned long long err = 0;
    if (steps_now - steps0 != n0 + n1) err |= MFX_TRACE_ERR_STEP;
    if (ep_now != ep && ep_now != ep + 1) err |= MFX_TRACE_ERR_EPISODE;
    if (!trace_count_ok(n0, rc) || !trace_count_ok(n1, rc) || !trace_count_ok(g0, rc) || !trace_count_ok(g1, rc))
        err |= MFX_TRACE_ERR_COUNT;
    if (err) trace_flag(d.state, err);
    head[MFX_TRACE_VALID] = err ? 0 : 1;
    head[MFX_TRACE_N] = n0;
    head[MFX_TRACE_N + 1] = n1;
    head[MFX_TRACE_EP_BEFORE] = ep;
    head[MFX_TRACE_EP_AFTER] = ep_now;
    head[MFX_TRACE_STEPS] = steps_now;
    int64_t* nx = d.carry + ((size_t)((step + 1) & 1) * K + k) * MFX_TRACE_CARRY;
    nx[0] = g0;
    nx[1] = g1;
    nx[2] = ep_now;
    nx[3] = steps_now;
    if (k == 0) d.state[0] = step + 1;
}

static int trace_shape(const char* who, const mfx_trace_src* s, const mfx_trace_dst* d) {
    if (!s || !d) return fail("%s: null argument", who);
    if (s->n_groups != 2) return fail("%s: two groups only, got n_groups = %d", who, s->n_groups);
    if (s->n_envs < 1) return fail("%s: n_envs = %d", who, s->n_envs);
    if (s->rowcap < 4 || (s->rowcap & 3) != 0) return fail("%s: rowcap must be a multiple of 4, got %d", who, s->rowcap);
    if (d->n_watch < 1 || d->n_watch > MFX_TRACE_MAX_ENVS)
        return fail("%s: 1 to %d watched envs, got %d", who, (int)MFX_TRACE_MAX_ENVS, d->n_watch);
    if (d->cap_steps < 1) return fail("%s: cap_steps >= 1, got %lld", who, (long long)d->cap_steps);
    if (!s->group_num || !s->alive || !s->stats || !s->agent_steps || !s->actions || !s->ids || !s->rewards || !s->rng)
        return fail("%s: a rollout buffer is missing", who);
    if (!d->envs || !d->carry || !d->head || !d->actions || !d->ids || !d->rewards || !d->alive || !d->state ||
        !d->seeds)
        return fail("%s: a destination buffer is missing", who);
    if ((((uintptr_t)s->actions | (uintptr_t)s->ids | (uintptr_t)s->rewards | (uintptr_t)d->actions | (uintptr_t)d->ids |
          (uintptr_t)d->rewards | (uintptr_t)d->alive) & 15) != 0)
        return fail("%s: the action, id and reward rows and the record arrays must be 16-byte aligned", who);
    if (((uintptr_t)s->alive & ((s->rowcap & 15) == 0 ? 15 : 3)) != 0)
        return fail("%s: the alive rows must be %d-byte aligned", who, (s->rowcap & 15) == 0 ? 16 : 4);
    if ((((uintptr_t)d->carry | (uintptr_t)d->head | (uintptr_t)d->state | (uintptr_t)s->stats |
          (uintptr_t)s->agent_steps) & 7) != 0)
        return fail("%s: the 8-byte arrays must be 8-byte aligned", who);
    return 0;
}

}  // namespace mfx

using namespace mfx;

extern "C" {

MFX_API int mfx_trace_sizes(int n_watch, int rowcap, int64_t cap_steps, size_t bytes[9]) {
    if (n_watch < 1 || n_watch > MFX_TRACE_MAX_ENVS || rowcap < 4 || (rowcap & 3) != 0 || cap_steps < 1 || !bytes)
        return fail("trace_sizes: bad argument");
    const size_t rows = (size_t)cap_steps * n_watch * 2 * rowcap;
    bytes[0] = (size_t)n_watch * 4;
    bytes[1] = (size_t)2 * n_watch * MFX_TRACE_CARRY * 8;
    bytes[2] = (size_t)cap_steps * n_watch * MFX_TRACE_HEAD * 8;
    bytes[3] = rows * 4;
    bytes[4] = rows * 4;
    bytes[5] = rows * 4;
    bytes[6] = rows;
    bytes[7] = 2 * 8;
    bytes[8] = (size_t)n_watch * 4;
    return 0;
}

MFX_API int mfx_trace_attach(const mfx_trace_src* src, const mfx_trace_dst* dst, const int32_t* h_envs, void* stream) {
    MFX_CHECK(trace_shape("trace_attach", src, dst));
    if (!h_envs) return fail("trace_attach: null argument");
    for (int k = 0; k < dst->n_watch; ++k) {
        if (h_envs[k] < 0 || h_envs[k] >= src->n_envs)
            return fail("trace_attach: watched env %d is outside [0, %d)", h_envs[k], src->n_envs);
        for (int j = 0; j < k; ++j)
            if (h_envs[j] == h_envs[k]) return fail("trace_attach: env %d is watched twice", h_envs[k]);
    }
    hipStream_t st = (hipStream_t)stream;
    MFX_HIP(hipMemcpyAsync(dst->envs, h_envs, sizeof(int32_t) * dst->n_watch, hipMemcpyHostToDevice, st));
    k_trace_attach<<<1, 64, 0, st>>>(*src, *dst);
    MFX_HIP(hipGetLastError());
    return 0;
}

MFX_API int mfx_trace_update(const mfx_trace_src* src, const mfx_trace_dst* dst, int64_t step, void* stream) {
    MFX_CHECK(trace_shape("trace_update", src, dst));
    k_trace_update<<<2 * dst->n_watch, 256, 0, (hipStream_t)stream>>>(*src, *dst, step);
    MFX_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
