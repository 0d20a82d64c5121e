// policy_act.h -- what an acting kernel does after its last layer, shared by the four of them (k_qnet_head and
// k_qb16_head: policy_kernels.hip, qnet_bf16_kernels.hip; k_acnet and k_acb16: acnet_kernels.hip,
// acnet_bf16_kernels.hip): the row map of a rollout batch and the draw's uniform (all four), the running-sum pick
// (q_sample_row and k_acb16), the clipped softmax policy and the actor-critic epilogue (k_acb16).  The Q heads'
// epilogue, q_epilogue, is in qsample.h, which includes this header.  k_acnet keeps its epilogue written out -- the
// same rule; acnet_kernels.hip says why.  Every operation is f32, in the order written (-ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "policy_gemm.h"

namespace mfx {

constexpr int kActMaxA = 32;                             // actions (the networks' last layer is padded to it)

// Compact agent i -> (view row, action slot, prob row): rows == null: (i, i, i); else row = rows[i]
// = e * rowcap + j of a rollout buffer, action slot e * act_env + act_off + j, prob row e -- or, with prob_by_row
// (a mean action per agent: the neighbourhood mean, neighbor_kernels.hip), the rollout row e * rowcap + j itself.
struct QRowMap {
    const int32_t* rows;
    int rowcap, act_env, act_off;
    int prob_by_row;

    // the view / feature row of compact agent i
    __device__ __forceinline__ int row(int i) const { return rows ? rows[i] : i; }
    // the prob row of a row
    __device__ __forceinline__ int prob_row(int row) const { return rows && !prob_by_row ? row / rowcap : row; }
    // the action slot of a row
    __device__ __forceinline__ size_t slot(int row, int i) const {
        return rows ? (size_t)(row / rowcap) * act_env + act_off + row % rowcap : (size_t)i;
    }
};

__device__ __forceinline__ uint32_t ac_mix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// The uniform of row `row` of group g at step `step` (tests/acnet_ref.py restates it).
__device__ __forceinline__ float ac_uniform(uint32_t seed, uint32_t step, int g, int row) {
    const uint32_t k = seed ^ ac_mix32(step * 0x9E3779B9u + (uint32_t)g * 0x632BE5ABu) ^
                       ac_mix32((uint32_t)row * 0x85EBCA77u + 0x165667B1u);
    return (float)(ac_mix32(k) >> 8) * (1.0f / 16777216.0f);
}

// The pick of every draw: thr = u * tot (one f32 multiply); the first a whose running f32 sum of x[0..a] (ascending)
// satisfies run > thr, and A - 1 if none does (rounding: u * tot at the very top).  tot: the f32 sum of x in the same
// order.
__device__ __forceinline__ int draw_running_sum(const float (&x)[kActMaxA], int A, float tot, float u) {
    const float thr = u * tot;
    float run = 0.f;
    int pick = -1;
#pragma unroll
    for (int a = 0; a < kActMaxA; ++a)
        if (a < A) {
            run += x[a];
            if (pick < 0 && run > thr) pick = a;
        }
    return pick < 0 ? A - 1 : pick;
}

// x[0..A) = clip(softmax(logit(0..A)), 1e-10, 1 - 1e-10); tot: its f32 sum in ascending action order.  logit(a): the
// finished logit of action a (k_acnet adds the policy bias as it loads; k_acb16's accumulators started at it).
template <class LF>
__device__ __forceinline__ void ac_policy_row(LF logit, float (&x)[kActMaxA], int A, float& tot) {
    float m = -__builtin_huge_valf();
#pragma unroll
    for (int a = 0; a < kActMaxA; ++a) {
        x[a] = a < A ? logit(a) : 0.f;
        if (a < A) m = fmaxf(m, x[a]);
    }
    float sum = 0.f;
#pragma unroll
    for (int a = 0; a < kActMaxA; ++a)
        if (a < A) { x[a] = expf(x[a] - m); sum += x[a]; }
    tot = 0.f;
#pragma unroll
    for (int a = 0; a < kActMaxA; ++a)
        if (a < A) { x[a] = fminf(fmaxf(x[a] / sum, 1e-10f), 1.0f - 1e-10f); tot += x[a]; }
}

// The actor-critic epilogue of compact agent i (lane group h == 0, i < n) from its logits: the policy to policy_out
// [n][A], the action drawn with the uniform (seed, step, group, row) to the row's slot (either may be null).
template <class LF>
__device__ __forceinline__ void ac_epilogue(LF logit, int A, int i, int row, const QRowMap& rm,
                                            float* policy_out, int32_t* act_out,
                                            uint32_t seed, uint32_t step, int group) {
    float x[kActMaxA], tot;
    ac_policy_row(logit, x, A, tot);
    if (policy_out) {
        float* po = policy_out + (size_t)i * A;
        for (int a = 0; a < A; ++a) po[a] = x[a];
    }
    if (act_out) act_out[rm.slot(row, i)] = draw_running_sum(x, A, tot, ac_uniform(seed, step, group, row));
}

}  // namespace mfx
