// qsample.h -- the Boltzmann draw over one row of Q values: the opt-in acting mode "boltzmann" of the Q network
// (k_qnet_head, k_qb16_head with kSample) and the stand-alone k_q_sample (qsample_kernels.hip).  One function, three
// users, so the three give the same action and the same weights bit for bit on the same Q row; its weight part
// (q_weights_row) is also the policy of the Boltzmann value target.  q_epilogue, at the end, is the one
// epilogue of the two heads, greedy or sampled.
//
// CONTRACT (include/magent_amd.h; tests/qsample_ref.py restates it in numpy).  For a row q[0..A) of f32 Q
// values -- exactly the values the forward writes to d_q -- and a temperature T (finite, > 0: the host refuses others):
//   weights   m = max_a q[a];  w[a] = expf((q[a] - m) / T): an f32 subtraction and an f32 IEEE division, one rounding
//             each (-ffp-contract=off), then expf
//   draw      tot = the f32 sum of w in ascending action order;  thr = u * tot (one f32 multiply);  the action is the
//             first a whose running f32 sum (same order) satisfies run > thr, and A - 1 if none does
//             (policy_act.h draw_running_sum: the function the actor-critic draw calls)
//   uniform   u = ac_uniform(seed, step, group, row) (policy_act.h: the function the actor-critic draw uses)
//   non-finite rows   a row with any NaN or +-inf entry takes the greedy action: the first maximum over its non-NaN
//             entries (the greedy epilogue's rule), action 0 if every entry is NaN; its weights are 1 at that action
//             and 0 elsewhere.  A rollout never receives an id the draw made from NaNs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "policy_act.h"

namespace mfx {

constexpr int kQSMaxA = kActMaxA;

// The sampling arguments of the Q network's kernels (kSample instantiations; the greedy ones never read them).
struct QSample {
    float T;                        // temperature
    uint32_t seed, step;
    int group;
    float* w;                       // [n][A] weights out, or null
};

// The weights alone (the "weights" and "non-finite rows" lines of the contract): x[0..A) holds the row's Q values on
// entry (entries past A are not read) and its weights on exit.  Returns -1 for a finite row, and the greedy action of
// a row with a non-finite entry (whose weights are 1 there, 0 elsewhere).  Four users: the three draws through
// q_sample_row, and the Boltzmann value target (k_mfq_target_soft, qt_row<kSoft>: DESIGN 7m), which weighs the
// target net's values by exactly the acting policy's weights.  tot: the f32 sum of the weights in ascending action
// order, accumulated as each weight is made (the draw's total; a caller that does not read it pays nothing).
__device__ __forceinline__ int q_weights_row(float (&x)[kQSMaxA], int A, float T, float& tot) {
    float m = -__builtin_huge_valf();
    int bi = -1;
    bool finite = true;
#pragma unroll
    for (int a = 0; a < kQSMaxA; ++a)
        if (a < A) {
            finite = finite && __builtin_fabsf(x[a]) < __builtin_huge_valf();    // (false for NaN and +-inf)
            if (x[a] > m || (x[a] == m && bi < 0)) { m = x[a]; bi = a; }        // first maximum, NaN never taken
        }
    if (!finite) {
        bi = max(bi, 0);
#pragma unroll
        for (int a = 0; a < kQSMaxA; ++a)
            if (a < A) x[a] = a == bi ? 1.f : 0.f;
        return bi;
    }
    tot = 0.f;
#pragma unroll
    for (int a = 0; a < kQSMaxA; ++a)
        if (a < A) { x[a] = expf((x[a] - m) / T); tot += x[a]; }
    return -1;
}

// The Boltzmann mean-field value of one row: v = sum_a f64(w[a]) f64(tq(a)) / sum_a f64(w[a]), both sums
// in ascending action order in float64 (each product of two f32 values is exact there), one f64 division.  w: the
// weights q_weights_row left.  A NaN or infinite tq(a) makes v NaN even where w[a] is 0.
template <class TQ>
__device__ __forceinline__ double q_soft_value(const float (&w)[kQSMaxA], int A, TQ tq) {
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int a = 0; a < kQSMaxA; ++a)
        if (a < A) {
            num += (double)w[a] * (double)tq(a);
            den += (double)w[a];
        }
    return num / den;
}

// x[0..A): the row's Q values on entry (entries past A are not read), its weights on exit.  u: the row's uniform.
__device__ __forceinline__ int q_sample_row(float (&x)[kQSMaxA], int A, float T, float u) {
    float tot;
    const int greedy = q_weights_row(x, A, T, tot);
    return greedy >= 0 ? greedy : draw_running_sum(x, A, tot, u);
}

// The Q epilogue of one agent tile: lane (h, c) holds the finished Q values (bias included) of actions 16 t + 4 h + r
// of compact agent i = the tile's base + c in qv[t][r]; row: the agent's row (rm.row of i clamped below n).  The Q
// values to q_out [n][A]; the action -- argmax (first maximum) over the agent's four lanes, or with kSample the
// Boltzmann draw of qsample.h with the uniform (seed, step, group, the rollout row / the row of the whole dense batch
// n_off + i) and its weights to qs.w -- to the row's slot.
template <bool kSample>
__device__ __forceinline__ void q_epilogue(const f32x4 (&qv)[2], int A, int i, int n, int row, int n_off, int h, int c,
                                           const QRowMap& rm, float* q_out, int32_t* act_out,
                                           const QSample& qs) {
    float best = -__builtin_huge_valf();
    int bi = 1 << 30;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = 16 * t + 4 * h + r;
            if (a < A) {
                const float x = qv[t][r];
                if (q_out && i < n) q_out[(size_t)i * A + a] = x;
                if (!kSample && (x > best || (x == best && a < bi))) { best = x; bi = a; }
            }
        }
    if constexpr (kSample) {
        // the agent's row gathered from its four lanes (every lane of the agent gets it; lane h == 0 uses it): the
        // draw sums the weights in ascending action order
        float x[kQSMaxA];
#pragma unroll
        for (int a = 0; a < kQSMaxA; ++a) x[a] = __shfl(qv[a >> 4][a & 3], 16 * ((a >> 2) & 3) + c);
        if (h == 0 && i < n) {
            bi = q_sample_row(x, A, qs.T, ac_uniform(qs.seed, qs.step, qs.group, rm.rows ? row : n_off + i));
            if (qs.w) {
                float* wr = qs.w + (size_t)i * A;
#pragma unroll
                for (int a = 0; a < kQSMaxA; ++a)
                    if (a < A) wr[a] = x[a];
            }
        }
    } else {
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) {              // lanes c, c + 16, c + 32, c + 48
            const float ob = __shfl_xor(best, o);
            const int oi = __shfl_xor(bi, o);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
    }
    if (h == 0 && i < n && act_out) act_out[rm.slot(row, i)] = bi;
}

// n rows of a Q table [n][A] (2 <= A <= 32): act [n] and / or w [n][A]; row i drawn with (seed, step, group,
// rows ? rows[i] : i).  One lane per row, grid-stride.
hipError_t launch_q_sample(const float* q, const int32_t* rows, int n, int A, float T, uint32_t seed, uint32_t step,
                           int group, float* w, int32_t* act, hipStream_t st);

}  // namespace mfx
