// acnet_bf16.h -- the interface between the actor-critic network's handle (acnet_kernels.hip: the C ABI, the packed
// f32 blob) and its bf16 acting forward (acnet_bf16_kernels.hip), the weight-image geometry both sides and the tests
// read, and x / 0.1, which the two forwards share (the row map, the uniform and this forward's epilogue: policy_act.h).
//
// As in qnet_bf16.h every matrix is used TRANSPOSED, as the A operand of v_mfma_f32_16x16x32_bf16 (rows = output
// units), the layer input as the B operand (columns = agents): lane l (h = l >> 4, c = l & 15) holds A[c][8 h + j],
// B[8 h + j][c], j < 8, and D[4 h + r][c], r < 4.  Element j of lane group h in k-step s means input
//
//     k = acb16_k(linear, s, h, j) = 32 s + 8 h + j                          linear: the input comes from memory
//                                  = 32 s + 16 (j >> 2) + 4 h + (j & 3)      else: from two accumulator tiles (qb16_k)
//
// The view and the feature layer read 8 consecutive floats per lane (two 16-B loads); the 512-wide dense layer and
// the policy layer take the previous layer's accumulators, tiles 2 s and 2 s + 1, as they lie in the registers.
// The bf16 IMAGE of a [K][16 MT] row-major f32 matrix is, per k-step s (32 rows, zero past K) and unit tile t, the
// 64 lanes' A fragments: 8 bf16 (16 B) at ((s MT + t) 64 + l), element j = W[acb16_k(.., s, l >> 4, j)][16 t + (l & 15)].
// With MT = 16 a k-step is one 16-KB CHUNK; the policy layer (MT = 2) over one half of the dense layer's units, 8
// k-steps, is one chunk as well.  The chunks follow each other in one allocation in the order the kernel consumes
// them -- the view layer, the feature layer, then per output half of the dense layer its 16 k-steps and the policy
// chunk that folds that half into the logits -- so the kernel keeps loading ahead across the layer boundaries.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "policy_act.h"

namespace mfx {

// x / 0.1f, correctly rounded (the reference's dense / 0.1): q = x * 10, one fma residual and one fma correction --
// equal to the IEEE quotient for every f32 |x| >= 2^-100 (checked exhaustively, scripts/micro/div_tenth.c); tinier
// nonzero x take the division.
__device__ __forceinline__ float div_tenth(float x) {
    const float q = x * 10.0f, r = __builtin_fmaf(-q, 0.1f, x);
    float y = __builtin_fmaf(r, 10.0f, q);
    if (__builtin_expect(x != 0.f && __builtin_fabsf(x) < 0x1p-100f, 0)) y = x / 0.1f;
    return y;
}

__host__ __device__ constexpr int acb16_k(bool linear, int s, int h, int j) {
    return linear ? 32 * s + 8 * h + j : 32 * s + 16 * (j >> 2) + 4 * h + (j & 3);
}

// k_acb16: 4 waves x 16 agents per workgroup, one workgroup per 64 rows.
constexpr int kAB16Waves = 4;
constexpr int kAB16Rows = 64;                            // rows per workgroup
constexpr int kAB16H = 256;                              // hidden width: 16 unit tiles, one chunk per k-step
constexpr int kAB16Chunk = 16 * 64;                      // 16-B units of a chunk
constexpr int kAB16PolMT = 2;                            // the policy layer: 32 columns
constexpr int kAB16HalfChunks = 16 + 1;                  // a dense half: its 16 k-steps, then the policy layer over it

__host__ __device__ constexpr int acb16_steps(int K) { return (K + 31) / 32; }
// chunks of a network: view, feature, dense units 0..255 + policy, dense units 256..511 + policy
__host__ __device__ constexpr int acb16_chunks(int V, int F) {
    return acb16_steps(V) + acb16_steps(F) + 2 * kAB16HalfChunks;
}
__host__ __device__ constexpr size_t acb16_total_units(int V, int F) { return (size_t)acb16_chunks(V, F) * kAB16Chunk; }

// The device view of one network in bf16 mode: the chunk sequence and the f32 biases of the blob.
struct ACB16Net {
    const uint4* chunks;
    const float *bv, *be, *bd, *bp;
    int V, F, A;
    int nsv, nse;                   // k-steps of the view layer (ceil(V / 32)) and the feature layer (ceil(F / 32))
};

// Fills net (pointers into img and the blob) and converts the four matrices on st.  w: the 19 blocks of the packed
// blob in its order (acnet_kernels.hip); img: acb16_total_units(V, F) units.
hipError_t acb16_build(ACB16Net* net, const float* const* w, int V, int F, int A, uint4* img, hipStream_t st);

// The policy path of n rows (d_n: the count on the device, n its upper bound): policy_out [n][A] and / or the drawn
// actions, by k_acnet's rule (policy_act.h ac_epilogue).
hipError_t acb16_forward(const ACB16Net& net, const float* view, size_t view_ld, const float* feat, size_t feat_ld,
                         QRowMap rm, int n, const int32_t* d_n, float* policy_out, int32_t* act_out, uint32_t seed,
                         uint32_t step, int group, hipStream_t st);

}  // namespace mfx
