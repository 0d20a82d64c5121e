// qnet_bf16.h -- the interface between the Q network's handle (policy_kernels.hip: the C ABI, the packed f32 blob)
// and its bf16 forward (qnet_bf16_kernels.hip), plus the weight-image geometry both sides and the tests read.
//
// Every matrix of the network is used TRANSPOSED, as the A operand of v_mfma_f32_16x16x32_bf16 (rows = output
// units), with the layer input as the B operand (columns = agents, or positions in the convolutions).  Lane l
// (h = l >> 4, c = l & 15) holds A[c][8 h + j] and B[8 h + j][c], j < 8, and D[4 h + r][c], r < 4.  So a lane owns
// units 16 t + 4 h + r of accumulator tile t, and two neighbouring tiles (2 s, 2 s + 1) give it the 8 values of the
// next layer's B operand for k-step s -- if element j of lane group h means
//
//     k = qb16_k(s, h, j) = 32 s + 16 (j >> 2) + 4 h + (j & 3)            (tile parity j >> 2, register j & 3)
//
// EVERY product of the network uses this k order, the ones whose input comes from memory included (Conv1's im2col
// gather, Dense-Emb, Prob-Emb).  The bf16 IMAGE of a [K][16 MT] row-major f32 matrix is, per k-step s (32 rows,
// zero past K) and unit tile t, the 64 lanes' A fragments: 8 bf16 (16 B) at ((s MT + t) 64 + l), element j =
// W[qb16_k(s, l >> 4, j)][16 t + (l & 15)] -- one coalesced 16-B load (or one conflict-free ds_read_b128) per
// MFMA, no address arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "policy_gemm.h"
#include "qsample.h"

namespace mfx {

__host__ __device__ constexpr int qb16_k(int s, int h, int j) { return 32 * s + 16 * (j >> 2) + 4 * h + (j & 3); }
__host__ __device__ constexpr size_t qb16_img_units(int K, int mt) { return (size_t)((K + 31) / 32) * mt * 64; }   // of 16 B

// k_qb16_conv: one wave per agent, 4 agents per workgroup pass, a grid-stride loop over passes from a capped grid.
constexpr int kB16ConvAgents = 4;
constexpr int kB16ConvMaxGrid = 512;
// k_qb16_head: 4 waves x 32 agents (two B tiles per wave share every weight fragment read).
constexpr int kB16HeadWaves = 4, kB16HeadTiles = 2;
constexpr int kB16HeadAgents = kB16HeadWaves * kB16HeadTiles * 16;

// The device view of one network in bf16 mode: the nine images (one allocation) and the f32 biases of the blob.
struct QB16Net {
    const uint4 *w1, *w2, *wd, *we, *wp1, *wp2, *w2d, *wo, *wq;
    const float *b1, *b2, *bd, *be, *bp1, *bp2, *b2d, *bo, *bq;
    int F, A, use_mf;
    int nse, ns2;                   // k-steps of Dense-Emb (ceil(F / 32)) and Dense2 (9, or 10 with mean field)
};

// 16-B units of the nine images of a network with F features.
size_t qb16_total_units(int F, int use_mf);

// Fills net (pointers into img and the blob) and converts the nine matrices on st.  m: the 18 blocks of the packed
// blob in its order (w1 b1 w2 b2 wd bd we be wp1 bp1 wp2 bp2 w2d b2d wo bo wq bq).
hipError_t qb16_build(QB16Net* net, const float* const* m, int F, int A, int use_mf, uint4* img, hipStream_t st);

// One pass (m <= the pass size) of the forward: conv -> act (m x 2,592 bf16) -> head.  The arguments are those of
// k_qnet_conv2 / k_qnet_head (policy_kernels.hip).  qs: the Boltzmann draw (qsample.h) in place of the argmax; null: greedy.
hipError_t qb16_forward(const QB16Net& net, const float* view, size_t view_ld, const float* feat, size_t feat_ld,
                        const void* prob, int prob_f64, size_t prob_ld, QRowMap rm, int m, uint16_t* act_buf,
                        float* q_out, int32_t* act_out, const int32_t* d_n, int n_off, hipStream_t st,
                        const QSample* qs = nullptr);

}  // namespace mfx
