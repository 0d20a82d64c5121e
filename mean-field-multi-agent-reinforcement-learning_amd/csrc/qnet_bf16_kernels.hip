// qnet_bf16_kernels.hip -- the Q network's forward (policy_kernels.hip: ValueNet._construct_net / ValueNet.act) with
// bf16 matrix operands on v_mfma_f32_16x16x32_bf16: the opt-in acting mode precision = 1 of mfx_qnet_set_precision.
//
// NUMERICAL CONTRACT (tests/qnet_bf16_ref.py restates it in numpy; the GPU tests hold the kernels to it)
//   * The operands of every matrix product are rounded to bf16, round-to-nearest-even:
//       - the weight matrices Conv1, Conv2, Dense-Obs, Dense-Emb, Prob-Emb, Dense-Act-Prob, Dense2, Dense-Out and
//         Q-Value, once, when the images are built (set_weights / set_precision);
//       - the view and the feature inputs, f32 -> bf16;
//       - the mean action: f32 -> bf16 on the dense path, f64 -> f32 -> bf16 on the rollout path, whose buffer is
//         float64 (two roundings; the reference applies them the same way);
//       - each layer's activation after bias and ReLU: Conv1 out, Conv2 out, h_obs, h_emb, Prob-Emb out, h_prob,
//         Dense2 out, Dense-Out out.
//   * Products are accumulated in f32 (the MFMA accumulator, which starts at the f32 bias); ReLU is applied in f32.
//   * The Q values are written in f32, unrounded.  Argmax takes the first maximum; the opt-in Boltzmann draw
//     (k_qb16_head<.., true>) is qsample.h's, in f32 on those Q values (q_epilogue: k_qnet_head's).
//   * An agent's result does not depend on its position in the batch or on the batch size: every agent is one
//     column of its MFMAs, accumulated in one fixed order.
//
// Operand layout, the k permutation and the weight images: qnet_bf16.h.  Two kernels, as on the f32 path:
//   k_qb16_conv  one wave per agent (4 per workgroup, a grid-stride loop).  Conv2's 18 weight fragments live in
//                registers for the kernel's life.  The view is staged into the wave's LDS as bf16; Conv1 is an
//                implicit GEMM over 8 position tiles x 2 channel tiles x 2 k-steps (K 63 -> 64, operands gathered
//                from the staged view), its output [121][32] bf16 kept in LDS; Conv2 over 6 position tiles (the rows
//                past position 80 clamped, never stored) x 2 x 9 k-steps, one (ky, kx) block of 32 channels per
//                k-step, a lane's 8 channels one ds_read_b128.  The 2,592 activations go to HBM as bf16 (5 KB per
//                agent), one 16-B store per lane and position tile, in the order the MFMA leaves them -- the order
//                qb16_k gives Dense-Obs's k-step = position.
//   k_qb16_head  4 waves x 32 agents.  Dense-Obs: 81 k-steps, the 16-KB weight chunk of a k-step staged in LDS
//                (double buffered through registers) and shared by the four waves, each fragment read feeding two
//                MFMAs (the wave's two agent tiles); the activations straight from HBM, 16 B per lane and step, a
//                step ahead.  The small layers chain in registers (pack_relu: two accumulator tiles -> one B
//                fragment), their weight fragments read from the images in L2.  Epilogue and row map:
//                k_qnet_head's, the same functions (qsample.h q_epilogue, policy_act.h QRowMap).
// No scratch, no spills (tests/test_policy_bf16_cpu.py); LDS 40 KB (conv) and 32 KB (head) per workgroup, two
// workgroups per CU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "qnet_bf16.h"

namespace mfx {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int kVH = 13, kVW = 13, kNC = 7, kViewF = kVH * kVW * kNC;   // Battle view: 1,183 floats
constexpr int kC1 = 11, kC2 = 9, kCh = 32;
constexpr int kP1 = kC1 * kC1, kP2 = kC2 * kC2;                         // 121, 81 positions
constexpr int kFlat = kP2 * kCh;                                        // 2,592
constexpr int kViewLds = 1184, kC1Lds = kP1 * kCh;                      // bf16 elements per wave
constexpr size_t kConvSmem = (size_t)kB16ConvAgents * (kViewLds + kC1Lds) * 2;
constexpr int kObsUnits = 16 * 64;                                      // 16-B units of one Dense-Obs k-step (16 KB)
constexpr size_t kHeadSmem = (size_t)2 * kObsUnits * 16;

__device__ __forceinline__ f32x4 mfma32(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// two f32 -> two bf16 (RNE) in one register
__device__ __forceinline__ uint32_t pk2(float lo, float hi) {
    const bf16x2 v = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(uint32_t, v);
}

__device__ __forceinline__ uint16_t bf16_bits(float x) { return __builtin_bit_cast(uint16_t, (__bf16)x); }

__device__ __forceinline__ bf16x8 frag(uint4 u) { return __builtin_bit_cast(bf16x8, u); }

__device__ __forceinline__ uint4 pack8(const float* v) {
    return make_uint4(pk2(v[0], v[1]), pk2(v[2], v[3]), pk2(v[4], v[5]), pk2(v[6], v[7]));
}

// relu of two neighbouring accumulator tiles (units 16 (2 s) + 4 h + r and 16 (2 s + 1) + 4 h + r) -> the B fragment
// of the next layer's k-step s (element j = tile parity j >> 2, register j & 3: qb16_k)
__device__ __forceinline__ uint4 pack_relu(f32x4 lo, f32x4 hi) {
    return make_uint4(pk2(fmaxf(lo[0], 0.f), fmaxf(lo[1], 0.f)), pk2(fmaxf(lo[2], 0.f), fmaxf(lo[3], 0.f)),
                      pk2(fmaxf(hi[0], 0.f), fmaxf(hi[1], 0.f)), pk2(fmaxf(hi[2], 0.f), fmaxf(hi[3], 0.f)));
}

__device__ __forceinline__ f32x4 bias4(const float* bias, int t, int h) {
    const float4 b = *reinterpret_cast<const float4*>(bias + 16 * t + 4 * h);
    return {b.x, b.y, b.z, b.w};
}

// One image: a thread per bf16 element (layout: qnet_bf16.h).
__global__ void __launch_bounds__(256) k_qb16_image(const float* __restrict__ src, int K, int N, uint16_t* __restrict__ dst,
                                                    size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int mt = N / 16, j = (int)(i & 7), l = (int)((i >> 3) & 63);
    const size_t q = i >> 9;
    const int t = (int)(q % mt), s = (int)(q / mt);
    const int k = qb16_k(s, l >> 4, j);
    dst[i] = bf16_bits(k < K ? src[(size_t)k * N + 16 * t + (l & 15)] : 0.f);
}

// Offset of im2col column k (ky, kx, ci) in the staged 13 x 13 x 7 view; the pad column 63 reads element 0 against a
// zero weight row.
__device__ __forceinline__ int conv1_koff(int k) {
    if (k >= 63) return 0;
    const int ky = k / 21, kx = (k % 21) / 7, ci = k % 7;
    return (ky * kVW + kx) * kNC + ci;
}

// ------------------------------------------------------------------------------------------ conv
__global__ void __launch_bounds__(64 * kB16ConvAgents, 2)
k_qb16_conv(QB16Net p, const float* __restrict__ view, size_t view_ld, const int32_t* __restrict__ rows, int n,
            uint16_t* __restrict__ out, const int32_t* __restrict__ d_n, int n_off) {
    extern __shared__ __attribute__((aligned(16))) uint16_t csm[];
    if (d_n) n = min(max(*d_n - n_off, 0), n);
    if (n <= 0) return;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, h = lane >> 4, c = lane & 15;
    uint16_t* vs = csm + wid * (kViewLds + kC1Lds);
    uint16_t* c1 = vs + kViewLds;
    bf16x8 w2f[9][2];
#pragma unroll
    for (int b = 0; b < 9; ++b)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) w2f[b][ct] = frag(p.w2[(b * 2 + ct) * 64 + lane]);
    const f32x4 b1v[2] = {bias4(p.b1, 0, h), bias4(p.b1, 1, h)}, b2v[2] = {bias4(p.b2, 0, h), bias4(p.b2, 1, h)};
    uint32_t koff[2][4];                                 // Conv1's im2col offsets of elements 2 j, 2 j + 1, 16 bits each
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            koff[s][j] = (uint32_t)conv1_koff(qb16_k(s, h, 2 * j)) | ((uint32_t)conv1_koff(qb16_k(s, h, 2 * j + 1)) << 16);
    // Conv2's operand offsets: position tile mt, this lane's position (clamped past 80) and channel group
    int cb[6];
#pragma unroll
    for (int mt = 0; mt < 6; ++mt) {
        const int pa = min(mt * 16 + c, kP2 - 1);
        cb[mt] = ((pa / kC2) * kC1 + pa % kC2) * kCh + 8 * h;
    }
    constexpr int kVR = (kViewF + 63) / 64;              // 19 floats of the next agent's view per lane, in flight
    float vr[kVR];
    auto fetch = [&](int i) {
        if (i >= n) return;
        const float* src = view + (size_t)(rows ? rows[i] : i) * view_ld;
#pragma unroll
        for (int j = 0; j < kVR; ++j) {
            const int q = lane + 64 * j;
            vr[j] = q < kViewF ? src[q] : 0.f;
        }
    };
    const int step = gridDim.x * kB16ConvAgents;
    int i = blockIdx.x * kB16ConvAgents + wid;
    fetch(i);
    for (; i < n; i += step) {
#pragma unroll
        for (int j = 0; j < kVR; ++j) {
            const int q = lane + 64 * j;
            if (q < kViewLds) vs[q] = bf16_bits(vr[j]);
        }
        qwave_sync();                                    // the wave's view is whole
        fetch(i + step);
        // ---- Conv1^T: channels on the rows, 16 positions on the lanes' column index; 8 position tiles (121 of 128).
        // Its four weight fragments are re-read per agent (L1 / L2 hits) through a pointer the compiler cannot see
        // through: hoisted out of the agent loop they would sit in 16 registers under Conv2, which has none to spare.
        const uint4* w1p = p.w1;
        asm volatile("" : "+s"(w1p));
        bf16x8 w1f[2][2];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) w1f[s][ct] = frag(w1p[(s * 2 + ct) * 64 + lane]);
#pragma unroll 2
        for (int mt = 0; mt < 8; ++mt) {
            const int pos = mt * 16 + c, pa = min(pos, kP1 - 1);
            const int vb = ((pa / kC1) * kVW + pa % kC1) * kNC;
            f32x4 d0 = b1v[0], d1 = b1v[1];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                uint32_t u[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    u[j] = (uint32_t)vs[vb + (koff[s][j] & 0xffff)] | ((uint32_t)vs[vb + (koff[s][j] >> 16)] << 16);
                const bf16x8 x = frag(make_uint4(u[0], u[1], u[2], u[3]));
                d0 = mfma32(w1f[s][0], x, d0);
                d1 = mfma32(w1f[s][1], x, d1);
            }
            if (pos < kP1) *reinterpret_cast<uint4*>(c1 + pos * kCh + 8 * h) = pack_relu(d0, d1);
        }
        qwave_sync();                                    // conv1's output is whole
        // ---- Conv2^T: 6 position tiles x 2 channel tiles, k-step b = (ky, kx) block b of 32 input channels
        f32x4 acc[6][2];
#pragma unroll
        for (int mt = 0; mt < 6; ++mt) { acc[mt][0] = b2v[0]; acc[mt][1] = b2v[1]; }
#pragma unroll
        for (int b = 0; b < 9; ++b) {
            const int so = ((b / 3) * kC1 + b % 3) * kCh;
#pragma unroll
            for (int mt = 0; mt < 6; ++mt) {
                const bf16x8 x = frag(*reinterpret_cast<const uint4*>(c1 + cb[mt] + so));
                acc[mt][0] = mfma32(w2f[b][0], x, acc[mt][0]);
                acc[mt][1] = mfma32(w2f[b][1], x, acc[mt][1]);
            }
        }
        uint16_t* o = out + (size_t)i * kFlat + 8 * h;
#pragma unroll
        for (int mt = 0; mt < 6; ++mt) {
            const int pos = mt * 16 + c;
            if (pos < kP2) *reinterpret_cast<uint4*>(o + pos * kCh) = pack_relu(acc[mt][0], acc[mt][1]);
        }
        qwave_sync();                                    // (the next agent's stores stay behind this one's reads)
    }
}

// ------------------------------------------------------------------------------------------ head
// acc[a][t] += W^T tile t . b[a] for k-step s of an image of MT unit tiles (fragments from global memory / L2)
template <int MT>
__device__ __forceinline__ void layer_step(f32x4 (&acc)[2][MT], const uint4* __restrict__ img, int s, int lane, uint4 b0,
                                           uint4 b1) {
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const bf16x8 w = frag(img[(s * MT + t) * 64 + lane]);
        acc[0][t] = mfma32(w, frag(b0), acc[0][t]);
        acc[1][t] = mfma32(w, frag(b1), acc[1][t]);
    }
}

template <int MT>
__device__ __forceinline__ void layer_bias(f32x4 (&acc)[2][MT], const float* __restrict__ bias, int h) {
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[0][t] = acc[1][t] = bias4(bias, t, h);
}

// kSample: the Boltzmann draw of qsample.h in place of the argmax (qs; the greedy instantiations never read it).
template <typename PT, bool kSample>
__global__ void __launch_bounds__(64 * kB16HeadWaves, 2)
k_qb16_head(QB16Net p, const uint16_t* __restrict__ act, int n, const float* __restrict__ feat, size_t feat_ld,
            const PT* __restrict__ prob, size_t prob_ld, QRowMap rm, float* __restrict__ q_out,
            int32_t* __restrict__ act_out, const int32_t* __restrict__ d_n, int n_off, QSample qs) {
    extern __shared__ __attribute__((aligned(16))) uint4 hsm[];
    if (d_n) n = min(max(*d_n - n_off, 0), n);
    if ((int)blockIdx.x * kB16HeadAgents >= n) return;            // (uniform: a launch sized for the upper bound)
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h = lane >> 4, c = lane & 15;
    int base[2], ia[2], row[2], env[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        base[a] = ((blockIdx.x * kB16HeadWaves + wid) * kB16HeadTiles + a) * 16;
        ia[a] = min(base[a] + c, n - 1);                 // this lane's agents (clamped: junk columns, never written)
        row[a] = rm.row(ia[a]);
        env[a] = rm.prob_row(row[a]);
    }
    // ---- Dense-Obs^T [256 x 32 agents]: k-step s = conv position s; this lane's 8 activations of it: 16 B at 8 h
    f32x4 hobs[2][16];
    layer_bias<16>(hobs, p.bd, h);
    {
        const uint4* ar[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) ar[a] = reinterpret_cast<const uint4*>(act + (size_t)ia[a] * kFlat) + h;
        uint4 pre[4], bc[2], bn[2];
#pragma unroll
        for (int q = 0; q < 4; ++q) pre[q] = p.wd[q * 256 + tid];
#pragma unroll
        for (int q = 0; q < 4; ++q) hsm[q * 256 + tid] = pre[q];
        bc[0] = ar[0][0];
        bc[1] = ar[1][0];
        bn[0] = bc[0];
        bn[1] = bc[1];
        __syncthreads();
#pragma unroll 1
        for (int s = 0; s < kP2; ++s) {
            const uint4* cur = hsm + (s & 1) * kObsUnits;
            // the next step's weights and activations, in flight (the last step re-reads its own: no branch, so the
            // prefetch stays in registers; the chunk it stores is never read)
            const int sn = min(s + 1, kP2 - 1);
#pragma unroll
            for (int q = 0; q < 4; ++q) pre[q] = p.wd[(size_t)sn * kObsUnits + q * 256 + tid];
            bn[0] = ar[0][4 * sn];
            bn[1] = ar[1][4 * sn];
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const bf16x8 w = frag(cur[t * 64 + lane]);
                hobs[0][t] = mfma32(w, frag(bc[0]), hobs[0][t]);
                hobs[1][t] = mfma32(w, frag(bc[1]), hobs[1][t]);
            }
            uint4* nxt = hsm + ((s + 1) & 1) * kObsUnits;
#pragma unroll
            for (int q = 0; q < 4; ++q) nxt[q * 256 + tid] = pre[q];
            __syncthreads();
            bc[0] = bn[0];
            bc[1] = bn[1];
        }
    }
    uint4 hb[2][8];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int s = 0; s < 8; ++s) hb[a][s] = pack_relu(hobs[a][2 * s], hobs[a][2 * s + 1]);
    // ---- Dense-Emb^T [32 x 32]: the features, f32 -> bf16, gathered in qb16_k order
    f32x4 hemb[2][2];
    layer_bias<2>(hemb, p.be, h);
    {
        const int F = p.F;
#pragma unroll
        for (int s = 0; s < 8; ++s) {                    // (F <= 256; unrolled: the accumulators stay in registers)
            if (s >= p.nse) break;
            uint4 b[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const float* fr = feat + (size_t)row[a] * feat_ld;
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int k = qb16_k(s, h, j);
                    v[j] = k < F ? fr[k] : 0.f;
                }
                b[a] = pack8(v);
            }
            layer_step<2>(hemb, p.we, s, lane, b[0], b[1]);
        }
    }
    // ---- mean field: Prob-Emb^T [64 x 32] (one k-step: A <= 32), Dense-Act-Prob^T [32 x 32]; prob cast to f32 first
    f32x4 hp[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) hp[a][0] = hp[a][1] = {0.f, 0.f, 0.f, 0.f};
    if (p.use_mf) {
        const int A = p.A;
        f32x4 p1[2][4];
        layer_bias<4>(p1, p.bp1, h);
        uint4 b[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const PT* pr = prob + (size_t)env[a] * prob_ld;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = qb16_k(0, h, j);
                v[j] = k < A ? (float)pr[k] : 0.f;
            }
            b[a] = pack8(v);
        }
        layer_step<4>(p1, p.wp1, 0, lane, b[0], b[1]);
        layer_bias<2>(hp, p.bp2, h);
#pragma unroll
        for (int s = 0; s < 2; ++s)
            layer_step<2>(hp, p.wp2, s, lane, pack_relu(p1[0][2 * s], p1[0][2 * s + 1]),
                          pack_relu(p1[1][2 * s], p1[1][2 * s + 1]));
    }
    // ---- Dense2^T [128 x 32] over concat(h_obs 256, h_emb 32[, h_prob 32]): k-steps 0-7, 8[, 9]
    f32x4 d2[2][8];
    layer_bias<8>(d2, p.b2d, h);
#pragma unroll
    for (int s = 0; s < 8; ++s) layer_step<8>(d2, p.w2d, s, lane, hb[0][s], hb[1][s]);
    layer_step<8>(d2, p.w2d, 8, lane, pack_relu(hemb[0][0], hemb[0][1]), pack_relu(hemb[1][0], hemb[1][1]));
    if (p.use_mf) layer_step<8>(d2, p.w2d, 9, lane, pack_relu(hp[0][0], hp[0][1]), pack_relu(hp[1][0], hp[1][1]));
    f32x4 d3[2][4];
    layer_bias<4>(d3, p.bo, h);
#pragma unroll
    for (int s = 0; s < 4; ++s)
        layer_step<4>(d3, p.wo, s, lane, pack_relu(d2[0][2 * s], d2[0][2 * s + 1]), pack_relu(d2[1][2 * s], d2[1][2 * s + 1]));
    f32x4 qv[2][2];
    layer_bias<2>(qv, p.bq, h);
#pragma unroll
    for (int s = 0; s < 2; ++s)
        layer_step<2>(qv, p.wq, s, lane, pack_relu(d3[0][2 * s], d3[0][2 * s + 1]), pack_relu(d3[1][2 * s], d3[1][2 * s + 1]));
    // ---- Q values (the accumulators started at the bias): q_epilogue per agent tile
#pragma unroll
    for (int a = 0; a < 2; ++a)
        q_epilogue<kSample>(qv[a], p.A, base[a] + c, n, row[a], n_off, h, c, rm, q_out, act_out, qs);
}

// K (rows read; the blob pads them with zero rows to a multiple of 4) and unit tiles of the nine matrices
struct ImgShape { int K, mt; };
void shapes(int F, int A, int use_mf, ImgShape* sh) {
    const int Fp = (F + 3) & ~3, Ap = (A + 3) & ~3, Kc = 256 + 32 + (use_mf ? 32 : 0);
    const ImgShape s[9] = {{64, 2}, {288, 2}, {kFlat, 16}, {Fp, 2}, {Ap, 4}, {64, 2}, {Kc, 8}, {128, 4}, {64, 2}};
    for (int k = 0; k < 9; ++k) sh[k] = s[k];
}

}  // namespace

size_t qb16_total_units(int F, int use_mf) {
    ImgShape sh[9];
    shapes(F, 32, use_mf, sh);
    size_t n = 0;
    for (int k = 0; k < 9; ++k) n += qb16_img_units(sh[k].K, sh[k].mt);
    return n;
}

hipError_t qb16_build(QB16Net* net, const float* const* m, int F, int A, int use_mf, uint4* img, hipStream_t st) {
    ImgShape sh[9];
    shapes(F, A, use_mf, sh);
    const uint4** w[9] = {&net->w1, &net->w2, &net->wd, &net->we, &net->wp1, &net->wp2, &net->w2d, &net->wo, &net->wq};
    const float** b[9] = {&net->b1, &net->b2, &net->bd, &net->be, &net->bp1, &net->bp2, &net->b2d, &net->bo, &net->bq};
    uint4* dst = img;
    for (int k = 0; k < 9; ++k) {
        *w[k] = dst;
        *b[k] = m[2 * k + 1];
        const size_t units = qb16_img_units(sh[k].K, sh[k].mt), n = units * 8;
        if (use_mf || (k != 4 && k != 5))                // (Prob-Emb and Dense-Act-Prob: mean field only)
            k_qb16_image<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(m[2 * k], sh[k].K, sh[k].mt * 16,
                                                                       reinterpret_cast<uint16_t*>(dst), n);
        dst += units;
    }
    net->F = F;
    net->A = A;
    net->use_mf = use_mf;
    net->nse = (sh[3].K + 31) / 32;
    net->ns2 = (sh[6].K + 31) / 32;
    return hipGetLastError();
}

hipError_t qb16_forward(const QB16Net& net, const float* view, size_t view_ld, const float* feat, size_t feat_ld,
                        const void* prob, int prob_f64, size_t prob_ld, QRowMap rm, int m, uint16_t* act_buf,
                        float* q_out, int32_t* act_out, const int32_t* d_n, int n_off, hipStream_t st,
                        const QSample* qs) {
    if (m <= 0) return hipSuccess;
    const int cgrid = std::min((m + kB16ConvAgents - 1) / kB16ConvAgents, kB16ConvMaxGrid);
    k_qb16_conv<<<cgrid, 64 * kB16ConvAgents, kConvSmem, st>>>(net, view, view_ld, rm.rows, m, act_buf, d_n, n_off);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int hgrid = (m + kB16HeadAgents - 1) / kB16HeadAgents;
    const QSample s = qs ? *qs : QSample{};
#define MFX_QB16_HEAD(PT, SMP)                                                                                      \
    k_qb16_head<PT, SMP><<<hgrid, 64 * kB16HeadWaves, kHeadSmem, st>>>(                                              \
        net, act_buf, m, feat, feat_ld, static_cast<const PT*>(prob), prob_ld, rm, q_out, act_out, d_n, n_off, s)
    if (qs) { if (prob_f64) MFX_QB16_HEAD(double, true); else MFX_QB16_HEAD(float, true); }
    else { if (prob_f64) MFX_QB16_HEAD(double, false); else MFX_QB16_HEAD(float, false); }
#undef MFX_QB16_HEAD
    return hipGetLastError();
}

}  // namespace mfx
