// qtrain_kernels.hip -- one minibatch of ValueNet's training loop (algo/base.py:123-279, algo/q_learning.py: sample ->
// calc_target_q -> train -> update) for the Q network of policy_kernels.hip, hand-written for gfx950, f32 throughout.
//
// The parameters (eval, target), Adam's moments and the gradient are five blobs in the packed layout of
// mfx_qnet_blob_size (18 blocks, K and N padding).  A minibatch is a fixed list of launches on the caller's stream,
// ordered by kernel boundaries only (no grid barrier, no spin wait, no floating-point atomic):
//
//    1 k_qt_rows       validate idx / actions, the row lists (idx, (idx + 1) % n); a bad one sets the sticky error word
//    2 k_qt_gemm<Conv1F>   three forwards at once (blockIdx.y: target(next), eval(next), eval(cur)), activations kept
//    3 k_qt_gemm<Conv2F>
//    4 k_qt_gemm<DObsF>
//    5 k_qt_head       the small layers of the three forwards, one workgroup per row
//    6 k_qt_loss<rule> y (the max rule, or the opt-in Boltzmann value v^MF: mfx_qtrain_set_target), d = y - q[a], dL/dq, back through Q-Value, Dense-Out, Dense2, Dense-Act-Prob (per row); stats
//    7 k_qt_dw_small   dW / db of every small layer and Dense-Obs's bias: one thread per element, rows in order
//    8 k_qt_gemm<DObsB>    da2 = dh . Wd^T, masked by Conv2's ReLU
//    9 k_qt_gemm<DWd>      dWd = a2^T . dh   (K = B)
//   10 k_qt_gemm<Conv2B>   Conv2's transposed convolution, masked by Conv1's ReLU
//   11 k_qt_gemm<DW2>      dW2 over B x 81 positions (+ db2 as a row of ones)
//   12 k_qt_gemm<DW1>      dW1 over B x 121 positions (+ db1 in the padding row's place)
//   13 k_qt_adam       Adam, then target <- (1 - tau) target + tau eval_new; skipped while the error word is set
//
// Every backward kernel reads the eval blob before launch 13 writes it, so each weight read sees the pre-step value.
// k_qt_gemm: one wave per 16 x 16 output tile on v_mfma_f32_16x16x4_f32 (lane l holds A[l & 15][k = l >> 4],
// B[k = l >> 4][l & 15], D[(l >> 4) * 4 + r][l & 15]); a K step is 16 wide, lane group h = l >> 4 taking k = 16 s +
// 4 h + j, j = 0..3 (16-B operand reads where k is contiguous).  K may be split over KS waves of the workgroup, each a
// contiguous range of steps; their partial tiles are summed from LDS in wave order.  So every sum has one fixed
// order, whatever the grid: two runs from the same state give bitwise equal blobs.  Rows, columns and k past the
// operand's extent read as zero and are never stored.
// Padding entries (conv1's 64th K row, `we` rows past F, `wp1` rows past A, `wq` / `bq` columns past A) get a
// gradient of exactly zero by a select in the store, so Adam and the soft update keep them at +0 for ever.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <new>

#include "mfx_common.h"
#include "policy_gemm.h"
#include "qsample.h"
#include "../../include/magent_amd.h"

namespace mfx {
namespace {

constexpr int kTV = 13 * 13 * 7;        // view floats per row
constexpr int kTC1 = 121 * 32;          // conv1 activations per row [11][11][32]
constexpr int kTC2 = 81 * 32;           // conv2 activations per row [9][9][32] = Dense-Obs's input (y, x, c)
constexpr int kTMaxB = 4096;

struct QT {
    // the replay ring's columns, in place
    const float* obs;
    const float* feat;
    const int32_t* act;
    const float* rew;
    const uint8_t* term;
    const uint8_t* mask;
    const float* prob;
    const int64_t* idx;
    int n, B;
    int F, Fp, A, Ap, use_mf, Kc;
    int off[18];
    float *eval, *target, *m, *v, *g;
    int32_t* rows;                       // [2][B]: current rows, next rows (validated)
    int32_t* acts;                       // [B] (validated)
    int32_t* err;                        // code, bad value (lo, hi), minibatches applied
    float *c1, *c2, *hobs, *hemb, *p1, *p2, *d2, *d3, *q;      // [3 jobs][B][...] post-ReLU activations, q [..][32]
    float *dq, *dx3, *dx2, *dhobs, *demb, *dp2, *dp1, *dc2, *dc1;   // [B][...] gradients of the pre-activations
    float* stats;                        // (loss, mean q[a]) of this minibatch
    double gamma;
    float lr_t, sqrt_bc2, omb1, omb2, eps, tau;
    int rule;                            // MFX_QTARGET_MAX / MFX_QTARGET_BOLTZMANN: which k_qt_loss the host launches
    float soft_T;                        // the Boltzmann rule's temperature (finite, > 0: set_target refuses others)
};

// jobs of the forward launches: 0 target(next rows), 1 eval(next rows), 2 eval(current rows)
__device__ __forceinline__ const float* job_w(const QT& t, int job) { return job == 0 ? t.target : t.eval; }
__device__ __forceinline__ const int32_t* job_rows(const QT& t, int job) { return t.rows + (job == 2 ? 0 : t.B); }

__device__ __forceinline__ int conv1_off(int k) {          // im2col column k = (ky, kx, ci) in the 13 x 13 x 7 view
    const int ky = k / 21, kx = (k % 21) / 7, ci = k % 7;
    return (ky * 13 + kx) * 7 + ci;
}

__device__ __forceinline__ void ld4(const float* p, float (&v)[4]) {
    const float4 x = *reinterpret_cast<const float4*>(p);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
}
__device__ __forceinline__ void zero4(float (&v)[4]) { v[0] = v[1] = v[2] = v[3] = 0.f; }

// sum over k < K of x(k) * w(k): eight chains (k mod 8), one rounding per product, combined pairwise -- one fixed order.
template <class FX, class FW>
__device__ __forceinline__ float dot8(int K, FX x, FW w) {
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int k = 0;
    for (; k + 8 <= K; k += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = __builtin_fmaf(x(k + j), w(k + j), s[j]);
    }
#pragma unroll
    for (int j = 0; j < 7; ++j)
        if (k + j < K) s[j] = __builtin_fmaf(x(k + j), w(k + j), s[j]);
    return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
}

// ------------------------------------------------------------------------------------------ 1: rows
__global__ void __launch_bounds__(256) k_qt_rows(QT t) {
    __shared__ int bad;
    if (threadIdx.x == 0) bad = t.B;
    __syncthreads();
    for (int b = threadIdx.x; b < t.B; b += 256) {
        const int64_t i = t.idx[b];
        const bool ok = i >= 0 && i < (int64_t)t.n;
        const int row = ok ? (int)i : 0;
        const int a = t.act[row];                       // (row is inside the ring whatever idx held)
        const bool aok = a >= 0 && a < t.A;
        if (!ok || !aok) atomicMin(&bad, b);
        t.rows[b] = row;
        t.rows[t.B + b] = ok ? (row + 1) % t.n : 0;
        t.acts[b] = ok && aok ? a : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0 && bad < t.B && t.err[0] == 0) {
        const int64_t i = t.idx[bad];
        if (i < 0 || i >= (int64_t)t.n) {
            t.err[1] = (int32_t)(uint32_t)((uint64_t)i & 0xFFFFFFFFu);
            t.err[2] = (int32_t)(uint32_t)((uint64_t)i >> 32);
            t.err[0] = MFX_QTRAIN_BAD_INDEX;
        } else {
            const int a = t.act[(int)i];
            t.err[1] = a;
            t.err[2] = a < 0 ? -1 : 0;
            t.err[0] = MFX_QTRAIN_BAD_ACTION;
        }
    }
}

// ------------------------------------------------------------------------------------------ the tile GEMM
template <int KS, int TPB, class Op>
__global__ void __launch_bounds__(64 * KS * TPB) k_qt_gemm(QT t) {
    __shared__ f32x4 part[KS * TPB][64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, h = lane >> 4, c = lane & 15;
    const int tile = blockIdx.x * TPB + wid / KS, ks = wid % KS, job = blockIdx.y;
    const int tiles_n = Op::N(t) / 16, tiles_m = (Op::M(t) + 15) / 16;
    const bool live = tile < tiles_m * tiles_n;
    const int tm = tile / tiles_n, tn = tile % tiles_n;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        // four accumulator chains (one per j), summed pairwise at the end: a quarter of the sequential chain length
        // (rounding error) and no MFMA waits for the one before it
        f32x4 ch[4] = {acc, acc, acc, acc};
        const int steps = (Op::K(t) + 15) / 16, per = (steps + KS - 1) / KS;
        const int s0 = ks * per, s1 = min(steps, s0 + per);
        const typename Op::A ca = Op::a_ctx(t, job, tm * 16 + c);
        const typename Op::Bc cb = Op::b_ctx(t, job, tn * 16 + c);
#pragma unroll 2
        for (int s = s0; s < s1; ++s) {
            float av[4], bv[4];
            Op::a(t, ca, 16 * s + 4 * h, av);
            Op::b(t, cb, 16 * s + 4 * h, bv);
#pragma unroll
            for (int j = 0; j < 4; ++j) ch[j] = mfma4(av[j], bv[j], ch[j]);
        }
        acc = (ch[0] + ch[1]) + (ch[2] + ch[3]);
    }
    if constexpr (KS > 1) {
        part[wid][lane] = acc;
        __syncthreads();
        if (ks == 0)
            for (int k = 1; k < KS; ++k) acc += part[wid + k][lane];     // wave order: one fixed sum
    }
    if (live && ks == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) Op::store(t, job, tm * 16 + h * 4 + r, tn * 16 + c, acc[r]);
    }
}

struct PtrOk {
    const float* p;
    bool ok;
};

// Conv1 forward: [B * 121 positions] x [32] over K 63 (64th column: padding).
struct Conv1F {
    static __device__ int M(const QT& t) { return t.B * 121; }
    static __device__ int N(const QT&) { return 32; }
    static __device__ int K(const QT&) { return 64; }
    typedef PtrOk A;
    typedef PtrOk Bc;
    static __device__ A a_ctx(const QT& t, int job, int m) {
        A c;
        c.ok = m < t.B * 121;
        const int mm = c.ok ? m : 0, b = mm / 121, pos = mm % 121;
        c.p = t.obs + (size_t)job_rows(t, job)[b] * kTV + ((pos / 11) * 13 + pos % 11) * 7;
        return c;
    }
    static __device__ void a(const QT&, const A& c, int k0, float (&v)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (c.ok && k0 + j < 63) ? c.p[conv1_off(k0 + j)] : 0.f;
    }
    static __device__ Bc b_ctx(const QT& t, int job, int n) { return {job_w(t, job) + t.off[0] + n, true}; }
    static __device__ void b(const QT&, const Bc& c, int k0, float (&v)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = c.p[(k0 + j) * 32];
    }
    static __device__ void store(const QT& t, int job, int m, int n, float x) {
        if (m < t.B * 121) t.c1[((size_t)job * t.B * 121 + m) * 32 + n] = fmaxf(x + job_w(t, job)[t.off[1] + n], 0.f);
    }
};

// Conv2 forward: [B * 81] x [32] over K 288 = (ky, kx, ci).
struct Conv2F {
    static __device__ int M(const QT& t) { return t.B * 81; }
    static __device__ int N(const QT&) { return 32; }
    static __device__ int K(const QT&) { return 288; }
    typedef PtrOk A;
    typedef PtrOk Bc;
    static __device__ A a_ctx(const QT& t, int job, int m) {
        A c;
        c.ok = m < t.B * 81;
        const int mm = c.ok ? m : 0, b = mm / 81, pos = mm % 81;
        c.p = t.c1 + ((size_t)job * t.B + b) * kTC1 + ((pos / 9) * 11 + pos % 9) * 32;
        return c;
    }
    static __device__ void a(const QT&, const A& c, int k0, float (&v)[4]) {
        const int blk = k0 >> 5, ci = k0 & 31;
        if (c.ok) ld4(c.p + ((blk / 3) * 11 + blk % 3) * 32 + ci, v); else zero4(v);
    }
    static __device__ Bc b_ctx(const QT& t, int job, int n) { return {job_w(t, job) + t.off[2] + n, true}; }
    static __device__ void b(const QT&, const Bc& c, int k0, float (&v)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = c.p[(k0 + j) * 32];
    }
    static __device__ void store(const QT& t, int job, int m, int n, float x) {
        if (m < t.B * 81) t.c2[((size_t)job * t.B * 81 + m) * 32 + n] = fmaxf(x + job_w(t, job)[t.off[3] + n], 0.f);
    }
};

// Dense-Obs forward: [B] x [256] over K 2,592.
struct DObsF {
    static __device__ int M(const QT& t) { return t.B; }
    static __device__ int N(const QT&) { return 256; }
    static __device__ int K(const QT&) { return kTC2; }
    typedef PtrOk A;
    typedef PtrOk Bc;
    static __device__ A a_ctx(const QT& t, int job, int m) {
        return {t.c2 + ((size_t)job * t.B + (m < t.B ? m : 0)) * kTC2, m < t.B};
    }
    static __device__ void a(const QT&, const A& c, int k0, float (&v)[4]) {
        if (c.ok) ld4(c.p + k0, v); else zero4(v);
    }
    static __device__ Bc b_ctx(const QT& t, int job, int n) { return {job_w(t, job) + t.off[4] + n, true}; }
    static __device__ void b(const QT&, const Bc& c, int k0, float (&v)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = c.p[(size_t)(k0 + j) * 256];
    }
    static __device__ void store(const QT& t, int job, int m, int n, float x) {
        if (m < t.B) t.hobs[((size_t)job * t.B + m) * 256 + n] = fmaxf(x + job_w(t, job)[t.off[5] + n], 0.f);
    }
};

// Dense-Obs backward to its input: da2 [B] x [2,592] = dh [B][256] . Wd^T, masked by Conv2's ReLU.
struct DObsB {
    static __device__ int M(const QT& t) { return t.B; }
    static __device__ int N(const QT&) { return kTC2; }
    static __device__ int K(const QT&) { return 256; }
    typedef PtrOk A;
    typedef PtrOk Bc;
    static __device__ A a_ctx(const QT& t, int, int m) { return {t.dhobs + (size_t)(m < t.B ? m : 0) * 256, m < t.B}; }
    static __device__ void a(const QT&, const A& c, int k0, float (&v)[4]) {
        if (c.ok) ld4(c.p + k0, v); else zero4(v);
    }
    static __device__ Bc b_ctx(const QT& t, int, int n) { return {t.eval + t.off[4] + (size_t)n * 256, true}; }
    static __device__ void b(const QT&, const Bc& c, int k0, float (&v)[4]) { ld4(c.p + k0, v); }
    static __device__ void store(const QT& t, int, int m, int n, float x) {
        if (m < t.B) t.dc2[(size_t)m * kTC2 + n] = t.c2[((size_t)2 * t.B + m) * kTC2 + n] > 0.f ? x : 0.f;
    }
};

// dWd [2,592] x [256] = a2^T . dh over K = B rows.
struct DWd {
    static __device__ int M(const QT&) { return kTC2; }
    static __device__ int N(const QT&) { return 256; }
    static __device__ int K(const QT& t) { return t.B; }
    typedef PtrOk A;
    typedef PtrOk Bc;
    static __device__ A a_ctx(const QT& t, int, int m) { return {t.c2 + (size_t)2 * t.B * kTC2 + m, true}; }
    static __device__ void a(const QT& t, const A& c, int k0, float (&v)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = k0 + j < t.B ? c.p[(size_t)(k0 + j) * kTC2] : 0.f;
    }
    static __device__ Bc b_ctx(const QT& t, int, int n) { return {t.dhobs + n, true}; }
    static __device__ void b(const QT& t, const Bc& c, int k0, float (&v)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = k0 + j < t.B ? c.p[(size_t)(k0 + j) * 256] : 0.f;
    }
    static __device__ void store(const QT& t, int, int m, int n, float x) { t.g[t.off[4] + (size_t)m * 256 + n] = x; }
};

// Conv2 backward to its input: [B * 121] x [32 ci] over K 288 = (ky, kx, co); position (y, x) of conv1's output takes
// dc2 at (y - ky, x - kx) where that is inside 9 x 9.  Masked by Conv1's ReLU.
struct Conv2B {
    static __device__ int M(const QT& t) { return t.B * 121; }
    static __device__ int N(const QT&) { return 32; }
    static __device__ int K(const QT&) { return 288; }
    struct A {
        const float* p;
        int y, x;
        bool ok;
    };
    typedef PtrOk Bc;
    static __device__ A a_ctx(const QT& t, int, int m) {
        A c;
        c.ok = m < t.B * 121;
        const int mm = c.ok ? m : 0, b = mm / 121, pos = mm % 121;
        c.y = pos / 11;
        c.x = pos % 11;
        c.p = t.dc2 + (size_t)b * kTC2;
        return c;
    }
    static __device__ void a(const QT&, const A& c, int k0, float (&v)[4]) {
        const int blk = k0 >> 5, co = k0 & 31, yy = c.y - blk / 3, xx = c.x - blk % 3;
        if (c.ok && yy >= 0 && yy < 9 && xx >= 0 && xx < 9) ld4(c.p + (yy * 9 + xx) * 32 + co, v); else zero4(v);
    }
    static __device__ Bc b_ctx(const QT& t, int, int n) { return {t.eval + t.off[2] + n * 32, true}; }
    static __device__ void b(const QT&, const Bc& c, int k0, float (&v)[4]) {
        ld4(c.p + (k0 >> 5) * 1024 + (k0 & 31), v);                   // w2[((ky, kx) * 32 + ci) * 32 + co]
    }
    static __device__ void store(const QT& t, int, int m, int n, float x) {
        if (m < t.B * 121) t.dc1[(size_t)m * 32 + n] = t.c1[((size_t)2 * t.B * 121 + m) * 32 + n] > 0.f ? x : 0.f;
    }
};

// dW2 [288 (ky, kx, ci)] x [32 co] over K = B * 81 positions; row 288 is a row of ones: db2.
struct DW2 {
    static __device__ int M(const QT&) { return 289; }
    static __device__ int N(const QT&) { return 32; }
    static __device__ int K(const QT& t) { return t.B * 81; }
    struct A {
        const float* p;
        int kind;                     // 0: a weight row, 1: the bias row, 2: past the end
    };
    typedef PtrOk Bc;
    static __device__ A a_ctx(const QT& t, int, int m) {
        const int mm = m < 288 ? m : 0, blk = mm >> 5;
        return {t.c1 + (size_t)2 * t.B * kTC1 + ((blk / 3) * 11 + blk % 3) * 32 + (mm & 31), m < 288 ? 0 : m == 288 ? 1 : 2};
    }
    static __device__ void a(const QT& t, const A& c, int k0, float (&v)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + j, b = k / 81, pos = k % 81;
            v[j] = (k >= t.B * 81 || c.kind == 2) ? 0.f
                   : c.kind == 1                  ? 1.f
                                                  : c.p[(size_t)b * kTC1 + ((pos / 9) * 11 + pos % 9) * 32];
        }
    }
    static __device__ Bc b_ctx(const QT& t, int, int n) { return {t.dc2 + n, true}; }
    static __device__ void b(const QT& t, const Bc& c, int k0, float (&v)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = k0 + j < t.B * 81 ? c.p[(size_t)(k0 + j) * 32] : 0.f;
    }
    static __device__ void store(const QT& t, int, int m, int n, float x) {
        if (m < 288) t.g[t.off[2] + m * 32 + n] = x;
        else if (m == 288) t.g[t.off[3] + n] = x;
    }
};

// dW1 [64 (ky, kx, ci)] x [32 co] over K = B * 121 positions; the padding row 63 carries ones: db1, and its own
// gradient is stored as zero.
struct DW1 {
    static __device__ int M(const QT&) { return 64; }
    static __device__ int N(const QT&) { return 32; }
    static __device__ int K(const QT& t) { return t.B * 121; }
    struct A {
        int off;
        bool bias;
    };
    typedef PtrOk Bc;
    static __device__ A a_ctx(const QT&, int, int m) { return {conv1_off(m < 63 ? m : 0), m >= 63}; }
    static __device__ void a(const QT& t, const A& c, int k0, float (&v)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + j;
            if (k >= t.B * 121) { v[j] = 0.f; continue; }
            const int b = k / 121, pos = k % 121;
            v[j] = c.bias ? 1.f : t.obs[(size_t)t.rows[b] * kTV + ((pos / 11) * 13 + pos % 11) * 7 + c.off];
        }
    }
    static __device__ Bc b_ctx(const QT& t, int, int n) { return {t.dc1 + n, true}; }
    static __device__ void b(const QT& t, const Bc& c, int k0, float (&v)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = k0 + j < t.B * 121 ? c.p[(size_t)(k0 + j) * 32] : 0.f;
    }
    static __device__ void store(const QT& t, int, int m, int n, float x) {
        if (m < 63) t.g[t.off[0] + m * 32 + n] = x;
        else if (m == 63) { t.g[t.off[0] + 63 * 32 + n] = 0.f; t.g[t.off[1] + n] = x; }
    }
};

// ------------------------------------------------------------------------------------------ 5: the small layers
// One workgroup (128 lanes) per (row, job): lane n sums output unit n over k (dot8's fixed order), one rounding per product.
__global__ void __launch_bounds__(128) k_qt_head(QT t) {
    __shared__ float xc[320], pl[64], y2[128], y3[64];
    const int b = blockIdx.x, job = blockIdx.y, tid = threadIdx.x;
    const size_t rb = (size_t)job * t.B + b;
    const float* w = job_w(t, job);
    const int row = job_rows(t, job)[b];
    for (int k = tid; k < 256; k += 128) xc[k] = t.hobs[rb * 256 + k];
    if (tid < 32) {
        const float* fr = t.feat + (size_t)row * t.F;
        const float* we = w + t.off[6] + tid;
        float s = dot8(t.F, [&](int k) { return fr[k]; }, [&](int k) { return we[k * 32]; });
        s = fmaxf(s + w[t.off[7] + tid], 0.f);
        xc[256 + tid] = s;
        t.hemb[rb * 32 + tid] = s;
    }
    if (t.use_mf) {
        if (tid >= 64) {
            const int n = tid - 64;
            const float* pr = t.prob + (size_t)row * t.A;
            const float* wp = w + t.off[8] + n;
            float s = dot8(t.A, [&](int k) { return pr[k]; }, [&](int k) { return wp[k * 64]; });
            s = fmaxf(s + w[t.off[9] + n], 0.f);
            pl[n] = s;
            t.p1[rb * 64 + n] = s;
        }
        __syncthreads();
        if (tid < 32) {
            const float* wp = w + t.off[10] + tid;
            float s = dot8(64, [&](int k) { return pl[k]; }, [&](int k) { return wp[k * 32]; });
            s = fmaxf(s + w[t.off[11] + tid], 0.f);
            xc[288 + tid] = s;
            t.p2[rb * 32 + tid] = s;
        }
    }
    __syncthreads();
    {
        const float* wp = w + t.off[12] + tid;
        float s = dot8(t.Kc, [&](int k) { return xc[k]; }, [&](int k) { return wp[k * 128]; });
        s = fmaxf(s + w[t.off[13] + tid], 0.f);
        y2[tid] = s;
        t.d2[rb * 128 + tid] = s;
    }
    __syncthreads();
    if (tid < 64) {
        const float* wp = w + t.off[14] + tid;
        float s = dot8(128, [&](int k) { return y2[k]; }, [&](int k) { return wp[k * 64]; });
        s = fmaxf(s + w[t.off[15] + tid], 0.f);
        y3[tid] = s;
        t.d3[rb * 64 + tid] = s;
    }
    __syncthreads();
    if (tid < 32) {
        const float* wp = w + t.off[16] + tid;
        const float s = dot8(64, [&](int k) { return y3[k]; }, [&](int k) { return wp[k * 32]; });
        t.q[rb * 32 + tid] = tid < t.A ? s + w[t.off[17] + tid] : 0.f;
    }
}

// ------------------------------------------------------------------------------------------ 6: target, loss, head backward
// Row b's target y, q[a] and mask.
// kMaxRule: best = np.argmax of the eval net's next-state Q (first maximum; the first NaN wins, as k_mfq_target);
//   y = f32(f64(r) + ((1 - done) * f64(q_t[best])) * gamma).
// kSoftRule (opt-in; k_mfq_target_soft's arithmetic): the weights of qsample.h on the eval net's next-state Q
//   (job 1) at t.soft_T, v = their float64 mean of the target net's next-state Q (job 0);
//   y = f32(f64(r) + ((1 - done) * v) * gamma).
constexpr int kMaxRule = MFX_QTARGET_MAX, kSoftRule = MFX_QTARGET_BOLTZMANN;

template <int kRule>
__device__ __forceinline__ void qt_row(const QT& t, int b, float& y, float& qa, float& mk) {
    const float* qe = t.q + ((size_t)t.B + b) * 32;
    const float* qt = t.q + (size_t)b * 32;
    if constexpr (kRule == kSoftRule) {
        const int row = t.rows[b];
        const double notdone = 1.0 - (t.term[row] ? 1.0 : 0.0);
        float x[kQSMaxA];
#pragma unroll
        for (int a = 0; a < kQSMaxA; ++a) x[a] = a < t.A ? qe[a] : 0.f;
        float tot;
        q_weights_row(x, t.A, t.soft_T, tot);
        const double v = q_soft_value(x, t.A, [&](int a) { return qt[a]; });
        y = (float)((double)t.rew[row] + (notdone * v) * t.gamma);
    } else {
        int best = 0;
        float bv = qe[0];
        if (!isnan(bv)) {
            for (int k = 1; k < t.A; ++k) {
                const float x = qe[k];
                if (isnan(x)) { best = k; break; }
                if (x > bv) { bv = x; best = k; }
            }
        }
        const int row = t.rows[b];
        const double notdone = 1.0 - (t.term[row] ? 1.0 : 0.0);
        y = (float)((double)t.rew[row] + (notdone * (double)qt[best]) * t.gamma);
    }
    const int row = t.rows[b];
    qa = t.q[((size_t)2 * t.B + b) * 32 + t.acts[b]];
    mk = t.mask[row] ? 1.f : 0.f;
}

template <int kRule>
__global__ void __launch_bounds__(128) k_qt_loss(QT t) {
    __shared__ int cnt[128];
    __shared__ float red[2][128];
    __shared__ float s3[64], s2[128], sp2[32];
    const int b = blockIdx.x, tid = threadIdx.x, B = t.B;
    int c = 0;
    for (int i = tid; i < B; i += 128) c += t.mask[t.rows[i]] ? 1 : 0;
    cnt[tid] = c;
    if (b == 0) {                                   // the stats: per-lane partial sums over rows tid, tid + 128, ...
        float l = 0.f, qs = 0.f;
        for (int i = tid; i < B; i += 128) {
            float y, qa, mk;
            qt_row<kRule>(t, i, y, qa, mk);
            const float d = y - qa;
            l += d * d * mk;
            qs += qa;
        }
        red[0][tid] = l;
        red[1][tid] = qs;
    }
    __syncthreads();
    int total = 0;
    for (int i = 0; i < 128; ++i) total += cnt[i];
    const float sm = (float)total;                  // sum of the masks (exact: at most 4,096 ones)
    if (b == 0 && tid == 0) {
        float l = 0.f, qs = 0.f;
        for (int i = 0; i < 128; ++i) { l += red[0][i]; qs += red[1][i]; }
        t.stats[0] = l / sm;
        t.stats[1] = qs / (float)B;
    }
    float y, qa, mk;
    qt_row<kRule>(t, b, y, qa, mk);
    const int a = t.acts[b];
    const float gq = (-2.f * (y - qa) * mk) / sm;   // dL/dq[a]
    const float* w = t.eval;
    if (tid < 32) t.dq[(size_t)b * 32 + tid] = tid == a ? gq : 0.f;
    if (tid < 64) {
        const float x = t.d3[((size_t)2 * B + b) * 64 + tid] > 0.f ? w[t.off[16] + tid * 32 + a] * gq : 0.f;
        s3[tid] = x;
        t.dx3[(size_t)b * 64 + tid] = x;
    }
    __syncthreads();
    {
        const float* wr = w + t.off[14] + tid * 64;
        float s = dot8(64, [&](int n) { return wr[n]; }, [&](int n) { return s3[n]; });
        s = t.d2[((size_t)2 * B + b) * 128 + tid] > 0.f ? s : 0.f;
        s2[tid] = s;
        t.dx2[(size_t)b * 128 + tid] = s;
    }
    __syncthreads();
    for (int k = tid; k < t.Kc; k += 128) {
        const float* wr = w + t.off[12] + k * 128;
        float s = dot8(128, [&](int n) { return wr[n]; }, [&](int n) { return s2[n]; });
        if (k < 256) {
            t.dhobs[(size_t)b * 256 + k] = t.hobs[((size_t)2 * B + b) * 256 + k] > 0.f ? s : 0.f;
        } else if (k < 288) {
            t.demb[(size_t)b * 32 + k - 256] = t.hemb[((size_t)2 * B + b) * 32 + k - 256] > 0.f ? s : 0.f;
        } else {
            s = t.p2[((size_t)2 * B + b) * 32 + k - 288] > 0.f ? s : 0.f;
            sp2[k - 288] = s;
            t.dp2[(size_t)b * 32 + k - 288] = s;
        }
    }
    if (t.use_mf) {
        __syncthreads();
        if (tid < 64) {
            const float* wr = w + t.off[10] + tid * 32;
            const float s = dot8(32, [&](int n) { return wr[n]; }, [&](int n) { return sp2[n]; });
            t.dp1[(size_t)b * 64 + tid] = t.p1[((size_t)2 * B + b) * 64 + tid] > 0.f ? s : 0.f;
        }
    }
}

// ------------------------------------------------------------------------------------------ 7: the small dW / db
// out[k][n] = sum over rows b (dot8's fixed order) of x[b][k] * d[b][n]; x = 1 for a bias.  Entries with k >= kv or n >= nv are
// padding: stored as zero.
struct QSeg {
    const float* x;       // null: a bias
    const float* d;
    float* out;
    int ldx, ldd, K, kv, N, nv, start, ring;      // ring: x is a ring column, indexed by the row list
};
struct QSegs {
    QSeg s[16];
    int count, total;
};

__global__ void __launch_bounds__(256) k_qt_dw_small(QT t, QSegs sg) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= sg.total) return;
    int si = 0;
    for (int i = 1; i < sg.count; ++i)
        if (e >= sg.s[i].start) si = i;
    const QSeg& s = sg.s[si];
    const int local = e - s.start, k = local / s.N, n = local % s.N;
    float sum = 0.f;
    if (k < s.kv && n < s.nv) {
        const float* d = s.d + n;
        auto dv = [&](int b) { return d[(size_t)b * s.ldd]; };
        if (!s.x) sum = dot8(t.B, [](int) { return 1.f; }, dv);
        else if (s.ring) sum = dot8(t.B, [&](int b) { return s.x[(size_t)t.rows[b] * s.ldx + k]; }, dv);
        else sum = dot8(t.B, [&](int b) { return s.x[(size_t)b * s.ldx + k]; }, dv);
    }
    s.out[local] = sum;
}

// ------------------------------------------------------------------------------------------ 13: Adam + soft update
// torch.optim.Adam in its lerp form, each update one fused multiply-add on the old value (one rounding of the result):
// m <- m + (1 - b1)(g - m); v <- v + (1 - b2)(g g - v); p <- p - (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps);
// then target <- (1 - tau) target + tau p as target + tau (p - target).  lr_t = lr / (1 - b1^t) and sqrt_bc2 come from
// the host (computed in double from the step count).  A padding entry has g = m = v = p = target = 0 and keeps +0.
__global__ void __launch_bounds__(256) k_qt_adam(QT t, int n) {
    if (t.err[0] != 0) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) t.err[3] += 1;
    if (i >= n) return;
    const float g = t.g[i], m0 = t.m[i], v0 = t.v[i], tg = t.target[i];
    const float m = __builtin_fmaf(t.omb1, g - m0, m0);
    const float v = __builtin_fmaf(t.omb2, g * g - v0, v0);
    const float p = __builtin_fmaf(-t.lr_t, m / (sqrtf(v) / t.sqrt_bc2 + t.eps), t.eval[i]);
    t.m[i] = m;
    t.v[i] = v;
    t.eval[i] = p;
    t.target[i] = __builtin_fmaf(t.tau, p - tg, tg);
}

// ------------------------------------------------------------------------------------------ the handle
struct QTrain {
    int F, A, use_mf, Fp, Ap, Kc;
    size_t blob_n = 0;
    int off[18];
    float* state = nullptr;            // eval, target, m, v, g: 5 blobs
    int32_t* err = nullptr;
    DevBuf<int32_t> ints;              // rows [2][B], acts [B]
    DevBuf<float> fw, bw;
    float* stats_scratch = nullptr;
    double lr = 1e-4, beta1 = 0.9, beta2 = 0.999, eps = 1e-8, tau = 0.005, gamma = 0.95;
    long long step = 0;
    int rule = MFX_QTARGET_MAX;        // mfx_qtrain_set_target
    float soft_T = 0.1f;
};

constexpr size_t kFwRow = kTC1 + kTC2 + 256 + 32 + 64 + 32 + 128 + 64 + 32;       // per (job, row)
constexpr size_t kBwRow = 32 + 64 + 128 + 256 + 32 + 32 + 64 + kTC2 + kTC1;       // per row

int qt_fill(QTrain* h, const mfx_qtrain_ring* ring, long long n, const int64_t* d_idx, int B, float* d_stats, QT* out) {
    if (B < 1 || B > kTMaxB) return fail("qtrain: a minibatch of %d rows (1..%d)", B, kTMaxB);
    // rows are int32 in the kernels; every row-scaled offset there is 64-bit, so any int32 ring length is taken
    if (n < 1 || n > 0x7FFFFFFFll) return fail("qtrain: a ring of %lld entries (1..2^31 - 1)", n);
    if (!ring || !ring->obs0 || !ring->feat0 || !ring->actions || !ring->rewards || !ring->terminals || !ring->masks ||
        (h->use_mf && !ring->prob))
        return fail("qtrain: a ring column is missing");
    if (!d_idx) return fail("qtrain: no index list");
    try {
        h->ints.ensure((size_t)3 * B);
        h->fw.ensure((size_t)3 * B * kFwRow);
        h->bw.ensure((size_t)B * kBwRow);
    } catch (const HipFailure& f) { return fail("%s", f.what()); }
    QT t{};
    t.obs = ring->obs0; t.feat = ring->feat0; t.act = ring->actions; t.rew = ring->rewards; t.term = ring->terminals;
    t.mask = ring->masks; t.prob = ring->prob; t.idx = d_idx; t.n = (int)n; t.B = B;
    t.F = h->F; t.Fp = h->Fp; t.A = h->A; t.Ap = h->Ap; t.use_mf = h->use_mf; t.Kc = h->Kc;
    for (int k = 0; k < 18; ++k) t.off[k] = h->off[k];
    t.eval = h->state; t.target = h->state + h->blob_n; t.m = h->state + 2 * h->blob_n; t.v = h->state + 3 * h->blob_n;
    t.g = h->state + 4 * h->blob_n;
    t.rows = h->ints.p; t.acts = h->ints.p + 2 * (size_t)B; t.err = h->err;
    float* f = h->fw.p;
    const size_t R = (size_t)3 * B;
    t.c1 = f; f += R * kTC1; t.c2 = f; f += R * kTC2; t.hobs = f; f += R * 256; t.hemb = f; f += R * 32;
    t.p1 = f; f += R * 64; t.p2 = f; f += R * 32; t.d2 = f; f += R * 128; t.d3 = f; f += R * 64; t.q = f;
    f = h->bw.p;
    const size_t b = (size_t)B;
    t.dq = f; f += b * 32; t.dx3 = f; f += b * 64; t.dx2 = f; f += b * 128; t.dhobs = f; f += b * 256;
    t.demb = f; f += b * 32; t.dp2 = f; f += b * 32; t.dp1 = f; f += b * 64; t.dc2 = f; f += b * kTC2; t.dc1 = f;
    t.stats = d_stats ? d_stats : h->stats_scratch;
    t.gamma = h->gamma;
    t.rule = h->rule; t.soft_T = h->soft_T;
    t.omb1 = (float)(1.0 - h->beta1); t.omb2 = (float)(1.0 - h->beta2); t.eps = (float)h->eps; t.tau = (float)h->tau;
    *out = t;
    return 0;
}

void qt_segments(const QT& t, QSegs* sg) {
    int c = 0, total = 0;
    const size_t B = t.B;
    auto add = [&](const float* x, int ldx, int K, int kv, const float* d, int ldd, int N, int nv, float* out, int ring) {
        sg->s[c++] = QSeg{x, d, out, ldx, ldd, K, kv, N, nv, total, ring};
        total += K * N;
    };
    const float *hobs = t.hobs + 2 * B * 256, *hemb = t.hemb + 2 * B * 32, *p1 = t.p1 + 2 * B * 64, *p2 = t.p2 + 2 * B * 32,
                *d2 = t.d2 + 2 * B * 128, *d3 = t.d3 + 2 * B * 64;
    float* g = t.g;
    add(hobs, 256, 256, 256, t.dx2, 128, 128, 128, g + t.off[12], 0);
    add(hemb, 32, 32, 32, t.dx2, 128, 128, 128, g + t.off[12] + 256 * 128, 0);
    if (t.use_mf) add(p2, 32, 32, 32, t.dx2, 128, 128, 128, g + t.off[12] + 288 * 128, 0);
    add(nullptr, 0, 1, 1, t.dx2, 128, 128, 128, g + t.off[13], 0);
    add(d2, 128, 128, 128, t.dx3, 64, 64, 64, g + t.off[14], 0);
    add(nullptr, 0, 1, 1, t.dx3, 64, 64, 64, g + t.off[15], 0);
    add(d3, 64, 64, 64, t.dq, 32, 32, t.A, g + t.off[16], 0);
    add(nullptr, 0, 1, 1, t.dq, 32, 32, t.A, g + t.off[17], 0);
    add(t.feat, t.F, t.Fp, t.F, t.demb, 32, 32, 32, g + t.off[6], 1);
    add(nullptr, 0, 1, 1, t.demb, 32, 32, 32, g + t.off[7], 0);
    add(nullptr, 0, 1, 1, t.dhobs, 256, 256, 256, g + t.off[5], 0);
    if (t.use_mf) {
        add(t.prob, t.A, t.Ap, t.A, t.dp1, 64, 64, 64, g + t.off[8], 1);
        add(nullptr, 0, 1, 1, t.dp1, 64, 64, 64, g + t.off[9], 0);
        add(p1, 64, 64, 64, t.dp2, 32, 32, 32, g + t.off[10], 0);
        add(nullptr, 0, 1, 1, t.dp2, 32, 32, 32, g + t.off[11], 0);
    }
    sg->count = c;
    sg->total = total;
}

template <int KS, int TPB, class Op>
void qt_gemm(const QT& t, int M, int N, int jobs, hipStream_t st) {
    const int tiles = ((M + 15) / 16) * (N / 16);
    k_qt_gemm<KS, TPB, Op><<<dim3((tiles + TPB - 1) / TPB, jobs), 64 * KS * TPB, 0, st>>>(t);
}

// Launches 1-12: the gradient of one minibatch into the handle's gradient blob, and the stats.
int qt_gradient(const QT& t, hipStream_t st) {
    const int B = t.B;
    k_qt_rows<<<1, 256, 0, st>>>(t);
    qt_gemm<1, 4, Conv1F>(t, B * 121, 32, 3, st);
    qt_gemm<1, 4, Conv2F>(t, B * 81, 32, 3, st);
    qt_gemm<4, 1, DObsF>(t, B, 256, 3, st);
    k_qt_head<<<dim3(B, 3), 128, 0, st>>>(t);
    if (t.rule == kSoftRule) k_qt_loss<kSoftRule><<<B, 128, 0, st>>>(t);
    else k_qt_loss<kMaxRule><<<B, 128, 0, st>>>(t);
    QSegs sg;
    qt_segments(t, &sg);
    k_qt_dw_small<<<(sg.total + 255) / 256, 256, 0, st>>>(t, sg);
    qt_gemm<1, 4, DObsB>(t, B, kTC2, 1, st);
    qt_gemm<1, 4, DWd>(t, kTC2, 256, 1, st);
    qt_gemm<1, 4, Conv2B>(t, B * 121, 32, 1, st);
    qt_gemm<16, 1, DW2>(t, 289, 32, 1, st);
    qt_gemm<16, 1, DW1>(t, 64, 32, 1, st);
    MFX_HIP(hipGetLastError());
    return 0;
}

}  // namespace
}  // namespace mfx

using namespace mfx;

extern "C" {

MFX_API int mfx_qtrain_create(int feature, int n_action, int use_mf, void** handle) {
    if (!handle) return fail("qtrain_create: null handle pointer");
    size_t n = 0, off[18];
    MFX_CHECK(mfx_qnet_blob_size(feature, n_action, use_mf, &n, off));
    auto* h = new (std::nothrow) QTrain();
    if (!h) return fail("qtrain: out of memory");
    h->F = feature; h->A = n_action; h->use_mf = use_mf ? 1 : 0;
    h->Fp = (feature + 3) & ~3; h->Ap = (n_action + 3) & ~3; h->Kc = 256 + 32 + (use_mf ? 32 : 0);
    h->blob_n = n;
    for (int k = 0; k < 18; ++k) h->off[k] = (int)off[k];
    if (hipMalloc(&h->state, 5 * n * sizeof(float)) != hipSuccess || hipMalloc(&h->err, 8 * sizeof(int32_t)) != hipSuccess) {
        if (h->state) (void)hipFree(h->state);
        delete h;
        return fail("qtrain: hipMalloc of the state (%zu floats)", 5 * n);
    }
    h->stats_scratch = reinterpret_cast<float*>(h->err + 4);
    MFX_HIP(hipMemset(h->state, 0, 5 * n * sizeof(float)));
    MFX_HIP(hipMemset(h->err, 0, 8 * sizeof(int32_t)));
    MFX_HIP(hipStreamSynchronize(nullptr));      // the zeros are in place before any stream's set_state / run
    *handle = h;
    return 0;
}

MFX_API int mfx_qtrain_destroy(void* handle) {
    auto* h = static_cast<QTrain*>(handle);
    if (!h) return 0;
    if (h->state) (void)hipFree(h->state);
    if (h->err) (void)hipFree(h->err);
    delete h;
    return 0;
}

MFX_API int mfx_qtrain_set_hyper(void* handle, double lr, double beta1, double beta2, double eps, double tau, double gamma) {
    auto* h = static_cast<QTrain*>(handle);
    if (!h) return fail("qtrain: null handle");
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps > 0.0) ||
        !(tau >= 0.0 && tau <= 1.0))
        return fail("qtrain_set_hyper: lr >= 0, beta in [0, 1), eps > 0 (an entry with g = m = v = 0 must divide by it), tau in [0, 1]");
    h->lr = lr; h->beta1 = beta1; h->beta2 = beta2; h->eps = eps; h->tau = tau; h->gamma = gamma;
    return 0;
}

MFX_API int mfx_qtrain_set_target(void* handle, int rule, float temperature) {
    auto* h = static_cast<QTrain*>(handle);
    if (!h) return fail("qtrain: null handle");
    if (rule != MFX_QTARGET_MAX && rule != MFX_QTARGET_BOLTZMANN)
        return fail("qtrain_set_target: rule %d (0 max, 1 boltzmann)", rule);
    if (rule == MFX_QTARGET_BOLTZMANN) {
        if (h->A < 2) return fail("qtrain_set_target: the boltzmann rule takes 2 <= n_action <= 32; the handle has %d", h->A);
        if (!(std::isfinite(temperature) && temperature > 0.f))
            return fail("qtrain_set_target: the temperature must be finite and > 0; got %g", (double)temperature);
        h->soft_T = temperature;
    }
    h->rule = rule;
    return 0;
}

static int qt_which(QTrain* h, int which, size_t n_floats, float** p) {
    if (which < MFX_QTRAIN_EVAL || which > MFX_QTRAIN_ADAM_V) return fail("qtrain: state %d (0 eval, 1 target, 2 m, 3 v)", which);
    if (n_floats != h->blob_n) return fail("qtrain: %zu floats, the layout has %zu", n_floats, h->blob_n);
    *p = h->state + (size_t)which * h->blob_n;
    return 0;
}

MFX_API int mfx_qtrain_set_state(void* handle, int which, const float* d_blob, size_t n_floats, void* stream) {
    auto* h = static_cast<QTrain*>(handle);
    if (!h) return fail("qtrain: null handle");
    float* p;
    MFX_CHECK(qt_which(h, which, n_floats, &p));
    MFX_HIP(hipMemcpyAsync(p, d_blob, n_floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

MFX_API int mfx_qtrain_get_state(void* handle, int which, float* d_out, size_t n_floats, void* stream) {
    auto* h = static_cast<QTrain*>(handle);
    if (!h) return fail("qtrain: null handle");
    float* p;
    MFX_CHECK(qt_which(h, which, n_floats, &p));
    MFX_HIP(hipMemcpyAsync(d_out, p, n_floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

MFX_API int mfx_qtrain_reset_optimizer(void* handle, void* stream) {
    auto* h = static_cast<QTrain*>(handle);
    if (!h) return fail("qtrain: null handle");
    MFX_HIP(hipMemsetAsync(h->state + 2 * h->blob_n, 0, 2 * h->blob_n * sizeof(float), (hipStream_t)stream));
    MFX_HIP(hipMemsetAsync(h->err + 3, 0, sizeof(int32_t), (hipStream_t)stream));
    h->step = 0;
    return 0;
}

MFX_API int mfx_qtrain_step_count(void* handle, long long* t) {
    if (!handle || !t) return fail("qtrain: null handle");
    *t = static_cast<QTrain*>(handle)->step;
    return 0;
}

MFX_API int mfx_qtrain_grads(void* handle, const mfx_qtrain_ring* ring, long long n, const int64_t* d_idx, int B,
                             float* d_grad_blob, float* d_stats, void* stream) {
    auto* h = static_cast<QTrain*>(handle);
    if (!h) return fail("qtrain: null handle");
    QT t;
    MFX_CHECK(qt_fill(h, ring, n, d_idx, B, d_stats, &t));
    MFX_CHECK(qt_gradient(t, (hipStream_t)stream));
    if (d_grad_blob)
        MFX_HIP(hipMemcpyAsync(d_grad_blob, t.g, h->blob_n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

MFX_API int mfx_qtrain_run(void* handle, const mfx_qtrain_ring* ring, long long n, const int64_t* d_idx, int n_batches,
                           int B, float* d_stats, void* stream) {
    auto* h = static_cast<QTrain*>(handle);
    if (!h) return fail("qtrain: null handle");
    if (n_batches < 0) return fail("qtrain_run: %d minibatches", n_batches);
    QT t;
    MFX_CHECK(qt_fill(h, ring, n, d_idx, B, d_stats, &t));
    const int grid = (int)((h->blob_n + 255) / 256);
    for (int i = 0; i < n_batches; ++i) {
        t.idx = d_idx + (size_t)i * B;
        t.stats = d_stats ? d_stats + 2 * (size_t)i : h->stats_scratch;
        MFX_CHECK(qt_gradient(t, (hipStream_t)stream));
        const double s = (double)(h->step + 1);
        t.lr_t = (float)(h->lr / (1.0 - pow(h->beta1, s)));
        t.sqrt_bc2 = (float)sqrt(1.0 - pow(h->beta2, s));
        k_qt_adam<<<grid, 256, 0, (hipStream_t)stream>>>(t, (int)h->blob_n);
        MFX_HIP(hipGetLastError());
        h->step += 1;
    }
    return 0;
}

MFX_API int mfx_qtrain_error(void* handle, int* code, long long* bad_value, void* stream) {
    auto* h = static_cast<QTrain*>(handle);
    if (!h) return fail("qtrain: null handle");
    int32_t e[4];
    MFX_HIP(hipMemcpyAsync(e, h->err, sizeof e, hipMemcpyDeviceToHost, (hipStream_t)stream));
    MFX_HIP(hipStreamSynchronize((hipStream_t)stream));
    *code = e[0];
    *bad_value = (long long)(((uint64_t)(uint32_t)e[2] << 32) | (uint32_t)e[1]);
    h->step = e[3];                       // the minibatches applied: those enqueued after a bad one were skipped
    if (e[0]) MFX_HIP(hipMemsetAsync(h->err, 0, 3 * sizeof(int32_t), (hipStream_t)stream));
    return 0;
}

}  // extern "C"
