// actrain_kernels.hip -- the training step of the actor-critic network (ActorCritic.train / MFAC.train, algo/ac.py:
// one gradient of pg + value_coef vf + ent_coef neg_entropy over all rows of a round, then one Adam step), f32, on the
// device, for the network of acnet_kernels.hip in its packed blob layout.  The contract is in include/magent_amd.h
// (mfx_actrain_*), the float64 restatement in tests/actrain_ref.py.
//
// Rows are taken in place, in chunks of chunk_rows (scratch: the kept activations and the backward intermediates,
// 11 KB per row with the mean field).  Per chunk:
//   forward   every dense layer is one call of k_at_gemm (NN) with bias + ReLU in its store; the activations are kept:
//             X [rows][512 | 544] = concat(h_view, h_emb [, p2]), D [rows][512], P1, VD, the logits Z and the value
//   loss      k_at_loss, one thread per row: the action check, softmax, clamp, the three loss terms, dL/dz (over Z in
//             place) and dL/dv; per-workgroup partial stats, summed in workgroup order by k_at_stats
//   backward  dD by k_at_dd (K = n_action: VALU), dVD by k_at_dvd, then k_at_gemm (NT: the weights read transposed)
//             with the ReLU mask in its store: dX = relu'(X) (dD Wd^T [+ dVD Wvd^T]), dP1
//   dW        k_at_gemm (TN: K = the chunk's rows), K split over blockIdx.z in slices of kATSplit rows, each slice's
//             tile stored to its own partial blob; db by k_at_colsum the same way; k_at_reduce adds the slices in
//             order onto the gradient blob, chunk after chunk (the biases: in double to the end, rounded once)
// then k_at_adam over the blob.  No floating-point atomics and no cross-workgroup waits: every sum has one order
// fixed by (n, chunk_rows, shape).
//
// k_at_gemm is one tiled MFMA GEMM (v_mfma_f32_16x16x4_f32): a workgroup of four waves computes a 128 x (32 WN) tile
// of C, each wave 64 x (16 WN) as 4 x WN accumulator tiles; the operand slabs (32 k x 128 m, 32 k x 32 WN n) go
// through LDS, shared by the waves, the next slab's global loads in flight in registers during the MFMAs.  Operands
// are addressed by two strides each, so the same kernel reads activations, transposed activations and transposed
// weights; the thread-to-element map of a slab follows the contiguous direction (AT / BT).  One accumulator's chain
// runs over k ascending (the MFMA adds its four k in lane-group order), so leaving out inputs that are exactly zero
// -- the view's input support -- leaves every result bit for bit the same.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "mfx_common.h"
#include "policy_gemm.h"
#include "acnet_bf16.h"
#include "../../include/magent_amd.h"

namespace mfx {
namespace {

constexpr int kATBlocks = 19;            // the blob's blocks (acnet_kernels.hip)
constexpr int kATH = 256;
constexpr int kBM = 128, kBK = 32;       // C rows per workgroup, k per staged slab
constexpr int kLdA = kBM + 8;            // slab row stride: an MFMA operand read (4 k-rows x 16) meets every bank twice
constexpr int kATSplit = 512;            // rows per K slice of the weight gradients
constexpr int kATDefaultChunk = 12288;   // rows per chunk: 137 MB of scratch + 24 partial blobs (72 MB at Battle's shape)
constexpr int kATMaxChunk = 262144;

struct GemmArgs {
    const float* A;                      // element (m, k) at A[m' sAm + k' sAk], m' = midx[m], k' = kidx[k] when given
    const float* B;                      // element (k, n) at B[k' sBk + n sBn]
    float* C;                            // element (m, n) at C[m' ldc + n] (+ blockIdx.z csplit: the K slice's blob)
    const int* kidx;
    const int* midx;
    const float* bias;                   // [N], added
    const float* mask;                   // [M][ldmask]: the result where mask > 0, else 0 (ReLU's backward)
    int sAm, sAk, sBk, sBn, ldc, ldmask;
    int M, N, K;
    int addc_n;                          // columns n < addc_n add the value C holds
    int relu, ascale;                    // ascale: A's elements / 0.1
    int chain;                           // 1: one fma chain over all of K (the view layer: its support drops exact-zero
                                         // terms from the chain, which keeps every bit only while the chain is one);
                                         // 0: a chain per 32-k slab, the slabs' sums added in order (a shorter chain:
                                         // less rounding error over a long K)
    int ksplit;                          // > 0: slice blockIdx.z takes k in [z ksplit, (z + 1) ksplit)
    size_t csplit;
};

template <bool AT, bool BT, int WN>
__global__ void __launch_bounds__(256) k_at_gemm(GemmArgs g) {
    constexpr int BN = 32 * WN, LdB = BN + 8, NB = BN / 8;
    __shared__ float As[kBK * kLdA];
    __shared__ float Bs[kBK * LdB];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h = lane >> 4, c = lane & 15;
    const int wm = wid >> 1, wn = wid & 1;
    const int m0 = blockIdx.y * kBM, n0 = blockIdx.x * BN;
    const int kbeg = g.ksplit ? (int)blockIdx.z * g.ksplit : 0;
    const int kend = g.ksplit ? min(g.K, kbeg + g.ksplit) : g.K;
    float* C = g.C + (size_t)blockIdx.z * g.csplit;
    float ra[16], rb[NB];
    auto a_pos = [&](int j, int& mm, int& kk) {
        if (AT) { mm = tid & 127; kk = (tid >> 7) + 2 * j; } else { kk = tid & 31; mm = (tid >> 5) + 8 * j; }
    };
    auto b_pos = [&](int j, int& nn, int& kk) {
        if (BT) { kk = tid & 31; nn = (tid >> 5) + 8 * j; } else { nn = tid % BN; kk = tid / BN + (256 / BN) * j; }
    };
    auto load = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            int mm, kk;
            a_pos(j, mm, kk);
            const int m = m0 + mm, k = k0 + kk;
            float x = 0.f;
            if (m < g.M && k < kend) {
                const int mi = g.midx ? g.midx[m] : m, ki = g.kidx ? g.kidx[k] : k;
                x = g.A[(size_t)mi * g.sAm + (size_t)ki * g.sAk];
                if (g.ascale) x = div_tenth(x);
            }
            ra[j] = x;
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            int nn, kk;
            b_pos(j, nn, kk);
            const int n = n0 + nn, k = k0 + kk;
            float x = 0.f;
            if (n < g.N && k < kend) {
                const int ki = g.kidx ? g.kidx[k] : k;
                x = g.B[(size_t)ki * g.sBk + (size_t)n * g.sBn];
            }
            rb[j] = x;
        }
    };
    f32x4 acc[4][WN], sum[4][WN];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) { acc[i][j] = {0.f, 0.f, 0.f, 0.f}; sum[i][j] = {0.f, 0.f, 0.f, 0.f}; }
    load(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += kBK) {
        __syncthreads();                                 // the slab before this one has been read
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            int mm, kk;
            a_pos(j, mm, kk);
            As[kk * kLdA + mm] = ra[j];
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            int nn, kk;
            b_pos(j, nn, kk);
            Bs[kk * LdB + nn] = rb[j];
        }
        __syncthreads();
        if (k0 + kBK < kend) load(k0 + kBK);             // in flight during this slab's MFMAs
#pragma unroll
        for (int ks = 0; ks < kBK / 4; ++ks) {
            float a[4], b[WN];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = As[(4 * ks + h) * kLdA + wm * 64 + i * 16 + c];
#pragma unroll
            for (int j = 0; j < WN; ++j) b[j] = Bs[(4 * ks + h) * LdB + wn * 16 * WN + j * 16 + c];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = mfma4(a[i], b[j], acc[i][j]);
        }
        if (!g.chain) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) { sum[i][j] += acc[i][j]; acc[i][j] = {0.f, 0.f, 0.f, 0.f}; }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) acc[i][j] += sum[i][j];      // (chain: + 0, exact)
    // lane (h, c) holds rows 4 h + r, column c of each 16 x 16 tile
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + wm * 64 + i * 16 + 4 * h + r;
            if (m >= g.M) continue;
            const int mo = g.midx ? g.midx[m] : m;
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                const int n = n0 + wn * 16 * WN + j * 16 + c;
                if (n >= g.N) continue;
                float v = acc[i][j][r];
                if (g.bias) v += g.bias[n];
                const size_t ci = (size_t)mo * g.ldc + n;
                if (n < g.addc_n) v += C[ci];
                if (g.mask) v = g.mask[(size_t)m * g.ldmask + n] > 0.f ? v : 0.f;
                if (g.relu) v = fmaxf(v, 0.f);
                C[ci] = v;
            }
        }
}

// ------------------------------------------------------------------------------------------ the loss head
// Row i: z -> s = softmax, p = clamp(s, 1e-10f, 1 - 1e-10f), lp = log(p + 1e-6f); the stats' terms; dL/dz over z in
// place (columns past A: 0) and dL/dv.  The action is checked before it selects anything; a bad one sets the sticky
// error word (the first wins) and the row goes on with action 0 -- k_at_adam then applies nothing.
// ADV (mfx_actrain_set_advantage): the policy term's advantage is read from the column advcol instead of
// being formed as R - v; the value term and dL/dv use R - v either way.  ADV = false is the reference's head, its code
// untouched by the other instantiation (profiles/gae_resources.txt).
struct LossArgs {
    float* Z;                 // [rows][32]
    const float* val;
    const int32_t* act;
    const float* ret;
    float* dv;
    float* part;              // [workgroups][4]
    int32_t* err;
    int rows, A;
    float n_rows, value_coef, ent_coef;  // n_rows: all rows of the step (the means' divisor)
};

template <bool ADV>
__global__ void __launch_bounds__(256) k_at_loss(LossArgs a, const float* __restrict__ advcol) {
    __shared__ float red[4][256];
    __shared__ float sk[32][256];                        // the row's softmax, one column per thread
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    float st[4] = {0.f, 0.f, 0.f, 0.f};
    if (i < a.rows) {
        int ac = a.act[i];
        if (ac < 0 || ac >= a.A) {
            if (atomicCAS(&a.err[0], 0, (int)MFX_ACTRAIN_BAD_ACTION) == 0) { a.err[1] = ac; a.err[2] = ac < 0 ? -1 : 0; }
            ac = 0;
        }
        float* z = a.Z + (size_t)i * 32;
        const int A = a.A;
        float mx = -__builtin_huge_valf();
        for (int k = 0; k < A; ++k) mx = fmaxf(mx, z[k]);
        float sum = 0.f;
        for (int k = 0; k < A; ++k) {
            const float e = expf(z[k] - mx);
            sk[k][tid] = e;
            sum += e;
        }
        const float v = a.val[i], R = a.ret[i], adv = ADV ? advcol[i] : R - v;
        float ent = 0.f, lpa = 0.f, dot = 0.f;
        for (int k = 0; k < A; ++k) {
            const float sx = sk[k][tid] / sum;
            const float p = fminf(fmaxf(sx, 1e-10f), 1.0f - 1e-10f);
            const float q = p + 1e-6f, lp = logf(q);
            ent += p * lp;
            float gk = a.ent_coef * (lp + p / q);
            if (k == ac) { lpa = lp; gk += -adv / q; }
            const bool inside = sx >= 1e-10f && sx <= 1.0f - 1e-10f;             // torch's clamp backward
            gk = inside ? gk / a.n_rows : 0.f;
            dot += sx * gk;
            sk[k][tid] = sx;
            z[k] = gk;
        }
        for (int k = 0; k < 32; ++k) z[k] = k < A ? sk[k][tid] * (z[k] - dot) : 0.f;
        a.dv[i] = (-2.f * a.value_coef * (R - v)) / a.n_rows;
        st[0] = -adv * lpa; st[1] = (R - v) * (R - v); st[2] = ent; st[3] = v;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) red[q][tid] = st[q];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {                  // a fixed tree
        if (tid < w) {
#pragma unroll
            for (int q = 0; q < 4; ++q) red[q][tid] += red[q][tid + w];
        }
        __syncthreads();
    }
    if (tid < 4) a.part[(size_t)blockIdx.x * 4 + tid] = red[tid][0];
}

// The PPO head (mfx_actrain_set_ppo): the ADV = true head with the policy term replaced by the clipped
// surrogate of the probability ratio r = exp(lp_a - lp_old[i]).  A row is clipped when its ratio has left [lo, hi] in
// the direction its advantage pushes (strictly: a row on the bound is not clipped); a clipped row's policy term is the
// constant -adv bound and adds nothing to dL/dp.  Two more per-row terms go to part2 [workgroups][2]: clipped ? 1 : 0
// and (r - 1) - d, the k3 estimate of the KL.  lp_new (may be null): lp_a per row.  A sibling of k_at_loss and not a
// third instantiation of it, so that the two existing heads keep their symbols and their code
// (profiles/ppo_resources.txt); everything outside the policy term is that kernel's text.
struct PpoArgs {
    const float* adv;         // the chunk's rows of the three columns
    const float* lp_old;
    float* lp_new;
    float* part2;             // [workgroups][2]
    float lo, hi;
};

__global__ void __launch_bounds__(256) k_at_loss_ppo(LossArgs a, PpoArgs o) {
    __shared__ float red[6][256];
    __shared__ float sk[32][256];                        // the row's softmax, one column per thread
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    float st[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (i < a.rows) {
        int ac = a.act[i];
        if (ac < 0 || ac >= a.A) {
            if (atomicCAS(&a.err[0], 0, (int)MFX_ACTRAIN_BAD_ACTION) == 0) { a.err[1] = ac; a.err[2] = ac < 0 ? -1 : 0; }
            ac = 0;
        }
        float* z = a.Z + (size_t)i * 32;
        const int A = a.A;
        float mx = -__builtin_huge_valf();
        for (int k = 0; k < A; ++k) mx = fmaxf(mx, z[k]);
        float sum = 0.f;
        for (int k = 0; k < A; ++k) {
            const float e = expf(z[k] - mx);
            sk[k][tid] = e;
            sum += e;
        }
        const float v = a.val[i], R = a.ret[i], adv = o.adv[i];
        // the taken action's log-probability first: the ratio decides what the loop below adds at k == ac
        const float sa = sk[ac][tid] / sum;
        const float lpa = logf(fminf(fmaxf(sa, 1e-10f), 1.0f - 1e-10f) + 1e-6f);
        const float d = lpa - o.lp_old[i];
        const float r = expf(d);
        const bool clipped = (adv > 0.f && r > o.hi) || (adv < 0.f && r < o.lo);
        if (o.lp_new) o.lp_new[i] = lpa;
        float ent = 0.f, dot = 0.f;
        for (int k = 0; k < A; ++k) {
            const float sx = sk[k][tid] / sum;
            const float p = fminf(fmaxf(sx, 1e-10f), 1.0f - 1e-10f);
            const float q = p + 1e-6f, lp = logf(q);
            ent += p * lp;
            float gk = a.ent_coef * (lp + p / q);
            if (k == ac && !clipped) gk += -(adv * r) / q;
            const bool inside = sx >= 1e-10f && sx <= 1.0f - 1e-10f;             // torch's clamp backward
            gk = inside ? gk / a.n_rows : 0.f;
            dot += sx * gk;
            sk[k][tid] = sx;
            z[k] = gk;
        }
        for (int k = 0; k < 32; ++k) z[k] = k < A ? sk[k][tid] * (z[k] - dot) : 0.f;
        a.dv[i] = (-2.f * a.value_coef * (R - v)) / a.n_rows;
        st[0] = clipped ? -adv * (adv > 0.f ? o.hi : o.lo) : -adv * r;
        st[1] = (R - v) * (R - v); st[2] = ent; st[3] = v;
        st[4] = clipped ? 1.f : 0.f; st[5] = (r - 1.f) - d;
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) red[q][tid] = st[q];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {                  // a fixed tree
        if (tid < w) {
#pragma unroll
            for (int q = 0; q < 6; ++q) red[q][tid] += red[q][tid + w];
        }
        __syncthreads();
    }
    if (tid < 4) a.part[(size_t)blockIdx.x * 4 + tid] = red[tid][0];
    else if (tid < 6) o.part2[(size_t)blockIdx.x * 2 + (tid - 4)] = red[tid][0];
}

// stats = (pg, value_coef vf, ent_coef neg_entropy, mean value): the workgroups' partials in order, in double
__global__ void k_at_stats(const float* __restrict__ part, int nblocks, double inv_n, float value_coef, float ent_coef,
                           float* __restrict__ stats) {
    const int q = threadIdx.x;
    if (q >= 4) return;
    double s = 0.0;
    for (int b = 0; b < nblocks; ++b) s += (double)part[(size_t)b * 4 + q];
    s *= inv_n;
    if (q == 1) s *= (double)value_coef;
    if (q == 2) s *= (double)ent_coef;
    stats[q] = (float)s;
}

// (clip_frac, approx_kl): the PPO head's two partials per workgroup, in order, in double, over the call's n
__global__ void k_at_ppo_stats(const float* __restrict__ part2, int nblocks, double inv_n, float* __restrict__ out) {
    const int q = threadIdx.x;
    if (q >= 2) return;
    double s = 0.0;
    for (int b = 0; b < nblocks; ++b) s += (double)part2[(size_t)b * 2 + q];
    out[q] = (float)(s * inv_n);
}

// dD[i][j] = D[i][j] > 0 ? (sum_a dz[i][a] Wp[j][a]) / 0.1 (+ dv[i] wval[j][0], AC) : 0
__global__ void __launch_bounds__(256) k_at_dd(const float* __restrict__ D, const float* __restrict__ dz,
                                               const float* __restrict__ wp, const float* __restrict__ dv,
                                               const float* __restrict__ wval, int A, float* __restrict__ dd) {
    const int i = blockIdx.x, j = blockIdx.y * 256 + threadIdx.x;
    const size_t e = (size_t)i * 512 + j;
    float out = 0.f;
    if (D[e] > 0.f) {
        const float* z = dz + (size_t)i * 32;
        const float* w = wp + (size_t)j * 32;
        float s = 0.f;
        for (int a = 0; a < A; ++a) s += z[a] * w[a];
        out = div_tenth(s);
        if (wval) out += dv[i] * wval[(size_t)j * 16];
    }
    dd[e] = out;
}

// dVD[i][j] = VD[i][j] > 0 ? dv[i] wvo[j][0] : 0
__global__ void __launch_bounds__(256) k_at_dvd(const float* __restrict__ VD, const float* __restrict__ dv,
                                                const float* __restrict__ wvo, float* __restrict__ dvd) {
    const int i = blockIdx.x, j = threadIdx.x;
    const size_t e = (size_t)i * 256 + j;
    dvd[e] = VD[e] > 0.f ? dv[i] * wvo[(size_t)j * 16] : 0.f;
}

// The bias gradients: column sums of Y [rows][ld], in double from the rows to the end of the step (a bias block can be
// a single number with cancelling terms).  Thread (column c, quarter q) adds rows q, q + 4, ... of its K slice, the
// quarters are added in order: dpart [slices][kATBias]; k_at_bias_acc adds the slices in order onto dsum [kATBias], chunk
// after chunk; k_at_bias_out rounds once into the gradient blob.  Job j's columns sit at base[j] of the kATBias entries.
constexpr int kATBias = 2048;            // >= 256 + 256 + 512 + 32 + 256 + 16 + 32 + 64 (+ 16)
struct ColJobs {
    const float* y[9];
    int ld[9], n[9], base[9];
    size_t off[9];
};

__global__ void __launch_bounds__(256) k_at_colsum(ColJobs jb, int rows, double* __restrict__ dpart) {
    __shared__ double red[4][64];
    const int job = blockIdx.z, sl = blockIdx.y, c = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + c, n = jb.n[job];
    if ((int)blockIdx.x * 64 >= n) return;               // (uniform)
    const int r1 = min(rows, (sl + 1) * kATSplit);
    double s = 0.0;
    if (col < n) {
        const float* y = jb.y[job] + col;
        const size_t ld = (size_t)jb.ld[job];
        for (int r = sl * kATSplit + q; r < r1; r += 4) s += (double)y[(size_t)r * ld];
    }
    red[q][c] = s;
    __syncthreads();
    if (q == 0 && col < n) dpart[(size_t)sl * kATBias + jb.base[job] + col] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

__global__ void __launch_bounds__(256) k_at_bias_acc(double* __restrict__ dsum, const double* __restrict__ dpart, int used,
                                                    int slices) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= used) return;
    double s = dsum[i];
    for (int k = 0; k < slices; ++k) s += dpart[(size_t)k * kATBias + i];
    dsum[i] = s;
}

__global__ void __launch_bounds__(256) k_at_bias_out(ColJobs jb, const double* __restrict__ dsum, float* __restrict__ grad) {
    const int job = blockIdx.y, col = blockIdx.x * 256 + threadIdx.x;
    if (col < jb.n[job]) grad[jb.off[job] + col] = (float)dsum[jb.base[job] + col];
}

// grad[i] += the slices' partials, in slice order
__global__ void __launch_bounds__(256) k_at_reduce(float* __restrict__ grad, const float* __restrict__ part, size_t n,
                                                   int slices) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = grad[i];
    for (int k = 0; k < slices; ++k) s += part[(size_t)k * n + i];
    grad[i] = s;
}

// torch.optim.Adam in k_qt_adam's form (qtrain_kernels.hip): lr_t = lr / (1 - b1^t) and sqrt_bc2 = sqrt(1 - b2^t) come
// from the host in double.  A padding entry has g = m = v = p = 0 and keeps +0.  Nothing is applied while the error
// word is set; err[3] counts the steps applied.
struct AdamArgs {
    float *p, *m, *v;
    const float* g;
    int32_t* err;
    float omb1, omb2, lr_t, sqrt_bc2, eps;
};

__global__ void __launch_bounds__(256) k_at_adam(AdamArgs t, size_t n) {
    if (t.err[0] != 0) return;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) t.err[3] += 1;
    if (i >= n) return;
    const float g = t.g[i], m0 = t.m[i], v0 = t.v[i];
    const float m = __builtin_fmaf(t.omb1, g - m0, m0);
    const float v = __builtin_fmaf(t.omb2, g * g - v0, v0);
    t.m[i] = m;
    t.v[i] = v;
    t.p[i] = __builtin_fmaf(-t.lr_t, m / (sqrtf(v) / t.sqrt_bc2 + t.eps), t.p[i]);
}

// ------------------------------------------------------------------------------------------ the handle
struct ACTrain {
    int V, F, A, use_mf, LC;
    size_t blob_n = 0;
    size_t off[kATBlocks];
    float* state = nullptr;              // parameters, m, v, g: 4 blobs
    int32_t* err = nullptr;              // [0] code, [1..2] the bad value, [3] steps applied; [4..7] the stats scratch
    int* sup = nullptr;                  // the supported view inputs, ascending
    int supK = 0;
    int chunk = kATDefaultChunk;
    const float* adv = nullptr;          // the advantage column of the next grads / step calls (null: ret - v)
    const float* lp_old = nullptr;       // mfx_actrain_set_ppo: the behaviour log-probabilities (null: no PPO head)
    float* lp_new = nullptr;
    float ppo_lo = 0.f, ppo_hi = 0.f;
    DevBuf<float> pp, pstat;             // the PPO head's partials [workgroups][2]; (clip_frac, approx_kl)
    DevBuf<float> act, part, sp;         // the chunk's activations and intermediates; the K slices' blobs; stats partials
    DevBuf<double> bias;                 // dsum [kATBias], then dpart [slices][kATBias]
    size_t part_slices = 0;
    double lr = 1e-4, beta1 = 0.9, beta2 = 0.999, eps = 1e-8, value_coef = 0.1, ent_coef = 0.08;
    long long step = 0;
};

int at_gemm(hipStream_t st, bool AT, bool BT, bool wide, const GemmArgs& g, int slices = 1) {
    const int BN = wide ? 128 : 32;
    const dim3 grid((g.N + BN - 1) / BN, (g.M + kBM - 1) / kBM, slices);
    if (AT && !BT && wide) k_at_gemm<true, false, 4><<<grid, 256, 0, st>>>(g);
    else if (AT && !BT) k_at_gemm<true, false, 1><<<grid, 256, 0, st>>>(g);
    else if (!AT && BT && wide) k_at_gemm<false, true, 4><<<grid, 256, 0, st>>>(g);
    else if (!AT && BT) k_at_gemm<false, true, 1><<<grid, 256, 0, st>>>(g);
    else if (!AT && !BT && wide) k_at_gemm<false, false, 4><<<grid, 256, 0, st>>>(g);
    else if (!AT && !BT) k_at_gemm<false, false, 1><<<grid, 256, 0, st>>>(g);
    else return fail("actrain: no GEMM form for both operands transposed");
    return 0;
}

// The gradient of the n rows into the handle's gradient blob, and the stats.
int at_gradient(ACTrain* h, const mfx_actrain_rows* rows, long long n, float* d_stats, hipStream_t st) {
    if (n < 1) return fail("actrain: %lld rows (at least 1)", n);
    if (h->lp_old && !h->adv)
        return fail("actrain: d_logp_old is set (mfx_actrain_set_ppo) without an advantage column "
                    "(mfx_actrain_set_advantage): the PPO head reads both");
    if (!rows || !rows->obs || !rows->feat || !rows->act || !rows->ret || (h->use_mf && !rows->prob))
        return fail("actrain: a row column is missing");
    const int cmax = (int)std::min<long long>(n, h->chunk);
    const int smax = (cmax + kATSplit - 1) / kATSplit;
    const int LC = h->LC, mf = h->use_mf, A = h->A, V = h->V, F = h->F;
    const size_t per_row = (size_t)2 * LC + 2 * 512 + 32 + 2 + (mf ? 64 + 256 + 256 + 64 : 0);
    const size_t nblocks = (size_t)((n + 255) / 256) + (size_t)((n + h->chunk - 1) / h->chunk);
    try {
        h->act.ensure(per_row * cmax);
        h->sp.ensure(nblocks * 4);
        if (h->lp_old) {
            h->pp.ensure(nblocks * 2);
            h->pstat.ensure(2);
        }
        h->bias.ensure((size_t)(1 + smax) * kATBias);
        if ((size_t)smax > h->part_slices) {
            h->part.ensure((size_t)smax * h->blob_n);
            h->part_slices = (size_t)smax;
            // entries no kernel writes (padding, unsupported view rows) are read by k_at_reduce: zero for good
            MFX_HIP(hipMemsetAsync(h->part.p, 0, h->part.n * sizeof(float), st));
        }
    } catch (const HipFailure& f) { return fail("%s", f.what()); }
    const size_t cm = (size_t)cmax;
    float* f = h->act.p;
    float* X = f; f += cm * LC;
    float* D = f; f += cm * 512;
    float* Z = f; f += cm * 32;
    float* VAL = f; f += cm;
    float* DV = f; f += cm;
    float* DX = f; f += cm * LC;
    float* DD = f; f += cm * 512;
    float *P1 = nullptr, *VD = nullptr, *DVD = nullptr, *DP1 = nullptr;
    if (mf) { P1 = f; f += cm * 64; VD = f; f += cm * 256; DVD = f; f += cm * 256; DP1 = f; f += cm * 64; }
    float* par = h->state;
    float* grad = h->state + 3 * h->blob_n;
    float* part = h->part.p;
    auto W = [&](int k) { return par + h->off[k]; };
    auto G = [&](int k) { return part + h->off[k]; };
    MFX_HIP(hipMemsetAsync(grad, 0, h->blob_n * sizeof(float), st));
    double* dsum = h->bias.p;
    double* dpart = h->bias.p + kATBias;
    MFX_HIP(hipMemsetAsync(dsum, 0, kATBias * sizeof(double), st));
    ColJobs jb{};
    int nj = 0, nbias = 0;
    const float n_rows = (float)n;                       // (exact up to 2^24 rows; rounded beyond)
    size_t block0 = 0;
    for (long long r0 = 0; r0 < n; r0 += h->chunk) {
        const int m = (int)std::min<long long>(h->chunk, n - r0);
        const int slices = (m + kATSplit - 1) / kATSplit;
        const float* obs = rows->obs + (size_t)r0 * V;
        const float* feat = rows->feat + (size_t)r0 * F;
        const float* prob = mf ? rows->prob + (size_t)r0 * A : nullptr;
        // ---- forward (NN): C = relu(A B + bias)
        auto fwd = [&](const float* a, int lda, const float* b, int ldb, float* c, int ldc, int N, int K, const float* bias,
                       int relu, bool wide, const int* kidx = nullptr, int ascale = 0, int chain = 0) {
            GemmArgs g{};
            g.chain = chain;
            g.A = a; g.sAm = lda; g.sAk = 1; g.B = b; g.sBk = ldb; g.sBn = 1; g.C = c; g.ldc = ldc;
            g.M = m; g.N = N; g.K = K; g.bias = bias; g.relu = relu; g.kidx = kidx; g.ascale = ascale;
            return at_gemm(st, false, false, wide, g);
        };
        MFX_CHECK(fwd(obs, V, W(0), kATH, X, LC, kATH, h->sup ? h->supK : V, W(1), 1, true, h->sup, 0, 1));
        MFX_CHECK(fwd(feat, F, W(2), kATH, X + kATH, LC, kATH, F, W(3), 1, true));
        MFX_CHECK(fwd(X, LC, W(4), kATH, D, 512, kATH, 512, W(6), 1, true));
        MFX_CHECK(fwd(X, LC, W(5), kATH, D + kATH, 512, kATH, 512, W(6) + kATH, 1, true));
        MFX_CHECK(fwd(D, 512, W(7), 32, Z, 32, A, 512, W(8), 0, false, nullptr, 1));
        if (mf) {
            MFX_CHECK(fwd(prob, A, W(11), 64, P1, 64, 64, A, W(12), 1, false));
            MFX_CHECK(fwd(P1, 64, W(13), 32, X + 512, LC, 32, 64, W(14), 1, false));
            MFX_CHECK(fwd(X, LC, W(15), kATH, VD, kATH, kATH, 544, W(16), 1, true));
            MFX_CHECK(fwd(VD, kATH, W(17), 16, VAL, 1, 1, kATH, W(18), 0, false));
        } else {
            MFX_CHECK(fwd(D, 512, W(9), 16, VAL, 1, 1, 512, W(10), 0, false));
        }
        // ---- loss head
        const int lb = (m + 255) / 256;
        LossArgs la{Z, VAL, rows->act + r0, rows->ret + r0, DV, h->sp.p + block0 * 4, h->err, m, A, n_rows,
                    (float)h->value_coef, (float)h->ent_coef};
        if (h->lp_old) {
            const PpoArgs po{h->adv + r0, h->lp_old + r0, h->lp_new ? h->lp_new + r0 : nullptr, h->pp.p + block0 * 2,
                             h->ppo_lo, h->ppo_hi};
            k_at_loss_ppo<<<lb, 256, 0, st>>>(la, po);
        } else if (h->adv) k_at_loss<true><<<lb, 256, 0, st>>>(la, h->adv + r0);
        else k_at_loss<false><<<lb, 256, 0, st>>>(la, nullptr);
        block0 += (size_t)lb;
        // ---- row-side backward (NT): C = mask (A W^T [+ C])
        k_at_dd<<<dim3(m, 2), 256, 0, st>>>(D, Z, W(7), DV, mf ? nullptr : W(9), A, DD);
        auto bwd = [&](const float* a, int lda, const float* w, int ldw, float* c, int ldc, int N, int K, int addc_n,
                       const float* mask, int ldmask, bool wide) {
            GemmArgs g{};
            g.A = a; g.sAm = lda; g.sAk = 1; g.B = w; g.sBk = 1; g.sBn = ldw; g.C = c; g.ldc = ldc;
            g.M = m; g.N = N; g.K = K; g.addc_n = addc_n; g.mask = mask; g.ldmask = ldmask;
            return at_gemm(st, false, true, wide, g);
        };
        MFX_CHECK(bwd(DD, 512, W(4), kATH, DX, LC, 512, kATH, 0, nullptr, 0, true));
        MFX_CHECK(bwd(DD + kATH, 512, W(5), kATH, DX, LC, 512, kATH, 512, mf ? nullptr : X, LC, true));
        if (mf) {
            k_at_dvd<<<m, 256, 0, st>>>(VD, DV, W(17), DVD);
            MFX_CHECK(bwd(DVD, kATH, W(15), kATH, DX, LC, 544, kATH, 512, X, LC, true));
            MFX_CHECK(bwd(DX + 512, LC, W(13), 32, DP1, 64, 64, 32, 0, P1, 64, false));
        }
        // ---- weight gradients (TN, K = the chunk's rows, sliced): partial blobs
        auto dw = [&](const float* x, int ldx, int M, const float* dy, int ldd, int N, float* c, int ldc, bool wide,
                      const int* midx = nullptr, int ascale = 0) {
            GemmArgs g{};
            g.A = x; g.sAm = 1; g.sAk = ldx; g.B = dy; g.sBk = ldd; g.sBn = 1; g.C = c; g.ldc = ldc;
            g.M = M; g.N = N; g.K = m; g.midx = midx; g.ascale = ascale; g.ksplit = kATSplit; g.csplit = h->blob_n;
            return at_gemm(st, true, false, wide, g, slices);
        };
        MFX_CHECK(dw(obs, V, h->sup ? h->supK : V, DX, LC, kATH, G(0), kATH, true, h->sup));
        MFX_CHECK(dw(feat, F, F, DX + kATH, LC, kATH, G(2), kATH, true));
        MFX_CHECK(dw(X, LC, 512, DD, 512, kATH, G(4), kATH, true));
        MFX_CHECK(dw(X, LC, 512, DD + kATH, 512, kATH, G(5), kATH, true));
        MFX_CHECK(dw(D, 512, 512, Z, 32, A, G(7), 32, false, nullptr, 1));
        nj = nbias = 0;
        auto col = [&](const float* y, int ld, int ncol, int k) {
            jb.y[nj] = y; jb.ld[nj] = ld; jb.n[nj] = ncol; jb.off[nj] = h->off[k]; jb.base[nj] = nbias;
            nbias += ncol;
            ++nj;
        };
        col(DX, LC, kATH, 1);
        col(DX + kATH, LC, kATH, 3);
        col(DD, 512, 512, 6);
        col(Z, 32, A, 8);
        if (mf) {
            MFX_CHECK(dw(X, LC, 544, DVD, kATH, kATH, G(15), kATH, true));
            MFX_CHECK(dw(VD, kATH, kATH, DV, 1, 1, G(17), 16, false));
            MFX_CHECK(dw(P1, 64, 64, DX + 512, LC, 32, G(13), 32, false));
            MFX_CHECK(dw(prob, A, A, DP1, 64, 64, G(11), 64, false));
            col(DVD, kATH, kATH, 16);
            col(DV, 1, 1, 18);
            col(DX + 512, LC, 32, 14);
            col(DP1, 64, 64, 12);
        } else {
            MFX_CHECK(dw(D, 512, 512, DV, 1, 1, G(9), 16, false));
            col(DV, 1, 1, 10);
        }
        k_at_colsum<<<dim3(8, slices, nj), 256, 0, st>>>(jb, m, dpart);
        k_at_bias_acc<<<(nbias + 255) / 256, 256, 0, st>>>(dsum, dpart, nbias, slices);
        k_at_reduce<<<(unsigned)((h->blob_n + 255) / 256), 256, 0, st>>>(grad, part, h->blob_n, slices);
    }
    k_at_bias_out<<<dim3(2, nj), 256, 0, st>>>(jb, dsum, grad);
    k_at_stats<<<1, 64, 0, st>>>(h->sp.p, (int)block0, 1.0 / (double)n, (float)h->value_coef, (float)h->ent_coef,
                                 d_stats ? d_stats : reinterpret_cast<float*>(h->err + 4));
    if (h->lp_old) k_at_ppo_stats<<<1, 64, 0, st>>>(h->pp.p, (int)block0, 1.0 / (double)n, h->pstat.p);
    MFX_HIP(hipGetLastError());
    return 0;
}

int at_which(ACTrain* h, int which, size_t n_floats, float** p) {
    if (which < MFX_ACTRAIN_PARAMS || which > MFX_ACTRAIN_ADAM_V) return fail("actrain: state %d (0 parameters, 1 m, 2 v)", which);
    if (n_floats != h->blob_n) return fail("actrain: %zu floats, the layout has %zu", n_floats, h->blob_n);
    *p = h->state + (size_t)which * h->blob_n;
    return 0;
}

}  // namespace
}  // namespace mfx

using namespace mfx;

extern "C" {

MFX_API int mfx_actrain_create(int view_floats, int feature, int n_action, int use_mf, void** handle) {
    if (!handle) return fail("actrain_create: null handle pointer");
    size_t n = 0, off[kATBlocks];
    MFX_CHECK(mfx_acnet_blob_size(view_floats, feature, n_action, use_mf, &n, off));
    auto* h = new (std::nothrow) ACTrain();
    if (!h) return fail("actrain: out of memory");
    h->V = view_floats; h->F = feature; h->A = n_action; h->use_mf = use_mf ? 1 : 0; h->LC = use_mf ? 544 : 512;
    h->blob_n = n;
    for (int k = 0; k < kATBlocks; ++k) h->off[k] = off[k];
    if (hipMalloc(&h->state, 4 * n * sizeof(float)) != hipSuccess || hipMalloc(&h->err, 8 * sizeof(int32_t)) != hipSuccess) {
        if (h->state) (void)hipFree(h->state);
        delete h;
        return fail("actrain: hipMalloc of the state (%zu floats)", 4 * n);
    }
    MFX_HIP(hipMemset(h->state, 0, 4 * n * sizeof(float)));
    MFX_HIP(hipMemset(h->err, 0, 8 * sizeof(int32_t)));
    MFX_HIP(hipStreamSynchronize(nullptr));      // the zeros are in place before any stream's set_state / step
    *handle = h;
    return 0;
}

MFX_API int mfx_actrain_destroy(void* handle) {
    auto* h = static_cast<ACTrain*>(handle);
    if (!h) return 0;
    if (h->state) (void)hipFree(h->state);
    if (h->err) (void)hipFree(h->err);
    if (h->sup) (void)hipFree(h->sup);
    delete h;
    return 0;
}

MFX_API int mfx_actrain_set_hyper(void* handle, double lr, double beta1, double beta2, double eps, double value_coef,
                                  double ent_coef) {
    auto* h = static_cast<ACTrain*>(handle);
    if (!h) return fail("actrain: null handle");
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps > 0.0))
        return fail("actrain_set_hyper: lr >= 0, beta in [0, 1), eps > 0 (an entry with g = m = v = 0 must divide by it)");
    h->lr = lr; h->beta1 = beta1; h->beta2 = beta2; h->eps = eps; h->value_coef = value_coef; h->ent_coef = ent_coef;
    return 0;
}

MFX_API int mfx_actrain_set_state(void* handle, int which, const float* d_blob, size_t n_floats, void* stream) {
    auto* h = static_cast<ACTrain*>(handle);
    if (!h) return fail("actrain: null handle");
    float* p;
    MFX_CHECK(at_which(h, which, n_floats, &p));
    MFX_HIP(hipMemcpyAsync(p, d_blob, n_floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

MFX_API int mfx_actrain_get_state(void* handle, int which, float* d_out, size_t n_floats, void* stream) {
    auto* h = static_cast<ACTrain*>(handle);
    if (!h) return fail("actrain: null handle");
    float* p;
    MFX_CHECK(at_which(h, which, n_floats, &p));
    MFX_HIP(hipMemcpyAsync(d_out, p, n_floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

MFX_API int mfx_actrain_reset_optimizer(void* handle, void* stream) {
    auto* h = static_cast<ACTrain*>(handle);
    if (!h) return fail("actrain: null handle");
    MFX_HIP(hipMemsetAsync(h->state + h->blob_n, 0, 2 * h->blob_n * sizeof(float), (hipStream_t)stream));
    MFX_HIP(hipMemsetAsync(h->err + 3, 0, sizeof(int32_t), (hipStream_t)stream));
    h->step = 0;
    return 0;
}

MFX_API int mfx_actrain_step_count(void* handle, long long* t) {
    if (!handle || !t) return fail("actrain: null handle");
    *t = static_cast<ACTrain*>(handle)->step;
    return 0;
}

MFX_API int mfx_actrain_set_input_support(void* handle, const uint8_t* mask, int n, void* stream) {
    auto* h = static_cast<ACTrain*>(handle);
    if (!h) return fail("actrain: null handle");
    if (mask && n != h->V) return fail("actrain_set_input_support: %d entries, the view has %d floats", n, h->V);
    MFX_HIP(hipStreamSynchronize((hipStream_t)stream));          // (launches that read the list being replaced)
    if (h->sup) (void)hipFree(h->sup);
    h->sup = nullptr;
    h->supK = 0;
    // the rows of wv's gradient that the new support leaves unwritten must read as zero in every slice's blob
    if (h->part.p) MFX_HIP(hipMemsetAsync(h->part.p, 0, h->part.n * sizeof(float), (hipStream_t)stream));
    if (!mask) return 0;
    std::vector<int> idx;
    for (int k = 0; k < n; ++k)
        if (mask[k]) idx.push_back(k);
    if (idx.empty()) idx.push_back(0);                           // (an all-zero view: one input, zero by the contract)
    if (hipMalloc(&h->sup, idx.size() * sizeof(int)) != hipSuccess) return fail("actrain_set_input_support: hipMalloc");
    MFX_HIP(hipMemcpy(h->sup, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice));
    h->supK = (int)idx.size();
    return 0;
}

MFX_API int mfx_actrain_set_chunk_rows(void* handle, int chunk_rows) {
    auto* h = static_cast<ACTrain*>(handle);
    if (!h) return fail("actrain: null handle");
    if (chunk_rows == 0) chunk_rows = kATDefaultChunk;
    if (chunk_rows < 1 || chunk_rows > kATMaxChunk) return fail("actrain_set_chunk_rows: %d (1..%d; 0: the default, %d)", chunk_rows, kATMaxChunk, kATDefaultChunk);
    h->chunk = chunk_rows;
    return 0;
}

MFX_API int mfx_actrain_set_advantage(void* handle, const float* d_adv) {
    auto* h = static_cast<ACTrain*>(handle);
    if (!h) return fail("actrain: null handle");
    h->adv = d_adv;
    return 0;
}

MFX_API int mfx_actrain_set_ppo(void* handle, const float* d_logp_old, double clip, float* d_logp_new) {
    auto* h = static_cast<ACTrain*>(handle);
    if (!h) return fail("actrain: null handle");
    if (!d_logp_old) {
        h->lp_old = nullptr;
        h->lp_new = nullptr;
        return 0;
    }
    if (!(clip > 0.0) || !std::isfinite(clip)) return fail("actrain_set_ppo: clip %g must be finite and > 0", clip);
    h->lp_old = d_logp_old;
    h->lp_new = d_logp_new;
    h->ppo_lo = (float)(1.0 - clip);
    h->ppo_hi = (float)(1.0 + clip);
    return 0;
}

MFX_API int mfx_actrain_ppo_stats(void* handle, float* d_out2, void* stream) {
    auto* h = static_cast<ACTrain*>(handle);
    if (!h) return fail("actrain: null handle");
    if (!d_out2) return fail("actrain_ppo_stats: null d_out2");
    if (!h->pstat.p) {                    // no PPO gradient yet
        MFX_HIP(hipMemsetAsync(d_out2, 0, 2 * sizeof(float), (hipStream_t)stream));
        return 0;
    }
    MFX_HIP(hipMemcpyAsync(d_out2, h->pstat.p, 2 * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

MFX_API int mfx_actrain_grads(void* handle, const mfx_actrain_rows* rows, long long n, float* d_grad_blob,
                              float* d_stats, void* stream) {
    auto* h = static_cast<ACTrain*>(handle);
    if (!h) return fail("actrain: null handle");
    MFX_CHECK(at_gradient(h, rows, n, d_stats, (hipStream_t)stream));
    if (d_grad_blob)
        MFX_HIP(hipMemcpyAsync(d_grad_blob, h->state + 3 * h->blob_n, h->blob_n * sizeof(float), hipMemcpyDeviceToDevice,
                               (hipStream_t)stream));
    return 0;
}

MFX_API int mfx_actrain_step(void* handle, const mfx_actrain_rows* rows, long long n, float* d_stats, void* stream) {
    auto* h = static_cast<ACTrain*>(handle);
    if (!h) return fail("actrain: null handle");
    MFX_CHECK(at_gradient(h, rows, n, d_stats, (hipStream_t)stream));
    const double s = (double)(h->step + 1);
    AdamArgs t{h->state, h->state + h->blob_n, h->state + 2 * h->blob_n, h->state + 3 * h->blob_n, h->err,
               (float)(1.0 - h->beta1), (float)(1.0 - h->beta2), (float)(h->lr / (1.0 - pow(h->beta1, s))),
               (float)sqrt(1.0 - pow(h->beta2, s)), (float)h->eps};
    k_at_adam<<<(unsigned)((h->blob_n + 255) / 256), 256, 0, (hipStream_t)stream>>>(t, h->blob_n);
    MFX_HIP(hipGetLastError());
    h->step += 1;
    return 0;
}

MFX_API int mfx_actrain_error(void* handle, int* code, long long* bad_value, void* stream) {
    auto* h = static_cast<ACTrain*>(handle);
    if (!h) return fail("actrain: null handle");
    int32_t e[4];
    MFX_HIP(hipMemcpyAsync(e, h->err, sizeof e, hipMemcpyDeviceToHost, (hipStream_t)stream));
    MFX_HIP(hipStreamSynchronize((hipStream_t)stream));
    *code = e[0];
    *bad_value = (long long)(((uint64_t)(uint32_t)e[2] << 32) | (uint32_t)e[1]);
    h->step = e[3];                       // the steps applied: one enqueued with a bad action was skipped
    if (e[0]) MFX_HIP(hipMemsetAsync(h->err, 0, 3 * sizeof(int32_t), (hipStream_t)stream));
    return 0;
}

}  // extern "C"
