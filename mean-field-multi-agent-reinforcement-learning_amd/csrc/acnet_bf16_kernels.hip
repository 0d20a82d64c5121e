// acnet_bf16_kernels.hip -- the policy path of the actor-critic network (acnet_kernels.hip: ActorCritic / MFAC
// ._create_network and the act) with bf16 matrix operands on v_mfma_f32_16x16x32_bf16: the opt-in acting mode
// precision = 1 of mfx_acnet_set_precision.  Per agent:
//
//   view [V] --dense 256, relu--> h_view;  feature [F] --dense 256, relu--> h_emb
//   concat(h_view, h_emb) [512] --dense 512, relu--> d
//   policy = clip(softmax(dense(d / 0.1) -> A), 1e-10, 1 - 1e-10);  act ~ multinomial(log policy)
//
// The value heads and the prob input are not part of this mode (acting only).
//
// NUMERICAL CONTRACT (tests/acnet_bf16_ref.py restates it in numpy; the GPU tests hold the kernel to it)
//   * The operands of every matrix product are rounded to bf16, round-to-nearest-even:
//       - the four weight matrices (view, feature, dense, policy), once, when the images are built (set_weights /
//         set_precision);
//       - the view and the feature inputs, f32 -> bf16;
//       - h_view and h_emb after bias and ReLU;
//       - div_tenth(relu(d)): the f32 division k_acnet does (correctly rounded), then ONE rounding to bf16.
//   * Products are accumulated in f32 (the MFMA accumulator, which starts at the f32 bias); ReLU is applied in f32.
//   * Softmax, the clip and the draw are f32 and unrounded: policy_act.h's ac_epilogue, the rule k_acnet writes out
//     (ac_uniform and the running-sum pick).
//   * An agent's result does not depend on its position in the batch or on the batch size: every agent is one
//     column of its MFMAs, accumulated in one fixed order.
//   * The view layer runs the dense k order whether or not an input support is set on the handle.
//
// One kernel, k_acb16: 4 waves x 16 agents per workgroup, one workgroup per 64 rows.  Every layer of 256 output
// units consumes one 16-KB weight chunk per k-step of 32 inputs (acnet_bf16.h): 37 for the Battle view, 2 for its
// features, 16 + 16 for the dense layer's two output halves, each half followed by one chunk that holds the policy
// layer over that half's units (8 k-steps x 2 tiles): one sequence in memory.  A chunk is loaded three k-steps
// ahead into registers (16 B x 4 per lane), stored into one of two LDS buffers a step before its use and shared by
// the four waves: one barrier per k-step.  A lane streams its agent's f32 view row straight from HBM, 32 B per
// k-step (two 16-B loads, three k-steps ahead as well), and converts it once.  Everything in flight is an ordinary
// register load, so the compiler counts its vmcnt waits and weights and view rows stay outstanding across the
// barriers (the counter retires in issue order, and with a chunk copied direct-to-LDS the compiler turns every later
// wait into vmcnt(0)).  The
// activations never leave the registers (two accumulator tiles -> one B fragment, as qnet_bf16_kernels.hip's
// pack_relu); each dense half is folded into the policy logits by its policy chunk as soon as it is whole, so at most
// 256 f32 activations per agent are live.  No scratch, no spills (tests/test_acnet_bf16_cpu.py); LDS 40 KB per
// workgroup, two workgroups per CU (registers).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <utility>

#include "acnet_bf16.h"

namespace mfx {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // a view row is only 4-B aligned
// 16 B of the images, LDS and the B fragments: a native vector (arrays of HIP's uint4 struct are not always promoted to
// registers)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kLead = 3;                                 // chunks (and view k-steps) in flight ahead of the MFMAs
constexpr int kMaxA = kAB16PolMT * 16;                   // policy columns
static_assert(kMaxA == kActMaxA, "ac_epilogue's row");
constexpr int kLgOff = 2 * kAB16Chunk;                   // (16-B units) the logits follow the two chunk buffers
// The dynamic LDS of k_acb16: the one size the kernel's offsets and the launch share.
constexpr size_t kAcb16Smem = (size_t)kLgOff * 16 + (size_t)kAB16Waves * 16 * kMaxA * 4;
static_assert(kAcb16Smem == (size_t)2 * kAB16Chunk * 16 + (size_t)kAB16Rows * kMaxA * 4, "two chunks + a logit row per agent");
static_assert(kAB16Chunk == 4 * 64 * kAB16Waves, "four 16-B units per lane and chunk");
static_assert(8 * kAB16PolMT * 64 == kAB16Chunk, "the policy layer over one dense half is one chunk");

__device__ __forceinline__ f32x4 mfma32(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// two f32 -> two bf16 (RNE) in one register
__device__ __forceinline__ uint32_t pk2(float lo, float hi) {
    const bf16x2 v = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(uint32_t, v);
}

__device__ __forceinline__ uint16_t bf16_bits(float x) { return __builtin_bit_cast(uint16_t, (__bf16)x); }

__device__ __forceinline__ bf16x8 frag(u32x4 u) { return __builtin_bit_cast(bf16x8, u); }

__device__ __forceinline__ u32x4 pack8(const float* v) {
    return u32x4{pk2(v[0], v[1]), pk2(v[2], v[3]), pk2(v[4], v[5]), pk2(v[6], v[7])};
}

// relu of two neighbouring accumulator tiles (units 16 (2 s) + 4 h + r and 16 (2 s + 1) + 4 h + r) -> the B fragment
// of the next layer's k-step s (element j = tile parity j >> 2, register j & 3: acb16_k, not linear)
__device__ __forceinline__ u32x4 pack_relu(f32x4 lo, f32x4 hi) {
    return u32x4{pk2(fmaxf(lo[0], 0.f), fmaxf(lo[1], 0.f)), pk2(fmaxf(lo[2], 0.f), fmaxf(lo[3], 0.f)),
                 pk2(fmaxf(hi[0], 0.f), fmaxf(hi[1], 0.f)), pk2(fmaxf(hi[2], 0.f), fmaxf(hi[3], 0.f))};
}

// the same with relu(x) / 0.1 (f32, correctly rounded) in front of the one rounding to bf16
__device__ __forceinline__ float dt(float x) { return div_tenth(fmaxf(x, 0.f)); }
__device__ __forceinline__ u32x4 pack_relu_tenth(f32x4 lo, f32x4 hi) {
    return u32x4{pk2(dt(lo[0]), dt(lo[1])), pk2(dt(lo[2]), dt(lo[3])), pk2(dt(hi[0]), dt(hi[1])),
                 pk2(dt(hi[2]), dt(hi[3]))};
}

__device__ __forceinline__ f32x4 bias4(const float* bias, int t, int h) {
    const float4 b = *reinterpret_cast<const float4*>(bias + 16 * t + 4 * h);
    return {b.x, b.y, b.z, b.w};
}

// One image: a thread per bf16 element (layout: acnet_bf16.h).
__global__ void __launch_bounds__(256) k_acb16_image(const float* __restrict__ src, int K, int N, int linear,
                                                     uint16_t* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int mt = N / 16, j = (int)(i & 7), l = (int)((i >> 3) & 63);
    const size_t q = i >> 9;
    const int t = (int)(q % mt), s = (int)(q / mt);
    const int k = acb16_k(linear != 0, s, l >> 4, j);
    dst[i] = bf16_bits(k < K ? src[(size_t)k * N + 16 * t + (l & 15)] : 0.f);
}

// The chunk-end barrier: this wave's part of the next chunk is in LDS and its reads of this one are done.  A bare
// barrier, not __syncthreads(), whose fence would drain the loads in flight; inside the asm, so the compiler may not
// move an LDS access across it.
__device__ __forceinline__ void chunk_sync() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// acc[t] += chunk tile t (W^T, 16 units x 32 inputs) . b, t < 16: one k-step of a 256-unit layer
__device__ __forceinline__ void mfma16(const u32x4* cur, u32x4 b, f32x4* acc) {
    const bf16x8 bb = frag(b);
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = mfma32(frag(cur[t * 64]), bb, acc[t]);
}

// f(integral_constant<int, 0>) .. f(integral_constant<int, N - 1>): a loop unrolled by the language, not by a pass
// that may decline a long body
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

// Steps over chunks g0 .. g0 + count - 1 (kCount > 0: that many, unrolled by static_for, the step an
// integral_constant, so `work` may index registers by it).  On entry chunk g0 is in LDS buffer g0 & 1; on exit chunk g0 + count is (past glast: the last one again).
// Step i (u = i % kLead: the ring slot, static): chunk g0 + i + kLead is loaded into registers, work(i, u, cur)
// issues the layer's own loads and runs the step's MFMAs on the chunk in LDS (cur: this lane's fragment of tile 0,
// tile t 64 units on), and chunk g0 + i + 1 -- loaded kLead - 1 steps ago -- goes to the other buffer.
template <int kCount, class WF>
__device__ __forceinline__ void chunk_steps(const u32x4* __restrict__ chunks, int g0, int count, int glast, u32x4* lds,
                                            int tid, WF work) {
    const int lane = tid & 63;
    u32x4 wr[kLead][4];
    auto wload = [&](int g, u32x4* d) {
        const u32x4* src = chunks + (size_t)min(g, glast) * kAB16Chunk + tid;
#pragma unroll
        for (int q = 0; q < 4; ++q) d[q] = src[q * 256];
    };
#pragma unroll
    for (int u = 1; u < kLead; ++u) wload(g0 + u, wr[u]);
    auto body = [&](auto i, int u) {
        wload(g0 + i + kLead, wr[u]);
        work(i, u, lds + ((g0 + i) & 1) * kAB16Chunk + lane);
        u32x4* nxt = lds + ((g0 + i + 1) & 1) * kAB16Chunk + tid;
#pragma unroll
        for (int q = 0; q < 4; ++q) nxt[q * 256] = wr[(u + 1) % kLead][q];
        chunk_sync();
    };
    if constexpr (kCount > 0) {
        static_for<kCount>([&](auto ic) { body(ic, decltype(ic)::value % kLead); });
    } else {
        for (int i0 = 0; i0 < count; i0 += kLead) {
#pragma unroll
            for (int u = 0; u < kLead; ++u)
                if (i0 + u < count) body(i0 + u, u);
        }
    }
}

// ------------------------------------------------------------------------------------------ forward
__global__ void __launch_bounds__(64 * kAB16Waves, 2)
k_acb16(ACB16Net p, const float* __restrict__ view, size_t view_ld, const float* __restrict__ feat, size_t feat_ld,
        QRowMap rm, int n, const int32_t* __restrict__ d_n, float* __restrict__ policy_out,
        int32_t* __restrict__ act_out, uint32_t seed, uint32_t step, int group) {
    extern __shared__ __attribute__((aligned(16))) u32x4 csm[];
    const u32x4* chunks = reinterpret_cast<const u32x4*>(p.chunks);
    if (d_n) n = min(*d_n, n);
    if ((int)blockIdx.x * kAB16Rows >= n) return;                  // (uniform: a launch sized for the upper bound)
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h = lane >> 4, c = lane & 15;
    const int base = (blockIdx.x * kAB16Waves + wid) * 16;
    const int ia = min(base + c, n - 1);                           // this lane's agent (clamped: junk, never written)
    const int row = rm.row(ia);
    const float* vrow = view + (size_t)row * view_ld;
    const float* vr = vrow + 8 * h;                                // this lane's 8 floats of k-step s: vr[32 s ..]
    const float* fr = feat + (size_t)row * feat_ld;
    const int V = p.V, F = p.F, nfull = V >> 5, nsv = p.nsv, nse = p.nse;
    const int glast = nsv + nse + 2 * kAB16HalfChunks - 1;                              // the last chunk

    // ---- the loads that arrive first: chunk 0, the view's partial last k-step and the features' first (inputs past
    // V / F: the last float, replaced by zero)
    u32x4 w0[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) w0[q] = chunks[q * 256 + tid];
    float tl[8], fv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = 32 * nfull + 8 * h + j;
        const float x = vrow[min(k, V - 1)];
        tl[j] = k < V ? x : 0.f;
    }
    auto fload = [&](int s) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 32 * s + 8 * h + j;
            const float x = fr[min(k, F - 1)];
            fv[j] = k < F ? x : 0.f;
        }
    };
    fload(0);
    // ---- view k-steps 0 .. kLead - 1 in flight (whole k-steps only: 32 s + 8 h + 7 < V)
    f32x4u pf[kLead][2] = {};
    auto vload = [&](int s, f32x4u* d) {
        const float* src = vr + 32 * min(s, nfull - 1);
        d[0] = *reinterpret_cast<const f32x4u*>(src);
        d[1] = *reinterpret_cast<const f32x4u*>(src + 4);
    };
    if (nfull > 0) {
#pragma unroll
        for (int u = 0; u < kLead; ++u) vload(u, pf[u]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) csm[q * 256 + tid] = w0[q];
    chunk_sync();

    // ---- h_view^T [256 x 16]: the whole k-steps from the ring, then the partial one
    f32x4 hv[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) hv[t] = bias4(p.bv, t, h);
    chunk_steps<0>(chunks, 0, nsv, glast, csm, tid, [&](int i, int u, const u32x4* cur) {
        const float x[8] = {pf[u][0][0], pf[u][0][1], pf[u][0][2], pf[u][0][3],
                            pf[u][1][0], pf[u][1][1], pf[u][1][2], pf[u][1][3]};
        const u32x4 b = i < nfull ? pack8(x) : pack8(tl);
        if (nfull > 0) vload(i + kLead, pf[u]);
        mfma16(cur, b, hv);
    });
    u32x4 hb[16];                                                  // the concat as B fragments: k-steps 0-7 h_view, 8-15 h_emb
#pragma unroll
    for (int s = 0; s < 8; ++s) hb[s] = pack_relu(hv[2 * s], hv[2 * s + 1]);
    // ---- h_emb^T [256 x 16]: the features a k-step ahead
    {
        f32x4 he[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) he[t] = bias4(p.be, t, h);
        chunk_steps<0>(chunks, nsv, nse, glast, csm, tid, [&](int i, int, const u32x4* cur) {
            const u32x4 b = pack8(fv);
            fload(min(i + 1, nse - 1));
            mfma16(cur, b, he);
        });
#pragma unroll
        for (int s = 0; s < 8; ++s) hb[8 + s] = pack_relu(he[2 * s], he[2 * s + 1]);
    }
    // ---- dense [512] in two halves of 256 units, each 16 k-steps and then one chunk that folds it into the policy
    // logits (the policy layer's 8 k-steps x 2 tiles over that half's units): one unrolled sequence of 34 chunks
    f32x4 pl[kAB16PolMT], dh[16];
#pragma unroll
    for (int t = 0; t < kAB16PolMT; ++t) pl[t] = bias4(p.bp, t, h);
    chunk_steps<2 * kAB16HalfChunks>(chunks, nsv + nse, 2 * kAB16HalfChunks, glast, csm, tid,
                                     [&](auto ic, int, const u32x4* cur) {
        constexpr int half = decltype(ic)::value / kAB16HalfChunks, s = decltype(ic)::value % kAB16HalfChunks;
        if constexpr (s == 0) {
#pragma unroll
            for (int t = 0; t < 16; ++t) dh[t] = bias4(p.bd + half * kAB16H, t, h);
        }
        if constexpr (s < 16) {
            mfma16(cur, hb[s], dh);
        } else {
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const bf16x8 bb = frag(pack_relu_tenth(dh[2 * ks], dh[2 * ks + 1]));
#pragma unroll
                for (int t = 0; t < kAB16PolMT; ++t) pl[t] = mfma32(frag(cur[(ks * kAB16PolMT + t) * 64]), bb, pl[t]);
            }
        }
    });
    // ---- policy: logits of agent c, actions 16 t + 4 h + r, through LDS to lane c of the wave (h == 0): softmax,
    // clip, the draw -- ac_epilogue (the bias is already in the logits)
    float* lg = reinterpret_cast<float*>(csm + kLgOff) + wid * 16 * kMaxA;
#pragma unroll
    for (int t = 0; t < kAB16PolMT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) lg[c * kMaxA + 16 * t + 4 * h + r] = pl[t][r];
    qwave_sync();
    const int i = base + c;
    if (h == 0 && i < n) {
        const int A = p.A;
        ac_epilogue([&](int a) { return lg[c * kMaxA + a]; }, A, i, row, rm, policy_out, act_out, seed, step, group);
    }
}


}  // namespace

hipError_t acb16_build(ACB16Net* net, const float* const* w, int V, int F, int A, uint4* img, hipStream_t st) {
    const int Vp = (V + 3) & ~3, Fp = (F + 3) & ~3;
    const int nsv = acb16_steps(V), nse = acb16_steps(F);
    // (source, K rows, columns, linear k order, k-steps) in chunk order: view, feature, then per dense half its 16
    // k-steps and the policy layer's 8 over that half's units (2 tiles x 8 k-steps: one chunk)
    const struct { const float* src; int K, N, linear, steps; } m[6] = {
        {w[0], Vp, kAB16H, 1, nsv}, {w[2], Fp, kAB16H, 1, nse},
        {w[4], 2 * kAB16H, kAB16H, 0, 16}, {w[7], kAB16H, kMaxA, 0, 8},
        {w[5], 2 * kAB16H, kAB16H, 0, 16}, {w[7] + (size_t)kAB16H * kMaxA, kAB16H, kMaxA, 0, 8}};
    uint4* dst = img;
    for (int k = 0; k < 6; ++k) {
        const size_t units = (size_t)m[k].steps * (m[k].N / 16) * 64, n = units * 8;
        k_acb16_image<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(m[k].src, m[k].K, m[k].N, m[k].linear,
                                                                   reinterpret_cast<uint16_t*>(dst), n);
        dst += units;
    }
    net->chunks = img;
    net->bv = w[1]; net->be = w[3]; net->bd = w[6]; net->bp = w[8];
    net->V = V; net->F = F; net->A = A;
    net->nsv = nsv; net->nse = nse;
    return hipGetLastError();
}

hipError_t acb16_forward(const ACB16Net& net, const float* view, size_t view_ld, const float* feat, size_t feat_ld,
                         QRowMap rm, int n, const int32_t* d_n, float* policy_out, int32_t* act_out, uint32_t seed,
                         uint32_t step, int group, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const int grid = (n + kAB16Rows - 1) / kAB16Rows;
    k_acb16<<<grid, 64 * kAB16Waves, kAcb16Smem, st>>>(net, view, view_ld, feat, feat_ld, rm, n, d_n, policy_out,
                                                        act_out, seed, step, group);
    return hipGetLastError();
}

}  // namespace mfx
