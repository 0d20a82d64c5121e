// gae_kernels.hip -- the opt-in GAE(lambda) advantage estimator of the actor-critic models on the device rollout loop
// (ActorCritic.advantage = "gae"): the walk along each agent's chain of step-major rows that
// mfx_chain_returns walks (collect_kernels.hip), and the normalisation of the advantage column.  The contract is in
// include/magent_amd.h (mfx_chain_gae, mfx_adv_normalize), the numpy restatement in tests/gae_ref.py.
//
// k_chain_gae is latency-bound like k_chain_returns: one lane per chain, one dependent load (prev[r]) per row; a row's
// reward and value loads depend on r alone and are in flight together with it.  The normalisation is three passes over
// one float column (4 B read per row twice, 4 B read + 4 B written once): nothing to tune at a round's 10^5..10^6 rows.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mfx_common.h"
#include "../../include/magent_amd.h"

namespace mfx {

// err[0] = 1, err[1] = an offending index; zero at load; read, and cleared when set, by mfx_chain_gae (its own word:
// a fault here never shows up in mfx_chain_returns, nor the other way round)
__device__ int64_t g_gae_err[2];

// Chain i, from its tail row t back along prev: nxt = V[t], g = 0; per row delta = (rew + gamma nxt) - V, g = delta +
// gl g; adv = g, rew = g + V; nxt = V.  Every operation is a rounded double operation of its own (-ffp-contract=off).
// k_chain_returns' guards: a tail outside [0, n_rows), or a prev that is neither -1 nor in [0, r), ends the walk before
// any further load or store (rows are step-major: a predecessor lies strictly below its row, so no walk can cycle).
__global__ void __launch_bounds__(256) k_chain_gae(float* __restrict__ rew, float* __restrict__ adv,
                                                   const int64_t* __restrict__ prev, const int64_t* __restrict__ tails,
                                                   const float* __restrict__ V, int64_t n_tails, int64_t n_rows,
                                                   double gamma, double gl, int64_t* err) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tails) return;
    int64_t r = tails[i], above = n_rows;
    double nxt = 0.0, g = 0.0;
    bool first = true;
    do {
        if (r < 0 || r >= above) {
            err[1] = r;                              // (any offender: lanes may race here, each with a bad index)
            err[0] = 1;
            return;
        }
        const int64_t p = prev[r];                   // the only load the next row waits for
        const double x = (double)rew[r], v = (double)V[r];
        if (first) { nxt = v; first = false; }       // the tail's value stands for the state after it
        const double t = gamma * nxt;
        const double delta = (x + t) - v;
        const double u = gl * g;
        g = delta + u;
        adv[r] = (float)g;
        rew[r] = (float)(g + v);
        nxt = v;
        above = r;
        r = p;
    } while (r != -1);
}

// ---- the normalisation: mean and population standard deviation in double, two passes, one summation order per n.
// Workgroup b sums elements [b span, (b + 1) span): thread t its elements t, t + 256, ... in order, then the threads
// by a fixed tree; k_adv_stat adds the workgroups' partials in index order.
constexpr int kAdvMaxParts = 1024;
constexpr int64_t kAdvSpan = 4096;
// [0, kAdvMaxParts) the partials, then mean, std.  The library's own scratch: calls must not overlap on two streams.
__device__ double g_adv_scratch[kAdvMaxParts + 2];

template <bool CENTRED>
__global__ void __launch_bounds__(256) k_adv_sum(const float* __restrict__ adv, int64_t n, int64_t span, double* sc) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int64_t a = (int64_t)blockIdx.x * span, b = a + span < n ? a + span : n;
    const double mean = CENTRED ? sc[kAdvMaxParts] : 0.0;
    double s = 0.0;
    for (int64_t r = a + tid; r < b; r += 256) {
        const double d = (double)adv[r] - mean;
        s += CENTRED ? d * d : d;
    }
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {                  // a fixed tree
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) sc[blockIdx.x] = red[0];
}

// pass 0: mean = sum / n; pass 1: std = sqrt(sum / n)
template <bool CENTRED>
__global__ void k_adv_stat(double* sc, int parts, int64_t n) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int k = 0; k < parts; ++k) s += sc[k];
    const double m = s / (double)n;
    if (CENTRED) sc[kAdvMaxParts + 1] = sqrt(m);
    else sc[kAdvMaxParts] = m;
}

__global__ void __launch_bounds__(256) k_adv_apply(float* __restrict__ adv, int64_t n, const double* __restrict__ sc) {
    const double mean = sc[kAdvMaxParts], den = sc[kAdvMaxParts + 1] + 1e-8;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256)
        adv[r] = (float)(((double)adv[r] - mean) / den);
}

}  // namespace mfx

using namespace mfx;

extern "C" {

MFX_API int mfx_chain_gae(float* d_rew, float* d_adv, const int64_t* d_prev, const int64_t* d_tails,
                          const float* d_value_rows, int64_t n_tails, int64_t n_rows, double gamma, double lambda,
                          void* stream) {
    if (!(gamma >= 0.0 && gamma <= 1.0)) return fail("chain_gae: gamma %g is outside [0, 1]", gamma);
    if (!(lambda >= 0.0 && lambda <= 1.0)) return fail("chain_gae: lambda %g is outside [0, 1]", lambda);
    if (n_tails < 0 || n_rows < 0) return fail("chain_gae: n_tails and n_rows must be >= 0");
    if (n_tails == 0) return 0;
    if (!d_rew || !d_adv || !d_prev || !d_tails || !d_value_rows) return fail("chain_gae: null argument");
    if (d_rew == d_adv) return fail("chain_gae: the advantage column must not be the reward column");
    if (n_tails > n_rows) return fail("chain_gae: %lld tails for %lld rows", (long long)n_tails, (long long)n_rows);
    hipStream_t st = (hipStream_t)stream;
    int64_t* err = nullptr;
    MFX_HIP(hipGetSymbolAddress((void**)&err, HIP_SYMBOL(g_gae_err)));
    const unsigned grid = (unsigned)((n_tails + 255) / 256);
    const double gl = gamma * lambda;
    k_chain_gae<<<grid, 256, 0, st>>>(d_rew, d_adv, d_prev, d_tails, d_value_rows, n_tails, n_rows, gamma, gl, err);
    MFX_HIP(hipGetLastError());
    int64_t h[2] = {0, 0};
    MFX_HIP(hipMemcpyAsync(h, err, sizeof h, hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    if (h[0]) {
        const int64_t z[2] = {0, 0};
        MFX_HIP(hipMemcpyAsync(err, z, sizeof z, hipMemcpyHostToDevice, st));
        MFX_HIP(hipStreamSynchronize(st));
        return fail("chain_gae: row index %lld is outside its chain's rows (tails in [0, %lld), a predecessor in "
                    "[0, its row))", (long long)h[1], (long long)n_rows);
    }
    return 0;
}

MFX_API int mfx_adv_normalize(float* d_adv, int64_t n, void* stream) {
    if (n < 0) return fail("adv_normalize: n must be >= 0");
    if (n == 0) return 0;
    if (!d_adv) return fail("adv_normalize: null argument");
    hipStream_t st = (hipStream_t)stream;
    double* sc = nullptr;
    MFX_HIP(hipGetSymbolAddress((void**)&sc, HIP_SYMBOL(g_adv_scratch)));
    // the partition is a function of n alone: at most kAdvMaxParts workgroups of equal spans, 4096 elements or more
    int64_t parts = (n + kAdvSpan - 1) / kAdvSpan;
    if (parts > kAdvMaxParts) parts = kAdvMaxParts;
    const int64_t span = (n + parts - 1) / parts;
    parts = (n + span - 1) / span;
    k_adv_sum<false><<<(unsigned)parts, 256, 0, st>>>(d_adv, n, span, sc);
    k_adv_stat<false><<<1, 1, 0, st>>>(sc, (int)parts, n);
    k_adv_sum<true><<<(unsigned)parts, 256, 0, st>>>(d_adv, n, span, sc);
    k_adv_stat<true><<<1, 1, 0, st>>>(sc, (int)parts, n);
    const int64_t wgs = (n + 255) / 256, cap = (int64_t)device_cus() * 8;
    k_adv_apply<<<(unsigned)(wgs < cap ? wgs : cap), 256, 0, st>>>(d_adv, n, sc);
    MFX_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
