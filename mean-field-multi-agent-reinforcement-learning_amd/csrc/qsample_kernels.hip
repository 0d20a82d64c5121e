// qsample_kernels.hip -- k_q_sample: the Boltzmann draw of qsample.h on a Q table in memory, for the callers whose Q
// values do not come from the fused forward (ValueNet.act_dev on a view shape that runs the torch module) and for the
// tests, which feed it arbitrary rows.  The fused epilogues of k_qnet_head / k_qb16_head call the same q_sample_row,
// so they give this kernel's actions and weights bit for bit on the Q values they write.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "mfx_common.h"
#include "qsample.h"
#include "../../include/magent_amd.h"

namespace mfx {

// One lane per row, grid-stride; no LDS.  Row i reads q[i][0..A), writes act[i] and w[i][0..A).
__global__ void __launch_bounds__(256) k_q_sample(const float* __restrict__ q, const int32_t* __restrict__ rows, int n, int A,
                                                  float T, uint32_t seed, uint32_t step, int group, float* __restrict__ w,
                                                  int32_t* __restrict__ act) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float* qr = q + (size_t)i * A;
        float x[kQSMaxA];
#pragma unroll
        for (int a = 0; a < kQSMaxA; ++a) x[a] = a < A ? qr[a] : 0.f;
        const int pick = q_sample_row(x, A, T, ac_uniform(seed, step, group, rows ? rows[i] : i));
        if (act) act[i] = pick;
        if (w) {
            float* wr = w + (size_t)i * A;
#pragma unroll
            for (int a = 0; a < kQSMaxA; ++a)
                if (a < A) wr[a] = x[a];
        }
    }
}

hipError_t launch_q_sample(const float* q, const int32_t* rows, int n, int A, float T, uint32_t seed, uint32_t step,
                           int group, float* w, int32_t* act, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const int grid = std::min((n + 255) / 256, 4096);
    k_q_sample<<<grid, 256, 0, st>>>(q, rows, n, A, T, seed, step, group, w, act);
    return hipGetLastError();
}

}  // namespace mfx

using namespace mfx;

extern "C" {

// d_rows: the row of the uniform per table row (null: row i), e.g. e * rowcap + j of a rollout.
MFX_API int mfx_q_sample_rows(const float* d_q, const int32_t* d_rows, int n, int A, float temperature, uint32_t seed,
                              uint32_t step, int group, float* d_w, int32_t* d_act, void* stream) {
    if (n < 0 || A < 2 || A > kQSMaxA) return fail("q_sample: n >= 0 and 2 <= A <= 32; got n %d, A %d", n, A);
    if (!(std::isfinite(temperature) && temperature > 0.f))
        return fail("q_sample: the temperature must be finite and > 0; got %g", (double)temperature);
    if (n && !d_q) return fail("q_sample: no Q table");
    MFX_HIP(launch_q_sample(d_q, d_rows, n, A, temperature, seed, step, group, d_w, d_act, (hipStream_t)stream));
    return 0;
}

MFX_API int mfx_q_sample(const float* d_q, int n, int A, float temperature, uint32_t seed, uint32_t step, int group,
                         float* d_w, int32_t* d_act, void* stream) {
    return mfx_q_sample_rows(d_q, nullptr, n, A, temperature, seed, step, group, d_w, d_act, stream);
}

}  // extern "C"
