// ppo_kernels.hip -- the behaviour log-probabilities of the opt-in PPO objective (ActorCritic.objective = "ppo",
// DESIGN 7u): logp[i] = log(policy[i][act[i]] + 1e-6f) over a round's rows, from the clamped policy of the f32 forward
// (mfx_acnet_forward) at the round's pre-update weights.  The contract is in include/magent_amd.h (mfx_policy_logp),
// the loss head that reads the column is k_at_loss_ppo (actrain_kernels.hip).
//
// One lane per row: 4 B of action, one 4 B gather from the row's n_action floats, 4 B stored -- a single pass over
// columns the forward has just written; nothing to tune against the forward's own traffic.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mfx_common.h"
#include "../../include/magent_amd.h"

namespace mfx {

// The action is checked before it selects anything: a row whose action is outside [0, A) loads nothing from the policy
// and gets +0 (the training step that follows reports it).
__global__ void __launch_bounds__(256) k_policy_logp(const float* __restrict__ policy, const int32_t* __restrict__ act,
                                                     long long n, int A, float* __restrict__ logp) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int a = act[i];
        float lp = 0.f;
        if (a >= 0 && a < A) lp = logf(policy[(size_t)i * A + a] + 1e-6f);
        logp[i] = lp;
    }
}

}  // namespace mfx

using namespace mfx;

extern "C" {

MFX_API int mfx_policy_logp(const float* d_policy, const int32_t* d_act, long long n, int n_action, float* d_logp,
                            void* stream) {
    if (n_action < 2 || n_action > 32) return fail("policy_logp: n_action %d (2..32)", n_action);
    if (n < 0) return fail("policy_logp: n must be >= 0");
    if (n == 0) return 0;
    if (!d_policy || !d_act || !d_logp) return fail("policy_logp: null argument");
    const long long wgs = (n + 255) / 256, cap = (long long)device_cus() * 8;
    k_policy_logp<<<(unsigned)(wgs < cap ? wgs : cap), 256, 0, (hipStream_t)stream>>>(d_policy, d_act, n, n_action, d_logp);
    MFX_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
