// ising_mc_kernels.hip -- Metropolis baseline of the Ising lattice on gfx950 (the MCMC curve the MF-Q order
// parameter is set against).
//
// R independent replicas, one workgroup each, the spins in LDS; the lattice and the neighbour table are the MF-Q
// kernels' (ising_kernels.hip: agent i at row i / L, column i % L; nbr [N][4] ascending ids).  Restricted to the
// 4-neighbour lattice (view 1) of even side: the sites of one parity of row + column have all their neighbours in
// the other, so a half-sweep updates its sites in place and in parallel, and a sweep is the two half-sweeps, parity
// 0 first.  Site i of replica r with spin s and `a` neighbours equal to s flips when
//     philox_uniform_in(kPhiloxDomainMc, seed, r, sweep, i) < acc[r][a]
// acc comes from the host (mfrl_amd.ising.metropolis_table): the kernel calls no exp(), so the chain is bit-exact
// against its numpy restatement (tests/ising_trace_ref.py).  Lattices above 1024 sites loop over them as
// k_ising_mfq_big does (lane l: sites l, l + 1024, ...).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "ising_kernels.h"
#include "ising_philox.h"

namespace mfx {

__global__ void __launch_bounds__(1024) k_ising_mc(IsingMcArgs a) {
    extern __shared__ uint8_t sp[];                                   // [N]
    __shared__ double acc[5];
    __shared__ int cnt[2];
    const int r = blockIdx.x, N = a.N, L = a.L;
    uint8_t* S = a.spins + (size_t)r * N;
    for (int i = threadIdx.x; i < N; i += blockDim.x) sp[i] = S[i] ? 1 : 0;
    if (threadIdx.x < 5) acc[threadIdx.x] = a.acc[(size_t)r * 5 + threadIdx.x];
    if (threadIdx.x == 0) { cnt[0] = 0; cnt[1] = 0; }
    __syncthreads();
    for (int s = 0; s < a.sweeps; ++s) {
        for (int par = 0; par < 2; ++par) {
            for (int i = threadIdx.x; i < N; i += blockDim.x) {
                if (((i / L + i % L) & 1) != par) continue;
                const int si = sp[i];
                int same = 0;
                for (int k = 0; k < 4; ++k) same += sp[a.nbr[i * 4 + k]] == si;
                const double u = philox_uniform_in(kPhiloxDomainMc, a.seed, (uint32_t)r, (uint32_t)s, (uint32_t)i);
                if (u < acc[same]) sp[i] = (uint8_t)(1 - si);
            }
            __syncthreads();
        }
        int ups = 0;
        for (int i = threadIdx.x; i < N; i += blockDim.x) ups += sp[i];
        const int b = s & 1;
        atomicAdd(&cnt[b], ups);
        __syncthreads();
        if (threadIdx.x == 0) {
            const int n_up = cnt[b], n_down = N - n_up;
            a.order_out[(size_t)r * a.sweeps + s] = (double)(n_up > n_down ? n_up - n_down : n_down - n_up) / ((double)N + 0.0);
            a.nup_out[(size_t)r * a.sweeps + s] = n_up;
            cnt[b ^ 1] = 0;                                           // the next sweep's counter (added to after two barriers)
        }
    }
    for (int i = threadIdx.x; i < N; i += blockDim.x) S[i] = sp[i];
}

hipError_t launch_ising_mc(const IsingMcArgs& a, int R, hipStream_t st) {
    // the checkerboard needs the 4-neighbour lattice of even side (L = 2 has two neighbours, not four)
    if (a.L < 4 || (a.L & 1) || a.N != a.L * a.L || a.N > 32767 || a.sweeps < 1 || R < 1) return hipErrorInvalidValue;
    const int threads = a.N >= 1024 ? 1024 : ((a.N + 63) / 64) * 64;
    k_ising_mc<<<R, threads, (size_t)a.N, st>>>(a);
    return hipGetLastError();
}

}  // namespace mfx
