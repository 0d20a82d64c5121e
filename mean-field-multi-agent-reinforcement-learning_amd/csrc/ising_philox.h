// ising_philox.h -- the counter-based draws of the Ising kernels (device code; ising_kernels.hip, ising_mc_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mfx {

// ------------------------------------------------------------------ Philox 4x32-10 (perf mode)
__device__ __forceinline__ void philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// The fourth counter word names the consumer, so two kernels never share a draw: the MF-Q Boltzmann uniforms and
// the Metropolis acceptance draws of k_ising_mc.
constexpr uint32_t kPhiloxDomainMfq = 0x5EED1u;
constexpr uint32_t kPhiloxDomainMc = 0x5EED2u;

__device__ __forceinline__ double philox_uniform_in(uint32_t domain, uint32_t seed, uint32_t rep, uint32_t t,
                                                    uint32_t i) {
    uint32_t c[4] = {i, t, rep, domain};
    philox(c, seed, 0xA511E9B3u);
    const uint64_t bits = ((uint64_t)(c[0] >> 5) << 26) | (c[1] >> 6);   // 53 bits, like random_sample
    return (double)bits * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ double philox_uniform(uint32_t seed, uint32_t rep, uint32_t t, uint32_t i) {
    return philox_uniform_in(kPhiloxDomainMfq, seed, rep, t, i);
}

}  // namespace mfx
