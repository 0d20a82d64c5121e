// ising_engine.cpp -- host runtime + C ABI of the Ising lattice and tabular MF-Q kernels.
//
// The reference has no native layer here (everything is python: examples/ising_model and
// main_MFQ_Ising.py).  This ABI is what this repository's drop-in `examples.ising_model`
// package and `mfrl_amd.ising` bind through ctypes; host buffers in, host buffers out.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ising_kernels.h"
#include "mfx_common.h"
#include "../../include/magent_amd.h"

namespace mfx {

struct IsingEngine {
    int R = 1, N = 0, K = 0;
    hipStream_t stream = nullptr;
    DevBuf<int16_t> nbr;
    DevBuf<uint8_t> spins, obs, spins_out;
    DevBuf<int32_t> actions, n_up, steps;
    DevBuf<double> reward, order, q, u, order_t;
    DevBuf<uint32_t> mask;
    DevBuf<int32_t> nup_t;
    DevBuf<int32_t> err;
    // the trace / sweep / Metropolis calls (part 3b of the header)
    DevBuf<double> temps, rsum_t, mse_t, acc;
    DevBuf<int32_t> stream_of;
    DevBuf<uint8_t> spins_s;                                 // [n_streams][N] the streams' env.reset spins
    hipEvent_t mark[2] = {nullptr, nullptr};                 // mfx_ising_mark
    // mfx_ising_mfq_run_stream's two pass slots: pass p's words are generated and walked (gen stream) into slot
    // p % 2 while pass p - 1's episode runs out of the other (stream)
    struct Slot {
        DevBuf<uint32_t> words, off[2], mask;
        DevBuf<uint16_t> perm;
        DevBuf<double> q, order_t;
        DevBuf<int32_t> nup_t, steps;
        hipEvent_t produced = nullptr, consumed = nullptr;
    } slot[2];
    hipStream_t gen = nullptr;
    ~IsingEngine() {
        for (auto& m : mark)
            if (m) (void)hipEventDestroy(m);
        for (auto& sl : slot) {
            if (sl.produced) (void)hipEventDestroy(sl.produced);
            if (sl.consumed) (void)hipEventDestroy(sl.consumed);
        }
        if (gen) (void)hipStreamDestroy(gen);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

}  // namespace mfx

using mfx::IsingEngine;

extern "C" {

// R replicas of an N-agent lattice whose neighbour table nbr[N][K] (ascending ids) comes from
// Ising.py:_calc_mask (computed by the python Scenario).
MFX_API int mfx_ising_create(int R, int N, int K, const int16_t* nbr, void** handle) {
    if (R < 1 || N < 1 || N > 32767 || K < 1 || K > 16) return mfx::fail("ising: need 1 <= N <= 32767, 1 <= K <= 16");
    try {
        auto* e = new IsingEngine();
        e->R = R; e->N = N; e->K = K;
        MFX_HIP_THROW(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
        e->nbr.ensure((size_t)N * K);
        MFX_HIP_THROW(hipMemcpy(e->nbr.p, nbr, sizeof(int16_t) * N * K, hipMemcpyHostToDevice));
        e->spins.ensure((size_t)R * N);
        MFX_HIP_THROW(hipMemset(e->spins.p, 0, (size_t)R * N));
        *handle = e;
        return 0;
    } catch (const std::exception& ex) {
        return mfx::fail("%s", ex.what());
    }
}

MFX_API int mfx_ising_destroy(void* h) { delete static_cast<IsingEngine*>(h); return 0; }

MFX_API int mfx_ising_set_spins(void* h, const uint8_t* spins) {
    auto* e = static_cast<IsingEngine*>(h);
    MFX_HIP(hipMemcpy(e->spins.p, spins, (size_t)e->R * e->N, hipMemcpyHostToDevice));
    return 0;
}

MFX_API int mfx_ising_get_spins(void* h, uint8_t* spins) {
    auto* e = static_cast<IsingEngine*>(h);
    MFX_HIP(hipMemcpy(spins, e->spins.p, (size_t)e->R * e->N, hipMemcpyDeviceToHost));
    return 0;
}

// One IsingMultiAgentEnv.step for every replica: actions [R][N] -> rewards [R][N] f64,
// observations [R][N][K] u8 (neighbour spins), n_up [R], order parameter [R].
MFX_API int mfx_ising_step(void* h, const int32_t* actions, double* reward, uint8_t* obs, int32_t* n_up,
                           double* order) {
    auto* e = static_cast<IsingEngine*>(h);
    const size_t RN = (size_t)e->R * e->N;
    try {
        e->actions.ensure(RN); e->reward.ensure(RN); e->obs.ensure(RN * e->K); e->n_up.ensure(e->R);
        e->order.ensure(e->R);
    } catch (const std::exception& ex) {
        return mfx::fail("%s", ex.what());
    }
    MFX_HIP(hipMemcpyAsync(e->actions.p, actions, sizeof(int32_t) * RN, hipMemcpyHostToDevice, e->stream));
    MFX_HIP(mfx::launch_ising_step(e->R, e->N, e->K, e->nbr.p, e->spins.p, e->actions.p, e->reward.p, e->obs.p,
                                   e->n_up.p, e->order.p, e->stream));
    MFX_HIP(hipMemcpyAsync(reward, e->reward.p, sizeof(double) * RN, hipMemcpyDeviceToHost, e->stream));
    MFX_HIP(hipMemcpyAsync(obs, e->obs.p, RN * e->K, hipMemcpyDeviceToHost, e->stream));
    MFX_HIP(hipMemcpyAsync(n_up, e->n_up.p, sizeof(int32_t) * e->R, hipMemcpyDeviceToHost, e->stream));
    MFX_HIP(hipMemcpyAsync(order, e->order.p, sizeof(double) * e->R, hipMemcpyDeviceToHost, e->stream));
    MFX_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

// The whole tabular MF-Q episode of main_MFQ_Ising.py for every replica, starting from the
// current spins.  u: host [R][T][N] uniforms or null (Philox, `seed`); mask: host
// [R][T][ceil(N/32)] act_group bits or null (act_rate 1).  Outputs (host, nullable except q):
// q [R][N][K+1][2], order [R][T], n_up [R][T], steps [R]; spins are updated in place.
MFX_API int mfx_ising_mfq_run(void* h, int T, double temperature, double lr, double decay_rate, int decay_gap,
                              const double* u, const uint32_t* mask, unsigned seed, double* q, double* order,
                              int32_t* n_up, int32_t* steps) {
    auto* e = static_cast<IsingEngine*>(h);
    const int R = e->R, N = e->N, K = e->K, words = (N + 31) / 32;
    if (T < 1) return mfx::fail("ising mfq: T must be >= 1");
    if (decay_gap < 1) return mfx::fail("ising mfq: decay_gap must be >= 1");
    mfx::IsingMfqArgs a{};
    try {
        if (u) {
            e->u.ensure((size_t)R * T * N);
            MFX_HIP_THROW(hipMemcpyAsync(e->u.p, u, sizeof(double) * R * T * N, hipMemcpyHostToDevice, e->stream));
        }
        if (mask) {
            e->mask.ensure((size_t)R * T * words);
            MFX_HIP_THROW(hipMemcpyAsync(e->mask.p, mask, sizeof(uint32_t) * R * T * words, hipMemcpyHostToDevice,
                                         e->stream));
        }
        e->q.ensure((size_t)R * N * (K + 1) * 2);
        e->order_t.ensure((size_t)R * T);
        e->nup_t.ensure((size_t)R * T);
        e->steps.ensure(R);
        e->spins_out.ensure((size_t)R * N);
    } catch (const std::exception& ex) {
        return mfx::fail("%s", ex.what());
    }
    a.N = N; a.K = K; a.T = T; a.nbr = e->nbr.p; a.spins0 = e->spins.p;
    a.u = u ? e->u.p : nullptr; a.mask = mask ? e->mask.p : nullptr;
    a.temperature = temperature; a.lr = lr; a.decay_rate = decay_rate; a.decay_gap = decay_gap; a.seed = seed;
    a.q_out = e->q.p; a.order_out = e->order_t.p; a.nup_out = e->nup_t.p; a.spins_out = e->spins_out.p;
    a.steps_out = e->steps.p;
    MFX_HIP(mfx::launch_ising_mfq(a, R, e->stream));
    MFX_HIP(hipMemcpyAsync(e->spins.p, e->spins_out.p, (size_t)R * N, hipMemcpyDeviceToDevice, e->stream));
    MFX_HIP(hipMemcpyAsync(q, e->q.p, sizeof(double) * R * N * (K + 1) * 2, hipMemcpyDeviceToHost, e->stream));
    if (order) MFX_HIP(hipMemcpyAsync(order, e->order_t.p, sizeof(double) * R * T, hipMemcpyDeviceToHost, e->stream));
    if (n_up) MFX_HIP(hipMemcpyAsync(n_up, e->nup_t.p, sizeof(int32_t) * R * T, hipMemcpyDeviceToHost, e->stream));
    if (steps) MFX_HIP(hipMemcpyAsync(steps, e->steps.p, sizeof(int32_t) * R, hipMemcpyDeviceToHost, e->stream));
    MFX_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

// main_MFQ_Ising.py with its numpy stream generated on the device (k_mt_words, k_ising_scan): replica r is the
// script run with seed seed0 + r -- RandomState(seed0 + r), make_world's N discarded choice(2) draws, then per
// episode env.reset's N spins and per step the N Boltzmann uniforms and the act_group permutation
// (choice(N, int(act_rate N), replace=False)) -- for `episodes` episodes in sequence on the one stream, each until
// its own early stop (-epi).  Nothing is read back between episodes: the next episode's first draw is found on the
// device from the steps the previous one ran.  Outputs (host; nullable except q), per episode:
// q [E][R][N][K+1][2], order [E][R][T], n_up [E][R][T], steps [E][R]; the spins end as the last episode left them.
MFX_API int mfx_ising_mfq_run_stream(void* h, int T, double temperature, double lr, double decay_rate, int decay_gap,
                                     double act_rate, unsigned seed0, int episodes, double* q, double* order,
                                     int32_t* n_up, int32_t* steps) {
    auto* e = static_cast<IsingEngine*>(h);
    const int R = e->R, N = e->N, K = e->K, mw = (N + 31) / 32;
    if (T < 1 || episodes < 1) return mfx::fail("ising mfq stream: T and episodes must be >= 1");
    if (decay_gap < 1) return mfx::fail("ising mfq stream: decay_gap must be >= 1");
    if (!(act_rate >= 0.0 && act_rate <= 1.0)) return mfx::fail("ising mfq stream: act_rate must be in [0, 1]");
    const int n_upd = (int)(act_rate * N);                  // int(act_rate * n_agents), main_MFQ_Ising.py:126
    // words per replica: make_world's N, then per episode N spins and per step 2 N uniforms + the permutation's
    // draws (N - 1 accepted words plus rejections: ~0.5 N expected, bounded here by 2 N -- a walk past the end sets
    // the error word) + one chunk of read-ahead (k_ising_scan reads 64 words at a time; its prefetch clamps at the stride)
    const size_t per = (size_t)N + (size_t)episodes * ((size_t)N + (size_t)T * 4 * N) + 320;
    const size_t blocks_z = (per + 623) / 624;
    const size_t W = blocks_z * 624;
    // the per-step word offsets (k_ising_scan's off, k_ising_mfq's woff, the next episode's prev_off) are 32-bit
    if (W > (size_t)UINT32_MAX)
        return mfx::fail("ising mfq stream: %zu words per replica (episodes x T x 4 N) exceed the 32-bit word offsets; "
                         "run fewer episodes per call or mode 'host'", W);
    const int blocks = (int)blocks_z;
    // replicas per pass: a slot's word streams within 64 GB and a third of the free memory.  Big passes: the walk
    // is one latency-bound wave per replica, so a pass's walk takes about as long whatever its replicas -- 16384
    // replicas at 2000 steps: 3.41e10 spin-steps/s in 16-GB passes, 3.86e10 in 64-GB ones (MFX_ISING_PASS_GB: A/B only)
    const char* pg = getenv("MFX_ISING_PASS_GB");
    size_t pass_bytes = (size_t)64 << 30;
    {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess && fr / 3 < pass_bytes) pass_bytes = std::max<size_t>(fr / 3, (size_t)1 << 30);
    }
    if (pg) pass_bytes = (size_t)std::max(1, atoi(pg)) << 30;
    const int Rb = (int)std::max<size_t>(1, std::min<size_t>((size_t)R, pass_bytes / (W * 4)));
    const int P = (R + Rb - 1) / Rb;                           // passes
    const size_t QR = (size_t)N * (K + 1) * 2;
    try {
        for (int k = 0; k < std::min(P, 2); ++k) {
            auto& sl = e->slot[k];
            sl.words.ensure((size_t)Rb * W);
            for (auto& o : sl.off) o.ensure((size_t)Rb * (T + 1));
            if (n_upd < N) { sl.perm.ensure((size_t)Rb * N); sl.mask.ensure((size_t)Rb * T * mw); }
            sl.q.ensure((size_t)Rb * QR);
            sl.order_t.ensure((size_t)Rb * T);
            sl.nup_t.ensure((size_t)Rb * T);
            sl.steps.ensure(Rb);
            if (!sl.produced) MFX_HIP_THROW(hipEventCreateWithFlags(&sl.produced, hipEventDisableTiming));
            if (!sl.consumed) MFX_HIP_THROW(hipEventCreateWithFlags(&sl.consumed, hipEventDisableTiming));
        }
        if (!e->gen) MFX_HIP_THROW(hipStreamCreateWithFlags(&e->gen, hipStreamNonBlocking));
        e->err.ensure(1);
        e->spins_out.ensure((size_t)R * N);
    } catch (const std::exception& ex) {
        return mfx::fail("%s", ex.what());
    }
    MFX_HIP(hipMemsetAsync(e->err.p, 0, sizeof(int32_t), e->stream));
    hipStream_t gs = e->gen;                                         // the generation's own stream
    {   // the gen stream starts after the error word is cleared
        hipEvent_t ready = e->slot[0].consumed;
        MFX_HIP(hipEventRecord(ready, e->stream));
        MFX_HIP(hipStreamWaitEvent(e->gen, ready, 0));
    }
    auto scan = [&](IsingEngine::Slot& sl, int r0, int nr, int ep, hipStream_t st) -> hipError_t {
        mfx::IsingScanArgs sa{};
        sa.N = N; sa.T = T; sa.n_upd = n_upd; sa.words = sl.words.p; sa.wstride = W;
        sa.prev_off = ep ? sl.off[(ep - 1) & 1].p : nullptr;
        sa.prev_steps = ep ? sl.steps.p : nullptr;
        sa.spins0 = e->spins.p + (size_t)r0 * N;
        sa.off = sl.off[ep & 1].p;
        sa.mask = n_upd < N ? sl.mask.p : nullptr;
        sa.perm = n_upd < N ? sl.perm.p : nullptr;
        sa.err = e->err.p;
        return mfx::launch_ising_scan(sa, nr, st);
    };
    // pass p's generation and first walk (gen stream), into slot p % 2 once pass p - 2 has released it
    auto produce = [&](int p) -> hipError_t {
        auto& sl = e->slot[p & 1];
        const int r0 = p * Rb, nr = std::min(Rb, R - r0);
        hipError_t err;
        if (p >= 2 && (err = hipStreamWaitEvent(gs, sl.consumed, 0)) != hipSuccess) return err;
        if ((err = mfx::launch_mt_words(seed0, r0, nr, blocks, sl.words.p, W, gs)) != hipSuccess) return err;
        if ((err = scan(sl, r0, nr, 0, gs)) != hipSuccess) return err;
        return hipEventRecord(sl.produced, gs);
    };
    MFX_HIP(produce(0));
    if (P > 1) MFX_HIP(produce(1));
    for (int p = 0; p < P; ++p) {
        auto& sl = e->slot[p & 1];
        const int r0 = p * Rb, nr = std::min(Rb, R - r0);
        MFX_HIP(hipStreamWaitEvent(e->stream, sl.produced, 0));
        for (int ep = 0; ep < episodes; ++ep) {
            if (ep) MFX_HIP(scan(sl, r0, nr, ep, e->stream));       // (after the previous episode's early stop)
            mfx::IsingMfqArgs a{};
            a.N = N; a.K = K; a.T = T; a.nbr = e->nbr.p; a.spins0 = e->spins.p + (size_t)r0 * N;
            a.words = sl.words.p; a.woff = sl.off[ep & 1].p; a.wstride = W;
            a.mask = n_upd < N ? sl.mask.p : nullptr;
            a.temperature = temperature; a.lr = lr; a.decay_rate = decay_rate; a.decay_gap = decay_gap;
            a.q_out = sl.q.p; a.order_out = sl.order_t.p; a.nup_out = sl.nup_t.p;
            a.spins_out = e->spins_out.p + (size_t)r0 * N; a.steps_out = sl.steps.p;
            MFX_HIP(mfx::launch_ising_mfq(a, nr, e->stream));
            const size_t er = (size_t)ep * R + r0;               // this pass's rows of episode ep's outputs
            MFX_HIP(hipMemcpyAsync(q + er * QR, sl.q.p, sizeof(double) * nr * QR, hipMemcpyDeviceToHost, e->stream));
            if (order)
                MFX_HIP(hipMemcpyAsync(order + er * T, sl.order_t.p, sizeof(double) * nr * T, hipMemcpyDeviceToHost,
                                       e->stream));
            if (n_up)
                MFX_HIP(hipMemcpyAsync(n_up + er * T, sl.nup_t.p, sizeof(int32_t) * nr * T, hipMemcpyDeviceToHost,
                                       e->stream));
            if (steps)
                MFX_HIP(hipMemcpyAsync(steps + er, sl.steps.p, sizeof(int32_t) * nr, hipMemcpyDeviceToHost, e->stream));
        }
        MFX_HIP(hipEventRecord(sl.consumed, e->stream));
        if (p + 2 < P) MFX_HIP(produce(p + 2));
    }
    MFX_HIP(hipMemcpyAsync(e->spins.p, e->spins_out.p, (size_t)R * N, hipMemcpyDeviceToDevice, e->stream));
    int32_t err = 0;
    MFX_HIP(hipMemcpyAsync(&err, e->err.p, sizeof(err), hipMemcpyDeviceToHost, e->stream));
    MFX_HIP(hipStreamSynchronize(e->stream));
    if (err) return mfx::fail("ising mfq stream: a replica's draws ran past its %zu generated words", W);
    return 0;
}

/* ------------------------------------------------------------------ part 3b: trace, sweep, Metropolis */

namespace {

// every temperature finite and above zero (the Boltzmann exponent divides by it)
int check_temps(const char* who, const double* temps, int R) {
    for (int r = 0; r < R; ++r)
        if (!(temps[r] > 0.0) || !std::isfinite(temps[r]))
            return mfx::fail("%s: temperature %g of replica %d is not a finite value above zero", who, temps[r], r);
    return 0;
}

// rows a replica never writes read as NaN (every byte 0xFF is a quiet NaN)
hipError_t fill_nan(double* p, size_t n, hipStream_t st) { return hipMemsetAsync(p, 0xFF, sizeof(double) * n, st); }

}  // namespace

// mfx_ising_mfq_run (host u or Philox, host mask, from the current spins) with a clamp temperature per replica
// (temps[R]; null: `temperature`) and the per-step trace: rsum [R][T] and mse [R][T] (nullable), NaN past a
// replica's stop step.
MFX_API int mfx_ising_mfq_run_trace(void* h, int T, double temperature, const double* temps, double lr,
                                    double decay_rate, int decay_gap, const double* u, const uint32_t* mask,
                                    unsigned seed, double* q, double* order, int32_t* n_up, int32_t* steps,
                                    double* rsum, double* mse) {
    auto* e = static_cast<IsingEngine*>(h);
    const int R = e->R, N = e->N, K = e->K, words = (N + 31) / 32;
    if (T < 1) return mfx::fail("ising mfq trace: T must be >= 1");
    if (decay_gap < 1) return mfx::fail("ising mfq trace: decay_gap must be >= 1");
    if (temps && check_temps("ising mfq trace", temps, R)) return -1;
    mfx::IsingMfqArgs a{};
    try {
        if (u) {
            e->u.ensure((size_t)R * T * N);
            MFX_HIP_THROW(hipMemcpyAsync(e->u.p, u, sizeof(double) * R * T * N, hipMemcpyHostToDevice, e->stream));
        }
        if (mask) {
            e->mask.ensure((size_t)R * T * words);
            MFX_HIP_THROW(hipMemcpyAsync(e->mask.p, mask, sizeof(uint32_t) * R * T * words, hipMemcpyHostToDevice,
                                         e->stream));
        }
        if (temps) {
            e->temps.ensure(R);
            MFX_HIP_THROW(hipMemcpyAsync(e->temps.p, temps, sizeof(double) * R, hipMemcpyHostToDevice, e->stream));
        }
        e->q.ensure((size_t)R * N * (K + 1) * 2);
        e->order_t.ensure((size_t)R * T);
        e->nup_t.ensure((size_t)R * T);
        e->rsum_t.ensure((size_t)R * T);
        e->mse_t.ensure((size_t)R * T);
        e->steps.ensure(R);
        e->spins_out.ensure((size_t)R * N);
    } catch (const std::exception& ex) {
        return mfx::fail("%s", ex.what());
    }
    MFX_HIP(fill_nan(e->rsum_t.p, (size_t)R * T, e->stream));
    MFX_HIP(fill_nan(e->mse_t.p, (size_t)R * T, e->stream));
    a.N = N; a.K = K; a.T = T; a.nbr = e->nbr.p; a.spins0 = e->spins.p;
    a.u = u ? e->u.p : nullptr; a.mask = mask ? e->mask.p : nullptr;
    a.temperature = temperature; a.lr = lr; a.decay_rate = decay_rate; a.decay_gap = decay_gap; a.seed = seed;
    a.q_out = e->q.p; a.order_out = e->order_t.p; a.nup_out = e->nup_t.p; a.spins_out = e->spins_out.p;
    a.steps_out = e->steps.p;
    a.temps = temps ? e->temps.p : nullptr; a.rsum_out = e->rsum_t.p; a.mse_out = e->mse_t.p;
    MFX_HIP(mfx::launch_ising_mfq_trace(a, R, e->stream));
    MFX_HIP(hipMemcpyAsync(e->spins.p, e->spins_out.p, (size_t)R * N, hipMemcpyDeviceToDevice, e->stream));
    MFX_HIP(hipMemcpyAsync(q, e->q.p, sizeof(double) * R * N * (K + 1) * 2, hipMemcpyDeviceToHost, e->stream));
    if (order) MFX_HIP(hipMemcpyAsync(order, e->order_t.p, sizeof(double) * R * T, hipMemcpyDeviceToHost, e->stream));
    if (n_up) MFX_HIP(hipMemcpyAsync(n_up, e->nup_t.p, sizeof(int32_t) * R * T, hipMemcpyDeviceToHost, e->stream));
    if (steps) MFX_HIP(hipMemcpyAsync(steps, e->steps.p, sizeof(int32_t) * R, hipMemcpyDeviceToHost, e->stream));
    if (rsum) MFX_HIP(hipMemcpyAsync(rsum, e->rsum_t.p, sizeof(double) * R * T, hipMemcpyDeviceToHost, e->stream));
    if (mse) MFX_HIP(hipMemcpyAsync(mse, e->mse_t.p, sizeof(double) * R * T, hipMemcpyDeviceToHost, e->stream));
    MFX_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

// A temperature sweep in one launch: single episode, reference-stream mode.  n_streams numpy streams
// (RandomState(seed0 + s)) are generated and walked once (k_mt_words, k_ising_scan); replica r runs the script at
// temps[r] on stream stream_of[r] (null: stream r, n_streams == R), as the script run with one seed at several -t.
// Outputs (host; nullable except q): q [R][N][K+1][2], order / rsum / mse [R][T] (NaN past the stop step),
// n_up [R][T], steps [R]; the spins end as each replica left them.
MFX_API int mfx_ising_mfq_run_sweep(void* h, int T, const double* temps, const int32_t* stream_of, int n_streams,
                                    unsigned seed0, double lr, double decay_rate, int decay_gap, double act_rate,
                                    double* q, double* order, int32_t* n_up, int32_t* steps, double* rsum,
                                    double* mse) {
    auto* e = static_cast<IsingEngine*>(h);
    const int R = e->R, N = e->N, K = e->K, mw = (N + 31) / 32;
    if (T < 1) return mfx::fail("ising mfq sweep: T must be >= 1");
    if (decay_gap < 1) return mfx::fail("ising mfq sweep: decay_gap must be >= 1");
    if (!(act_rate >= 0.0 && act_rate <= 1.0)) return mfx::fail("ising mfq sweep: act_rate must be in [0, 1]");
    if (!temps) return mfx::fail("ising mfq sweep: temps is required");
    if (n_streams < 1) return mfx::fail("ising mfq sweep: n_streams must be >= 1");
    if (!stream_of && n_streams != R)
        return mfx::fail("ising mfq sweep: without stream_of every replica reads its own stream: n_streams %d != "
                         "the handle's %d replicas", n_streams, R);
    if (check_temps("ising mfq sweep", temps, R)) return -1;
    if (stream_of)
        for (int r = 0; r < R; ++r)
            if (stream_of[r] < 0 || stream_of[r] >= n_streams)
                return mfx::fail("ising mfq sweep: stream_of[%d] = %d is outside [0, %d)", r, stream_of[r], n_streams);
    const int n_upd = (int)(act_rate * N);
    const size_t per = (size_t)N + ((size_t)N + (size_t)T * 4 * N) + 320;      // as mfx_ising_mfq_run_stream, one episode
    const size_t blocks_z = (per + 623) / 624;
    const size_t W = blocks_z * 624;
    if (W > (size_t)UINT32_MAX)
        return mfx::fail("ising mfq sweep: %zu words per stream (T x 4 N) exceed the 32-bit word offsets", W);
    {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess && (size_t)n_streams * W * 4 > fr / 2)
            return mfx::fail("ising mfq sweep: %d streams of %zu words do not fit in half the free device memory; "
                             "sweep fewer seeds per call", n_streams, W);
    }
    auto& sl = e->slot[0];
    const size_t QR = (size_t)N * (K + 1) * 2;
    try {
        sl.words.ensure((size_t)n_streams * W);
        sl.off[0].ensure((size_t)n_streams * (T + 1));
        if (n_upd < N) { sl.perm.ensure((size_t)n_streams * N); sl.mask.ensure((size_t)n_streams * T * mw); }
        e->spins_s.ensure((size_t)n_streams * N);
        e->temps.ensure(R);
        if (stream_of) e->stream_of.ensure(R);
        e->q.ensure((size_t)R * QR);
        e->order_t.ensure((size_t)R * T);
        e->nup_t.ensure((size_t)R * T);
        e->rsum_t.ensure((size_t)R * T);
        e->mse_t.ensure((size_t)R * T);
        e->steps.ensure(R);
        e->spins_out.ensure((size_t)R * N);
        e->err.ensure(1);
    } catch (const std::exception& ex) {
        return mfx::fail("%s", ex.what());
    }
    hipStream_t st = e->stream;
    MFX_HIP(hipMemsetAsync(e->err.p, 0, sizeof(int32_t), st));
    MFX_HIP(hipMemcpyAsync(e->temps.p, temps, sizeof(double) * R, hipMemcpyHostToDevice, st));
    if (stream_of)
        MFX_HIP(hipMemcpyAsync(e->stream_of.p, stream_of, sizeof(int32_t) * R, hipMemcpyHostToDevice, st));
    MFX_HIP(fill_nan(e->order_t.p, (size_t)R * T, st));
    MFX_HIP(fill_nan(e->rsum_t.p, (size_t)R * T, st));
    MFX_HIP(fill_nan(e->mse_t.p, (size_t)R * T, st));
    MFX_HIP(mfx::launch_mt_words(seed0, 0, n_streams, (int)blocks_z, sl.words.p, W, st));
    mfx::IsingScanArgs sa{};
    sa.N = N; sa.T = T; sa.n_upd = n_upd; sa.words = sl.words.p; sa.wstride = W;
    sa.spins0 = e->spins_s.p; sa.off = sl.off[0].p;
    sa.mask = n_upd < N ? sl.mask.p : nullptr;
    sa.perm = n_upd < N ? sl.perm.p : nullptr;
    sa.err = e->err.p;
    MFX_HIP(mfx::launch_ising_scan(sa, n_streams, st));
    mfx::IsingMfqArgs a{};
    a.N = N; a.K = K; a.T = T; a.nbr = e->nbr.p; a.spins0 = e->spins_s.p;
    a.words = sl.words.p; a.woff = sl.off[0].p; a.wstride = W;
    a.mask = n_upd < N ? sl.mask.p : nullptr;
    a.temperature = temps[0]; a.lr = lr; a.decay_rate = decay_rate; a.decay_gap = decay_gap;
    a.q_out = e->q.p; a.order_out = e->order_t.p; a.nup_out = e->nup_t.p; a.spins_out = e->spins_out.p;
    a.steps_out = e->steps.p;
    a.temps = e->temps.p; a.stream_of = stream_of ? e->stream_of.p : nullptr;
    a.rsum_out = e->rsum_t.p; a.mse_out = e->mse_t.p;
    MFX_HIP(mfx::launch_ising_mfq_trace(a, R, st));
    MFX_HIP(hipMemcpyAsync(e->spins.p, e->spins_out.p, (size_t)R * N, hipMemcpyDeviceToDevice, st));
    MFX_HIP(hipMemcpyAsync(q, e->q.p, sizeof(double) * R * QR, hipMemcpyDeviceToHost, st));
    if (order) MFX_HIP(hipMemcpyAsync(order, e->order_t.p, sizeof(double) * R * T, hipMemcpyDeviceToHost, st));
    if (n_up) MFX_HIP(hipMemcpyAsync(n_up, e->nup_t.p, sizeof(int32_t) * R * T, hipMemcpyDeviceToHost, st));
    if (steps) MFX_HIP(hipMemcpyAsync(steps, e->steps.p, sizeof(int32_t) * R, hipMemcpyDeviceToHost, st));
    if (rsum) MFX_HIP(hipMemcpyAsync(rsum, e->rsum_t.p, sizeof(double) * R * T, hipMemcpyDeviceToHost, st));
    if (mse) MFX_HIP(hipMemcpyAsync(mse, e->mse_t.p, sizeof(double) * R * T, hipMemcpyDeviceToHost, st));
    int32_t err = 0;
    MFX_HIP(hipMemcpyAsync(&err, e->err.p, sizeof(err), hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    if (err) return mfx::fail("ising mfq sweep: a stream's draws ran past its %zu generated words", W);
    return 0;
}

// Metropolis baseline (k_ising_mc) from the current spins: `sweeps` checkerboard sweeps of every replica under its
// acceptance row acc[r][0..4] (host, each in [0, 1]).  4-neighbour lattices of even side only.  Outputs (host):
// order [R][sweeps], n_up [R][sweeps]; the spins are updated in place.
MFX_API int mfx_ising_mc_run(void* h, int sweeps, const double* acc, unsigned seed, double* order, int32_t* n_up) {
    auto* e = static_cast<IsingEngine*>(h);
    const int R = e->R, N = e->N, K = e->K;
    int L = 0;
    while (L * L < N) ++L;
    if (K != 4)
        return mfx::fail("ising mc: the checkerboard Metropolis kernel runs the 4-neighbour lattice (view 1), not K = %d",
                         K);
    if (L * L != N || (L & 1) || L < 4)
        return mfx::fail("ising mc: the checkerboard needs a square lattice of even side >= 4, not N = %d", N);
    if (sweeps < 1) return mfx::fail("ising mc: sweeps must be >= 1");
    if (!acc || !order || !n_up) return mfx::fail("ising mc: acc, order and n_up are required");
    for (int k = 0; k < R * 5; ++k)
        if (!(acc[k] >= 0.0 && acc[k] <= 1.0)) return mfx::fail("ising mc: acc[%d][%d] = %g is not in [0, 1]", k / 5, k % 5, acc[k]);
    try {
        e->acc.ensure((size_t)R * 5);
        e->order_t.ensure((size_t)R * sweeps);
        e->nup_t.ensure((size_t)R * sweeps);
    } catch (const std::exception& ex) {
        return mfx::fail("%s", ex.what());
    }
    MFX_HIP(hipMemcpyAsync(e->acc.p, acc, sizeof(double) * R * 5, hipMemcpyHostToDevice, e->stream));
    mfx::IsingMcArgs a{};
    a.N = N; a.L = L; a.sweeps = sweeps; a.nbr = e->nbr.p; a.spins = e->spins.p; a.acc = e->acc.p; a.seed = seed;
    a.order_out = e->order_t.p; a.nup_out = e->nup_t.p;
    MFX_HIP(mfx::launch_ising_mc(a, R, e->stream));
    MFX_HIP(hipMemcpyAsync(order, e->order_t.p, sizeof(double) * R * sweeps, hipMemcpyDeviceToHost, e->stream));
    MFX_HIP(hipMemcpyAsync(n_up, e->nup_t.p, sizeof(int32_t) * R * sweeps, hipMemcpyDeviceToHost, e->stream));
    MFX_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

// An event pair on the engine's stream around whatever calls run between mark(0) and mark(1) (measurement only).
MFX_API int mfx_ising_mark(void* h, int which) {
    auto* e = static_cast<IsingEngine*>(h);
    if (which < 0 || which > 1) return mfx::fail("ising mark: which is 0 (start) or 1 (stop)");
    if (!e->mark[which]) MFX_HIP(hipEventCreate(&e->mark[which]));
    MFX_HIP(hipEventRecord(e->mark[which], e->stream));
    return 0;
}

MFX_API int mfx_ising_marked_ms(void* h, float* ms) {
    auto* e = static_cast<IsingEngine*>(h);
    if (!e->mark[0] || !e->mark[1]) return mfx::fail("ising marked_ms: mark 0 and mark 1 first");
    MFX_HIP(hipEventSynchronize(e->mark[1]));
    MFX_HIP(hipEventElapsedTime(ms, e->mark[0], e->mark[1]));
    return 0;
}

}  // extern "C"
