// battle_dropin.cpp -- the Battle engine's drop-in path (env 0, host buffers): the host cache, the deferred and fast
// step, the resident server and the host_* calls of the reference ABI.
#include "battle_engine.h"

namespace mfx {

size_t BattleEngine::info_off(int g, int what) const {         // in the record at info_src
    const size_t r = info_src_rows;
    const size_t base = 64 + (size_t)g * (((r * kInfoRowBytes) + 15) & ~(size_t)15);
    if (what == kGetId) return base;
    if (what == kGetReward) return base + r * 4;
    if (what == kGetPos) return base + r * 8;
    return base + r * 16;                                        // kGetAlive
}

// Queue the record's launch and its one copy to pinned memory (no sync).
int BattleEngine::queue_info() {
    const int G = n_groups();
    size_t rows = 1;
    for (int g = 0; g < G; g++) rows = std::max(rows, (size_t)std::max(group_ub[g], 1));
    try {
        if (rows > info_rows) info_rows = rows;
        st_info.ensure(64 + (size_t)G * info_region());
        pin_info.ensure(64 + (size_t)G * info_region());
    } catch (const HipFailure& f) {
        return fail("%s", f.what());
    }
    MFX_HIP(launch_get_env0(d_gp, s, st_info.p, (int)info_rows, stream));
    MFX_HIP(hipMemcpyAsync(pin_info.p, st_info.p, 64 + (size_t)G * info_region(), hipMemcpyDeviceToHost, stream));
    return 0;
}

// after the sync that follows queue_info (or k_dropin_step): this epoch's group sizes and info are
// on the host, in the record at src
int BattleEngine::take_info(const uint8_t* src, size_t rows) {
    info_src = src ? src : pin_info.p;
    info_src_rows = src ? rows : info_rows;
    for (int g = 0; g < n_groups(); g++) hn[g] = info_hdr()[g];
    n_ep = info_ep = epoch;
    return report_err(info_hdr()[kMaxGroups]);
}

int BattleEngine::ensure_info() {
    if (info_ep == epoch) return 0;
    MFX_CHECK(flush_deferred());
    MFX_CHECK(queue_info());
    MFX_HIP(hipStreamSynchronize(stream));
    return take_info();
}

int BattleEngine::num_env0(int g) {
    if (!allocated) return 0;
    if (ensure_counts() != 0) return 0;
    return hn[g];
}

size_t BattleEngine::obs_row_bytes() const {
    size_t b = 0;
    for (int g = 0; g < n_groups(); g++) {
        const TypeParams& T = gp.type[g];
        b = std::max(b, (size_t)4 * ((size_t)T.view_w * T.view_h * gp.n_ch + gp.feat_size[g]));
    }
    return (b + 15) & ~(size_t)15;
}

// views + features of every group of env 0 (and the info of the same epoch) in one transfer
int BattleEngine::ensure_obs() {
    if (obs_ep == epoch) return 0;
    MFX_CHECK(flush_deferred());
    MFX_CHECK(ensure_counts());
    obs_fast = false;
    const int G = n_groups();
    int rowcap = 4;
    for (int g = 0; g < G; g++) rowcap = std::max(rowcap, group_ub[g]);
    rowcap = (rowcap + 3) & ~3;
    size_t vmax = 0, fmax = 0;
    for (int g = 0; g < G; g++) {
        const TypeParams& T = gp.type[g];
        vmax = std::max(vmax, (size_t)T.view_w * T.view_h * gp.n_ch);
        fmax = std::max(fmax, (size_t)gp.feat_size[g]);
    }
    try {
        obs_rows = std::max(obs_rows, (size_t)rowcap);
        st_view.ensure((size_t)G * E * rowcap * (vmax + fmax));   // (+ fmax: the packed one-env layout)
        st_feat.ensure((size_t)G * E * rowcap * fmax);
        pin_obs.ensure((size_t)G * obs_rows * obs_row_bytes());
    } catch (const HipFailure& f) {
        return fail("%s", f.what());
    }
    obs_packed = E == 1;
    if (obs_packed) {
        // one env: every group's views, each followed by its features, back to back in the
        // staging buffer and in pin_obs -- one copy for all of it
        size_t off = 0;
        for (int g = 0; g < G; g++) {
            const TypeParams& T = gp.type[g];
            const size_t VF = (size_t)T.view_w * T.view_h * gp.n_ch, F = gp.feat_size[g];
            obs_pack_off[g] = off;
            if (!hn[g]) continue;
            float* dv = st_view.p + off;
            MFX_CHECK(observe(g, dv, dv + (size_t)hn[g] * VF, rowcap));
            off += (size_t)hn[g] * (VF + F);
        }
        if (off) MFX_HIP(hipMemcpyAsync(pin_obs.p, st_view.p, sizeof(float) * off, hipMemcpyDeviceToHost, stream));
    } else {
        for (int g = 0; g < G; g++) {
            if (!hn[g]) continue;
            const TypeParams& T = gp.type[g];
            const size_t VF = (size_t)T.view_w * T.view_h * gp.n_ch, F = gp.feat_size[g];
            float* dv = st_view.p + (size_t)g * E * rowcap * vmax;
            float* df = st_feat.p + (size_t)g * E * rowcap * fmax;
            MFX_CHECK(observe(g, dv, df, rowcap));
            uint8_t* hv = pin_obs.p + obs_off_view(g);
            MFX_HIP(hipMemcpyAsync(hv, dv, sizeof(float) * hn[g] * VF, hipMemcpyDeviceToHost, stream));
            MFX_HIP(hipMemcpyAsync(hv + sizeof(float) * obs_rows * VF, df, sizeof(float) * hn[g] * F,
                                   hipMemcpyDeviceToHost, stream));
        }
    }
    MFX_CHECK(queue_info());                 // this epoch's ids (and the error word) ride along
    MFX_HIP(hipStreamSynchronize(stream));
    obs_ep = epoch;
    return take_info();
}

// ------------------------------------------------------------------ drop-in (env 0, host buffers)
// The fast step applies to one env whose config the fused rollout supports and whose image plus
// step / observation scratch fits one workgroup's LDS.
size_t BattleEngine::fast_rows_now() const {
    size_t r = 4;
    for (int g = 0; g < n_groups(); g++) r = std::max(r, (size_t)group_ub[g]);
    return (r + 3) & ~(size_t)3;
}
bool BattleEngine::fast_dropin_ok() const {
    if (!fast_enabled || E != 1 || !allocated || gp.dsl || turn || food) return false;
    for (int g = 0; g < n_groups(); g++) {
        const TypeParams& T = gp.type[g];
        if (T.body_w != 1 || T.body_h != 1 || T.view_w != gp.type[0].view_w || T.view_h != gp.type[0].view_h)
            return false;
    }
    return dropin_smem_bytes(gp, s.cells_n, s.cap, s.acap, (int)fast_rows_now()) <= kLdsBytes;
}

int BattleEngine::ensure_mbox() {
    if (mbox.p) return 0;
    try { mbox.ensure(1, hipHostMallocCoherent); } catch (const HipFailure& f) { return fail("%s", f.what()); }
    memset(mbox.p, 0, sizeof(DropinMailbox));
    return 0;
}

// Run deferred set_action / clear_dead for real, in call order (clear_dead came first).
// Stop the resident server (if one may be running) and wait until it has left: its LDS image
// must not outlive a change made by anything else, and nothing else may wait behind it.
int BattleEngine::quiesce() {
    if (!res_live) return 0;
    res_live = false;
    DropinMailbox* mb = mbox.p;
    mb->cmd = kDropinStop;
    __atomic_store_n(&mb->req, ++fast_seq, __ATOMIC_RELEASE);
    MFX_HIP(hipStreamSynchronize(stream));
    return 0;
}
int BattleEngine::flush_deferred() {
    MFX_CHECK(quiesce());
    bool acts = false;
    for (int g = 0; g < kMaxGroups; g++) acts |= defer_act[g];
    spec_ep = 0;
    if (!defer_clear && !acts) return 0;
    if (defer_clear) {
        defer_clear = false;
        MFX_HIP(launch_clear_dead(d_gp, s, stream));
    }
    for (int g = 0; g < n_groups(); g++) {
        if (!defer_act[g]) continue;
        defer_act[g] = false;
        const int rowcap = std::max(group_ub[g], 1);
        try { st_i32.ensure((size_t)E * rowcap); } catch (const HipFailure& f) { return fail("%s", f.what()); }
        if (defer_n[g])
            MFX_HIP(hipMemcpyAsync(st_i32.p, pin_fact.p + (size_t)g * fact_rows, sizeof(int) * defer_n[g],
                                   hipMemcpyHostToDevice, stream));
        MFX_HIP(launch_set_action(d_gp, s, g, st_i32.p, rowcap, stream));
    }
    if (acts) MFX_HIP(hipStreamSynchronize(stream));   // pin_fact may be rewritten next
    return 0;
}
// set_action deferred: the actions wait in host-mapped memory for the step's launch.
int BattleEngine::fast_set_action(int g, const int* actions) {
    if (defer_act[g]) MFX_CHECK(flush_deferred());      // a second call for the group before a step
    const int n = num_env0(g);
    const size_t rows = fast_rows_now();
    try {
        if (fact_rows < rows || pin_fact.n < (size_t)n_groups() * rows) {
            MFX_CHECK(flush_deferred());
            MFX_HIP_THROW(hipStreamSynchronize(stream));
            fact_rows = std::max(fact_rows, rows);
            pin_fact.ensure((size_t)n_groups() * fact_rows, hipHostMallocCoherent);
        }
        pending_ub += group_ub[g];
        ensure_capacity(0, pending_ub);
    } catch (const HipFailure& f) {
        return fail("%s", f.what());
    }
    if (n) memcpy(pin_fact.p + (size_t)g * fact_rows, actions, sizeof(int) * n);
    // the resident server also finds them in its mailbox, tagged with the request that will carry
    // them (read in the same poll as the request, battle/dropin.inc dropin_wait)
    mail_tag[g] = ~0u;
    if (res_enabled && own_stream && env_flag("MFX_DROPIN_MAIL", false) &&
        (size_t)n_groups() * fact_rows <= (size_t)kMailActs) {
        bool ok = true;
        for (int i = 0; i < n && ok; i++) ok = (uint32_t)actions[i] <= 0xFFFFu;
        if (ok) {
            if (ensure_mbox() != 0) return -1;
            const uint32_t tag = (fast_seq + 1) & 0xFFFFu;
            uint32_t* d = mbox.p->acts + (size_t)g * fact_rows;
            for (int i = 0; i < n; i++) d[i] = (tag << 16) | (uint32_t)actions[i];
            mail_tag[g] = tag;
            mail_stride[g] = fact_rows;
        }
    }
    acts_since_step[g]++;
    defer_act[g] = true;
    defer_n[g] = n;
    const int keep_n = n_ep == epoch;
    touch();
    ro_prep_stale = true;
    spec_ep = 0;
    if (keep_n) n_ep = epoch;                           // group sizes do not change
    return 0;
}
// env.step(): one k_dropin_step launch and one sync.

int BattleEngine::fast_step(int* done) {
#ifdef MFX_STAMPS
    hst_t0 = std::chrono::steady_clock::now();
#endif
    touch();
    ro_prep_stale = true;
    MFX_CHECK(sync_cells());
    const int G = n_groups();
    const size_t rows = fast_rows_now();
    DropinArgs da{};
    try {
        const size_t rec = (64 + (size_t)G * (((rows * kInfoRowBytes) + 15) & ~(size_t)15) + 255) & ~(size_t)255;
        // rec | observation set 0 | set 1: request k writes set k & 1, so the arrays a caller got
        // from get_observation (mfx_env_observation_view) stay intact through the next step
        size_t off = rec;
        size_t vo[kMaxGroups], fo[kMaxGroups];
        for (int g = 0; g < G; g++) {
            const TypeParams& T = gp.type[g];
            vo[g] = off; off = (off + rows * T.view_w * T.view_h * gp.n_ch * 4 + 255) & ~(size_t)255;
            fo[g] = off; off = (off + rows * gp.feat_size[g] * 4 + 255) & ~(size_t)255;
        }
        const size_t set_bytes = off - rec;
        off += set_bytes;
        if (pin_fast.n < off || (res_live && (int)rows != res_da.rows)) {
            if (quiesce() != 0) throw HipFailure("quiesce failed");
            MFX_HIP_THROW(hipStreamSynchronize(stream));   // the last launch may still write it
            if (pin_fast.n < off && pin_fast.p) {           // callers may still hold views of it
                retired.push_back(pin_fast.p);
                pin_fast.p = pin_fast.d = nullptr;
                pin_fast.n = 0;
            }
            pin_fast.ensure(off, hipHostMallocCoherent);
        }
        fast_set_bytes = set_bytes;
        if (!pin_flag.p) {
            pin_flag.ensure(2, hipHostMallocCoherent);
            pin_flag.p[0] = pin_flag.p[1] = 0;
        }
        fast_rows = rows;
        fast_rec = rec;
        for (int g = 0; g < G; g++) { fast_view[g] = vo[g]; fast_feat[g] = fo[g]; }
    } catch (const HipFailure& f) {
        return fail("%s", f.what());
    }
    for (int g = 0; g < G; g++) {
        da.acts[g] = defer_act[g] ? pin_fact.d + (size_t)g * fact_rows : nullptr;
        da.n_acts[g] = defer_act[g] ? defer_n[g] : 0;
        da.view[g] = reinterpret_cast<float*>(pin_fast.d + fast_view[g]);
        da.feat[g] = reinterpret_cast<float*>(pin_fast.d + fast_feat[g]);
    }
    da.pending_clear = defer_clear;
    da.obs_alt = fast_set_bytes / sizeof(float);
    da.rows = (int)rows;
    da.rec_step = pin_fast.d;
    da.flag = pin_flag.d;
    begin_step();
    fast_res = res_enabled && own_stream && !s.serial_step;
    if (fast_res) {
        MFX_CHECK(ensure_mbox());
        DropinMailbox* mb = mbox.p;
        const uint32_t seq = ++fast_seq;
        bool tagged = true;
        for (int g = 0; g < G; g++)
            if (defer_act[g] && (mail_tag[g] != (seq & 0xFFFFu) || mail_stride[g] != fact_rows)) tagged = false;
        mb->cmd = kDropinStep;
        mb->pending_clear = defer_clear;
        for (int g = 0; g < kMaxGroups; g++) mb->n_acts[g] = g < G && defer_act[g] ? defer_n[g] : -1;
        mb->tagged = tagged;
        mb->act_stride = (int32_t)std::max<size_t>(fact_rows, 1);
        // a server that left on its idle timeout wrote the last request it answered into done[3]
        // on its way out: relaunch it at once (wait_fast's stream query would notice ~100 us later)
        if (res_live && __atomic_load_n(&mb->done[3], __ATOMIC_ACQUIRE) == seq - 1) res_live = false;
        __atomic_store_n(&mb->req, seq, __ATOMIC_RELEASE);
        if (!res_live) {
            for (int g = 0; g < G; g++) da.acts[g] = pin_fact.d + (size_t)g * fact_rows;
            da.mb = mbox.d;
            da.seq = seq - 1;
            da.idle = res_idle_ticks();
            {   // MFX_DROPIN_MAIL=1: poll the tagged actions with the header (just the words they need)
                const size_t words = 16 + (size_t)G * fact_rows;
                da.mail_passes = words <= 256 ? 1 : words <= (size_t)kMailWords ? 2 : 0;
                if (!env_flag("MFX_DROPIN_MAIL", false)) da.mail_passes = 0;   // measured neutral: off
            }
            da.variant = res_variant();
            res_da = da;
            MFX_HIP(launch_dropin_step(gp, d_gp, s, da, stream));
            res_live = true;
        }
    } else {
        MFX_CHECK(quiesce());
        da.seq = ++fast_seq;
        const hipError_t le = launch_dropin_step(gp, d_gp, s, da, stream);
        MFX_HIP(le);
    }
    s.serial_step = 0;
    obs_seq = fast_seq;
#ifdef MFX_STAMPS
    hst_t1 = std::chrono::steady_clock::now();
#endif
    MFX_CHECK(wait_fast(0, fast_seq));        // the records; the observation is still being written
#ifdef MFX_STAMPS
    const auto hst_t2 = std::chrono::steady_clock::now();
#endif
    defer_clear = false;
    for (int g = 0; g < kMaxGroups; g++) defer_act[g] = false;
    pending_ub = 0;
    MFX_CHECK(take_info(pin_fast.p, rows));
    *done = info_hdr()[kMaxGroups + 1];
    spec_ep = epoch;
#ifdef MFX_STAMPS
    const auto hst_t3 = std::chrono::steady_clock::now();
    hst[0] += std::chrono::duration<double, std::micro>(hst_t1 - hst_t0).count();
    hst[1] += std::chrono::duration<double, std::micro>(hst_t2 - hst_t1).count();
    hst[2] += std::chrono::duration<double, std::micro>(hst_t3 - hst_t2).count();
    hst_n++;
#endif
    return 0;
}
// Spin on k_dropin_step's completion word `which` (0 records, 1 observation) of request `seq`.
// The stream is polled now and then, so a failed or faulted launch is reported instead of awaited;
// a resident server that left on its idle timeout before seeing the request is launched again.
int BattleEngine::wait_fast(int which, uint32_t seq) {
    const bool res = fast_res;
    volatile uint32_t* f = res ? &mbox.p->done[which] : pin_flag.p + which;
    // the stream is queried every ~100 us of waiting (a query costs microseconds; polling it by
    // iteration count delayed the detection of the word)
    const auto t_start = std::chrono::steady_clock::now();
    auto t_next = t_start + std::chrono::microseconds(100);
    for (uint32_t k = 1, relaunched = 0;; k++) {
        if (*f == seq) break;
        if ((k & 63) == 0 && std::chrono::steady_clock::now() >= t_next) {
            t_next = std::chrono::steady_clock::now() + std::chrono::microseconds(100);
            if (t_next - t_start > std::chrono::seconds(20))
                return fail("k_dropin_step: request %u unanswered after 20 s (word %d = %u)", seq, which, *f);
            const hipError_t q = hipStreamQuery(stream);
            if (q == hipSuccess) {
                if (*f == seq) break;
                if (res && res_live && seq == fast_seq && relaunched < 2) {
                    DropinArgs da = res_da;      // the request is still posted: serve it
                    da.seq = seq - 1;
                    MFX_HIP(launch_dropin_step(gp, d_gp, s, da, stream));
                    relaunched++;
                    res_relaunch++;
                    continue;
                }
                return fail("k_dropin_step finished without publishing word %d", which);
            }
            if (q != hipErrorNotReady) return fail("k_dropin_step: %s", hipGetErrorString(q));
        }
        __builtin_ia32_pause();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return 0;
}
int BattleEngine::res_variant() {
    static const int v = env_int("MFX_DROPIN_VARIANT", 0);
    return v;
}
long long BattleEngine::res_idle_us() {                       // (read each time: tests change it)
    return std::max(1, env_int("MFX_DROPIN_IDLE_US", 2000));
}
unsigned long long BattleEngine::res_idle_ticks() const {
    int dev = 0, khz = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess ||
        khz <= 0)
        khz = 100000;                                  // gfx9: 100 MHz
    return (unsigned long long)res_idle_us() * (unsigned long long)khz / 1000ull;
}
// clear_dead right after a fast step: deferred; the step's launch already left what the getters
// and get_observation ask next.
int BattleEngine::fast_clear_dead() {
    defer_clear = true;
    touch();
    ro_prep_stale = true;
    spec_ep = 0;
    // the record after clear_dead, from the step's record (clear_dead_env): the alive rows in
    // order, reward = next_r + group reward = step_reward + 0
    const size_t rows = fast_rows, region = ((rows * kInfoRowBytes) + 15) & ~(size_t)15;
    clr_rec.resize(fast_rec);
    const uint8_t* src = pin_fast.p;
    uint8_t* dst = clr_rec.data();
    memcpy(dst, src, 64);
    int32_t* hdr = reinterpret_cast<int32_t*>(dst);
    for (int g = 0; g < n_groups(); g++) {
        const int n = std::min(hdr[g], (int)rows);
        const uint8_t* b = src + 64 + (size_t)g * region;
        uint8_t* o = dst + 64 + (size_t)g * region;
        const int32_t* ids = reinterpret_cast<const int32_t*>(b);
        const int32_t* pos = reinterpret_cast<const int32_t*>(b + rows * 8);
        const uint8_t* alive = b + rows * 16;
        int32_t* oids = reinterpret_cast<int32_t*>(o);
        float* orew = reinterpret_cast<float*>(o + rows * 4);
        int32_t* opos = reinterpret_cast<int32_t*>(o + rows * 8);
        uint8_t* oalive = o + rows * 16;
        volatile float zero = 0.0f;
        const float r = gp.type[g].step_reward + zero;
        int k = 0;
        for (int i = 0; i < n; i++) {
            if (!alive[i]) continue;
            oids[k] = ids[i]; orew[k] = r; opos[2 * k] = pos[2 * i]; opos[2 * k + 1] = pos[2 * i + 1]; oalive[k] = 1;
            k++;
        }
        hdr[g] = k;
    }
    MFX_CHECK(take_info(dst, rows));
    obs_fast = true;
    obs_ep = epoch;
    return 0;
}

int BattleEngine::host_observe(int g, float** bufs) {
    if (!allocated) return fail("get_observation before reset");
    if (g < 0 || g >= n_groups()) return fail("get_observation: bad group %d", g);
    MFX_CHECK(ensure_obs());
    const int n = hn[g];
    if (n == 0) return 0;
    const TypeParams& T = gp.type[g];
    const size_t VF = (size_t)T.view_w * T.view_h * gp.n_ch, F = gp.feat_size[g];
    if (obs_fast) {
        MFX_CHECK(wait_fast(1, obs_seq));
        const size_t o = (obs_seq & 1) ? fast_set_bytes : 0;
        memcpy(bufs[0], pin_fast.p + o + fast_view[g], sizeof(float) * n * VF);
        memcpy(bufs[1], pin_fast.p + o + fast_feat[g], sizeof(float) * n * F);
        return 0;
    }
    if (obs_packed) {
        const float* hv = reinterpret_cast<const float*>(pin_obs.p) + obs_pack_off[g];
        memcpy(bufs[0], hv, sizeof(float) * n * VF);
        memcpy(bufs[1], hv + (size_t)n * VF, sizeof(float) * n * F);
        return 0;
    }
    const uint8_t* hv = pin_obs.p + obs_off_view(g);
    memcpy(bufs[0], hv, sizeof(float) * n * VF);
    memcpy(bufs[1], hv + sizeof(float) * obs_rows * VF, sizeof(float) * n * F);
    return 0;
}
// get_observation without the copy: host pointers to env 0's observation of group g, written by
// the drop-in step into pinned memory (the set of the last request; the next request writes the
// other set, so they stay valid until the step after next).  1: not available (the caller copies
// through host_observe).
int BattleEngine::observation_view(int g, float** view, float** feat, int* n, int* rows) {
    if (!allocated) return fail("get_observation before reset");
    if (g < 0 || g >= n_groups()) return fail("get_observation: bad group %d", g);
    MFX_CHECK(ensure_obs());
    if (!obs_fast) return 1;
    MFX_CHECK(wait_fast(1, obs_seq));
    const size_t o = (obs_seq & 1) ? fast_set_bytes : 0;
    *view = reinterpret_cast<float*>(pin_fast.p + o + fast_view[g]);
    *feat = reinterpret_cast<float*>(pin_fast.p + o + fast_feat[g]);
    *n = hn[g];
    *rows = (int)fast_rows;
    return 0;
}
// No sync: the actions go out of pinned memory (one region per group, reused once the previous
// copy from it has left), the launch is queued, device errors surface at the next cache fetch.
int BattleEngine::host_set_action(int g, const int* actions) {
    if (!allocated) return fail("set_action before reset");
    if (g < 0 || g >= n_groups()) return fail("set_action: bad group %d", g);
    if (fast_dropin_ok()) return fast_set_action(g, actions);
    const int n = num_env0(g);
    const int rowcap = std::max(group_ub[g], 1);
    try {
        st_i32.ensure((size_t)E * rowcap);
        if (pin_act.n < (size_t)n_groups() * rowcap) {
            MFX_HIP_THROW(hipStreamSynchronize(stream));            // no copy may be in flight
            pin_act.ensure((size_t)n_groups() * rowcap);
        }
        if (!act_ev[g]) MFX_HIP_THROW(hipEventCreateWithFlags(&act_ev[g], hipEventDisableTiming));
    } catch (const HipFailure& f) {
        return fail("%s", f.what());
    }
    const size_t stride = pin_act.n / n_groups();
    int32_t* pa = pin_act.p + (size_t)g * stride;
    MFX_HIP(hipEventSynchronize(act_ev[g]));
    if (n) {
        memcpy(pa, actions, sizeof(int) * n);
        MFX_HIP(hipMemcpyAsync(st_i32.p, pa, sizeof(int) * n, hipMemcpyHostToDevice, stream));
        MFX_HIP(hipEventRecord(act_ev[g], stream));
    }
    const int keep_n = n_ep == epoch;
    MFX_CHECK(set_action(g, st_i32.p, rowcap));   // a state change: last_act feeds the features
    if (keep_n) n_ep = epoch;                     // group sizes do not change
    return 0;
}
int BattleEngine::host_step(int* done) {
    if (!allocated) return fail("step before reset");
    if (fast_dropin_ok()) return fast_step(done);
    MFX_CHECK(step(nullptr));
    MFX_CHECK(queue_info());                   // done + rewards / alive / positions in one transfer
    MFX_HIP(hipStreamSynchronize(stream));
    *done = info_hdr()[kMaxGroups + 1];
    return take_info();
}
// clear_dead without a sync: with this epoch's alive flags at hand, the new group sizes are known.
int BattleEngine::host_clear_dead() {
    if (spec_ep != 0 && spec_ep == epoch) return fast_clear_dead();
    const int G = n_groups();
    int nn[kMaxGroups] = {};
    const bool known = allocated && info_ep == epoch && n_ep == epoch;
    if (known)
        for (int g = 0; g < G; g++) {
            const uint8_t* al = info_src + info_off(g, kGetAlive);
            for (int i = 0; i < hn[g]; i++) nn[g] += al[i] != 0;
        }
    MFX_CHECK(clear_dead());
    if (known) { for (int g = 0; g < G; g++) hn[g] = nn[g]; n_ep = epoch; }
    return 0;
}
int BattleEngine::host_get(int g, int what, void* out, size_t elem_bytes) {
    if (g < 0 || g >= n_groups()) return fail("get: bad group %d", g);
    const int n = num_env0(g);
    if (n == 0) return 0;
    if (what == kGetId || what == kGetReward || what == kGetPos || what == kGetAlive) {
        MFX_CHECK(ensure_info());
        memcpy(out, info_src + info_off(g, what), elem_bytes * n);
        return 0;
    }
    const int rowcap = std::max(group_ub[g], 1);
    st_u8.ensure((size_t)E * rowcap * elem_bytes);
    MFX_CHECK(get(g, what, st_u8.p, rowcap));
    MFX_HIP(hipMemcpyAsync(out, st_u8.p, elem_bytes * n, hipMemcpyDeviceToHost, stream));
    MFX_HIP(hipStreamSynchronize(stream));
    return check_err();
}

// One call per getter of the drop-in wrapper (mfx_env_get_rows): the group's size n, and for what 0 id /
// 1 reward / 2 alive / 3 pos the n rows copied into out when n <= cap (what -1: the size only).
int BattleEngine::get_rows(int g, int what, void* out, int cap) {
    MFX_CHECK(sync_cells());
    if (g < 0 || g >= n_groups()) return fail("get_rows: bad group %d", g);
    if (what < -1 || what > 3) return fail("get_rows: bad field %d", what);
    if (!allocated) return 0;
    MFX_CHECK(ensure_counts());
    const int n = hn[g];
    if (what < 0 || n == 0 || n > cap) return n;
    static const int field[4] = {kGetId, kGetReward, kGetAlive, kGetPos};
    static const size_t bytes[4] = {4, 4, 1, 8};
    MFX_CHECK(host_get(g, field[what], out, bytes[what]));
    return n;
}

}  // namespace mfx
