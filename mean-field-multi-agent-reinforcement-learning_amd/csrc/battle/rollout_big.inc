// Part of battle_kernels.hip (one translation unit; included in order, not compiled alone):
// large envs: k_obs_prep, k_observe_items, k_step_big, k_rollout_big
// ==================================================================================
//  envs too large for one workgroup's LDS (256x256 / 4096 agents): state stays in HBM
// ==================================================================================
// One 1024-lane workgroup per env.  LDS holds the step scratch (BigScratch), the move order and,
// for the rollout, the action buffers; the cells and per-id arrays are read and written in place.
constexpr int kBigThreads = 1024;
#ifndef MFX_BIG_ROLLOUT_THREADS
#define MFX_BIG_ROLLOUT_THREADS 512
#endif
// k_rollout_big shares its CUs with the other sub-batch's k_observe: 8 waves of <= 128 VGPRs and
// ~80 KB of LDS leave room for observation workgroups beside it
constexpr int kBigRolloutThreads = MFX_BIG_ROLLOUT_THREADS;

// lds_env (the few-env path, RolloutArgs::lds_step): the env itself is staged in LDS for its step --
// the env image of k_rollout (carve_env), its group counters and the action buffers.
struct BigLayout { size_t sm, atk, mov, sorted, ahist, red, big, img, cnt, act, rid, hist, total; };

__host__ __device__ inline BigLayout big_layout(const GameParams& gp, int cap, int acap, bool rollout,
                                                bool lds_env = false) {
    auto r16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    BigLayout L;
    size_t o = 0;
    L.sm = o;     o += step_sm_bytes(gp.n_groups);
    L.atk = o;    o += lds_env ? r16((size_t)acap * 4) : 0;   // else the attack / move buffers are State::atk /
    L.mov = o;    o += lds_env ? r16((size_t)acap * 4) : 0;   //   mov (HBM)
    L.sorted = o; o += (gp.large_map && !rollout) ? r16((size_t)acap * 4) : 0;   // rollout: RolloutArgs::big_sort
    L.ahist = o;  o += rollout ? r16((size_t)gp.n_groups * 64 * 4) : 0;
    size_t big = big_scratch_bytes(acap, cap, true, gp.large_map != 0);
    if (lds_env && step_par_bytes(acap, cap) > big) big = step_par_bytes(acap, cap);   // few_env_step's team forms
    L.big = o;    o += r16(big);
    L.red = L.big;                   // block_sum runs after the step: the step scratch is dead
    L.img = o;    o += lds_env ? env_image_bytes(gp.W * gp.H, cap, gp.n_groups) : 0;
    L.cnt = o;    o += lds_env ? 16 * 3 : 0;          // grp_n, grp_dead, grp_reward
    L.act = o;    o += lds_env ? r16((size_t)gp.n_groups * cap * 4) : 0;   // few_env_step: the actions
    L.rid = o;    o += lds_env ? r16((size_t)cap * 2) : 0;                 // few_env_step: the reference ids
    L.hist = o;   o += lds_env ? r16((size_t)gp.n_groups * 13 * 13 * 4) : 0;   // few_snapshot: minimap counts, zero
    L.total = o;
    return L;
}

size_t big_step_smem_bytes(const GameParams& gp, int cap, int acap, bool rollout, bool lds_env) {
    return big_layout(gp, cap, acap, rollout, lds_env).total;
}

// The inputs every observing chunk of env e shares (Battle shape): the per-group minimap density
// (obs_minimap) and the packed hp/max | group word of every listed agent, written to HBM once.
// hist: G * 169 ints of LDS.
__device__ void obs_prep_env(const GameParams& gp, const EnvView& v, float* __restrict__ mm_out,
                             uint32_t* __restrict__ info_out, int* hist) {
    constexpr int VW = BattleShape::VW, VH = BattleShape::VH, NV = VW * VH, G = BattleShape::G;
    const int sw = (gp.W + VW - 1) / VW, sh = (gp.H + VH - 1) / VH;
    for (int i = TID; i < G * NV; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (int j = 0; j < G; ++j) {
        const int n = v.grp_n[j];
        const float mx = gp.type[j].hp;
        for (int i = TID; i < n; i += blockDim.x) {
            const int id = v.grp_ids[j * v.cap + i];
            const uint32_t p = v.xy[id];
            atomicAdd(&hist[j * NV + ((int)(p >> 16) / sh) * VW + (int)(p & 0xFFFF) / sw], 1);
            info_out[id] = __float_as_uint(v.hp[id] / mx) | ((uint32_t)j << 31);
        }
    }
    __syncthreads();
    for (int i = TID; i < G * NV; i += blockDim.x) {
        const int n = v.grp_n[i / NV];
        mm_out[i] = n ? (float)hist[i] / (float)n : __uint_as_float(0xFFC00000u);
    }
}

// File env e's observation work items for the step of parity par: one item per obs_item_rows
// agents of each group (lane 0; one atomic per env).
__device__ __forceinline__ void obs_file_items(const RolloutArgs& ra, const EnvView& v, int G, int e, int par) {
    if (TID != 0 || !ra.obs_items) return;
    const int R = ra.obs_item_rows;
    int k = 0;
    for (int g = 0; g < G; ++g) k += (v.grp_n[g] + R - 1) / R;
    if (!k) return;
    const int l = e % ra.obs_lists;
    const int base = atomicAdd(ra.obs_cnt + (par * kXcds + l) * kObsCntPad, k);
    uint32_t* out = ra.obs_items + par * ra.obs_par_stride + l * ra.obs_list_stride + base;
    for (int g = 0, j = 0; g < G; ++g)
        for (int c = 0; c * R < v.grp_n[g]; ++c) out[j++] = ((uint32_t)e << 12) | ((uint32_t)g << 10) | (uint32_t)c;
}

__global__ void __launch_bounds__(256) k_obs_prep(const GameParams* __restrict__ gp, State s, RolloutArgs ra, int par) {
    __shared__ int hist[BattleShape::G * BattleShape::VW * BattleShape::VH];
    constexpr int NV = BattleShape::VW * BattleShape::VH;
    const int e = blockIdx.x;
    const EnvView v = global_view(s, e, gp->n_groups);
    obs_prep_env(*gp, v, ra.obs_mm + (size_t)e * BattleShape::G * NV, ra.obs_info + (size_t)e * s.cap, hist);
    obs_file_items(ra, v, gp->n_groups, e, par);
}

// get_observation of every group of the large envs as a stream of work items (obs_item_rows agents
// of one group of one env each), taken by persistent workgroups from the list the previous step
// filed, so the launch stays balanced whatever the spread of group sizes.  The shared inputs
// (minimap, per-id info) come from obs_prep_env; the cells and the info words are read from HBM
// kObsPf 64-cell blocks at a time.  A workgroup takes items from its own XCD's list first (list
// blockIdx % obs_lists: the items of one env stay on one XCD, so its cells and info words are fetched
// into one L2, not eight) and then helps the other lists.  Workgroup 0 clears the other parity's
// counters for the next step's filing (the previous k_rollout_big has finished with them).
__global__ void __launch_bounds__(256) k_observe_items(const GameParams* __restrict__ gpp, State s, RolloutArgs ra,
                                                       int par) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int item;
    constexpr int NV = BattleShape::VW * BattleShape::VH, NC = BattleShape::NC, F = BattleShape::F;
    const GameParams& gp = *gpp;
    const int G = BattleShape::G, R = ra.obs_item_rows, W = gp.W, H = gp.H;
    const int lane = TID & 63, wid = TID >> 6, nw = blockDim.x >> 6;
    size_t off = 0;
    ObsSmem sm = carve_obs(smem, gp, 0, 0, R, obs_stage_floats(gp, 0, true, blockDim.x), true, off);
    obs_prologue(gp, sm, 0);
    if (blockIdx.x == 0 && TID < 2 * kXcds) ra.obs_cnt[((par ^ 1) * kXcds + (TID >> 1)) * kObsCntPad + (TID & 1)] = 0;
    const int L = ra.obs_lists, x = (int)(blockIdx.x % (unsigned)L);
    int li = 0;                                      // lists exhausted so far (x, x + 1, ...)
    float* st = sm.stage + wid * kWaveStageFloats;
    while (true) {
        if (TID == 0) {
            int got = -1;
            for (; li < L; ++li) {
                const int l = (x + li) % L;
                int32_t* c = ra.obs_cnt + (par * kXcds + l) * kObsCntPad;
                const int i = atomicAdd(c + 1, 1);
                if (i < c[0]) { got = (int)ra.obs_items[par * ra.obs_par_stride + l * ra.obs_list_stride + i]; break; }
            }
            item = got;
        }
        __syncthreads();
        const int it = item;
        if (it < 0) break;
        const int e = it >> 12, g = (it >> 10) & 3, a0 = (it & 1023) * R;
        const EnvView v = global_view(s, e, G);
        const int na = min(R, v.grp_n[g] - a0);
        const float* mmg = ra.obs_mm + (size_t)e * G * NV;
        for (int i = TID; i < G * NV; i += blockDim.x) sm.mm[i] = mmg[i];
        EnvView vc = v;
        vc.grp_ids = v.grp_ids + a0;
        obs_agent_records(gp, vc, sm, g, na);
        __syncthreads();
        const TypeParams& T = gp.type[g];
        float* ov = ra.view[g] + ((size_t)e * ra.rowcap + a0) * (NV * NC);
        float* of = ra.feat[g] + ((size_t)e * ra.rowcap + a0) * F;
        const float* mm_own = sm.mm + g * NV;
        const float* mm_en = sm.mm + (g ^ 1) * NV;
        g_u16* cells = (g_u16*)v.cells;
        g_cu32* info = (g_cu32*)(ra.obs_info + (size_t)e * s.cap);
        const int ncell = na * NV;
        for (int base = wid * kObsPf * kWaveCells; base < ncell; base += nw * kObsPf * kWaveCells) {
            CellPre p[kObsPf];
            uint32_t cv[kObsPf], inf[kObsPf];
#pragma unroll
            for (int d = 0; d < kObsPf; ++d)
                p[d] = obs_cell_pre(sm, mm_own, mm_en, W, H, base + d * kWaveCells + lane, ncell);
#pragma unroll
            for (int d = 0; d < kObsPf; ++d) cv[d] = cells[p[d].idx];
#pragma unroll
            for (int d = 0; d < kObsPf; ++d) inf[d] = info[(p[d].ok && cv[d] < kCellFood) ? cv[d] : 0u];
#pragma unroll
            for (int d = 0; d < kObsPf; ++d) {
                const int b = base + d * kWaveCells;
                if (b >= ncell) break;
                obs_stage_cell(st, lane, obs_cell_post_g(p[d], cv[d], inf[d], g));
                wave_sync_lds();
                obs_flush(ov + (size_t)b * NC, st, lane, min(kWaveCells, ncell - b));
                wave_sync_lds();
            }
        }
        // features (GridWorld.cc:411-421)
        const int emb = gp.emb, nact = T.n_action;
        for (int q = TID; q < na * F; q += blockDim.x) {
            const int a = q / F, f = q - a * F;
            const int id = vc.grp_ids[g * v.cap + a];
            float val = 0.0f;
            if (f < emb) val = (float)((v.rid[id] >> f) & 1);
            if (f == emb + (int)last_action(v.last_act[id])) val = 1.0f;
            if (f == emb + nact) val = v.last_r[id];
            const uint32_t pos = v.xy[id];
            if (f == emb + nact + 1) val = (float)(int)(pos & 0xFFFF) / (float)W;
            if (f == emb + nact + 2) val = (float)(int)(pos >> 16) / (float)H;
            __builtin_nontemporal_store(val, of + q);
        }
        __syncthreads();                               // LDS (records, minimap, item) is reused
    }
}

// GridWorld::step for one env per workgroup, in place in HBM (the per-call path's large envs).
__global__ void __launch_bounds__(kBigThreads) k_step_big(const GameParams* __restrict__ gpp, State s) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const GameParams& gp = *gpp;
    const int e = blockIdx.x;
    const BigLayout L = big_layout(gp, s.cap, s.acap, false);
    StepSmem& sm = *reinterpret_cast<StepSmem*>(smem + L.sm);
    const BigScratch bs = carve_big(smem + L.big, s.acap, s.cap, true, gp.large_map != 0);
    EnvView v = global_view(s, e, gp.n_groups);
    uint32_t rng = s.rng[e];
    int done = 0;
    load_serial_types(gp, sm);
    step_env_core<false, false, true>(gp, s, v, s.atk + (size_t)e * s.acap, s.n_atk[e], s.mov + (size_t)e * s.acap,
                                      s.n_mov[e], reinterpret_cast<uint32_t*>(smem + L.sorted), rng, sm, done, false,
                                      ParScratch{}, s.id_counter[e], nullptr, 0, &bs);
    if (TID == 0) {
        s.rng[e] = rng;
        s.n_atk[e] = 0;
        s.n_mov[e] = 0;
        s.done[e] = done;
    }
}

// clear_dead (GridWorld.cc:696-728: ordered compaction + Agent::init_reward) that also renumbers the
// slots to the list order: the live agents of group 0, then of group 1, ... take slots 0, 1, ... in
// the order clear_dead keeps.  Without it a slot is the agent's id for the whole episode and the live
// agents (10-20 % of a 256x256 episode's 4096 ids late in a fight) are scattered over every 128-B line
// of each per-slot array, so the next step fetches nearly all of them; with it they are dense.  The
// ids move along in rid (features, get_agent_id and the policy keys read rid), and every live
// agent's cell takes its new slot number.  Two passes through LDS records (16 B per live agent): every
// old slot is read before any new one is written.  rec: >= 16 * (live agents) bytes of LDS.
// full: rewrite every live agent's slot even when none moves (MFX_RENUMBER=2, A/B only).
__device__ void clear_dead_renumber(const GameParams& gp, const State& s, EnvView& v, int e, uint4* rec, int* wave_tot,
                                    bool full) {
    __shared__ int gb[kMaxGroups + 1];        // first new slot of each group (LDS: indexed by a lane's group)
    const int G = gp.n_groups, W = gp.W;
    int nb = 0, moved = 0;
    for (int g = 0; g < G; ++g) {
        if (TID == 0) gb[g] = nb;
        const int n = v.grp_n[g];
        const uint16_t* ids = v.grp_ids + g * v.cap;
        for (int i0 = 0; i0 < n; i0 += blockDim.x) {
            const int i = i0 + TID;
            int id = 0, alive = 0;
            uint32_t m = 0;
            if (i < n) { id = ids[i]; m = v.meta[id]; alive = !meta_dead(m); }
            int tot;
            const int r = team_scan<false>(alive, wave_tot, tot);
            if (alive) {
                const uint32_t mk = meta_keep_dir(meta_make(0, kOpNull, g), m);
                rec[nb + r] = make_uint4(v.xy[id], __float_as_uint(v.hp[id]), __float_as_uint(v.next_r[id]),
                                         (uint32_t)v.rid[id] | (mk << 16) | ((uint32_t)v.last_act[id] << 24));
                moved |= nb + r != id;
            }
            nb += tot;
        }
    }
    if (TID == 0) gb[G] = nb;
    // no live agent changes slot (no death since the last renumbering, or only at the end of the slot range):
    // the slots and cells stand; clear_dead's own fields and the compacted lists change
    if (!__syncthreads_or(moved || full)) {
        for (int k = TID; k < nb; k += blockDim.x) {
            const uint4 r = rec[k];
            const uint32_t mk = (r.w >> 16) & 0xFFu;
            const int g = (int)meta_group(mk);
            v.last_r[k] = __uint_as_float(r.z);
            v.next_r[k] = gp.type[g].step_reward;
            v.op_obj[k] = -1;
            v.meta[k] = (uint8_t)mk;
            v.grp_ids[g * v.cap + (k - gb[g])] = (uint16_t)k;     // (a dead list entry may precede it)
        }
    } else {
    for (int k = TID; k < nb; k += blockDim.x) {
        const uint4 r = rec[k];
        const uint32_t mk = (r.w >> 16) & 0xFFu;
        const int g = (int)meta_group(mk);
        v.xy[k] = r.x;
        v.hp[k] = __uint_as_float(r.y);
        v.last_r[k] = __uint_as_float(r.z);
        v.next_r[k] = gp.type[g].step_reward;
        v.op_obj[k] = -1;
        v.meta[k] = (uint8_t)mk;
        v.last_act[k] = (uint8_t)(r.w >> 24);
        v.rid[k] = (uint16_t)(r.w & 0xFFFFu);
        v.cells[(r.x >> 16) * W + (r.x & 0xFFFFu)] = (uint16_t)k;
        v.grp_ids[g * v.cap + (k - gb[g])] = (uint16_t)k;
    }
    }
    if (TID < G) { v.grp_n[TID] = gb[TID + 1] - gb[TID]; v.grp_dead[TID] = 0; v.grp_reward[TID] = 0.0f; }
    if (TID == 0) { s.rid_off[e] += s.id_counter[e] - nb; s.id_counter[e] = nb; }
    __syncthreads();
}

// One training-loop step after get_observation (k_observe, per group) of env e by the whole
// workgroup: the rush policy + mean action, set_action, step, get_reward, clear_dead, and the
// episode restart from the reset image -- what agent_phase and the tail of k_rollout do, in HBM --
// then the next observation's shared inputs (obs_prep_env).  misc: 4 ints of LDS.
// The env's state between HBM (gv) and the LDS image (lv): to_lds (cnt: the LDS group counters) or back; idc:
// the env's id counter (the stepper keeps it in LDS), rid: the reference ids too.
__device__ __forceinline__ void big_env_copy(const State& s, int G, const EnvView& from, EnvView& to, int32_t* cnt,
                                             bool to_lds, int idc) {
    const int cap = s.cap;
    if ((s.cells_n & 7) == 0) {
        const uint4* src = reinterpret_cast<const uint4*>(from.cells);
        uint4* dst = reinterpret_cast<uint4*>(to.cells);
        for (int i = TID; i < (s.cells_n >> 3); i += blockDim.x) dst[i] = src[i];
    } else {
        for (int i = TID; i < s.cells_n; i += blockDim.x) to.cells[i] = from.cells[i];
    }
    for (int i = TID; i < idc; i += blockDim.x) {
        to.xy[i] = from.xy[i]; to.hp[i] = from.hp[i]; to.next_r[i] = from.next_r[i]; to.last_r[i] = from.last_r[i];
        to.op_obj[i] = from.op_obj[i]; to.last_act[i] = from.last_act[i]; to.meta[i] = from.meta[i];
        to.rid[i] = from.rid[i];
    }
    for (int g = 0; g < G; ++g)
        for (int i = TID; i < from.grp_n[g]; i += blockDim.x) to.grp_ids[g * cap + i] = from.grp_ids[g * cap + i];
    if (TID < G) {
        if (to_lds) { cnt[TID] = from.grp_n[TID]; cnt[4 + TID] = from.grp_dead[TID]; }
        else { to.grp_n[TID] = from.grp_n[TID]; to.grp_dead[TID] = from.grp_dead[TID]; }
        to.grp_reward[TID] = from.grp_reward[TID];
    }
}

// flags (few-env pipeline, RolloutArgs::few_pipe): kStepLoad -- stage the env into LDS first (lds_step);
// kStepStore -- write it back to HBM at the end; kStepPrep -- the next observation's shared inputs (obs_prep_env).
// The queue kernel's step passes all three; the pipelined stepper keeps the env in LDS between its steps.
constexpr int kStepLoad = 1, kStepStore = 2, kStepPrep = 4, kStepAll = 7;
// kExt: the actions come from ra.actions (a learned policy's forward wrote them) instead of the on-device rush
// policy, as in agent_phase: nothing is written to ra.actions, an id outside [0, 64) stays out of the mean action
// (set_action rejects it), and an episode end zeroes the env's mean-action rows (the next episode's first
// former_act_prob, k_rollout kMode 1).
template <bool kExt = false>
__device__ __forceinline__ void big_env_step(const GameParams& gp, const State& s, const RolloutArgs& ra, int e,
                                             uint32_t step_index, char* smem, int* misc, int flags = kStepAll) {
    // misc: 0 n_atk, 1 n_mov, 2 episode end
    const int G = gp.n_groups, cap = s.cap, acap = s.acap;
    const bool lds = ra.lds_step != 0;
    const BigLayout L = big_layout(gp, cap, acap, true, lds);
    StepSmem& sm = *reinterpret_cast<StepSmem*>(smem + L.sm);
    uint32_t* atk = lds ? reinterpret_cast<uint32_t*>(smem + L.atk) : s.atk + (size_t)e * acap;
    uint32_t* mov = lds ? reinterpret_cast<uint32_t*>(smem + L.mov) : s.mov + (size_t)e * acap;
    uint32_t* sorted = ra.big_sort + (size_t)e * acap;
    int* ahist = reinterpret_cast<int*>(smem + L.ahist);
    float* red = reinterpret_cast<float*>(smem + L.red);
    BigScratch bs = carve_big(smem + L.big, acap, cap, true, gp.large_map != 0);
#ifdef MFX_STAMPS
    bs.srow = ra.env_base + e;
#endif
    MFX_BSTAMP(bs.srow, 0);
    const EnvView gv = global_view(s, e, G);
    EnvView v = gv;
    load_serial_types(gp, sm);
    if (TID == 0) { misc[0] = 0; misc[1] = 0; }
    if (lds) {
        // few LDS-sized envs: the env's state comes into LDS for the step (one round trip of loads issued
        // together), every phase below then reads LDS instead of this XCD's L2, and the state goes back
        // at the end; the action buffers live in LDS.  The observation items read the written-back state.
        EnvView lv = carve_env(smem + L.img, s.cells_n, cap, G);
        int32_t* cnt = reinterpret_cast<int32_t*>(smem + L.cnt);
        lv.grp_n = cnt; lv.grp_dead = cnt + 4; lv.grp_reward = reinterpret_cast<float*>(cnt + 8);
        lv.rid = gv.rid; lv.food = gv.food;
        if (flags & kStepLoad) {
            const int idc = s.id_counter[e];
            if ((s.cells_n & 7) == 0) {
                const uint4* src = reinterpret_cast<const uint4*>(gv.cells);
                uint4* dst = reinterpret_cast<uint4*>(lv.cells);
                for (int i = TID; i < (s.cells_n >> 3); i += blockDim.x) dst[i] = src[i];
            } else {
                for (int i = TID; i < s.cells_n; i += blockDim.x) lv.cells[i] = gv.cells[i];
            }
            for (int i = TID; i < idc; i += blockDim.x) {
                lv.xy[i] = gv.xy[i]; lv.hp[i] = gv.hp[i]; lv.next_r[i] = gv.next_r[i]; lv.last_r[i] = gv.last_r[i];
                lv.op_obj[i] = gv.op_obj[i]; lv.last_act[i] = gv.last_act[i]; lv.meta[i] = gv.meta[i];
            }
            for (int g = 0; g < G; ++g)
                for (int i = TID; i < gv.grp_n[g]; i += blockDim.x) lv.grp_ids[g * cap + i] = gv.grp_ids[g * cap + i];
            if (TID < G) { cnt[TID] = gv.grp_n[TID]; cnt[4 + TID] = gv.grp_dead[TID]; lv.grp_reward[TID] = gv.grp_reward[TID]; }
            __syncthreads();
        }
        v = lv;
    }
    int ntot = 0;
    for (int g = 0; g < G; ++g) ntot += v.grp_n[g];
    // ---------------- policy + mean action (former_act_prob)
    // meta and positions of every id staged in LDS (the step scratch is free until the attacks): the
    // policy's and set_action's dependent lookups become LDS reads; the cells stay in HBM
    EnvView vp = v;                        // (big_region_bytes holds cap * (5 + 2 * kMaxGroups) bytes)
    if (!lds) {
        const int idc = s.id_counter[e];
        uint32_t* xy_l = reinterpret_cast<uint32_t*>(bs.base);
        uint8_t* meta_l = reinterpret_cast<uint8_t*>(bs.base + (size_t)cap * 4);
        for (int i = TID; i < idc; i += blockDim.x) { xy_l[i] = v.xy[i]; meta_l[i] = v.meta[i]; }
        vp.xy = xy_l; vp.meta = meta_l;
#ifndef MFX_BIG_NO_IDS_STAGE
        uint16_t* ids_l = reinterpret_cast<uint16_t*>(bs.base + (size_t)cap * 5);
        for (int g = 0; g < G; ++g)
            for (int i = TID; i < v.grp_n[g]; i += blockDim.x) ids_l[g * cap + i] = v.grp_ids[g * cap + i];
        vp.grp_ids = ids_l;
#endif
    }
    for (int i = TID; i < G * 64; i += blockDim.x) ahist[i] = 0;
    __syncthreads();
    if constexpr (kExt) {
        for (int t = TID; t < ntot; t += blockDim.x) {
            int g = 0, i = t;
            while (i >= v.grp_n[g]) { i -= v.grp_n[g]; ++g; }
            const int a = ra.actions[((size_t)e * G + g) * ra.rowcap + i];
            if ((unsigned)a < 64u) atomicAdd(&ahist[g * 64 + a], 1);
        }
    } else {
    const uint32_t ekey = ra.policy_seed ^ mix32(step_index * 0x9E3779B9u + (uint32_t)(ra.env_base + e) * 0x632BE5ABu);
    // two agents per lane per pass: both policies' HBM loads (position, 8 attack cells, their
    // occupants) are in flight together, the stores come after
    for (int t = TID; t < ntot; t += 2 * blockDim.x) {
        int a[2], gg[2], ii[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            int g = 0, i = t + j * (int)blockDim.x;
            a[j] = -1; gg[j] = 0; ii[j] = i;
            if (i >= ntot) continue;
            while (i >= v.grp_n[g]) { i -= v.grp_n[g]; ++g; }
            const int id = vp.grp_ids[g * cap + i];
            const uint32_t key = ekey ^ mix32((uint32_t)v.rid[id] * 0x85EBCA77u + (uint32_t)g);
            a[j] = rush_action(gp, sm.tt[g], vp, g, id, key, ra.eps);
            gg[j] = g; ii[j] = i;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (a[j] < 0) continue;
            ra.actions[((size_t)e * G + gg[j]) * ra.rowcap + ii[j]] = a[j];
            atomicAdd(&ahist[gg[j] * 64 + a[j]], 1);
        }
    }
    }
    __syncthreads();
    for (int t = TID; t < G * 64; t += blockDim.x) {
        const int g = t >> 6, k = t & 63, na = sm.tt[g].n_action, n = v.grp_n[g];
        if (k < na)   // empty group: np.mean of nothing is NaN
            ra.mean_act[((size_t)e * G + g) * ra.mean_stride + k] =
                n ? (double)ahist[t] / (double)n : __longlong_as_double(0x7FF8000000000000ll);
    }
    MFX_BSTAMP(bs.srow, 1);
    // ---------------- set_action (group order) and step
    for (int g = 0; g < G; ++g)            // vp: positions from LDS, last_act written to HBM
        set_action_group<false>(gp, s, vp, g, ra.actions + ((size_t)e * G + g) * ra.rowcap, atk, misc[0], mov, misc[1],
                                sm.wave_tot, acap);
    MFX_BSTAMP(bs.srow, 2);
    uint32_t rng = s.rng[e];
    int done = 0;
    step_env_core<false, false, true>(gp, s, v, atk, misc[0], mov, misc[1], sorted, rng, sm, done, false, ParScratch{},
                                      s.id_counter[e], nullptr, 0, &bs);
    MFX_BSTAMP(bs.srow, 10);
    // ---------------- get_reward, episode return, kills
    float kills = 0.0f, ret[kMaxGroups];
    for (int g = 0; g < G; ++g) {
        const int n = v.grp_n[g];
        float part = 0.0f;
        for (int i = TID; i < n; i += blockDim.x) {
            const float r = v.next_r[v.grp_ids[g * cap + i]] + v.grp_reward[g];
            ra.rewards[((size_t)e * G + g) * ra.rowcap + i] = r;
            if constexpr (kExt) {              // get_agent_id / get_alive before clear_dead (the replay collector)
                if (i < ra.rowcap) {
                    const int id = v.grp_ids[g * cap + i];
                    ra.ids[((size_t)e * G + g) * ra.rowcap + i] = (int32_t)v.rid[id];
                    ra.alive[((size_t)e * G + g) * ra.rowcap + i] = (uint8_t)!meta_dead(v.meta[id]);
                }
            }
            part += r;
        }
        ret[g] = block_sum_waves(part, red);
        kills += (float)v.grp_dead[g];
    }
    MFX_BSTAMP(bs.srow, 11);
    // ---------------- clear_dead
    if (ra.renumber) clear_dead_renumber(gp, s, v, e, reinterpret_cast<uint4*>(bs.base), sm.wave_tot, ra.renumber == 2);
    else clear_dead_env<false>(gp, v, sm.wave_tot);
    MFX_BSTAMP(bs.srow, 12);
    // ---------------- episode end -> reset image (env.reset + add_agents of the template)
    if (TID == 0) {
        double* st = ra.stats + (size_t)e * 4;
        st[3] += kills;
        float* er = ra.ep_return + (size_t)e * G;
        for (int g = 0; g < G; ++g) er[g] += ret[g];
        int len = ra.ep_len[e] + 1;
        misc[2] = 0;
        if (done || len >= ra.max_steps) {
            st[0] += 1.0;
            st[1] += er[0];
            st[2] += G > 1 ? er[1] : 0.0f;
            for (int g = 0; g < G; ++g) er[g] = 0.0f;
            len = 0;
            misc[2] = 1;
        }
        ra.ep_len[e] = len;
        ra.agent_steps[e] += (unsigned long long)ntot;
        s.rng[e] = rng;
        s.n_atk[e] = 0;
        s.n_mov[e] = 0;
        s.done[e] = done;
    }
    __syncthreads();
    if (misc[2]) {
        const EnvView im = carve_env(reinterpret_cast<char*>(const_cast<uint4*>(ra.reset_image)), s.cells_n, cap, G);
        const int32_t* img_scal = reinterpret_cast<const int32_t*>(
            reinterpret_cast<const char*>(ra.reset_image) + env_image_bytes(s.cells_n, cap, G));
        const int idc = img_scal[4];
        for (int i = TID; i < s.cells_n; i += blockDim.x) v.cells[i] = im.cells[i];
        for (int i = TID; i < idc; i += blockDim.x) {
            v.xy[i] = im.xy[i]; v.hp[i] = im.hp[i]; v.next_r[i] = im.next_r[i]; v.last_r[i] = im.last_r[i];
            v.op_obj[i] = im.op_obj[i]; v.last_act[i] = im.last_act[i]; v.meta[i] = im.meta[i];
            v.rid[i] = (uint16_t)i;                  // a fresh episode: slot == id
        }
        for (int g = 0; g < G; ++g)
            for (int i = TID; i < img_scal[g]; i += blockDim.x) v.grp_ids[g * cap + i] = im.grp_ids[g * cap + i];
        if (TID < G) { v.grp_n[TID] = img_scal[TID]; v.grp_dead[TID] = 0; v.grp_reward[TID] = 0.0f; }
        if (TID == 0) { s.id_counter[e] = idc; s.rid_off[e] = 0; }
        if constexpr (kExt)
            for (int t = TID; t < G * ra.mean_stride; t += blockDim.x)
                ra.mean_act[(size_t)e * G * ra.mean_stride + t] = 0.0;
        __syncthreads();
    }
    MFX_BSTAMP(bs.srow, 13);
    if (lds && (flags & kStepStore)) {     // the state back to HBM (the caller drains the stores)
        const int idc = s.id_counter[e];
        if ((s.cells_n & 7) == 0) {
            const uint4* src = reinterpret_cast<const uint4*>(v.cells);
            uint4* dst = reinterpret_cast<uint4*>(gv.cells);
            for (int i = TID; i < (s.cells_n >> 3); i += blockDim.x) dst[i] = src[i];
        } else {
            for (int i = TID; i < s.cells_n; i += blockDim.x) gv.cells[i] = v.cells[i];
        }
        for (int i = TID; i < idc; i += blockDim.x) {
            gv.xy[i] = v.xy[i]; gv.hp[i] = v.hp[i]; gv.next_r[i] = v.next_r[i]; gv.last_r[i] = v.last_r[i];
            gv.op_obj[i] = v.op_obj[i]; gv.last_act[i] = v.last_act[i]; gv.meta[i] = v.meta[i];
        }
        for (int g = 0; g < G; ++g)
            for (int i = TID; i < v.grp_n[g]; i += blockDim.x) gv.grp_ids[g * cap + i] = v.grp_ids[g * cap + i];
        if (TID < G) { gv.grp_n[TID] = v.grp_n[TID]; gv.grp_dead[TID] = v.grp_dead[TID]; gv.grp_reward[TID] = v.grp_reward[TID]; }
    }
    // ---------------- the next observation's shared inputs
    if (ra.obs_mm && (flags & kStepPrep)) {
        constexpr int NV = BattleShape::VW * BattleShape::VH;
        obs_prep_env(gp, v, ra.obs_mm + (size_t)e * G * NV, ra.obs_info + (size_t)e * cap,
                     reinterpret_cast<int*>(smem + L.big));
    }
    MFX_BSTAMP(bs.srow, 14);
}

// The queue kernel's step as a real call (MFX_BIGQ_CALL, A/B only): the step's register peak is then
// not added to the values the item loop keeps live, but its 436 B of stack per lane cost more than the
// inlined form's few spills (256x256 bench 8.6e8 vs 9.6e8 agent-steps/s, same box).
__device__ __attribute__((noinline)) void big_env_step_call(const GameParams& gp, const State& s,
                                                            const RolloutArgs& ra, int e, uint32_t step_index,
                                                            char* smem, int* misc) {
    big_env_step(gp, s, ra, e, step_index, smem, misc);
}

// kExt: a learned policy's step (big_env_step<true>: the actions are read from ra.actions).
template <bool kExt>
__global__ void __launch_bounds__(kBigRolloutThreads) k_rollout_big(const GameParams* __restrict__ gpp,
                                                             const RolloutCtx* __restrict__ ctx, uint32_t step_index) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int misc[4];
    const RolloutArgs& ra = ctx->ra;
    const int e = blockIdx.x;
    big_env_step<kExt>(*gpp, ctx->s, ra, e, step_index, smem, misc);
    if (ra.obs_mm && ra.obs_items) {
        __syncthreads();
        obs_file_items(ra, global_view(ctx->s, e, gpp->n_groups), gpp->n_groups, e, (int)((step_index + 1) & 1));
    }
}

// ==================================================================================
//  large envs, one launch for n_sub steps of every env: k_rollout_bigq
// ==================================================================================
// Persistent 512-lane workgroups take observation items (64 agents of one group of one env) from
// per-XCD queues; the workgroup that finishes the LAST item of env e's step runs that step
// (big_env_step) at once and files env e's items of its next step -- into the same queues while the
// launch has steps left for e, else into the other parity's queues, which the next launch drains.
// One kernel keeps the whole chip on the observation write stream while the latency-bound steps
// run in between (the two-stream pipeline above gives a third of the chip to each item launch).
//
// Env e lives on ONE XCD: its items go to list e % 8 and a workgroup takes items only from the list of
// the XCD it runs on (HW_REG_XCC_ID), so the last finisher that steps env e is on that XCD too.  This
// is what keeps the observation rows right: steps t and t + 1 of env e write the same view rows from
// different workgroups, and two XCDs' L2s holding dirty copies of one line would write back in either
// order; through one L2 the later store wins (each item's waves drain their stores before its q_left
// decrement, which the next step's items causally follow).  The host takes this path only with all 8
// XCDs in one device (SPX), where a full-occupancy grid puts 64 workgroups on each.
// Hand-offs inside the launch (MI355X_MICROARCH.md, inter-workgroup visibility): the stepper's
// writes of env e (state, minimap, info words, q_si) -> every wave drains its stores, workgroup
// barrier (the stores are in this XCD's L2, which every consumer of the env reads through: no L2
// write-back), then the item words (agent-scope atomic stores, tagged with the consuming launch).
// A consumer polls its item word relaxed, then one agent-scope acquire (L1 invalidate) before any
// plain load of the env.  The item counters and
// q_left and the per-XCD done counts (xcd_done) are agent-scope atomics.
// Item word: tag << 26 | (filed step & 63) << 20 | env << 7 | group << 6 | chunk.  The tag tells this
// launch's filings from the next launch's; the step bits are the in-kernel guard of the hand-off: a
// consumer reads the env's step counter q_si[e] with a plain load after its acquire, like the rest of
// the env's state, and a counter that is not the step the item was filed for (the stepper's stores not
// visible) sets error word 5 (mfx_battle_rollout_check).
// Error words (q_done[2]): 2 a wait without progress, 3 a ticket past the list, 4 a workgroup whose XCC
// id is not 0-7 (not one SPX device of 8 XCDs), 5 the guard above.
constexpr uint32_t kQEnvBits = 13, kQTagShift = 26, kQTagMask = 0x3Fu, kQStepShift = 20, kQStepMask = 63u;
constexpr int kQErrStall = 2, kQErrList = 3, kQErrXcc = 4, kQErrGuard = 5;
#ifndef MFX_BIGQ_PF
#define MFX_BIGQ_PF kObsPf
#endif
constexpr int kQPf = MFX_BIGQ_PF;                 // 64-cell blocks in flight per wave in the item stream
// Every wait of the queue kernels is bounded in wall-clock time: after kQStallTicks of the 100 MHz s_memrealtime
// clock (10 s) without the awaited progress the wait gives up and sets error word 2 (kQErrStall), which rollout_check /
// every parity test / the bench's self-check report.  Work of other processes on the device (or a profiler's) can thus
// delay a launch by up to 10 s per wait; a longer foreign occupation of an XCD is reported as a stall, not waited out
// (a watchdog against a hang of the device, not a limit the product's own launches come near: their waits last
// microseconds).
constexpr unsigned long long kQStallTicks = 10ull * 100000000ull;
__device__ __forceinline__ bool q_stalled(unsigned long long t0, uint32_t spins) {
    return (spins & 63u) == 63u && __builtin_amdgcn_s_memrealtime() - t0 > kQStallTicks;
}

__device__ __forceinline__ int qld(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t qldu(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int xcc_id() {        // HW_REG_XCC_ID (id 20), bits [3:0]: 0-7 in SPX mode
    return (int)(__builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 15u);
}

// Lane 0: file env e's items of step si (one per obs_item_rows agents of each group; one empty item when
// every group is empty, so the step still runs) into queue (par, e % kXcds) with tag; q_left[e] first.
// rec (optional): the pipelined stepper's record of its filing -- the first slot, the count and the words (few_steal
// races the holders for them).  At most 2 x 64 items (the host takes this path with <= 64 chunks per group).
struct FewFiled { int first, count; uint32_t words[2 * 64]; unsigned long long steal[2]; };
__device__ __forceinline__ void bigq_file(const RolloutArgs& ra, const int32_t* grp_n, int G, int e, int par,
                                          uint32_t tag, uint32_t si, FewFiled* rec = nullptr) {
    const int R = ra.obs_item_rows;
    int n[kMaxGroups], k = 0;
    for (int g = 0; g < G; ++g) { n[g] = qld(grp_n + g); k += (n[g] + R - 1) / R; }
    const int kk = k ? k : 1;
    __hip_atomic_store(ra.q_left + e, kk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int l = e % kXcds;
    int32_t* c = ra.q_cnt + (par * kXcds + l) * kObsCntPad;
    const int base = __hip_atomic_fetch_add(c, kk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (rec) { rec->first = base; rec->count = kk; }
    uint32_t* out = ra.q_items + ((size_t)par * kXcds + l) * ra.q_list_cap + base;
    const uint32_t head = (tag << kQTagShift) | ((si & kQStepMask) << kQStepShift) | ((uint32_t)e << 7);
    if (!k) {
        __hip_atomic_store(out, head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (rec) rec->words[0] = head;
        return;
    }
    for (int g = 0, j = 0; g < G; ++g)
        for (int ch = 0; ch * R < n[g]; ++ch, ++j) {
            const uint32_t w = head | ((uint32_t)g << 6) | (uint32_t)ch;
            __hip_atomic_store(out + j, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (rec) rec->words[j] = w;
        }
}

// Lane 0: a ticket of queue parity par in this XCD's own list (no help across XCDs: see
// k_rollout_bigq), then the item filed into its slot, or -1 when every env has done its steps of this
// launch on this XCD (xcd_done reached its target) or on a stuck queue (error word).  One fetch-add takes the next slot,
// filed or not yet filed (then the workgroup waits for the filer's word); a compare-and-swap pop
// serialised the 64 workgroups of an XCD on one counter (5x slower).  Slots past the last filing of
// the launch are never filled: their holders leave when their XCD's count reaches the target.
// The launch's count of env-steps done on XCD x -- a word of the other parity's counters, which the host zeroes
// before every launch -- and its target, n_sub steps of every env e = x (mod 8).  A workgroup leaves when its XCD's
// count is reached: a launch holds an XCD only while it has work there, and that work needs only the launch's
// workgroups on that XCD (env e lives on XCD e % 8), so no set of these launches can starve each other.
__device__ __forceinline__ int32_t* xcd_done(const RolloutArgs& ra, int par, int x) {
    return ra.q_cnt + ((par ^ 1) * kXcds + x) * kObsCntPad + 2;
}
__device__ __forceinline__ int32_t xcd_target(int E, int x, int n_sub) {
    return x < E ? ((E - 1 - x) / kXcds + 1) * n_sub : 0;
}

__device__ __forceinline__ int bigq_ticket(const RolloutArgs& ra, int par, int x) {
    return __hip_atomic_fetch_add(ra.q_cnt + (par * kXcds + x) * kObsCntPad + 1, 1, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
}

// bigq_wait's answers besides an item word: the launch is over (or an error word is set), the slot's item was
// taken by its env's stepper (few_steal), this workgroup claimed a stepper role (kPipe: the env in *claim).
constexpr int kQOver = -1, kQSkip = -2, kQClaim = -3;
// The pipelined form's mark of an item its stepper observed itself (few_steal): env field 8191 (never an env of
// that path: at most a quarter of the grid's workgroups) and chunk 63, under the launch's tag.
constexpr uint32_t kQStolen = (((1u << kQEnvBits) - 1u) << 7) | 63u;

// kPipe (the pipelined few-env form): forward progress needs no co-residency beyond one workgroup of the launch
// per XCD.  A stepper role nobody has claimed yet (its workgroup not resident) is claimed here by a waiting
// worker, which keeps its ticket for after the env's steps; an item can have been taken by its own env's stepper
// (few_steal), which leaves the stolen mark: holder and stepper race for the word with a compare-and-swap.
template <bool kPipe>
__device__ int bigq_wait(const RolloutArgs& ra, int par, int x, int t, uint32_t tag, int32_t xtarget, int E,
                         int* claim) {
    uint32_t* w = ra.q_items + ((size_t)par * kXcds + x) * ra.q_list_cap + t;
    if ((size_t)t >= ra.q_list_cap) {
        __hip_atomic_store(ra.q_done + 2, kQErrList, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return kQOver;
    }
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (uint32_t spins = 0; !q_stalled(t0, spins); ++spins) {
        uint32_t v = qldu(w);
        if ((v >> kQTagShift) == tag) {                  // consumed: the slot reads 0 until refiled
            if (kPipe) {
                const uint32_t mark = (tag << kQTagShift) | kQStolen;
                if (v != mark && __hip_atomic_compare_exchange_strong(w, &v, 0u, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                                      __HIP_MEMORY_SCOPE_AGENT))
                    return (int)(v & ((1u << kQTagShift) - 1));
                __hip_atomic_store(w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the stepper took it
                return kQSkip;
            }
            __hip_atomic_store(w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return (int)(v & ((1u << kQTagShift) - 1));
        }
        if (qld(xcd_done(ra, par, x)) >= xtarget) return kQOver;
        if (kPipe && (spins & 15) == 15 && x + kXcds * qld(ra.q_step + x) < E) {
            const int c = __hip_atomic_fetch_add(ra.q_step + x, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (x + kXcds * c < E) { *claim = x + kXcds * c; return kQClaim; }
        }
        __builtin_amdgcn_s_sleep(2);
    }
    __hip_atomic_store(ra.q_done + 2, kQErrStall, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return kQOver;
}

// Seed the queues of parity par (the caller zeroed their counters): obs_prep_env of every env, its
// step counter and its items for the first launch.
__global__ void __launch_bounds__(256) k_bigq_seed(const GameParams* __restrict__ gp, State s, RolloutArgs ra, int par,
                                                   uint32_t tag, uint32_t step_index) {
    __shared__ int hist[BattleShape::G * BattleShape::VW * BattleShape::VH];
    constexpr int NV = BattleShape::VW * BattleShape::VH;
    const int e = blockIdx.x;
    const EnvView v = global_view(s, e, gp->n_groups);
    obs_prep_env(*gp, v, ra.obs_mm + (size_t)e * BattleShape::G * NV, ra.obs_info + (size_t)e * s.cap, hist);
    if (TID == 0) {
        ra.q_si[e] = step_index;
        bigq_file(ra, v.grp_n, gp->n_groups, e, par, tag, step_index);
    }
}

// ---------------- few envs, pipelined (RolloutArgs::few_pipe; k_rollout_bigq<true>)
// One workgroup per env is its STEPPER for the whole launch: it stages the env in LDS once, and per step writes
// a snapshot of what the observation reads (cells, group counts and lists, positions, ids, last actions and
// rewards, the minimap and the packed hp / group words) into the env's snapshot of that step's parity, files the
// step's observation items (once the previous step's items are all done: they write the same view rows), and
// steps at once -- the rush policy reads the LDS state, not the views -- while the other workgroups of its XCD
// observe the snapshot.  The state goes back to HBM after the launch's last step.  A step then costs the stepper's
// own phases plus the snapshot, not the observation on top (the queue kernel runs a step only after its items).
// The stepper of env e runs on XCD e % 8 like every item of env e (claimed per XCD, q_step), so the snapshot
// reaches the items through one L2 (the argument of k_rollout_bigq's hand-off below).
struct SnapLayout { size_t cells, grp_n, grp_ids, xy, rid, last_act, last_r, info, mm, total; };
__host__ __device__ inline SnapLayout snap_layout(int cells_n, int cap, int G) {
    auto r16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    SnapLayout L;
    size_t o = 0;
    L.cells = o;    o += r16((size_t)cells_n * 2);
    L.grp_n = o;    o += 16;
    L.grp_ids = o;  o += r16((size_t)G * cap * 2);
    L.xy = o;       o += r16((size_t)cap * 4);
    L.rid = o;      o += r16((size_t)cap * 2);
    L.last_act = o; o += r16((size_t)cap);
    L.last_r = o;   o += r16((size_t)cap * 4);
    L.info = o;     o += r16((size_t)cap * 4);
    L.mm = o;       o += r16((size_t)G * BattleShape::VW * BattleShape::VH * 4);
    L.total = o;
    return L;
}

// The snapshot of env e, parity p, as an EnvView (the fields the observation reads) + its info / minimap.
__device__ __forceinline__ EnvView snap_view(const State& s, const RolloutArgs& ra, int e, int p, int G,
                                            uint32_t** info, float** mm) {
    const SnapLayout L = snap_layout(s.cells_n, s.cap, G);
    char* b = reinterpret_cast<char*>(ra.few_snap) + ((size_t)e * 2 + (size_t)p) * ra.few_snap_bytes;
    EnvView v{};
    v.cap = s.cap;
    v.cells = reinterpret_cast<uint16_t*>(b + L.cells);
    v.grp_n = reinterpret_cast<int32_t*>(b + L.grp_n);
    v.grp_ids = reinterpret_cast<uint16_t*>(b + L.grp_ids);
    v.xy = reinterpret_cast<uint32_t*>(b + L.xy);
    v.rid = reinterpret_cast<uint16_t*>(b + L.rid);
    v.last_act = reinterpret_cast<uint8_t*>(b + L.last_act);
    v.last_r = reinterpret_cast<float*>(b + L.last_r);
    *info = reinterpret_cast<uint32_t*>(b + L.info);
    *mm = reinterpret_cast<float*>(b + L.mm);
    return v;
}

// The stepper's LDS env view (the lds layout of big_layout; its contents persist between the steps of a launch).
// The reference ids are in LDS too: the few-env path never renumbers (RolloutArgs::renumber 0), so they only
// change at an episode restart.
__device__ __forceinline__ EnvView few_lds_view(const GameParams& gp, const State& s, char* smem, int e) {
    const BigLayout L = big_layout(gp, s.cap, s.acap, true, true);
    EnvView lv = carve_env(smem + L.img, s.cells_n, s.cap, gp.n_groups);
    int32_t* cnt = reinterpret_cast<int32_t*>(smem + L.cnt);
    lv.grp_n = cnt; lv.grp_dead = cnt + 4; lv.grp_reward = reinterpret_cast<float*>(cnt + 8);
    lv.rid = reinterpret_cast<uint16_t*>(smem + L.rid);
    lv.food = s.food ? s.food + (size_t)e * s.cells_n : nullptr;
    return lv;
}

// The snapshot of the stepper's LDS state into parity p: what the observation reads (cells, group lists and
// counts, positions, reference ids, last actions and rewards) and the packed hp / group info words, from lanes
// TID >= store0 (64: wave 0 leaves at once for the step); the minimap counts go into the LDS histogram (L.hist, all
// zero between snapshots) and fcnt (LDS) keeps the group counts the items are filed for.  No load from HBM.  Ends
// with the barrier after which the state may change; the minimap itself (few_minimap) reads only the histogram and
// fcnt, so it can follow while wave 0 steps.
// The views, the snapshot's pointers and the per-group constants come precomputed for the launch (FewSnapCtx):
// rebuilt per step from the kernel arguments they cost ~4K cycles of dependent scalar loads before the first copy.
// Every array goes out in 16-B units through one flat loop over its segments (the LDS image and the snapshot pad
// each array to 16 B, so a rounded-up tail stays inside both), and the minimap counts take both groups in one pass.
// An LDS pointer that went through memory (the per-launch contexts below hold generic pointers) rebuilt on the
// dynamic LDS base: without it the compiler cannot tell the pointee is LDS and every access through it is a FLAT
// instruction -- a longer round trip that also waits (vmcnt) for the wave's outstanding HBM stores.  The 32-bit
// offset keeps the rebuild from folding back into the loaded pointer.
template <class T>
__device__ __forceinline__ T* lds_rebase(T* p, char* smem) {
    const uint32_t off = (uint32_t)(reinterpret_cast<uintptr_t>(p) - reinterpret_cast<uintptr_t>(smem));
    return reinterpret_cast<T*>(smem + off);
}
__device__ __forceinline__ void lds_rebase_view(EnvView& v, char* smem) {   // (food stays in HBM)
    v.cells = lds_rebase(v.cells, smem); v.xy = lds_rebase(v.xy, smem); v.hp = lds_rebase(v.hp, smem);
    v.next_r = lds_rebase(v.next_r, smem); v.last_r = lds_rebase(v.last_r, smem);
    v.last_act = lds_rebase(v.last_act, smem); v.op_obj = lds_rebase(v.op_obj, smem);
    v.meta = lds_rebase(v.meta, smem); v.grp_ids = lds_rebase(v.grp_ids, smem);
    v.grp_n = lds_rebase(v.grp_n, smem); v.grp_dead = lds_rebase(v.grp_dead, smem);
    v.grp_reward = lds_rebase(v.grp_reward, smem); v.rid = lds_rebase(v.rid, smem);
}

struct FewSnapArrays { uint16_t* cells; uint32_t* xy; uint16_t* rid; uint8_t* last_act; float* last_r; uint16_t* grp_ids;
                       int32_t* grp_n; };
struct FewSnapCtx {                  // (one copy in LDS per stepper, made once per launch)
    FewSnapArrays lv;                // the stepper's LDS env
    const float* hp;                 //   and its hp
    FewSnapArrays sv[2];             // the snapshot of each parity
    uint32_t* info[2];
    float* mm[2];
    int* hist;
    int cells_n, cap, sw, sh;
    float hp_max[kMaxGroups];
};
__device__ __forceinline__ FewSnapArrays few_snap_arrays(const EnvView& v) {
    return FewSnapArrays{v.cells, v.xy, v.rid, v.last_act, v.last_r, v.grp_ids, v.grp_n};
}
// Lane 0 only (the caller's barrier publishes it).
__device__ __forceinline__ void few_snap_ctx(const GameParams& gp, const State& s, const RolloutArgs& ra, char* smem,
                                             int e, FewSnapCtx& c) {
    const int G = gp.n_groups;
    const EnvView lv = few_lds_view(gp, s, smem, e);
    c.lv = few_snap_arrays(lv);
    c.hp = lv.hp;
    for (int p = 0; p < 2; ++p) c.sv[p] = few_snap_arrays(snap_view(s, ra, e, p, G, &c.info[p], &c.mm[p]));
    const BigLayout L = big_layout(gp, s.cap, s.acap, true, true);
    c.hist = reinterpret_cast<int*>(smem + L.hist);
    c.cells_n = s.cells_n;
    c.cap = s.cap;
    c.sw = (gp.W + BattleShape::VW - 1) / BattleShape::VW;
    c.sh = (gp.H + BattleShape::VH - 1) / BattleShape::VH;
    for (int g = 0; g < kMaxGroups; ++g) c.hp_max[g] = g < G ? gp.type[g].hp : 1.0f;
}
__device__ __forceinline__ void few_snapshot(const FewSnapCtx& c, char* smem, int p, int idc, int store0,
                                             int32_t* fcnt, int srow = -1) {
    static_assert(BattleShape::G == 2, "the segment table below");
    constexpr int VW = BattleShape::VW, NV = VW * BattleShape::VH, G = BattleShape::G;
    (void)srow;
#ifdef MFX_STAMPS
    // stamps build: the first copying lane's clock at its sub-phases (slots 24-27; no barrier of their own)
#define MFX_SNAP_STAMP(i)                                                                                        \
    do {                                                                                                         \
        if ((int)TID == store0 && g_stamps && srow >= 0) g_stamps[srow * kStampW + (i)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#else
#define MFX_SNAP_STAMP(i) do {} while (0)
#endif
    FewSnapArrays lv = c.lv;
    lv.cells = lds_rebase(lv.cells, smem); lv.xy = lds_rebase(lv.xy, smem); lv.rid = lds_rebase(lv.rid, smem);
    lv.last_act = lds_rebase(lv.last_act, smem); lv.last_r = lds_rebase(lv.last_r, smem);
    lv.grp_ids = lds_rebase(lv.grp_ids, smem); lv.grp_n = lds_rebase(lv.grp_n, smem);
    const float* hp = lds_rebase(c.hp, smem);
    int* hist = lds_rebase(c.hist, smem);
    const FewSnapArrays sv = c.sv[p];
    const int cap = c.cap;
    const int t0 = (int)TID - store0, T = (int)blockDim.x - store0;
    const int n0 = lv.grp_n[0], n1 = lv.grp_n[1];
    if (TID < G) fcnt[TID] = lv.grp_n[TID];
    if (t0 >= 0) {
        MFX_SNAP_STAMP(24);
        // segments in 16-B units: cells, xy, rid, last_act, last_r, the two group lists
        const int u0 = (c.cells_n * 2 + 15) >> 4, u1 = (idc * 4 + 15) >> 4, u2 = (idc * 2 + 15) >> 4, u3 = (idc + 15) >> 4;
        const int u5 = (n0 * 2 + 15) >> 4, u6 = (n1 * 2 + 15) >> 4;
        const int e0 = u0, e1 = e0 + u1, e2 = e1 + u2, e3 = e2 + u3, e4 = e3 + u1, e5 = e4 + u5, e6 = e5 + u6;
        for (int i = t0; i < e6; i += T) {
            const uint4* src;
            uint4* dst;
            int k;
            if (i < e0) { k = i; src = reinterpret_cast<const uint4*>(lv.cells); dst = reinterpret_cast<uint4*>(sv.cells); }
            else if (i < e1) { k = i - e0; src = reinterpret_cast<const uint4*>(lv.xy); dst = reinterpret_cast<uint4*>(sv.xy); }
            else if (i < e2) { k = i - e1; src = reinterpret_cast<const uint4*>(lv.rid); dst = reinterpret_cast<uint4*>(sv.rid); }
            else if (i < e3) { k = i - e2; src = reinterpret_cast<const uint4*>(lv.last_act); dst = reinterpret_cast<uint4*>(sv.last_act); }
            else if (i < e4) { k = i - e3; src = reinterpret_cast<const uint4*>(lv.last_r); dst = reinterpret_cast<uint4*>(sv.last_r); }
            else if (i < e5) { k = i - e4; src = reinterpret_cast<const uint4*>(lv.grp_ids); dst = reinterpret_cast<uint4*>(sv.grp_ids); }
            else { k = i - e5; src = reinterpret_cast<const uint4*>(lv.grp_ids + cap); dst = reinterpret_cast<uint4*>(sv.grp_ids + cap); }
            dst[k] = src[k];
        }
        if (t0 < G) sv.grp_n[t0] = lv.grp_n[t0];
        MFX_SNAP_STAMP(25);
        MFX_SNAP_STAMP(26);
        // the minimap counts and the packed hp / group words (obs_prep_env's), both groups in one pass
        uint32_t* info = c.info[p];
        for (int i = t0; i < n0 + n1; i += T) {
            const int j = i < n0 ? 0 : 1;
            const int id = lv.grp_ids[j * cap + (i - (j ? n0 : 0))];
            const uint32_t q = lv.xy[id];
            atomicAdd(&hist[j * NV + ((int)(q >> 16) / c.sh) * VW + (int)(q & 0xFFFF) / c.sw], 1);
            info[id] = __float_as_uint(hp[id] / (j ? c.hp_max[1] : c.hp_max[0])) | ((uint32_t)j << 31);
        }
        MFX_SNAP_STAMP(27);
    }
    __syncthreads();
#undef MFX_SNAP_STAMP
}

// The snapshot's minimap density from the histogram and fcnt (obs_prep_env's), by lanes t0 = TID - store0 >= 0 of
// the waves that made it, after few_snapshot's barrier and after every one of them has passed it; the histogram
// goes back to zero.
__device__ __forceinline__ void few_minimap(const FewSnapCtx& c, char* smem, int p, int t0, int T, const int32_t* fcnt) {
    constexpr int NV = BattleShape::VW * BattleShape::VH, G = BattleShape::G;
    float* mm = c.mm[p];
    int* hist = lds_rebase(c.hist, smem);
    for (int i = t0; i < G * NV; i += T) {
        const int n = fcnt[i / NV];
        mm[i] = n ? (float)hist[i] / (float)n : __uint_as_float(0xFFC00000u);
        hist[i] = 0;
    }
}

// One step of the stepper's env, all of it in LDS: k_rollout's agent phase (agent_phase: the rush policy and
// mean action, set_action, GridWorld::step in the team forms, get_reward, clear_dead) by wave 0 alone (kW, up to
// RolloutArgs::few_wave_max agents) or the workgroup, then (few_env_end, whole workgroup) the episode end and
// restart.  The per-env scalars (id counter, minstd state, episode length / return, statistics, agent-steps) stay
// in sc for the whole launch, so the step issues no load from HBM (the reset image aside); the actions, mean
// action and rewards are stored as every step does.  rng / done / kills: lane 0's.
// The step's views and scratch carvings, like FewSnapCtx made once per launch (lane 0; the caller's barrier
// publishes it): rebuilt per step from the kernel arguments they were a chain of dependent scalar loads at the head of
// the policy phase and of the episode end.
struct FewStepCtx {
    EnvView v;
    ParScratch ps;
    BigScratch bs;
    StepSmem* sm;
    uint32_t* atk;
    uint32_t* mov;
    uint32_t* sorted;
    int* ahist;
    int32_t* act;
};
__device__ __forceinline__ void few_step_ctx(const GameParams& gp, const State& s, const RolloutArgs& ra, char* smem,
                                             int e, FewStepCtx& c) {
    const int cap = s.cap, acap = s.acap;
    const BigLayout L = big_layout(gp, cap, acap, true, true);
    c.v = few_lds_view(gp, s, smem, e);
    c.ps = carve_par(smem + L.big, acap, cap);
    c.bs = carve_big(smem + L.big, acap, cap, false);
    c.sm = reinterpret_cast<StepSmem*>(smem + L.sm);
    c.atk = reinterpret_cast<uint32_t*>(smem + L.atk);
    c.mov = reinterpret_cast<uint32_t*>(smem + L.mov);
    c.sorted = ra.big_sort + (size_t)e * acap;          // (large maps only)
    c.ahist = reinterpret_cast<int*>(smem + L.ahist);
    c.act = reinterpret_cast<int32_t*>(smem + L.act);
}

template <bool kW, class Mid = NoMid>
__device__ __forceinline__ void few_agents(const GameParams& gp, const State& s, const RolloutArgs& ra, int e, uint32_t si,
                                           const FewStepCtx& fc, char* smem, int* misc, EnvScalars& sc,
                                           int stamp_row, uint32_t& rng, int& done, float& kills,
                                           const Mid& mid = Mid()) {
#ifdef MFX_STAMPS
    if (kW && TID == 0 && g_stamps) g_stamps[stamp_row * kStampW + 9] = __builtin_amdgcn_s_memtime();
#endif
    EnvView v = fc.v;
    lds_rebase_view(v, smem);
    ParScratch ps = fc.ps;
    ps.ord = lds_rebase(ps.ord, smem); ps.jv = lds_rebase(ps.jv, smem); ps.att = lds_rebase(ps.att, smem);
    ps.tgt = lds_rebase(ps.tgt, smem); ps.eff = lds_rebase(ps.eff, smem); ps.dmg = lds_rebase(ps.dmg, smem);
    ps.death = lds_rebase(ps.death, smem); ps.death_new = lds_rebase(ps.death_new, smem);
    ps.owner = lds_rebase(ps.owner, smem); ps.flag = lds_rebase(ps.flag, smem);
    BigScratch bs = fc.bs;
    bs.ord = lds_rebase(bs.ord, smem); bs.jv = lds_rebase(bs.jv, smem); bs.hd = lds_rebase(bs.hd, smem);
    bs.lst = lds_rebase(bs.lst, smem); bs.att = lds_rebase(bs.att, smem); bs.tgt = lds_rebase(bs.tgt, smem);
    bs.pg = lds_rebase(bs.pg, smem); bs.death = lds_rebase(bs.death, smem); bs.owner = lds_rebase(bs.owner, smem);
    bs.flag = lds_rebase(bs.flag, smem); bs.base = lds_rebase(bs.base, smem);
#ifdef MFX_STAMPS
    if (!kW) { bs.srow = stamp_row; bs.sbase = -3; }       // the team attack's internals in slots 0-3 (free here)
#endif
    StepSmem* sm = lds_rebase(fc.sm, smem);
    int32_t* act = lds_rebase(fc.act, smem);
    float* red = reinterpret_cast<float*>(act);            // the reward sums run after set_action
    (void)stamp_row;
    if (TID == 0) { misc[0] = 0; misc[1] = 0; }
    psync<kW>();
#ifdef MFX_STAMPS
    if (kW && TID == 0 && g_stamps) g_stamps[stamp_row * kStampW + 10] = __builtin_amdgcn_s_memtime();
#endif
    rng = sc.rng;
    done = 0;
    kills = 0.0f;
    agent_phase<true, kW, false, Mid>(gp, s, ra, v, sc, misc, *sm, act, lds_rebase(fc.ahist, smem),
                                      lds_rebase(fc.atk, smem), lds_rebase(fc.mov, smem), fc.sorted, red, ps, &bs, e,
                                      si, stamp_row, rng, done, kills, ra.env_base + e, mid);
}

// Whole workgroup, after few_agents: the episode end -> reset image (env.reset + add_agents of the template).
// ntot: the agents before the step.
__device__ __forceinline__ void few_env_end(const GameParams& gp, const State& s, const RolloutArgs& ra, int e,
                                            const FewStepCtx& fc, char* smem, int* misc, EnvScalars& sc,
                                            int stamp_row, int ntot, uint32_t rng, int done, float kills) {
    const int G = gp.n_groups, cap = s.cap;
    EnvView v = fc.v;
    lds_rebase_view(v, smem);
    (void)stamp_row;
    if (TID == 0) {
        sc.stats[3] += kills;
        int len = sc.ep_len + 1;
        misc[2] = 0;
        if (done || len >= ra.max_steps) {
            sc.stats[0] += 1.0;
            sc.stats[1] += sc.ep_return[0];
            sc.stats[2] += G > 1 ? sc.ep_return[1] : 0.0f;
            for (int g = 0; g < G; ++g) sc.ep_return[g] = 0.0f;
            len = 0;
            misc[2] = 1;
        }
        sc.ep_len = len;
        sc.rng = rng;
        sc.agent_steps += (unsigned long long)ntot;
        misc[3] = done;
    }
    __syncthreads();
    if (misc[2]) {
        const EnvView im = carve_env(reinterpret_cast<char*>(const_cast<uint4*>(ra.reset_image)), s.cells_n, cap, G);
        const int32_t* img_scal = reinterpret_cast<const int32_t*>(
            reinterpret_cast<const char*>(ra.reset_image) + env_image_bytes(s.cells_n, cap, G));
        const int idc = img_scal[4];
        for (int i = TID; i < s.cells_n; i += blockDim.x) v.cells[i] = im.cells[i];
        for (int i = TID; i < idc; i += blockDim.x) {
            v.xy[i] = im.xy[i]; v.hp[i] = im.hp[i]; v.next_r[i] = im.next_r[i]; v.last_r[i] = im.last_r[i];
            v.op_obj[i] = im.op_obj[i]; v.last_act[i] = im.last_act[i]; v.meta[i] = im.meta[i];
            v.rid[i] = (uint16_t)i;                  // a fresh episode: slot == id
        }
        for (int g = 0; g < G; ++g)
            for (int i = TID; i < img_scal[g]; i += blockDim.x) v.grp_ids[g * cap + i] = im.grp_ids[g * cap + i];
        if (TID < G) { v.grp_n[TID] = img_scal[TID]; v.grp_dead[TID] = 0; v.grp_reward[TID] = 0.0f; }
        if (TID == 0) { sc.id_counter = idc; s.rid_off[e] = 0; }
        __syncthreads();
    }
    MFX_BSTAMP(stamp_row, 13);
#ifdef MFX_STAMPS
    if (TID == 0 && g_stamps) g_stamps[stamp_row * kStampW + 31] = __builtin_amdgcn_s_memrealtime();
#endif
}

// Lane 0: wait until env e has no items left (its previous step observed); false on a stuck wait (error word).
// few_file calls it only once every outstanding item is held by a running workgroup (few_steal took back the rest).
__device__ __forceinline__ bool few_wait_items(const RolloutArgs& ra, int e) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (uint32_t spins = 0; !q_stalled(t0, spins); ++spins) {
        if (qld(ra.q_left + e) == 0) return true;
        __builtin_amdgcn_s_sleep(1);
    }
    __hip_atomic_store(ra.q_done + 2, kQErrStall, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return false;
}

// One wave: take back the items of env e's last filing (rec) that no workgroup has taken yet -- a holder resets its
// slot to 0 when it takes the item (bigq_wait), so lane j races slot first + j (and + 64) with one compare-and-swap
// of the filed word against the stolen mark.  rec->steal: which were taken; returns their number (every lane).
__device__ __forceinline__ int few_steal(const RolloutArgs& ra, int par, uint32_t tag, int e, FewFiled* rec) {
    const int lane = TID & 63;
    uint32_t* w = ra.q_items + ((size_t)par * kXcds + e % kXcds) * ra.q_list_cap + rec->first;
    const uint32_t mark = (tag << kQTagShift) | kQStolen;
    int n = 0;
    for (int h = 0; h < 2; ++h) {
        const int j = h * 64 + lane;
        bool took = false;
        if (j < rec->count) {
            uint32_t v = rec->words[j];
            took = __hip_atomic_compare_exchange_strong(w + j, &v, mark, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT);
        }
        const unsigned long long b = __ballot(took);
        if (lane == 0) rec->steal[h] = b;
        n += __popcll(b);
    }
    return n;
}

// One wave (the stepper's filer): file env e's items of step si once its previous step's items are all observed
// (they write the same view rows).  Common case: q_left[e] reads 0 and the items go out at once.  Else the items
// nobody has taken are taken back (few_steal) -- no other workgroup of the launch may be resident on this XCD, or
// all may be busy -- and the filing waits for the stepper to observe them itself after its step (few_stolen): 0.
// Items already taken are held by running workgroups, so the wait for them ends.  1: filed; -1: a stuck wait.
__device__ __forceinline__ int few_file(const RolloutArgs& ra, const int32_t* fcnt, int G, int e, int par,
                                        uint32_t tag, uint32_t si, FewFiled* rec) {
    const int lane = TID & 63;
    int r = 1;
    if (lane == 0) r = qld(ra.q_left + e) == 0 ? 1 : 2;
    r = __shfl(r, 0);
    if (r == 2) {
        if (few_steal(ra, par, tag, e, rec) > 0) return 0;
        if (lane == 0) r = few_wait_items(ra, e) ? 1 : -1;
        r = __shfl(r, 0);
        if (r < 0) return -1;
    }
    if (lane == 0) {
        __hip_atomic_store(ra.q_si + e, si, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bigq_file(ra, fcnt, G, e, par, tag, si, rec);
    }
    return 1;
}

// One observation item of the pipelined form (bigq_file's word it: env, group and chunk of obs_item_rows agents): the
// view and feature rows from the env's snapshot of the filed step's parity, with LDS scratch at base; then every wave
// drains its stores and the item is counted off (q_left; the env-step's last item counts the observed env-step in
// xcd_done: the stepper stepped already).  The whole workgroup; returns in every lane whether it was the step's last
// item, *qstep (LDS) the env's step counter then.  (k_rollout_bigq<false> keeps its own copy of this body inline:
// as a call its step spilled 3x the scratch.)
__device__ __forceinline__ bool few_observe(const GameParams& gp, const State& s, const RolloutArgs& ra, int par, int it,
                                             char* base, int* qflag, uint32_t* qstep) {
    constexpr int NV = BattleShape::VW * BattleShape::VH, NC = BattleShape::NC, F = BattleShape::F;
    const int G = BattleShape::G, R = ra.obs_item_rows, W = gp.W, H = gp.H;
    const int lane = TID & 63, wid = TID >> 6, nw = blockDim.x >> 6;
    const int e = (it >> 7) & ((1 << kQEnvBits) - 1), g = (it >> 6) & 1, a0 = (it & 63) * R;
    {
        size_t off = 0;
        ObsSmem sm = carve_obs(base, gp, 0, 0, R, obs_stage_floats(gp, 0, true, blockDim.x), true, off);
        obs_prologue(gp, sm, 0);
        uint32_t* snap_info = nullptr;
        float* snap_mm = nullptr;
        const EnvView v = snap_view(s, ra, e, (int)((it >> kQStepShift) & 1), G, &snap_info, &snap_mm);
        const int na = min(R, qld(v.grp_n + g) - a0);
        const float* mmg = snap_mm;
        for (int i = TID; i < G * NV; i += blockDim.x) sm.mm[i] = mmg[i];
        EnvView vc = v;
        vc.grp_ids = v.grp_ids + a0;
        obs_agent_records(gp, vc, sm, g, na);
        __syncthreads();
        const TypeParams& T = gp.type[g];
        float* ov = ra.view[g] + ((size_t)e * ra.rowcap + a0) * (NV * NC);
        float* of = ra.feat[g] + ((size_t)e * ra.rowcap + a0) * F;
        const float* mm_own = sm.mm + g * NV;
        const float* mm_en = sm.mm + (g ^ 1) * NV;
        g_u16* cells = (g_u16*)v.cells;
        g_cu32* info = (g_cu32*)snap_info;
        float* st = sm.stage + wid * kWaveStageFloats;
        const int ncell = na * NV;
        for (int b0 = wid * kQPf * kWaveCells; b0 < ncell; b0 += nw * kQPf * kWaveCells) {
            CellPre p[kQPf];
            uint32_t cv[kQPf], inf[kQPf];
#pragma unroll
            for (int d = 0; d < kQPf; ++d)
                p[d] = obs_cell_pre(sm, mm_own, mm_en, W, H, b0 + d * kWaveCells + lane, ncell);
#pragma unroll
            for (int d = 0; d < kQPf; ++d) cv[d] = cells[p[d].idx];
#pragma unroll
            for (int d = 0; d < kQPf; ++d) inf[d] = info[(p[d].ok && cv[d] < kCellFood) ? cv[d] : 0u];
#pragma unroll
            for (int d = 0; d < kQPf; ++d) {
                const int b = b0 + d * kWaveCells;
                if (b >= ncell) break;
                obs_stage_cell(st, lane, obs_cell_post_g(p[d], cv[d], inf[d], g));
                wave_sync_lds();
                obs_flush(ov + (size_t)b * NC, st, lane, min(kWaveCells, ncell - b));
                wave_sync_lds();
            }
        }
        // features (GridWorld.cc:411-421)
        const int emb = gp.emb, nact = T.n_action;
        for (int q = TID; q < na * F; q += blockDim.x) {
            const int a = q / F, f = q - a * F;
            const int id = vc.grp_ids[g * v.cap + a];
            float val = 0.0f;
            if (f < emb) val = (float)((v.rid[id] >> f) & 1);
            if (f == emb + (int)last_action(v.last_act[id])) val = 1.0f;
            if (f == emb + nact) val = v.last_r[id];
            const uint32_t pos = v.xy[id];
            if (f == emb + nact + 1) val = (float)(int)(pos & 0xFFFF) / (float)W;
            if (f == emb + nact + 2) val = (float)(int)(pos >> 16) / (float)H;
            __builtin_nontemporal_store(val, of + q);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every wave: its view rows have reached L2
    __syncthreads();                          // and every load of env e's state has returned
    if (TID == 0) {
        const int left = __hip_atomic_fetch_add(ra.q_left + e, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *qflag = left == 1;
        if (left == 1) *qstep = qldu(ra.q_si + e);
        if (left == 1) __hip_atomic_fetch_add(xcd_done(ra, par, e % kXcds), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    return *qflag != 0;
}

// The whole stepper workgroup, after its step: observe the items few_file took back (their snapshot is in HBM, the
// scratch past the stepper's LDS layout), then wait for the rest and file the step's items.  False: a stuck wait.
__device__ __forceinline__ bool few_stolen(const GameParams& gp, const State& s, const RolloutArgs& ra, int e, int par,
                                           uint32_t tag, uint32_t si, FewFiled* rec, const int32_t* fcnt, char* scratch,
                                           int* oflag, uint32_t* ostep, int* okw) {
    // this CU's L1 may hold lines of the snapshot from items it observed earlier: drop them, as an item holder does
    if (TID == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    for (int h = 0; h < 2; ++h) {
        unsigned long long m = rec->steal[h];
        while (m) {
            const int j = h * 64 + __builtin_ctzll(m);
            m &= m - 1;
            (void)few_observe(gp, s, ra, par, (int)(rec->words[j] & ((1u << kQTagShift) - 1)), scratch, oflag, ostep);
        }
    }
    if (TID == 0) {
        const bool ok = few_wait_items(ra, e);
        if (ok) {
            __hip_atomic_store(ra.q_si + e, si, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            bigq_file(ra, fcnt, BattleShape::G, e, par, tag, si, rec);
        }
        *okw = ok;
    }
    __syncthreads();
    return *okw != 0;
}

// The pipelined few-env form of k_rollout_bigq (RolloutArgs::few_pipe): stepper workgroups per env, every item
// filed and observed within the launch (parity par, tag_cur), xcd_done counting the env-steps whose items are all
// observed.  The stepper roles are claimed per XCD, first by every workgroup as it starts, then by waiting workers
// (bigq_wait): any workgroup of the launch on an XCD can step its envs, observe their items and take back the items
// nobody has taken (few_file), so the launch completes with one resident workgroup per XCD -- other work on the
// device (another process, a profiler, a second stream) may hold the rest.  x: this workgroup's XCD.
__device__ __forceinline__ void few_rollout(const GameParams& gp, const State& s, const RolloutArgs& ra, int x,
                                            uint32_t si0, int n_sub, int par, uint32_t tag_cur, char* smem) {
    __shared__ int misc[4];
    __shared__ int qitem, qflag, qclaim;
    __shared__ uint32_t qstep;
    const int G = BattleShape::G;
    const int lane = TID & 63, wid = TID >> 6, nw = blockDim.x >> 6;
    int step_env = -1;
    {
        // the stepper role: env x + 8 t for the t-th workgroup of this XCD to ask
        if (TID == 0) {
            const int t = __hip_atomic_fetch_add(ra.q_step + x, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int e = x + kXcds * t;
            qclaim = e < s.E ? e : -1;
        }
        __syncthreads();
        step_env = qclaim;
    }
    int held = -1;                                // lane 0: a ticket kept while this workgroup steps a claimed env
    while (true) {
        if (step_env >= 0) {
            const int e = step_env;
            __shared__ EnvScalars fsc;
            __shared__ int32_t fcnt[kMaxGroups];
            __shared__ int farrive, fdefer, oflag;
            __shared__ uint32_t ostep;
            __shared__ FewFiled ffil;
            const BigLayout L = big_layout(gp, s.cap, s.acap, true, true);
            char* const oscratch = smem + L.total;        // few_stolen's observation scratch (bigq_smem_bytes)
            if (TID == 0) { farrive = 0; fdefer = 0; ffil.count = 0; ffil.first = 0; }
            {                                     // the env and its scalars into LDS for the whole launch
                const EnvView gv = global_view(s, e, G);
                EnvView lv = few_lds_view(gp, s, smem, e);
                big_env_copy(s, G, gv, lv, lv.grp_n, true, s.id_counter[e]);
                load_serial_types(gp, *reinterpret_cast<StepSmem*>(smem + L.sm));
                int* hist = reinterpret_cast<int*>(smem + L.hist);          // (few_snapshot: zero between steps)
                for (int i = TID; i < G * BattleShape::VW * BattleShape::VH; i += blockDim.x) hist[i] = 0;
                if (TID == 0) {
                    fsc.id_counter = s.id_counter[e];
                    fsc.rng = s.rng[e];
                    fsc.ep_len = ra.ep_len[e];
                    for (int k = 0; k < 4; ++k) fsc.stats[k] = ra.stats[(size_t)e * 4 + k];
                    for (int g = 0; g < G; ++g) fsc.ep_return[g] = ra.ep_return[(size_t)e * G + g];
                    fsc.agent_steps = ra.agent_steps[e];
                    misc[3] = s.done[e];
                }
                __syncthreads();
            }
            bool ok = true;
            __shared__ FewSnapCtx snc;
            __shared__ FewStepCtx stc;
            if (TID == 0) { few_snap_ctx(gp, s, ra, smem, e, snc); few_step_ctx(gp, s, ra, smem, e, stc); }
            __syncthreads();
            for (int k = 0; k < n_sub && ok; ++k) {
                const uint32_t si = si0 + (uint32_t)k;
                // stamps build: one row per env and step of the launch (the buffer holds E * n_sub rows)
                const int srow = ra.env_base + e + s.E * k;
                (void)srow;
                MFX_BSTAMP(srow, 20);
#ifdef MFX_STAMPS
                if (TID == 0 && g_stamps) g_stamps[srow * kStampW + 30] = __builtin_amdgcn_s_memrealtime();
#endif
                int ntot = 0;
                for (int g = 0; g < G; ++g) ntot += lds_rebase(snc.lv.grp_n, smem)[g];
                const bool wave = ntot <= ra.few_wave_max;
                // overlap: wave 0 steps at once while the other waves drain the snapshot's stores and the last
                // of them files the items (only wave 0 reads or writes the env meanwhile; fcnt holds the counts)
                const bool overlap = wave;
                few_snapshot(snc, smem, (int)(si & 1u), fsc.id_counter, overlap ? 64 : 0, fcnt, srow);
                uint32_t rng = 0;
                int done = 0;
                float kills = 0.0f;
                if (!overlap) {
                    few_minimap(snc, smem, (int)(si & 1u), TID, blockDim.x, fcnt);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every wave: its snapshot stores reached L2
                    {
                        // the workgroup team: its first barrier (few_agents) follows every wave's drain, and the
                        // last wave files the items beside the policy loop (agent_phase's mid), where it holds no
                        // agent up to 448 of them
#ifdef MFX_STAMPS
                        if (TID == 0 && g_stamps) {
                            const unsigned long long t = __builtin_amdgcn_s_memtime();
                            g_stamps[srow * kStampW + 21] = t; g_stamps[srow * kStampW + 22] = t;
                        }
#endif
#ifndef MFX_BIGQ_NO_PRIO
                        __builtin_amdgcn_s_setprio(3);
#endif
                        auto file_items = [&]() {
                            if (wid == nw - 1) {
                                const int r = few_file(ra, fcnt, G, e, par, tag_cur, si, &ffil);
                                if (lane == 0) { qflag = r >= 0; fdefer = r == 0; }
                            }
                        };
                        few_agents<false>(gp, s, ra, e, si, stc, smem, misc, fsc, srow, rng, done, kills, file_items);
                        ok = qflag;                   // (read after the step's later barriers)
                    }
                } else {                              // (few_snapshot ended with the barrier: its LDS reads are done)
#ifdef MFX_STAMPS
                    if (TID == 0 && g_stamps) {
                        const unsigned long long t = __builtin_amdgcn_s_memtime();
                        g_stamps[srow * kStampW + 21] = t; g_stamps[srow * kStampW + 22] = t;
                    }
#endif
                    if (wid == 0) {
#ifndef MFX_BIGQ_NO_PRIO
                        __builtin_amdgcn_s_setprio(3);
#endif
                        few_agents<true>(gp, s, ra, e, si, stc, smem, misc, fsc, srow, rng, done, kills);
                    } else {
                        few_minimap(snc, smem, (int)(si & 1u), (int)TID - 64, (int)blockDim.x - 64, fcnt);
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's snapshot stores reached L2
                        if (lane == 0) atomicAdd(&farrive, 1);
                        if (wid == nw - 1) {
                            if (lane == 0) {
                                while (__hip_atomic_load(&farrive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < nw - 1)
                                    __builtin_amdgcn_s_sleep(1);
                                farrive = 0;
                            }
                            const int r = few_file(ra, fcnt, G, e, par, tag_cur, si, &ffil);
                            if (lane == 0) { qflag = r >= 0; fdefer = r == 0; }
                        }
                    }
                    __syncthreads();
                    ok = qflag;
                }
                few_env_end(gp, s, ra, e, stc, smem, misc, fsc, srow, ntot, rng, done, kills);
                if (ok && fdefer) {                   // (uniform: few_env_end ended with a barrier)
                    ok = few_stolen(gp, s, ra, e, par, tag_cur, si, &ffil, fcnt, oscratch, &oflag, &ostep, &qflag);
                    if (TID == 0) fdefer = 0;
                    __syncthreads();
                }
#ifndef MFX_BIGQ_NO_PRIO
                __builtin_amdgcn_s_setprio(0);
#endif
            }
            {                                     // the state and its scalars back to HBM
                EnvView gv = global_view(s, e, G);
                const EnvView lv = few_lds_view(gp, s, smem, e);
                big_env_copy(s, G, lv, gv, nullptr, false, fsc.id_counter);
                if (TID == 0) {
                    s.id_counter[e] = fsc.id_counter;
                    s.rng[e] = fsc.rng;
                    s.n_atk[e] = 0;
                    s.n_mov[e] = 0;
                    s.done[e] = misc[3];
                    ra.ep_len[e] = fsc.ep_len;
                    for (int k = 0; k < 4; ++k) ra.stats[(size_t)e * 4 + k] = fsc.stats[k];
                    for (int g = 0; g < G; ++g) ra.ep_return[(size_t)e * G + g] = fsc.ep_return[g];
                    ra.agent_steps[e] = fsc.agent_steps;
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            step_env = -1;
            // then an item worker like the others (a stuck wait stops the launch: the error word is set)
            if (!ok) break;
        }
        __syncthreads();               // every lane has read the previous answer (a skip or a claim)
        if (TID == 0) {
            int t = held;
            held = -1;
            if (t < 0) t = bigq_ticket(ra, par, x);
            int c = -1;
            const int r = bigq_wait<true>(ra, par, x, t, tag_cur, xcd_target(s.E, x, n_sub), s.E, &c);
            if (r == kQClaim) { held = t; qclaim = c; }
            qitem = r;
        }
        __syncthreads();
        const int it = qitem;
        if (it == kQOver) break;
        if (it == kQClaim) { step_env = qclaim; continue; }
        if (it < 0) continue;                     // (kQSkip: its env's stepper observed the item itself)
        // acquire: the env's state reached this XCD's L2 before the item word (see above); drop this CU's
        // L1 lines of it.  Then the guard: the step counter, read like the state, is the filed step.
        if (TID == 0) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const uint32_t w = (uint32_t)it;
            const uint32_t seen = ra.q_si[(w >> 7) & ((1u << kQEnvBits) - 1u)];   // a plain load, as the state is read
            if (((seen ^ (w >> kQStepShift)) & kQStepMask) != 0u)
                __hip_atomic_store(ra.q_done + 2, kQErrGuard, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        (void)few_observe(gp, s, ra, par, it, smem, &qflag, &qstep);   // (the stepper stepped already)
    }
}

// One launch: steps [si0, si0 + n_sub) of every env.  tag_cur / tag_next: the item tags of this
// launch and of the next one.
// two workgroups per CU (<= 128 VGPRs; ~80 KB of LDS each).  kPipe: the pipelined few-env form (few_rollout).
template <bool kPipe>
__global__ void __launch_bounds__(kBigRolloutThreads, 2 * kBigRolloutThreads / 256) k_rollout_bigq(const GameParams* __restrict__ gpp,
                                                              const RolloutCtx* __restrict__ ctx, uint32_t si0,
                                                              int n_sub, int par, uint32_t tag_cur,
                                                              uint32_t tag_next) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int misc[4];
    __shared__ int qitem, qflag;
    __shared__ uint32_t qstep;
    constexpr int NV = BattleShape::VW * BattleShape::VH, NC = BattleShape::NC, F = BattleShape::F;
    const GameParams& gp = *gpp;
    const State& s = ctx->s;
    const RolloutArgs& ra = ctx->ra;
    const int G = BattleShape::G, R = ra.obs_item_rows, W = gp.W, H = gp.H;
    const int lane = TID & 63, wid = TID >> 6, nw = blockDim.x >> 6;
    const int x = xcc_id();
    if (x >= kXcds) {                             // not one SPX device of 8 XCDs: env e's list would be orphaned
        if (TID == 0) __hip_atomic_store(ra.q_done + 2, kQErrXcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    if (kPipe) {
        few_rollout(gp, s, ra, x, si0, n_sub, par, tag_cur, smem);
        return;
    }
    int next_t = -1;                              // lane 0: a ticket taken while the last item streamed
    while (true) {
        if (TID == 0) {
            const int t = next_t >= 0 ? next_t : bigq_ticket(ra, par, x);
            int c = -1;
            qitem = bigq_wait<false>(ra, par, x, t, tag_cur, xcd_target(s.E, x, n_sub), s.E, &c);
        }
        __syncthreads();
        const int it = qitem;
        if (it < 0) break;
        // acquire: the env's state reached this XCD's L2 before the item word (see above); drop this CU's
        // L1 lines of it.  Then the guard: the step counter, read like the state, is the filed step.
        if (TID == 0) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const uint32_t w = (uint32_t)qitem;
            const uint32_t seen = ra.q_si[(w >> 7) & ((1u << kQEnvBits) - 1u)];   // a plain load, as the state is read
            if (((seen ^ (w >> kQStepShift)) & kQStepMask) != 0u)
                __hip_atomic_store(ra.q_done + 2, kQErrGuard, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#ifdef MFX_BIGQ_TICKET_PF
            next_t = bigq_ticket(ra, par, x);     // its round trip overlaps this item
#endif
        }
        __syncthreads();
        const int e = (it >> 7) & ((1 << kQEnvBits) - 1), g = (it >> 6) & 1, a0 = (it & 63) * R;
        {
            size_t off = 0;
            ObsSmem sm = carve_obs(smem, gp, 0, 0, R, obs_stage_floats(gp, 0, true, blockDim.x), true, off);
            obs_prologue(gp, sm, 0);
            const EnvView v = global_view(s, e, G);      // (the step runs after the items)
            const int na = min(R, qld(v.grp_n + g) - a0);
            const float* mmg = ra.obs_mm + (size_t)e * G * NV;
            for (int i = TID; i < G * NV; i += blockDim.x) sm.mm[i] = mmg[i];
            EnvView vc = v;
            vc.grp_ids = v.grp_ids + a0;
            obs_agent_records(gp, vc, sm, g, na);
            __syncthreads();
            const TypeParams& T = gp.type[g];
            float* ov = ra.view[g] + ((size_t)e * ra.rowcap + a0) * (NV * NC);
            float* of = ra.feat[g] + ((size_t)e * ra.rowcap + a0) * F;
            const float* mm_own = sm.mm + g * NV;
            const float* mm_en = sm.mm + (g ^ 1) * NV;
            g_u16* cells = (g_u16*)v.cells;
            g_cu32* info = (g_cu32*)(ra.obs_info + (size_t)e * s.cap);
            float* st = sm.stage + wid * kWaveStageFloats;
            const int ncell = na * NV;
            for (int base = wid * kQPf * kWaveCells; base < ncell; base += nw * kQPf * kWaveCells) {
                CellPre p[kQPf];
                uint32_t cv[kQPf], inf[kQPf];
#pragma unroll
                for (int d = 0; d < kQPf; ++d)
                    p[d] = obs_cell_pre(sm, mm_own, mm_en, W, H, base + d * kWaveCells + lane, ncell);
#pragma unroll
                for (int d = 0; d < kQPf; ++d) cv[d] = cells[p[d].idx];
#pragma unroll
                for (int d = 0; d < kQPf; ++d) inf[d] = info[(p[d].ok && cv[d] < kCellFood) ? cv[d] : 0u];
#pragma unroll
                for (int d = 0; d < kQPf; ++d) {
                    const int b = base + d * kWaveCells;
                    if (b >= ncell) break;
                    obs_stage_cell(st, lane, obs_cell_post_g(p[d], cv[d], inf[d], g));
                    wave_sync_lds();
                    obs_flush(ov + (size_t)b * NC, st, lane, min(kWaveCells, ncell - b));
                    wave_sync_lds();
                }
            }
            // features (GridWorld.cc:411-421)
            const int emb = gp.emb, nact = T.n_action;
            for (int q = TID; q < na * F; q += blockDim.x) {
                const int a = q / F, f = q - a * F;
                const int id = vc.grp_ids[g * v.cap + a];
                float val = 0.0f;
                if (f < emb) val = (float)((v.rid[id] >> f) & 1);
                if (f == emb + (int)last_action(v.last_act[id])) val = 1.0f;
                if (f == emb + nact) val = v.last_r[id];
                const uint32_t pos = v.xy[id];
                if (f == emb + nact + 1) val = (float)(int)(pos & 0xFFFF) / (float)W;
                if (f == emb + nact + 2) val = (float)(int)(pos >> 16) / (float)H;
                __builtin_nontemporal_store(val, of + q);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every wave: its view rows have reached L2
        __syncthreads();                          // and every load of env e's state has returned
        if (TID == 0) {
            const int left = __hip_atomic_fetch_add(ra.q_left + e, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            qflag = left == 1;
            if (left == 1) qstep = qldu(ra.q_si + e);
        }
        __syncthreads();
        if (!qflag) continue;
        // the last item of env e's step: the step itself (LDS re-carved by big_env_step)
        const uint32_t si = qstep;
#ifndef MFX_BIGQ_NO_PRIO
        // the latency-bound step ahead of the streaming waves of its CU: +1.1 % (3 of 3 interleaved
        // runs, profiles/r02_bigq_sweeps.txt)
        __builtin_amdgcn_s_setprio(3);
#endif
#ifdef MFX_BIGQ_CALL
        big_env_step_call(gp, s, ra, e, si, smem, misc);
#else
        big_env_step(gp, s, ra, e, si, smem, misc);
#endif
#ifndef MFX_BIGQ_NO_PRIO
        __builtin_amdgcn_s_setprio(0);
#endif
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // every wave: its stores have left
        __syncthreads();
        if (TID == 0) {
            // No agent-scope release (L2 write-back): every consumer of env e runs on this XCD and reads
            // through its L2, which the drained stores above have reached; the consumers' acquire drops
            // their CUs' L1 lines.  The write-back of the XCD's whole dirty L2 (the streaming view rows
            // of 64 workgroups) per env-step cost 7 % (1.07-1.11e9 vs 1.17-1.18e9, 3 of 3 interleaved runs,
            // parity tests green both ways: profiles/r02_bigq_sweeps.txt).  MFX_BIGQ_RELEASE: A/B only.
#ifdef MFX_BIGQ_RELEASE
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
#endif
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const bool last = (int)(si + 1u - si0) >= n_sub;
            __hip_atomic_store(ra.q_si + e, si + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            bigq_file(ra, s.grp_n + (size_t)e * G, G, e, last ? par ^ 1 : par, last ? tag_next : tag_cur, si + 1u);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_fetch_add(xcd_done(ra, par, e % kXcds), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

