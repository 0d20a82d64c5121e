// battle_rollout.cpp -- the Battle engine's fused rollout (bench / throughput path): rollout_init, the plan
// (BattleEngine::Plan, rollout_plan and its per-family sizing), one step function per plan, the learned-policy steps.
#include "battle_engine.h"

namespace mfx {

// ------------------------------------------------------------------ env slices
// A per-env buffer is listed twice, here: in sub_state (State) or in env_args (RolloutArgs).
// envs [e0, e0 + n) of s / ra as a batch of their own (every per-env array offset by e0)
State BattleEngine::sub_state(int e0, int n) const {
    State q = s;
    const size_t G = (size_t)n_groups(), c = (size_t)s.cap, a = (size_t)s.acap, cn = (size_t)s.cells_n;
    q.E = n;
    q.cells += e0 * cn; q.xy += e0 * c; q.hp += e0 * c; q.next_r += e0 * c; q.last_r += e0 * c;
    q.last_act += e0 * c; q.op_obj += e0 * c; q.meta += e0 * c; q.grp_ids += e0 * G * c;
    q.grp_n += e0 * G; q.grp_dead += e0 * G; q.grp_reward += e0 * G; q.id_counter += e0; q.rng += e0;
    q.rid += e0 * c; q.rid_off += e0;
    q.atk += e0 * a; q.n_atk += e0; q.mov += e0 * a; q.n_mov += e0; q.done += e0;
    if (q.food) q.food += e0 * cn;
    q.idx_mark += e0;
    return q;
}
RolloutArgs BattleEngine::env_args(int e0) const {
    RolloutArgs q = ra;
    const int G = n_groups();
    const size_t rc = (size_t)ra.rowcap;
    for (int g = 0; g < G; g++) {
        const TypeParams& T = gp.type[g];
        q.view[g] += e0 * rc * T.view_w * T.view_h * gp.n_ch;
        q.feat[g] += e0 * rc * gp.feat_size[g];
    }
    q.actions += e0 * G * rc; q.rewards += e0 * G * rc; q.mean_act += (size_t)e0 * G * ra.mean_stride;
    q.ids += e0 * G * rc; q.alive += e0 * G * rc;
    q.ep_return += (size_t)e0 * G; q.ep_len += e0; q.stats += (size_t)e0 * 4; q.agent_steps += e0;
    if (q.obs_mm) { q.obs_mm += (size_t)e0 * G * 169; q.obs_info += (size_t)e0 * s.cap; }
    q.env_base = e0;
    if (q.big_sort) q.big_sort += (size_t)e0 * s.acap;
    return q;
}

// The two-stream pipeline's view of sub-batch k (envs from e0): every per-env array from e0, the sub-batch's own
// item lists and counters.
RolloutArgs BattleEngine::stream_args(int e0, int k) const {
    RolloutArgs q = env_args(e0);
    if (q.obs_items) {   // sub-batch k's lists: obs_lists x obs_list_stride items from (e0 + kXcds k) env slots
        const size_t slots = (size_t)n_groups() * ((ra.rowcap + ra.obs_item_rows - 1) / ra.obs_item_rows);
        q.obs_items += ((size_t)e0 + (size_t)kXcds * k) * slots;
        q.obs_cnt += 2 * kXcds * kObsCntPad * k;
        const int n = sub_envs(k);
        q.obs_list_stride = (size_t)((n + ra.obs_lists - 1) / ra.obs_lists) * slots;
    }
    return q;
}
// The queue kernel's view of env chunk k (envs [e0, e0 + n)): every per-env array from e0, the chunk's own
// queue lists and counters (plan_big_queue sizes them: q_list_cap per list of one chunk).
RolloutArgs BattleEngine::chunk_args(int e0, int k) const {
    RolloutArgs q = env_args(e0);
    q.q_items += (size_t)k * 2 * kXcds * ra.q_list_cap;
    q.q_cnt += (size_t)k * 2 * kXcds * kObsCntPad;
    q.q_left += e0; q.q_si += e0;
    return q;
}

// Bytes of one env's state a large-env step and its observation items cycle through (cells, the per-slot arrays,
// the group lists, the action buffers, the observation's minimap and info words, the move sort buffer).
size_t BattleEngine::env_state_bytes() const {
    const size_t c = (size_t)s.cap, a = (size_t)s.acap, G = (size_t)n_groups();
    return (size_t)s.cells_n * 2 + c * (4 + 4 + 4 + 4 + 1 + 4 + 1 + 2 + 4) + G * c * 2 + 3 * a * 4 + G * 169 * 4;
}

// ------------------------------------------------------------------ twin state (Plan::Pipe)
void BattleEngine::free_twin() {
    State none{};
    twin_fields(tw, none, [](auto& p, auto&) { if (p) (void)hipFree(p); p = nullptr; });
    tw_cap = tw_E = -1;
    ro_par = 0;
}
void BattleEngine::alloc_twin() {
    if (tw_cap == s.cap && tw_E == E) return;
    free_twin();
    const size_t c = (size_t)s.cap, G = (size_t)n_groups();
    alloc(tw.xy, E * c); alloc(tw.hp, E * c); alloc(tw.next_r, E * c); alloc(tw.last_r, E * c);
    alloc(tw.last_act, E * c); alloc(tw.op_obj, E * c); alloc(tw.meta, E * c); alloc(tw.grp_ids, E * G * c);
    alloc(tw.grp_n, E * G); alloc(tw.grp_dead, E * G); alloc(tw.grp_reward, E * G); alloc(tw.id_counter, E);
    alloc(tw.rng, E);
    tw_cap = s.cap; tw_E = E;
}
// s with tw's copies of the twin fields
State BattleEngine::twin_state() const {
    State t = s, x = tw;
    twin_fields(t, x, [](auto& a, auto& b) { a = b; });
    return t;
}
void BattleEngine::swap_twin() { twin_fields(s, tw, [](auto& a, auto& b) { std::swap(a, b); }); }

// ------------------------------------------------------------------ fused rollout
// Template placement per group (host arrays, applied in group order at every episode start),
// followed by an immediate reset + placement of every env.
int BattleEngine::rollout_init(const int* tmpl_n, const int* const* xs, const int* const* ys, int max_steps,
                               float eps, uint32_t seed, int stagger) {
    MFX_CHECK(flush_deferred());
    const int G = n_groups();
    if (!allocated) MFX_CHECK(reset());
    int total = 0, rowcap = 4, tcap = 1;
    for (int g = 0; g < G; g++) { total += tmpl_n[g]; rowcap = std::max(rowcap, tmpl_n[g]); tcap = std::max(tcap, tmpl_n[g]); }
    rowcap = (rowcap + 3) & ~3;                      // 16-B aligned rows (4 * 1183 floats)
    for (int g = 0; g < G; g++) {
        if (gtype(g).n_action > 64) return fail("rollout: n_action must be <= 64");
        if (gp.type[g].view_w != gp.type[0].view_w || gp.type[g].view_h != gp.type[0].view_h)
            return fail("rollout: every group must share one view size; use the per-call API");
    }
    if (gp.dsl) return fail("rollout: reward rules outside the attack/kill/collide form need the per-call API");
    if (turn || food) return fail("rollout: turn_mode / food_mode need the per-call API");
    for (int g = 0; g < G; g++)
        if (gp.type[g].body_w != 1 || gp.type[g].body_h != 1) return fail("rollout: 1x1 bodies only; use the per-call API");
    for (int g = 0; g < G; g++)
        if (gp.type[g].can_absorb) return fail("rollout: can_absorb types need the per-call API");
    try {
        ensure_capacity(total, total);
        ro_queue_want = env_flag("MFX_BIG_FUSED", true);
        const size_t smem = rollout_smem_bytes(gp, s.cells_n, s.cap, s.acap, rowcap);
        // envs too large for one workgroup's LDS run k_observe + k_rollout_big with the state in HBM
        const bool big = smem > kLdsBytes;
        if (big && (!gp.par_step || big_step_smem_bytes(gp, s.cap, s.acap, true) > kLdsBytes))
            return fail("rollout: env too large for the fused kernels (%zu bytes of LDS); use the per-call API", smem);
        // few envs (configs[3]: 8 per GPU): one workgroup per env would leave the chip idle and put each
        // env's whole observation on one CU; the queue kernel spreads every env's observation over many
        // workgroups (small items) and steps it in HBM, like the large envs
        // (batches of at most kSmallEMax LDS-sized envs take the queue kernel; MFX_SMALL_E overrides)
        ro_small_e = !big && battle_shape(gp) && n_groups() == 2 && gp.par_step &&
                     E <= env_int("MFX_SMALL_E", kSmallEMax) &&
                     big_step_smem_bytes(gp, s.cap, s.acap, true) <= kLdsBytes;
        // the family of the plan: rollout_plan() keeps it and decides the rest
        ro_plan = big || ro_small_e ? Plan::BigStreams : Plan::Fused;
        std::vector<int> hx((size_t)G * tcap, 0), hy((size_t)G * tcap, 0);
        for (int g = 0; g < G; g++)
            for (int i = 0; i < tmpl_n[g]; i++) { hx[(size_t)g * tcap + i] = xs[g][i]; hy[(size_t)g * tcap + i] = ys[g][i]; }
        ro_tx.ensure(hx.size()); ro_ty.ensure(hy.size());
        MFX_HIP_THROW(hipMemcpy(ro_tx.p, hx.data(), sizeof(int) * hx.size(), hipMemcpyHostToDevice));
        MFX_HIP_THROW(hipMemcpy(ro_ty.p, hy.data(), sizeof(int) * hy.size(), hipMemcpyHostToDevice));
        RolloutArgs a{};
        for (int g = 0; g < G; g++) {
            const TypeParams& T = gp.type[g];
            ro_view[g].ensure((size_t)E * rowcap * T.view_w * T.view_h * gp.n_ch);
            ro_feat[g].ensure((size_t)E * rowcap * gp.feat_size[g]);
            a.view[g] = ro_view[g].p; a.feat[g] = ro_feat[g].p;
            a.tmpl_n[g] = tmpl_n[g];
        }
        int na = 0;
        for (int g = 0; g < G; g++) na = std::max(na, gtype(g).n_action);
        ro_actions.ensure((size_t)E * G * rowcap); ro_rewards.ensure((size_t)E * G * rowcap);
        ro_mean.ensure((size_t)E * G * na); ro_return.ensure((size_t)E * G); ro_eplen.ensure(E);
        ro_ids.ensure((size_t)E * G * rowcap); ro_alive.ensure((size_t)E * G * rowcap);
        MFX_HIP_THROW(hipMemset(ro_ids.p, 0, sizeof(int32_t) * E * G * rowcap));
        MFX_HIP_THROW(hipMemset(ro_alive.p, 0, (size_t)E * G * rowcap));
        ro_stats.ensure((size_t)E * 4); ro_steps.ensure(E);
        MFX_HIP_THROW(hipMemset(ro_return.p, 0, sizeof(float) * E * G));
        MFX_HIP_THROW(hipMemset(ro_mean.p, 0, sizeof(double) * ro_mean.n));   // former_act_prob = 0 at step 0
        // stagger episode phases over envs: env e's first episode is cut at max_steps - e*max_steps/E,
        // so after max_steps steps the batch cycles through every phase of an episode uniformly
        std::vector<int32_t> phase((size_t)E);
        for (int e = 0; e < E; e++) phase[e] = stagger ? (int32_t)((long long)e * max_steps / E) : 0;
        MFX_HIP_THROW(hipMemcpy(ro_eplen.p, phase.data(), sizeof(int32_t) * E, hipMemcpyHostToDevice));
        MFX_HIP_THROW(hipMemset(ro_stats.p, 0, sizeof(double) * E * 4));
        MFX_HIP_THROW(hipMemset(ro_steps.p, 0, sizeof(unsigned long long) * E));
        a.rowcap = rowcap; a.actions = ro_actions.p; a.rewards = ro_rewards.p; a.mean_act = ro_mean.p;
        a.mean_stride = na;
        a.ids = ro_ids.p; a.alive = ro_alive.p;
        a.ep_return = ro_return.p; a.ep_len = ro_eplen.p; a.stats = ro_stats.p; a.agent_steps = ro_steps.p;
        a.tmpl_x = ro_tx.p; a.tmpl_y = ro_ty.p; a.tmpl_cap = tcap;
        a.max_steps = max_steps; a.policy_seed = seed; a.step_index = 0; a.eps = eps;
        ra = a;
    } catch (const HipFailure& f) {
        return fail("%s", f.what());
    }
    MFX_CHECK(reset());
    for (int g = 0; g < G; g++) MFX_CHECK(add_agents(g, tmpl_n[g], "custom", xs[g], ys[g], nullptr));
    MFX_CHECK(rollout_plan());
    rollout_ready = true;
    walls_after_init = false;
    return 0;
}

// Reset image, work queue and persistent grid for the current capacity: the shared prologue, then the sizing of the
// plan's family.  Everything but the family (LDS-sized or HBM plans: rollout_init) is decided afresh here.
int BattleEngine::rollout_plan() {
    ro_prep_stale = true;                    // the large-env observation inputs follow the new plan
    try {
        const bool hbm = plan_hbm();
        plan_prologue();
        if (hbm) {
            plan_big_lists();
            ro_plan = battle_shape(gp) ? plan_big_queue() : Plan::BigStreams;
            plan_big_batches();
        } else {
            ro_plan = env_flag("MFX_ROLLOUT_PIPE", kPipeDefault) ? Plan::Pipe : Plan::Fused;
            if (ro_plan == Plan::Pipe) plan_twin();
            else MFX_HIP_THROW(rollout_grid(gp, s, ra.rowcap, 0, 0, &ro_grid));
        }
        ro_cap = s.cap;
        ro_ctx.ensure(1);
        ro_ctx_host.s = s; ro_ctx_host.ra = ra; ro_ctx_host.w = s;
        MFX_HIP_THROW(hipMemcpyAsync(ro_ctx.p, &ro_ctx_host, sizeof(RolloutCtx), hipMemcpyHostToDevice, stream));
        if (ro_plan == Plan::BigQueue) {
            ro_qc_ctx.ensure(ro_qchunks);
            std::vector<RolloutCtx> qc(ro_qchunks);
            for (int k = 0; k < ro_qchunks; ++k) {
                const int e0 = ro_qc_e0[k], n = ro_qc_e0[k + 1] - e0;
                ro_qc_s[k] = ro_qchunks > 1 ? sub_state(e0, n) : s;
                ro_qc_ra[k] = ro_qchunks > 1 ? chunk_args(e0, k) : ra;
                qc[k].s = ro_qc_s[k]; qc[k].ra = ro_qc_ra[k]; qc[k].w = ro_qc_s[k];
                ro_qc_par[k] = 0;
                ro_qc_launch[k] = ro_qlaunch;
            }
            MFX_HIP_THROW(hipMemcpyAsync(ro_qc_ctx.p, qc.data(), sizeof(RolloutCtx) * ro_qchunks, hipMemcpyHostToDevice,
                                         stream));
        }
        MFX_HIP_THROW(hipStreamSynchronize(stream));
    } catch (const HipFailure& f) {
        return fail("%s", f.what());
    }
    return 0;
}

// Every plan: the work counters, k_rollout's class lists, the reset image and its walls.
void BattleEngine::plan_prologue() {
    ro_work.ensure(4);                   // [0..1] k_rollout, [2..3] k_rollout_obs
    MFX_HIP_THROW(hipMemsetAsync(ro_work.p, 0, 4 * sizeof(int32_t), stream));
    ro_image.ensure((rollout_reset_image_bytes(gp, s.cells_n, s.cap) + 15) / 16);
    // queue for the next launch: every env in class 0 in index order, other counts zero
    ro_cls_cnt.ensure(3 * 8); ro_cls_list.ensure((size_t)2 * 8 * E);
    const int qp = (int)(ro_launch % 6);
    std::vector<int32_t> cnt(3 * 8, 0), idx((size_t)E);
    cnt[(qp % 3) * 8] = E;
    for (int e = 0; e < E; e++) idx[e] = e;
    MFX_HIP_THROW(hipMemcpy(ro_cls_cnt.p, cnt.data(), sizeof(int32_t) * cnt.size(), hipMemcpyHostToDevice));
    MFX_HIP_THROW(hipMemcpy(ro_cls_list.p + (size_t)(qp & 1) * 8 * E, idx.data(), sizeof(int32_t) * E,
                            hipMemcpyHostToDevice));
    ra.work = ro_work.p; ra.work_sel = 0; ra.reset_image = ro_image.p;
    ra.cls_cnt = ro_cls_cnt.p; ra.cls_list = ro_cls_list.p; ra.cls_stride = E;
    MFX_HIP_THROW(launch_reset_image(gp, d_gp, s, ra, ro_image.p, stream));
    {   // the walls of the reset image (agents removed), shared by every env's install
        std::vector<uint16_t> cells((size_t)s.cells_n);
        MFX_HIP_THROW(hipStreamSynchronize(stream));
        MFX_HIP_THROW(hipMemcpy(cells.data(), ro_image.p, cells.size() * 2, hipMemcpyDeviceToHost));
        for (auto& c : cells) if (c < kCellFood) c = kCellEmpty;
        ro_walls.ensure((cells.size() * 2 + 15) / 16);
        MFX_HIP_THROW(hipMemcpy(ro_walls.p, cells.data(), cells.size() * 2, hipMemcpyHostToDevice));
        ra.wall_image = ro_walls.p;
    }
    ra.renumber = 0;
    ra.lds_step = 0;
    ra.few_pipe = 0;
}

// The HBM plans: the step's sort buffer and forms, and for Battle-shape envs the observation inputs and the
// two-stream pipeline's item lists and grids (the policy form's grid with them).
void BattleEngine::plan_big_lists() {
    ro_grid = E;
    ro_sort.ensure((size_t)E * s.acap);
    ra.big_sort = ro_sort.p;
    // envs too large for LDS: clear_dead renumbers the slots to the list order (dense per-slot
    // arrays); LDS-sized envs (few-env path) keep slot == id, as k_rollout assumes
    // (MFX_RENUMBER: A/B only: 0 = off, 2 = no identity fast path)
    ra.renumber = ro_small_e ? 0 : std::min(std::max(env_int("MFX_RENUMBER", 1), 0), 2);
    // few LDS-sized envs: each env is staged in LDS for its step (big_env_step)
    ra.lds_step = ro_small_e && env_flag("MFX_LDS_STEP", true);           // A/B only: 0 = the step in HBM
    if (!battle_shape(gp)) return;
    ro_mm.ensure((size_t)E * n_groups() * 169);
    ro_info.ensure((size_t)E * s.cap);
    ra.obs_mm = ro_mm.p; ra.obs_info = ro_info.p;
    const int R = kItemRows;
    const size_t slots = (size_t)(ra.rowcap + R - 1) / R;
    // per sub-batch of n envs: obs_lists lists of ceil(n / obs_lists) envs' items each,
    // i.e. at most n + kXcds env slots
    const size_t par_stride = ((size_t)E + (size_t)kXcds * kMaxSplit) * n_groups() * slots;
    ro_items.ensure(2 * par_stride);
    ro_cnt.ensure(2 * kXcds * kObsCntPad * kMaxSplit);
    ra.obs_lists = kXcds;                           // one list per XCD (profiles/r02_xcd_items_ab.txt)
    ra.obs_items = ro_items.p; ra.obs_cnt = ro_cnt.p;
    ra.obs_par_stride = par_stride; ra.obs_item_rows = R;
    MFX_HIP_THROW(observe_items_grid(gp, R, &ro_item_grid));
    {   // the policy form's launch runs alone: every slot of the chip (256x256, 2048 envs: 7.9 ms per
        // step + observation against 11.6 at a third), but no more workgroups than items (one
        // 40x40 env: 0.13 ms against 0.35 with the full grid) -- MFX_POLICY_ITEM_DIV: A/B only
        const int pd = env_int("MFX_POLICY_ITEM_DIV", 1);
        const long long items = (long long)E * n_groups() * (long long)slots;
        ro_pol_item_grid = std::max(1, ro_item_grid / (pd > 0 ? pd : 1));
        ro_pol_item_grid = (int)std::min<long long>(ro_pol_item_grid, std::max<long long>(kXcds, items));
        if (ro_pol_item_grid >= kXcds) ro_pol_item_grid -= ro_pol_item_grid % kXcds;
    }
    ro_item_grid = std::max(1, ro_item_grid / kItemGridDiv);
    if (ro_item_grid >= kXcds) ro_item_grid -= ro_item_grid % kXcds;   // as many per XCD
}

// The queue kernel (k_rollout_bigq) on the HBM plans of Battle-shape envs: rows per item, whether the kernel takes
// the batch (else Plan::BigStreams), the pipelined few-env form, the env chunks, the lists' capacity and the grid.
BattleEngine::Plan BattleEngine::plan_big_queue() {
    // the queue-driven kernel: item words hold 13 env bits and 6 chunk bits
    const int rv = env_int("MFX_BIGQ_ROWS", 0);                       // sweeps only
    const int Rq = rv > 0 ? rv : (ro_small_e ? kSmallERows : kBigqRows);
    const int chunks = (ra.rowcap + Rq - 1) / Rq;
    if (!(ro_queue_want && E <= 8192 && chunks <= 64 && n_groups() == 2 &&
          bigq_smem_bytes(gp, s.cap, s.acap, Rq, ra.lds_step) <= kLdsBytes))
        return Plan::BigStreams;
    MFX_HIP_THROW(bigq_grid(gp, s.cap, s.acap, Rq, ra.lds_step, &ro_q_grid));
    if (ro_q_grid <= 0) return Plan::BigStreams;          // (0: not one SPX device of 8 XCDs)
    // few envs with the env staged in LDS: the pipelined form (a stepper workgroup per env
    // steps while the items observe its snapshot) while the steppers leave at least 3 of 4
    // of every XCD's workgroups to the items
    ra.few_pipe = ra.lds_step && E <= ro_q_grid / 4 && env_flag("MFX_FEW_PIPE", true) &&      // A/B only: 0 = off
                  bigq_smem_bytes(gp, s.cap, s.acap, Rq, true, true) <= kLdsBytes;
    if (ra.few_pipe) {
        // (the stepper's scratch for the items it takes back follows its LDS layout)
        int pg = 0;
        MFX_HIP_THROW(bigq_grid(gp, s.cap, s.acap, Rq, true, &pg, true));
        ra.few_pipe = E <= std::min(ro_q_grid, pg) / 4;
        // (the pipe grid only when the pipelined form stays: the queue-step form keeps its
        // full grid)
        if (ra.few_pipe) ro_q_grid = std::min(ro_q_grid, pg);
    }
    // env chunks (not pipelined): envs per launch by the state bytes one launch cycles through
    ro_qchunks = 1;
    if (!ra.few_pipe) {
        const int want = env_int("MFX_BIGQ_CHUNK", INT_MIN);         // A/B and tests: envs per launch
        if (want != INT_MIN) {                                       // (set: one launch unless 0 < want < E)
            if (want > 0 && want < E)
                ro_qchunks = (int)std::min<long long>(kMaxQChunks, ((long long)E + want - 1) / want);
        } else {
            const size_t k = (size_t)E * env_state_bytes() / kBigqChunkBytes;
            ro_qchunks = (int)std::max<size_t>(1, std::min<size_t>(kMaxQChunks, k));
        }
    }
    for (int k = 0; k <= ro_qchunks; ++k) ro_qc_e0[k] = (int)((long long)E * k / ro_qchunks);
    const int qmax = (E + ro_qchunks - 1) / ro_qchunks;
    // per list and parity: one filing per env and step of a launch (<= 64 steps; the
    // pipelined form kMaxPipeSub) (+ the tickets workgroups hold past the last filing: two
    // per workgroup); one such set per env chunk
    const size_t lcap = (size_t)((qmax + kXcds - 1) / kXcds) * (ra.few_pipe ? kMaxPipeSub : 64) *
                        (size_t)(n_groups() * chunks) + 2 * (size_t)ro_q_grid;
    ro_q_items.ensure(2 * kXcds * lcap * ro_qchunks);
    ro_q_cnt.ensure(2 * kXcds * kObsCntPad * ro_qchunks);
    ro_q_left.ensure(E); ro_q_si.ensure(E); ro_q_done.ensure(kObsCntPad);
    MFX_HIP_THROW(hipMemsetAsync(ro_q_items.p, 0, ro_q_items.n * sizeof(uint32_t), stream));
    MFX_HIP_THROW(hipMemsetAsync(ro_q_done.p, 0, kObsCntPad * sizeof(int32_t), stream));
    ra.q_items = ro_q_items.p; ra.q_cnt = ro_q_cnt.p; ra.q_left = ro_q_left.p;
    ra.q_si = ro_q_si.p; ra.q_done = ro_q_done.p; ra.q_list_cap = lcap;
    ra.obs_item_rows = Rq;
    if (ra.few_pipe) {
        // (at most 64: attack_wave / move_wave give each attacker and mover one lane)
        ra.few_wave_max = kFewWaveMax;
        ra.few_snap_bytes = few_snap_bytes(s.cells_n, s.cap, n_groups());
        ro_snap.ensure((size_t)E * 2 * ra.few_snap_bytes);
        ro_q_step.ensure(kXcds);
        ra.few_snap = ro_snap.p; ra.q_step = ro_q_step.p;
        // one workgroup per CU while that leaves 3 of 4 to the items: the stepper then has its
        // CU to itself (8 envs 0.0222 -> 0.0219 ms per step, profiles/r04_few_grid_ab.txt)
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
            cus % kXcds == 0 && 4 * E <= cus)
            ro_q_grid = std::min(ro_q_grid, cus);
    }
    const int qg = env_int("MFX_BIGQ_GRID", 0);                       // sweeps only
    // (a multiple of kXcds: every XCD's list needs workgroups of its own)
    if (qg > 0) ro_q_grid = std::min(ro_q_grid, std::max(kXcds, qg - qg % kXcds));
    return ra.few_pipe ? Plan::FewPipe : Plan::BigQueue;
}

// The HBM plans' batches, cut from ra as the sizing above left it: the two-stream pipeline's sub-batches with
// their streams and events, and the policy form's one batch.
void BattleEngine::plan_big_batches() {
    const int K = std::min(ro_split, E);
    ro_sub_ctx.ensure(K);
    std::vector<RolloutCtx> subs(K);
    for (int k = 0; k < K; k++) {
        const int e0 = (int)((long long)E * k / K), e1 = (int)((long long)E * (k + 1) / K);
        ro_sub_n[k] = e1 - e0;
        ro_sub_s[k] = sub_state(e0, e1 - e0);
        ro_sub_ra[k] = stream_args(e0, k);
        subs[k].s = ro_sub_s[k]; subs[k].ra = ro_sub_ra[k];
        if (!ro_str[k]) MFX_HIP_THROW(hipStreamCreateWithFlags(&ro_str[k], hipStreamNonBlocking));
    }
    for (auto& x : ro_ev) if (!x) MFX_HIP_THROW(hipEventCreateWithFlags(&x, hipEventDisableTiming));
    MFX_HIP_THROW(hipMemcpyAsync(ro_sub_ctx.p, subs.data(), sizeof(RolloutCtx) * K, hipMemcpyHostToDevice,
                                 stream));
    // the policy form: one batch, the item lists of kItemRows agents (never the queue kernel's Rq)
    RolloutArgs q = ra;
    q.env_base = 0;
    q.few_pipe = 0;
    if (q.obs_items) {
        const size_t slots = (size_t)n_groups() * ((ra.rowcap + kItemRows - 1) / kItemRows);
        q.obs_item_rows = kItemRows;
        q.obs_list_stride = (size_t)((E + q.obs_lists - 1) / q.obs_lists) * slots;
    }
    ro_pol_ra = q;
    RolloutCtx pc{};
    pc.s = s; pc.ra = q; pc.w = s;
    ro_pol_ctx.ensure(1);
    MFX_HIP_THROW(hipMemcpy(ro_pol_ctx.p, &pc, sizeof(RolloutCtx), hipMemcpyHostToDevice));
}

// Plan::Pipe: the grids of its two kernels, the twin state and the two contexts that trade places.
void BattleEngine::plan_twin() {
    MFX_HIP_THROW(rollout_grid(gp, s, ra.rowcap, 1, kPipeStepPerCu, &ro_grid));
    MFX_HIP_THROW(rollout_obs_grid(gp, s, ra.rowcap, kPipeObsPerCu, &ro_obs_grid));
    alloc_twin();
    ro_par = 0;
    ro_twin_host[0].s = s; ro_twin_host[0].ra = ra; ro_twin_host[0].w = twin_state();
    ro_twin_host[1].s = twin_state(); ro_twin_host[1].ra = ra; ro_twin_host[1].w = s;
    ro_twin_ctx.ensure(2);
    MFX_HIP_THROW(hipMemcpyAsync(ro_twin_ctx.p, ro_twin_host, sizeof(ro_twin_host), hipMemcpyHostToDevice,
                                 stream));
    if (!ro_str[0]) MFX_HIP_THROW(hipStreamCreateWithFlags(&ro_str[0], hipStreamNonBlocking));
    for (auto& x : ro_ev) if (!x) MFX_HIP_THROW(hipEventCreateWithFlags(&x, hipEventDisableTiming));
}

// Plan again when the state has moved since the plan (a new capacity, reallocated or swapped arrays).
int BattleEngine::replan_if_moved() {
    const State& planned = ro_plan == Plan::Pipe ? ro_twin_host[ro_par].s : ro_ctx_host.s;
    if (s.cap != ro_cap || memcmp(&planned, &s, sizeof(State)) != 0) MFX_CHECK(rollout_plan());
    return 0;
}

// The generic (non-Battle-shape) observation of batch q / qa into its rollout buffers, group by group.
int BattleEngine::observe_groups(const State& q, const RolloutArgs& qa, hipStream_t st) {
    for (int g = 0; g < n_groups(); g++)
        MFX_HIP(launch_observe(gp, d_gp, q, g, qa.rowcap, qa.view[g], qa.feat[g], qa.rowcap, st));
    return 0;
}

int BattleEngine::rollout_step(int n_steps) {
    MFX_CHECK(flush_deferred());
    touch();
    if (!rollout_ready) return fail("rollout_step before rollout_init");
    if (walls_after_init) return fail("rollout: walls added after rollout_init are not part of the rollout's episodes");
    MFX_CHECK(replan_if_moved());
    // after a learned policy's launches the queue kernel's filings, tags and parities (and the pipeline's item
    // lists) are out of date: re-seed
    if (ro_prep_form != 0) { ro_prep_stale = true; ro_prep_form = 0; }
    switch (ro_plan) {
        case Plan::Fused: return step_fused(n_steps);
        case Plan::Pipe: return step_pipe(n_steps);
        case Plan::BigStreams: return step_big_streams(n_steps);
        case Plan::BigQueue: return step_big_queue(n_steps);
        case Plan::FewPipe: return step_few_pipe(n_steps);
    }
    return 0;
}

// Plan::FewPipe
int BattleEngine::step_few_pipe(int n_steps) {
    // the pipelined few-env form: every launch files and observes its own items (parity 0, a fresh tag),
    // the steppers claimed per XCD; q_left must read 0 (no items outstanding) at a launch start
    MFX_CHECK(sync_cells());
    const size_t lst = (size_t)kXcds * kObsCntPad;
    if (ro_prep_stale) {
        ro_qlaunch++;
        MFX_HIP(hipMemsetAsync(ro_q_items.p, 0, ro_q_items.n * sizeof(uint32_t), stream));
        MFX_HIP(hipMemsetAsync(ro_q_done.p, 0, kObsCntPad * sizeof(int32_t), stream));
        MFX_HIP(hipMemsetAsync(ro_q_left.p, 0, (size_t)E * sizeof(int32_t), stream));
    }
    ro_prep_stale = false;
    for (int i = 0; i < n_steps;) {
        const int k = std::min(sub_steps(), n_steps - i);
        // a slot whose item its stepper took back keeps the stolen mark if no holder reached it before the
        // launch ended (k_rollout_bigq: bigq_wait / few_steal): clear the lists when the tag comes round
        if (qtag(ro_qlaunch) == 1)
            MFX_HIP(hipMemsetAsync(ro_q_items.p, 0, ro_q_items.n * sizeof(uint32_t), stream));
        // (both parities: parity 1 holds the per-XCD done counts, k_rollout_bigq xcd_done)
        MFX_HIP(hipMemsetAsync(ro_q_cnt.p, 0, 2 * lst * sizeof(int32_t), stream));
        MFX_HIP(hipMemsetAsync(ro_q_step.p, 0, kXcds * sizeof(int32_t), stream));
        // (no BigqSerial: the pipelined form completes with one workgroup of its grid per XCD, and its grid
        // -- one or two workgroups per CU, at most half of an XCD's slots -- never holds a whole XCD)
        MFX_HIP(launch_rollout_bigq(gp, d_gp, s, ro_ctx.p, ra.obs_item_rows, ra.step_index, k, 0,
                                    qtag(ro_qlaunch), qtag(ro_qlaunch + 1), ro_q_grid,
                                    ra.lds_step, stream, true));
        ro_qlaunch++;
        ro_launch++;
        ra.step_index += k;
        i += k;
    }
    return 0;
}

// Plan::BigQueue
int BattleEngine::step_big_queue(int n_steps) {
    MFX_CHECK(sync_cells());
    const size_t lst = (size_t)kXcds * kObsCntPad;           // counters of one parity
    if (ro_prep_stale) {
        // Re-seed after per-call calls: the last launch's filings for the next launch (never
        // consumed) still hold the live tag in the slots past the new, smaller filing count --
        // clear every slot and move to a fresh tag, so no stale word can pass for an item.
#ifndef MFX_AB_R2_RESEED                 // A/B only: the round-2 re-seed, which the regression test must catch
        MFX_HIP(hipMemsetAsync(ro_q_items.p, 0, ro_q_items.n * sizeof(uint32_t), stream));
#endif
        MFX_HIP(hipMemsetAsync(ro_q_cnt.p, 0, ro_q_cnt.n * sizeof(int32_t), stream));
        MFX_HIP(hipMemsetAsync(ro_q_done.p, 0, kObsCntPad * sizeof(int32_t), stream));
        for (int c = 0; c < ro_qchunks; ++c) {
            ro_qc_par[c] = 0;
#ifndef MFX_AB_R2_RESEED
            ro_qc_launch[c]++;
#endif
            MFX_HIP(launch_bigq_seed(d_gp, ro_qc_s[c], ro_qc_ra[c], 0, qtag(ro_qc_launch[c]), ra.step_index,
                                     stream));
        }
    }
    ro_prep_stale = false;
    // chunk after chunk, each through every launch of the n steps (the envs are independent; within a
    // chunk the launches chain as one batch's would)
    for (int c = 0; c < ro_qchunks; ++c) {
        int32_t* cnt = ro_q_cnt.p + (size_t)c * 2 * lst;
        uint32_t si = ra.step_index;
        for (int i = 0; i < n_steps;) {
            const int k = std::min(sub_steps(), n_steps - i);
            MFX_HIP(hipMemsetAsync(cnt + (ro_qc_par[c] ^ 1) * lst, 0, lst * sizeof(int32_t), stream));
            BigqSerial serial(stream);
            MFX_HIP(serial.status());
            MFX_HIP(launch_rollout_bigq(gp, d_gp, ro_qc_s[c], ro_qc_ctx.p + c, ra.obs_item_rows, si, k,
                                        ro_qc_par[c], qtag(ro_qc_launch[c]), qtag(ro_qc_launch[c] + 1),
                                        ro_q_grid, ra.lds_step, stream));
            ro_qc_par[c] ^= 1;
            ro_qc_launch[c]++;
            ro_launch++;
            si += k;
            i += k;
        }
    }
    ra.step_index += n_steps;
    return 0;
}

// Plan::BigStreams
int BattleEngine::step_big_streams(int n_steps) {
    MFX_CHECK(sync_cells());
    const int K = std::min(ro_split, E);
    if (ra.obs_mm && ro_prep_stale) {
        if (ra.obs_items)
            MFX_HIP(hipMemsetAsync(ro_cnt.p, 0, sizeof(int32_t) * 2 * kXcds * kObsCntPad * kMaxSplit, stream));
        for (int k = 0; k < K; k++)
            MFX_HIP(launch_obs_prep(d_gp, ro_sub_s[k], ro_sub_ra[k], (int)(ra.step_index & 1), stream));
    }
    ro_prep_stale = false;
    // fork: every sub-batch stream waits for the caller's stream, the caller joins them all
    MFX_HIP(hipEventRecord(ro_ev[kMaxSplit], stream));
    for (int k = 0; k < K; k++) MFX_HIP(hipStreamWaitEvent(ro_str[k], ro_ev[kMaxSplit], 0));
    for (int i = 0; i < n_steps; i++) {
        for (int k = 0; k < K; k++) {
            const State& q = ro_sub_s[k];
            const RolloutArgs& qa = ro_sub_ra[k];
            if (qa.obs_items) {
                MFX_HIP(launch_observe_items(gp, d_gp, q, qa, (int)(ra.step_index & 1), ro_item_grid,
                                             ro_str[k]));
            } else {                           // generic (non-Battle-shape) observation
                MFX_CHECK(observe_groups(q, qa, ro_str[k]));
            }
            MFX_HIP(launch_rollout_big(gp, d_gp, q, ro_sub_ctx.p + k, ra.step_index, ra.lds_step, ro_str[k]));
        }
        ro_launch++;
        ra.step_index++;
    }
    for (int k = 0; k < K; k++) {
        MFX_HIP(hipEventRecord(ro_ev[k], ro_str[k]));
        MFX_HIP(hipStreamWaitEvent(stream, ro_ev[k], 0));
    }
    return 0;
}

// Plan::Pipe
int BattleEngine::step_pipe(int n_steps) {
    for (int i = 0; i < n_steps; i++) {
        const RolloutCtx* c = ro_twin_ctx.p + ro_par;
        const int qp = (int)(ro_launch % 6);
        MFX_HIP(hipEventRecord(ro_ev[kMaxSplit], stream));
        MFX_HIP(hipStreamWaitEvent(ro_str[0], ro_ev[kMaxSplit], 0));
        MFX_HIP(launch_rollout_obs(gp, d_gp, s, c, ra.rowcap, ra.work_sel, qp, ro_obs_grid, ro_str[0]));
        MFX_HIP(launch_rollout(gp, d_gp, s, c, ra.rowcap, ra.step_index, ra.work_sel, qp, ro_grid, 1, 1, stream));
        MFX_HIP(hipEventRecord(ro_ev[0], ro_str[0]));
        MFX_HIP(hipStreamWaitEvent(stream, ro_ev[0], 0));
        swap_twin();                     // the written copy is the state now
        ro_par ^= 1;
        ro_launch++;
        ra.step_index++;
        ra.work_sel ^= 1;
        cells_stale = true;
    }
    return 0;
}

// Plan::Fused
int BattleEngine::step_fused(int n_steps) {
    for (int i = 0; i < n_steps;) {
        const int k = std::min(sub_steps(), n_steps - i);
        MFX_HIP(launch_rollout(gp, d_gp, s, ro_ctx.p, ra.rowcap, ra.step_index, ra.work_sel, (int)(ro_launch % 6),
                               ro_grid, 0, k, stream));
        ro_launch++;
        ra.step_index += k;
        ra.work_sel ^= 1;
        cells_stale = true;
        i += k;
    }
    return 0;
}

// A learned policy's launches (include/magent_amd.h mfx_battle_rollout_policy_step): mode 2 observes every
// env into the rollout buffers; mode 1 acts with the actions in the rollout's action buffer (the
// policy's forward on that observation), steps, and observes the new state.  LDS-sized envs in large batches:
// the fused k_rollout (kMode).  Every plan with the state in HBM (plan_hbm(): large envs, few LDS-sized envs, pipelined or not,
// MFX_BIG_FUSED=0): k_rollout_big<ext> + k_observe_items on the engine's stream (rollout_policy_big).
int BattleEngine::rollout_policy_step(int mode) {
    MFX_CHECK(flush_deferred());
    touch();
    if (!rollout_ready) return fail("rollout_policy_step before rollout_init");
    if (mode != 1 && mode != 2) return fail("rollout_policy_step: mode %d (1 step, 2 observe)", mode);
    if (walls_after_init) return fail("rollout: walls added after rollout_init are not part of the rollout's episodes");
    MFX_CHECK(replan_if_moved());
    if (plan_hbm()) return rollout_policy_big(mode);
    if (ro_plan == Plan::Pipe)
        return fail("rollout_policy_step: a learned policy does not step on the observation/step pipeline "
                    "(MFX_ROLLOUT_PIPE=1); unset it");
    MFX_HIP(launch_rollout_mode(gp, d_gp, s, ro_ctx.p, ra.rowcap, ra.step_index, ra.work_sel, (int)(ro_launch % 6),
                                ro_grid, mode, stream));
    ro_launch++;
    if (mode == 1) ra.step_index++;
    ra.work_sel ^= 1;
    cells_stale = true;
    return 0;
}

// The policy form of the large-env plans.  The observation of step t reads the item lists of parity t & 1:
// mode 2 files them itself (k_obs_prep, after clearing both parities' counters: a drained list's tickets are
// spent, and after a rollout_step the lists hold the other form's items); mode 1's k_rollout_big<ext> files
// parity (t + 1) & 1 for the observation that follows it, whose workgroup 0 clears parity t & 1 for the step
// after.  Everything runs on the engine's stream, in order.
int BattleEngine::rollout_policy_big(int mode) {
    MFX_CHECK(sync_cells());
    const bool items = ro_pol_ra.obs_items != nullptr;
    auto observe = [&](int par) -> int {
        if (items) {
            MFX_HIP(launch_observe_items(gp, d_gp, s, ro_pol_ra, par, ro_pol_item_grid, stream));
        } else {                                   // generic (non-Battle-shape) observation
            MFX_CHECK(observe_groups(s, ro_pol_ra, stream));
        }
        return 0;
    };
    if (mode == 2) {
        if (items) {
            MFX_HIP(hipMemsetAsync(ro_cnt.p, 0, sizeof(int32_t) * ro_cnt.n, stream));
            MFX_HIP(launch_obs_prep(d_gp, s, ro_pol_ra, (int)(ra.step_index & 1), stream));
        }
        MFX_CHECK(observe((int)(ra.step_index & 1)));
    } else {
        if (ro_prep_stale || ro_prep_form != 1)
            return fail("rollout_policy_step: observe first (mode 2) after rollout_init, rollout_step or a per-call "
                        "call: the action buffer must follow the current observation");
        MFX_HIP(launch_rollout_big(gp, d_gp, s, ro_pol_ctx.p, ra.step_index, ra.lds_step, stream, true));
        ra.step_index++;
        MFX_CHECK(observe((int)(ra.step_index & 1)));
    }
    ro_launch++;
    ro_prep_stale = false;
    ro_prep_form = 1;
    return 0;
}

// Which kernels rollout_policy_step runs (include/magent_amd.h mfx_battle_rollout_policy_path).
int BattleEngine::rollout_policy_path() const {
    if (!rollout_ready || ro_plan == Plan::Pipe) return -1;
    return plan_hbm() ? 2 : 0;
}

// Synchronise and report the device error word and, on the queue-driven large-env kernel, its queue
// error word: 0 if neither is set.
int BattleEngine::rollout_check() {
    if (!rollout_ready) return fail("rollout_check before rollout_init");
    if (plan_queue()) {
        int32_t w[kObsCntPad] = {};
        MFX_HIP(hipMemcpyAsync(w, ro_q_done.p, sizeof(w), hipMemcpyDeviceToHost, stream));
        MFX_HIP(hipStreamSynchronize(stream));
        static const char* msg[] = {"", "", "a wait without progress (stalled queue)", "a ticket past the list",
                                    "a workgroup outside XCDs 0-7 (not one SPX device)",
                                    "hand-off guard: an item saw a step counter other than its own"};
        if (w[2]) return fail("rollout: k_rollout_bigq error %d: %s", w[2], w[2] > 0 && w[2] < 6 ? msg[w[2]] : "?");
    }
    return check_err();
}

// Which kernels rollout_step runs (include/magent_amd.h mfx_battle_rollout_path).
int BattleEngine::rollout_path() const {
    if (!rollout_ready) return -1;
    switch (ro_plan) {
        case Plan::Fused: return 0;
        case Plan::Pipe: return 1;
        case Plan::BigStreams: return 2;
        case Plan::BigQueue: case Plan::FewPipe: return 3;
    }
    return -1;
}

// Steps per launch: ro_sub, or with ro_sub 0 (mfx_battle_rollout_set_substeps(game, 0)) the measured best of the
// path (profiles/r04_substeps_auto.txt, one MI355X): the pipelined few-env stepper kMaxPipeSub -- a launch ends
// with its slowest env's steps (the envs step independently inside it), and a longer launch averages each env's
// heavy early-episode steps with its light ones: 8 envs 0.0356 -> 0.0285 ms per step from 20 to 64 steps per
// launch --, in practice the whole rollout_step(n) as one launch; k_rollout below 96 envs per CU 2 (its workgroups'
// heaviest units end the launch: 8192 envs 0.556 -> 0.594 of peak, 16384 0.62 -> 0.63), else 20 (32768
// envs 0.75 at 5, 0.77 at 20; the bench's 131072, 0.84-0.86); the large-env queue kernel 20.
int BattleEngine::sub_steps() const {
    // (one step per launch: the two-kernel observation / step pipeline and the large-env two-stream pipeline --
    // rollout_step launches those per step whatever ro_sub says)
    if (ro_plan == Plan::Pipe || ro_plan == Plan::BigStreams) return 1;
    const bool pipe = ro_plan == Plan::FewPipe;
    if (ro_sub > 0) return std::min(ro_sub, pipe ? kMaxPipeSub : kMaxSub);
    if (plan_hbm()) return pipe ? kMaxPipeSub : 20;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        cus = 256;
    return E < 96 * cus ? 2 : 20;
}

// Lanes over which the rollout sums a group's rewards of an env with n agents (the order the episode
// returns follow): k_rollout's wave 0 up to 64 agents, else its workgroup; the step of the large-env
// and few-env queue paths (big_env_step) 512 lanes; the pipelined few-env stepper (few_env_step) k_rollout's
// team forms: wave 0 up to 64 agents, else its 512-lane workgroup.
int BattleEngine::rollout_sum_lanes(int n) const {
    if (!rollout_ready) return -1;
    if (ro_plan == Plan::FewPipe) return n <= ra.few_wave_max ? 64 : 512;
    if (plan_hbm()) return 512;                       // kBigRolloutThreads (battle/rollout_big.inc)
    return n <= 64 ? 64 : 256;
}

int BattleEngine::rollout_info(int* grid, int* lds_bytes) {
    if (!rollout_ready) return fail("rollout_info before rollout_init");
    *grid = ro_grid;
    *lds_bytes = (int)(plan_hbm() ? big_step_smem_bytes(gp, s.cap, s.acap, true, ra.lds_step)
                              : rollout_smem_bytes(gp, s.cells_n, s.cap, s.acap, ra.rowcap));
    return 0;
}

int BattleEngine::rollout_buffer(const char* name, int group, void** ptr, size_t* bytes) {
    if (!rollout_ready) return fail("rollout_buffer before rollout_init");
    const int G = n_groups();
    if (group < 0 || group >= G) return fail("bad group");
    const TypeParams& T = gp.type[group];
    const size_t rc = ra.rowcap;
    if (!strcmp(name, "view")) { *ptr = ra.view[group]; *bytes = E * rc * T.view_w * T.view_h * gp.n_ch * 4; }
    else if (!strcmp(name, "feature")) { *ptr = ra.feat[group]; *bytes = E * rc * gp.feat_size[group] * 4; }
    else if (!strcmp(name, "actions")) { *ptr = ra.actions; *bytes = (size_t)E * G * rc * 4; }
    else if (!strcmp(name, "rewards")) { *ptr = ra.rewards; *bytes = (size_t)E * G * rc * 4; }
    else if (!strcmp(name, "ids")) { *ptr = ra.ids; *bytes = (size_t)E * G * rc * 4; }
    else if (!strcmp(name, "alive")) { *ptr = ra.alive; *bytes = (size_t)E * G * rc; }
    else if (!strcmp(name, "mean_action")) { *ptr = ra.mean_act; *bytes = ro_mean.n * 8; }
    else if (!strcmp(name, "episode_return")) { *ptr = ra.ep_return; *bytes = (size_t)E * G * 4; }
    else if (!strcmp(name, "stats")) { *ptr = ra.stats; *bytes = (size_t)E * 4 * 8; }
    else if (!strcmp(name, "agent_steps")) { *ptr = ra.agent_steps; *bytes = (size_t)E * 8; }
    else if (!strcmp(name, "group_num")) { *ptr = s.grp_n; *bytes = (size_t)E * G * 4; }
    else if (!strcmp(name, "rng")) { *ptr = s.rng; *bytes = (size_t)E * 4; }   // the envs' shuffle engines (minstd states)
    else return fail("unknown rollout buffer %s", name);
    return 0;
}

}  // namespace mfx
