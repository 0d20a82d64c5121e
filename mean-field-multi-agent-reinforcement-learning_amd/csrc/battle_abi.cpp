// battle_abi.cpp -- the C ABI of the Battle engine: the reference's env_* / gridworld_* calls (env 0, host buffers)
// and the batched device API mfx_battle_* (include/magent_amd.h).
#include "battle_engine.h"

using mfx::BattleEngine;

// ============================================================================ C ABI
#define MFX_ENV(h) static_cast<BattleEngine*>(h)
#define MFX_GUARD(expr)                                                          \
    try {                                                                        \
        return (expr);                                                           \
    } catch (const std::exception& ex) {                                         \
        return mfx::fail("%s", ex.what());                                       \
    }

extern "C" {

// ---- reference runtime_api.h:118-181 ------------------------------------------------
MFX_API int env_new_game(void** game, const char* name) {
    if (strcmp(name, "GridWorld") != 0) return mfx::fail("invalid name of game: %s", name);
    MFX_GUARD((*game = new BattleEngine(), 0));
}
MFX_API int env_delete_game(void* game) { delete MFX_ENV(game); return 0; }
MFX_API int env_config_game(void* game, const char* name, void* value) { MFX_GUARD(MFX_ENV(game)->set_config(name, value)); }
MFX_API int env_reset(void* game) { MFX_GUARD(MFX_ENV(game)->reset()); }
MFX_API int env_get_observation(void* game, int group, float** buffer) { MFX_GUARD(MFX_ENV(game)->host_observe(group, buffer)); }
// get_observation without the copy (the drop-in fast step): pointers to env 0's observation of the
// group in engine-owned pinned memory (n rows of blocks of `rows`), valid until the step after next or
// the engine's deletion.  Returns 1 when the observation is not held that way (use env_get_observation).
MFX_API int mfx_env_observation_view(void* game, int group, float** view, float** feature, int* n, int* rows) {
    MFX_GUARD(MFX_ENV(game)->observation_view(group, view, feature, n, rows));
}
MFX_API int env_set_action(void* game, int group, const int* actions) { MFX_GUARD(MFX_ENV(game)->host_set_action(group, actions)); }
MFX_API int env_step(void* game, int* done) { MFX_GUARD(MFX_ENV(game)->host_step(done)); }
MFX_API int env_get_reward(void* game, int group, float* buffer) {
    MFX_GUARD(MFX_ENV(game)->host_get(group, mfx::kGetReward, buffer, 4));
}
MFX_API int env_get_info(void* game, int group, const char* name, void* buffer) {
    MFX_GUARD(MFX_ENV(game)->get_info_global(group, name, buffer));
}
// The drop-in wrapper's getters in one FFI call each where the reference's wrapper makes two
// (gridworld.py get_agent_id / get_reward / get_alive / get_pos: env_get_info("num"), then env_get_info(name) or
// env_get_reward): returns the group's size n and, when n <= cap, copies its n rows of field `what` (0 id int32,
// 1 reward float32, 2 alive uint8, 3 pos int32 pairs; -1: the size only) into out.  -1 on error.
MFX_API int mfx_env_get_rows(void* game, int group, int what, void* out, int cap) {
    MFX_GUARD(MFX_ENV(game)->get_rows(group, what, out, cap));
}
MFX_API int env_render(void* game) { MFX_GUARD(MFX_ENV(game)->render()); }
MFX_API int env_render_next_file(void* game) { MFX_GUARD((MFX_ENV(game)->next_file(), 0)); }

MFX_API int gridworld_register_agent_type(void* game, const char* name, int n, const char** keys, float* values) {
    MFX_GUARD(MFX_ENV(game)->register_type(name, n, keys, values));
}
MFX_API int gridworld_new_group(void* game, const char* agent_type_name, int* group) {
    MFX_GUARD(MFX_ENV(game)->new_group(agent_type_name, group));
}
MFX_API int gridworld_add_agents(void* game, int group, int n, const char* method, const int* pos_x, const int* pos_y,
                                 const int* dir) {
    MFX_GUARD(MFX_ENV(game)->add_agents(group, n, method, pos_x, pos_y, dir));
}
MFX_API int gridworld_clear_dead(void* game) { MFX_GUARD(MFX_ENV(game)->host_clear_dead()); }
MFX_API int gridworld_set_goal(void* game, int group, const char* method, const int* linear_buffer) {
    (void)linear_buffer;
    MFX_GUARD(MFX_ENV(game)->set_goal(group, method));
}
MFX_API int gridworld_define_agent_symbol(void* game, int no, int group, int index) {
    BattleEngine* e = MFX_ENV(game);
    if (no < 0) return mfx::fail("bad symbol number");
    if ((size_t)no >= e->syms.size()) e->syms.resize(no + 1);
    e->syms[no] = {group, index};
    return 0;
}
MFX_API int gridworld_define_event_node(void* game, int no, int op, int* inputs, int n_inputs) {
    BattleEngine* e = MFX_ENV(game);
    if (no < 0) return mfx::fail("bad event node number");
    if ((size_t)no >= e->nodes.size()) e->nodes.resize(no + 1);
    e->nodes[no].op = op;
    e->nodes[no].raw.assign(inputs, inputs + n_inputs);
    return 0;
}
// The reference python passes only 6 of these 7 arguments (gridworld.py:719-722);
// auto_value is never read (it only matters for OP_ALIGN, RewardEngine.cc:252).
MFX_API int gridworld_add_reward_rule(void* game, int on, int* receiver, float* value, int n_receiver, bool is_terminal,
                                      bool auto_value) {
    (void)auto_value;
    BattleEngine* e = MFX_ENV(game);
    BattleEngine::Rule r;
    r.on = on;
    r.recv.assign(receiver, receiver + n_receiver);
    r.val.assign(value, value + n_receiver);
    r.terminal = is_terminal;
    e->rules.push_back(std::move(r));
    return 0;
}

// ---- batched device API (include/magent_amd.h) ---------------------------------------
MFX_API int mfx_battle_set_num_envs(void* game, int n_envs) {
    BattleEngine* e = MFX_ENV(game);
    if (e->allocated) return mfx::fail("set_num_envs must precede the first reset");
    if (n_envs < 1) return mfx::fail("n_envs must be >= 1");
    e->E = n_envs;
    return 0;
}
MFX_API int mfx_battle_set_stream(void* game, void* stream) {
    BattleEngine* e = MFX_ENV(game);
    MFX_CHECK(e->quiesce());
    if (e->own_stream && e->stream) { (void)hipStreamSynchronize(e->stream); (void)hipStreamDestroy(e->stream); }
    e->stream = (hipStream_t)stream;
    e->own_stream = false;
    e->stream_set = true;
    return 0;
}
MFX_API int mfx_battle_observe(void* game, int group, float* d_view, float* d_feature, int rowcap) {
    MFX_GUARD(MFX_ENV(game)->observe(group, d_view, d_feature, rowcap));
}
MFX_API int mfx_battle_set_action(void* game, int group, const int* d_actions, int rowcap) {
    MFX_GUARD(MFX_ENV(game)->set_action(group, d_actions, rowcap));
}
MFX_API int mfx_battle_step(void* game, int* d_done) { MFX_GUARD(MFX_ENV(game)->step(d_done)); }
MFX_API int mfx_battle_get(void* game, int group, int what, void* d_out, int rowcap) {
    MFX_GUARD(MFX_ENV(game)->get(group, what, d_out, rowcap));
}
MFX_API int mfx_battle_clear_dead(void* game) { MFX_GUARD(MFX_ENV(game)->clear_dead()); }
MFX_API int mfx_battle_sync(void* game) {
    BattleEngine* e = MFX_ENV(game);
    if (!e->allocated) return 0;
    MFX_CHECK(e->quiesce());
    MFX_HIP(hipStreamSynchronize(e->stream));
    return e->check_err();
}
MFX_API int mfx_battle_rollout_init(void* game, const int* tmpl_n, const int* const* xs, const int* const* ys,
                                    int max_steps, float eps, unsigned seed, int stagger) {
    MFX_GUARD(MFX_ENV(game)->rollout_init(tmpl_n, xs, ys, max_steps, eps, seed, stagger));
}
MFX_API int mfx_battle_rollout_step(void* game, int n_steps) { MFX_GUARD(MFX_ENV(game)->rollout_step(n_steps)); }
MFX_API int mfx_battle_rollout_buffer(void* game, const char* name, int group, void** ptr, size_t* bytes) {
    MFX_GUARD(MFX_ENV(game)->rollout_buffer(name, group, ptr, bytes));
}
// Copy a rollout buffer (see rollout_buffer names) to dst (host or device pointer),
// asynchronously on the engine stream; `bytes` may be smaller than the buffer.
MFX_API int mfx_battle_rollout_copy(void* game, const char* name, int group, void* dst, size_t bytes) {
    BattleEngine* e = MFX_ENV(game);
    void* src = nullptr;
    size_t n = 0;
    MFX_CHECK(e->rollout_buffer(name, group, &src, &n));
    if (bytes > n) return mfx::fail("rollout_copy: %zu bytes requested, buffer has %zu", bytes, n);
    MFX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, e->stream));
    return 0;
}
// The same for bytes [offset, offset + bytes) of the buffer (e.g. one env's rows).
MFX_API int mfx_battle_rollout_copy_at(void* game, const char* name, int group, size_t offset, void* dst, size_t bytes) {
    BattleEngine* e = MFX_ENV(game);
    void* src = nullptr;
    size_t n = 0;
    MFX_CHECK(e->rollout_buffer(name, group, &src, &n));
    if (offset > n || bytes > n - offset)
        return mfx::fail("rollout_copy_at: bytes [%zu, %zu) outside the buffer (%zu)", offset, offset + bytes, n);
    MFX_HIP(hipMemcpyAsync(dst, static_cast<const char*>(src) + offset, bytes, hipMemcpyDefault, e->stream));
    return 0;
}
// The inverse, for the buffers a caller supplies: "actions" (a policy's actions for mfx_battle_rollout_policy_step).
MFX_API int mfx_battle_rollout_write(void* game, const char* name, int group, const void* src, size_t bytes) {
    BattleEngine* e = MFX_ENV(game);
    if (strcmp(name, "actions") != 0) return mfx::fail("rollout_write: buffer %s is not writable (only actions)", name);
    void* dst = nullptr;
    size_t n = 0;
    MFX_CHECK(e->rollout_buffer(name, group, &dst, &n));
    if (bytes > n) return mfx::fail("rollout_write: %zu bytes given, buffer has %zu", bytes, n);
    MFX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, e->stream));
    return 0;
}
// Diagnostic build only: route k_rollout phase stamps ([E][16] u64 s_memtime) to d_buf.
MFX_API int mfx_battle_set_stamp_buffer(void* d_buf) {
    MFX_HIP(mfx::set_stamp_buffer((unsigned long long*)d_buf));
    return 0;
}
// Launch geometry of the fused rollout: persistent grid (workgroups) and LDS bytes per workgroup.
MFX_API int mfx_battle_rollout_info(void* game, int* grid, int* lds_bytes) {
    MFX_GUARD(MFX_ENV(game)->rollout_info(grid, lds_bytes));
}

// Synchronise; -1 and the message if a device error was raised or (k_rollout_bigq) the in-launch work
// queue reported an error.
MFX_API int mfx_battle_rollout_check(void* game) {
    MFX_GUARD(MFX_ENV(game)->rollout_check());
}
// A learned policy's launches: mode 2 observes every env, mode 1 acts with the action buffer, steps, observes.
MFX_API int mfx_battle_rollout_policy_step(void* game, int mode) {
    MFX_GUARD(MFX_ENV(game)->rollout_policy_step(mode));
}
// The kernels rollout_policy_step runs, numbered like mfx_battle_rollout_path: 0 k_rollout, 2 k_observe_items +
// k_rollout_big; -1: the plan refuses a learned policy (MFX_ROLLOUT_PIPE=1).
MFX_API int mfx_battle_rollout_policy_path(void* game, int* path) {
    if (!MFX_ENV(game)->has_rollout()) return mfx::fail("rollout_policy_path before rollout_init");
    *path = MFX_ENV(game)->rollout_policy_path();
    return 0;
}
// The kernels rollout_step runs: 0 k_rollout, 1 k_rollout_obs + k_rollout (pipeline), 2 k_observe_items +
// k_rollout_big (large-env pipeline), 3 k_rollout_bigq.
MFX_API int mfx_battle_rollout_path(void* game, int* path) {
    const int p = MFX_ENV(game)->rollout_path();
    if (p < 0) return mfx::fail("rollout_path before rollout_init");
    *path = p;
    return 0;
}

// Lanes over which the rollout sums a group's rewards of an env with n_agents agents (the summation order
// the episode returns follow; the oracle replay restates it).
MFX_API int mfx_battle_rollout_sum_lanes(void* game, int n_agents, int* lanes) {
    const int l = MFX_ENV(game)->rollout_sum_lanes(n_agents);
    if (l < 0) return mfx::fail("rollout_sum_lanes before rollout_init");
    *lanes = l;
    return 0;
}

// Steps per k_rollout launch (1..64; up to 1024 on the pipelined few-env path, the others run 64 at most): every
// env runs that many consecutive steps while its image stays
// in LDS; the large-env queue kernel k_rollout_bigq runs that many steps of every env per launch (its
// item lists hold one filing per env and step of a launch: lcap in rollout_plan, hence <= 64).
// rollout_step(n) results are identical for any value (the last step's buffers, the same state); only
// the launch count changes.  Ignored by the two pipelines (one step per launch).  0: chosen per path and batch
// (BattleEnv::sub_steps); mfx_battle_rollout_get_substeps reports the value in force.
MFX_API int mfx_battle_rollout_set_substeps(void* game, int n_sub) {
    if (n_sub < 0 || n_sub > 1024) return mfx::fail("rollout_set_substeps: %d not in 0..1024", n_sub);
    MFX_ENV(game)->set_sub_steps(n_sub);
    return 0;
}

MFX_API int mfx_battle_rollout_get_substeps(void* game, int* n_sub) {
    if (!MFX_ENV(game)->has_rollout()) return mfx::fail("rollout_get_substeps before rollout_init");
    *n_sub = MFX_ENV(game)->sub_steps();
    return 0;
}

MFX_API int mfx_battle_rollout_rowcap(void* game, int* rowcap) {
    *rowcap = MFX_ENV(game)->rollout_rowcap();
    return 0;
}
MFX_API int mfx_battle_rollout_mean_stride(void* game, int* stride) {
    *stride = MFX_ENV(game)->rollout_mean_stride();
    return 0;
}
// The inputs of group g's observation view that can be non-zero (Map::extract_view, Map.cc:130-218): every channel
// of a cell inside the view range, only the minimap channels (group2channel(k) + 2, GridWorld.cc:396-409) of a cell
// outside it.  mask[n], n = view_h * view_w * n_ch (the view's NHWC order): 1 = may be non-zero, 0 = always 0.
MFX_API int mfx_battle_view_support(void* game, int group, uint8_t* mask, int n) {
    BattleEngine* e = MFX_ENV(game);
    if (group < 0 || group >= e->n_groups()) return mfx::fail("view_support: bad group");
    if (!e->allocated) {                     // (once allocated, gp is the parameter set the device runs on)
        try {
            MFX_CHECK(e->build_params());
        } catch (const std::exception& ex) {
            return mfx::fail("%s", ex.what());
        }
    }
    const mfx::TypeParams& T = e->gp.type[group];
    const int NC = e->gp.n_ch, cells = T.view_w * T.view_h;
    if (n != cells * NC) return mfx::fail("view_support: %d entries, the view has %d", n, cells * NC);
    for (int c = 0; c < cells; c++)
        for (int ch = 0; ch < NC; ch++) {
            bool mm = false;
            for (int k = 0; e->minimap && k < e->n_groups(); k++) mm = mm || ch == e->group2channel(k) + 2;
            mask[c * NC + ch] = (uint8_t)(T.view_mask[c] || mm);
        }
    return 0;
}
MFX_API int mfx_battle_group_capacity(void* game, int group, int* cap) {
    BattleEngine* e = MFX_ENV(game);
    if (group < 0 || group >= e->n_groups()) return mfx::fail("bad group");
    *cap = e->allocated ? e->group_ub[group] : 0;
    return 0;
}

}  // extern "C"

