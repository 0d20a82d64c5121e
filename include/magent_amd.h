/*
 * magent_amd.h -- C ABI of the MI355X-native Battle / Ising mean-field engine (libmagent.so).
 *
 * Part 1 is the reference's own ABI, symbol for symbol: the 18 GridWorld entry points of
 * examples/battle_model/src/runtime_api.h:20-55 (implemented at runtime_api.cc:15-169), so
 * the reference python wrapper examples/battle_model/python/magent/gridworld.py (ctypes, no
 * argtypes) and c_lib.py:13-31 bind this library unchanged.  Those calls act on env 0 and move
 * data through caller-owned host buffers, exactly like the reference.  On one env whose config the
 * fused kernels take, set_action and clear_dead are deferred and env_step is one request to a
 * resident k_dropin_step workgroup (a mailbox in coherent host memory; MFX_DROPIN_RESIDENT=0: one
 * launch per step) that also leaves the getters' record and the next observation in pinned memory;
 * any other call first stops the server and runs the deferred work (MFX_DROPIN_FAST=0: one launch
 * per call).
 *
 * Part 2 is this library's batched device API: E envs per engine, every buffer in HBM.
 * Part 3 covers the Ising lattice / tabular MF-Q (the reference's examples/ising_model and
 * main_MFQ_Ising.py are pure python; there is no reference ABI to mirror).
 * Part 4 covers the mean-field training-loop kernels.
 *
 * Conventions: every function returns 0 on success and -1 on failure (message on stderr and in
 * mfx_last_error()); the reference returns 0 and aborts on fatal errors instead.  "d_" pointers
 * are device pointers, the others host pointers.  Streams are hipStream_t passed as void*.
 */
#ifndef MAGENT_AMD_H
#define MAGENT_AMD_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- part 1: reference ABI */
/* runtime_api.h:20 env_new_game -- name must be "GridWorld" (DiscreteSnake is out of scope) */
int env_new_game(void **game, const char *name);
/* runtime_api.h:21 */
int env_delete_game(void *game);
/* runtime_api.h:22 -- keys of GridWorld::set_config (GridWorld.cc:126-155): map_width,
 * map_height (int*), minimap_mode, food_mode, turn_mode, goal_mode (bool*), embedding_size (int*),
 * render_dir (char*), seed (int*) -- every key the reference accepts */
int env_config_game(void *game, const char *key, void *value);
/* runtime_api.h:25 */
int env_reset(void *game);
/* runtime_api.h:26 -- bufs[0] = float[n][view_h][view_w][n_ch], bufs[1] = float[n][feature] */
int env_get_observation(void *game, int group, float **bufs);
/* runtime_api.h:27 -- actions int32[n] in group-vector order */
int env_set_action(void *game, int group, const int *actions);
/* runtime_api.h:28 */
int env_step(void *game, int *done);
/* runtime_api.h:29 -- float[n] */
int env_get_reward(void *game, int group, float *buffer);
/* runtime_api.h:32 -- num, id, pos, alive, action_space, view_space, feature_space,
 * view2attack, attack_base, both_attack, global_minimap, mean_info, walls_info,
 * render_window_info, attack_event, groups_info (GridWorld.cc:777-978); and one name the reference lacks,
 * move_delta: int32 [n_move][2], the (dx, dy) of move action a (the scripted opponent's table, mfx_rule_create) */
int env_get_info(void *game, int group, const char *name, void *buffer);
/* runtime_api.h:35-36 -- RenderGenerator's frame files: config.json + video_<n>.txt of env 0
 * (RenderGenerator.cc), byte-identical to the reference build's; only the websocket server and the
 * JS viewer are out of scope */
int env_render(void *game);
int env_render_next_file(void *game);
/* runtime_api.h:42 -- AgentType reflection keys (AgentType.cc:63-101) */
int gridworld_register_agent_type(void *game, const char *name, int n, const char **keys, float *values);
/* runtime_api.h:43 */
int gridworld_new_group(void *game, const char *agent_type_name, int *group);
/* runtime_api.h:44-45 -- method "custom" | "random" | "fill"; group -1 = walls */
int gridworld_add_agents(void *game, int group, int n, const char *method, const int *pos_x, const int *pos_y,
                         const int *dir);
/* runtime_api.h:48 */
int gridworld_clear_dead(void *game);
/* runtime_api.h:49 -- "random" only (GridWorld.cc:729-740): advances the engine LCG like the
 * reference, goals are never read back */
int gridworld_set_goal(void *game, int group, const char *method, const int *linear_buffer);
/* runtime_api.h:52-55 -- the full reward DSL (RewardEngine.cc:14-443): and / or / not over
 * attack / kill / collide / at / in / die / in_a_line events, 'any' / 'all' / fixed-index symbols,
 * group receivers, terminal rules.  Rules of the one-event attack/kill/collide form run
 * data-parallel, the rest through a one-lane interpreter; 'align' fails loudly (the reference
 * never fills the counters it reads).  The reference python passes 6 arguments to the
 * 7-parameter add_reward_rule; auto_value is never read (RewardEngine.cc:252, OP_ALIGN only). */
int gridworld_define_agent_symbol(void *game, int no, int group, int index);
int gridworld_define_event_node(void *game, int no, int op, int *inputs, int n_inputs);
int gridworld_add_reward_rule(void *game, int on, int *receiver, float *value, int n_receiver, bool is_terminal,
                              bool auto_value);
/* Extension of env_get_observation (runtime_api.h:26) for the drop-in python: the same views and
 * features of env 0 (n agents), as pointers into engine-owned pinned memory the drop-in step wrote
 * them to (no copy), in blocks of `rows` agents that stay at those addresses until the group
 * outgrows them; valid until the step after next or env_delete_game.  Returns 1 (nothing set) when
 * the observation is not held that way -- call env_get_observation then. */
int mfx_env_observation_view(void *game, int group, float **view, float **feature, int *n, int *rows);
/* Extension of env_get_info("num") + env_get_info("id" / "alive" / "pos") / env_get_reward (runtime_api.h:29, :32)
 * for the drop-in python: one call per getter.  Returns the group's agent count n and, when n <= cap, copies
 * its n rows of field `what` (0 id int32, 1 reward float32, 2 alive uint8, 3 pos int32 x 2; -1: the count only)
 * into out; -1 on error. */
int mfx_env_get_rows(void *game, int group, int what, void *out, int cap);

/* ---------------------------------------------------------------- part 2: batched Battle */
/* Before the first env_reset: make the engine hold n_envs identical envs. */
int mfx_battle_set_num_envs(void *game, int n_envs);
/* Launch everything on this hipStream_t (may be the null stream). */
int mfx_battle_set_stream(void *game, void *stream);
/* Per-call API on device buffers; per-agent arrays are [E][rowcap][...]. */
int mfx_battle_observe(void *game, int group, float *d_view, float *d_feature, int rowcap);
int mfx_battle_set_action(void *game, int group, const int *d_actions, int rowcap);
int mfx_battle_step(void *game, int *d_done);
/* what: 0 num ([E]), 1 reward (f32), 2 id (i32), 3 alive (u8), 4 pos (i32 x2), 5 hp (f32) */
int mfx_battle_get(void *game, int group, int what, void *d_out, int rowcap);
int mfx_battle_clear_dead(void *game);
/* Wait for the stream and report any device-side error (capacity, bad action, ...). */
int mfx_battle_sync(void *game);
/* Upper bound of a group's size (rows needed per env). */
int mfx_battle_group_capacity(void *game, int group, int *cap);
/* Fused rollout: one launch per training-loop step for all envs (obs for every group, on-device
 * rush policy, set_action, step, reward, mean action, clear_dead, restart at done / max_steps).
 * tmpl_n[G], xs[G][tmpl_n[g]], ys[...]: placement re-applied at every episode start. */
int mfx_battle_rollout_init(void *game, const int *tmpl_n, const int *const *xs, const int *const *ys,
                            int max_steps, float eps, unsigned seed, int stagger);
int mfx_battle_rollout_step(void *game, int n_steps);
/* Steps per launch (1..64, up to 1024 on the pipelined few-env path; default 1; 0 = chosen per path and batch
 * size): k_rollout runs each env's steps
 * back to back with its image resident in LDS; the large-env queue kernel (k_rollout_bigq) runs every env's
 * steps in one launch.  rollout_step(n) gives identical results for every value.  get: the value in force. */
int mfx_battle_rollout_set_substeps(void *game, int n_sub);
int mfx_battle_rollout_get_substeps(void *game, int *n_sub);
/* names: view, feature, actions, rewards, mean_action, episode_return, stats, agent_steps, group_num, ids, alive, rng.
 * ids (int32 [E][G][rowcap]) and alive (uint8 [E][G][rowcap]) are written by mfx_battle_rollout_policy_step only
 * (mfx_battle_rollout_step leaves them alone): row i of group g of env e holds what mfx_battle_get's id / alive
 * getters would report for that member after the step and before clear_dead -- the row order of actions and
 * rewards.  Copyable (rollout_copy / rollout_copy_at), not writable.
 * rng (uint32 [E]): every env's shuffle engine, a minstd state (GridWorld.cc:31, :512); no reset re-seeds it. */
int mfx_battle_rollout_buffer(void *game, const char *name, int group, void **d_ptr, size_t *bytes);
int mfx_battle_rollout_copy(void *game, const char *name, int group, void *dst, size_t bytes);
/* bytes [offset, offset + bytes) of a rollout buffer (e.g. one env's rows), async on the engine stream */
int mfx_battle_rollout_copy_at(void *game, const char *name, int group, size_t offset, void *dst, size_t bytes);
int mfx_battle_rollout_rowcap(void *game, int *rowcap);
/* Doubles per [env][group] row of the rollout's mean-action buffer (the largest n_action of the groups). */
int mfx_battle_rollout_mean_stride(void *game, int *stride);
/* Persistent grid (workgroups per launch) and dynamic LDS bytes per workgroup of the fused rollout. */
int mfx_battle_rollout_info(void *game, int *grid, int *lds_bytes);
/* Synchronises the engine stream; -1 (message in mfx_last_error) if a device error was raised or, on the
 * large-env queue kernel k_rollout_bigq, its work queue reported an error (a stall, a workgroup outside
 * XCDs 0-7, or the hand-off guard: an item that saw a step counter other than its own). */
int mfx_battle_rollout_check(void *game);
/* The kernels rollout_step runs: 0 k_rollout, 1 k_rollout_obs + k_rollout (pipeline), 2 k_observe_items +
 * k_rollout_big (large-env pipeline), 3 k_rollout_bigq. */
int mfx_battle_rollout_path(void *game, int *path);
/* Lanes over which the rollout sums a group's rewards of an env with n_agents agents: the summation order of
 * the episode returns (64: one wave, 256 / 512: a workgroup's lane-strided partials, then wave sums). */
int mfx_battle_rollout_sum_lanes(void *game, int n_agents, int *lanes);
/* A learned policy in the loop: mode 2 writes every env's observation into the rollout buffers; mode 1 takes
 * the actions in the rollout's action buffer (a policy forward on that observation, e.g. mfx_qnet_act_rollout;
 * an id outside [0, 64) is rejected like set_action's and left out of the mean action), runs set_action / step /
 * reward / mean action / clear_dead / restart and writes the next observation.  The mean-action buffer then
 * holds each group's former_act_prob (zeros at an episode's first step).  Every plan but the observation/step
 * pipeline (MFX_ROLLOUT_PIPE=1) takes it: large batches of LDS-sized envs on the fused k_rollout, large envs and
 * batches of few LDS-sized envs on k_rollout_big + k_observe_items, one step per call on the engine's stream
 * (mfx_battle_rollout_policy_path).  A mode-2 call must precede the first mode-1 call after rollout_init,
 * rollout_step or any per-call API use; rollout_step and the policy steps interleave exactly. */
int mfx_battle_rollout_policy_step(void *game, int mode);
/* The kernels rollout_policy_step runs, numbered like mfx_battle_rollout_path: 0 k_rollout, 2 k_observe_items +
 * k_rollout_big; -1 when the plan refuses a learned policy. */
int mfx_battle_rollout_policy_path(void *game, int *path);
/* Copy `bytes` bytes from src (device or host) into a rollout buffer, async on the engine stream: the inverse of
 * mfx_battle_rollout_copy.  Only "actions" is writable. */
int mfx_battle_rollout_write(void *game, const char *name, int group, const void *src, size_t bytes);
/* The inputs of group `group`'s observation view that can be non-zero (Map.cc:130-218): mask[n] (n = view_h *
 * view_w * n_ch, NHWC) = 1 for every channel of a cell inside the view range and for the minimap channels of the
 * cells outside it, else 0 (never written: always zero). */
int mfx_battle_view_support(void *game, int group, uint8_t *mask, int n);
/* Diagnostic build only (libmagent_stamps.so): per-phase s_memtime stamps [E][16]. */
int mfx_battle_set_stamp_buffer(void *d_buf);

/* ---------------------------------------------------------------- part 3: Ising MF-Q */
int mfx_ising_create(int replicas, int n_agents, int k, const int16_t *nbr, void **handle);
int mfx_ising_destroy(void *handle);
int mfx_ising_set_spins(void *handle, const uint8_t *spins);
int mfx_ising_get_spins(void *handle, uint8_t *spins);
/* IsingMultiAgentEnv.step for every replica (environment.py:49-78) */
int mfx_ising_step(void *handle, const int32_t *actions, double *reward, uint8_t *obs, int32_t *n_up,
                   double *order);
/* The episode loop of main_MFQ_Ising.py (:84-159) in one launch per batch of replicas. */
int mfx_ising_mfq_run(void *handle, int T, double temperature, double lr, double decay_rate, int decay_gap,
                      const double *u, const uint32_t *mask, unsigned seed, double *q, double *order,
                      int32_t *n_up, int32_t *steps);
/* main_MFQ_Ising.py with its numpy RandomState stream generated on the device (MT19937, numpy's legacy draws: the
 * Boltzmann uniforms and the act_group permutation): replica r runs the script with seed seed0 + r for `episodes`
 * episodes in sequence on one stream (-epi), each until its early stop; outputs per episode (host, nullable except
 * q): q [E][R][N][K+1][2], order [E][R][T], n_up [E][R][T], steps [E][R]. */
int mfx_ising_mfq_run_stream(void *handle, int T, double temperature, double lr, double decay_rate, int decay_gap,
                             double act_rate, unsigned seed0, int episodes, double *q, double *order, int32_t *n_up,
                             int32_t *steps);

/* ---------------------------------------------------------------- part 3b: Ising trace, sweep, Metropolis
 * The trace: next to order / n_up, every executed step t < steps[r] of replica r also gives
 *   rsum[r][t] = sum(reward) of the step (main_MFQ_Ising.py:158).  Every reward is a multiple of 0.5 with
 *                |reward| <= K / 2, so the sum is exact in any order;
 *   mse[r][t]  = sum over the step's act_group of (Q_new[i] - target[st_i][act_i])^2, over N (:125-133): Q_new the
 *                entry just updated, st_i the agent's up-neighbour count on the old spins,
 *                target[s][a] = (a ? 1 : -1) (2 s - K) / 2 -- at K = 4 the script's reward_target table (:77-81).
 * Summation order of the mse (the script adds in act_group order; the device has only the group's mask): the
 * workgroup has B = 64 ceil(N / 64) <= 1024 lanes; lane l adds the terms of its own agents l, l + B, ... in ascending
 * index; an xor butterfly with masks 1, 2, 4, 8, 16, 32 runs over each wave's 64 lanes (v = v + v[lane ^ m]); lane 0
 * adds the waves' partials in wave order and divides by (double) N.  Single IEEE float64 operations, no
 * floating-point atomics: bitwise reproducible (tests/ising_trace_ref.py restates it).  Against the script's order
 * the mse differs by at most 2 N 2^-53 of itself.
 * Rows t >= steps[r] of rsum / mse (and, from mfx_ising_mfq_run_sweep, of order) read as NaN. */
/* mfx_ising_mfq_run with the trace and, optional, a clamp temperature per replica: temps [R] (null: `temperature`),
 * every entry finite and above zero.  rsum, mse [R][T] host, nullable. */
int mfx_ising_mfq_run_trace(void *handle, int T, double temperature, const double *temps, double lr,
                            double decay_rate, int decay_gap, const double *u, const uint32_t *mask, unsigned seed,
                            double *q, double *order, int32_t *n_up, int32_t *steps, double *rsum, double *mse);
/* A temperature sweep in one launch (single episode, the device's numpy streams): n_streams streams
 * RandomState(seed0 + s) are generated and walked once; replica r runs main_MFQ_Ising.py at temps[r] on stream
 * stream_of[r] -- its words, step offsets, act_group masks and env.reset spins -- as the script run with one seed at
 * several -t.  stream_of null: stream r, and n_streams must equal the handle's replicas.  Returns -1 with a message
 * on a temperature that is not finite and above zero or a stream_of entry outside [0, n_streams); temps has the
 * handle's R entries.  Outputs host, nullable except q: q [R][N][K+1][2], order / rsum / mse [R][T], n_up [R][T],
 * steps [R]. */
int mfx_ising_mfq_run_sweep(void *handle, int T, const double *temps, const int32_t *stream_of, int n_streams,
                            unsigned seed0, double lr, double decay_rate, int decay_gap, double act_rate, double *q,
                            double *order, int32_t *n_up, int32_t *steps, double *rsum, double *mse);
/* Metropolis baseline from the current spins, 4-neighbour lattices of even side >= 4 only (-1 with a message
 * otherwise): per sweep the sites of even row + column, then the odd ones; site i of replica r with `a` neighbours
 * equal to it flips when u < acc[r][a], acc [R][5] host values in [0, 1] (no exp() on the device), u the Philox draw
 * of counter (i, sweep, r, 0x5EED2) under key (seed, 0xA511E9B3), 53 bits as the MF-Q draws (whose fourth counter
 * word is 0x5EED1).  order, n_up [R][sweeps] after each sweep; the spins are updated in place. */
int mfx_ising_mc_run(void *handle, int sweeps, const double *acc, unsigned seed, double *order, int32_t *n_up);
/* Measurement: record event `which` (0 start, 1 stop) on the handle's stream; the milliseconds between the two. */
int mfx_ising_mark(void *handle, int which);
int mfx_ising_marked_ms(void *handle, float *ms);

/* ---------------------------------------------------------------- part 4: mean-field kernels */
/* senario_battle.py:141 -- d_acts [B][rowcap], d_counts [B] -> d_out [B][n_action] float64, 1 <= n_action <= 256.
 * Row b pools its first n = min(d_counts[b], rowcap) slots (a negative count reads as 0; the row-list kernels cap
 * the same counts): out[b][a] = (slots equal to a) / n.  An action outside [0, n_action) is counted in no entry
 * while n stays the divisor; n = 0 gives a row of NaN. */
int mfx_mean_action(const int32_t *d_acts, const int32_t *d_counts, int B, int rowcap, int n_action, double *d_out,
                    void *stream);
/* algo/base.py:192-220 */
int mfx_mfq_target(const float *d_eq, const float *d_tq, const float *d_r, const uint8_t *d_done, int M, int A,
                   double gamma, double *d_out, void *stream);
/* The opt-in Boltzmann mean-field value target (csrc/qsample.h; tests/qtarget_ref.py restates it): the
 * paper's v^MF (arXiv 1802.05438 eqs. 9-11), the value of the next state under the policy that acts, where
 * mfx_mfq_target takes the value of the greedy action.  It has no counterpart in the reference.  For one row, with
 * e_q[0..A) from the eval net and t_q[0..A) from the target net on the next state, 2 <= A <= 32, temperature T:
 *   weights   exactly the acting weights of mfx_q_sample at T: m = max e_q, w[a] = expf((e_q[a] - m) / T) in f32, one
 *             rounding per operation -- its non-finite rule included: a row of e_q with any NaN or +-inf has w = 1 at
 *             its greedy action (first maximum over the non-NaN entries, 0 if all are NaN) and 0 elsewhere.  (The max
 *             rule's argmax lets the first NaN win; this rule follows the acting policy instead.)
 *   value     num = sum_a f64(w[a]) f64(t_q[a]), den = sum_a f64(w[a]), both in ascending action order in float64
 *             (each product is exact there); v = num / den, one f64 division.  A NaN or infinite t_q[a] makes v NaN
 *             even where w[a] = 0.
 *   target    y = f64(r) + ((1 - done) * v) * gamma: the form, the dtype rules and the `done` reading (any non-zero
 *             byte) of mfx_mfq_target; float64 out.
 * One lane per row (k_mfq_target_soft).  d_T, when not null, is a one-element f32 device value that overrides T (a
 * captured graph follows a temperature that changes between replays); a device-side temperature that is not finite
 * and > 0 makes every target (and d_w entry) of that launch NaN.  A outside 2..32, and with d_T null a T that is not
 * finite and > 0, return -1 (mfx_last_error) and nothing is launched.  M = 0 is a no-op.  d_w: [M][A] weights out,
 * or null. */
int mfx_mfq_target_boltzmann(const float *d_eq, const float *d_tq, const float *d_r, const uint8_t *d_done, int M, int A,
                             double gamma, float T, const float *d_T, double *d_out, float *d_w, void *stream);
/* algo/ac.py:305-320 -- numpy1 = 1: the reference's NumPy-1 promotion (float64 running return, the
 * default of the python wrapper); 0: NEP-50 (float32), as the same lines run under NumPy 2 */
int mfx_mfac_returns(float *d_rew, const int64_t *d_offsets, const float *d_value, int n_ep, double gamma,
                     int numpy1, void *stream);

/* ---------------------------------------------------------------- part 4b: neighbourhood mean action (opt-in) */
/* The paper's mean action (arXiv 1802.05438 eq. 6), a_bar_j = 1 / |N(j)| sum_{k in N(j)} a_k over agent j's own
 * neighbours, where mfx_mean_action, the rollout's mean buffer and the reference give every agent of a group the
 * group-wide mean (csrc/neighbor_kernels.hip; tests/neighbor_mean_ref.py restates it).  For a list of n
 * members of one group with positions (x_j, y_j) and actions a_j, radius R >= 0:
 *   N_R(j)     the members k with max(|x_k - x_j|, |y_k - y_j|) <= R, j itself included: |N_R(j)| >= 1, no NaN case
 *   out[j][a]  (float)((double)(members of N_R(j) with action a) / (double)|N_R(j)|), a < n_action; an action outside
 *              [0, n_action) is counted in no entry while the divisor stays (mfx_mean_action's rule)
 * Integer counts and one float64 division per entry: bitwise reproducible, no tolerance.  One workgroup per list on
 * a persistent grid scans, per member, the window of a W x H byte grid kept in LDS; plain vector stores only.
 * Limits: 1 <= n_action <= 64, R >= 0, W * H + 5 * rowcap + 1040 bytes of LDS <= 160 KiB (256 x 256 with 4096 rows
 * fits; 512 x 512 does not).  Anything else returns -1 (mfx_last_error names the limit) and nothing is launched.
 *
 * mfx_neighbor_mean  the definition on a compact list: d_pos [B][rowcap][2] (x, y), d_actions [B][rowcap], d_counts
 *                    [B] (capped at rowcap, a negative one reads as 0) -> d_out [B][rowcap][n_action] float32; rows
 *                    at and past the count are left as they are.  The positions of one list must be distinct cells
 *                    inside the map, as the engine guarantees for its agents: this is the caller's contract and is
 *                    not checked (a position outside the map gets a row of zeros and counts for nobody).
 * The rollout forms run the same device code behind another loader, for group `group` of an engine behind
 * mfx_battle_rollout_init, on the engine's stream; nothing is read back.  d_out [E][rowcap][n_action] float32 and
 * d_state (2 * E int32: prev_num [E], prev_episode [E]) are the caller's; one workgroup owns an env's entries.
 *   mfx_neighbor_mean_reset    after the policy observe: rows j < group_num[e][group] zero (the reference starts an
 *                              episode from a zero mean, senario_battle.py:89), prev_num = group_num, prev_episode =
 *                              (int)stats[e][0].
 *   mfx_neighbor_mean_rollout  once after every mfx_battle_rollout_policy_step.  Members are the survivors of the
 *                              step, the rows j < group_num[e][group] of the new observation: (x, y) = (rint(feat[F - 2]
 *                              W), rint(feat[F - 1] H)) of feature row j (the observation writes (float)x / (float)W
 *                              there: exact); the action of survivor j is the action-buffer entry of the j-th row
 *                              with alive != 0 among the first prev_num rows (actions and alive keep the order of
 *                              before clear_dead).  Agents that died in the step have no position and count for
 *                              nobody.  An env whose episode number differs from prev_episode restarted in the
 *                              step: its rows j < group_num are zero.  Rows j >= group_num are left as they are.
 *                              Then prev_num and prev_episode are rewritten, in the same launch.
 * Both refuse a group whose features carry no position (minimap_mode off).  With no death in the step and R >= max(W,
 * H) every row equals the rollout's mean_action[e][group][a] cast to float, bit for bit; with R = 0 it is the one-hot
 * row of the agent's own action. */
int mfx_neighbor_mean(const int32_t *d_pos, const int32_t *d_actions, const int32_t *d_counts, int B, int rowcap,
                      int n_action, int radius, int W, int H, float *d_out, void *stream);
int mfx_neighbor_mean_reset(void *game, int group, float *d_out, int32_t *d_state);
int mfx_neighbor_mean_rollout(void *game, int group, int radius, float *d_out, int32_t *d_state);

/* ---------------------------------------------------------------- part 5: policy forward */
/* The Q network of ValueNet._construct_net (algo/base.py:123-183) and its greedy act (:228-254), forward
 * only, f32 MFMA (csrc/policy_kernels.hip); the Battle view (13 x 13 x 7), features F <= 256, n_action <= 32.
 * Weights: one float32 blob of n_floats in the layout mfx_qnet_blob_size reports (18 offsets: w1 b1 w2 b2
 * wd bd we be wp1 bp1 wp2 bp2 w2d b2d wo bo wq bq, every matrix [K][N] row-major, K padded to 4). */
int mfx_qnet_blob_size(int feature, int n_action, int use_mf, size_t *n_floats, size_t *offsets);
int mfx_qnet_create(int view_h, int view_w, int n_ch, int feature, int n_action, int use_mf, void **handle);
int mfx_qnet_destroy(void *handle);
int mfx_qnet_set_weights(void *handle, const float *d_blob, size_t n_floats, void *stream);
/* Acting precision of mfx_qnet_forward / mfx_qnet_act_rollout: 0 = f32 (the default at create), 1 = bf16 matrix
 * operands (weights, inputs and each layer's activation rounded to nearest even), f32 accumulation, biases, ReLU
 * and Q values (csrc/qnet_bf16_kernels.hip states the contract).  Any other value is refused and the handle keeps
 * its mode.  The f32 blob is kept in both modes; with weights set, the images the new mode lacks are built on
 * `stream`, so switching needs no re-upload and the f32 results are the same before and after. */
int mfx_qnet_set_precision(void *handle, int precision, void *stream);
int mfx_qnet_precision(void *handle, int *precision);
/* A forward needs weights.  Every acting call of this part -- mfx_qnet_forward, mfx_qnet_act_rollout and their
 * _sample / _rows forms, mfx_acnet_forward, mfx_acnet_act_rollout -- on a handle that has had no mfx_*_set_weights
 * returns -1 ("... needs weights (mfx_*_set_weights)" in mfx_last_error()) in both precisions, before anything is
 * launched: until then the blob and the weight images the kernels read are bare allocations.  One handle may serve
 * callers on several streams (two engines that share a network): the Q network's pass buffer is kept per stream, and
 * each caller brings its own d_rows / d_total.  Each stream that ever calls a Q handle keeps its buffer, grow-only
 * (10 KB per row of its largest call, at most 2^18 rows = 2.7 GB), until mfx_qnet_destroy; and the calls on one handle
 * must come from one host thread at a time (the per-stream table, like the rest of the handle, is not locked). */
/* n agents: view [n][1183], feature [n][F], prob [n][A] (mean field, else null) -> q [n][A], act [n] */
int mfx_qnet_forward(void *handle, const float *d_view, const float *d_feat, const float *d_prob, int n, float *d_q,
                     int32_t *d_act, void *stream);
/* group g of a rollout batch -> the rollout's action buffer (live rows); d_rows: E * rowcap ints scratch, d_total:
 * 1 + ceil(E / 64) ints (the row count, then per-64-env chunk totals) -- one buffer of E * rowcap + 1 + ceil(E / 64)
 * ints with d_total = d_rows + E * rowcap is the usual layout */
int mfx_qnet_act_rollout(void *handle, const float *d_view, const float *d_feat, const int32_t *d_counts,
                         const double *d_mean, int mean_stride, int E, int G, int g, int rowcap, int32_t *d_rows,
                         int32_t *d_total, int32_t *d_act, void *stream);
/* (the row count stays on the device: the kernels are launched for E * rowcap rows and read *d_total) */

/* The opt-in Boltzmann acting mode of the Q network (csrc/qsample.h; tests/qsample_ref.py restates it).
 * The reference's act, and every entry point above, is greedy; these draw the action instead.  For a row of f32 Q
 * values q[0..A) -- exactly the values the forward writes to d_q -- and a temperature T:
 *   weights   m = max_a q[a];  w[a] = expf((q[a] - m) / T), the subtraction and the IEEE division in f32, one
 *             rounding each
 *   draw      tot = the f32 sum of w in ascending action order;  thr = u * tot (one f32 multiply);  the action is
 *             the first a whose running f32 sum, same order, satisfies run > thr, and A - 1 if none does (the rule
 *             of the actor-critic draw)
 *   uniform   u = the counter hash of (seed, step, group, row) that draws the actor-critic actions (ac_uniform):
 *             row = i with group 0 for the forward, row = e * rowcap + j with the group index for a rollout, as
 *             mfx_acnet_forward / mfx_acnet_act_rollout define it
 *   non-finite rows   a row with any NaN or +-inf takes the greedy action (the first maximum over its non-NaN
 *             entries; 0 if all are NaN), weights 1 there and 0 elsewhere: a rollout never gets an id made from NaNs
 *   temperature   must be finite and > 0; anything else returns -1 (mfx_last_error) and nothing is launched
 * Both follow the handle's precision and run on every rollout plan the greedy calls do; they change nothing but
 * the action (and d_w): d_q is bit for bit mfx_qnet_forward's, and (d_act, d_w) are bit for bit mfx_q_sample's on
 * that d_q.  The training target is not part of this mode (mfx_mfq_target: max over e_q, unless the opt-in
 * mfx_mfq_target_boltzmann / mfx_qtrain_set_target is chosen as well).  d_w: [n][A] weights out
 * (null: not written); d_q, d_act may be null too. */
int mfx_qnet_forward_sample(void *handle, const float *d_view, const float *d_feat, const float *d_prob, int n,
                            float *d_q, float *d_w, int32_t *d_act, float temperature, uint32_t seed, uint32_t step,
                            void *stream);
int mfx_qnet_act_rollout_sample(void *handle, const float *d_view, const float *d_feat, const int32_t *d_counts,
                                const double *d_mean, int mean_stride, int E, int G, int g, int rowcap, int32_t *d_rows,
                                int32_t *d_total, int32_t *d_act, float temperature, uint32_t seed, uint32_t step,
                                void *stream);
/* mfx_qnet_act_rollout / _sample with a mean action per agent (the neighbourhood mean of part 4b) in
 * place of the env's row of d_mean: rollout row e * rowcap + j reads d_prob_rows [E][rowcap][A] float32 (A the
 * handle's n_action) at its own index.  Everything else -- the row list, the precisions, the draw and its uniform
 * (seed, step, g, e * rowcap + j), the rows written -- is the call's above: with d_prob_rows[e][j] = (float)
 * d_mean[e][g] for every live row the actions are bit for bit the same. */
int mfx_qnet_act_rollout_rows(void *handle, const float *d_view, const float *d_feat, const int32_t *d_counts,
                              const float *d_prob_rows, int E, int G, int g, int rowcap, int32_t *d_rows,
                              int32_t *d_total, int32_t *d_act, void *stream);
int mfx_qnet_act_rollout_rows_sample(void *handle, const float *d_view, const float *d_feat, const int32_t *d_counts,
                                     const float *d_prob_rows, int E, int G, int g, int rowcap, int32_t *d_rows,
                                     int32_t *d_total, int32_t *d_act, float temperature, uint32_t seed, uint32_t step,
                                     void *stream);
/* The draw alone on a Q table in memory (k_q_sample): d_q [n][A] f32, 2 <= A <= 32 -> d_act [n], d_w [n][A] (either
 * may be null); row i drawn with (seed, step, group, i) -- mfx_q_sample_rows: (seed, step, group, d_rows[i]), d_rows
 * null: i. */
int mfx_q_sample(const float *d_q, int n, int A, float temperature, uint32_t seed, uint32_t step, int group,
                 float *d_w, int32_t *d_act, void *stream);
int mfx_q_sample_rows(const float *d_q, const int32_t *d_rows, int n, int A, float temperature, uint32_t seed,
                      uint32_t step, int group, float *d_w, int32_t *d_act, void *stream);

/* The scripted opponents "rush" and "random" of the device rollout loop (csrc/rule_kernels.hip, k_rule_act; DESIGN
 * 7p; tests/rule_ref.py restates the rule in numpy).  The project's own deterministic rule -- not the reference's
 * rush_prey_infer_action -- giving one action per observation row from that row alone: view [VH][VW][7] f32 as
 * env_get_observation gives it to the observing group (0 wall, 1 own group, 3 own minimap, 4 enemy, 6 enemy minimap;
 * both minimaps carry +1 at the agent's own bin), feature [F] f32 ending in x / W, y / H.  cy = VH / 2, cx = VW / 2;
 * comparisons on f32 as written, arithmetic integer:
 *   A  attack       the first row-major cell with enemy > 0.5 and view2attack >= 0: attack_base + view2attack
 *   B  in view      else, if a cell has enemy > 0.5: the one minimising (r - cy)^2 + (c - cx)^2, first row-major on
 *                   ties; d = (c - cx, r - cy)
 *   C  out of view  own bin: the first row-major cell with own minimap > 1.0; D = enemy minimap, minus 1.0f at the own
 *                   bin; target: the first row-major cell among those of the largest D > 0.  With an own bin, a target
 *                   and target != own bin, d = 64 (sign(c - bx), sign(r - by)); else
 *                   d = 64 (sign(0.5f - fx), sign(0.5f - fy)), fx, fy the last two features
 *   move            a < attack_base is free if move[a] == (0, 0), or if (cy + my, cx + mx) is inside the view with
 *                   wall, own and enemy all <= 0.5; the free a minimising (dx - mx)^2 + (dy - my)^2, first index on
 *                   ties (0 if none is free)
 *   exploration     u1 = the actor-critic draw's uniform (seed, step, group, row); u1 < eps: the action is
 *                   min(int(u2 * n_action), n_action - 1), u2 = the uniform (seed ^ 0x68E31DA4, step, group, row), one
 *                   f32 multiply.  eps = 0 never draws; eps = 1 is the random opponent.
 * mfx_rule_create: shape = {view_h, view_w, channels, feature}; view2attack int32 [view_h][view_w]; move_dx, move_dy
 * int32 [attack_base] (env_get_info "move_delta").  Pure data -- no game pointer, no device memory -- so one handle
 * serves the drop-in env and a rollout batch.  Supported: 7 channels (two groups, minimap on, no food mode), no turn
 * mode (attack_base = the number of moves), view_h * view_w <= 256, 2 <= n_action <= 64, feature >= 2, moves within
 * 16 cells; anything else returns -1.
 * mfx_rule_act: n dense rows -> d_act [n], row i drawn with (seed, step, group, i).  mfx_rule_act_rollout: group g of
 * a rollout batch, the argument conventions of mfx_qnet_act_rollout_sample (d_rows: E * rowcap ints, d_total: 1 +
 * ceil(E / 64) ints); row j of env e drawn with (seed, step, g, e * rowcap + j); only the action slots of live rows
 * are written.  A null pointer, n < 0 or an eps outside [0, 1] (NaN included) returns -1 before anything is
 * launched. */
int mfx_rule_create(const int32_t *shape, int attack_base, int n_action, const int32_t *view2attack,
                    const int32_t *move_dx, const int32_t *move_dy, void **handle);
int mfx_rule_destroy(void *handle);
int mfx_rule_act(void *handle, const float *d_view, const float *d_feat, int n, float eps, uint32_t seed,
                 uint32_t step, int group, int32_t *d_act, void *stream);
int mfx_rule_act_rollout(void *handle, const float *d_view, const float *d_feat, const int32_t *d_counts, int E, int G,
                         int g, int rowcap, int32_t *d_rows, int32_t *d_total, int32_t *d_act, float eps, uint32_t seed,
                         uint32_t step, void *stream);

/* The compact row list the act_rollout calls build: d_rows[i] = e * rowcap + j over envs e, j < min(counts[e][g],
 * rowcap), in env order; d_total[0] = the row count (d_total: 1 + ceil(E / 64) ints). */
int mfx_rollout_rows(const int32_t *d_counts, int E, int G, int g, int rowcap, int32_t *d_rows, int32_t *d_total,
                     void *stream);

/* The actor-critic network of ActorCritic._create_network (algo/ac.py:48-98) / MFAC._create_network (:219-276)
 * and its act, tf.multinomial(log(policy)) (:43-46, :213-217), forward only, f32 MFMA
 * (csrc/acnet_kernels.hip); views of view_floats <= 4096 floats (flattened NHWC), features <= 256,
 * 2 <= n_action <= 32.  The feature width picks one of two kernel forms: up to 36 floats h_emb is recomputed
 * tile by tile from weights kept in LDS (two workgroups per CU), wider features hold it in registers (one).
 * Weights: one float32 blob in the layout mfx_acnet_blob_size reports (19 offsets: wv bv
 * we be wd0 wd1 bd wp bp wval bval wep bep wdp bdp wvd bvd wvo bvo, every matrix [K][N] row-major, K padded to
 * 4; the 512-wide dense layer split by output halves).  The draw of row r of group g at step t is the first
 * action whose running f32 sum of the clipped policy exceeds u * (its f32 total), u = a 24-bit counter hash of
 * (seed, t, g, r) (tests/acnet_ref.py restates it). */
int mfx_acnet_blob_size(int view_floats, int feature, int n_action, int use_mf, size_t *n_floats, size_t *offsets);
int mfx_acnet_create(int view_floats, int feature, int n_action, int use_mf, void **handle);
int mfx_acnet_destroy(void *handle);
int mfx_acnet_set_weights(void *handle, const float *d_blob, size_t n_floats, void *stream);
/* The view inputs that can be non-zero, mask[n] (n = view_floats; e.g. mfx_battle_view_support), or null for the dense
 * order: later forwards run the view layer over the supported inputs only, bit-identical when the others are zero
 * (the caller's contract).  A mask with n != view_floats is refused and leaves the handle's support as it was.
 * input_support_size: the inputs the view layer runs over (0 = dense). */
int mfx_acnet_set_input_support(void *handle, const uint8_t *mask, int n, void *stream);
int mfx_acnet_input_support_size(void *handle, int *k);
/* Acting precision of mfx_acnet_forward / mfx_acnet_act_rollout: 0 = f32 (the default at create), 1 = bf16, the
 * policy path only (csrc/acnet_bf16_kernels.hip states the contract; same shape range).  In bf16 the operands of every
 * matrix product -- the view, feature, dense and policy weights, the view and feature inputs, h_view and h_emb after
 * bias and ReLU, and relu(d) / 0.1 (the f32 division, then one rounding) -- are rounded to nearest even; accumulation
 * (from the f32 bias), ReLU, softmax, the clip and the draw are f32, the draw's rule and uniforms unchanged; a row's
 * result depends on neither its place in the batch nor the batch size; an input support does not change the results
 * (the view layer runs the dense order).  bf16 is acting only: a call with a non-null d_value returns -1 ("bf16 is
 * acting only" in mfx_last_error()) and launches nothing; d_prob is not read.  Any other value is refused and the
 * handle keeps its mode.  The f32 blob is kept in both modes: set_precision(1) builds the bf16 images from it on
 * `stream`, set_weights in bf16 mode rebuilds them, and after set_precision(0) the results are bit-identical to a
 * handle that never left f32. */
int mfx_acnet_set_precision(void *handle, int precision, void *stream);
int mfx_acnet_precision(void *handle, int *precision);
/* n agents: view [n][view_floats], feature [n][F], prob [n][A] float32 (the MF value head; else null) ->
 * policy [n][A], value [n], act [n] (each may be null); row i drawn with (seed, step, group 0, row i).  Needs weights
 * (the rule at mfx_qnet_forward). */
int mfx_acnet_forward(void *handle, const float *d_view, const float *d_feat, const float *d_prob, int n,
                      float *d_policy, float *d_value, int32_t *d_act, uint32_t seed, uint32_t step, void *stream);
/* group g of a rollout batch -> sampled actions in the rollout's action buffer (live rows; row j of env e drawn
 * with (seed, step, g, e * rowcap + j)); d_rows / d_total as mfx_qnet_act_rollout's; nothing is read back */
int mfx_acnet_act_rollout(void *handle, const float *d_view, const float *d_feat, const int32_t *d_counts, int E,
                          int G, int g, int rowcap, int32_t *d_rows, int32_t *d_total, int32_t *d_act, uint32_t seed,
                          uint32_t step, void *stream);

/* ---------------------------------------------------------------- part 6: replay rows */
/* The data path of the replay buffers (algo/tools.py:26-362): for i < n, row idx[i] (or i; modulo src_mod
 * when > 0) of every source column -> row dst_start + i (modulo dst_cap when > 0) of its destination column;
 * n_cols <= 12, row_bytes per column; one launch (csrc/replay_kernels.hip).  src_rows: rows of every source
 * column -- without src_mod an index in [-src_rows, 0) counts from the end, as numpy's indexing does; any other
 * index outside [0, src_rows) (the reference's numpy indexing raises IndexError) skips the row and is reported by
 * mfx_rows_copy_error (synchronising; -1 and *bad_index when one was met, -1 included, then cleared). */
int mfx_rows_copy(int n_cols, void *const *dst, const void *const *src, const int64_t *row_bytes, const int64_t *d_idx,
                  int64_t src_mod, int64_t src_rows, int64_t dst_start, int64_t dst_cap, int64_t n, void *stream);
/* The same move with the columns whose bit is set in shift_mask reading source row idx[i] + shift (before the
 * modulo, checked the same way): MemoryGroup.sample's next-state columns at next_idx = (idx + 1) % nb_entries
 * (algo/tools.py:239-262) in the launch of the current-state columns.  mfx_rows_copy = shift_mask 0. */
int mfx_rows_copy_shift(int n_cols, void *const *dst, const void *const *src, const int64_t *row_bytes,
                        const int64_t *d_idx, int64_t src_mod, int64_t src_rows, int64_t dst_start, int64_t dst_cap,
                        int64_t n, uint32_t shift_mask, int64_t shift, void *stream);
int mfx_rows_copy_error(int64_t *bad_index, void *stream);
/* The launch form mfx_rows_copy_shift would take for these columns (pointers, row sizes and MFX_ROWS_PIPE decide it;
 * nothing is launched): out[0] = 0 the one-row-per-wave form k_rows_copy / 1 the pipelined k_rows_pipe<NW, NU>,
 * out[1] = NW, out[2] = NU (both 0 for k_rows_copy), out[3] = the narrow units of a row, out[4 + k] = column k's
 * class: 0 narrow moved in dwords, 1 narrow moved in bytes, 2 wide (>= 512 B).  out: 4 + n_cols ints. */
int mfx_rows_copy_plan(int n_cols, void *const *dst, const void *const *src, const int64_t *row_bytes,
                       uint32_t shift_mask, int32_t *out);

/* Replay rows straight from the device rollout loop (csrc/collect_kernels.hip): one row of the step-row columns per
 * live agent of one group for every mfx_battle_rollout_policy_step, with no host work per step.
 *   mfx_collect_begin  after the policy's actions are in the action buffer, before the policy step: builds the
 *                      compact live-row list of the group (mfx_rollout_rows, into d_rows / d_total: E * rowcap ints
 *                      and 1 + ceil(E / 64) ints of the caller's own) and writes, for list entry k = row j of env e,
 *                      row n + k of obs / feat / act, prob = (float) of the env's n_action doubles of mean (when
 *                      dst->prob is not null), and the env's episode number stats[e][0] parked in key;
 *   mfx_collect_end    after the policy step, same list: rew from rewards, term = !alive, key = mfx_collect_key(e,
 *                      parked episode number, ids[row], n_envs, id_stride); then advances n by the list length behind
 *                      the row writes on the same stream.
 * d_state: two int64 on the device -- [0] the row counter n, [1] the sticky error word (bit 0: a step did not fit in
 * dst->capacity rows: none of its rows was written and n did not move; bit 1: an id outside [0, id_stride)).  The
 * bound is checked before any store.  mfx_collect_reset sets n and clears the error word.  Everything is launched
 * on `stream` (the engine's); nothing is read back. */
typedef struct mfx_collect_src {          /* the rollout buffers (mfx_battle_rollout_buffer) and their shape */
    const float *view, *feat;             /* [E][rowcap][view_floats], [E][rowcap][feat_floats] of the group */
    const int32_t *actions;               /* [E][G][rowcap] */
    const float *rewards;                 /* [E][G][rowcap] */
    const double *mean;                   /* [E][G][mean_stride] (may be null without prob) */
    const double *stats;                  /* [E][4] */
    const int32_t *counts;                /* [E][G] group_num */
    const int32_t *ids;                   /* [E][G][rowcap] */
    const uint8_t *alive;                 /* [E][G][rowcap] */
    int32_t n_envs, n_groups, group, rowcap, view_floats, feat_floats, n_action, mean_stride;
} mfx_collect_src;
typedef struct mfx_collect_dst {          /* the step-row columns, `capacity` rows each */
    float *obs, *feat;
    int32_t *act;
    float *rew;
    uint8_t *term;                        /* 0 / 1 */
    float *prob;                          /* [capacity][n_action], or null */
    int64_t *key;
    int64_t capacity;
} mfx_collect_dst;
int mfx_collect_reset(int64_t *d_state, int64_t n, void *stream);
int mfx_collect_begin(const mfx_collect_src *src, const mfx_collect_dst *dst, int32_t *d_rows, int32_t *d_total,
                      int64_t *d_state, void *stream);
int mfx_collect_end(const mfx_collect_src *src, const mfx_collect_dst *dst, const int32_t *d_rows,
                    const int32_t *d_total, int64_t *d_state, int64_t id_stride, void *stream);
/* mfx_collect_begin with a mean action per agent (part 4b): list entry k = row j of env e takes its prob
 * from d_prob_rows[(e * rowcap + j) * n_action + a] (float32 [E][rowcap][n_action] of the group, copied bit for bit)
 * where mfx_collect_begin casts the env's row of src->mean; src->mean is not read.  dst->prob must not be null.
 * Everything else, mfx_collect_end and mfx_collect_end_linked included, is unchanged. */
int mfx_collect_begin_rows(const mfx_collect_src *src, const mfx_collect_dst *dst, const float *d_prob_rows,
                           int32_t *d_rows, int32_t *d_total, int64_t *d_state, void *stream);
/* (episode * n_envs + env) * id_stride + id: injective over env < n_envs, episode >= 0, id < id_stride (host) */
int64_t mfx_collect_key(int64_t env, int64_t episode, int64_t id, int64_t n_envs, int64_t id_stride);

/* Episode chains for the actor-critic models, whose returns run backwards along each agent's rows of one episode.
 *   mfx_collect_end_linked  mfx_collect_end, and in the same launch two more columns of step row r = n + k:
 *                      d_prev[r] = the row of the same key one step earlier, or -1; d_tail[r] = 1 while r is the
 *                      last row of its key (the predecessor's tail is cleared).  d_last: n_envs * id_stride int64,
 *                      [env * id_stride + id] = the newest row of that id, -1 when empty (mfx_collect_links_reset
 *                      before a session's first step); an entry left by an earlier episode fails the key
 *                      comparison.  A live id occurs once per env and step: no atomics.  The capacity rule holds:
 *                      a step that does not fit touches neither d_last, d_prev nor d_tail.
 *   mfx_chain_returns  in place on d_rew: for tail i, keep = d_value[i]; along r = d_tails[i], d_prev[r], ... to
 *                      -1: keep = keep * gamma + d_rew[r]; d_rew[r] = keep, in mfx_mfac_returns' two arithmetic
 *                      forms (numpy1).  Rows are step-major: a predecessor is below its row.  A tail outside
 *                      [0, n_rows) or a predecessor outside [0, its row) ends that walk before any further store
 *                      and the call returns -1 (it synchronises `stream` to report it). */
int mfx_collect_end_linked(const mfx_collect_src *src, const mfx_collect_dst *dst, const int32_t *d_rows,
                           const int32_t *d_total, int64_t *d_state, int64_t id_stride, int64_t *d_last,
                           int64_t *d_prev, uint8_t *d_tail, void *stream);
int mfx_collect_links_reset(int64_t *d_last, int64_t n, void *stream);
int mfx_chain_returns(float *d_rew, const int64_t *d_prev, const int64_t *d_tails, const float *d_value,
                      int64_t n_tails, int64_t n_rows, double gamma, int numpy1, void *stream);

/* GAE(lambda) advantages along the same chains (csrc/gae_kernels.hip; opt-in; tests/gae_ref.py restates it).
 *   mfx_chain_gae      d_value_rows: one f32 value V[r] per row, [n_rows]; d_adv: [n_rows], not d_rew.  For tail i with
 *                      t = d_tails[i], along r = t, d_prev[r], ... to -1, with x = d_rew[r] read before it is overwritten:
 *                          nxt = (double)V[t];  g = 0.0
 *                          per row r:  v = (double)V[r]
 *                                      delta = ((double)x + gamma * nxt) - v
 *                                      g     = delta + gl * g              (gl = gamma * lambda, formed once on the host)
 *                                      d_adv[r] = (float)g;  d_rew[r] = (float)(g + v);  nxt = v
 *                      every operation a rounded double operation of its own (no contraction).  The tail convention is the
 *                      reference's: the value of a chain's last row stands for the state after it, as mfx_chain_returns'
 *                      keep does, so lambda = 1 leaves the reference's bootstrapped return in d_rew and d_adv = return - V,
 *                      and lambda = 0 the one-step TD error in d_adv.  Rows that are on no chain keep both columns.
 *                      gamma and lambda must lie in [0, 1] (NaN is refused), before any launch.  The guards are
 *                      mfx_chain_returns': a tail outside [0, n_rows) or a predecessor outside [0, its row) ends that walk
 *                      before any further load or store, in either column, and the call returns -1 with the index in the
 *                      message (it synchronises `stream` to report it; the error word is this call's own and is cleared).
 *   mfx_adv_normalize  d_adv[0, n) <- (float)(((double)d_adv[r] - mean) / (std + 1e-8)), mean and the population standard
 *                      deviation in double, two passes.  One summation order per n: workgroup b sums elements [b span,
 *                      (b + 1) span) -- span = ceil(n / min(ceil(n / 4096), 1024)) -- each thread its elements t, t + 256,
 *                      ... in order, the threads by a fixed tree; then the workgroups' partials in index order.  No
 *                      floating-point atomics: equal input gives bitwise equal output.  n = 1 or a constant column gives
 *                      all zeros (exactly, while n < 2^29).  n = 0 does nothing.  Nothing is read back.  The scratch is
 *                      the library's: two calls must not run at once on two streams of a device. */
int mfx_chain_gae(float *d_rew, float *d_adv, const int64_t *d_prev, const int64_t *d_tails, const float *d_value_rows,
                  int64_t n_tails, int64_t n_rows, double gamma, double lambda, void *stream);
int mfx_adv_normalize(float *d_adv, int64_t n, void *stream);

/* ---------------------------------------------------------------- part 7: episode outcomes (csrc/score_kernels.hip) */
/* The scorekeeper of the device rollout loop: per-episode outcomes of every env with Runner.run's own win rule
 * (algo/tools.py, train=False), with no host work per step.  Group 0 is "main", group 1 "opponent"; two groups only
 * (any other n_groups is refused on the host).  The sources are the rollout buffers of mfx_battle_rollout_buffer, or
 * any device arrays of the same layout.
 *   mfx_score_attach   after the policy observe, before the first policy step: per env, carry = {n_cur[g] = start[g] =
 *                      group_num[e][g], ep = (int64)stats[e][0], steps0 = agent_steps[e], len = 0}, ret0[g] =
 *                      stats[e][1 + g]; zeroes totals, log and state.
 *   mfx_score_update   exactly once after every mfx_battle_rollout_policy_step, one launch.  Per env:
 *                      guard   agent_steps[e] - steps0 must be n_cur[0] + n_cur[1], else error bit 0 (a step was not
 *                              scored, or was scored twice); (int64)stats[e][0] - ep must be 0 or 1, else bit 1; a
 *                              carried or new group size outside [0, rowcap] is bit 2.  An env that fails one is not
 *                              scored in this call -- totals and log untouched -- and its carry is taken afresh as
 *                              attach does (n_cur, start, ep, steps0, len and ret0, not only n_cur and steps0), so
 *                              later calls stay in bounds and in step.  What that costs: an episode that ends in
 *                              the same call as a failed guard appears in neither the totals nor the log, and the
 *                              episode the env is in counts its length and start sizes from this call on.  The
 *                              sticky word tells the host that the totals are incomplete (finish() raises).
 *                      surv[g] = non-zero bytes among alive[e][g][0 .. n_cur[g]); later bytes are never counted.
 *                      len += 1; the episode ended iff (int64)stats[e][0] == ep + 1.  Then, with nums[g] = n_cur[g]
 *                      (the members of the last step, those that died in it included: get_num before clear_dead),
 *                      kill[0] = start[0] - nums[1], kill[1] = start[1] - nums[0]; winner = 0 (kill[0] > kill[1]),
 *                      1 (<) or 2 (equal: counts for both); ret[g] = stats[e][1 + g] - ret0[g].  The record goes to
 *                      log[e][episodes scored so far] when that index is < ep_cap, else dropped += 1.  totals +=
 *                      episode, win / tie, kills, len.  Then len = 0, ep += 1, ret0 = stats now.
 *                      carry   n_cur[g] = group_num[e][g], steps0 = agent_steps[e]; at an episode end start = n_cur.
 *                      When an env's episode count reaches `target` (>= 1), state[0] += 1 (integer atomic).
 * Everything but the two state words is written by its env's own wave; no float atomics; nothing depends on the launch
 * order.  Nothing synchronises and nothing is read back: the host reads totals, log and state when it wants them. */
typedef struct mfx_score_src {
    const int32_t *group_num;             /* [E][2] */
    const uint8_t *alive;                 /* [E][2][rowcap] */
    const double *stats;                  /* [E][4] */
    const int64_t *agent_steps;           /* [E] */
    int32_t n_envs, n_groups, rowcap;     /* rowcap: a multiple of 4 */
} mfx_score_src;
typedef struct mfx_score_record {         /* 48 bytes */
    int32_t len, nums[2], surv[2], kill[2], winner;
    double ret[2];
} mfx_score_record;
enum { MFX_SCORE_N_CUR = 0, MFX_SCORE_START = 2, MFX_SCORE_EP = 4, MFX_SCORE_STEPS0 = 5, MFX_SCORE_LEN = 6,
       MFX_SCORE_CARRY = 8 };             /* int64 words of an env's carry ([7] is zero) */
enum { MFX_SCORE_EPISODES = 0, MFX_SCORE_MAIN_WINS = 1, MFX_SCORE_OPPO_WINS = 2, MFX_SCORE_TIES = 3,
       MFX_SCORE_KILLS = 4, MFX_SCORE_STEPS = 6, MFX_SCORE_DROPPED = 7, MFX_SCORE_TOTALS = 8 };
enum { MFX_SCORE_ERR_STEP = 1, MFX_SCORE_ERR_EPISODE = 2, MFX_SCORE_ERR_COUNT = 4 };
typedef struct mfx_score_dst {
    int64_t *carry;                       /* [E][MFX_SCORE_CARRY] */
    double *ret0;                         /* [E][2] */
    int64_t *totals;                      /* [E][MFX_SCORE_TOTALS] */
    mfx_score_record *log;                /* [E][ep_cap] */
    int64_t *state;                       /* [2]: envs that reached target, the sticky error word */
    int64_t ep_cap, target;               /* ep_cap >= 0 (0: log may be null), target >= 1 */
} mfx_score_dst;
/* bytes of carry, ret0, totals, log, state for n_envs envs and ep_cap records (host) */
int mfx_score_sizes(int n_envs, int64_t ep_cap, size_t bytes[5]);
int mfx_score_attach(const mfx_score_src *src, const mfx_score_dst *dst, void *stream);
int mfx_score_update(const mfx_score_src *src, const mfx_score_dst *dst, void *stream);

/* ---------------------------------------------------------------- part 8: watched-env trace (csrc/trace_kernels.hip) */
/* The recorder of the device rollout loop: per step, for each of K watched envs (1 <= K <= MFX_TRACE_MAX_ENVS), the
 * rows that let a one-env engine re-run the env from the round's start and prove the re-run right
 * (mfrl_amd.recorder: RolloutRecorder, replay).  Two groups only.  The sources are the rollout buffers of
 * mfx_battle_rollout_buffer, or any device arrays of the same layout, 16-byte aligned (alive: 4-byte).
 * A round starts from reset + placement, but an env's shuffle engine (the minstd state behind the attack order,
 * GridWorld.cc:507-512) is never re-seeded by a reset: it runs on from round to round.  So the state it has at attach
 * ("rng" of mfx_battle_rollout_buffer) is part of the trace, and a re-run starts from it (the "seed" config key).
 *
 * One launch per step, after the step.  A learned policy's step reads the action buffer and never writes it
 * (agent_phase / big_env_step with kExt: csrc/battle/rollout.inc, rollout_big.inc), so the actions the step acted with
 * are still there behind it; group_num is not -- clear_dead and a restart rewrite it inside the step -- so the group
 * sizes of before the step are carried from attach / the previous update, as the scorekeeper carries n_cur.  Hence no
 * begin / end pair: nothing else the record needs is gone after the step.
 *   mfx_trace_attach   after the policy observe, before the first policy step.  h_envs: the K watched env indices on
 *                      the host, each in [0, n_envs), no duplicate (refused otherwise); they are copied to dst->envs on
 *                      `stream`.  Zeroes state; carry[0][k] = {group_num[e][0], group_num[e][1], (int64)stats[e][0],
 *                      agent_steps[e]}; seeds[k] = rng[e]; a group size outside [0, rowcap] sets MFX_TRACE_ERR_COUNT.
 *   mfx_trace_update   exactly once after every mfx_battle_rollout_policy_step; `step` = updates since attach (0, 1,
 *                      ...: the host knows it without a readback).  step >= cap_steps: MFX_TRACE_FULL is set and nothing
 *                      else is written.  Otherwise, for watched env k (e = envs[k]) with {n0, n1, ep, steps0} =
 *                      carry[step & 1][k]:
 *                      guard   agent_steps[e] - steps0 must be n0 + n1, else MFX_TRACE_ERR_STEP (a step was not
 *                              recorded, or was recorded twice); (int64)stats[e][0] - ep must be 0 or 1, else
 *                              MFX_TRACE_ERR_EPISODE; n0, n1 and the new group sizes must lie in [0, rowcap], else
 *                              MFX_TRACE_ERR_COUNT.  A failed guard sets its bits in the sticky word and the record's
 *                              valid word to 0; the carry is taken afresh either way.
 *                      head[step][k] = {valid, n0, n1, ep, (int64)stats[e][0], agent_steps[e]} (MFX_TRACE_HEAD words);
 *                      actions / ids / rewards / alive [step][k][g][0 .. rowcap) = the source rows [e][g][0 .. rowcap)
 *                      verbatim, stale entries at and past n[g] included (no address depends on n);
 *                      carry[(step + 1) & 1][k] = {group_num[e][0], group_num[e][1], (int64)stats[e][0],
 *                      agent_steps[e]}; state[0] = step + 1.
 *                      An envs[k] outside [0, n_envs) on the device (the host refused it: a corrupted list) sets
 *                      MFX_TRACE_ERR_ENV, valid = 0, and no row is read or written.
 * One workgroup per (watched env, group); the lanes move the int32 / float rows as 16-byte vectors (rowcap is a multiple
 * of 4) and the alive row as 16-byte vectors when rowcap is a multiple of 16, else as dwords; the group-0 workgroup
 * writes the head and the carry of the other parity, which no workgroup of the launch reads.  Plain stores, one integer
 * atomic OR on the error word, no float atomics; nothing depends on the launch order.  Nothing synchronises and nothing
 * is read back.  Nothing is written outside dst's arrays: every offset is a function of step < cap_steps, k < K, g < 2
 * and the row index < rowcap alone. */
enum { MFX_TRACE_MAX_ENVS = 16, MFX_TRACE_HEAD = 6, MFX_TRACE_CARRY = 4 };
enum { MFX_TRACE_VALID = 0, MFX_TRACE_N = 1, MFX_TRACE_EP_BEFORE = 3, MFX_TRACE_EP_AFTER = 4, MFX_TRACE_STEPS = 5 };
enum { MFX_TRACE_ERR_STEP = 1, MFX_TRACE_ERR_EPISODE = 2, MFX_TRACE_ERR_COUNT = 4, MFX_TRACE_FULL = 8,
       MFX_TRACE_ERR_ENV = 16 };
typedef struct mfx_trace_src {
    const int32_t *group_num;             /* [E][2] */
    const uint8_t *alive;                 /* [E][2][rowcap] */
    const double *stats;                  /* [E][4] */
    const int64_t *agent_steps;           /* [E] */
    const int32_t *actions;               /* [E][2][rowcap] */
    const int32_t *ids;                   /* [E][2][rowcap] */
    const float *rewards;                 /* [E][2][rowcap] */
    const uint32_t *rng;                  /* [E] */
    int32_t n_envs, n_groups, rowcap;     /* rowcap: a multiple of 4 */
} mfx_trace_src;
typedef struct mfx_trace_dst {
    int32_t *envs;                        /* [K] watched env indices (device; written by attach) */
    int64_t *carry;                       /* [2][K][MFX_TRACE_CARRY], by step parity */
    int64_t *head;                        /* [cap_steps][K][MFX_TRACE_HEAD] */
    int32_t *actions;                     /* [cap_steps][K][2][rowcap] */
    int32_t *ids;                         /* [cap_steps][K][2][rowcap] */
    float *rewards;                       /* [cap_steps][K][2][rowcap] */
    uint8_t *alive;                       /* [cap_steps][K][2][rowcap] */
    int64_t *state;                       /* [2]: steps recorded, the sticky error word */
    uint32_t *seeds;                      /* [K] the watched envs' shuffle-engine states at attach */
    int64_t cap_steps;                    /* >= 1 */
    int32_t n_watch;                      /* K */
} mfx_trace_dst;
/* bytes of envs, carry, head, actions, ids, rewards, alive, state, seeds (host) */
int mfx_trace_sizes(int n_watch, int rowcap, int64_t cap_steps, size_t bytes[9]);
int mfx_trace_attach(const mfx_trace_src *src, const mfx_trace_dst *dst, const int32_t *h_envs, void *stream);
int mfx_trace_update(const mfx_trace_src *src, const mfx_trace_dst *dst, int64_t step, void *stream);

/* ---------------------------------------------------------------- Q-network training (csrc/qtrain_kernels.hip) */
/* ValueNet's minibatch step (algo/base.py:123-279, algo/q_learning.py) for the Q network above, f32, on the device:
 * sample rows idx and (idx + 1) % n straight from the replay ring -> y = f32(f64(r) + ((1 - done) f64(q_target[argmax
 * q_eval])) gamma) on the next rows -> loss = sum d^2 m / sum m with d = y - q_eval[a] on the current rows -> backward
 * -> Adam (bias-corrected by the step count) -> target <- (1 - tau) target + tau eval.  Battle view 13 x 13 x 7,
 * feature <= 256, n_action <= 32.
 * The handle owns four blobs in the layout of mfx_qnet_blob_size -- the eval and target parameters and Adam's m and v
 * -- and the step count.  Padding entries of every blob stay exactly zero.  The trained eval blob can go to
 * mfx_qnet_set_weights device to device.
 *   set_hyper        defaults: lr 1e-4, betas 0.9 / 0.999, eps 1e-8 (torch's Adam), tau 0.005, gamma 0.95; eps must be
 *                    > 0 (an entry whose g, m and v are all zero divides by it and must stay zero)
 *   set_target       the rule of y (host state, read by the grads / run calls that follow): MFX_QTARGET_MAX, the
 *                    default and the reference's rule above, or MFX_QTARGET_BOLTZMANN (opt-in): y = f32(f64(r)
 *                    + ((1 - done) v) gamma) with v of mfx_mfq_target_boltzmann -- weights from q_eval on the next rows
 *                    at `temperature`, values from q_target on the next rows -- rounded once to f32.  The temperature
 *                    must be finite and > 0 (read only for the boltzmann rule) and the handle have >= 2 actions; a
 *                    refusal leaves the handle as it was.  Launch count, buffers and bitwise reproducibility are
 *                    the same under both rules, and MAX after BOLTZMANN is bit for bit a fresh handle's MAX.
 *   set/get_state    `which` = MFX_QTRAIN_EVAL / TARGET / ADAM_M / ADAM_V; n_floats must be the blob size; a copy on
 *                    `stream`.  Setting eval or target leaves the moments and the step count alone.
 *   reset_optimizer  zeroes m, v and the step count
 *   step_count       minibatches applied (host copy; exact after mfx_qtrain_error)
 *   grads            the gradient of one minibatch in blob layout (padding zero) into d_grad_blob and (loss, mean
 *                    q[a]) into d_stats (either may be null); no state changes; bit for bit the gradient run applies
 *   run              n_batches minibatches in sequence, all enqueued by this one call: d_idx [n_batches][B] int64,
 *                    d_stats [n_batches][2] (or null); nothing is read back, nothing synchronises
 *   error            synchronises `stream`; *code = 0, or MFX_QTRAIN_BAD_INDEX (an idx outside [0, n)) /
 *                    MFX_QTRAIN_BAD_ACTION (a ring action outside [0, n_action)) with the offending value in
 *                    *bad_value, and clears it.  Indices and actions are checked on the device before any load
 *                    that depends on them; from the bad minibatch on nothing is applied (state and step count
 *                    unchanged, stats undefined) until this call has cleared the word.
 * 1 <= B <= 4096, 1 <= n <= 2^31 - 1 (row offsets are 64-bit).  A null handle is refused.  Every sum has a fixed order: equal state and equal indices give bitwise equal results.  All
 * launches go to `stream`; the ring columns must stay valid until they have run. */
typedef struct mfx_qtrain_ring {          /* MemoryGroup's ring columns, rows [0, n) live */
    const float *obs0;                    /* [rows][13 * 13 * 7] */
    const float *feat0;                   /* [rows][feature] */
    const int32_t *actions;               /* [rows] */
    const float *rewards;                 /* [rows] */
    const uint8_t *terminals;             /* [rows] 0 / 1 */
    const uint8_t *masks;                 /* [rows] 0 / 1 */
    const float *prob;                    /* [rows][n_action] (mean field), else null */
} mfx_qtrain_ring;
enum { MFX_QTRAIN_EVAL = 0, MFX_QTRAIN_TARGET = 1, MFX_QTRAIN_ADAM_M = 2, MFX_QTRAIN_ADAM_V = 3 };
enum { MFX_QTRAIN_BAD_INDEX = 1, MFX_QTRAIN_BAD_ACTION = 2 };
enum { MFX_QTARGET_MAX = 0, MFX_QTARGET_BOLTZMANN = 1 };
int mfx_qtrain_create(int feature, int n_action, int use_mf, void **handle);
int mfx_qtrain_destroy(void *handle);
int mfx_qtrain_set_hyper(void *handle, double lr, double beta1, double beta2, double eps, double tau, double gamma);
int mfx_qtrain_set_target(void *handle, int rule, float temperature);
int mfx_qtrain_set_state(void *handle, int which, const float *d_blob, size_t n_floats, void *stream);
int mfx_qtrain_get_state(void *handle, int which, float *d_out, size_t n_floats, void *stream);
int mfx_qtrain_reset_optimizer(void *handle, void *stream);
int mfx_qtrain_step_count(void *handle, long long *t);
int mfx_qtrain_grads(void *handle, const mfx_qtrain_ring *ring, long long n, const int64_t *d_idx, int B,
                     float *d_grad_blob, float *d_stats, void *stream);
int mfx_qtrain_run(void *handle, const mfx_qtrain_ring *ring, long long n, const int64_t *d_idx, int n_batches, int B,
                   float *d_stats, void *stream);
int mfx_qtrain_error(void *handle, int *code, long long *bad_value, void *stream);

/* ---------------------------------------------------------------- AC-network training (csrc/actrain_kernels.hip) */
/* ActorCritic.train / MFAC.train (algo/ac.py) for the actor-critic network above, f32, on the device: one gradient
 * over n contiguous rows in place, then one Adam step.  Shapes: those of mfx_acnet_create (view_floats <= 4096,
 * feature <= 256, 2 <= n_action <= 32, use_mf).
 * The handle owns three blobs in the layout of mfx_acnet_blob_size -- the parameters and Adam's m and v -- and the
 * step count.  Padding entries of every blob (K rows past V / F / A, policy columns past A, value columns 1..15) stay
 * +0 for ever.  The trained parameters can go to mfx_acnet_set_weights device to device.
 * Rows: mfx_actrain_rows, n >= 1 rows each (row offsets are 64-bit); ret is the reward column after mfx_chain_returns /
 * mfx_mfac_returns (the bootstrap value and the returns are not this step's).
 * Forward: the f32 network of acnet_kernels.hip (tests/acnet_ref.py).  Loss, with means over all n rows:
 *   adv = ret - v (a constant); p = clamp(softmax(z), 1e-10f, 1 - 1e-10f), z = Wp (d / 0.1) + bp; lp = log(p + 1e-6f);
 *   L = -mean(adv lp[a]) + value_coef mean((ret - v)^2) + ent_coef mean(sum_k p_k lp_k).
 * Backward: dL/dv = -2 value_coef (ret - v) / n; dL/dp_k = (-adv [k = a] / (p_a + 1e-6) + ent_coef (lp_k + p_k / (p_k +
 * 1e-6))) / n where the softmax output lies in the clamp's closed interval, else 0 (torch's clamp backward; the bounds
 * are their f32 values, and float32(1 - 1e-10) = 1, so only the lower bound ever masks); dL/dz_k = s_k (dL/dp_k - sum_j
 * s_j dL/dp_j); the / 0.1 of the forward is a / 0.1 in the backward; ReLU masks are (kept post-activation value > 0).
 *   set_hyper        defaults: lr 1e-4, betas 0.9 / 0.999, eps 1e-8 (torch's Adam), value_coef 0.1, ent_coef 0.08; eps
 *                    must be > 0 (an entry whose g, m and v are all zero divides by it and must stay zero)
 *   set/get_state    `which` = MFX_ACTRAIN_PARAMS / ADAM_M / ADAM_V; n_floats must be the blob size; a copy on `stream`.
 *                    Setting the parameters leaves the moments and the step count alone.
 *   reset_optimizer  zeroes m, v and the step count
 *   step_count       steps applied (host copy; exact after mfx_actrain_error)
 *   set_input_support  mask[n] (n = view_floats) or null, the meaning and the caller's contract of
 *                    mfx_acnet_set_input_support: the view layer's forward and its weight gradient run over the supported
 *                    inputs only; gradient rows of unsupported inputs are +0; with the unsupported inputs zero the result
 *                    is bit-identical to the dense one.  Synchronises `stream`.
 *   set_chunk_rows   rows per chunk, 1 .. 262144 (0: the default, 12288 -- 137 MB of scratch for the kept activations
 *                    and the backward intermediates at 11 KB per row, plus 24 partial gradient blobs).  Each chunk's
 *                    weight-gradient partials are added into the gradient blob in chunk order.
 *   set_advantage    d_adv: a float32 column of n rows, or null (the default).  Host state, read by the grads / step
 *                    calls that follow: with a column, adv of the policy term is d_adv[i] (mfx_chain_gae's, opt-in,
 *                    DESIGN 7q) where the default forms ret - v; the value term and dL/dv use ret - v either way, ret
 *                    being the reward column after the walk.  The column must stay valid until those calls have run.
 *                    Null restores the default, bit for bit a fresh handle's.  mfx_actrain_rows is unchanged.
 *   set_ppo          d_logp_old: a float32 column of n rows, or null (the default).  Host state, read by the grads / step
 *                    calls that follow (opt-in; tests/ppo_ref.py restates it): with a column the policy term
 *                    is PPO's clipped surrogate.  Per row, in f32 with no contraction, lp = log(p_a + 1e-6f) as above and
 *                    adv = the advantage column's entry:
 *                        d = lp - d_logp_old[i];  r = expf(d);  lo = (float)(1.0 - clip);  hi = (float)(1.0 + clip)
 *                        clipped = (adv > 0 && r > hi) || (adv < 0 && r < lo)     (strict: a row on the bound is not)
 *                        dL/dp_a gets -(adv r) / (p_a + 1e-6) / n where the default adds -adv / (p_a + 1e-6) / n, and
 *                                nothing when clipped;  the row's policy loss is -adv r, clipped: -adv (adv > 0 ? hi : lo)
 *                    The value term, dL/dv, the entropy term, the clamp's mask, the / n, the action check and the error
 *                    word are the default's; d_stats stays four floats (pg_loss the mean of the row terms above).  Two
 *                    more means over the call's n rows -- clip_frac, of clipped ? 1 : 0, and approx_kl, of (r - 1) - d
 *                    (the non-negative k3 estimate) -- are summed like the stats (per-workgroup partials in index order,
 *                    in double) into two device floats the handle owns.  d_logp_new (may be null): lp is stored there per
 *                    row.  clip must be finite and > 0 (NaN is refused), before any launch; a grads / step call with
 *                    d_logp_old set and no advantage column is refused.  The columns must stay valid until those calls
 *                    have run.  Null d_logp_old restores the default, bit for bit a fresh handle's (clip and d_logp_new
 *                    are not read).
 *   ppo_stats        a device-to-device copy on `stream` of (clip_frac, approx_kl) of the last grads / step call made
 *                    with d_logp_old set, into d_out2 [2]; (0, 0) before any such call.  Nothing synchronises.
 *   grads           the gradient in blob layout (padding exactly zero) into d_grad_blob and (pg_loss, vf_loss, ent_loss,
 *                    mean value) -- vf_loss and ent_loss with their coefficients, as ActorCritic.train prints them -- into
 *                    d_stats (either may be null); no state changes; bit for bit the gradient step applies
 *   step             grads, then Adam (bias-corrected from the step count), enqueued by this one call; nothing is read
 *                    back, nothing synchronises
 *   error            synchronises `stream`; *code = 0 or MFX_ACTRAIN_BAD_ACTION (an action outside [0, n_action)) with
 *                    the offending value in *bad_value, and clears it.  The action is checked on the device before any
 *                    load that depends on it; a step with a bad action applies nothing (state and step count unchanged,
 *                    stats undefined), nor does any later one until this call has cleared the word.
 * No floating-point atomics, no grid barrier, no spin wait, no cooperative launch: every sum has one fixed order that
 * depends only on (n, chunk_rows, shape), so equal state, rows and chunk_rows give bitwise equal results.  All launches
 * go to `stream`; the row columns must stay valid until they have run. */
typedef struct mfx_actrain_rows {
    const float *obs;                     /* [n][view_floats] */
    const float *feat;                    /* [n][feature] */
    const int32_t *act;                   /* [n] */
    const float *ret;                     /* [n] */
    const float *prob;                    /* [n][n_action] (mean field), else null */
} mfx_actrain_rows;
enum { MFX_ACTRAIN_PARAMS = 0, MFX_ACTRAIN_ADAM_M = 1, MFX_ACTRAIN_ADAM_V = 2 };
enum { MFX_ACTRAIN_BAD_ACTION = 1 };
int mfx_actrain_create(int view_floats, int feature, int n_action, int use_mf, void **handle);
int mfx_actrain_destroy(void *handle);
int mfx_actrain_set_hyper(void *handle, double lr, double beta1, double beta2, double eps, double value_coef,
                          double ent_coef);
int mfx_actrain_set_state(void *handle, int which, const float *d_blob, size_t n_floats, void *stream);
int mfx_actrain_get_state(void *handle, int which, float *d_out, size_t n_floats, void *stream);
int mfx_actrain_reset_optimizer(void *handle, void *stream);
int mfx_actrain_step_count(void *handle, long long *t);
int mfx_actrain_set_input_support(void *handle, const uint8_t *mask, int n, void *stream);
int mfx_actrain_set_chunk_rows(void *handle, int chunk_rows);
int mfx_actrain_set_advantage(void *handle, const float *d_adv);
int mfx_actrain_set_ppo(void *handle, const float *d_logp_old, double clip, float *d_logp_new);
int mfx_actrain_ppo_stats(void *handle, float *d_out2, void *stream);
int mfx_actrain_grads(void *handle, const mfx_actrain_rows *rows, long long n, float *d_grad_blob, float *d_stats,
                      void *stream);
int mfx_actrain_step(void *handle, const mfx_actrain_rows *rows, long long n, float *d_stats, void *stream);
int mfx_actrain_error(void *handle, int *code, long long *bad_value, void *stream);

/* The behaviour log-probabilities of the PPO head (csrc/ppo_kernels.hip; opt-in): d_logp[i] = logf(d_policy[i
 * n_action + a] + 1e-6f) with a = d_act[i], for i < n.  d_policy: [n][n_action], the clamped policy mfx_acnet_forward
 * writes.  The action is checked before it selects anything: a row whose action is outside [0, n_action) reads nothing
 * from the policy and gets +0; the training step that follows on those rows reports it (MFX_ACTRAIN_BAD_ACTION) and
 * applies nothing.  n = 0 does nothing; n_action outside 2..32 is refused.  One lane per row: no atomics, nothing is
 * read back, equal input gives bitwise equal output. */
int mfx_policy_logp(const float *d_policy, const int32_t *d_act, long long n, int n_action, float *d_logp, void *stream);

/* ---------------------------------------------------------------- measurement */
/* The HBM write ceiling on this device, measured in-process beside the bench (csrc/diag_kernels.hip): total_bytes
 * of float4 stores over the device region [d_buf, d_buf + region_bytes), wrapping; shape 0..7: bit 0 = nontemporal
 * stores, bits 1-2 = 4 / 8 / 16 KiB chunks, one workgroup per chunk, or (3) 4 KiB chunks on a persistent grid;
 * *ms = HIP-event time (synchronises). */
int mfx_store_ceiling(void *d_buf, size_t region_bytes, size_t total_bytes, int shape, void *stream, float *ms);

/* ---------------------------------------------------------------- library */
const char *mfx_last_error(void);
const char *mfx_build_info(void);
int mfx_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* MAGENT_AMD_H */
