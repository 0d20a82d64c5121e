// battle_engine.h -- the Battle engine's host class, internal to csrc/battle_*.cpp.
//
// One class, defined over several translation units by job:
//   battle_engine.cpp   configuration, the reward DSL compiler, device state, the per-call device API
//   battle_rollout.cpp  the fused rollout: its plan (BattleEngine::Plan), the per-plan steps, the policy steps
//   battle_dropin.cpp   the env-0 host cache, the deferred / fast drop-in step, the resident server, host_*
//   battle_render.cpp   get_info, render and the recording helpers
//   battle_abi.cpp      the C ABI (include/magent_amd.h and the reference's runtime_api.h)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cstring>
#include <fstream>
#include <sstream>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "battle_kernels.h"
#include "battle_layout.h"
#include "mfx_common.h"
#include "../../include/magent_amd.h"

namespace mfx {

// LDS of one workgroup (gfx950: 160 KB a CU): what a kernel's image plus scratch must fit in for its plan to apply
constexpr size_t kLdsBytes = 160 * 1024;

// The queue kernels (k_rollout_bigq) hand work between the workgroups of one launch.  Each env lives on one XCD, an
// XCD's work of a launch completes with any one of the launch's workgroups resident there, and a workgroup leaves as
// soon as its XCD's work is done (rollout_big.inc xcd_done); the pipelined few-env form also claims stepper roles and
// takes back unclaimed items from waiting workgroups (few_rollout).  So neither needs its whole grid co-resident.
// The large-env form still runs one launch at a time per process and device (this lock: each such launch waits for
// the previous one's completion event on its device) -- its grid fills every CU, and two of them dispatched at once
// would split the chip between two copies of the same observation stream for no gain.
class BigqSerial {
  public:
    explicit BigqSerial(hipStream_t st) : st_(st), lock_(mu()) {
        if (hipGetDevice(&dev_) != hipSuccess || dev_ < 0 || dev_ >= kDevs) dev_ = -1;
        else if (has()[dev_]) err_ = hipStreamWaitEvent(st_, ev()[dev_], 0);
    }
    ~BigqSerial() {
        if (dev_ < 0) return;
        if (!ev()[dev_] && hipEventCreateWithFlags(&ev()[dev_], hipEventDisableTiming) != hipSuccess) return;
        if (hipEventRecord(ev()[dev_], st_) == hipSuccess) has()[dev_] = true;
    }
    hipError_t status() const { return err_; }

  private:
    static constexpr int kDevs = 64;
    static std::mutex& mu() { static std::mutex m; return m; }
    static hipEvent_t* ev() { static hipEvent_t e[kDevs] = {}; return e; }
    static bool* has() { static bool h[kDevs] = {}; return h; }
    hipStream_t st_;
    std::lock_guard<std::mutex> lock_;
    int dev_ = -1;
    hipError_t err_ = hipSuccess;
};

// ------------------------------------------------------------------ host-side ranges
struct HostRange {                                  // Range.h:14-113
    int w = 0, h = 0, count = 0, x1 = 0, y1 = 0, x2 = 0, y2 = 0;
    std::vector<uint8_t> in;
    std::vector<int> dx, dy;
};

struct AgentTypeSpec {                               // AgentType.cc:28-131
    std::string name;
    int width = 1, length = 1;
    float speed = 1, hp = 1, view_radius = 1, view_angle = 360, attack_radius = 0, attack_angle = 0;
    float hear_radius = 0, speak_radius = 0;
    int speak_ability = 0;
    float damage = 0, trace = 0, eat_ability = 0, step_recover = 0, kill_supply = 0, food_supply = 0;
    bool attack_in_group = false, can_absorb = false;
    float step_reward = 0, kill_reward = 0, dead_penalty = 0, attack_penalty = 0;
    HostRange view, attack, move;
    int turn_base = 0, attack_base = 0, n_action = 0;
};

// ------------------------------------------------------------------ the engine
class BattleEngine {
public:
    // --- configuration (GridWorld.cc:126-155)
    int W = 0, H = 0, emb = 0;
    bool minimap = false, food = false, turn = false, goal = false;
    bool large_map = false; int n_sep = 8;
    uint32_t rng_init = 1;                          // seed(0) -> state 1 (GridWorld.cc:31)
    std::map<std::string, AgentTypeSpec> types;
    std::vector<std::string> group_types;
    struct Sym { int group, index; };
    struct Node { int op; std::vector<int> raw; };
    struct Rule { int on; std::vector<int> recv; std::vector<float> val; bool terminal; };
    std::vector<Sym> syms; std::vector<Node> nodes; std::vector<Rule> rules;

    // --- device
    int E = 1;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool stream_set = false;                          // a caller-provided stream (may be the null stream)
    GameParams gp{};
    GameParams* d_gp = nullptr;
    State s{};
    uint32_t* d_sort = nullptr;
    int32_t* d_err = nullptr;
    bool allocated = false;
    // render (RenderGenerator.cc): config.json + video_<file>.txt frames of env 0
    std::string render_dir;
    int file_ct = 0, frame_ct = 0, frame_per_file = 10000;
    bool first_render = true;
    int max_ids = 0;                                 // upper bound of id_counter over envs
    std::vector<int> group_ub;                       // upper bound of grp_n per group
    int pending_ub = 0;                              // upper bound of queued actions
    int acts_since_step[kMaxGroups] = {};            // set_action calls per group since the last step
    // drop-in staging (env 0, host buffers)
    DevBuf<float> st_view, st_feat, st_f32;
    // Drop-in host cache (env 0).  The reference call sequence asks the same state many times per step
    // (get_num before every getter, both groups' observations, ids / rewards / alive of both groups);
    // every state change bumps `epoch`, and a getter fetches everything it may be asked next for the
    // current epoch in ONE device-to-host transfer into pinned memory with ONE stream sync: two syncs
    // per training-loop step (observations + ids before the actions, done + rewards / alive / positions
    // after the step) instead of one or two per call.
    uint64_t epoch = 1, n_ep = 0, obs_ep = 0, info_ep = 0;
    int hn[kMaxGroups] = {};                 // group sizes of env 0 (valid when n_ep == epoch)
    size_t obs_rows = 0, info_rows = 0;      // rows per group of the staging layouts below
    bool obs_packed = false;                 // one env: pin_obs holds views|features per group packed
    size_t obs_pack_off[kMaxGroups] = {};    //   at these float offsets
    DevBuf<uint8_t> st_info;                 // env 0's record (k_get_env0): header, then per group
                                             //   ids i32 | reward f32 | pos 2 x i32 | alive u8, x rows
    PinBuf<uint8_t> pin_obs, pin_info;       // host copies: views + features, info, in the same layouts
    PinBuf<int32_t> pin_act;                 // [G][rows] actions on their way to the device
    hipEvent_t act_ev[kMaxGroups] = {};      // that copy of group g has left pin_act
    const uint8_t* info_src = nullptr;       // the record the getters answer from (pin_info or pin_fast)
    size_t info_src_rows = 0;                //   and its rows per group
    // Fast drop-in step (k_dropin_step, battle/dropin.inc): set_action and clear_dead are deferred and
    // env.step() is ONE launch that also leaves the records of the post-step and post-clear_dead states
    // and the next observation in host-mapped memory.  Deferred work runs for real (flush_deferred)
    // before anything else reads or changes the device state.
    bool fast_enabled = env_flag("MFX_DROPIN_FAST", true);   // MFX_DROPIN_FAST=0: the per-call path (A/B, tests)
    bool defer_act[kMaxGroups] = {};         // group g's actions wait in pin_fact
    int defer_n[kMaxGroups] = {};
    bool defer_clear = false;                // clear_dead waits for the next k_dropin_step
    uint64_t spec_ep = 0;                    // epoch at which the step record / the observation blocks apply
    bool obs_fast = false;                   // the observation cache is pin_fast's blocks
    MappedBuf<uint8_t> pin_fast;             // rec_step | per group view block, feature block
    MappedBuf<int32_t> pin_fact;             // [G][fact_rows] deferred actions
    MappedBuf<uint32_t> pin_flag;            // [2] k_dropin_step's completion words (coherent)
    uint32_t fast_seq = 0;                   // sequence number of the last k_dropin_step request
    uint32_t obs_seq = 0;                    // the request whose observation the cache holds
    // Resident server (engines on their own stream, MFX_DROPIN_RESIDENT != 0): one k_dropin_step launch
    // keeps env 0 in LDS and answers every env.step() posted in the mailbox (battle_layout.h
    // DropinMailbox) -- no launch, no install per step.  It leaves after a stop request (quiesce(),
    // before anything else touches the stream or the state) or after res_idle_us without a request,
    // and is relaunched by the next step.
    bool res_enabled = env_flag("MFX_DROPIN_RESIDENT", true);
    bool res_live = false;                   // a server was launched and not asked to stop
    bool fast_res = false;                   // the last request went to the resident server
    int res_relaunch = 0;                    // relaunches after an idle exit (statistics)
    MappedBuf<DropinMailbox> mbox;
    uint32_t mail_tag[kMaxGroups] = {};      // tag of group g's actions in mbox->acts (~0: not there)
    size_t mail_stride[kMaxGroups] = {};     //   and the per-group stride they were written with
    DropinArgs res_da{};                     // the arguments of the live server (relaunch)
    size_t fast_rows = 0, fact_rows = 0;
    size_t fast_rec = 0, fast_view[kMaxGroups] = {}, fast_feat[kMaxGroups] = {}, fast_set_bytes = 0;
    std::vector<void*> retired;              // outgrown pin_fast blocks (views may outlive them), freed last
    std::vector<uint8_t> clr_rec;            // the record after a deferred clear_dead (host-built)
    DevBuf<int> st_i32, st_xs, st_ys, st_dirs;
    DevBuf<uint8_t> st_u8;
    // fused rollout (bench / throughput path)
    bool rollout_ready = false;
    // Which kernels rollout_step runs.  rollout_init chooses between the LDS-sized plans (Fused, Pipe) and the plans
    // with the state in HBM (the other three: envs too large for one workgroup's LDS, or few LDS-sized envs);
    // rollout_plan() decides everything else, afresh on every call, and keeps that choice.
    enum class Plan {
        Fused,                               // k_rollout
        Pipe,                                // k_rollout_obs + k_rollout (MFX_ROLLOUT_PIPE=1)
        BigStreams,                          // k_observe_items + k_rollout_big on two streams (MFX_BIG_FUSED=0)
        BigQueue,                            // k_rollout_bigq, in chunks of envs (default of the HBM plans)
        FewPipe,                             // k_rollout_bigq, pipelined: few LDS-sized envs (RolloutArgs::few_pipe)
    };
    Plan ro_plan = Plan::Fused;
    bool plan_hbm() const { return ro_plan != Plan::Fused && ro_plan != Plan::Pipe; }   // state in HBM (k_rollout_big*)
    bool plan_queue() const { return ro_plan == Plan::BigQueue || ro_plan == Plan::FewPipe; }   // k_rollout_bigq
    bool ro_small_e = false;                 // LDS-sized envs on the large-env path: few envs (kSmallEMax)
    RolloutArgs ra{};
    DevBuf<float> ro_view[kMaxGroups], ro_feat[kMaxGroups], ro_rewards, ro_return;
    DevBuf<float> ro_mm;                     // large envs: next observation's minimap   [E][G][169]
    DevBuf<uint32_t> ro_info;                //             and per-id hp/max | group     [E][cap]
    DevBuf<uint32_t> ro_sort;                //             band-ordered moves            [E][acap]
    DevBuf<uint32_t> ro_items;               //             observation work items        [2][E*G*slots]
    DevBuf<int32_t> ro_cnt;                  //             their counters                [split][2][2]
    int ro_item_grid = 0;                    //             persistent grid of k_observe_items
    // large envs, queue-driven (k_rollout_bigq, default): one launch per ro_sub steps of every env
    bool ro_queue_want = true;               // MFX_BIG_FUSED=0 at rollout_init: the two-stream pipeline (A/B)
    DevBuf<uint32_t> ro_q_items, ro_q_si;    // [2][kXcds][list cap] tagged items; [E] next step index
    DevBuf<uint8_t> ro_snap;                 // few_pipe: [E][2] observation snapshots
    DevBuf<int32_t> ro_q_step;               // few_pipe: [kXcds] stepper claims
    DevBuf<int32_t> ro_q_cnt, ro_q_left, ro_q_done;
    int ro_q_grid = 0, ro_qpar = 0;
    uint32_t ro_qlaunch = 0;                 // launches so far (item tags)
    // Large envs on the queue kernel (not pipelined): the envs run in ro_qchunks consecutive launches per block of
    // steps, each over one chunk of envs with queues of its own.  One launch over all envs slows past ~2048 envs at
    // 256x256 (0.80 of the HBM roofline at 2048, 0.77 at 2560, 0.71 at 3072, 0.62-0.64 at 4096, ~0.3 MB of env state
    // each); 4096 envs as two launches of 2048 run at 0.79, while 3072 as two of 1536 gain nothing (0.711 vs 0.714):
    // so the chunks are at least kBigqChunkBytes of state (2048 envs at 256x256) -- floor(state / kBigqChunkBytes)
    // of them (profiles/r05_bigq_chunks.txt).
    static constexpr int kMaxQChunks = 8;
    static constexpr size_t kBigqChunkBytes = (size_t)2048 * 312648;
    int ro_qchunks = 1;
    int ro_qc_e0[kMaxQChunks + 1] = {};
    int ro_qc_par[kMaxQChunks] = {};
    uint32_t ro_qc_launch[kMaxQChunks] = {};
    State ro_qc_s[kMaxQChunks];
    RolloutArgs ro_qc_ra[kMaxQChunks];
    DevBuf<RolloutCtx> ro_qc_ctx;
    static uint32_t qtag(uint32_t launch) { return launch % 63u + 1u; }   // 6 tag bits (rollout_big.inc), never 0
    bool ro_prep_stale = true;               // ro_mm / ro_info / items lag the state (per-call calls since)
    // A learned policy on the large-env plans (rollout_policy_step): all E envs as one batch on the engine's own
    // stream, k_observe_items (lists of kItemRows agents in ro_items / ro_cnt) + k_rollout_big<ext>.  Its args are its
    // own: on the queue plans, ra holds the queue kernel's rows per item and ro_sub_ra is cut from that.
    RolloutArgs ro_pol_ra{};
    DevBuf<RolloutCtx> ro_pol_ctx;
    int ro_pol_item_grid = 0;                // its k_observe_items grid: the launch has the chip to itself
    // whose observation inputs, item lists and parities are current: 0 rollout_step's form, 1 the policy form's.
    // The other form re-seeds on its next call, as after per-call calls (ro_prep_stale).
    int ro_prep_form = 0;
    DevBuf<int32_t> ro_actions, ro_eplen, ro_tx, ro_ty;
    DevBuf<int32_t> ro_ids;                  // [E][G][rowcap] ids / alive flags of the last policy step (RolloutArgs::ids)
    DevBuf<uint8_t> ro_alive;
    DevBuf<double> ro_mean, ro_stats;
    DevBuf<unsigned long long> ro_steps;
    DevBuf<int32_t> ro_work;                 // k_rollout work-queue counters (2)
    DevBuf<int32_t> ro_cls_cnt, ro_cls_list; // k_rollout work queue (weight-class lists)
    uint64_t ro_launch = 0;                  // launches so far (queue phase = ro_launch % 6)
    DevBuf<uint4> ro_image;                  // reset image (k_reset_image)
    DevBuf<uint4> ro_walls;                  // its cells without the agents (RolloutArgs::wall_image)
    bool cells_stale = false;                // State::cells lags the fused rollout (sync_cells)
    bool walls_after_init = false;           // walls added after rollout_init: not in the rollout's cells
    DevBuf<RolloutCtx> ro_ctx;               // device copy of {s, ra} read by k_rollout
    RolloutCtx ro_ctx_host{};
    int ro_grid = 0, ro_cap = 0;
    // fused rollout: consecutive steps of each env per k_rollout launch (env image kept in LDS between
    // them; the launch's ramp-up / tail and the install / write-back are paid once per ro_sub steps)
    int ro_sub = 1;                          // 0: chosen per path and batch (sub_steps)
    // large-env path: the envs split into ro_split independent sub-batches, each a pipeline
    // (k_observe_items -> k_rollout_big) on its own stream, so one sub-batch's latency-bound step
    // overlaps the other's HBM-bound observation.  Each item launch takes a third of the chip's
    // k_observe_items slots, leaving room for the other stream's step.  Measured at 256x256 / 4096
    // agents, 1024 envs (profiles/r01_big_sweeps.txt): 2 streams / 1/3 grid / 64-agent items best.
    static constexpr int kBigSplit = 2, kItemGridDiv = 3, kItemRows = 64;
    static constexpr int kBigqRows = 512;         // agents per k_rollout_bigq observation item (64: 9.6e8, 256: 1.06e9, 384-512: 1.08e9, 1024: 1.04e9; profiles/r02_bigq_sweeps.txt)
    static constexpr bool kPipeDefault = false;   // measured slower than the fused step
    // Batches of at most kSmallEMax LDS-sized envs run on k_rollout_bigq (64x64 / 256 agents, one MI355X,
    // profiles/r03_small_e_sweep.txt, r03_crossover.txt): 8 envs 0.0435 vs 0.0944 ms per step (k_rollout),
    // 64 envs 0.050 vs 0.121, 1024 envs 3.00e8 vs 2.59e8 agent-steps/s; k_rollout wins from 2048 envs on
    // (4.0e8 vs 3.2e8).  16-agent items: 0.0435 ms per step at 8 envs vs 0.0461 (32), 0.0497 (64), 0.0441 (8).
    static constexpr int kSmallEMax = 1024;
    static constexpr int kSmallERows = 16;
    // the pipelined few-env stepper: wave 0 alone steps envs of up to this many agents (k_rollout's threshold)
    static constexpr int kFewWaveMax = 64;
    // steps per launch: at most 64 (k_rollout, the queue kernel's item lists); the pipelined few-env form's lists
    // are sized for kMaxPipeSub (its item words' 6 step bits only guard the hand-off, modulo 64)
    static constexpr int kMaxSub = 64, kMaxPipeSub = 1024;
    static constexpr int kPipeStepPerCu = 4, kPipeObsPerCu = 2;
    int ro_split = kBigSplit;
    hipStream_t ro_str[kMaxSplit] = {};
    hipEvent_t ro_ev[kMaxSplit + 1] = {};
    State ro_sub_s[kMaxSplit];
    RolloutArgs ro_sub_ra[kMaxSplit];
    int ro_sub_n[kMaxSplit] = {};            // envs of sub-batch k
    int sub_envs(int k) const { return ro_sub_n[k]; }
    DevBuf<RolloutCtx> ro_sub_ctx;
    // observation/step pipeline (LDS-sized envs): k_rollout_obs on ro_str[0] observes every env
    // from one copy of the per-env state while k_rollout<.., kSplit> steps the same envs from it
    // and writes the other copy (tw); the copies trade places after every launch.
    State tw{};                              // the other copy (the kTwin fields below)
    int tw_cap = -1, tw_E = -1;
    int ro_par = 0;                          // 0: s is ro_twin_ctx[0].s
    int ro_obs_grid = 0;
    DevBuf<RolloutCtx> ro_twin_ctx;          // [2]: {s, ra, tw} and {tw, ra, s} as planned
    RolloutCtx ro_twin_host[2] = {};
    ~BattleEngine();
    void release();

    int n_groups() const { return (int)group_types.size(); }
    AgentTypeSpec& gtype(int g) { return types.at(group_types.at(g)); }
    int group2channel(int g) const { return (food ? 2 : 1) + g * (minimap ? 3 : 2); }
    int feature_size(int g) {
        int f = emb + gtype(g).n_action + 1;
        if (goal) f += 2;
        if (minimap) f += 2;
        return f;
    }

    // ---- battle_engine.cpp: configuration, the reward DSL, device state, the per-call device API
    int set_config(const char* key, void* p);
    int register_type(const char* name, int n, const char** keys, const float* values);
    int new_group(const char* type_name, int* group);
    bool simple_rule(const Rule& R) const;
    int node_symbols(int ni, std::set<int>& rel, std::map<int, int>& infer, int depth) const;
    int post_order(int ni, std::vector<int>& out, int depth) const;
    int compile_dsl(DslProgram& P) const;
    int build_params();
    template <class T> static void alloc(T*& ptr, size_t n) {
        MFX_HIP_THROW(hipMalloc(&ptr, sizeof(T) * std::max<size_t>(n, 1)));
    }
    // (Re)allocate per-agent arrays with a new capacity, preserving contents row by row.
    template <class T> void grow(T*& ptr, size_t rows, size_t old_cap, size_t new_cap) {
        T* np;
        alloc(np, rows * new_cap);
        if (ptr && old_cap)
            MFX_HIP_THROW(hipMemcpy2DAsync(np, new_cap * sizeof(T), ptr, old_cap * sizeof(T), old_cap * sizeof(T),
                                           rows, hipMemcpyDeviceToDevice, stream));
        MFX_HIP_THROW(hipStreamSynchronize(stream));
        if (ptr) (void)hipFree(ptr);
        ptr = np;
    }
    void ensure_capacity(int need_ids, int need_actions);
    int reset();
    int add_agents(int group, int n, const char* method, const int* xs, const int* ys, const int* dirs);
    int set_goal(int group, const char* method);
    int check_err();
    void touch() { ++epoch; }                // any state change of env 0 (drop-in host cache)
    int report_err(int32_t h);
    int sync_cells();
    int observe(int g, float* d_view, float* d_feat, int rowcap);
    int set_action(int g, const int* d_actions, int rowcap);
    void begin_step();
    int step(int* d_done);
    int get(int g, int what, void* d_out, int rowcap);
    int clear_dead();

    // ---- battle_rollout.cpp: the fused rollout
    State sub_state(int e0, int n) const;
    RolloutArgs env_args(int e0) const;
    RolloutArgs stream_args(int e0, int k) const;
    RolloutArgs chunk_args(int e0, int k) const;
    size_t env_state_bytes() const;
    // The per-env fields k_rollout reads and writes back (the pipeline keeps two copies of them).
    template <class F> static void twin_fields(State& a, State& b, F&& f) {
        f(a.xy, b.xy); f(a.hp, b.hp); f(a.next_r, b.next_r); f(a.last_r, b.last_r); f(a.last_act, b.last_act);
        f(a.op_obj, b.op_obj); f(a.meta, b.meta); f(a.grp_ids, b.grp_ids); f(a.grp_n, b.grp_n);
        f(a.grp_dead, b.grp_dead); f(a.grp_reward, b.grp_reward); f(a.id_counter, b.id_counter); f(a.rng, b.rng);
    }
    void free_twin();
    void alloc_twin();
    State twin_state() const;
    void swap_twin();
    int rollout_init(const int* tmpl_n, const int* const* xs, const int* const* ys, int max_steps, float eps,
                     uint32_t seed, int stagger);
    int rollout_plan();
    void plan_prologue();
    void plan_big_lists();
    Plan plan_big_queue();
    void plan_big_batches();
    void plan_twin();
    int replan_if_moved();
    int observe_groups(const State& q, const RolloutArgs& qa, hipStream_t st);
    int rollout_step(int n_steps);
    int step_fused(int n_steps);
    int step_pipe(int n_steps);
    int step_big_streams(int n_steps);
    int step_big_queue(int n_steps);
    int step_few_pipe(int n_steps);
    int rollout_policy_step(int mode);
    int rollout_policy_big(int mode);
    int rollout_policy_path() const;
    int rollout_check();
    int rollout_path() const;
    int sub_steps() const;
    void set_sub_steps(int n_sub) { ro_sub = n_sub; }
    bool has_rollout() const { return rollout_ready; }
    int rollout_rowcap() const { return ra.rowcap; }
    int rollout_mean_stride() const { return ra.mean_stride; }
    int rollout_sum_lanes(int n) const;
    int rollout_info(int* grid, int* lds_bytes);
    int rollout_buffer(const char* name, int group, void** ptr, size_t* bytes);

    // ---- battle_dropin.cpp: the env-0 host cache, the fast step, the resident server, host_*
    // env 0's record (k_get_env0): 64-B header (group sizes, error word, done), then per group
    // ids | rewards | positions | alive, info_rows rows each
    static constexpr size_t kInfoRowBytes = 4 + 4 + 8 + 1;
    size_t info_region() const { return ((info_rows * kInfoRowBytes) + 15) & ~(size_t)15; }
    size_t info_off(int g, int what) const;
    const int32_t* info_hdr() const { return reinterpret_cast<const int32_t*>(info_src); }
    int queue_info();
    int take_info(const uint8_t* src = nullptr, size_t rows = 0);
    int ensure_info();
    int ensure_counts() { return n_ep == epoch ? 0 : ensure_info(); }
    int num_env0(int g);
    size_t obs_off_view(int g) const { return (size_t)g * obs_rows * obs_row_bytes(); }
    size_t obs_row_bytes() const;
    int ensure_obs();
    size_t fast_rows_now() const;
    bool fast_dropin_ok() const;
    int ensure_mbox();
    int quiesce();
    int flush_deferred();
    int fast_set_action(int g, const int* actions);
#ifdef MFX_STAMPS
    // diagnostic build: host-side split of env.step() (enter -> request posted -> record seen -> return)
    double hst[3] = {0, 0, 0};
    long hst_n = 0;
    std::chrono::steady_clock::time_point hst_t0, hst_t1;
#endif
    int fast_step(int* done);
    int wait_fast(int which, uint32_t seq);
    static int res_variant();
    static long long res_idle_us();
    unsigned long long res_idle_ticks() const;
    int fast_clear_dead();
    int host_observe(int g, float** bufs);
    int observation_view(int g, float** view, float** feat, int* n, int* rows);
    int host_set_action(int g, const int* actions);
    int host_step(int* done);
    int host_clear_dead();
    int host_get(int g, int what, void* out, size_t elem_bytes);
    int get_rows(int g, int what, void* out, int cap);

    // ---- battle_render.cpp: get_info, render, the recording helpers
    int get_info(int group, const char* name, void* buf);
    void next_file() { file_ct++; frame_ct = 0; }
    void start_recording();
    std::vector<int> attack_events();
    void gen_config();
    int render();
    std::vector<int> group_pos(int g);
    int mean_info(int group, float* out);
    int get_info_global(int group, const char* name, void* buf);
};

}  // namespace mfx
