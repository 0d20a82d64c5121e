// Part of battle_kernels.hip (one translation unit; included in order, not compiled alone):
// the fused rollout step k_rollout (and the pipeline's k_rollout_obs)
// ==================================================================================
//  fused rollout step: the whole reference training-loop step for one env per workgroup,
//  env state resident in LDS for the duration of the launch (senario_battle.play :96-171:
//  get_observation x G -> policy -> set_action x G -> step -> get_reward -> mean action ->
//  clear_dead, plus episode restart at done / max_steps).
// ==================================================================================
__device__ __forceinline__ uint32_t mix32(uint32_t h) {      // murmur3 finalizer
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// Synthetic rush policy of SURVEY.md 8(d) (tests/battle_driver.rush_policy): attack the
// first attack cell (index order = view2attack row-major order) holding an enemy, else move
// 2 cells toward the map centre; with probability eps a uniform random action instead.
// The synthetic rush policy (SURVEY.md 8(d)): attack the first enemy among the attack cells in
// view2attack order, else advance +-2 in x toward the centre; with probability eps a uniform
// action.  The group index is lane-varying, so the type fields come from the LDS table, and the
// attack cells are read 8 at a time (independent LDS reads instead of a dependent chain).
__device__ __forceinline__ int rush_action(const GameParams& gp, const SerialType& S, const EnvView& v, int g,
                                           int id, uint32_t key, float eps) {
    const uint32_t p = v.xy[id];
    const int x = p & 0xFFFF, y = p >> 16, W = gp.W, H = gp.H;
    int a = 2 * x < W ? 8 : 4;               // (float)x / W < 0.5f exactly: x, W < 2^16, so x / W is 1 / 2W off 0.5
    if (a >= S.turn_base) a = S.turn_base - 1;
    const int bx = x + S.att_x_off, by = y + S.att_y_off, na = S.n_attack;
    for (int k0 = 0; k0 < na; k0 += 8) {
        uint32_t c[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = k0 + j;
            const int ox = bx + S.att_dx[k], oy = by + S.att_dy[k];
            const bool in = k < na && ox >= 0 && oy >= 0 && ox < W && oy < H;
            const uint32_t cv = v.cells[in ? oy * W + ox : 0];
            c[j] = in ? cv : kCellEmpty;
        }
        int hit = -1;
#pragma unroll
        for (int j = 7; j >= 0; --j) {
            const uint32_t m = v.meta[c[j] < kCellFood ? c[j] : 0u];
            if (c[j] < kCellFood && (int)meta_group(m) != g) hit = k0 + j;
        }
        if (hit >= 0) { a = S.attack_base + hit; break; }
    }
    const uint32_t h = mix32(key);
    if ((float)(h >> 8) * (1.0f / 16777216.0f) < eps) a = (int)(mix32(h ^ 0x68E31DA4u) % (uint32_t)S.n_action);
    return a;
}

// Fixed-order workgroup sum in two barriers: butterfly within each wave, then the wave partials in
// wave order (red: one float per wave).
__device__ __forceinline__ float block_sum_waves(float x, float* red) {
    const int nw = blockDim.x >> 6;
    x = wave_sum(x);
    if ((TID & 63) == 0) red[TID >> 6] = x;
    __syncthreads();
    float r = 0.0f;
    for (int w = 0; w < nw; ++w) r += red[w];
    __syncthreads();
    return r;
}

#ifndef MFX_ROLLOUT_THREADS
#define MFX_ROLLOUT_THREADS 256
#endif
#ifndef MFX_ROLLOUT_OCC
#define MFX_ROLLOUT_OCC 5          // workgroups per CU the register budget is sized for
#endif
// LDS plan of k_rollout: the env (cells, per-id arrays, group lists) stays resident for the whole
// launch; one scratch region is shared by the observation phase (minimap, bins, hp/max, staging) and
// the policy/step phase (actions, histogram, attack/move buffers; the reduction reuses the actions).
struct RolloutUnion { size_t act, ahist, atk, mov, sorted, red, par, total; };

__host__ __device__ inline RolloutUnion rollout_union(const GameParams& gp, int cap, int acap, int threads) {
    auto r16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    RolloutUnion u;
    size_t o = 0;
    u.act = o;    o += r16((size_t)(gp.n_groups * cap > threads ? gp.n_groups * cap : threads) * 4);
    u.red = u.act;                                 // block_sum after the step: the actions are dead
    u.ahist = o;  o += r16((size_t)gp.n_groups * 64 * 4);
    u.atk = o;    o += r16((size_t)acap * 4);
    u.mov = o;    o += r16((size_t)acap * 4);
    u.sorted = o; o += gp.large_map ? r16((size_t)acap * 4) : 0;
    // the step scratch: ParScratch (wave-team / small-n forms) or BigScratch in its compact form
    // (attack_big / move_jump for the whole-workgroup team), never both in one step
    const size_t pb = par_scratch_bytes(acap, cap), bb = big_scratch_bytes(acap, cap, false);
    u.par = o;    o += gp.par_step ? r16(pb > bb ? pb : bb) : 0;
    u.total = o;
    return u;
}

__host__ __device__ inline size_t rollout_scratch_bytes(const GameParams& gp, int cap, int acap, int rows, int threads,
                                                        bool kB) {
    // (Battle shape: the agent records of every group at once, rollout_observe_groups)
    const size_t obs = obs_smem_core(gp, 0, cap, rows * (kB ? gp.n_groups : 1), obs_stage_floats(gp, 0, kB, threads), kB);
    const size_t stp = rollout_union(gp, cap, acap, threads).total;
    return obs > stp ? obs : stp;
}

// Bytes of the resident env image in LDS: cells, the seven per-id arrays, the group lists.  The
// same layout is used for the reset image in HBM (RolloutArgs::reset_image).
__host__ __device__ inline size_t env_image_bytes(int cells_n, int cap, int G) {
    auto r16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    return r16((size_t)cells_n * 2) + 5 * r16((size_t)cap * 4) + 2 * r16(cap) + r16((size_t)G * cap * 2);
}

#ifndef MFX_LDS_PAD
#define MFX_LDS_PAD 0              // experiments only: extra dynamic LDS per workgroup (lowers occupancy)
#endif
// env image | scratch union | StepSmem (G type entries)
__host__ __device__ inline size_t rollout_main_bytes(const GameParams& gp, int cells_n, int cap, int acap, int rows,
                                                     bool kB) {
    return env_image_bytes(cells_n, cap, gp.n_groups) +
           rollout_scratch_bytes(gp, cap, acap, rows, MFX_ROLLOUT_THREADS, kB);
}

size_t rollout_smem_bytes(const GameParams& gp, int cells_n, int cap, int acap, int rows) {
    return rollout_main_bytes(gp, cells_n, cap, acap, rows, is_battle_shape(gp)) + step_sm_bytes(gp.n_groups) +
           MFX_LDS_PAD;
}

size_t rollout_reset_image_bytes(const GameParams& gp, int cells_n, int cap) {
    return env_image_bytes(cells_n, cap, gp.n_groups) + 64;
}

// Carve the env image out of LDS (or any base) in the layout above.
__device__ __forceinline__ EnvView carve_env(char* base, int cells_n, int cap, int G) {
    size_t off = 0;
    auto carve = [&](size_t bytes) { char* p = base + off; off += (bytes + 15) & ~(size_t)15; return p; };
    EnvView v;
    v.cap = cap;
    v.cells = reinterpret_cast<uint16_t*>(carve((size_t)cells_n * 2));
    v.xy = reinterpret_cast<uint32_t*>(carve((size_t)cap * 4));
    v.hp = reinterpret_cast<float*>(carve((size_t)cap * 4));
    v.next_r = reinterpret_cast<float*>(carve((size_t)cap * 4));
    v.last_r = reinterpret_cast<float*>(carve((size_t)cap * 4));
    v.op_obj = reinterpret_cast<int32_t*>(carve((size_t)cap * 4));
    v.last_act = reinterpret_cast<uint8_t*>(carve((size_t)cap));
    v.meta = reinterpret_cast<uint8_t*>(carve((size_t)cap));
    v.grp_ids = reinterpret_cast<uint16_t*>(carve((size_t)G * cap * 2));
    v.rid = nullptr;                     // images are never renumbered: slot == id
    return v;
}

__device__ __forceinline__ void copy16(void* dst, const void* src, size_t bytes) {   // 16-B aligned, bytes % 16 == 0
    uint4* d = reinterpret_cast<uint4*>(dst);
    const uint4* q = reinterpret_cast<const uint4*>(src);
    for (size_t i = TID; i < (bytes >> 4); i += blockDim.x) d[i] = q[i];
}

// env.reset() + add_agents(custom) of the template (GridWorld.cc:76-124, Map.cc:23-47, 200-247),
// computed once per rollout_init by one workgroup; k_rollout copies it in at every episode start.
// in_lds 0: built in place in HBM (images larger than LDS, the k_rollout_big path).
__global__ void __launch_bounds__(256) k_reset_image(const GameParams* __restrict__ gpp, int cells_n, int cap,
                                                     RolloutArgs ra, uint4* __restrict__ image, int in_lds) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int scal[8];
    const GameParams& gp = *gpp;
    const int G = gp.n_groups, W = gp.W, H = gp.H;
    char* base = in_lds ? smem : reinterpret_cast<char*>(image);
    EnvView v = carve_env(base, cells_n, cap, G);
    const size_t bytes = env_image_bytes(cells_n, cap, G);
    for (size_t i = TID; i < bytes / 4; i += blockDim.x) reinterpret_cast<uint32_t*>(base)[i] = 0;
    __syncthreads();
    for (int c = TID; c < W * H; c += blockDim.x) {
        const int x = c % W, y = c / W;
        v.cells[c] = (x == 0 || y == 0 || x == W - 1 || y == H - 1) ? kCellWall : kCellEmpty;
    }
    __syncthreads();
    if (TID == 0) {
        int idc = 0;
        for (int g = 0; g < kMaxGroups; ++g) scal[g] = 0;
        for (int g = 0; g < G; ++g) {
            const TypeParams& T = gp.type[g];
            for (int i = 0; i < ra.tmpl_n[g]; ++i) {
                const int x = ra.tmpl_x[g * ra.tmpl_cap + i], y = ra.tmpl_y[g * ra.tmpl_cap + i];
                if (!is_blank(v.cells, W, H, x, y, -1) || idc >= cap) continue;
                const int id = idc++;
                v.cells[y * W + x] = (uint16_t)id;
                v.xy[id] = (uint32_t)x | ((uint32_t)y << 16);
                v.hp[id] = T.hp; v.last_r[id] = 0.0f; v.next_r[id] = T.step_reward;
                v.last_act[id] = T.n_action; v.op_obj[id] = -1;
                v.meta[id] = (uint8_t)meta_make(0, kOpNull, g);
                v.grp_ids[g * cap + scal[g]++] = (uint16_t)id;
            }
        }
        scal[4] = idc;
        for (int k = 5; k < 8; ++k) scal[k] = 0;
    }
    __syncthreads();
    if (in_lds) copy16(image, smem, bytes);
    if (TID < 8) reinterpret_cast<int32_t*>(reinterpret_cast<char*>(image) + bytes)[TID] = scal[TID];
}

// Per-env scalars of k_rollout, held in LDS while the env is resident.  Word w of this struct is
// loaded / stored by lane w (addresses from PfTable).
struct EnvScalars {
    int32_t grp_n[kMaxGroups];          // words 0-3
    int32_t grp_dead[kMaxGroups];       // 4-7
    float grp_reward[kMaxGroups];       // 8-11
    float ep_return[kMaxGroups];        // 12-15
    int32_t id_counter;                 // 16
    uint32_t rng;                       // 17
    int32_t ep_len;                     // 18
    int32_t pad;                        // 19
    double stats[4];                    // 20-27
    unsigned long long agent_steps;     // 28-29
};
constexpr int kScalarWords = 30;

// Register prefetch of one env (k_rollout fast path): while env e is processed, every lane of
// waves 0-2 holds its share of env e+1's image (up to 5 rows of 16 B; wave 0 also one scalar word),
// so the next install is LDS stores only.  Wave 3 alone writes env e back: a wave's vmcnt is in
// order, so the prefetch waves must not have the write-back stores queued ahead of their loads.
// The image's 16-B rows are numbered in LDS order: the cells (nc16 rows), then
// [xy hp next_r last_r op_obj] (c4 = cap/4 rows each), [last_act] [meta] (c4/4 each), [grp_ids] (G*c4/2).
constexpr int kPfLanes = MFX_ROLLOUT_THREADS - 64; // every wave but the last
constexpr int kPfSlots = 5;
constexpr int kPfRows = kPfSlots * kPfLanes;
constexpr int kWbWave = MFX_ROLLOUT_THREADS / 64 - 1;   // the write-back wave

__host__ __device__ inline int image_small_rows(int c4, int G) { return 5 * c4 + 2 * (c4 >> 2) + G * (c4 >> 1); }

struct EnvPrefetch {
    uint4 r[kPfSlots];
    uint32_t w;
};

// Address plan of the env image, built once per workgroup in LDS: for each source array (the six
// 4-byte per-id arrays, meta, grp_ids) and each EnvScalars word, the env-0 address and the bytes
// per env.  A prefetch row is then ONE load from base + e * stride + offset; choosing among
// separate pointers per lane instead would serialise the loads (each predicated load into the same
// registers waits for the previous one).
struct PfTable {
    unsigned long long walls;           // RolloutArgs::wall_image (cells rows, shared by every env)
    unsigned long long base[8];         // xy hp next_r last_r op_obj, last_act, meta, grp_ids
    unsigned int stride[8];
    unsigned long long sbase[32];       // 0: word absent (group >= G, padding)
    unsigned int sstride[32];
};

__device__ __forceinline__ void pf_table_init(PfTable& pt, const State& s, const RolloutArgs& ra, int G) {
    const int t = TID;
    const unsigned cap4 = (unsigned)s.cap * 4u;
    if (t == 0) pt.walls = (unsigned long long)ra.wall_image;
    if (t < 8) {
        const void* p = nullptr;
        unsigned st = cap4;
        if (t == 0) p = s.xy;
        if (t == 1) p = s.hp;
        if (t == 2) p = s.next_r;
        if (t == 3) p = s.last_r;
        if (t == 4) p = s.op_obj;
        if (t == 5) { p = s.last_act; st = (unsigned)s.cap; }
        if (t == 6) { p = s.meta; st = (unsigned)s.cap; }
        if (t == 7) { p = s.grp_ids; st = (unsigned)s.cap * 2u * (unsigned)G; }
        pt.base[t] = (unsigned long long)p;
        pt.stride[t] = st;
    }
    if (t < 32) {
        const int g = t & 3;
        const char* p = nullptr;
        unsigned st = 4;
        if (t < 16 && g < G) {
            st = 4u * (unsigned)G;
            if ((t >> 2) == 0) p = reinterpret_cast<const char*>(s.grp_n + g);
            if ((t >> 2) == 1) p = reinterpret_cast<const char*>(s.grp_dead + g);
            if ((t >> 2) == 2) p = reinterpret_cast<const char*>(s.grp_reward + g);
            if ((t >> 2) == 3) p = reinterpret_cast<const char*>(ra.ep_return + g);
        }
        if (t == 16) p = reinterpret_cast<const char*>(s.id_counter);
        if (t == 17) p = reinterpret_cast<const char*>(s.rng);
        if (t == 18) p = reinterpret_cast<const char*>(ra.ep_len);
        if (t >= 20 && t < 28) { p = reinterpret_cast<const char*>(ra.stats) + 4 * (t - 20); st = 32; }
        if (t >= 28 && t < 30) { p = reinterpret_cast<const char*>(ra.agent_steps) + 4 * (t - 28); st = 8; }
        pt.sbase[t] = (unsigned long long)p;
        pt.sstride[t] = st;
    }
}

// Table addresses are integers: cast them to the GLOBAL address space.  A generic pointer would
// make these flat_load / flat_store, which also count in lgkmcnt, so every later LDS wait would
// wait for the HBM round trip too.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u32x4 g_u32x4;
typedef __attribute__((address_space(1))) uint32_t g_u32;

__device__ __forceinline__ uint4 ld_g16(const g_u32x4* p) {
#ifdef MFX_NT_LD
    const u32x4 x = __builtin_nontemporal_load(p);
#else
    const u32x4 x = *p;
#endif
    return make_uint4(x.x, x.y, x.z, x.w);
}

// Address of 16-B row k of the per-id / group-list part of env e's image (LDS order, see EnvPrefetch).
__device__ __forceinline__ const g_u32x4* small_row_addr(const PfTable& pt, int e, int k, int sh, int c4) {
    const int j = k >> sh, k2 = k - 5 * c4, q = c4 >> 2;
    const int a = j < 5 ? j : (k2 < q ? 5 : (k2 < 2 * q ? 6 : 7));
    const int r = j < 5 ? (k & (c4 - 1)) : (k2 < q ? k2 : (k2 < 2 * q ? k2 - q : k2 - 2 * q));
    return (const g_u32x4*)(pt.base[a] + (unsigned long long)e * pt.stride[a] + (unsigned)r * 16u);
}

// Address of row r of env e's whole image: the cells first, then the small part.
__device__ __forceinline__ const g_u32x4* image_row_addr(const PfTable& pt, const State& s, int e, int r, int nc16,
                                                         int sh, int c4) {
    const unsigned long long cells = pt.walls + (unsigned)r * 16u;            // walls only (L2-resident)
    return r < nc16 ? (const g_u32x4*)cells : small_row_addr(pt, e, r - nc16, sh, c4);
}

__device__ __forceinline__ g_u32* scalar_addr(const PfTable& pt, int e, int w) {
    const unsigned long long b = pt.sbase[w];
    return b ? (g_u32*)(b + (unsigned long long)e * pt.sstride[w]) : nullptr;
}

__device__ __forceinline__ uint32_t load_scalar_word(const PfTable& pt, int e, int w) {
    const g_u32* p = scalar_addr(pt, e, w);
    return p ? *p : 0u;
}

__device__ __forceinline__ void pf_issue(EnvPrefetch& pf, const PfTable& pt, const State& s, int e, int nrows,
                                         int nc16, int sh, int c4) {
    const int t = TID;
    if (t >= kPfLanes) return;
#pragma unroll
    for (int j = 0; j < kPfSlots; ++j) {
        const int r = t + j * kPfLanes;
        if (r < nrows) pf.r[j] = ld_g16(image_row_addr(pt, s, e, r, nc16, sh, c4));
    }
    if (t < kScalarWords) pf.w = load_scalar_word(pt, e, t);
}

__device__ __forceinline__ void pf_install(const EnvPrefetch& pf, char* image, EnvScalars& sc, int nrows) {
    // One unconditional vmcnt(0) (gfx9 encoding: vmcnt 0, expcnt 7, lgkmcnt 15).  Left to the
    // compiler, the waits sit inside the exec-masked stores below, so along the skipped paths the
    // registers still look in flight and the next pf_issue waits again before every load.
    __builtin_amdgcn_s_waitcnt(0x0F70);
    const int t = TID;
    if (t >= kPfLanes) return;
    uint4* d = reinterpret_cast<uint4*>(image);
#pragma unroll
    for (int j = 0; j < kPfSlots; ++j) {
        const int r = t + j * kPfLanes;
        if (r < nrows) d[r] = pf.r[j];
    }
    if (t < kScalarWords) reinterpret_cast<uint32_t*>(&sc)[t] = pf.w;
}

// 16-B copy by one wave (lane stride 64).
__device__ __forceinline__ void wcopy16(void* dst, const void* src, size_t bytes, int lane) {
#ifdef MFX_NT_WB
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    u32x4_t* d = reinterpret_cast<u32x4_t*>(dst);
    const u32x4_t* q = reinterpret_cast<const u32x4_t*>(src);
    for (size_t i = lane; i < (bytes >> 4); i += 64) __builtin_nontemporal_store(q[i], d + i);
#else
    uint4* d = reinterpret_cast<uint4*>(dst);
    const uint4* q = reinterpret_cast<const uint4*>(src);
    for (size_t i = lane; i < (bytes >> 4); i += 64) d[i] = q[i];
#endif
}

// Generic install (maps / capacities beyond the prefetch budget): straight copies.
__device__ __forceinline__ void install_sync(const State& s, const PfTable& pt, int e, int G, const EnvView& v,
                                             EnvScalars& sc) {
    const EnvView gv = global_view(s, e, G);
    const int cap = s.cap;
    const uint16_t* walls = reinterpret_cast<const uint16_t*>(pt.walls);
    if ((s.cells_n & 7) == 0) {
        copy16(v.cells, walls, (size_t)s.cells_n * 2);
    } else {
        for (int i = TID; i < s.cells_n; i += blockDim.x) v.cells[i] = walls[i];
    }
    copy16(v.xy, gv.xy, (size_t)cap * 4);
    copy16(v.hp, gv.hp, (size_t)cap * 4);
    copy16(v.next_r, gv.next_r, (size_t)cap * 4);
    copy16(v.last_r, gv.last_r, (size_t)cap * 4);
    copy16(v.op_obj, gv.op_obj, (size_t)cap * 4);
    copy16(v.last_act, gv.last_act, (size_t)cap);
    copy16(v.meta, gv.meta, (size_t)cap);
    copy16(v.grp_ids, gv.grp_ids, (size_t)G * cap * 2);
    if (TID < kScalarWords)
        reinterpret_cast<uint32_t*>(&sc)[TID] = load_scalar_word(pt, e, TID);
}

// Work queue of k_rollout: envs heaviest first (an env's step time grows with its agent count), so
// a launch does not end on a tail of a few late episode starts.  Every workgroup files the envs it
// finishes under their new weight class in the next launch's class lists (buffered in LDS, one
// atomic per class per flush); the next launch walks the lists class by class.
constexpr int kOrderClasses = 8;

__device__ __forceinline__ int env_weight_class(int w) {
    return w >= 192 ? 0 : w >= 128 ? 1 : w >= 96 ? 2 : w >= 64 ? 3 : w >= 48 ? 4 : w >= 32 ? 5 : w >= 16 ? 6 : 7;
}



constexpr int kQueueBuf = 32;                      // envs buffered per workgroup before a flush

// Env at queue position i of this launch (qpre: prefix of the class counts, qpre[8] = E).
__device__ __forceinline__ int queue_env(const RolloutArgs& ra, const int* qpre, int i, int E, int qphase) {
    if (i >= E) return E;
    int c = 0;
    while (c < kOrderClasses - 1 && i >= qpre[c + 1]) ++c;
    return ra.cls_list[((size_t)(qphase & 1) * kOrderClasses + c) * ra.cls_stride + (i - qpre[c])];
}

// The envs a workgroup takes at the launch start (queue tiers): two -- its first env and the one it prefetches --
// workgroup b of G taking ranks b and 2G - 1 - b of the heaviest-first order, and the queue counter hands out ranks
// 2G, 2G + 1, ... after that, one claim per env, made at the start of an env's LAST step and resolved at its end (the
// env after the prefetched one).  So no workgroup starts with several of the heaviest envs (an episode start is 20
// steps of ~256 agents), a workgroup's ranks ascend (its envs past E come last), and at the end of the queue a
// workgroup holds one env beyond the one it runs, not three (round 3's three claims ahead: 0.442 against 0.536-0.544
// at 8192 envs, profiles/r04_queue_ab.txt).
__device__ __forceinline__ void queue_initial(int* r2) {
    const int G = (int)gridDim.x, b = (int)blockIdx.x;
    r2[0] = b; r2[1] = 2 * G - 1 - b;
}
__device__ __forceinline__ int queue_claim(const RolloutArgs& ra, int work_sel) {
    return atomicAdd(ra.work + work_sel, 1) + 2 * (int)gridDim.x;
}

// Thread 0: append the buffered envs to the next launch's class lists.
__device__ __forceinline__ void queue_flush(const RolloutArgs& ra, const int* wg_env, const uint8_t* wg_cls, int n,
                                            int qphase, int* tmp) {
    const int cn = (qphase + 1) % 3, ln = (qphase + 1) & 1;
    for (int c = 0; c < kOrderClasses; ++c) tmp[c] = 0;
    for (int k = 0; k < n; ++k) ++tmp[wg_cls[k]];
    for (int c = 0; c < kOrderClasses; ++c)
        tmp[c] = tmp[c] ? atomicAdd(ra.cls_cnt + cn * kOrderClasses + c, tmp[c]) : 0;
    for (int k = 0; k < n; ++k) {
        const int c = wg_cls[k];
        ra.cls_list[((size_t)ln * kOrderClasses + c) * ra.cls_stride + tmp[c]++] = wg_env[k];
    }
}

// Policy, mean action, set_action, step, get_reward and clear_dead of one env, run by a team (see
// psync): the whole workgroup, or wave 0 alone when the env has at most 64 agents.
#ifndef MFX_FUSED_BIG
#define MFX_FUSED_BIG 1            // k_rollout's workgroup teams use attack_big / move_jump
#endif
// kExt: the actions come from ra.actions (a learned policy's forward wrote them, mfx_qnet_act_rollout)
// instead of the on-device rush policy.
// mid (the few-env stepper): called by every lane right after the policy phase's first barrier, beside the policy
// loop (the stepper's last wave files the step's observation items there when it holds no agent).
struct NoMid { __device__ void operator()() const {} };
template <bool kB, bool kW, bool kExt = false, class Mid = NoMid>
__device__ __forceinline__ void agent_phase(const GameParams& gp, const State& s, const RolloutArgs& ra, EnvView& v,
                                            EnvScalars& sc, int* misc, StepSmem& sm, int32_t* act, int* ahist,
                                            uint32_t* atk, uint32_t* mov, uint32_t* sorted, float* red,
                                            const ParScratch ps, const BigScratch* bs, int e, uint32_t step_index,
                                            int stamp_row, uint32_t& rng, int& done, float& kills, int key_e = -1,
                                            const Mid& mid = Mid()) {
    (void)stamp_row;
    const int G = gp.n_groups, cap = s.cap, acap = s.acap;
#ifdef MFX_STAMPS
    if (TID == 0 && g_stamps) g_stamps[stamp_row * kStampW + 16] = (unsigned long long)(v.grp_n[0] + (G > 1 ? v.grp_n[1] : 0));
#endif
    // ---------------- policy + mean action (former_act_prob), all groups in one pass
    {
        int ntot = 0;
        for (int g = 0; g < G; ++g) ntot += v.grp_n[g];
#ifdef MFX_STAMPS
        if (kW && TID == 0 && g_stamps) g_stamps[stamp_row * kStampW + 11] = __builtin_amdgcn_s_memtime();
#endif
        for (int i = TID; i < G * 64; i += team_lanes<kW>()) ahist[i] = 0;
        psync<kW>();
        mid();
        if (kW) MFX_TSTAMP(kW, 23);          // (stamps build, wave teams: slots 23 / 28 split the policy phase)
        // key_e: the env's index in the whole batch where e is a sub-batch's (the few-env stepper)
        const uint32_t ekey = ra.policy_seed ^ mix32(step_index * 0x9E3779B9u + (uint32_t)(key_e < 0 ? e : key_e) * 0x632BE5ABu);
        for (int t = TID; t < ntot; t += team_lanes<kW>()) {
            int g = 0, i = t;
            while (i >= v.grp_n[g]) { i -= v.grp_n[g]; ++g; }
            int a;
            if (kExt) {
                a = ra.actions[((size_t)e * G + g) * ra.rowcap + i];
            } else {
                const int id = v.grp_ids[g * cap + i];
                const uint32_t key = ekey ^ mix32((uint32_t)id * 0x85EBCA77u + (uint32_t)g);
                a = rush_action(gp, sm.tt[g], v, g, id, key, ra.eps);
                if (i < ra.rowcap) ra.actions[((size_t)e * G + g) * ra.rowcap + i] = a;
            }
            act[g * cap + i] = a;
            if (!kExt || (unsigned)a < 64u) atomicAdd(&ahist[g * 64 + a], 1);   // (set_action rejects a bad id)
        }
        psync<kW>();
        if (kW) MFX_TSTAMP(kW, 28);
        for (int t = TID; t < G * 64; t += team_lanes<kW>()) {
            const int g = t >> 6, k = t & 63, na = sm.tt[g].n_action, n = v.grp_n[g];
            if (k < na)   // empty group: np.mean of nothing is NaN
                ra.mean_act[((size_t)e * G + g) * ra.mean_stride + k] = n ? (double)ahist[t] / (double)n : __longlong_as_double(0x7FF8000000000000ll);
        }
    }
    MFX_TSTAMP(kW, 4);
    // ---------------- set_action (group order) and step
    if (kW) set_action_wave(gp, s, v, sm.tt, act, atk, misc[0], mov, misc[1], acap);
    else if (blockDim.x <= 512) set_action_team(gp, s, v, sm.tt, act, atk, misc[0], mov, misc[1], sm.wave_tot, acap);
    else
        for (int g = 0; g < G; ++g) set_action_group<kW>(gp, s, v, g, act + g * cap, atk, misc[0], mov, misc[1], sm.wave_tot, acap);
    MFX_TSTAMP(kW, 5);
    step_env_core<kW>(gp, s, v, atk, misc[0], mov, misc[1], sorted, rng, sm, done, true, ps, sc.id_counter, nullptr,
                      0, MFX_FUSED_BIG ? bs : nullptr, stamp_row);
    MFX_TSTAMP(kW, 6);
    // ---------------- get_reward, episode return, kills
    for (int g = 0; g < G; ++g) {
        const int n = v.grp_n[g];
        float part = 0.0f;
        for (int i = TID; i < n; i += team_lanes<kW>()) {
            const float r = v.next_r[v.grp_ids[g * cap + i]] + v.grp_reward[g];
            if (i < ra.rowcap) ra.rewards[((size_t)e * G + g) * ra.rowcap + i] = r;
            if constexpr (kExt) {              // get_agent_id / get_alive before clear_dead (the replay collector)
                if (i < ra.rowcap) {
                    const int id = v.grp_ids[g * cap + i];
                    ra.ids[((size_t)e * G + g) * ra.rowcap + i] = ref_id(v, id);
                    ra.alive[((size_t)e * G + g) * ra.rowcap + i] = (uint8_t)!meta_dead(v.meta[id]);
                }
            }
            part += r;
        }
        const float tot = kW ? wave_sum(part) : block_sum_waves(part, red);
        if (TID == 0) { sc.ep_return[g] += tot; kills += (float)v.grp_dead[g]; }
    }
    MFX_TSTAMP(kW, 7);
    // ---------------- clear_dead
    clear_dead_env<kW>(gp, v, sm.wave_tot);
    MFX_TSTAMP(kW, 8);
}

// get_observation of every group of the env in LDS (after obs_prologue + obs_minimap): rows of
// env e in ra.view / ra.feat.
// records_ready: the agent records were written with the minimap (obs_minimap_add) and a barrier
// has passed since.
template <bool kB>
__device__ __forceinline__ void rollout_observe_groups(const GameParams& gp, const RolloutArgs& ra, const EnvView& v,
                                                       const ObsSmem& osm, int e, bool records_ready) {
    if (kB) {                                  // every group's records, one barrier, every group's stream
        if (!records_ready) {
            for (int g = 0; g < BattleShape::G; ++g) {
                ObsSmem og = osm;
                og.aq = osm.aq + g * ra.rowcap;
                obs_agent_records(gp, v, og, g, min(v.grp_n[g], ra.rowcap));
            }
            __syncthreads();
        }
#ifndef MFX_DIAG_NO_OBS                              // diagnostic builds only: everything but the stream
        for (int g = 0; g < BattleShape::G; ++g) {
            constexpr size_t VF = (size_t)BattleShape::VW * BattleShape::VH * BattleShape::NC;
            ObsSmem og = osm;
            og.aq = osm.aq + g * ra.rowcap;
            obs_stream_battle(gp, v, og, g, min(v.grp_n[g], ra.rowcap), ra.view[g] + (size_t)e * ra.rowcap * VF,
                              ra.feat[g] + (size_t)e * ra.rowcap * BattleShape::F, osm.stage);
        }
#endif
        __syncthreads();
        return;
    }
    for (int g = 0; g < gp.n_groups; ++g) {
        const TypeParams& T = gp.type[g];
        const size_t VF = (size_t)T.view_w * T.view_h * gp.n_ch;
        float* ov = ra.view[g] + (size_t)e * ra.rowcap * VF;
        float* of = ra.feat[g] + (size_t)e * ra.rowcap * gp.feat_size[g];
        const int n = min(v.grp_n[g], ra.rowcap);
        obs_prologue(gp, osm, g);
        __syncthreads();
        for (int a0 = 0; a0 < n; a0 += kObsK) obs_rows<kB>(gp, v, osm, g, a0, min(kObsK, n - a0), ov, of);
    }
}

// One launch = one training-loop step for every env.  Persistent workgroups: the grid is what
// fits on the chip at once, and each workgroup takes envs from a work queue, keeping env e in LDS
// while the next env's image is already in flight into registers.
// kSplit: the step half of the observation/step pipeline -- no observation, and env e is written
// back to ctx->w instead of ctx->s.
// kMode 0: the training-loop step with the on-device rush policy; 1: a learned policy's step -- act with the
// actions already in ra.actions (its forward on the observation the previous launch left), step, observe
// the new state; 2: observe only (the first observation of a learned-policy loop).  1 and 2: n_sub == 1.
template <bool kB, bool kPf, bool kSplit, int kMode = 0>
__global__ void __launch_bounds__(MFX_ROLLOUT_THREADS, MFX_ROLLOUT_OCC) k_rollout(const GameParams* __restrict__ gpp,
                                                                 const RolloutCtx* __restrict__ ctx,
                                                                 uint32_t step_index, int work_sel, int qphase,
                                                                 int n_sub) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ EnvScalars sc;
    __shared__ int misc[8];                  // 0 n_atk, 1 n_mov, 3 episode end, 4 done, 5-7 queue hand-off
    __shared__ int32_t n_before[kMaxGroups];
    __shared__ PfTable pt;
    __shared__ PfTable ptw;                  // kSplit: the write-back copy's addresses
    __shared__ int qpre[kOrderClasses + 1], qtmp[kOrderClasses];
    __shared__ int wg_env[kQueueBuf];
    __shared__ uint8_t wg_cls[kQueueBuf];
    __shared__ int wg_n;                     // envs buffered in wg_env / wg_cls
    // StepSmem (serial type table, scan / flag words) follows the env image and the scratch union
    StepSmem& sm = *reinterpret_cast<StepSmem*>(
        smem + rollout_main_bytes(kconst(gpp), kconst(ctx).s.cells_n, kconst(ctx).s.cap, kconst(ctx).s.acap,
                                  kconst(ctx).ra.rowcap, kB));
    // Work queue: position i of this launch is env queue_env(i) (class lists, heaviest first).
    // The hand-off is pipelined so that no queue access is waited on: while env e_k is processed,
    // e_{k+1} is being prefetched, thread 0 holds e_{k+2} (o) and the queue slot of e_{k+3} (g),
    // and both loads land before the next install's vmcnt(0).
    int e, en;
    int g = 0;
    EnvPrefetch pf;
#pragma unroll
    for (int j = 0; j < kPfSlots; ++j) pf.r[j] = make_uint4(0, 0, 0, 0);
    pf.w = 0;
    {
        const GameParams& gp = kconst(gpp);
        const State& s = kconst(ctx).s;
        const RolloutArgs& ra = kconst(ctx).ra;
        const int G = gp.n_groups, c4 = s.cap >> 2, sh = __ffs(c4) - 1;
        const int nc16 = s.cells_n >> 3, nrows = nc16 + image_small_rows(c4, G);
        if (TID == 0) {
            if (blockIdx.x == 0) {
                ra.work[work_sel ^ 1] = 0;
                for (int c = 0; c < kOrderClasses; ++c) ra.cls_cnt[((qphase + 2) % 3) * kOrderClasses + c] = 0;
            }
            int acc = 0;
            for (int c = 0; c < kOrderClasses; ++c) { qpre[c] = acc; acc += ra.cls_cnt[(qphase % 3) * kOrderClasses + c]; }
            qpre[kOrderClasses] = acc;
            int r3[2];
            queue_initial(r3);
            for (int k = 0; k < 2; ++k) misc[5 + k] = queue_env(ra, qpre, r3[k], s.E, qphase);
            wg_n = 0;
        }
        load_serial_types(gp, sm);
        pf_table_init(pt, s, ra, G);
        if (kSplit) pf_table_init(ptw, kconst(ctx).w, ra, G);
        __syncthreads();
        e = misc[5]; en = misc[6];
        if (kPf && e < s.E) pf_issue(pf, pt, s, e, nrows, nc16, sh, c4);
    }
    while (true) {
    // every iteration re-reads its parameters through scalar loads (see RolloutCtx)
    const GameParams& gp = kconst(gpp);
    const State& s = kconst(ctx).s;
    const RolloutArgs& ra = kconst(ctx).ra;
    if (e >= s.E) break;
    const int G = gp.n_groups, cap = s.cap, acap = s.acap;
    // ---------------- carve LDS
    EnvView v = carve_env(smem, s.cells_n, cap, G);
    v.grp_n = sc.grp_n; v.grp_dead = sc.grp_dead; v.grp_reward = sc.grp_reward;
    const size_t soff = env_image_bytes(s.cells_n, cap, G);
    char* uni = smem + soff;                 // scratch shared by the observation and the step phases
    size_t soff2 = soff;
    ObsSmem osm = carve_obs(smem, gp, 0, cap, ra.rowcap * (kB ? G : 1), obs_stage_floats(gp, 0, kB, blockDim.x), kB,
                            soff2);
    if (!kB) osm.info = nullptr;
    const RolloutUnion u = rollout_union(gp, cap, acap, blockDim.x);
    int32_t* act = reinterpret_cast<int32_t*>(uni + u.act);
    int* ahist = reinterpret_cast<int*>(uni + u.ahist);
    uint32_t* atk = reinterpret_cast<uint32_t*>(uni + u.atk);
    uint32_t* mov = reinterpret_cast<uint32_t*>(uni + u.mov);
    uint32_t* sorted = reinterpret_cast<uint32_t*>(uni + u.sorted);
    float* red = reinterpret_cast<float*>(uni + u.red);
    const size_t img_bytes = env_image_bytes(s.cells_n, cap, G);
    const int32_t* img_scal = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(ra.reset_image) + img_bytes);
    const int c4 = cap >> 2, sh = __ffs(c4) - 1;
    const int nc16 = s.cells_n >> 3, nrows = nc16 + image_small_rows(c4, G);
    {
        const int stamp_row = e;
        (void)stamp_row;
        MFX_STAMP(0);
        // ---------------- install env e
        if (kPf) pf_install(pf, smem, sc, nrows);
        else install_sync(s, pt, e, G, v, sc);
        // n_sub consecutive steps of env e while its image stays in LDS (one install and one write-back
        // for all of them); step sub is the launch's step step_index + sub for this env, exactly as if
        // it came from its own launch
        for (int sub = 0; sub < n_sub; ++sub) {
        if (TID == 0) {
            misc[0] = 0; misc[1] = 0;
        }
        constexpr bool kMmFused = kB && !kSplit && MFX_MM_IN_INSTALL;
        // the agents onto the walls-only cells: every listed agent is alive at an install (the lists
        // were compacted at the end of the env's previous step); for sub > 0 the cells are already
        // current and the pass only rebuilds the minimap histogram (rewriting the same ids)
        auto placement = [&]() {
            if (kMmFused) {                      // the minimap histogram rides on the placement pass
                obs_prologue(gp, osm, 0);
                for (int i = TID; i < G * BattleShape::VW * BattleShape::VH; i += blockDim.x) osm.hist[i] = 0;
            }
            __syncthreads();
            for (int q = 0; q < G; ++q) {
                const int nq = sc.grp_n[q];
                for (int i = TID; i < nq; i += blockDim.x) {
                    const int id = v.grp_ids[q * cap + i];
                    const uint32_t p = v.xy[id];
                    if (!meta_dead(v.meta[id])) v.cells[(p >> 16) * gp.W + (p & 0xFFFF)] = (uint16_t)id;
                    if (kMmFused) obs_minimap_add(gp, v, osm, q, id, p, i, ra.rowcap);
                }
            }
            __syncthreads();
        };
        // ---------------- get_observation for every group (k_rollout_obs in the pipeline)
        auto observe = [&]() {
            if (!kSplit) {
                if (kB && MFX_MM_IN_INSTALL) {
                    obs_minimap_finish<kB>(gp, v, osm);
                } else {
                    obs_prologue(gp, osm, 0);
                    obs_minimap<kB>(gp, v, osm, 0);      // one view size for every group (rollout_plan)
                }
                MFX_STAMP(2);
                rollout_observe_groups<kB>(gp, ra, v, osm, e, kB && MFX_MM_IN_INSTALL);
            }
            if (kSplit) __syncthreads();           // (rollout_observe_groups ends with one: the scratch changes hands)
        };
        // ---------------- policy, set_action, step, get_reward, clear_dead (agent_phase), episode end
        auto step_env = [&]() {
        uint32_t rng = sc.rng;
        int done = 0;
        float kills = 0.0f;
#ifdef MFX_ROLLOUT_PRIO
        __builtin_amdgcn_s_setprio(3);         // the latency-bound agent phases ahead of streaming waves
#endif
        {
            const ParScratch ps = carve_par(uni + u.par, acap, cap);
            BigScratch bs = carve_big(uni + u.par, acap, cap, false);
#ifdef MFX_STAMPS
            bs.srow = stamp_row; bs.sbase = 20;        // attack_big's stamps in slots 23-26
#endif
            int ntot = 0;
            for (int g = 0; g < G; ++g) ntot += v.grp_n[g];
#ifdef MFX_DIAG_OBS_ONLY                             // diagnostic builds only: the observation alone
            if (false) {
#else
            if (ntot <= 64) {
#endif
                if (TID < 64)                  // wave 0 (and its lane 0 below) alone; the others wait at
                    agent_phase<kB, true, kMode == 1>(gp, s, ra, v, sc, misc, sm, act, ahist, atk, mov, sorted, red,
                                                      ps, &bs, e, step_index + sub, stamp_row, rng, done, kills,
                                                      ra.env_base + e);
            } else {                               // (the episode-end barrier)
#ifndef MFX_DIAG_OBS_ONLY
                agent_phase<kB, false, kMode == 1>(gp, s, ra, v, sc, misc, sm, act, ahist, atk, mov, sorted, red, ps,
                                                   &bs, e, step_index + sub, stamp_row, rng, done, kills,
                                                   ra.env_base + e);
#endif
            }
        }
#ifdef MFX_ROLLOUT_PRIO
        __builtin_amdgcn_s_setprio(0);
#endif
        // ---------------- episode end -> reset + re-place the template (env.reset + add_agents)
        if (TID == 0) {
            sc.stats[3] += kills;
            int len = sc.ep_len + 1;
            misc[3] = 0;
            if (done || len >= ra.max_steps) {
                sc.stats[0] += 1.0;
                sc.stats[1] += sc.ep_return[0];
                sc.stats[2] += G > 1 ? sc.ep_return[1] : 0.0f;
                for (int g = 0; g < G; ++g) sc.ep_return[g] = 0.0f;
                len = 0;
                misc[3] = 1;
            }
            sc.ep_len = len;
            sc.rng = rng;
            misc[4] = done;
            unsigned long long tot = 0;
            for (int g = 0; g < G; ++g) tot += (unsigned)n_before[g];
            sc.agent_steps += tot;
        }
        __syncthreads();
        if (kMode == 1 && misc[3]) {           // the next episode's first former_act_prob is zeros (senario_battle.py:89)
            for (int t = TID; t < G * ra.mean_stride; t += blockDim.x) ra.mean_act[(size_t)e * G * ra.mean_stride + t] = 0.0;
        }
        if (misc[3]) {
            copy16(v.cells, ra.reset_image, img_bytes);
            if (TID < G) {
                sc.grp_n[TID] = img_scal[TID];
                sc.grp_dead[TID] = 0;
                sc.grp_reward[TID] = 0.0f;
            }
            if (TID == 0) sc.id_counter = img_scal[4];
            __syncthreads();
        }
        };
        placement();
        MFX_STAMP(13);
        if (TID < G) n_before[TID] = sc.grp_n[TID];
        if (sub == 0) {
#ifdef MFX_STAMPS
            if (TID == 0 && g_stamps) g_stamps[stamp_row * kStampW + 29] = (unsigned long long)(sc.grp_n[0] + (G > 1 ? sc.grp_n[1] : 0));
#endif
            if (kPf && en < s.E) pf_issue(pf, pt, s, en, nrows, nc16, sh, c4);
        }
        // the env after the prefetched one is claimed at the start of this env's last step (its atomic lands under
        // the step) and resolved at the end of the env
        if (TID == 0 && sub == n_sub - 1) g = queue_claim(ra, work_sel);
        MFX_STAMP(1);
        if (kMode == 0) {                      // the training-loop step: observe, then act and step
            observe();
            MFX_STAMP(3);
            step_env();
        } else if (kMode == 1) {               // act on the observation the last launch left, then observe
            step_env();
            placement();                       // (the minimap histogram of the stepped state)
            observe();
        } else {                               // observe only (the first observation of a learned-policy loop)
            observe();
        }
        }                                        // n_sub steps of env e
        MFX_STAMP(9);
        if (TID == 0) {                        // file the env for the next launch's queue
            int w = 0, w0 = 0;
            for (int q = 0; q < G; ++q) { w += sc.grp_n[q]; w0 += img_scal[q]; }
            // with few envs per workgroup (< 16): its weight over the next launch's n_sub steps (assumed this
            // launch's) -- an env that reaches the episode cap inside them restarts with the template's w0 agents
            // for the rest; filed by its current (late-game, light) size it would be taken last and end the launch
            // on a heavy tail.  With many envs per workgroup the tail is short anyway and the current size wins
            // (heavy and light units mixed through the launch: 0.859 against 0.834, profiles/r04_queue_ab.txt)
            const int left = ra.max_steps - sc.ep_len;
            if (s.E < 16 * (int)gridDim.x && left < n_sub)
                w = (w * max(left, 0) + w0 * (n_sub - max(left, 0))) / n_sub;
            wg_env[wg_n] = e;
            wg_cls[wg_n] = (uint8_t)env_weight_class(w);
            misc[5] = queue_env(ra, qpre, g, s.E, qphase);                         // next iteration's prefetch
            if (++wg_n == kQueueBuf) { queue_flush(ra, wg_env, wg_cls, wg_n, qphase, qtmp); wg_n = 0; }
        }
        // ---------------- write the env back (wave kWbWave only, see EnvPrefetch)
        if ((TID >> 6) == kWbWave) {
            const int lane = TID & 63;
            const EnvView gv = global_view(kSplit ? kconst(ctx).w : s, e, G);   // cells: rebuilt at the next install
            const int idc = sc.id_counter;
            const size_t n4 = ((size_t)idc + 3) & ~(size_t)3, n16 = ((size_t)idc + 15) & ~(size_t)15;
            wcopy16(gv.xy, v.xy, n4 * 4, lane);
            wcopy16(gv.hp, v.hp, n4 * 4, lane);
            wcopy16(gv.next_r, v.next_r, n4 * 4, lane);
            wcopy16(gv.last_r, v.last_r, n4 * 4, lane);
            wcopy16(gv.op_obj, v.op_obj, n4 * 4, lane);
            wcopy16(gv.last_act, v.last_act, n16, lane);
            wcopy16(gv.meta, v.meta, n16, lane);
            for (int g = 0; g < G; ++g)
                wcopy16(gv.grp_ids + g * cap, v.grp_ids + g * cap, (((size_t)v.grp_n[g] + 7) & ~(size_t)7) * 2, lane);
            if (lane < kScalarWords) {
                g_u32* p = scalar_addr(kSplit ? ptw : pt, e, lane);
                if (p) *p = reinterpret_cast<const uint32_t*>(&sc)[lane];
            }
            if (lane == 0) { s.n_atk[e] = 0; s.n_mov[e] = 0; s.done[e] = misc[4]; }
        }
        MFX_STAMP(10);
        __syncthreads();                       // LDS reads of the write-back are done; hand-off visible
        e = en;
        en = misc[5];
    }
    }
    if (TID == 0 && wg_n) queue_flush(kconst(ctx).ra, wg_env, wg_cls, wg_n, qphase, qtmp);
}

#ifndef MFX_OBS_OCC
#define MFX_OBS_OCC 8              // k_rollout_obs: <= 64 VGPRs, so it fits beside k_rollout's waves
#endif
// The observation half of the pipeline: get_observation of every env of the launch from the
// state before the step (ctx->s), beside k_rollout<.., kSplit> which steps the same envs from the
// same copy and writes the other.  Persistent workgroups on their own counter (RolloutArgs::work
// [2 + sel]) over the same heaviest-first queue; env e+1's image is in flight into registers
// while env e is observed.  LDS: the env image, then the observation scratch.
template <bool kB, bool kPf>
__global__ void __launch_bounds__(MFX_ROLLOUT_THREADS, MFX_OBS_OCC) k_rollout_obs(const GameParams* __restrict__ gpp,
                                                                                 const RolloutCtx* __restrict__ ctx,
                                                                                 int work_sel, int qphase) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ EnvScalars sc;
    __shared__ int misc[4];                  // 0-1 queue hand-off
    __shared__ PfTable pt;
    __shared__ int qpre[kOrderClasses + 1];
    int e, en;
    EnvPrefetch pf;
#pragma unroll
    for (int j = 0; j < kPfSlots; ++j) pf.r[j] = make_uint4(0, 0, 0, 0);
    pf.w = 0;
    {
        const GameParams& gp = kconst(gpp);
        const State& s = kconst(ctx).s;
        const RolloutArgs& ra = kconst(ctx).ra;
        const int G = gp.n_groups, c4 = s.cap >> 2, sh = __ffs(c4) - 1;
        const int nc16 = s.cells_n >> 3, nrows = nc16 + image_small_rows(c4, G);
        if (TID == 0) {
            if (blockIdx.x == 0) ra.work[2 + (work_sel ^ 1)] = 0;
            int acc = 0;
            for (int c = 0; c < kOrderClasses; ++c) { qpre[c] = acc; acc += ra.cls_cnt[(qphase % 3) * kOrderClasses + c]; }
            qpre[kOrderClasses] = acc;
            for (int k = 0; k < 2; ++k) misc[k] = queue_env(ra, qpre, atomicAdd(ra.work + 2 + work_sel, 1), s.E, qphase);
        }
        pf_table_init(pt, s, ra, G);
        __syncthreads();
        e = misc[0]; en = misc[1];
        if (kPf && e < s.E) pf_issue(pf, pt, s, e, nrows, nc16, sh, c4);
    }
    while (true) {
        const GameParams& gp = kconst(gpp);
        const State& s = kconst(ctx).s;
        const RolloutArgs& ra = kconst(ctx).ra;
        if (e >= s.E) break;
        const int G = gp.n_groups, cap = s.cap;
        EnvView v = carve_env(smem, s.cells_n, cap, G);
        v.grp_n = sc.grp_n; v.grp_dead = sc.grp_dead; v.grp_reward = sc.grp_reward;
        size_t soff = env_image_bytes(s.cells_n, cap, G);
        ObsSmem osm = carve_obs(smem, gp, 0, cap, ra.rowcap * (kB ? G : 1), obs_stage_floats(gp, 0, kB, blockDim.x),
                                kB, soff);
        if (!kB) osm.info = nullptr;
        const int c4 = cap >> 2, sh = __ffs(c4) - 1;
        const int nc16 = s.cells_n >> 3, nrows = nc16 + image_small_rows(c4, G);
        if (kPf) pf_install(pf, smem, sc, nrows);
        else install_sync(s, pt, e, G, v, sc);
        __syncthreads();
        for (int q = 0; q < G; ++q) {           // the listed agents onto the walls-only cells
            const int nq = sc.grp_n[q];
            for (int i = TID; i < nq; i += blockDim.x) {
                const int id = v.grp_ids[q * cap + i];
                const uint32_t p = v.xy[id];
                if (!meta_dead(v.meta[id])) v.cells[(p >> 16) * gp.W + (p & 0xFFFF)] = (uint16_t)id;
            }
        }
        if (TID == 0) misc[0] = queue_env(ra, qpre, atomicAdd(ra.work + 2 + work_sel, 1), s.E, qphase);
        __syncthreads();
        if (kPf && en < s.E) pf_issue(pf, pt, s, en, nrows, nc16, sh, c4);
        obs_prologue(gp, osm, 0);
        obs_minimap<kB>(gp, v, osm, 0);
        rollout_observe_groups<kB>(gp, ra, v, osm, e, false);
        __syncthreads();                        // the image and the hand-off change hands
        e = en;
        en = misc[0];
    }
}

