// battle_engine.cpp -- host runtime of the Battle engine: configuration, the reward DSL compiler, device state and
// the per-call device API.  (The fused rollout, the drop-in path, render and the C ABI: battle_engine.h.)
//
// The C ABI is the reference's own (runtime_api.h:118-181: env_* / gridworld_*), so the
// reference python wrapper (gridworld.py, via ctypes) and this repository's drop-in
// `magent` package both bind it unchanged.  Those calls work on env 0 and move data
// through host buffers.  The batched device API (mfx_battle_*) drives all E envs of an
// engine with device pointers and never leaves HBM.  See include/magent_amd.h.
#include "battle_engine.h"

namespace mfx {

// ------------------------------------------------------------------ host-side ranges
static HostRange circle_range(float radius, float inner, int parity) {   // Range.h:171-215
    const double eps = 1e-8;
    HostRange r;
    int width = 2 * (int)(radius + eps) + parity;
    const int center = (int)radius;
    if (width % 2 != parity) width++;
    r.w = r.h = width;
    r.in.assign((size_t)width * width, 0);
    const double delta = parity == 0 ? 0.5 : 0;
    for (int i = 0; i < width; i++)
        for (int j = 0; j < width; j++) {
            const double ddx = std::fabs(j - center + delta), ddy = std::fabs(i - center + delta);
            const double dis = std::sqrt(ddx * ddx + ddy * ddy);
            if (dis < radius + eps && dis > inner - eps) {
                r.in[(size_t)i * width + j] = 1;
                r.dx.push_back(j - center);
                r.dy.push_back(i - center);
            }
        }
    r.count = (int)r.dx.size();
    r.x1 = r.y1 = -center;
    r.x2 = r.y2 = width - center - 1;
    return r;
}

static HostRange sector_range(float angle, float radius, int parity) {   // Range.h:121-166
    const double PI = 3.1415926536, eps = 0.00001;
    HostRange r;
    const int height = (int)(radius + 0.5);
    int width = (int)(2 * radius * std::sin(angle / 2 * (PI / 180)) + 0.5);
    if (width % 2 != parity) width--;
    r.w = width; r.h = height;
    r.in.assign((size_t)std::max(0, width * height), 0);
    for (int i = 0; i < height; i++)
        for (int j = 0; j < width; j++) {
            const double ddx = std::fabs(j - (width - 1) / 2.0), ddy = std::fabs((double)(height - i));
            const double dis = std::sqrt(ddx * ddx + ddy * ddy);
            if (dis < radius + 0.2 + eps && ddx / ddy < std::tan(angle / 2 * PI / 180) + eps) {
                r.in[(size_t)i * width + j] = 1;
                r.dx.push_back(j - width / 2);
                r.dy.push_back(i - height);
            }
        }
    r.count = (int)r.dx.size();
    r.x1 = -width / 2; r.y1 = -height; r.x2 = (width - 1) / 2; r.y2 = -1;
    return r;
}

// ------------------------------------------------------------------ the engine
BattleEngine::~BattleEngine() {
    (void)quiesce();
    for (void* p : retired) (void)hipHostFree(p);
#ifdef MFX_STAMPS
    if (hst_n)
        fprintf(stderr, "[magent_amd stamps] fast_step host us: enter->posted %.2f posted->record %.2f record->return %.2f (%ld steps)\n",
                hst[0] / hst_n, hst[1] / hst_n, hst[2] / hst_n, hst_n);
#endif
    for (auto& x : act_ev) if (x) (void)hipEventDestroy(x);
    release();
    for (auto& x : ro_str) if (x) (void)hipStreamDestroy(x);
    for (auto& x : ro_ev) if (x) (void)hipEventDestroy(x);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
}

void BattleEngine::release() {
    for (void* p : {(void*)s.cells, (void*)s.xy, (void*)s.hp, (void*)s.next_r, (void*)s.last_r,
                    (void*)s.last_act, (void*)s.op_obj, (void*)s.meta, (void*)s.grp_ids, (void*)s.grp_n,
                    (void*)s.grp_dead, (void*)s.grp_reward, (void*)s.id_counter, (void*)s.rng, (void*)s.atk,
                    (void*)s.n_atk, (void*)s.mov, (void*)s.n_mov, (void*)s.done, (void*)s.idx_mark, (void*)s.food,
                    (void*)s.rid, (void*)s.rid_off, (void*)d_sort, (void*)d_gp,
                    (void*)d_err})
        if (p) (void)hipFree(p);
    s = State{}; d_sort = nullptr; d_gp = nullptr; d_err = nullptr; allocated = false;
    free_twin();
}

// ------------------------------------------------------------------ config
int BattleEngine::set_config(const char* key, void* p) {
    MFX_CHECK(quiesce());
    touch();
    if (!strcmp(key, "map_width")) W = *(int*)p;
    else if (!strcmp(key, "map_height")) H = *(int*)p;
    else if (!strcmp(key, "food_mode")) food = *(bool*)p;
    else if (!strcmp(key, "turn_mode")) turn = *(bool*)p;
    else if (!strcmp(key, "minimap_mode")) minimap = *(bool*)p;
    else if (!strcmp(key, "goal_mode")) goal = *(bool*)p;
    else if (!strcmp(key, "embedding_size")) emb = *(int*)p;
    else if (!strcmp(key, "render_dir")) render_dir = (const char*)p;
    else if (!strcmp(key, "seed")) {
        const unsigned long sv = (unsigned long)(long)*(int*)p;
        const uint64_t x = sv % 2147483647UL;
        rng_init = x ? (uint32_t)x : 1u;
        if (allocated) {
            std::vector<uint32_t> h((size_t)E, rng_init);
            MFX_HIP(hipMemcpyAsync(s.rng, h.data(), sizeof(uint32_t) * E, hipMemcpyHostToDevice, stream));
            MFX_HIP(hipStreamSynchronize(stream));
        }
    } else return fail("invalid argument in set_config: %s", key);
    return 0;
}

int BattleEngine::register_type(const char* name, int n, const char** keys, const float* values) {
    MFX_CHECK(quiesce());
    touch();
    if (types.count(name)) return fail("duplicated name of agent type: %s", name);
    AgentTypeSpec t;
    t.name = name;
    for (int i = 0; i < n; i++) {
        const char* k = keys[i];
        const float v = values[i];
#define MFX_I(f) if (!strcmp(k, #f)) { t.f = (int)(v + 0.5); continue; }
#define MFX_F(f) if (!strcmp(k, #f)) { t.f = v; continue; }
#define MFX_B(f) if (!strcmp(k, #f)) { t.f = (bool)(int)(v + 0.5); continue; }
        MFX_I(width) MFX_I(length) MFX_F(speed) MFX_F(hp) MFX_F(view_radius) MFX_F(view_angle)
        MFX_F(attack_radius) MFX_F(attack_angle) MFX_F(hear_radius) MFX_F(speak_radius)
        MFX_I(speak_ability) MFX_F(damage) MFX_F(trace) MFX_F(eat_ability) MFX_F(step_recover)
        MFX_F(kill_supply) MFX_F(food_supply) MFX_B(attack_in_group) MFX_B(can_absorb)
        MFX_F(step_reward) MFX_F(kill_reward) MFX_F(dead_penalty) MFX_F(attack_penalty)
#undef MFX_I
#undef MFX_F
#undef MFX_B
        // accepted and then recomputed from the body size (AgentType.cc:117-120)
        if (!strcmp(k, "view_x_offset") || !strcmp(k, "view_y_offset") || !strcmp(k, "att_x_offset") ||
            !strcmp(k, "att_y_offset") || !strcmp(k, "turn_x_offset") || !strcmp(k, "turn_y_offset"))
            continue;
        return fail("invalid agent config in register_agent_type: %s", k);
    }
    if (t.width < 1 || t.length < 1 || t.width > 8 || t.length > 8)
        return fail("agent bodies must be 1..8 cells wide and long");
    const int parity = t.width % 2;
    if (t.view_angle >= 180) {
        if (std::fabs(t.view_angle - 360) > 1e-5) return fail("only angle = 360 when angle > 180");
        t.view = circle_range(t.view_radius, 0, parity);
    } else t.view = sector_range(t.view_angle, t.view_radius, parity);
    if (t.attack_angle >= 180) {
        if (std::fabs(t.attack_angle - 360) > 1e-5) return fail("only angle = 360 when angle > 180");
        t.attack = circle_range(t.attack_radius, t.width / 2.0f, parity);
    } else t.attack = sector_range(t.attack_angle, t.attack_radius, parity);
    t.move = circle_range(t.speed, 0, 1);
    t.turn_base = t.move.count;
    t.attack_base = turn ? t.turn_base + 2 : t.turn_base;      // AgentType.cc:118-122 (turn at register)
    t.n_action = t.attack_base + t.attack.count;
    if (t.view.w * t.view.h > kMaxViewCells || t.view.w <= 0 || t.view.h <= 0)
        return fail("view range too large (max %d cells)", kMaxViewCells);
    if (t.move.count > kMaxRangeCount || t.attack.count > kMaxRangeCount)
        return fail("move/attack range too large (max %d cells)", kMaxRangeCount);
    types.emplace(t.name, std::move(t));
    return 0;
}

int BattleEngine::new_group(const char* type_name, int* group) {
    MFX_CHECK(quiesce());
    touch();
    if (!types.count(type_name)) return fail("invalid name of agent type in new_group: %s", type_name);
    if (n_groups() >= kMaxGroups) return fail("at most %d groups", kMaxGroups);
    if (allocated) return fail("new_group after the first reset is not supported");
    *group = n_groups();
    group_types.push_back(type_name);
    return 0;
}

// ------------------------------------------------------------------ reward DSL
// The common rule form handled by RuleParams (k_step / k_rollout without the interpreter).
bool BattleEngine::simple_rule(const Rule& R) const {
    if (R.on < 0 || R.on >= (int)nodes.size()) return false;
    const Node& N = nodes[R.on];
    if (N.op != kEvAttack && N.op != kEvKill && N.op != kEvCollide) return false;
    if (N.raw.size() < 2) return false;
    const int sa = N.raw[0], sb = N.raw[1];
    if (sa < 0 || sb < 0 || sa >= (int)syms.size() || sb >= (int)syms.size()) return false;
    if (syms[sa].index != -1 || syms[sb].index != -1 || syms[sa].group == syms[sb].group) return false;
    if ((int)R.recv.size() > kMaxRecv) return false;
    for (int x : R.recv)
        if (x != sa && x != sb) return false;
    return true;
}

// related_symbols / infer_map of a node (GridWorld::collect_related_symbol, RewardEngine.cc:68-101):
// std::set / std::map keyed by AgentSymbol*, i.e. ordered by symbol number; map insertion keeps
// the first entry for a key.
int BattleEngine::node_symbols(int ni, std::set<int>& rel, std::map<int, int>& infer, int depth) const {
    if (ni < 0 || ni >= (int)nodes.size() || depth > kMaxNodes)
        return fail("reward DSL: bad event node %d", ni);
    const Node& N = nodes[ni];
    const auto need = [&](size_t k) { return N.raw.size() >= k; };
    switch (N.op) {
        case kEvAnd: case kEvOr: {
            if (!need(2)) return fail("reward DSL: malformed node %d", ni);
            std::set<int> r0, r1; std::map<int, int> m0, m1;
            MFX_CHECK(node_symbols(N.raw[0], r0, m0, depth + 1));
            MFX_CHECK(node_symbols(N.raw[1], r1, m1, depth + 1));
            rel.insert(r0.begin(), r0.end()); rel.insert(r1.begin(), r1.end());
            infer.insert(m0.begin(), m0.end()); infer.insert(m1.begin(), m1.end());
            return 0;
        }
        case kEvNot: {
            if (!need(1)) return fail("reward DSL: malformed node %d", ni);
            std::set<int> r0; std::map<int, int> m0;
            MFX_CHECK(node_symbols(N.raw[0], r0, m0, depth + 1));
            rel.insert(r0.begin(), r0.end()); infer.insert(m0.begin(), m0.end());
            return 0;
        }
        case kEvKill: case kEvCollide: case kEvAttack:
            if (!need(2)) return fail("reward DSL: malformed node %d", ni);
            rel.insert(N.raw[0]); rel.insert(N.raw[1]);
            infer.insert(std::make_pair(N.raw[0], N.raw[1]));
            return 0;
        case kEvAt: case kEvIn: case kEvDie: case kEvInALine:
            if (!need(N.op == kEvAt ? 3 : N.op == kEvIn ? 5 : 1)) return fail("reward DSL: malformed node %d", ni);
            rel.insert(N.raw[0]);
            return 0;
        case kEvAlign:
            // reads counter_x / counter_y, which the reference allocates and never fills
            // (GridWorld.cc:99-100, :1039-1050 commented out): no defined result to reproduce
            return fail("reward DSL: 'align' reads uninitialised engine memory in the reference; not supported");
        default:
            return fail("reward DSL: invalid event op %d", N.op);
    }
}

int BattleEngine::post_order(int ni, std::vector<int>& out, int depth) const {
    if (depth > kMaxNodes) return fail("reward DSL: event graph too deep");
    if (std::find(out.begin(), out.end(), ni) != out.end()) return 0;
    const Node& N = nodes[ni];
    if (N.op == kEvAnd || N.op == kEvOr) {
        MFX_CHECK(post_order(N.raw[0], out, depth + 1));
        MFX_CHECK(post_order(N.raw[1], out, depth + 1));
    } else if (N.op == kEvNot) {
        MFX_CHECK(post_order(N.raw[0], out, depth + 1));
    }
    out.push_back(ni);
    return 0;
}

// GridWorld::init_reward_description (RewardEngine.cc:105-208) into a DslProgram.
int BattleEngine::compile_dsl(DslProgram& P) const {
    P = DslProgram{};
    if ((int)syms.size() > kMaxSyms) return fail("reward DSL: at most %d agent symbols", kMaxSyms);
    if ((int)nodes.size() > kMaxNodes) return fail("reward DSL: at most %d event nodes", kMaxNodes);
    const int G = n_groups();
    for (size_t i = 0; i < syms.size(); i++) {
        if (syms[i].group < 0 || syms[i].group >= G) return fail("reward DSL: symbol %zu has no valid group", i);
        if (syms[i].index < -2) return fail("reward DSL: symbol %zu has a bad index", i);
        P.sym[i] = DslSym{syms[i].group, syms[i].index};
    }
    auto sym_ok = [&](int x) { return x >= 0 && x < (int)syms.size(); };
    for (size_t i = 0; i < nodes.size(); i++) {
        const Node& N = nodes[i];
        DslNode& D = P.node[i];
        D = DslNode{N.op, -1, -1, 0, 0, 0, 0};
        const auto raw = [&](size_t k) { return k < N.raw.size() ? N.raw[k] : -1; };
        D.a = raw(0); D.b = raw(1);
        switch (N.op) {
            case kEvAnd: case kEvOr: case kEvNot:
                if (D.a < 0 || D.a >= (int)nodes.size() || (N.op != kEvNot && (D.b < 0 || D.b >= (int)nodes.size())))
                    return fail("reward DSL: node %zu has a bad input", i);
                break;
            case kEvKill: case kEvCollide: case kEvAttack:
                if (!sym_ok(D.a) || !sym_ok(D.b)) return fail("reward DSL: node %zu has a bad symbol", i);
                if (syms[D.b].index == -2)       // assert(!symbol_input[1]->is_all()) (RewardEngine.cc:221)
                    return fail("reward DSL: the object of attack/kill/collide cannot be a whole group");
                break;
            case kEvAt:
                if (!sym_ok(D.a)) return fail("reward DSL: node %zu has a bad symbol", i);
                D.i0 = raw(1); D.i1 = raw(2);
                break;
            case kEvIn:
                if (!sym_ok(D.a)) return fail("reward DSL: node %zu has a bad symbol", i);
                D.i0 = raw(1); D.i1 = raw(2); D.i2 = raw(3); D.i3 = raw(4);
                break;
            case kEvDie:
                if (!sym_ok(D.a)) return fail("reward DSL: node %zu has a bad symbol", i);
                break;
            case kEvInALine:
                if (!sym_ok(D.a) || syms[D.a].index != -2)      // assert(is_all()) (RewardEngine.cc:260)
                    return fail("reward DSL: in_a_line needs a whole-group symbol");
                break;
            default:
                break;                     // reported by node_symbols when a rule uses it
        }
    }
    P.n_rules = (int)rules.size();
    for (size_t r = 0; r < rules.size(); r++) {
        const Rule& R = rules[r];
        DslRule& D = P.rule[r];
        std::set<int> rel;
        std::map<int, int> infer;
        MFX_CHECK(node_symbols(R.on, rel, infer, 0));
        // input symbols: first the inferable subjects with their objects, then the rest
        std::vector<int> in, inf;
        std::set<int> added;
        for (int x : rel) {
            if (added.count(x)) continue;
            auto it = infer.find(x);
            if (it != infer.end()) {
                in.push_back(x); inf.push_back(it->second);
                added.insert(x); added.insert(it->second);
            }
        }
        for (int x : rel)
            if (!added.count(x)) { in.push_back(x); inf.push_back(-1); }
        if ((int)in.size() > kMaxSyms) return fail("reward rule %zu: too many symbols", r);
        D.n_in = (int)in.size();
        for (size_t k = 0; k < in.size(); k++) { D.in_sym[k] = (int8_t)in[k]; D.infer[k] = (int8_t)inf[k]; }
        std::vector<int> post;
        MFX_CHECK(post_order(R.on, post, 0));
        D.n_post = (int)post.size();
        for (size_t k = 0; k < post.size(); k++) D.post[k] = (int8_t)post[k];
        if ((int)R.recv.size() > kMaxRecv) return fail("reward rule %zu: too many receivers", r);
        D.n_recv = (int)R.recv.size();
        D.terminal = R.terminal;
        for (size_t k = 0; k < R.recv.size(); k++) {
            const int x = R.recv[k];
            if (!sym_ok(x)) return fail("reward rule %zu: bad receiver", r);
            // a receiver is bound only if the event involves it (RewardEngine.cc:191-193)
            if (syms[x].index != -2 && !rel.count(x))
                return fail("reward rule %zu: receiver %d is not involved in the triggering event", r, x);
            D.recv[k] = (int8_t)x;
            D.val[k] = R.val[k];
        }
    }
    return 0;
}

// ------------------------------------------------------------------ compile
int BattleEngine::build_params() {
    const int G = n_groups();
    if (W <= 0 || H <= 0) return fail("map_width/map_height not set");
    if (W > 0xFFFF || H > 0xFFFF) return fail("map too large");
    if (G == 0) return fail("no groups");
    GameParams p{};
    p.W = W; p.H = H; p.n_groups = G; p.minimap = minimap; p.emb = emb;
    p.turn_mode = turn; p.food_mode = food;
    p.n_ch = group2channel(G);
    if ((long)W * H > 99 * 99) { large_map = true; n_sep = (long)W * H > 1000 * 1000 ? 16 : 8; }  // sticky
    p.large_map = large_map; p.n_sep = n_sep; p.band_w = (W + n_sep - 1) / n_sep;
    for (int g = 0; g < G; g++) {
        AgentTypeSpec& t = gtype(g);
        TypeParams& T = p.type[g];
        T.hp = t.hp; T.damage = t.damage; T.step_recover = t.step_recover; T.kill_supply = t.kill_supply;
        T.step_reward = t.step_reward; T.kill_reward = t.kill_reward; T.dead_penalty = t.dead_penalty;
        T.attack_penalty = t.attack_penalty; T.attack_in_group = t.attack_in_group;
        T.can_absorb = t.can_absorb;
        T.n_action = t.n_action; T.turn_base = t.turn_base; T.attack_base = t.attack_base;
        T.n_move = t.move.count; T.n_attack = t.attack.count;
        T.view_w = t.view.w; T.view_h = t.view.h;
        T.view_x1 = t.width / 2 + t.view.x1;     // eye = pos + view offset (Map.cc:146-149)
        T.view_y1 = t.length / 2 + t.view.y1;
        T.att_x_off = t.width / 2; T.att_y_off = t.length / 2;
        T.body_w = t.width; T.body_h = t.length;
        T.view_off_x = t.width / 2; T.view_off_y = t.length / 2;
        T.view_lt_x = t.view.x1; T.view_lt_y = t.view.y1;
        T.eat_ability = t.eat_ability; T.food_supply = t.food_supply;
        for (int i = 0; i < t.move.count; i++) { T.move_dx[i] = (int8_t)t.move.dx[i]; T.move_dy[i] = (int8_t)t.move.dy[i]; }
        for (int i = 0; i < t.attack.count; i++) { T.att_dx[i] = (int8_t)t.attack.dx[i]; T.att_dy[i] = (int8_t)t.attack.dy[i]; }
        for (int i = 0; i < t.view.w * t.view.h; i++) {
            T.view_mask[i] = t.view.in[i];
            if (t.view.in[i]) T.view_bits[i >> 5] |= 1u << (i & 31);
        }
        p.feat_size[g] = feature_size(g);
    }
    // reward rules: the common form (one attack/kill/collide event between 'any' agents of two
    // groups, receivers among its subject/object) runs data-parallel (RuleParams); anything else
    // goes through the DSL interpreter (DslProgram), rule order preserved either way.
    if ((int)rules.size() > kMaxRules) return fail("at most %d reward rules", kMaxRules);
    bool simple = true;
    for (size_t r = 0; r < rules.size() && simple; r++) simple = simple_rule(rules[r]);
    p.n_rules = 0;
    p.dsl = 0;
    if (simple) {
        p.n_rules = (int)rules.size();
        for (size_t r = 0; r < rules.size(); r++) {
            const Rule& R = rules[r];
            const Node& N = nodes[R.on];
            const int sa = N.raw[0], sb = N.raw[1];
            RuleParams& RP = p.rules[r];
            RP.op = N.op == kEvAttack ? kOpAttack : (N.op == kEvKill ? kOpKill : kOpCollide);
            RP.subj_group = syms[sa].group; RP.obj_group = syms[sb].group;
            RP.n_recv = (int)R.recv.size(); RP.terminal = R.terminal;
            for (size_t k = 0; k < R.recv.size(); k++) {
                RP.recv_is_obj[k] = R.recv[k] == sb;
                RP.val[k] = R.val[k];
            }
        }
    } else {
        MFX_CHECK(compile_dsl(p.prog));
        p.dsl = 1;
    }
    p.record_events = first_render ? 0 : 1;
    p.par_step = 1;
    // kill_supply != 0 keeps the parallel forms: the per-call step's wave attack models it (<= 64 attackers),
    // every other attack falls back to the serial walk inside the step (step_env_core)
    // (round 5 stepped them serially throughout: forest 74 -> 30 us per step, r06_generic_step_times.jsonl).
    // Bodies larger than 1x1 keep them too (the per-call step's move_wave_body / attack_wave<.., true>) unless an
    // attack cell can fall on the attacker's own body: a self-hit would have to kill its attacker at its own turn,
    // which the fixed point's "alive at its turn" test does not model (circle ranges exclude the body).
    for (int g = 0; g < p.n_groups; g++) {
        const TypeParams& T = p.type[g];
        bool self_hit = false;
        for (int k = 0; k < T.n_attack; k++) {
            const int cx = T.att_x_off + T.att_dx[k], cy = T.att_y_off + T.att_dy[k];
            self_hit = self_hit || (cx >= 0 && cx < T.body_w && cy >= 0 && cy < T.body_h);
        }
        p.par_step &= !self_hit && !T.can_absorb;     // absorption: the serial move (do_move_one)
    }
    // turn and food mode run on k_step<.., kBody>'s wave forms (the other kernels walk them serially)
    gp = p;
    return 0;
}

void BattleEngine::ensure_capacity(int need_ids, int need_actions) {
    if ((need_ids > s.cap || need_actions > s.acap) && quiesce() != 0) throw HipFailure("resident server: stop failed");
    const int G = n_groups();
    if (need_ids > s.cap) {
        int nc = std::max(64, s.cap);
        while (nc < need_ids) nc *= 2;
        if (nc > kCellFood) nc = kCellFood;        // ids stay below the cell codes
        const int oc = s.cap;
        grow(s.xy, E, oc, nc); grow(s.hp, E, oc, nc); grow(s.next_r, E, oc, nc); grow(s.last_r, E, oc, nc);
        grow(s.last_act, E, oc, nc); grow(s.op_obj, E, oc, nc); grow(s.meta, E, oc, nc);
        grow(s.grp_ids, (size_t)E * G, oc, nc);
        grow(s.rid, E, oc, nc);
        s.cap = nc;
        MFX_HIP_THROW(launch_rid_fill(s, oc, stream));   // new slots: slot == id until renumbered
        MFX_HIP_THROW(hipStreamSynchronize(stream));
    }
    if (need_actions > s.acap) {
        int na = std::max(128, s.acap);
        while (na < need_actions) na *= 2;
        const int oa = s.acap;
        grow(s.atk, E, oa, na); grow(s.mov, E, oa, na); grow(d_sort, E, oa, na);
        if (s.ev) (void)hipFree(s.ev);
        alloc(s.ev, 1 + (size_t)3 * na);
        MFX_HIP_THROW(hipMemset(s.ev, 0, sizeof(int32_t)));
        s.acap = na;
    }
}

int BattleEngine::reset() {
    MFX_CHECK(flush_deferred());
    touch();
    for (int g = 0; g < kMaxGroups; g++) acts_since_step[g] = 0;
    ro_prep_stale = true;
    MFX_CHECK(build_params());
    try {
        const int G = n_groups();
        if (!allocated) {
            MFX_HIP_THROW(hipGetDevice(&device));
            if (!stream_set) { MFX_HIP_THROW(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)); own_stream = true; }
            s.E = E;
            s.cells_n = W * H;
            alloc(s.cells, (size_t)E * W * H);
            alloc(s.grp_n, (size_t)E * G); alloc(s.grp_dead, (size_t)E * G); alloc(s.grp_reward, (size_t)E * G);
            alloc(s.id_counter, E); alloc(s.rng, E); alloc(s.n_atk, E); alloc(s.n_mov, E); alloc(s.done, E);
            alloc(s.idx_mark, E); alloc(s.rid_off, E);
            if (food) alloc(s.food, (size_t)E * W * H);
            MFX_HIP_THROW(hipMemset(s.grp_reward, 0, sizeof(float) * E * G));   // Group ctor
            alloc(d_gp, 1); alloc(d_err, 1);
            MFX_HIP_THROW(hipMemset(d_err, 0, sizeof(int32_t)));
            s.err = d_err;
            std::vector<uint32_t> h((size_t)E, rng_init);
            MFX_HIP_THROW(hipMemcpy(s.rng, h.data(), sizeof(uint32_t) * E, hipMemcpyHostToDevice));
            group_ub.assign(G, 0);
            allocated = true;
            ensure_capacity(64, 128);
        } else if (s.cells_n != W * H) {
            return fail("map size changed after the first reset");
        }
        if (food && !s.food) alloc(s.food, (size_t)E * W * H);
        MFX_HIP_THROW(hipMemcpyAsync(d_gp, &gp, sizeof(GameParams), hipMemcpyHostToDevice, stream));
        MFX_HIP_THROW(launch_reset(d_gp, s, stream));
        cells_stale = false;
        next_file();                              // GridWorld.cc:102
        max_ids = 0;
        std::fill(group_ub.begin(), group_ub.end(), 0);
        pending_ub = 0;
        return 0;
    } catch (const HipFailure& f) {
        return fail("%s", f.what());
    }
}

// same placement for every env (host arrays)
int BattleEngine::add_agents(int group, int n, const char* method, const int* xs, const int* ys, const int* dirs) {
    MFX_CHECK(flush_deferred());
    touch();
    ro_prep_stale = true;
    if (!allocated) return fail("add_agents before reset");
    if (group >= n_groups() || group < -1) return fail("invalid group handle in add_agents: %d", group);
    MFX_CHECK(sync_cells());
    if (group < 0 && rollout_ready) walls_after_init = true;
    int m, count;
    std::vector<int> hx, hy, hd;
    if (!strcmp(method, "custom")) {
        m = 0; count = n;
        hx.assign(xs, xs + n); hy.assign(ys, ys + n);
        if (group >= 0) {                                  // GridWorld.cc:259-261
            hd.assign((size_t)n, kDirNorth);
            for (int i = 0; i < n && dirs; i++) {
                if (dirs[i] >= 4) return fail("invalid direction in GridWorld::add_agent");
                hd[i] = dirs[i];
            }
        }
    } else if (!strcmp(method, "random")) {
        m = 1; count = n;
    } else if (!strcmp(method, "fill")) {
        m = 2; count = std::max(0, xs[2]) * std::max(0, xs[3]);
        hx.assign(xs, xs + (turn && group >= 0 ? 5 : 4));   // {x, y, w, h, dir} (GridWorld.cc:270-273)
        if (turn && group >= 0 && (hx[4] < 0 || hx[4] >= 4)) return fail("invalid direction in GridWorld::add_agent");
    } else return fail("unsupported method in add_agents: %s", method);
    try {
        if (group >= 0) {
            ensure_capacity(max_ids + count, 0);
            max_ids += count;
            group_ub[group] += count;
        }
        if (hx.empty()) hx.push_back(0);
        if (hy.empty()) hy.push_back(0);
        if (hd.empty()) hd.push_back(kDirNorth);
        st_xs.ensure(hx.size()); st_ys.ensure(hy.size()); st_dirs.ensure(hd.size());
        MFX_HIP_THROW(hipMemcpyAsync(st_xs.p, hx.data(), sizeof(int) * hx.size(), hipMemcpyHostToDevice, stream));
        MFX_HIP_THROW(hipMemcpyAsync(st_ys.p, hy.data(), sizeof(int) * hy.size(), hipMemcpyHostToDevice, stream));
        MFX_HIP_THROW(hipMemcpyAsync(st_dirs.p, hd.data(), sizeof(int) * hd.size(), hipMemcpyHostToDevice, stream));
        MFX_HIP_THROW(launch_add_agents(d_gp, s, group, n, m, st_xs.p, st_ys.p, st_dirs.p, 0, stream));
        MFX_HIP_THROW(hipStreamSynchronize(stream));   // host vectors go out of scope
        return check_err();
    } catch (const HipFailure& f) {
        return fail("%s", f.what());
    }
}

// GridWorld::set_goal (GridWorld.cc:729-740): "random" only, goals never read back.
int BattleEngine::set_goal(int group, const char* method) {
    MFX_CHECK(flush_deferred());
    touch();
    if (strcmp(method, "random")) return fail("invalid goal type in GridWorld::set_goal");
    if (!allocated || group < 0 || group >= n_groups()) return fail("set_goal: bad state or group");
    MFX_HIP(launch_set_goal_random(d_gp, s, group, stream));
    MFX_HIP(hipStreamSynchronize(stream));
    return 0;
}

int BattleEngine::check_err() {
    MFX_CHECK(quiesce());
    int32_t h = 0;
    MFX_HIP(hipMemcpyAsync(&h, d_err, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    MFX_HIP(hipStreamSynchronize(stream));
    if (h) {
        MFX_HIP(hipMemsetAsync(d_err, 0, sizeof(int32_t), stream));
        static const char* msg[] = {"", "", "agent capacity exceeded", "no blank position for random placement",
                                    "output row capacity smaller than the group", "invalid action id",
                                    "action buffer overflow", "move claim table outside the step scratch"};
        return fail("device error %d: %s", h, h > 0 && h < 8 ? msg[h] : "unknown");
    }
    return 0;
}

int BattleEngine::report_err(int32_t h) {
    if (!h) return 0;
    MFX_CHECK(quiesce());
    MFX_HIP(hipMemsetAsync(d_err, 0, sizeof(int32_t), stream));
    static const char* msg[] = {"", "", "agent capacity exceeded", "no blank position for random placement",
                                "output row capacity smaller than the group", "invalid action id",
                                "action buffer overflow", "move claim table outside the step scratch"};
    return fail("device error %d: %s", h, h > 0 && h < 8 ? msg[h] : "unknown");
}

// ------------------------------------------------------------------ batched device API
// The fused rollout keeps the cells in LDS only; rebuild State::cells before the per-call path
// (or anything else that reads them) runs after rollout steps.
int BattleEngine::sync_cells() {
    if (!cells_stale) return 0;
    MFX_HIP(launch_rebuild_cells(d_gp, s, ro_walls.p, stream));
    cells_stale = false;
    return 0;
}

int BattleEngine::observe(int g, float* d_view, float* d_feat, int rowcap) {
    if (!allocated || g < 0 || g >= n_groups()) return fail("observe: bad state or group");
    MFX_CHECK(flush_deferred());
    MFX_CHECK(sync_cells());
    MFX_HIP(launch_observe(gp, d_gp, s, g, group_ub[g], d_view, d_feat, rowcap, stream));
    return 0;
}
int BattleEngine::set_action(int g, const int* d_actions, int rowcap) {
    MFX_CHECK(flush_deferred());
    touch();
    if (g >= 0 && g < kMaxGroups) acts_since_step[g]++;
    if (!allocated || g < 0 || g >= n_groups()) return fail("set_action: bad state or group");
    pending_ub += group_ub[g];
    try { ensure_capacity(0, pending_ub); } catch (const HipFailure& f) { return fail("%s", f.what()); }
    MFX_HIP(launch_set_action(d_gp, s, g, d_actions, rowcap, stream));
    return 0;
}
// A group's set_action called twice before a step: the serial forms (see State::serial_step).
void BattleEngine::begin_step() {
    s.serial_step = 0;
    for (int g = 0; g < kMaxGroups; g++) { s.serial_step |= acts_since_step[g] > 1; acts_since_step[g] = 0; }
}
int BattleEngine::step(int* d_done) {
    MFX_CHECK(flush_deferred());
    touch();
    ro_prep_stale = true;
    if (!allocated) return fail("step before reset");
    MFX_CHECK(sync_cells());
    begin_step();
    const hipError_t le = launch_step(gp, d_gp, s, max_ids, d_sort, stream);
    s.serial_step = 0;
    MFX_HIP(le);
    pending_ub = 0;
    if (d_done) MFX_HIP(hipMemcpyAsync(d_done, s.done, sizeof(int32_t) * E, hipMemcpyDeviceToDevice, stream));
    return 0;
}
int BattleEngine::get(int g, int what, void* d_out, int rowcap) {
    if (!allocated || g < 0 || g >= n_groups()) return fail("get: bad state or group");
    MFX_CHECK(flush_deferred());
    MFX_HIP(launch_get(d_gp, s, g, what, d_out, rowcap, stream));
    return 0;
}
int BattleEngine::clear_dead() {
    MFX_CHECK(flush_deferred());
    touch();
    ro_prep_stale = true;
    if (!allocated) return fail("clear_dead before reset");
    MFX_HIP(launch_clear_dead(d_gp, s, stream));
    return 0;
}

}  // namespace mfx
