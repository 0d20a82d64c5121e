// battle_render.cpp -- the Battle engine's get_info answers, render (frames of env 0) and the recording helpers.
#include "battle_engine.h"

namespace mfx {

int BattleEngine::get_info(int group, const char* name, void* buf) {   // GridWorld.cc:777-978
    int* ib = (int*)buf;
    const int G = n_groups();
    const bool need_group = strcmp(name, "both_attack") != 0;
    if (need_group && (group < 0 || group >= G)) return fail("invalid group %d for get_info(%s)", group, name);
    if (!strcmp(name, "num")) { if (!allocated) { ib[0] = 0; return 0; } ib[0] = num_env0(group); return 0; }
    if (!strcmp(name, "id")) return host_get(group, kGetId, buf, 4);
    if (!strcmp(name, "pos")) return host_get(group, kGetPos, buf, 8);
    if (!strcmp(name, "alive")) return host_get(group, kGetAlive, buf, 1);
    AgentTypeSpec& t = gtype(group);
    if (!strcmp(name, "action_space")) { ib[0] = t.n_action; return 0; }
    if (!strcmp(name, "view_space")) { ib[0] = t.view.h; ib[1] = t.view.w; ib[2] = group2channel(G); return 0; }
    if (!strcmp(name, "feature_space")) { ib[0] = feature_size(group); return 0; }
    if (!strcmp(name, "attack_base")) { ib[0] = t.attack_base; return 0; }
    if (!strcmp(name, "view2attack")) {
        for (int i = 0; i < t.view.w * t.view.h; i++) ib[i] = -1;
        for (int i = 0; i < t.attack.count; i++)
            ib[(t.attack.dy[i] - t.view.y1) * t.view.w + (t.attack.dx[i] - t.view.x1)] = i;
        return 0;
    }
    if (!strcmp(name, "move_delta")) {                           // (not in the reference: mfx_rule_create's move table)
        for (int i = 0; i < t.move.count; i++) { ib[2 * i] = t.move.dx[i]; ib[2 * i + 1] = t.move.dy[i]; }
        return 0;
    }
    if (!strcmp(name, "both_attack")) { ib[0] = 0; return 0; }   // statistics are compiled off (GridWorld.cc:501)
    if (!strcmp(name, "mean_info")) return mean_info(group, (float*)buf);
    return fail("unsupported info name in get_info: %s", name);
}

// ---- rendering (GridWorld.cc:1023-1033, RenderGenerator.cc): frames of env 0
void BattleEngine::start_recording() {                      // events are kept once first_render is false
    if (!first_render) return;
    first_render = false;
    gp.record_events = 1;
    if (allocated) MFX_HIP_THROW(hipMemcpy(d_gp, &gp, sizeof(GameParams), hipMemcpyHostToDevice));
}

std::vector<int> BattleEngine::attack_events() {            // (id, x, y) triples of the last step
    std::vector<int> ev;
    if (first_render || !allocated) return ev;
    MFX_HIP_THROW(hipStreamSynchronize(stream));
    int n = 0;
    MFX_HIP_THROW(hipMemcpy(&n, s.ev, sizeof(int), hipMemcpyDeviceToHost));
    ev.resize((size_t)3 * n);
    if (n) MFX_HIP_THROW(hipMemcpy(ev.data(), s.ev + 1, sizeof(int) * ev.size(), hipMemcpyDeviceToHost));
    return ev;
}

static std::string rgba(int r, int g, int b, float alpha) {
    std::stringstream ss;
    ss << "\"rgba(" << r << "," << g << "," << b << "," << alpha << ")\"";
    return ss.str();
}

template <class T> static void json(std::ofstream& os, const char* key, T value, bool last = false) {
    os << "\"" << key << "\": " << value;
    os << (last ? "" : ",") << std::endl;
}

void BattleEngine::gen_config() {                           // RenderGenerator.cc:58-111
    static const int colors[4][3] = {{192, 64, 64}, {64, 64, 192}, {64, 192, 64}, {64, 64, 64}};
    std::ofstream f(render_dir + "/" + "config.json");
    f << "{" << std::endl;
    json(f, "width", W);
    json(f, "height", H);
    json(f, "static-file", "\"static.map\"");
    json(f, "obstacle-style", rgba(127, 127, 127, 1));
    json(f, "dynamic-file-directory", "\".\"");
    json(f, "attack-style", rgba(63, 63, 63, 0.8f));
    json(f, "minimap-width", 300);
    json(f, "minimap-height", 250);
    f << "\"group\" : [" << std::endl;
    const int G = n_groups();
    for (int i = 0; i < G; i++) {
        const AgentTypeSpec& t = gtype(i);
        const int* c = colors[i];
        f << "{" << std::endl;
        json(f, "height", t.length);
        json(f, "width", t.width);
        json(f, "style", rgba(c[0], c[1], c[2], 1));
        json(f, "anchor", "[0, 0]");
        json(f, "max-speed", (int)t.speed);
        json(f, "speed-style", rgba(c[0], c[1], c[2], 0.01f));
        json(f, "vision-radius", t.view_radius);
        json(f, "vision-angle", t.view_angle);
        json(f, "vision-style", rgba(c[0], c[1], c[2], 0.2f));
        json(f, "attack-radius", t.attack_radius);
        json(f, "attack-angle", t.attack_angle);
        json(f, "attack-style", rgba(c[0], c[1], c[2], 0.1f));
        json(f, "broadcast-radius", 1, true);
        f << (i == G - 1 ? "}" : "},") << std::endl;
    }
    f << "]" << std::endl;
    f << "}" << std::endl;
}

int BattleEngine::render() {                                // GridWorld::render + RenderGenerator::render_a_frame
    if (render_dir.empty()) return 0;
    MFX_CHECK(flush_deferred());
    if (render_dir == "___debug___") return 0;   // the reference prints the map to stdout
    try {
        if (first_render) { start_recording(); gen_config(); }
        const int G = n_groups();
        std::ofstream fout(render_dir + "/" + "video_" + std::to_string(file_ct) + ".txt",
                           frame_ct == 0 ? std::ios::out : std::ios::app);
        if (frame_ct == 0) {
            std::vector<int> walls(2 * (size_t)W * H + 2);
            get_info_global(-1, "walls_info", walls.data());
            fout << "W" << " " << walls[0] << std::endl;
            for (int i = 1; i <= walls[0]; i++) fout << walls[2 * i] << " " << walls[2 * i + 1] << std::endl;
        }
        std::vector<int> ev = attack_events();
        // can_absorb groups: only their absorbed agents are drawn (RenderGenerator.cc:129-160)
        std::vector<std::vector<int>> absorbed((size_t)G);
        int num_agents = 0;
        for (int i = 0; i < G && allocated; i++) {
            const int n = num_env0(i);
            num_agents += n;
            if (!gtype(i).can_absorb || !n) continue;
            absorbed[i].resize(n);
            MFX_CHECK(host_get(i, kGetAbsorbed, absorbed[i].data(), 4));
            for (int j = 0; j < n; j++) num_agents -= absorbed[i][j] ? 0 : 1;
        }
        fout << "F" << " " << num_agents << " " << (int)(ev.size() / 3) << " " << 0 << std::endl;
        for (int i = 0; i < G && allocated; i++) {
            const int n = num_env0(i);
            if (!n) continue;
            std::vector<int> ids(n), pos(2 * (size_t)n), dir(n);
            std::vector<float> hp(n);
            MFX_CHECK(host_get(i, kGetId, ids.data(), 4));
            MFX_CHECK(host_get(i, kGetPos, pos.data(), 8));
            MFX_CHECK(host_get(i, kGetHp, hp.data(), 4));
            MFX_CHECK(host_get(i, kGetDir, dir.data(), 4));
            const float max_hp = gtype(i).hp;
            static const int dir2angle[] = {0, 90, 180, 270};   // RenderGenerator.cc:148
            for (int j = 0; j < n; j++) {
                if (!absorbed[i].empty() && !absorbed[i][j]) continue;
                int h = std::max(0, int(100 * hp[j] / max_hp));
                h = std::min(h, 100);
                fout << ids[j] << " " << h << " " << dir2angle[dir[j] & 3] << " " << pos[2 * j] << " "
                     << pos[2 * j + 1] << " " << i << std::endl;
            }
        }
        for (size_t k = 0; k < ev.size(); k += 3)
            fout << 0 << " " << ev[k] << " " << ev[k + 1] << " " << ev[k + 2] << std::endl;
        if (frame_ct++ > frame_per_file) { frame_ct = 0; file_ct++; }
    } catch (const HipFailure& f) {
        return fail("%s", f.what());
    }
    return 0;
}

// ---- get_info extras (GridWorld.cc:811-954), env 0, from the device state
std::vector<int> BattleEngine::group_pos(int g) {              // x, y per agent in group order (dead included)
    const int n = num_env0(g);
    std::vector<int> pos((size_t)2 * std::max(n, 1));
    if (n > 0 && host_get(g, kGetPos, pos.data(), 8) != 0) throw HipFailure("get pos");
    pos.resize((size_t)2 * n);
    return pos;
}

int BattleEngine::mean_info(int group, float* out) {           // GridWorld.cc:832-853
    MFX_CHECK(flush_deferred());
    const int n = num_env0(group), na = gtype(group).n_action;
    if (n == 0) return fail("mean_info of an empty group");          // the reference asserts
    std::vector<int> pos = group_pos(group), act((size_t)n);
    MFX_CHECK(host_get(group, kGetLastAct, act.data(), 4));
    float sum_x = 0, sum_y = 0;
    std::vector<int> counter((size_t)na, 0);
    for (int i = 0; i < n; i++) {
        sum_x += (float)pos[2 * i];
        sum_y += (float)pos[2 * i + 1];
        if (act[i] >= 0 && act[i] < na) counter[act[i]]++;   // before the first set_action the
    }                                                         // reference indexes out of range
    out[0] = sum_x / (float)n;
    out[1] = sum_y / (float)n;
    for (int k = 0; k < na; k++) out[2 + k] = (float)(1.0 * counter[k] / n);
    return 0;
}

// Keys the python wrapper asks with group -1 (gridworld.py:526-636).
int BattleEngine::get_info_global(int group, const char* name, void* buf) {
    MFX_CHECK(sync_cells());
    int* ib = (int*)buf;
    float* fb = (float*)buf;
    const int G = n_groups();
    if (!strcmp(name, "global_minimap")) {       // GridWorld.cc:807-830
        const int vh = (int)lround(fb[0]), vw = (int)lround(fb[1]);
        if (vh <= 0 || vw <= 0) return fail("global_minimap: bad size %d x %d", vh, vw);
        memset(fb, 0, sizeof(float) * vh * vw * G);
        const int sh = (H + vh - 1) / vh, sw = (W + vw - 1) / vw;
        for (int i = 0; i < G; i++) {
            // the reference computes (i - group + n_group) % n_group in size_t; group -1 -> (i+1) % n
            const size_t ch = ((size_t)i - (size_t)(long)group + (size_t)G) % (size_t)G;
            std::vector<int> pos = allocated ? group_pos(i) : std::vector<int>();
            const size_t n = pos.size() / 2;
            for (size_t j = 0; j < n; j++) fb[((size_t)(pos[2 * j + 1] / sh) * vw + pos[2 * j] / sw) * G + ch] += 1.0f;
            for (int y = 0; y < vh; y++)
                for (int x = 0; x < vw; x++) fb[((size_t)y * vw + x) * G + ch] /= (float)n;
        }
        return 0;
    }
    if (!strcmp(name, "walls_info")) {           // GridWorld.cc:854-863, Map.cc:621-627 (scan order)
        std::vector<uint16_t> cells((size_t)W * H);
        if (allocated) MFX_HIP(hipMemcpy(cells.data(), s.cells, cells.size() * 2, hipMemcpyDeviceToHost));
        int n = 0;
        for (int c = 0; c < W * H; c++)
            if (allocated && cells[c] == kCellWall) { ++n; ib[2 * n] = c % W; ib[2 * n + 1] = c / W; }
        ib[0] = n;
        return 0;
    }
    if (!strcmp(name, "render_window_info")) {   // GridWorld.cc:864-896
        const int x1 = ib[0], y1 = ib[1], x2 = ib[2], y2 = ib[3];
        int ct = 1;
        for (int i = 0; i < G; i++) {
            std::vector<int> pos = allocated ? group_pos(i) : std::vector<int>();
            std::vector<int> ids(pos.size() / 2), absorbed;
            if (!ids.empty()) MFX_CHECK(host_get(i, kGetId, ids.data(), 4));
            if (!ids.empty() && gtype(i).can_absorb) {          // GridWorld.cc:905-906
                absorbed.resize(ids.size());
                MFX_CHECK(host_get(i, kGetAbsorbed, absorbed.data(), 4));
            }
            for (size_t j = 0; j < ids.size(); j++) {
                const int x = pos[2 * j], y = pos[2 * j + 1];
                if (x < x1 || x > x2 || y < y1 || y > y2) continue;
                if (!absorbed.empty() && !absorbed[j]) continue;
                ib[4 * ct] = ids[j]; ib[4 * ct + 1] = x; ib[4 * ct + 2] = y; ib[4 * ct + 3] = i;
                ct++;
            }
        }
        ib[0] = ct - 1;
        ib[1] = (int)(attack_events().size() / 3);
        start_recording();                        // GridWorld.cc:882
        return 0;
    }
    if (!strcmp(name, "attack_event")) {         // GridWorld.cc:919-926
        std::vector<int> ev = attack_events();
        std::copy(ev.begin(), ev.end(), ib);
        return 0;
    }
    if (!strcmp(name, "groups_info")) {          // GridWorld.cc:934-949
        static const int colors[4][3] = {{192, 64, 64}, {64, 64, 192}, {64, 192, 64}, {64, 64, 64}};
        for (int i = 0; i < G; i++) {
            ib[5 * i] = 1; ib[5 * i + 1] = 1;     // 1 x 1 bodies (width, length)
            for (int k = 0; k < 3; k++) ib[5 * i + 2 + k] = colors[i][k];
        }
        return 0;
    }
    return get_info(group, name, buf);
}

}  // namespace mfx
