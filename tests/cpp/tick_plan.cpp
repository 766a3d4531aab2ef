// tick_plan.cpp — what a tick call decides (csrc/bge_tick_plan.hpp TickKnobs, TickPlan, TickGroups) on its own, against the
// expressions tick_impl computed inline before the header existed.  parent_plan() and parent_ticks() are those lines, copied: `w->`
// reaches a stand-in with members of the same names, std::getenv became env.get, and where tick_impl enqueued the zeroing of the adv
// words the copy records it.  Every combination of flags, scene and switches is compared field for field; the properties the
// source-text tests used to read off the spelling of those lines are asserted on the values.
// Built with -fsanitize=address,undefined by tests/test_tick_plan_cpu.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bge_tick_plan.hpp"

#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) {                                                              \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

namespace {

constexpr uint32_t kFuseTicksDefault = 8, kSoloTicksDefault = 512; // the values of the lines copied below, not the header's
constexpr double kNtThresholdBytes = 300.0e6;
static_assert(bge::kFuseTicksDefault == kFuseTicksDefault && bge::kSoloTicksDefault == kSoloTicksDefault && bge::kNtThresholdBytes == kNtThresholdBytes,
              "a default moved: a change of behaviour, not of this refactor");

const char* const kNames[7] = {"BGE_NT_STORES", "BGE_DEFER_ROW3", "BGE_WORLD_ROWS", "BGE_FLAG_WORD", "BGE_REST_PATH", "BGE_FUSE_TICKS", "BGE_SOLO_GROUPS"};

struct Env {
    const char* value[7]; // by kNames; nullptr: unset
    const char* get(const char* name) const
    {
        switch (name[4]) { // BGE_N, BGE_D, BGE_W, BGE_FL / BGE_FU, BGE_R, BGE_S
        case 'N': return value[0];
        case 'D': return value[1];
        case 'W': return value[2];
        case 'F': return name[5] == 'L' ? value[3] : value[5];
        case 'R': return value[4];
        default: return value[6];
        }
    }
};

// what the copied lines read of bge_world
struct World {
    struct {
        uint64_t n_slots;
        struct {
            size_t n;
            size_t size() const { return n; }
        } pass_tile_begin;
    } flat;
    bool any_frozen, ground_plane, static_contacts, dynamic_contacts;
    struct {
        bool all_flat, any_flat_all_dynamic;
    } shape;
    int profiling;
    bge::Row3State row3;
    bge::FuseClock fuse;
};

struct ParentPlan {
    bool nt_out, contacts, can_defer, rows_path, defer_row3, flag_word, rest_path, fusable, solo;
    uint32_t fuse_T;
};

ParentPlan parent_plan(const World* w, uint32_t flags, const Env& env)
{
    const bool phys = (flags & BGE_TICK_PHYSICS) != 0;
    const bool xform = (flags & BGE_TICK_TRANSFORMS) != 0;
    bool nt_out = static_cast<double>(w->flat.n_slots) * ((flags & BGE_TICK_NORMAL_MATRICES) ? 204.0 : 140.0) > kNtThresholdBytes;
    if (const char* e = env.get("BGE_NT_STORES")) nt_out = std::atoi(e) != 0;
    const bool contacts = phys && (w->ground_plane || w->static_contacts || w->dynamic_contacts);
    bool defer_env = true;
    if (const char* e = env.get("BGE_DEFER_ROW3")) defer_env = std::atoi(e) != 0;
    const bool can_defer = w->row3.may_defer(true, w->flat.pass_tile_begin.size() - 1, w->any_frozen, defer_env);
    bool rows_path = xform && !contacts && (!nt_out || can_defer) &&
                     !(flags & (BGE_TICK_AABBS | BGE_TICK_BROADPHASE | BGE_TICK_NORMAL_MATRICES | BGE_TICK_BULLET_BASIS | BGE_TICK_GATHER_ROOTS));
    if (const char* e = env.get("BGE_WORLD_ROWS")) rows_path = rows_path && std::atoi(e) != 0;
    const bool defer_row3 = rows_path && can_defer;
    bool flag_word = rows_path;
    if (const char* e = env.get("BGE_FLAG_WORD")) flag_word = flag_word && std::atoi(e) != 0;
    bool rest_path = xform && !(flags & (BGE_TICK_AABBS | BGE_TICK_BROADPHASE | BGE_TICK_NORMAL_MATRICES | BGE_TICK_BULLET_BASIS | BGE_TICK_GATHER_ROOTS));
    if (const char* e = env.get("BGE_REST_PATH")) rest_path = rest_path && std::atoi(e) != 0;
    uint32_t fuse_T = kFuseTicksDefault;
    const char* const fuse_env = env.get("BGE_FUSE_TICKS");
    if (fuse_env) fuse_T = static_cast<uint32_t>(std::max(1, std::atoi(fuse_env)));
    const bool fusable = phys && rows_path && flag_word && w->flat.pass_tile_begin.size() - 1 == 1 && !w->any_frozen && w->profiling != 2 && w->shape.any_flat_all_dynamic;
    bool solo_env = true;
    if (const char* e = env.get("BGE_SOLO_GROUPS")) solo_env = std::atoi(e) != 0;
    const bool solo = bge::SoloPlan::wanted(fusable, w->shape.all_flat, solo_env);
    if (solo && !fuse_env) fuse_T = kSoloTicksDefault; // (a solo group costs one launch whatever its size: its default is its own)
    return ParentPlan{nt_out, contacts, can_defer, rows_path, defer_row3, flag_word, rest_path, fusable, solo, fuse_T};
}

struct ParentTick {
    uint32_t serial, n_left, n_solo;
    bool launch, zeroed;
};

std::vector<ParentTick> parent_ticks(World* w, bool fusable, bool solo, uint32_t fuse_T, uint32_t ticks)
{
    std::vector<ParentTick> out;
    uint32_t group_first = 0, group_t0 = 0, group_n = 0; // the group tick t belongs to: its first serial, its first tick, its size
    for (uint32_t t = 0; t < ticks; ++t) {
        ParentTick p{};
        if (fusable && fuse_T > 1u && t == group_t0 + group_n) {
            group_t0 = t;
            group_n = bge::FuseClock::group_size(t, ticks, fuse_T);
            bool wrapped = false;
            if (!solo) group_first = w->fuse.begin_group(group_n, &wrapped); // (a solo group carries no serial)
            if (wrapped) p.zeroed = true;
        }
        // (a group of one tick has nothing to fuse: it goes out as every tick did, and no word is loaded)
        const bool fused = fusable && fuse_T > 1u && group_n > 1u && !solo;
        p.serial = fused ? group_first + (t - group_t0) : 0u;
        p.n_left = fused ? group_n - (t - group_t0) : 1u;
        const bge::SoloPlan plan = bge::SoloPlan::plan(solo && fuse_T > 1u, t - group_t0, group_n);
        p.n_solo = plan.n_solo;
        p.launch = plan.launch;
        out.push_back(p);
    }
    return out;
}

void set_env(const Env& env)
{
    for (int i = 0; i < 7; ++i) {
        if (env.value[i]) CHECK(setenv(kNames[i], env.value[i], 1) == 0);
        else CHECK(unsetenv(kNames[i]) == 0);
    }
}

uint64_t plans_checked = 0, rest_with_contacts = 0;

// every flags value and every scene under one environment
void check_plans(const Env& env, const bge::TickKnobs& knobs)
{
    const uint64_t sizes[3] = {1000000u, 1800000u, 4000000u}; // below 300e6 / 204, between that and 300e6 / 140, above
    static_assert(1000000 * 204.0 < 300.0e6 && 1800000 * 204.0 > 300.0e6 && 1800000 * 140.0 < 300.0e6 && 4000000 * 140.0 > 300.0e6, "");
    for (uint32_t scene = 0; scene < 3u * 2u * 2u * 2u * 2u * 2u * 3u * 2u; ++scene) {
        uint32_t r = scene;
        const auto take = [&r](uint32_t n) {
            const uint32_t v = r % n;
            r /= n;
            return v;
        };
        World w{};
        w.flat.n_slots = sizes[take(3)];
        w.flat.pass_tile_begin.n = 2u + take(2);
        w.any_frozen = take(2) != 0;
        w.ground_plane = take(2) != 0;
        w.shape.all_flat = take(2) != 0;
        w.shape.any_flat_all_dynamic = take(2) != 0;
        w.profiling = static_cast<int>(take(3));
        w.row3.pinned = take(2) != 0;
        const bge::TickScene s{w.flat.n_slots, w.flat.pass_tile_begin.n - 1, w.any_frozen, w.ground_plane, w.shape.all_flat, w.shape.any_flat_all_dynamic, w.profiling};
        for (uint32_t flags = 0; flags < 128u; ++flags) {
            const ParentPlan want = parent_plan(&w, flags, env);
            const bge::TickPlan got = bge::TickPlan::of(flags, s, knobs, w.row3);
            CHECK(got.nt_out == want.nt_out);
            CHECK(got.contacts == want.contacts);
            CHECK(got.rows_path == want.rows_path);
            CHECK(got.defer_row3 == want.defer_row3);
            CHECK(got.flag_word == want.flag_word);
            CHECK(got.rest_path == want.rest_path);
            CHECK(got.fusable == want.fusable);
            CHECK(got.solo == want.solo);
            CHECK(got.group_T == want.fuse_T);
            // the properties
            const bool phys = (flags & BGE_TICK_PHYSICS) != 0;
            if (got.fusable) {
                CHECK(phys && got.rows_path && got.flag_word && s.n_passes == 1 && !s.any_frozen && s.profiling != 2 && s.any_flat_all_dynamic);
            }
            if (got.solo) CHECK(got.fusable && s.all_flat && knobs.solo_groups);
            if (got.defer_row3) CHECK(got.rows_path && s.n_passes == 1 && !s.any_frozen && !w.row3.pinned);
            if (got.flag_word) CHECK(got.rows_path);
            CHECK(got.group_T >= 1u);
            // the variants as launch_tick decodes them (bge_kernels.hip)
            const bool in_variant = bge::tick_variant_has_rows_path((flags & 2u) != 0, (flags & (4u | 32u)) != 0, (flags & 16u) != 0, phys && (flags & 64u) != 0);
            if (!in_variant) CHECK(!got.rows_path && !got.rest_path);
            if (phys && w.ground_plane) {
                CHECK(got.contacts && !got.rows_path);
                rest_with_contacts += got.rest_path ? 1u : 0u;
            }
            ++plans_checked;
        }
    }
}

uint64_t calls_checked = 0;

void check_call(bool fusable, bool solo, uint32_t T, uint32_t K, uint32_t clock_start)
{
    World w{};
    w.fuse.next = clock_start;
    const std::vector<ParentTick> want = parent_ticks(&w, fusable, solo, T, K);
    bge::TickPlan plan{};
    plan.fusable = fusable;
    plan.solo = solo;
    plan.group_T = T;
    bge::FuseClock clock;
    clock.next = clock_start;
    bge::TickGroups groups(plan, K);
    std::vector<uint32_t> covered(K, 0);
    uint32_t group_t0 = 0, zeroings = 0;
    for (uint32_t t = 0; t < K; ++t) {
        const bge::TickGroups::Tick got = groups.next(t, clock);
        CHECK(got.serial == want[t].serial);
        CHECK(got.n_left == want[t].n_left);
        CHECK(got.n_solo == want[t].n_solo);
        CHECK(got.launch == want[t].launch);
        CHECK(got.clear_adv == want[t].zeroed);
        // the properties
        if (got.serial != 0u) CHECK(fusable && !solo && got.launch && got.n_left >= 1u && got.n_left <= T);
        else CHECK(got.n_left == 1u);
        if (got.n_solo > 1u) {
            CHECK(solo && got.launch && got.serial == 0u && t == group_t0 && got.n_solo == bge::FuseClock::group_size(t, K, T));
            group_t0 = t + got.n_solo; // (where the next group begins)
        } else if (got.launch && solo) {
            group_t0 = t + 1u;
        }
        if (got.clear_adv) CHECK(got.serial == 1u && !solo);
        zeroings += got.clear_adv ? 1u : 0u;
        for (uint32_t i = 0; got.launch && i < std::max(got.n_solo, 1u); ++i) {
            CHECK(t + i < K);
            covered[t + i]++;
        }
    }
    for (uint32_t c : covered) CHECK(c == 1u); // every tick is in exactly one launch's count
    CHECK(clock.next == w.fuse.next);
    if (solo || !fusable) CHECK(clock.next == clock_start && zeroings == 0u); // no serial was handed out
    ++calls_checked;
}

} // namespace

int main()
{
    // ---- TickKnobs::from_env reads the environment at every call: nothing is cached
    CHECK(clearenv() == 0);
    {
        const bge::TickKnobs unset = bge::TickKnobs::from_env(), none;
        CHECK(unset.nt_stores == -1 && unset.world_rows && unset.defer_row3 && unset.flag_word && unset.rest_path && unset.solo_groups && unset.fuse_ticks == 0u);
        CHECK(none.nt_stores == -1 && none.world_rows && none.defer_row3 && none.flag_word && none.rest_path && none.solo_groups && none.fuse_ticks == 0u);
        CHECK(setenv("BGE_SOLO_GROUPS", "0", 1) == 0);
        CHECK(!bge::TickKnobs::from_env().solo_groups);
        CHECK(setenv("BGE_SOLO_GROUPS", "1", 1) == 0);
        CHECK(bge::TickKnobs::from_env().solo_groups);
        CHECK(unsetenv("BGE_SOLO_GROUPS") == 0);
        CHECK(bge::TickKnobs::from_env().solo_groups);
        CHECK(setenv("BGE_FUSE_TICKS", "1", 1) == 0);
        CHECK(bge::TickKnobs::from_env().fuse_ticks == 1u);
        CHECK(setenv("BGE_FUSE_TICKS", "32", 1) == 0);
        CHECK(bge::TickKnobs::from_env().fuse_ticks == 32u);
        CHECK(setenv("BGE_FUSE_TICKS", "0", 1) == 0);
        CHECK(bge::TickKnobs::from_env().fuse_ticks == 1u); // max(1, atoi): set, so the solo default does not apply
        CHECK(setenv("BGE_FUSE_TICKS", "-3", 1) == 0);
        CHECK(bge::TickKnobs::from_env().fuse_ticks == 1u);
        CHECK(unsetenv("BGE_FUSE_TICKS") == 0);
        CHECK(bge::TickKnobs::from_env().fuse_ticks == 0u);
        CHECK(setenv("BGE_NT_STORES", "0", 1) == 0);
        CHECK(bge::TickKnobs::from_env().nt_stores == 0);
        CHECK(setenv("BGE_NT_STORES", "1", 1) == 0);
        CHECK(bge::TickKnobs::from_env().nt_stores == 1);
        CHECK(unsetenv("BGE_NT_STORES") == 0);
        CHECK(bge::TickKnobs::from_env().nt_stores == -1);
    }

    // ---- the plan: 3 x 2^5 x 4 environments (each really set, and read back by from_env), all scenes, all flags
    const char* const nt_values[3] = {nullptr, "0", "1"};
    const char* const fuse_values[4] = {nullptr, "1", "2", "8"};
    for (uint32_t e = 0; e < 3u * 32u * 4u; ++e) {
        Env env{};
        env.value[0] = nt_values[e % 3u];
        const uint32_t bits = (e / 3u) % 32u;
        const int boolean[5] = {1, 2, 3, 4, 6}; // kNames: the switches that default to on
        for (int b = 0; b < 5; ++b) env.value[boolean[b]] = (bits >> b & 1u) ? "0" : nullptr;
        env.value[5] = fuse_values[e / 96u];
        set_env(env);
        const bge::TickKnobs knobs = bge::TickKnobs::from_env();
        for (int i = 0; i < 7; ++i) CHECK(env.get(kNames[i]) == env.value[i]);
        check_plans(env, knobs);
    }
    CHECK(plans_checked == 384ull * 576ull * 128ull);
    CHECK(rest_with_contacts > 0u); // the rest path lives with the contact stages; the translation-row path does not
    // "1" for a switch reads as unset does
    {
        Env env{};
        for (int b : {1, 2, 3, 4, 6}) env.value[b] = "1";
        set_env(env);
        check_plans(env, bge::TickKnobs::from_env());
        const bge::TickKnobs k = bge::TickKnobs::from_env();
        CHECK(k.world_rows && k.defer_row3 && k.flag_word && k.rest_path && k.solo_groups);
    }

    // ---- the groups of a call
    const uint32_t Ks[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 17, 1000}, Ts[] = {1, 2, 3, 8, 32};
    for (uint32_t T : Ts) {
        for (uint32_t K : Ks) {
            for (uint32_t start : {1u, 0xfffffff0u}) { // (from 0xfffffff0 a group wraps)
                check_call(true, false, T, K, start);
                check_call(true, true, T, K, start);
                check_call(false, false, T, K, start);
            }
        }
    }
    // one group of the call wraps, and only its first launch carries the zeroing
    {
        bge::TickPlan plan{};
        plan.fusable = true;
        plan.group_T = 8;
        bge::FuseClock clock;
        clock.next = 0xfffffff0u;
        bge::TickGroups groups(plan, 40);
        uint32_t zeroings = 0;
        for (uint32_t t = 0; t < 40; ++t) {
            const bge::TickGroups::Tick g = groups.next(t, clock);
            CHECK(g.serial != 0u && g.launch && g.n_solo == 0u);
            if (g.clear_adv) {
                ++zeroings;
                CHECK(t % 8u == 0u && g.serial == 1u);
            }
        }
        CHECK(zeroings == 1u);
    }
    CHECK(calls_checked == 5u * 11u * 2u * 3u);
    std::printf("tick_plan ok\n");
    return 0;
}
