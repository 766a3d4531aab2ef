// tests/cpp/batches_demo_scene.cpp — GpuSceneMirror::SetDrawKey / ClearDrawKey / FetchDrawBatches in resident mode on the
// entities of tests/golden/demo_scene.json (plus a child and an entity without bounds): the ids come grouped by three keys in
// record order, and the fetched Transform::world equal, bit for bit, what FetchWorld copies for the same entities.
// Exit 0 = all checks passed, 77 = no usable GPU, anything else = a failed check (printed).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../banggameengine_amd/host/bge/gpu_systems.hpp"
#include "../../banggameengine_amd/host/bge/scene.hpp"
#include "../../banggameengine_amd/host/bge/scene_json.hpp"

static int failures = 0;
static void expect(bool ok, const char* what)
{
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) ++failures;
}

using Mirror = bge::GpuSceneMirror<bge::Scene>;
using Ids = std::vector<Mirror::Id>;
using Batches = std::vector<bge_draw_batch>;

// the file keeps position / rotationEuler / scale on the entity itself; returns the ids in file order, then a child of the last
// entity and a free-standing entity that never gets bounds
static bool build(const std::string& text, bge::Scene& scene, Ids& ids)
{
    bge::json::Value root;
    bge::json::Parser parser(text);
    std::string err;
    if (!parser.parse(root, &err)) return false;
    const bge::json::Value* entities = root.find("entities");
    if (!entities) return false;
    for (const bge::json::Value& e : entities->arr) {
        const auto id = scene.CreateEntity();
        auto* t = scene.AddTransform(id);
        bge::detail::read_vec3(e, "position", t->position);
        bge::detail::read_vec3(e, "rotationEuler", t->rotationEuler);
        bge::detail::read_vec3(e, "scale", t->scale);
        t->MarkDirty();
        ids.push_back(id);
    }
    const auto child = scene.CreateEntity();
    auto* ct = scene.AddTransform(child);
    ct->position = bge::float3{1.0f, 2.0f, 3.0f};
    ct->rotationEuler = bge::float3{0.3f, -0.2f, 0.1f};
    ct->MarkDirty();
    scene.SetParent(child, ids.back());
    ids.push_back(child);
    const auto bare = scene.CreateEntity();
    scene.AddTransform(bare)->position = bge::float3{6.0f, 0.0f, 0.0f};
    ids.push_back(bare);
    return true;
}

static bool same(const Batches& got, const std::vector<std::pair<uint32_t, uint32_t>>& want)
{
    if (got.size() != want.size()) return false;
    for (size_t k = 0; k < got.size(); ++k) {
        if (got[k].first_instance != want[k].first || got[k].instance_count != want[k].second) return false;
    }
    return true;
}

// the listed entities' Transform::world as FetchDrawBatches left them against what FetchWorld writes
static bool worlds_equal_fetch_world(Mirror& m, bge::Scene& scene, const Ids& listed)
{
    std::vector<float> kept;
    for (auto id : listed) kept.insert(kept.end(), scene.GetTransform(id)->world, scene.GetTransform(id)->world + 16);
    for (auto id : listed) std::memset(scene.GetTransform(id)->world, 0xee, 64);
    if (!m.FetchWorld(scene, listed)) return false;
    for (size_t k = 0; k < listed.size(); ++k) {
        if (std::memcmp(&kept[16 * k], scene.GetTransform(listed[k])->world, 64) != 0) return false;
    }
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    {
        Mirror probe;
        if (!probe.ok()) {
            std::printf("no usable GPU\n");
            return 77;
        }
    }
    std::ifstream f(argv[1]);
    std::stringstream ss;
    ss << f.rdbuf();
    bge::Scene scene;
    Ids ids;
    if (!build(ss.str(), scene, ids) || ids.size() != 5) {
        std::printf("scene did not load\n");
        return 3;
    }
    Mirror m;
    m.resident = true;
    const float lo[3] = {-0.5f, -0.5f, -0.5f}, hi[3] = {0.5f, 0.5f, 0.5f};
    for (size_t k = 0; k + 1 < ids.size(); ++k) m.SetBounds(ids[k], lo, hi); // (the last entity has none)
    m.SetDrawKey(ids[0], 2);
    m.SetDrawKey(ids[1], 0);
    m.SetDrawKey(ids[2], 2);
    m.SetDrawKey(ids[3], 1);
    m.SetDrawKey(ids[4], 0); // a key without bounds: not renderable, not listed
    expect(m.UpdateTransforms(scene), "the mirror ticks");
    for (auto id : ids) std::memset(scene.GetTransform(id)->world, 0xee, 64);
    Batches batches;
    Ids got;
    expect(m.FetchDrawBatches(scene, nullptr, 0, 3, batches, got), "FetchDrawBatches without planes");
    expect(got == Ids({ids[1], ids[3], ids[0], ids[2]}), "three keys: out follows record order (key, then index)");
    expect(same(batches, {{0, 1}, {1, 1}, {2, 2}}), "and the batches are their ranges");
    unsigned char untouched[64];
    std::memset(untouched, 0xee, 64);
    expect(std::memcmp(scene.GetTransform(ids[4])->world, untouched, 64) == 0, "an entity that is not listed is not written");
    expect(worlds_equal_fetch_world(m, scene, got), "Transform::world of each listed entity equals FetchWorld's");

    // fewer keys than in use: key 2 is left out
    expect(m.FetchDrawBatches(scene, nullptr, 0, 2, batches, got) && got == Ids({ids[1], ids[3]}) && same(batches, {{0, 1}, {1, 1}}),
           "n_keys = 2 leaves key 2 out");

    // x >= 2.5: the checkpoint (key 2) and its child (key 1); an empty batch in front
    const float right[1][4] = {{1.0f, 0.0f, 0.0f, -2.5f}};
    expect(m.FetchDrawBatches(scene, right, 1, 4, batches, got) && got == Ids({ids[3], ids[2]}), "one plane: the child, then the checkpoint");
    expect(same(batches, {{0, 0}, {0, 1}, {1, 1}, {2, 0}}), "empty batches keep their place");
    expect(worlds_equal_fetch_world(m, scene, got), "and their matrices");

    // ClearDrawKey: the entity leaves the result without another tick
    m.ClearDrawKey(ids[0]);
    expect(m.FetchDrawBatches(scene, nullptr, 0, 3, batches, got) && got == Ids({ids[1], ids[3], ids[2]}) && same(batches, {{0, 1}, {1, 1}, {2, 1}}),
           "after ClearDrawKey the entity is gone");
    m.SetDrawKey(ids[0], 1);
    expect(m.FetchDrawBatches(scene, nullptr, 0, 3, batches, got) && got == Ids({ids[1], ids[0], ids[3], ids[2]}) && same(batches, {{0, 1}, {1, 2}, {3, 1}}),
           "and back under another key");

    // a destroyed entity leaves; the entity that takes its place starts without a key
    m.ClearBounds(ids[1]);
    m.ClearDrawKey(ids[1]);
    scene.DestroyEntity(ids[1]);
    expect(m.UpdateTransforms(scene), "second tick (an entity is gone)");
    expect(m.FetchDrawBatches(scene, nullptr, 0, 3, batches, got) && got == Ids({ids[0], ids[3], ids[2]}) && same(batches, {{0, 0}, {0, 2}, {2, 1}}),
           "it is no longer listed");
    const auto fresh = scene.CreateEntity();
    scene.AddTransform(fresh)->position = bge::float3{9.0f, 0.0f, 0.0f};
    m.SetBounds(fresh, lo, hi);
    expect(m.UpdateTransforms(scene), "third tick (a new entity)");
    expect(m.FetchDrawBatches(scene, nullptr, 0, 3, batches, got) && got.size() == 3, "the new entity has no key yet");
    m.SetDrawKey(fresh, 0);
    expect(m.FetchDrawBatches(scene, nullptr, 0, 3, batches, got) && got.size() == 4 && got[0] == fresh && same(batches, {{0, 1}, {1, 2}, {3, 1}}),
           "until it is given one");
    expect(worlds_equal_fetch_world(m, scene, got), "and the matrices agree");

    expect(!m.FetchDrawBatches(scene, nullptr, 0, 0, batches, got) && got.empty() && batches.empty(), "n_keys = 0 is refused");
    expect(!m.FetchDrawBatches(scene, nullptr, 0, 65537, batches, got) && got.empty() && batches.empty(), "n_keys = 65537 is refused");
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
