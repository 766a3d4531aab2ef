// tests/cpp/visible_demo_scene.cpp — GpuSceneMirror::SetBounds / ClearBounds / FetchVisible in resident mode on the entities of
// tests/golden/demo_scene.json (plus a child and an entity without bounds): the ids come in ascending index order and the
// fetched Transform::world equal, bit for bit, what a second mirror in coherent mode copied back for the same entities.
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

static bool same_world(bge::Scene& a, bge::Scene& b, const Ids& ids)
{
    for (auto id : ids) {
        if (std::memcmp(a.GetTransform(id)->world, b.GetTransform(id)->world, 64) != 0) return false;
    }
    return true;
}
static void scrub(bge::Scene& s, const Ids& ids)
{
    for (auto id : ids) std::memset(s.GetTransform(id)->world, 0xee, 64);
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
    bge::Scene coherent, resident;
    Ids ids, ids2;
    if (!build(ss.str(), coherent, ids) || !build(ss.str(), resident, ids2) || ids != ids2 || ids.size() != 5) {
        std::printf("scene did not load\n");
        return 3;
    }
    Mirror mc, mr;
    mr.resident = true;
    const float lo[3] = {-0.5f, -0.5f, -0.5f}, hi[3] = {0.5f, 0.5f, 0.5f};
    for (size_t k = 0; k + 1 < ids.size(); ++k) mr.SetBounds(ids[k], lo, hi); // (the last entity has none)
    expect(mc.UpdateTransforms(coherent) && mr.UpdateTransforms(resident), "both mirrors tick");
    const Ids with_bounds(ids.begin(), ids.end() - 1);
    scrub(resident, ids);
    Ids got;
    expect(mr.FetchVisible(resident, nullptr, 0, got), "FetchVisible without planes");
    expect(got == with_bounds, "no planes: every entity with bounds, ascending");
    expect(same_world(coherent, resident, with_bounds), "their Transform::world equal coherent mode's bit for bit");
    unsigned char untouched[64];
    std::memset(untouched, 0xee, 64);
    expect(std::memcmp(resident.GetTransform(ids.back())->world, untouched, 64) == 0, "an entity that is not listed is not written");

    // x >= 2.5: the checkpoint (x = 5) and its child (x = 6); the two small entities at x = 0 are outside
    const float right[1][4] = {{1.0f, 0.0f, 0.0f, -2.5f}};
    scrub(resident, ids);
    expect(mr.FetchVisible(resident, right, 1, got) && got == Ids({ids[2], ids[3]}), "one plane: the checkpoint and its child");
    expect(same_world(coherent, resident, got), "and their matrices");

    // a view-projection through the static helper: the identity keeps |x|, |y| <= 1 and 0 <= z <= 1, which only the thin
    // ground slab at the origin reaches
    const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    float planes[6][4];
    Mirror::FrustumPlanes(identity, false, planes);
    expect(planes[0][0] == 1.0f && planes[0][3] == 1.0f && planes[5][2] == -1.0f && planes[4][2] == 1.0f && planes[4][3] == 0.0f,
           "FrustumPlanes of the identity");
    expect(mr.FetchVisible(resident, planes, 6, got) && got == Ids({ids[1]}), "the clip-space cube holds the ground slab only");

    // bounds go, an entity moves: the next Update sends both
    mr.ClearBounds(ids[2]);
    for (bge::Scene* s : {&coherent, &resident}) {
        auto* t = s->GetTransform(ids[0]);
        t->position = bge::float3{4.0f, 7.0f, -5.0f};
        t->MarkDirty();
    }
    expect(mc.UpdateTransforms(coherent) && mr.UpdateTransforms(resident), "second tick");
    scrub(resident, ids);
    expect(mr.FetchVisible(resident, right, 1, got) && got == Ids({ids[0], ids[3]}), "after ClearBounds and a move: the moved entity and the child");
    expect(same_world(coherent, resident, got), "and their matrices");

    // a destroyed entity leaves the list; the entity that takes its place starts without bounds
    mr.ClearBounds(ids[1]);
    for (bge::Scene* s : {&coherent, &resident}) s->DestroyEntity(ids[1]);
    expect(mc.UpdateTransforms(coherent) && mr.UpdateTransforms(resident), "third tick (an entity is gone)");
    expect(mr.FetchVisible(resident, nullptr, 0, got) && got == Ids({ids[0], ids[3]}), "it is no longer listed");
    Mirror::Id fresh = 0;
    for (bge::Scene* s : {&coherent, &resident}) {
        fresh = s->CreateEntity();
        s->AddTransform(fresh)->position = bge::float3{9.0f, 0.0f, 0.0f};
    }
    expect(mc.UpdateTransforms(coherent) && mr.UpdateTransforms(resident), "fourth tick (a new entity)");
    expect(mr.FetchVisible(resident, nullptr, 0, got) && got == Ids({ids[0], ids[3]}), "the new entity has no bounds yet");
    mr.SetBounds(fresh, lo, hi);
    scrub(resident, got);
    expect(mr.FetchVisible(resident, right, 1, got) && got.size() == 3, "until it is given some");
    expect(same_world(coherent, resident, got), "and the matrices agree again");

    const float many[17][4] = {};
    expect(!mr.FetchVisible(resident, many, 17, got) && got.empty(), "17 planes are refused");
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
