// tests/cpp/chartrig_demo_scene.cpp — GpuPhysicsSystem's character trigger events on the entities of tests/golden/demo_scene.json
// plus two trigger volumes this program adds: a plain one and a one-shot one.
//
// Ground is the box of half extents (50, 1, 50) at y = -0.01: its top is y = 0.99; the character (radius 0.35, skin 0.01) rests on
// it at y = 1.35.  Its layer mask leaves out the triggers' layer (4), so a volume is not an obstacle for it; the volumes' mask is
// the characters' group (2), so Ground, which reaches into both, is nothing to them.  Both volumes have
// half extents 1: the plain one at (5, 1.5, 0) is fed as x in [3.98, 6.02], the one-shot one stands at (0, 1.5, 5).  The character's
// box reaches radius + 0.02 = 0.37 from its centre, so it overlaps the plain volume for x in [3.61, 6.39]: walking 0.25 a step
// from x = 0 it Enters in step 15 (x = 3.75), Stays in steps 16 .. 25 and Exits in step 26 (x = 6.5).
// Exit 0 = all checks passed, 77 = no usable GPU, anything else = a failed check (printed).
#include <cmath>
#include <cstdio>
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

using Event = bge::GpuTriggerEvent;

// the file keeps position / rotationEuler / scale on the entity itself, and a box collider with a Static body on Ground
static bool build(const std::string& text, bge::Scene& scene)
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
        const bge::json::Value* cj = e.find("collider");
        const bge::json::Value* rj = e.find("rigidBody");
        if (!cj || !rj) continue;
        auto* c = scene.AddCollider(id);
        c->shape = bge::ColliderShape::Box;
        bge::detail::read_vec3(*cj, "size", c->size);
        auto* b = scene.AddRigidBody(id);
        b->type = bge::RigidBodyType::Static;
        b->layer = static_cast<uint32_t>(bge::detail::read_float(*rj, "layer", 1.0f));
    }
    return true;
}

static bge::EntityId add_volume(bge::Scene& scene, bge::float3 at, bool one_shot)
{
    const bge::EntityId id = scene.CreateEntity();
    auto* t = scene.AddTransform(id);
    t->position = at;
    t->MarkDirty();
    auto* v = scene.AddTriggerVolume(id);
    v->size = bge::float3{1.0f, 1.0f, 1.0f};
    v->mask = 2u; // the characters' group alone: Ground (layer 1) under the volume does not fire it in the world's own trigger pass
    v->oneShot = one_shot;
    return id;
}

static bge::EntityId add_entity_at(bge::Scene& scene, bge::float3 at)
{
    const bge::EntityId id = scene.CreateEntity();
    auto* t = scene.AddTransform(id);
    t->position = at;
    t->MarkDirty();
    return id;
}

static int active_triggers(bge_world* world)
{
    uint32_t index[64];
    uint8_t active[64];
    for (uint32_t i = 0; i < 64; ++i) index[i] = i;
    if (bge_world_trigger_active(world, 64, index, active) != BGE_OK) return -1;
    int n = 0;
    for (uint8_t a : active) n += a;
    return n;
}

static bool same(const Event& e, Event::Type type, bge::EntityId trigger, bge::EntityId other)
{
    return e.type == type && e.trigger == trigger && e.other == other;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    {
        bge::GpuSceneMirror<bge::Scene> probe;
        if (!probe.ok()) {
            std::printf("no usable GPU\n");
            return 77;
        }
    }
    std::ifstream f(argv[1]);
    std::stringstream ss;
    ss << f.rdbuf();
    bge::Scene scene;
    if (!build(ss.str(), scene)) return 3;
    const float rest = 0.99f + 0.36f, dt = 1.0f / 60.0f;
    const bge::EntityId plain = add_volume(scene, bge::float3{5.0f, 1.5f, 0.0f}, false);
    const bge::EntityId once = add_volume(scene, bge::float3{0.0f, 1.5f, 5.0f}, true);
    const bge::EntityId player = add_entity_at(scene, bge::float3{0.0f, rest + 0.01f, 0.0f});
    const bge::EntityId second = add_entity_at(scene, bge::float3{-20.0f, rest + 0.01f, -20.0f});

    bge::GpuPhysicsSystem<bge::Scene> physics;
    auto frame_of_physics = [&] {
        physics.Update(scene, 1.0 / 120.0);
        bge::GpuTransformSystem<bge::Scene>::Update(scene);
    };
    for (int i = 0; i < 3; ++i) frame_of_physics();
    bge::GpuSceneMirror<bge::Scene>& mirror = bge::GpuMirrors<bge::Scene>::Of(scene);
    expect(active_triggers(mirror.world()) == 2, "both volumes are active in the world");
    bge::GpuCharacterKnobs knobs;
    knobs.layerMask = ~4u; // everything but the triggers' layer: a volume is no obstacle
    expect(physics.CharacterTriggerEvents().empty(), "no events before anything is watched");
    physics.SetCharacterTriggerEvents(true);
    expect(mirror.AddCharacter(scene, player, knobs), "AddCharacter");
    auto frame = [&]() -> const std::vector<Event>& {
        if (!(physics.UpdateCharacters(dt, 1) && physics.SyncCharacters(scene))) ++failures;
        return physics.CharacterTriggerEvents();
    };
    expect(frame().empty() && frame().empty(), "the character lands clear of both volumes: no events");

    // through the plain volume
    expect(physics.SetCharacterWalk(player, 0.25f, 0.0f), "SetCharacterWalk");
    std::string seen;
    int bad = 0;
    for (int step = 1; step <= 30; ++step) {
        const std::vector<Event>& ev = frame();
        if (ev.size() > 1) ++bad;
        for (const Event& e : ev) {
            if (e.trigger != plain || e.other != player) ++bad;
            seen += e.type == Event::Type::Enter ? 'E' : (e.type == Event::Type::Stay ? 'S' : 'X');
        }
        if (ev.empty()) seen += '.';
    }
    std::printf("walk: %s\n", seen.c_str());
    expect(bad == 0 && seen == "..............ESSSSSSSSSSX....", "Enter in step 15, Stay in steps 16 .. 25, Exit in step 26, nothing else");
    expect(physics.TriggerEvents(scene).empty(), "the world's own trigger events do not see the character");

    // a second character is added while the first stands in the plain volume: the first Stays, it does not Enter again
    expect(physics.SetCharacterWalk(player, 0.0f, 0.0f) && physics.WarpCharacter(player, bge::float3{5.0f, rest + 0.01f, 0.0f}), "warp into the plain volume");
    {
        const std::vector<Event>& ev = frame();
        expect(ev.size() == 1 && same(ev[0], Event::Type::Enter, plain, player), "the warp Enters it");
    }
    {
        const std::vector<Event>& ev = frame();
        expect(ev.size() == 1 && same(ev[0], Event::Type::Stay, plain, player), "then it Stays");
    }
    expect(mirror.AddCharacter(scene, second, knobs) && mirror.CharacterCount() == 2, "a second character, far from both volumes");
    {
        const std::vector<Event>& ev = frame();
        expect(ev.size() == 1 && same(ev[0], Event::Type::Stay, plain, player), "the set was re-created: the first character Stays, nobody Enters");
    }

    // the one-shot volume: Enter once, then it is out of the world
    expect(physics.WarpCharacter(player, bge::float3{0.0f, rest + 0.01f, 5.0f}), "warp into the one-shot volume");
    {
        const std::vector<Event>& ev = frame();
        expect(ev.size() == 2 && same(ev[0], Event::Type::Exit, plain, player) && same(ev[1], Event::Type::Enter, once, player),
               "Exit of the plain volume, then Enter of the one-shot one: the order of the trigger array");
    }
    expect(!scene.GetTriggerVolume(once)->active && scene.GetTriggerVolume(plain)->active, "the one-shot volume is switched off in the scene");
    for (int i = 0; i < 2; ++i) frame_of_physics(); // (two frames of 1/120 s hold a sub-step: the re-sent volumes are posed again)
    expect(active_triggers(mirror.world()) == 1, "after the next trigger upload it is inactive in the world");
    expect(frame().empty() && frame().empty(), "it reports nothing further: no Stay, no Exit");
    expect(physics.WarpCharacter(second, bge::float3{5.0f, rest + 0.01f, 0.0f}), "the second character into the plain volume");
    {
        const std::vector<Event>& ev = frame();
        expect(ev.size() == 1 && same(ev[0], Event::Type::Enter, plain, second), "the plain volume still reports");
    }
    physics.SetCharacterTriggerEvents(false);
    expect(frame().empty() && physics.CharacterTriggerEvents().empty(), "switched off: no events");
    physics.RemoveCharacters();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
