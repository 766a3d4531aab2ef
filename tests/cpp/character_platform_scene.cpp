// tests/cpp/character_platform_scene.cpp — GpuPhysicsSystem's platform riding on the entities of tests/golden/demo_scene.json plus
// a Kinematic box that the game moves through its Transform every frame: with SetCharacterPlatformRiding(true) the character that
// stands on the box follows it and GetCharacterRide names the box; with riding off again the box leaves from under it.
//
// The platform is the box of half extents (2, 0.25, 2) at (0, 3, 0): its top is y = 3.25.  The character has the Config's radius
// 0.35 (skin 0.01), so it rests at y = 3.61 on the platform and at 0.99 + 0.36 = 1.35 on Ground.  A frame moves the platform by
// 0.05 in +x, runs one physics Update of 1/60 s and the characters' steps for its sub-steps.
// Exit 0 = all checks passed, 77 = no usable GPU, anything else = a failed check (printed).
#include <cmath>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "../../banggameengine_amd/host/bge/gpu_systems.hpp"
#include "../../banggameengine_amd/host/bge/scene.hpp"
#include "../../banggameengine_amd/host/bge/scene_json.hpp"

static int failures = 0;
static void expect(bool ok, const char* what)
{
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) ++failures;
}
static bool near(float a, float b, float tol) { return std::fabs(a - b) <= tol; }

// the file keeps position / rotationEuler / scale on the entity itself, and a box collider with a Static body on Ground
static bool build(const std::string& text, bge::Scene& scene, bge::EntityId& ground)
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
        ground = id;
    }
    return true;
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
    bge::EntityId ground = bge::kInvalidEntity;
    if (!build(ss.str(), scene, ground)) return 3;
    expect(ground != bge::kInvalidEntity, "Ground found");
    const bge::EntityId platform = scene.CreateEntity();
    {
        auto* t = scene.AddTransform(platform);
        t->position = bge::float3{0.0f, 3.0f, 0.0f};
        t->MarkDirty();
        auto* c = scene.AddCollider(platform);
        c->shape = bge::ColliderShape::Box;
        c->size = bge::float3{2.0f, 0.25f, 2.0f};
        auto* b = scene.AddRigidBody(platform);
        b->type = bge::RigidBodyType::Kinematic;
    }
    const float rest_on_platform = 3.25f + 0.36f, rest_on_ground = 0.99f + 0.36f;
    const bge::EntityId player = scene.CreateEntity();
    {
        auto* t = scene.AddTransform(player);
        t->position = bge::float3{0.0f, rest_on_platform + 0.01f, 0.0f};
        t->MarkDirty();
    }

    bge::GpuPhysicsSystem<bge::Scene> physics;
    using State = bge::GpuCharacterState<bge::float3>;
    using Ride = bge::GpuCharacterRide<bge::float3>;
    const float dt = 1.0f / 60.0f;
    for (int i = 0; i < 3; ++i) {
        physics.Update(scene, 1.0 / 120.0);
        bge::GpuTransformSystem<bge::Scene>::Update(scene);
    }
    State s;
    Ride r;
    physics.SetCharacterPlatformRiding(true);
    expect(physics.AddCharacter(player) && !physics.GetCharacterRide(player, r), "AddCharacter; no ride record before the first sync");
    expect(physics.UpdateCharacters(dt, 2) && physics.SyncCharacters(scene) && physics.GetCharacterState(player, s) && physics.GetCharacterRide(player, r),
           "two steps and a sync");
    expect(s.grounded && s.groundEntity == platform && near(s.position.y, rest_on_platform, 1e-4f), "it landed on the platform's top at y = 3.25 + radius + skin");
    expect(r.platform == platform && !r.carried && !r.lost && r.turn[3] == 1.0f, "GetCharacterRide names the platform; nothing carried yet");

    // riding on: the platform moves 0.05 a frame and the character with it
    int frames_carried = 0, frames_off_ground = 0;
    float seen_x = 0.0f; // where the platform was at the last physics sub-step, which is where the queries see it
    for (int frame = 0; frame < 60; ++frame) {
        auto* t = scene.GetTransform(platform);
        t->position.x += 0.05f;
        t->MarkDirty();
        physics.Update(scene, 1.0 / 60.0);
        bge::GpuTransformSystem<bge::Scene>::Update(scene);
        const int sub = physics.LastSubSteps();
        if (sub > 0) seen_x = t->position.x;
        if (!(physics.UpdateCharacters(dt, static_cast<uint32_t>(sub)) && physics.SyncCharacters(scene) && physics.GetCharacterState(player, s) &&
              physics.GetCharacterRide(player, r))) {
            ++failures;
        }
        if (r.carried) ++frames_carried;
        if (!s.grounded) ++frames_off_ground;
    }
    std::printf("riding on: platform at x = %.4f (seen at %.4f), character at (%.4f, %.4f, %.4f), carried in %d frames\n", scene.GetTransform(platform)->position.x,
                seen_x, s.position.x, s.position.y, s.position.z, frames_carried);
    expect(seen_x > 2.9f && near(s.position.x, seen_x, 1e-3f) && s.position.z == 0.0f, "the character followed the platform: 3 along +x");
    expect(frames_off_ground == 0 && s.groundEntity == platform && near(s.position.y, rest_on_platform, 1e-4f), "GROUNDED on the platform in every frame");
    expect(frames_carried >= 50 && r.platform == platform && !r.lost, "carried frame after frame; GetCharacterRide names the platform");
    expect(scene.GetTransform(player)->position.x == s.position.x, "SyncCharacters wrote the Transform");

    // riding off: the platform leaves from under the character
    physics.SetCharacterPlatformRiding(false);
    const float left_at = s.position.x;
    for (int frame = 0; frame < 90; ++frame) {
        auto* t = scene.GetTransform(platform);
        t->position.x += 0.05f;
        t->MarkDirty();
        physics.Update(scene, 1.0 / 60.0);
        bge::GpuTransformSystem<bge::Scene>::Update(scene);
        if (!(physics.UpdateCharacters(dt, static_cast<uint32_t>(physics.LastSubSteps())) && physics.SyncCharacters(scene) && physics.GetCharacterState(player, s))) {
            ++failures;
        }
    }
    std::printf("riding off: platform at x = %.4f, character at (%.4f, %.4f, %.4f)\n", scene.GetTransform(platform)->position.x, s.position.x, s.position.y,
                s.position.z);
    expect(near(s.position.x, left_at, 1e-3f) && !physics.GetCharacterRide(player, r), "with riding off the character does not follow; no ride record");
    expect(s.grounded && s.groundEntity == ground && near(s.position.y, rest_on_ground, 1e-4f), "the platform left: it fell onto Ground");
    physics.RemoveCharacters();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
