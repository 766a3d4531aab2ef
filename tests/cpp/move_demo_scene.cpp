// tests/cpp/move_demo_scene.cpp — GpuPhysicsSystem::MoveSphere on the entities of tests/golden/demo_scene.json: a sphere is walked
// across the Static box "Ground" with gravity folded into the displacement, one move per frame, until it leaves the box's edge and
// falls to the ground plane.
//
// Ground is the box of half extents (50, 1, 50) at y = -0.01: its top is y = 0.99 and its edge x = 50.  The sphere has radius 0.5
// and skin 0.01 and every call asks (0.2, -0.2, 0).  Falling, it meets the top where its centre is at 0.99 + 0.5 = 1.49; the
// approach has a L = |r.y| = 0.2, so the back-off skin / (a L) of the path is exactly skin of height: the centre comes to rest at
// y = 0.99 + radius + skin = 1.5.  From there a call meets the top at f = skin / 0.2, g = f - skin / 0.2 = 0: it stays, the
// leftover (1 - f) r slides to (0.19, 0, 0) and the second round is free: 0.19 forward per call at y = 1.5, and the probe of 0.1
// finds Ground at distance skin with normal +y.  Past the edge the same happens on the plane y = 0 at y = 0.51.
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

    bge::GpuPhysicsSystem<bge::Scene> physics;
    using Result = bge::GpuSphereMoveResult<bge::float3>;
    const float radius = 0.5f, skin = 0.01f, probe = 0.1f, slope = 0.7853982f;
    const bge::float3 step{0.2f, -0.2f, 0.0f};
    bge::float3 at{35.0f, 2.15f, 0.0f};
    Result res;
    expect(!physics.MoveSphere(at, step, radius, skin, probe, slope, 3u, res) && res.position.x == at.x && res.position.y == at.y,
           "no world before the first Update: the position is echoed");
    for (int i = 0; i < 3; ++i) {
        physics.Update(scene, 1.0 / 120.0);
        bge::GpuTransformSystem<bge::Scene>::Update(scene);
    }
    const float rest = 0.99f + radius + skin, rest_plane = radius + skin;
    bool all_valid = true, height_ok = true, grounded_ok = true, fell = false, one_round_trip = true;
    int landed_at = -1, left_at = -1, on_plane_at = -1;
    for (int call = 0; call < 120; ++call) {
        all_valid &= physics.MoveSphere(at, step, radius, skin, probe, slope, 3u, res);
        at = res.position;
        one_round_trip &= !res.outOfSlides && res.remaining.x == 0.0f && res.remaining.y == 0.0f && res.remaining.z == 0.0f;
        if (landed_at < 0 && res.hits > 0 && res.grounded) landed_at = call; // (the probe sees Ground one call before the touch)
        if (landed_at >= 0 && at.x <= 49.5f) { // on Ground's top, clear of its rounded edge
            height_ok &= near(at.y, rest, 1e-4f);
            grounded_ok &= res.grounded && res.groundEntity == ground && !res.groundTrigger && near(res.groundDistance, skin, 1e-4f) &&
                           res.groundNormal.y == 1.0f;
        }
        if (left_at < 0 && at.x > 50.5f) left_at = call;
        if (left_at >= 0 && !res.grounded) fell = true;
        if (on_plane_at < 0 && left_at >= 0 && res.grounded && res.groundEntity == bge::kInvalidEntity) on_plane_at = call;
    }
    std::printf("landed at call %d, past the edge at call %d, on the plane at call %d; ends at (%.4f, %.4f, %.4f)\n", landed_at, left_at,
                on_plane_at, at.x, at.y, at.z);
    expect(all_valid && one_round_trip, "every move is valid and spends its displacement");
    expect(landed_at >= 0 && landed_at <= 4, "lands on Ground within the first calls");
    expect(height_ok, "stays at y = 0.99 + radius + skin on Ground");
    expect(grounded_ok, "GROUNDED on Ground every call after landing, at distance skin, normal +y");
    expect(left_at > landed_at && fell, "leaves the edge and falls");
    expect(on_plane_at > left_at && res.grounded && res.groundEntity == bge::kInvalidEntity && near(at.y, rest_plane, 1e-4f) && at.x > 52.0f,
           "comes to rest on the plane at y = radius + skin and walks on");
    expect(at.z == 0.0f, "never leaves the plane of the motion");
    // the batched form gives the same as one call each
    std::vector<bge::GpuSphereMover<bge::float3>> movers(3);
    std::vector<Result> many;
    for (int i = 0; i < 3; ++i) {
        movers[i].position = bge::float3{10.0f * static_cast<float>(i), 2.15f, 1.0f};
        movers[i].displacement = step;
        movers[i].probeDistance = probe;
        movers[i].layerMask = 3u;
    }
    movers[2].skin = 0.0f; // invalid
    bool same = physics.MoveSpheres(movers, many) && many.size() == 3 && !many[2].valid && many[2].position.y == 2.15f;
    for (int i = 0; i < 2 && same; ++i) {
        Result one;
        same &= physics.MoveSphere(movers[i].position, step, 0.5f, 0.01f, probe, slope, 3u, one);
        same &= one.position.x == many[i].position.x && one.position.y == many[i].position.y && one.grounded == many[i].grounded && one.hits == many[i].hits;
    }
    expect(same, "MoveSpheres equals MoveSphere per mover; an invalid mover is reported and echoed");
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
