// tests/cpp/sphere_demo_scene.cpp — the sphere queries through the C++ adapter on the demo scene in the reference's format: a
// sphere cast down from the camera (the HUD ray's origin, src/core/Application.cpp:258-281) after a physics Update, and an
// overlap sphere around the Checkpoint trigger.
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

struct PhysicsRaycastHit { // src/physics/PhysicsAPI.h:12-18
    bge::EntityId entity = bge::kInvalidEntity;
    bge::float3 point{0.0f, 0.0f, 0.0f};
    bge::float3 normal{0.0f, 1.0f, 0.0f};
    float distance = 0.0f;
};

static int failures = 0;
static void expect(bool ok, const char* what)
{
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) ++failures;
}
static bool near(float a, float b, float tol) { return std::fabs(a - b) <= tol; }

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
    std::string err;
    if (!bge::LoadSceneFromJsonText(ss.str(), scene, &err)) {
        std::printf("scene: %s\n", err.c_str());
        return 3;
    }
    bge::EntityId ground = bge::kInvalidEntity, checkpoint = bge::kInvalidEntity;
    for (auto& kv : scene.GetTransforms()) {
        if (kv.second.position.y == -0.01f) ground = kv.first;
        if (kv.second.position.x == 5.0f && kv.second.position.z == 5.0f) checkpoint = kv.first;
    }
    expect(ground != bge::kInvalidEntity && checkpoint != bge::kInvalidEntity, "Ground and Checkpoint found");

    bge::GpuPhysicsSystem<bge::Scene> physics;
    PhysicsRaycastHit hit;
    const bge::float3 down{0.0f, -1.0f, 0.0f};
    expect(!physics.SphereCast(bge::float3{0.0f, 10.0f, 0.0f}, down, 200.0f, 0.5f, 1u, hit), "no world before the first Update");
    expect(physics.OverlapSphere(bge::float3{0.0f, 1.0f, 0.0f}, 1.0f, 1u).empty(), "no overlap before the first Update");
    for (int i = 0; i < 3; ++i) {
        physics.Update(scene, 1.0 / 120.0);
        bge::GpuTransformSystem<bge::Scene>::Update(scene);
    }
    // Ground's top face is y = -0.01 + 1 = 0.99 (half extents 50 x 1 x 50): a sphere of 0.5 from y = 10 stops with its centre at 1.49
    const float cam_y = 10.0f, radius = 0.5f;
    hit = PhysicsRaycastHit{};
    bool got = physics.SphereCast(bge::float3{0.0f, cam_y, 0.0f}, down, 200.0f, radius, 1u, hit);
    expect(got && hit.entity == ground, "sphere cast down from the camera hits Ground");
    expect(near(hit.point.y, 0.99f, 1e-5f) && near(hit.distance, cam_y - 0.99f - radius, 1e-4f), "contact at y = 0.99, distance origin.y - 0.99 - radius");
    expect(near(hit.point.x, 0.0f, 1e-6f) && near(hit.point.z, 0.0f, 1e-6f), "contact under the centre");
    expect(hit.normal.x == 0.0f && near(hit.normal.y, 1.0f, 1e-6f) && hit.normal.z == 0.0f, "normal +y");
    std::printf("SphereCast: Ground @ (%.2f, %.2f, %.2f) d=%.2f\n", hit.point.x, hit.point.y, hit.point.z, hit.distance);
    // through the Checkpoint trigger (layer 4, box 1.5 at (5, 1, 5), top y = 2.5): every layer sees the trigger, Ground, then the plane
    const std::vector<PhysicsRaycastHit> all =
        physics.SphereCastAll<PhysicsRaycastHit>(bge::float3{5.0f, cam_y, 5.0f}, down, 200.0f, radius, 0xffffffffu);
    expect(all.size() == 3 && all[0].entity == checkpoint && all[1].entity == ground && all[2].entity == bge::kInvalidEntity,
           "SphereCastAll with every layer: Checkpoint, Ground, the plane, in order");
    expect(all.size() == 3 && near(all[0].point.y, 2.5f, 1e-5f) && near(all[2].point.y, 0.0f, 0.0f) && near(all[2].distance, cam_y - radius, 1e-4f),
           "their contact heights 2.5, 0.99, 0");
    // a sphere resting on Ground beside the Checkpoint: the overlap reports what its radius reaches
    std::vector<bge::GpuOverlapHit> found = physics.OverlapSphere(bge::float3{0.0f, 0.99f + 0.5f + 0.25f, 0.0f}, 0.5f, 0xffffffffu);
    expect(found.empty(), "0.25 above Ground with radius 0.5: nothing");
    found = physics.OverlapSphere(bge::float3{0.0f, 0.99f + 0.25f, 0.0f}, 0.5f, 1u);
    expect(found.size() == 1 && found[0].entity == ground && !found[0].trigger && near(found[0].distance, 0.25f, 1e-5f), "0.25 above Ground: Ground at 0.25");
    found = physics.OverlapSphere(bge::float3{5.0f, 1.0f, 5.0f}, 0.1f, 4u);
    expect(found.size() == 1 && found[0].entity == checkpoint && found[0].trigger && found[0].distance == 0.0f, "inside the Checkpoint: distance 0");
    found = physics.OverlapSphere(bge::float3{5.0f, 1.0f, 5.0f}, 2.0f, 0xffffffffu);
    bool has_ground = false, has_checkpoint = false, has_plane = false;
    for (const bge::GpuOverlapHit& h : found) {
        has_ground |= h.entity == ground;
        has_checkpoint |= h.entity == checkpoint && h.trigger;
        has_plane |= h.entity == bge::kInvalidEntity;
    }
    expect(has_ground && has_checkpoint && has_plane && found.back().entity == bge::kInvalidEntity, "radius 2 at the Checkpoint: Ground, Checkpoint, the plane last");
    expect(!physics.SphereCast(bge::float3{0.0f, cam_y, 0.0f}, down, 200.0f, -1.0f, 1u, hit), "negative radius misses");
    expect(!physics.SphereCast(bge::float3{0.0f, cam_y, 0.0f}, down, 0.0f, radius, 1u, hit), "maxDistance 0 misses");
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
