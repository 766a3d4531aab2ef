// tests/cpp/raycast_demo_scene.cpp — the reference's HUD ray (src/core/Application.cpp:258-281) through the C++ adapter on the
// demo scene in the reference's format: Raycast(camera, (0, -1, 0), 200, kWorldLayerMask = 1) after a physics Update.
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
    expect(!physics.Raycast(bge::float3{0.0f, 10.0f, 0.0f}, bge::float3{0.0f, -1.0f, 0.0f}, 200.0f, 1u, hit), "no world before the first Update");
    for (int i = 0; i < 3; ++i) {
        physics.Update(scene, 1.0 / 120.0);
        bge::GpuTransformSystem<bge::Scene>::Update(scene);
    }
    // the HUD call: Ground's top face is y = -0.01 + 1 = 0.99 (half extents 50 x 1 x 50)
    const float cam_y = 10.0f;
    hit = PhysicsRaycastHit{};
    bool got = physics.Raycast(bge::float3{0.0f, cam_y, 0.0f}, bge::float3{0.0f, -1.0f, 0.0f}, 200.0f, 1u, hit);
    expect(got && hit.entity == ground, "HUD ray hits Ground");
    expect(near(hit.point.y, 0.99f, 1e-5f) && near(hit.distance, cam_y - 0.99f, 1e-4f), "at y = 0.99, distance origin.y - 0.99");
    expect(hit.normal.x == 0.0f && near(hit.normal.y, 1.0f, 1e-6f) && hit.normal.z == 0.0f, "normal +y");
    std::printf("Raycast: Ground @ (%.2f, %.2f, %.2f) d=%.2f\n", hit.point.x, hit.point.y, hit.point.z, hit.distance);
    // through the Checkpoint trigger (layer 4, box 1.5 at (5, 1, 5)): mask 1 sees Ground, mask 4 the trigger's top at y = 2.5
    hit = PhysicsRaycastHit{};
    got = physics.Raycast(bge::float3{5.0f, cam_y, 5.0f}, bge::float3{0.0f, -1.0f, 0.0f}, 200.0f, 1u, hit);
    expect(got && hit.entity == ground && near(hit.point.y, 0.99f, 1e-5f), "mask 1 through the Checkpoint hits Ground");
    hit = PhysicsRaycastHit{};
    got = physics.Raycast(bge::float3{5.0f, cam_y, 5.0f}, bge::float3{0.0f, -1.0f, 0.0f}, 200.0f, 4u, hit);
    expect(got && hit.entity == checkpoint && near(hit.point.y, 2.5f, 1e-5f), "mask 4 hits the Checkpoint");
    // mask 1 never sees the plane (group StaticFilter = 2); mask 2 sees it, with kInvalidEntity, under the Ground box's layer
    const std::vector<PhysicsRaycastHit> all =
        physics.RaycastAll<PhysicsRaycastHit>(bge::float3{5.0f, cam_y, 5.0f}, bge::float3{0.0f, -1.0f, 0.0f}, 200.0f, 0xffffffffu);
    expect(all.size() == 3 && all[0].entity == checkpoint && all[1].entity == ground && all[2].entity == bge::kInvalidEntity &&
               near(all[2].point.y, 0.0f, 1e-5f),
           "RaycastAll with every layer: Checkpoint, Ground, the plane, in order");
    hit = PhysicsRaycastHit{};
    got = physics.Raycast(bge::float3{100.0f, cam_y, 0.0f}, bge::float3{0.0f, -1.0f, 0.0f}, 200.0f, 2u, hit);
    expect(got && hit.entity == bge::kInvalidEntity && near(hit.point.y, 0.0f, 1e-6f) && hit.normal.y == 1.0f,
           "mask 2 beside Ground: the plane, kInvalidEntity, normal +y");
    expect(!physics.Raycast(bge::float3{100.0f, cam_y, 0.0f}, bge::float3{0.0f, -1.0f, 0.0f}, 200.0f, 1u, hit), "mask 1 beside Ground: nothing");
    expect(!physics.Raycast(bge::float3{0.0f, cam_y, 0.0f}, bge::float3{0.0f, -1.0f, 0.0f}, 0.0f, 1u, hit), "maxDistance 0 misses");
    expect(!physics.Raycast(bge::float3{0.0f, cam_y, 0.0f}, bge::float3{0.0f, -1.0f, 0.0f}, 200.0f, 0u, hit), "layerMask 0 misses");
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
