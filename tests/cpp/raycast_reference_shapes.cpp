// tests/cpp/raycast_reference_shapes.cpp — compile-only: GpuPhysicsSystem::Raycast / RaycastAll on types with the reference's
// member signatures (reference_shapes_mock.hpp) and a PhysicsRaycastHit shaped as src/physics/PhysicsAPI.h:12-18, through
// the call Application::Update makes for its HUD line (src/core/Application.cpp:258-281).
#include <cstdio>
#include <string>
#include <vector>

#include "reference_shapes_mock.hpp"

#include "../../banggameengine_amd/host/bge/gpu_systems.hpp"

struct PhysicsRaycastHit {
    EntityId entity = 0;
    float3 point{0.0f, 0.0f, 0.0f};
    float3 normal{0.0f, 1.0f, 0.0f};
    float distance = 0.0f;
};

std::string HudLine(bge::GpuPhysicsSystem<Scene>& physics, Scene& scene, const Camera& camera, const InputSystem& input, double dt)
{
    physics.Update(scene, camera, input, dt);
    std::string physicsLine;
    PhysicsRaycastHit rayHit{};
    float3 origin{0.0f, 10.0f, 0.0f};
    float3 dir{0.0f, -1.0f, 0.0f};
    constexpr uint32_t kWorldLayerMask = 1u;
    if (physics.Raycast(origin, dir, 200.0f, kWorldLayerMask, rayHit)) {
        char buffer[128];
        std::snprintf(buffer, sizeof(buffer), "Raycast: %u @ (%.2f, %.2f, %.2f) d=%.2f", static_cast<unsigned>(rayHit.entity),
                      rayHit.point.x, rayHit.point.y, rayHit.point.z, rayHit.distance);
        physicsLine = buffer;
    } else {
        physicsLine = "Raycast: sin impacto";
    }
    const std::vector<PhysicsRaycastHit> all = physics.RaycastAll<PhysicsRaycastHit>(origin, dir, 200.0f, kWorldLayerMask);
    return physicsLine + std::to_string(all.size());
}
