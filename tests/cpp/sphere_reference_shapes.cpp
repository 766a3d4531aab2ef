// tests/cpp/sphere_reference_shapes.cpp — compile-only: GpuPhysicsSystem::SphereCast / SphereCastAll / OverlapSphere (extensions
// without a reference counterpart) on types with the reference's member signatures (reference_shapes_mock.hpp) and a
// PhysicsRaycastHit shaped as src/physics/PhysicsAPI.h:12-18: a ground check and a proximity query after an Update.
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

std::string GroundLine(bge::GpuPhysicsSystem<Scene>& physics, Scene& scene, const Camera& camera, const InputSystem& input, double dt)
{
    physics.Update(scene, camera, input, dt);
    std::string line;
    PhysicsRaycastHit hit{};
    float3 feet{0.0f, 1.0f, 0.0f};
    float3 down{0.0f, -1.0f, 0.0f};
    constexpr uint32_t kWorldLayerMask = 1u;
    if (physics.SphereCast(feet, down, 0.6f, 0.4f, kWorldLayerMask, hit)) {
        char buffer[128];
        std::snprintf(buffer, sizeof(buffer), "Ground: %u @ (%.2f, %.2f, %.2f) d=%.2f", static_cast<unsigned>(hit.entity), hit.point.x,
                      hit.point.y, hit.point.z, hit.distance);
        line = buffer;
    }
    const std::vector<PhysicsRaycastHit> all = physics.SphereCastAll<PhysicsRaycastHit>(feet, down, 0.6f, 0.4f, kWorldLayerMask);
    const std::vector<bge::GpuOverlapHit> near = physics.OverlapSphere(feet, 5.0f, 0xffffffffu);
    for (const bge::GpuOverlapHit& h : near) line += h.trigger ? 't' : 'b';
    return line + std::to_string(all.size());
}
