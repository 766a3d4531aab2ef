// tests/cpp/recover_reference_shapes.cpp — compile-only: GpuPhysicsSystem::SpherePenetration / RecoverSphere / RecoverSpheres
// (extensions without a reference counterpart) on types with the reference's member signatures (reference_shapes_mock.hpp): a
// character frame after an Update — out of whatever came to lie on the character, then the move.
#include <string>
#include <vector>

#include "reference_shapes_mock.hpp"

#include "../../banggameengine_amd/host/bge/gpu_systems.hpp"

std::string RecoverFrame(bge::GpuPhysicsSystem<Scene>& physics, Scene& scene, const Camera& camera, const InputSystem& input, double dt)
{
    physics.Update(scene, camera, input, dt);
    constexpr uint32_t kWorldLayerMask = 3u;
    const float3 feet{0.0f, 0.3f, 0.0f};
    std::string line;
    bge::GpuPenetrationHit<float3> deepest;
    if (physics.SpherePenetration(feet, 0.4f, kWorldLayerMask, deepest)) {
        line += deepest.trigger ? 't' : 'b';
        line += std::to_string(static_cast<unsigned>(deepest.entity)) + std::to_string(deepest.depth + deepest.point.y + deepest.normal.y);
    }
    bge::GpuSphereRecoverResult<float3> out;
    if (physics.RecoverSphere(feet, 0.4f, 0.01f, kWorldLayerMask, out)) line += out.stuck ? 's' : (out.moved ? 'm' : 'c');
    bge::GpuSphereMoveResult<float3> moved;
    const float3 walk{0.1f, 0.0f, 0.0f};
    if (physics.MoveSphere(out.position, walk, 0.4f, 0.01f, 0.0f, 0.7853982f, kWorldLayerMask, moved)) line += moved.hits ? 'h' : 'f';
    std::vector<bge::GpuSphereRecover<float3>> crowd(2);
    crowd[1].position = float3{1.0f, 0.2f, 0.0f};
    std::vector<bge::GpuSphereRecoverResult<float3>> results;
    if (physics.RecoverSpheres(crowd, results)) line += results[1].hitTrigger ? 't' : 'b';
    return line + std::to_string(results.size()) + std::to_string(static_cast<unsigned>(out.hitEntity) + out.pushes) +
           std::to_string(out.pushed.y + out.hitNormal.y + out.hitDepth + out.remainingDepth);
}
