// tests/cpp/move_reference_shapes.cpp — compile-only: GpuPhysicsSystem::MoveSphere / MoveSpheres (extensions without a reference
// counterpart) on types with the reference's member signatures (reference_shapes_mock.hpp): a character frame after an Update —
// a horizontal move, then a vertical move with gravity and the ground probe.
#include <string>
#include <vector>

#include "reference_shapes_mock.hpp"

#include "../../banggameengine_amd/host/bge/gpu_systems.hpp"

std::string CharacterFrame(bge::GpuPhysicsSystem<Scene>& physics, Scene& scene, const Camera& camera, const InputSystem& input, double dt)
{
    physics.Update(scene, camera, input, dt);
    constexpr uint32_t kWorldLayerMask = 3u;
    const float3 feet{0.0f, 1.0f, 0.0f};
    const float3 walk{0.1f, 0.0f, 0.0f};
    bge::GpuSphereMoveResult<float3> moved;
    std::string line;
    if (physics.MoveSphere(feet, walk, 0.4f, 0.01f, 0.0f, 0.7853982f, kWorldLayerMask, moved)) line += moved.hits ? 'h' : 'f';
    const float3 fall{0.0f, -0.05f, 0.0f};
    if (physics.MoveSphere(moved.position, fall, 0.4f, 0.01f, 0.1f, 0.7853982f, kWorldLayerMask, moved) && moved.grounded) {
        line += std::to_string(static_cast<unsigned>(moved.groundEntity));
    }
    std::vector<bge::GpuSphereMover<float3>> crowd(2);
    crowd[1].position = float3{1.0f, 1.0f, 0.0f};
    crowd[1].displacement = walk;
    std::vector<bge::GpuSphereMoveResult<float3>> results;
    if (physics.MoveSpheres(crowd, results)) line += results[1].outOfSlides ? 'o' : (results[1].hitTrigger ? 't' : 'b');
    return line + std::to_string(results.size()) + std::to_string(moved.remaining.x + moved.hitNormal.y + moved.groundNormal.y + moved.groundDistance);
}
