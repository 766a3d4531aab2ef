// tests/cpp/step_reference_shapes.cpp — compile-only: GpuPhysicsSystem::StepMoveSphere / StepMoveSpheres (extensions without a
// reference counterpart) on types with the reference's member signatures (reference_shapes_mock.hpp): a character frame after an
// Update — the walk as a step move, then a vertical move with gravity and the ground probe.
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
    bge::GpuSphereStepResult<float3> walked;
    std::string line;
    if (physics.StepMoveSphere(feet, walk, 0.4f, 0.01f, 0.1f, 0.7853982f, kWorldLayerMask, 0.3f, walked)) {
        line += walked.stepped ? 's' : (walked.stepTried ? 't' : (walked.hits ? 'h' : 'f'));
    }
    const float3 fall{0.0f, -0.05f, 0.0f};
    bge::GpuSphereMoveResult<float3> moved;
    if (physics.MoveSphere(walked.position, fall, 0.4f, 0.01f, 0.1f, 0.7853982f, kWorldLayerMask, moved) && moved.grounded) {
        line += std::to_string(static_cast<unsigned>(moved.groundEntity));
    }
    std::vector<bge::GpuSphereStepMover<float3>> crowd(2);
    crowd[1].position = float3{1.0f, 1.0f, 0.0f};
    crowd[1].displacement = walk;
    crowd[1].stepHeight = 0.35f;
    std::vector<bge::GpuSphereStepResult<float3>> results;
    if (physics.StepMoveSpheres(crowd, results)) line += results[1].outOfSlides ? 'o' : (results[1].hitTrigger ? 't' : 'b');
    return line + std::to_string(results.size()) + std::to_string(walked.stepRise + walked.remaining.x + walked.hitNormal.y + walked.groundNormal.y + walked.groundDistance);
}
