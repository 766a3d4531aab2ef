// tests/cpp/character_reference_shapes.cpp — compile-only: GpuPhysicsSystem's character members (extensions in the place of the
// reference's btKinematicCharacterController) on types with the reference's member signatures (reference_shapes_mock.hpp): a frame
// as Application::Update would run it — the physics Update, the input turned into a walk and a jump, the characters' sub-steps,
// the write-back into the Transforms.
#include <string>

#include "reference_shapes_mock.hpp"

#include "../../banggameengine_amd/host/bge/gpu_systems.hpp"

std::string CharacterFrame(bge::GpuPhysicsSystem<Scene>& physics, Scene& scene, const Camera& camera, const InputSystem& input, EntityId player,
                           float yaw, float moveForward, float moveRight, bool sprint, bool jumpPressed, double dt)
{
    physics.Update(scene, camera, input, dt);
    std::string line;
    if (physics.AddCharacter(player)) line += 'a';
    float dx = 0.0f, dz = 0.0f;
    bge::GpuPhysicsSystem<Scene>::CharacterWalkFromInput(yaw, moveForward, moveRight, sprint, physics.GetConfig().walkSpeed, dt, dx, dz);
    if (physics.SetCharacterWalk(player, dx, dz)) line += 'w';
    if (jumpPressed && physics.CharacterJump(player)) line += 'j';
    if (physics.UpdateCharacters(static_cast<float>(physics.GetFixedStep()), static_cast<uint32_t>(physics.LastSubSteps()))) line += 'u';
    if (physics.SyncCharacters(scene)) line += 's';
    if (physics.CharacterOnGround(player)) line += 'g';
    bge::GpuCharacterState<float3> state;
    if (physics.GetCharacterState(player, state)) {
        line += state.jumped ? 'J' : (state.landed ? 'L' : (state.stepped ? 'S' : (state.headBump ? 'H' : '-')));
        line += std::to_string(state.groundEntity) + std::to_string(state.hitEntity) + std::to_string(state.steps);
        line += std::to_string(state.position.y + state.verticalVelocity + state.groundNormal.y + state.hitNormal.y + state.stepRise + state.recoveredBy.x);
        line += (state.valid && !state.stuck && !state.recovered && !state.outOfSlides && !state.groundTrigger && !state.hitTrigger) ? 'v' : 'x';
    }
    if (physics.WarpCharacter(player, float3{0.0f, 2.0f, 0.0f})) line += 'p';
    physics.RemoveCharacters();
    physics.LogStats();
    return line;
}
