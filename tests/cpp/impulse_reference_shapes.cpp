// tests/cpp/impulse_reference_shapes.cpp — compile-only: GpuPhysicsSystem's impulse and push members (extensions: include/bge_world.h
// "Impulses", "Character push") on types with the reference's member signatures (reference_shapes_mock.hpp): a frame that kicks a
// crate, spins it, wakes another, switches the characters' push on and runs the step that applies the queue.
#include <string>

#include "reference_shapes_mock.hpp"

#include "../../banggameengine_amd/host/bge/gpu_systems.hpp"

std::string ImpulseFrame(bge::GpuPhysicsSystem<Scene>& physics, Scene& scene, const Camera& camera, const InputSystem& input, EntityId crate,
                         EntityId sleeper, EntityId player, double dt)
{
    std::string line;
    physics.Update(scene, camera, input, dt);
    float3 kick{}, corner{};
    kick.x = 2.0f;
    corner.y = 0.5f;
    if (physics.ApplyImpulse(crate, kick, corner)) line += 'i';
    if (physics.ApplyCentralImpulse(crate, kick)) line += 'c';
    if (physics.ApplyTorqueImpulse(crate, corner)) line += 't';
    if (physics.ActivateBody(sleeper)) line += 'a';
    physics.SetCharacterPush(true, 250.0f);
    physics.SetCharacterPush(true, 250.0f, 0.7f);
    physics.Update(scene, camera, input, dt); // (the queue is applied at its head, in call order)
    if (physics.AddCharacter(player)) line += 'p';
    if (physics.UpdateCharacters(static_cast<float>(physics.GetFixedStep()), static_cast<uint32_t>(physics.LastSubSteps()))) line += 'u';
    if (physics.SyncCharacters(scene)) line += 's';
    physics.SetCharacterPush(false);
    physics.RemoveCharacters();
    return line;
}
