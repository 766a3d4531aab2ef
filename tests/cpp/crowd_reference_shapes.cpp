// tests/cpp/crowd_reference_shapes.cpp — compile-only: GpuPhysicsSystem's crowd members (extensions: include/bge_world.h "Crowd
// separation") on types with the reference's member signatures (reference_shapes_mock.hpp): a frame that switches the crowd on,
// runs the characters' sub-steps and reads what Separate found around the player.
#include <string>

#include "reference_shapes_mock.hpp"

#include "../../banggameengine_amd/host/bge/gpu_systems.hpp"

std::string CrowdFrame(bge::GpuPhysicsSystem<Scene>& physics, Scene& scene, const Camera& camera, const InputSystem& input, EntityId player,
                       EntityId other, double dt)
{
    physics.SetCharacterCrowd(true);
    physics.SetCharacterCrowd(true, 0.05f);
    physics.Update(scene, camera, input, dt);
    std::string line;
    if (physics.AddCharacter(player) && physics.AddCharacter(other)) line += 'a';
    if (physics.UpdateCharacters(static_cast<float>(physics.GetFixedStep()), static_cast<uint32_t>(physics.LastSubSteps()))) line += 'u';
    if (physics.SyncCharacters(scene)) line += 's';
    bge::GpuCharacterCrowd<float3> crowd;
    if (physics.GetCharacterCrowd(player, crowd)) {
        line += crowd.pushed ? 'P' : '-';
        line += crowd.clamped ? 'C' : '-';
        line += std::to_string(crowd.overlaps) + std::to_string(crowd.depth + crowd.push.x + crowd.push.y + crowd.push.z);
        if (crowd.other == other) line += 'o';
    }
    physics.SetCharacterCrowd(false);
    physics.RemoveCharacters();
    return line;
}
