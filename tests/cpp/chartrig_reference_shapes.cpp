// tests/cpp/chartrig_reference_shapes.cpp — compile-only: GpuPhysicsSystem's character trigger events (an extension:
// include/bge_world.h "Character trigger events") on types with the reference's member signatures (reference_shapes_mock.hpp): a
// frame that switches them on, runs the characters and reads the list the way a game would fire a checkpoint from it.
#include <string>

#include "reference_shapes_mock.hpp"

#include "../../banggameengine_amd/host/bge/gpu_systems.hpp"

std::string CharacterTriggerFrame(bge::GpuPhysicsSystem<Scene>& physics, Scene& scene, const Camera& camera, const InputSystem& input, EntityId player,
                                  double dt)
{
    physics.Update(scene, camera, input, dt);
    physics.SetCharacterTriggerEvents(true);
    std::string line;
    if (physics.AddCharacter(player)) line += 'a';
    if (physics.UpdateCharacters(static_cast<float>(physics.GetFixedStep()), static_cast<uint32_t>(physics.LastSubSteps()))) line += 'u';
    if (physics.SyncCharacters(scene)) line += 's';
    for (const bge::GpuTriggerEvent& e : physics.CharacterTriggerEvents()) {
        line += e.type == bge::GpuTriggerEvent::Type::Enter ? 'E' : (e.type == bge::GpuTriggerEvent::Type::Stay ? 'S' : 'X');
        line += std::to_string(e.trigger) + (e.other == player ? "p" : "o");
    }
    line += std::to_string(physics.TriggerEvents(scene).size());
    physics.SetCharacterTriggerEvents(false);
    physics.RemoveCharacters();
    return line;
}
