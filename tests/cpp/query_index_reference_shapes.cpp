// tests/cpp/query_index_reference_shapes.cpp — compile-only: GpuPhysicsSystem's query-index members (extensions:
// include/bge_world.h "Query index") on types with the reference's member signatures (reference_shapes_mock.hpp): a frame that
// switches the index on, runs the characters' sub-steps through it and reads what the last call did with it.
#include <string>

#include "reference_shapes_mock.hpp"

#include "../../banggameengine_amd/host/bge/gpu_systems.hpp"

std::string QueryIndexFrame(bge::GpuPhysicsSystem<Scene>& physics, Scene& scene, const Camera& camera, const InputSystem& input, EntityId player,
                            double dt)
{
    physics.SetQueryIndex(true);
    physics.SetQueryIndex(true, 4.0f);
    physics.Update(scene, camera, input, dt);
    std::string line;
    if (physics.AddCharacter(player)) line += 'a';
    if (physics.UpdateCharacters(static_cast<float>(physics.GetFixedStep()), static_cast<uint32_t>(physics.LastSubSteps()))) line += 'u';
    bge_query_index_stats stats{};
    if (physics.GetQueryIndexStats(stats)) line += std::to_string(stats.built) + std::to_string(stats.bodies_indexed + stats.bodies_wide) + std::to_string(stats.builds);
    physics.SetQueryIndex(false);
    physics.RemoveCharacters();
    return line;
}
