// tests/cpp/visible_reference_shapes.cpp — compile-only: the frustum-culling members of GpuSceneMirror (SetBounds, ClearBounds,
// FetchVisible, FrustumPlanes) on types shaped like the reference's (reference_shapes_mock.hpp), through the loop a renderer would
// run instead of src/render/Renderer.cpp:606-631: the ids FetchVisible returns instead of every MeshRenderer.
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <vector>

#include "reference_shapes_mock.hpp"

#include "../../banggameengine_amd/host/bge/gpu_systems.hpp"

using Mirror = bge::GpuSceneMirror<Scene>;
static_assert(std::is_same_v<Mirror::Id, EntityId>);
static_assert(std::is_same_v<decltype(&Mirror::SetBounds), void (Mirror::*)(EntityId, const float*, const float*)>);
static_assert(std::is_same_v<decltype(&Mirror::ClearBounds), void (Mirror::*)(EntityId)>);
static_assert(std::is_same_v<decltype(&Mirror::FetchVisible), bool (Mirror::*)(Scene&, const float (*)[4], size_t, std::vector<EntityId>&)>);
static_assert(std::is_same_v<decltype(&Mirror::FrustumPlanes), void (*)(const float*, bool, float (*)[4])>);

// BeginFrame's loop with the visible set: world matrices of the listed entities are in their Transform::world
float SubmitVisible(Scene& scene, const float viewProj[16], bool homogeneousDepth, EntityId mesh, const float aabbMin[3], const float aabbMax[3])
{
    Mirror& mirror = bge::GpuMirrors<Scene>::Of(scene);
    mirror.resident = true;
    mirror.SetBounds(mesh, aabbMin, aabbMax);
    bge::GpuTransformSystem<Scene>::Update(scene);
    float planes[6][4];
    Mirror::FrustumPlanes(viewProj, homogeneousDepth, planes);
    std::vector<EntityId> visible;
    float sum = 0.0f;
    if (!mirror.FetchVisible(scene, planes, 6, visible)) return sum;
    for (EntityId id : visible) {
        const Transform* transform = static_cast<const Scene&>(scene).GetTransform(id);
        if (!transform || transform->dirty) continue;
        sum += transform->world[12];
    }
    mirror.ClearBounds(mesh);
    return sum;
}
