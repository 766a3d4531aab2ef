// tests/cpp/batches_reference_shapes.cpp — compile-only: the draw-batch members of GpuSceneMirror (SetDrawKey, ClearDrawKey,
// FetchDrawBatches) on types shaped like the reference's (reference_shapes_mock.hpp), through the loop a renderer would run
// instead of src/render/Renderer.cpp:606-700: one range of the returned ids per draw key instead of every MeshRenderer.
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <vector>

#include "reference_shapes_mock.hpp"

#include "../../banggameengine_amd/host/bge/gpu_systems.hpp"

using Mirror = bge::GpuSceneMirror<Scene>;
static_assert(std::is_same_v<Mirror::Id, EntityId>);
static_assert(std::is_same_v<decltype(&Mirror::SetDrawKey), void (Mirror::*)(EntityId, uint32_t)>);
static_assert(std::is_same_v<decltype(&Mirror::ClearDrawKey), void (Mirror::*)(EntityId)>);
static_assert(std::is_same_v<decltype(&Mirror::FetchDrawBatches),
                             bool (Mirror::*)(Scene&, const float (*)[4], size_t, uint32_t, std::vector<bge_draw_batch>&, std::vector<EntityId>&)>);

// one "draw" per key: the matrices of its instances are in their Transform::world
float SubmitBatches(Scene& scene, const float viewProj[16], bool homogeneousDepth, EntityId mesh, uint32_t key, uint32_t n_keys)
{
    Mirror& mirror = bge::GpuMirrors<Scene>::Of(scene);
    mirror.resident = true;
    mirror.SetDrawKey(mesh, key);
    bge::GpuTransformSystem<Scene>::Update(scene);
    float planes[6][4];
    Mirror::FrustumPlanes(viewProj, homogeneousDepth, planes);
    std::vector<bge_draw_batch> batches;
    std::vector<EntityId> instances;
    float sum = 0.0f;
    if (!mirror.FetchDrawBatches(scene, planes, 6, n_keys, batches, instances)) return sum;
    for (uint32_t k = 0; k < n_keys; ++k) {
        for (uint32_t i = 0; i < batches[k].instance_count; ++i) {
            const Transform* transform = static_cast<const Scene&>(scene).GetTransform(instances[batches[k].first_instance + i]);
            if (transform) sum += transform->world[12] * static_cast<float>(k + 1);
        }
    }
    mirror.ClearDrawKey(mesh);
    return sum;
}
