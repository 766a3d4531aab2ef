// tests/cpp/debug_reference_shapes.cpp — compile-only: the four debug-overlay members of PhysicsSystem
// (src/physics/PhysicsSystem.h:77-82) on GpuPhysicsSystem with the reference's signatures, on types shaped like the reference's
// (reference_shapes_mock.hpp), through the calls Application makes (src/core/Application.cpp:173, 359-360), and bge::DebugLine
// against a local copy of the reference's 28-byte PhysicsDebugLine (src/physics/PhysicsDebugDraw.h).
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <vector>

#include "reference_shapes_mock.hpp"

#include "../../banggameengine_amd/host/bge/gpu_systems.hpp"

struct PhysicsDebugLine {
    float from[3];
    float to[3];
    uint32_t abgr = 0xff000000u;
};
static_assert(sizeof(PhysicsDebugLine) == 28 && sizeof(bge::DebugLine) == 28);
static_assert(offsetof(bge::DebugLine, from) == offsetof(PhysicsDebugLine, from) && offsetof(bge::DebugLine, to) == offsetof(PhysicsDebugLine, to) &&
              offsetof(bge::DebugLine, abgr) == offsetof(PhysicsDebugLine, abgr));
static_assert(std::is_same_v<decltype(bge::DebugLine::from), float[3]> && std::is_same_v<decltype(bge::DebugLine::to), float[3]> &&
              std::is_same_v<decltype(bge::DebugLine::abgr), uint32_t>);

using System = bge::GpuPhysicsSystem<Scene>;
// the reference's signatures: void ToggleDebugOverlay(); void SetDebugOverlayEnabled(bool); bool IsDebugOverlayEnabled() const;
// const PhysicsDebugLineBuffer& GetDebugLines() const
static_assert(std::is_same_v<decltype(&System::ToggleDebugOverlay), void (System::*)()>);
static_assert(std::is_same_v<decltype(&System::SetDebugOverlayEnabled), void (System::*)(bool)>);
static_assert(std::is_same_v<decltype(&System::IsDebugOverlayEnabled), bool (System::*)() const>);
static_assert(std::is_same_v<decltype(&System::GetDebugLines), const std::vector<bge::DebugLine>& (System::*)() const>);

// what a renderer does with the buffer (src/render/Renderer.cpp DrawDebugLines): reads from / to / abgr of every line
float DrawDebugLines(const std::vector<bge::DebugLine>& lines)
{
    float sum = 0.0f;
    for (const bge::DebugLine& line : lines) sum += line.from[0] + line.to[2] + static_cast<float>(line.abgr & 0xffu);
    return sum;
}

float Frame(System& physics, Scene& scene, const Camera& camera, const InputSystem& input, double dt, bool keyPressed)
{
    if (keyPressed) physics.ToggleDebugOverlay();  // Application.cpp:173
    physics.Update(scene, camera, input, dt);
    const System& view = physics;
    const bge::DebugLineBuffer& debugLines = view.GetDebugLines();  // Application.cpp:359
    physics.SetDebugRegion(float3{-10.0f, 0.0f, -10.0f}, float3{10.0f, 5.0f, 10.0f});
    physics.ClearDebugRegion();
    physics.SetDebugOverlayEnabled(view.IsDebugOverlayEnabled());
    return DrawDebugLines(debugLines);
}
