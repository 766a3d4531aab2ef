// tests/cpp/debug_demo_scene.cpp — the physics debug overlay (src/core/Application.cpp:173, 359-360) through the C++ adapter on the
// demo scene in the reference's format: empty while off; after ToggleDebugOverlay() and one Update the plane, Ground's box and the
// Checkpoint volume, in the order and colours include/bge_world.h states; empty again after toggling off.
// Exit 0 = all checks passed, 77 = no usable GPU, anything else = a failed check (printed).
#include <cmath>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../banggameengine_amd/host/bge/gpu_systems.hpp"
#include "../../banggameengine_amd/host/bge/scene.hpp"
#include "../../banggameengine_amd/host/bge/scene_json.hpp"

static int failures = 0;
static void expect(bool ok, const char* what)
{
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) ++failures;
}
static bool near(float a, float b, float tol) { return std::fabs(a - b) <= tol; }

// every end point of lines [first, first + 12) is a corner of the box centre +- half, and all 8 corners occur
static bool box_corners(const std::vector<bge::DebugLine>& l, size_t first, const float c[3], const float h[3], uint32_t abgr, float tol)
{
    unsigned seen = 0;
    for (size_t i = first; i < first + 12; ++i) {
        if (l[i].abgr != abgr) return false;
        for (const float* p : {l[i].from, l[i].to}) {
            unsigned code = 0;
            for (int a = 0; a < 3; ++a) {
                if (near(p[a], c[a] + h[a], tol)) code |= 1u << a;
                else if (!near(p[a], c[a] - h[a], tol)) return false;
            }
            seen |= 1u << code;
        }
    }
    return seen == 0xffu;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    {
        bge::GpuSceneMirror<bge::Scene> probe;
        if (!probe.ok()) {
            std::printf("no usable GPU\n");
            return 77;
        }
    }
    std::ifstream f(argv[1]);
    std::stringstream ss;
    ss << f.rdbuf();
    bge::Scene scene;
    std::string err;
    if (!bge::LoadSceneFromJsonText(ss.str(), scene, &err)) {
        std::printf("scene: %s\n", err.c_str());
        return 3;
    }
    bge::GpuPhysicsSystem<bge::Scene> physics;
    expect(!physics.IsDebugOverlayEnabled() && physics.GetDebugLines().empty(), "off and empty before the first Update");
    for (int i = 0; i < 3; ++i) {
        physics.Update(scene, 1.0 / 120.0);
        bge::GpuTransformSystem<bge::Scene>::Update(scene);
    }
    expect(physics.GetDebugLines().empty(), "empty while the overlay is off");
    physics.ToggleDebugOverlay();
    expect(physics.IsDebugOverlayEnabled(), "ToggleDebugOverlay switches it on");
    physics.Update(scene, 1.0 / 120.0);
    bge::GpuTransformSystem<bge::Scene>::Update(scene);
    const std::vector<bge::DebugLine>& lines = physics.GetDebugLines();
    std::printf("%zu lines\n", lines.size());
    expect(lines.size() == 36, "36 lines: the plane, Ground, the Checkpoint volume");
    if (lines.size() == 36) {
        bool grey = true;
        for (size_t i = 0; i < 12; ++i) grey = grey && lines[i].abgr == 0xff7f7f7fu && lines[i].from[1] == 0.0f && lines[i].to[1] == 0.0f;
        expect(grey, "12 grey plane lines in y = 0");
        expect(lines[0].from[0] == -25.0f && lines[0].from[2] == 25.0f && lines[0].to[0] == -25.0f && lines[0].to[2] == -25.0f,
               "the plane's first border line (-25, 0, 25) - (-25, 0, -25)");
        const float gc[3] = {0.0f, -0.01f, 0.0f}, gh[3] = {50.0f, 1.0f, 50.0f};
        expect(box_corners(lines, 12, gc, gh, 0xff7f7f7fu, 1e-4f), "12 grey lines on the corners of Ground's 50 x 1 x 50 box");
        const float cc[3] = {5.0f, 1.0f, 5.0f}, ch[3] = {1.5f, 1.5f, 1.5f};
        expect(box_corners(lines, 24, cc, ch, 0xffff00ffu, 1e-5f), "12 lines of the Checkpoint volume in 0xffff00ff");
    }
    // a region around the Checkpoint: the plane and the volume only
    physics.SetDebugRegion(bge::float3{4.0f, 0.0f, 4.0f}, bge::float3{6.0f, 2.0f, 6.0f});
    physics.Update(scene, 1.0 / 120.0);
    expect(physics.GetDebugLines().size() == 24 && physics.GetDebugLines()[12].abgr == 0xffff00ffu, "region: the plane and the Checkpoint");
    physics.ClearDebugRegion();
    physics.ToggleDebugOverlay();
    expect(!physics.IsDebugOverlayEnabled() && physics.GetDebugLines().empty(), "toggling off empties it again");
    physics.Update(scene, 1.0 / 120.0);
    expect(physics.GetDebugLines().empty(), "and it stays empty over an Update");
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
