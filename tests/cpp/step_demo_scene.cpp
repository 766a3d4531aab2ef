// tests/cpp/step_demo_scene.cpp — GpuPhysicsSystem::StepMoveSphere on the entities of tests/golden/demo_scene.json: a sphere walks
// on the ground plane into the side of the Static box "Ground" and gets onto it only with a step height above the box's top.
//
// Ground is the box of half extents (50, 1, 50) at y = -0.01: its top is y = 0.99 and its side x = 50.  The sphere has radius 0.5 and
// skin 0.01, stands on the plane at (52, 0.51, 0) and asks (-3, 0, 0) with a probe of 0.1.  The plain move meets the side head-on
// where the centre is at x = 50.5 and rests at 50.51.  With step_height 0.3 the raised sphere (centre 0.81, below the top) meets
// the same side at the same fraction and comes down on the plane where the plain move ended: nothing gained, the plain result
// stands.  With step_height 1.2 its underside (1.21) clears the top: it runs its whole way to x = 49, comes down 0.22 - skin onto
// the top and rests at y = 0.99 + radius + skin = 1.5, STEPPED and GROUNDED on Ground.
// Exit 0 = all checks passed, 77 = no usable GPU, anything else = a failed check (printed).
#include <cmath>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

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

// the file keeps position / rotationEuler / scale on the entity itself, and a box collider with a Static body on Ground
static bool build(const std::string& text, bge::Scene& scene, bge::EntityId& ground)
{
    bge::json::Value root;
    bge::json::Parser parser(text);
    std::string err;
    if (!parser.parse(root, &err)) return false;
    const bge::json::Value* entities = root.find("entities");
    if (!entities) return false;
    for (const bge::json::Value& e : entities->arr) {
        const auto id = scene.CreateEntity();
        auto* t = scene.AddTransform(id);
        bge::detail::read_vec3(e, "position", t->position);
        bge::detail::read_vec3(e, "rotationEuler", t->rotationEuler);
        bge::detail::read_vec3(e, "scale", t->scale);
        t->MarkDirty();
        const bge::json::Value* cj = e.find("collider");
        const bge::json::Value* rj = e.find("rigidBody");
        if (!cj || !rj) continue;
        auto* c = scene.AddCollider(id);
        c->shape = bge::ColliderShape::Box;
        bge::detail::read_vec3(*cj, "size", c->size);
        auto* b = scene.AddRigidBody(id);
        b->type = bge::RigidBodyType::Static;
        b->layer = static_cast<uint32_t>(bge::detail::read_float(*rj, "layer", 1.0f));
        ground = id;
    }
    return true;
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
    bge::EntityId ground = bge::kInvalidEntity;
    if (!build(ss.str(), scene, ground)) return 3;
    expect(ground != bge::kInvalidEntity, "Ground found");

    bge::GpuPhysicsSystem<bge::Scene> physics;
    using Result = bge::GpuSphereStepResult<bge::float3>;
    const float radius = 0.5f, skin = 0.01f, probe = 0.1f, slope = 0.7853982f;
    const bge::float3 at{52.0f, radius + skin, 0.0f}, walk{-3.0f, 0.0f, 0.0f};
    Result res;
    expect(!physics.StepMoveSphere(at, walk, radius, skin, probe, slope, 3u, 1.2f, res) && res.position.x == at.x && res.position.y == at.y,
           "no world before the first Update: the position is echoed");
    for (int i = 0; i < 3; ++i) {
        physics.Update(scene, 1.0 / 120.0);
        bge::GpuTransformSystem<bge::Scene>::Update(scene);
    }
    bge::GpuSphereMoveResult<bge::float3> plain;
    expect(physics.MoveSphere(at, walk, radius, skin, probe, slope, 3u, plain) && plain.hits == 1 && plain.hitEntity == ground &&
               near(plain.position.x, 50.0f + radius + skin, 1e-4f) && plain.grounded && plain.groundEntity == bge::kInvalidEntity,
           "MoveSphere stops at Ground's side, standing on the plane");
    Result none, low, high;
    expect(physics.StepMoveSphere(at, walk, radius, skin, probe, slope, 3u, 0.0f, none) && !none.stepTried && !none.stepped &&
               none.position.x == plain.position.x && none.position.y == plain.position.y && none.hits == plain.hits && none.grounded,
           "step height 0: the plain move");
    expect(physics.StepMoveSphere(at, walk, radius, skin, probe, slope, 3u, 0.3f, low) && low.stepTried && !low.stepped && low.stepRise == 0.0f &&
               low.position.x == plain.position.x && low.position.y == plain.position.y && low.position.z == plain.position.z &&
               low.hits == plain.hits && low.hitEntity == ground && low.grounded && low.groundEntity == bge::kInvalidEntity,
           "step height 0.3 is too small: tried, and it stays where MoveSphere leaves it");
    expect(physics.StepMoveSphere(at, walk, radius, skin, probe, slope, 3u, 1.2f, high) && high.stepTried && high.stepped, "step height 1.2: stepped");
    std::printf("stepped to (%.4f, %.4f, %.4f), rise %.4f\n", high.position.x, high.position.y, high.position.z, high.stepRise);
    expect(near(high.position.x, 49.0f, 1e-4f) && near(high.position.y, 0.99f + radius + skin, 1e-4f) && high.position.z == 0.0f,
           "ends on Ground's top at y = 0.99 + radius + skin, its whole way along");
    expect(high.grounded && high.groundEntity == ground && !high.groundTrigger && near(high.groundDistance, skin, 1e-4f) && high.groundNormal.y == 1.0f,
           "GROUNDED on Ground at distance skin, normal +y");
    expect(near(high.stepRise, 1.2f, 1e-6f) && high.hits == 0 && !high.outOfSlides && high.remaining.x == 0.0f, "rose by the step height and met nothing up there");
    // the batched form gives the same as one call each
    std::vector<bge::GpuSphereStepMover<bge::float3>> movers(3);
    std::vector<Result> many;
    for (int i = 0; i < 3; ++i) {
        movers[i].position = bge::float3{52.0f, radius + skin, 10.0f * static_cast<float>(i)};
        movers[i].displacement = walk;
        movers[i].probeDistance = probe;
        movers[i].layerMask = 3u;
        movers[i].stepHeight = i == 0 ? 0.3f : 1.2f;
    }
    movers[2].stepHeight = -1.0f; // invalid
    bool same = physics.StepMoveSpheres(movers, many) && many.size() == 3 && !many[2].valid && many[2].position.x == 52.0f && !many[2].stepped;
    for (int i = 0; i < 2 && same; ++i) {
        Result one;
        same &= physics.StepMoveSphere(movers[i].position, walk, radius, skin, probe, slope, 3u, movers[i].stepHeight, one);
        same &= one.position.x == many[i].position.x && one.position.y == many[i].position.y && one.grounded == many[i].grounded &&
                one.stepped == many[i].stepped && one.stepped == (i == 1);
    }
    expect(same, "StepMoveSpheres equals StepMoveSphere per mover; an invalid mover is reported and echoed");
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
