// tests/cpp/impulse_oracle.cpp — the fixture program of the impulse tests (include/bge_world.h "Impulses").  The oracle's C interface has
// no activate(); its RefPhysicsSystem exposes its body runtimes, so this program builds small scenes with the oracle's own headers,
// runs them, applies the rule of the header directly to a RefBodyRuntime at stated ticks (velocity edit, activation = ACTIVE_TAG,
// deactivationTime = 0), steps on and prints, per tick and body, the bits of origin, orientation, both velocities, the activation
// state and the timer.  Its output is committed as tests/golden/impulses_<scene>.json; tests/test_impulses_cpu.py rebuilds it and
// requires the same bytes, tests/test_gpu_impulses.py runs the same scenes on the device against the fixtures.
//
//     impulse_oracle <scene>        scene: a b c d e f
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../oracle/bullet_math.h"
#include "../../oracle/contact_ref.h"
#include "../../oracle/ecs_ref.h"
#include "../../oracle/physics_ref.h"

using namespace orc;

namespace {

constexpr uint32_t kAtPoint = 0, kCentral = 1, kTorque = 2, kWorldPoint = 4;
const float kDt = 1.0f / 60.0f;

struct BodyDesc {
    int type; // 0 Static, 1 Dynamic
    float size[3], pos[3], mass;
};
struct Kick {
    int tick; // applied BEFORE tick `tick` (counted from the first tick after the warm-up), 0-based
    uint32_t entity, flags;
    float impulse[3], point[3];
};
struct SceneDesc {
    const char* name;
    bool plane, staticContacts, dynamicContacts, basis;
    float gravityY;
    std::vector<BodyDesc> bodies;
    bool sleepFirst; // warm up until every Dynamic body is ISLAND_SLEEPING (otherwise 5 ticks)
    std::vector<Kick> kicks;
    int ticks;
};

uint32_t Bits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// "Apply" and "Wake" of the header on one runtime
void ApplyImpulse(RefBodyRuntime& rt, const Kick& k)
{
    const uint32_t kind = k.flags & 3u;
    const bt::Vec3 imp{k.impulse[0], k.impulse[1], k.impulse[2]};
    if (kind != kTorque) {
        rt.linvel.x = rt.linvel.x + imp.x * rt.invMass;
        rt.linvel.y = rt.linvel.y + imp.y * rt.invMass;
        rt.linvel.z = rt.linvel.z + imp.z * rt.invMass;
    }
    if (kind != kCentral) {
        const bt::Mat3 invI = ct::InvInertiaWorld(bt::MatFromQuat(rt.orn), rt.invInertiaLocal);
        bt::Vec3 t = imp;
        if (kind == kAtPoint) {
            bt::Vec3 r{k.point[0], k.point[1], k.point[2]};
            if (k.flags & kWorldPoint) r = ct::Sub(r, rt.origin);
            t = ct::Cross(r, imp);
        }
        rt.angvel = ct::Add(rt.angvel, ct::MatVec(invI, t));
    }
    rt.activation = kActiveTag;
    rt.deactivationTime = 0.0f;
}

void Step(RefScene& scene, RefPhysicsSystem& physics)
{
    physics.Update(scene, static_cast<double>(kDt));
    RefTransformSystemUpdate(scene);
}

void PrintBodies(RefPhysicsSystem& physics, size_t n, bool last)
{
    std::printf("  [");
    for (size_t i = 0; i < n; ++i) {
        const RefBodyRuntime& rt = physics.Runtimes()[static_cast<EntityId>(i + 1)];
        const float f[13] = {rt.origin.x, rt.origin.y, rt.origin.z, rt.orn.x,    rt.orn.y,    rt.orn.z,   rt.orn.w,
                             rt.linvel.x, rt.linvel.y, rt.linvel.z, rt.angvel.x, rt.angvel.y, rt.angvel.z};
        std::printf("\"");
        for (float v : f) std::printf("%08x", Bits(v));
        std::printf("%08x%08x\"%s", static_cast<uint32_t>(rt.activation), Bits(rt.deactivationTime), i + 1 < n ? ", " : "");
    }
    std::printf("]%s\n", last ? "" : ",");
}

int Run(const SceneDesc& s)
{
    RefScene scene;
    RefPhysicsSystem physics;
    physics.gravityY = s.gravityY;
    physics.orientMode = s.basis ? kOrientBasis : kOrientIdeal;
    physics.groundPlane = s.plane;
    physics.SetStaticContacts(s.staticContacts);
    physics.dynamicContacts = s.dynamicContacts;
    for (const BodyDesc& b : s.bodies) {
        const EntityId id = scene.CreateEntity();
        RefTransform* t = scene.AddTransform(id);
        t->position = Float3{b.pos[0], b.pos[1], b.pos[2]};
        RefCollider* c = scene.AddCollider(id);
        c->size = Float3{b.size[0], b.size[1], b.size[2]};
        RefRigidBody* rb = scene.AddRigidBody(id);
        rb->type = b.type ? RefBodyType::Dynamic : RefBodyType::Static;
        rb->mass = b.mass;
    }
    const size_t n = s.bodies.size();
    int warmup = 0;
    if (s.sleepFirst) {
        for (bool asleep = false; !asleep && warmup < 2000;) {
            Step(scene, physics);
            ++warmup;
            asleep = true;
            for (size_t i = 0; i < n; ++i) {
                if (s.bodies[i].type == 1 && physics.Runtimes()[static_cast<EntityId>(i + 1)].activation != kIslandSleeping) asleep = false;
            }
        }
        if (warmup >= 2000) {
            std::fprintf(stderr, "scene %s never fell asleep\n", s.name);
            return 2;
        }
    } else {
        for (; warmup < 5; ++warmup) Step(scene, physics);
    }
    std::printf("{\n \"scene\": \"%s\",\n \"dt\": \"%08x\",\n \"gravity_y\": \"%08x\",\n", s.name, Bits(kDt), Bits(s.gravityY));
    std::printf(" \"plane\": %d, \"static_contacts\": %d, \"dynamic_contacts\": %d, \"bullet_basis\": %d,\n", s.plane, s.staticContacts, s.dynamicContacts,
                s.basis);
    std::printf(" \"warmup_ticks\": %d,\n \"bodies\": [\n", warmup);
    for (size_t i = 0; i < n; ++i) {
        const BodyDesc& b = s.bodies[i];
        std::printf("  {\"type\": %d, \"size\": [\"%08x\", \"%08x\", \"%08x\"], \"position\": [\"%08x\", \"%08x\", \"%08x\"], \"mass\": \"%08x\"}%s\n", b.type,
                    Bits(b.size[0]), Bits(b.size[1]), Bits(b.size[2]), Bits(b.pos[0]), Bits(b.pos[1]), Bits(b.pos[2]), Bits(b.mass), i + 1 < n ? "," : "");
    }
    std::printf(" ],\n \"kicks\": [\n");
    for (size_t k = 0; k < s.kicks.size(); ++k) {
        const Kick& kk = s.kicks[k];
        std::printf("  {\"before_tick\": %d, \"entity\": %u, \"flags\": %u, \"impulse\": [\"%08x\", \"%08x\", \"%08x\"], \"point\": [\"%08x\", \"%08x\", \"%08x\"]}%s\n",
                    kk.tick, kk.entity, kk.flags, Bits(kk.impulse[0]), Bits(kk.impulse[1]), Bits(kk.impulse[2]), Bits(kk.point[0]), Bits(kk.point[1]),
                    Bits(kk.point[2]), k + 1 < s.kicks.size() ? "," : "");
    }
    // per body: origin 3, orientation 4, linear velocity 3, angular velocity 3, activation state, timer: 15 words of 8 hex digits
    std::printf(" ],\n \"after_warmup\":\n");
    PrintBodies(physics, n, false);
    std::printf(" \"ticks\": [\n");
    int asleepAgain = -1;
    for (int tick = 0; tick < s.ticks; ++tick) {
        for (const Kick& kk : s.kicks) {
            if (kk.tick == tick) ApplyImpulse(physics.Runtimes()[static_cast<EntityId>(kk.entity + 1)], kk);
        }
        Step(scene, physics);
        PrintBodies(physics, n, tick + 1 == s.ticks);
        if (asleepAgain < 0 && physics.Runtimes()[1].activation == kIslandSleeping) asleepAgain = tick + 1;
    }
    // how many ticks after the first kick body 0 is ISLAND_SLEEPING (again); -1: not within the run
    std::printf(" ],\n \"body0_asleep_after_ticks\": %d\n}\n", asleepAgain);
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    const BodyDesc crate{1, {0.5f, 0.5f, 0.5f}, {0.0f, 0.5f, 0.0f}, 1.0f};
    const Kick central{0, 0, kCentral, {1.5f, 0.0f, 0.5f}, {0.0f, 0.0f, 0.0f}};
    const Kick corner{0, 0, kAtPoint, {0.0f, 1.0f, 0.25f}, {0.5f, 0.5f, 0.5f}};
    const Kick cornerLater{15, 0, kAtPoint, {0.0f, 1.0f, 0.25f}, {0.5f, 0.5f, 0.5f}};
    std::vector<SceneDesc> scenes;
    // (a) a 1 kg box resting awake on the plane, kicked centrally, and later at a corner
    scenes.push_back({"a", true, false, false, false, -9.81f, {crate}, false, {central, cornerLater}, 40});
    // (b) the same box left until ISLAND_SLEEPING, then kicked at a corner
    scenes.push_back({"b", true, false, false, false, -9.81f, {crate}, true, {corner}, 40});
    // (c) a box on a Static box with static contacts on (no plane), asleep, kicked
    scenes.push_back({"c", false, true, false, false, -9.81f, {{1, {0.5f, 0.5f, 0.5f}, {0.0f, 1.5f, 0.0f}, 1.0f}, {0, {2.0f, 0.5f, 2.0f}, {0.0f, 0.5f, 0.0f}, 0.0f}},
                      true, {{0, 0, kCentral, {1.0f, 0.0f, 0.0f}, {0, 0, 0}}}, 40});
    // (d) Dynamic contacts on: a stack of three boxes on the plane, asleep; the top box (entity 2) is kicked
    scenes.push_back({"d", true, false, true, false, -9.81f,
                      {{1, {0.5f, 0.5f, 0.5f}, {0.0f, 0.5f, 0.0f}, 1.0f}, {1, {0.5f, 0.5f, 0.5f}, {0.0f, 1.5f, 0.0f}, 1.0f}, {1, {0.5f, 0.5f, 0.5f}, {0.0f, 2.5f, 0.0f}, 1.0f}},
                      true, {{0, 2, kCentral, {0.5f, 0.0f, 0.0f}, {0, 0, 0}}}, 40});
    // (e) scene (a) under the Bullet-basis orientation scheme
    scenes.push_back({"e", true, false, false, true, -9.81f, {crate}, false, {central, cornerLater}, 40});
    // (f) a free sleeper, no gravity: kicked to 0.25 m/s, slower than the sleeping threshold, it moves and sleeps again
    scenes.push_back({"f", false, false, false, false, 0.0f, {{1, {0.5f, 0.5f, 0.5f}, {1.0f, 2.0f, 3.0f}, 2.0f}}, true, {{0, 0, kCentral, {0.5f, 0.0f, 0.0f}, {0, 0, 0}}}, 130});
    if (argc != 2) {
        std::fprintf(stderr, "usage: impulse_oracle <scene>\n");
        return 1;
    }
    for (const SceneDesc& s : scenes) {
        if (std::string(argv[1]) == s.name) return Run(s);
    }
    std::fprintf(stderr, "unknown scene %s\n", argv[1]);
    return 1;
}
