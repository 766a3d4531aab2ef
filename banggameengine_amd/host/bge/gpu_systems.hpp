// bge/gpu_systems.hpp — the reference's system call shapes on top of the C ABI (include/bge_world.h).
//
//   reference call site (src/core/Application.cpp)            replacement (same name, same arguments)
//   :256  m_physics.Update(m_scene, *m_camera, m_input, dt)   m_gpuPhysics.Update(m_scene, *m_camera, m_input, dt)   [rigid-body slice]
//   :284  TransformSystem::Update(m_scene)                    bge::GpuTransformSystem<Scene>::Update(m_scene)
//   :283,285  m_scene.CountDirtyTransforms()                  unchanged (host flags are kept coherent)
//   :84   m_physics.ReloadConfigIfNeeded(m_scene)             m_gpuPhysics.ReloadConfigIfNeeded(m_scene)   [gravity, fixedStep]
//   :324-326  OnSceneReloaded / GetFixedStep                  same names
// GpuPhysicsSystem carries PhysicsSystem's public surface for this path (src/physics/PhysicsSystem.h:43-48, 77):
// SetConfigPath, void Initialize(), OnSceneReloaded, bool ReloadConfigIfNeeded, Update(Scene&, const Camera&, const
// InputSystem&, double), LogStats, GetFixedStep — and steps the world as the reference does: Bullet's
// stepSimulation(dt, 4, max(fixedStep, 1/240)) with its sub-step clock (bge_world_step_simulation).
//
// Header-only and templated on the scene type: it needs only the accessors the reference's Scene already has
// (GetTransforms, GetTransform, GetParent, HasTransform, GetRigidBodies, GetCollider — src/ecs/Scene.h:28-95)
// and the field names of Transform / RigidBody / Collider, so it compiles against the reference's own headers
// as well as against bge/scene.hpp.
//
// Coherence model ("coherent mode"): the host structs stay the source of truth at the points the reference's
// callers read them —  Transform::world and Transform::dirty after TransformSystem::Update,
// Transform::position / rotationEuler / dirty after PhysicsSystem::Update.  Per call the adapter
//   1. re-derives the dense entity index <-> EntityId map and the parent array when the set of Transforms or a
//      parent link changed (the reference has no topology version counter, so this is an O(N) scan — the
//      reference's own ForEachRootTransform does the same scan every call, src/ecs/Scene.cpp:523-533);
//   2. uploads the TRS of Transforms whose `dirty` flag is set (sparse, bge_world_upload_trs_indexed);
//   3. ticks the device world;
//   4. copies the results back into the host structs.
// Errors never throw (the reference's hot path has no exceptions): a failed call logs "[GPU] ..." to stderr and
// returns false, leaving the host structs as they were.
//
// Bodies collide with the ground plane only, not with each other (no convex-convex narrowphase on this path).
// Known deviations (documented in DESIGN.md): Transform::local is not refreshed; a Dynamic body whose Transform
// is edited BETWEEN PhysicsSystem::Update and TransformSystem::Update of the same tick continues from the edited
// position (the reference's Bullet body would ignore the edit).
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../../include/bge_world.h"
#include "scene_json.hpp" // the JSON reader (physics.json)

namespace bge {

// Trigger events as PhysicsSystem publishes them on its EventBus (src/physics/PhysicsSystem.h:50-62)
// One object GpuPhysicsSystem::OverlapSphere found (an extension: the reference has no such query)
struct GpuOverlapHit {
    uint32_t entity = 0;   // EntityId of the body or trigger; kInvalidEntity (0) for the ground plane
    bool trigger = false;  // a trigger ghost, not a rigid body
    float distance = 0.0f; // from the sphere's centre to the shape, 0 when the centre is inside it
};

// One sphere of GpuPhysicsSystem::MoveSpheres and what a move returns (extensions: include/bge_world.h "Sphere moves").  Vec3 is
// the engine's float3 (members x, y, z).
template <class Vec3> struct GpuSphereMover {
    Vec3 position{};         // centre before the move
    Vec3 displacement{};     // asked motion of this call (walk direction, gravity and dt folded in by the caller)
    float radius = 0.5f;
    float skin = 0.01f;      // > 0: the gap kept to what was hit
    float probeDistance = 0; // length of the ground probe straight down after the move; 0 = none
    float maxSlopeRad = 0.7853982f; // grounded needs a ground normal within this angle of +y
    uint32_t layerMask = 0xffffffffu;
};
template <class Vec3> struct GpuSphereMoveResult {
    Vec3 position{};       // centre after the move
    Vec3 remaining{};      // displacement left unspent (zero unless outOfSlides)
    bool valid = false;    // false: an input was not finite or out of range, or there is no world; position is echoed
    bool grounded = false; // the probe found ground no steeper than maxSlopeRad
    bool probeHit = false;
    bool outOfSlides = false;
    uint32_t hits = 0;           // rounds that hit something, 0 .. BGE_MOVE_SLIDES
    uint32_t hitEntity = 0;      // EntityId of the last thing hit; kInvalidEntity (0) for the ground plane or none
    bool hitTrigger = false;
    Vec3 hitNormal{};
    uint32_t groundEntity = 0;   // the probe's hit, same convention
    bool groundTrigger = false;
    float groundDistance = 0.0f;
    Vec3 groundNormal{};
};

// One sphere of GpuPhysicsSystem::StepMoveSpheres and what a step move returns (extensions: include/bge_world.h "Sphere step
// moves"): the mover and the result of MoveSpheres with the step height, and with whether a step was tried and taken.
template <class Vec3> struct GpuSphereStepMover : GpuSphereMover<Vec3> {
    float stepHeight = 0.0f; // >= 0: how far the sphere may rise to get over an obstacle; 0 = the plain move
};
template <class Vec3> struct GpuSphereStepResult : GpuSphereMoveResult<Vec3> {
    bool stepTried = false; // the first thing met was no walkable ground, and a step was looked for
    bool stepped = false;   // the step was taken: position is on top of (or behind) the obstacle
    float stepRise = 0.0f;  // how far it rose for it; 0 unless stepped
};

// What GpuPhysicsSystem::SpherePenetration finds, one sphere of RecoverSpheres and what a recovery returns (extensions:
// include/bge_world.h "Sphere penetration and recovery").  Vec3 is the engine's float3 (members x, y, z).
template <class Vec3> struct GpuPenetrationHit {
    uint32_t entity = 0;  // EntityId of the body or trigger; kInvalidEntity (0) for the ground plane
    bool trigger = false; // a trigger ghost, not a rigid body
    float depth = 0.0f;   // how far the shape reaches into the sphere, >= 0
    Vec3 point{};         // on the shape's surface
    Vec3 normal{};        // unit: the way out
};
template <class Vec3> struct GpuSphereRecover {
    Vec3 position{};
    float radius = 0.5f;
    float skin = 0.01f; // > 0: the gap left to what the sphere was pushed out of
    uint32_t layerMask = 0xffffffffu;
};
template <class Vec3> struct GpuSphereRecoverResult {
    Vec3 position{};     // centre after the recovery
    Vec3 pushed{};       // position after - position before
    bool valid = false;  // false: an input was not finite or out of range, or there is no world; position is echoed
    bool moved = false;  // at least one push
    bool stuck = false;  // still penetrating after BGE_RECOVER_ROUNDS pushes, by remainingDepth
    uint32_t pushes = 0; // 0 .. BGE_RECOVER_ROUNDS
    uint32_t hitEntity = 0; // EntityId of what the last push was out of; kInvalidEntity (0) for the ground plane or none
    bool hitTrigger = false;
    Vec3 hitNormal{};
    float hitDepth = 0.0f;
    float remainingDepth = 0.0f;
};

// What a character of GpuPhysicsSystem::AddCharacter is made with and what GetCharacterState returns (extensions:
// include/bge_world.h "Characters").  The state is that of the last SyncCharacters.
struct GpuCharacterKnobs {
    float radius = 0.35f;
    float skin = 0.01f;
    float stepHeight = 0.35f;
    float maxSlopeRad = 0.8726646f; // 50 degrees
    float probeDistance = 0.1f;
    float gravity = 9.81f;    // >= 0, downwards
    float jumpSpeed = 5.0f;
    float fallSpeed = 29.43f; // |gravity| * 3
    uint32_t layerMask = 0xffffffffu;
};
template <class Vec3> struct GpuCharacterState {
    Vec3 position{};
    float verticalVelocity = 0.0f;
    bool valid = false; // the last step was valid
    bool grounded = false, jumped = false, landed = false, headBump = false, recovered = false, stuck = false, stepped = false, outOfSlides = false;
    uint32_t groundEntity = 0; // EntityId of what the character stands on; kInvalidEntity (0) for the ground plane or none
    bool groundTrigger = false;
    Vec3 groundNormal{};
    uint32_t hitEntity = 0; // EntityId of the last thing the last step's slides hit; kInvalidEntity (0) for the plane or none
    bool hitTrigger = false;
    Vec3 hitNormal{};
    float stepRise = 0.0f;
    Vec3 recoveredBy{}; // what the last step's recovery pushed the character by
    uint32_t steps = 0;
};

// What GetCharacterRide returns (extension: include/bge_world.h "Character platform riding"): what the last UpdateCharacters' carry
// did to the character, as of the last SyncCharacters
template <class Vec3> struct GpuCharacterRide {
    bool carried = false;  // the platform moved and the character was moved with it
    bool lost = false;     // the platform left the world (or stopped being rideable) under the character
    uint32_t platform = 0; // EntityId of the body the character stood on when the call ended; kInvalidEntity (0) if none
    Vec3 carriedBy{};      // what the carry added to the position
    float turn[4] = {0.0f, 0.0f, 0.0f, 1.0f}; // xyzw: the platform's rotation since the call before, for the caller's facing
};

// What GetCharacterCrowd returns (extension: include/bge_world.h "Crowd separation"): what the last step of the last
// UpdateCharacters found around the character, as of the last SyncCharacters
template <class Vec3> struct GpuCharacterCrowd {
    bool pushed = false;   // another character overlapped this one and it was pushed away from the deepest
    bool clamped = false;  // the push was cut to maxPush
    uint32_t other = 0;    // EntityId of that character; kInvalidEntity (0) if none
    uint32_t overlaps = 0; // how many characters overlapped this one
    float depth = 0.0f;    // by how much `other` did
    Vec3 push{};           // what the step added to the position (level: y is 0)
};

struct GpuTriggerEvent {
    enum class Type { Enter, Stay, Exit };
    Type type = Type::Enter;
    uint32_t trigger = 0; // EntityId
    uint32_t other = 0;   // EntityId
};

// One line of the physics debug overlay: bge_debug_line has the members and layout of the reference's PhysicsDebugLine
// (src/physics/PhysicsDebugDraw.h: float from[3], to[3]; uint32_t abgr), so the renderer's loop over the buffer compiles unchanged
using DebugLine = ::bge_debug_line;
static_assert(sizeof(DebugLine) == 28, "28-byte line record");
using DebugLineBuffer = std::vector<DebugLine>;

namespace detail {
template <class S, class = void> struct has_trigger_volumes : std::false_type {};
template <class S> struct has_trigger_volumes<S, std::void_t<decltype(std::declval<S&>().GetTriggerVolumes())>> : std::true_type {};
} // namespace detail

template <class SceneT> class GpuSceneMirror {
public:
    using Id = uint32_t;

    explicit GpuSceneMirror(int device = -1, void* stream = nullptr)
    {
        bge_world_desc d{};
        d.struct_size = sizeof d;
        d.device = device;
        d.stream = stream;
        if (bge_world_create(&d, &world_) != BGE_OK) Log("bge_world_create");
        // every world of the reference has the static plane y = 0 (PhysicsSystem::EnsureGround, PhysicsSystem.cpp:149-166)
        else if (bge_world_set_ground_plane(world_, 1) != BGE_OK) Log("bge_world_set_ground_plane");
        // ... and its dispatcher collides Dynamic bodies with the Static / Kinematic ones (PhysicsSystem.cpp:122-128): box against box
        // here (Bullet's btBoxBoxDetector, include/bge_world.h) — what carries a body on demo.json's "Ground"
        else if (bge_world_set_static_contacts(world_, 1) != BGE_OK) Log("bge_world_set_static_contacts");
        // ... and with each other: boxes pile up, touching bodies sleep and wake as one island (include/bge_world.h)
        else if (bge_world_set_dynamic_contacts(world_, 1) != BGE_OK) Log("bge_world_set_dynamic_contacts");
    }
    ~GpuSceneMirror() { bge_world_destroy(world_); }
    GpuSceneMirror(const GpuSceneMirror&) = delete;
    GpuSceneMirror& operator=(const GpuSceneMirror&) = delete;

    bool ok() const { return world_ != nullptr; }
    bge_world* world() { return world_; }
    float gravity[3] = {0.0f, -9.81f, 0.0f}; // PhysicsSystem.cpp:130 with assets/config/physics.json:2
    // BGE_TICK_BULLET_BASIS: carry every Dynamic body's orientation the way Bullet does (basis round trip each step, euler
    // rewritten from it) instead of leaving a non-spinning body's orientation and euler untouched
    bool bullet_basis = false;
    // The ground plane is part of every reference world; SetGroundPlane(false) turns the bodies into free bodies (what
    // BASELINE's synthetic workloads are).  Takes effect on the next UpdatePhysics.
    void SetGroundPlane(bool on)
    {
        if (ok() && bge_world_set_ground_plane(world_, on ? 1 : 0) != BGE_OK) Log("bge_world_set_ground_plane");
        ground_plane_state = on ? 1 : 0;
    }
    // Contacts of Dynamic boxes with Static / Kinematic boxes (on by default, as in every reference world)
    void SetStaticContacts(bool on)
    {
        if (ok() && bge_world_set_static_contacts(world_, on ? 1 : 0) != BGE_OK) Log("bge_world_set_static_contacts");
    }

    // Contacts of Dynamic boxes with each other (on by default, as in every reference world; a scene of free bodies that never meet
    // saves the sub-step's pair search by switching them off)
    void SetDynamicContacts(bool on)
    {
        if (ok() && bge_world_set_dynamic_contacts(world_, on ? 1 : 0) != BGE_OK) Log("bge_world_set_dynamic_contacts");
    }

    // Resident mode: the world matrices stay on the device after TransformSystem::Update; only the host `dirty` flags
    // are kept coherent and the caller fetches the matrices it needs: the visible set (FetchVisible), or any list (FetchWorld).  Coherent
    // mode (default) copies every world matrix back each call, which is what makes the adapter a drop-in but also what
    // bounds it (64 B per entity over PCIe + a hash-map scatter).
    bool resident = false;

    // world matrices of the given entities straight from the device into their Transform::world
    bool FetchWorld(SceneT& scene, const std::vector<Id>& entities)
    {
        index_list_.clear();
        for (Id id : entities) {
            auto it = index_of_.find(id);
            if (it != index_of_.end()) index_list_.push_back(it->second);
        }
        if (!down_.resize(index_list_.size() * 16 + 1)) return Log("bge_host_alloc");
        if (!index_list_.empty() &&
            bge_world_download_world_indexed(world_, index_list_.size(), index_list_.data(), down_.data()) != BGE_OK) {
            return Log("bge_world_download_world_indexed");
        }
        for (size_t k = 0; k < index_list_.size(); ++k) {
            if (auto* t = scene.GetTransform(ids_[index_list_[k]])) std::memcpy(t->world, &down_[16 * k], 64);
        }
        return true;
    }

    // EXTENSION without a reference counterpart (its renderer submits every MeshRenderer, src/render/Renderer.cpp:606-665): the
    // model-space box of an entity's mesh.  An entity with bounds is renderable; FetchVisible lists the renderable entities a view
    // sees (include/bge_world.h "Frustum culling").  Sent lazily with the other dirty data, and again to the new index when a
    // re-topology moves the entity.
    void SetBounds(Id id, const float min[3], const float max[3])
    {
        Bounds b;
        for (int a = 0; a < 3; ++a) {
            b.v[a] = (min[a] + max[a]) * 0.5f;
            b.v[3 + a] = (max[a] - min[a]) * 0.5f;
        }
        bounds_[id] = b;
        bounds_stale_ = true;
    }
    void ClearBounds(Id id)
    {
        if (bounds_.erase(id)) bounds_stale_ = true;
    }
    // The six planes of a view-projection matrix (bx row-vector convention; homogeneousDepth as bgfx::getCaps()->homogeneousDepth)
    static void FrustumPlanes(const float viewProj16[16], bool homogeneousDepth, float planes[6][4])
    {
        (void)bge_frustum_planes(viewProj16, homogeneousDepth ? 1 : 0, &planes[0][0]);
    }
    // The renderable entities inside the n planes (inward-pointing, n <= 16) after the last TransformSystem::Update, in ascending
    // index order: one query on the device, one copy of the visible matrices into their Transform::world (as FetchWorld writes them)
    bool FetchVisible(SceneT& scene, const float planes[][4], size_t n, std::vector<Id>& out)
    {
        out.clear();
        if (!ok() || !UploadBounds()) return false;
        bge_cull_desc desc{};
        desc.struct_size = sizeof desc;
        desc.n_planes = static_cast<uint32_t>(n);
        if (n > BGE_CULL_MAX_PLANES) return Log("FetchVisible: more than 16 planes");
        if (n) std::memcpy(desc.planes, planes, n * 16);
        const size_t cap = ids_.size();
        index_list_.resize(cap);
        if (!down_.resize(cap * 16 + 1)) return Log("bge_host_alloc");
        uint64_t total = 0;
        if (bge_world_visible(world_, &desc, index_list_.data(), down_.data(), nullptr, cap, &total) != BGE_OK) return Log("bge_world_visible");
        out.reserve(total);
        for (uint64_t k = 0; k < total; ++k) {
            const Id id = ids_[index_list_[k]];
            auto* t = scene.GetTransform(id);
            if (!t) continue;
            std::memcpy(t->world, &down_[16 * k], 64);
            out.push_back(id);
        }
        return true;
    }

    // EXTENSION: the draw key of an entity, the caller's id of its mesh + material (MeshRenderer { mesh, material },
    // src/ecs/MeshRenderer.h).  FetchDrawBatches groups the visible entities by it (include/bge_world.h "Draw batches").  Kept per
    // EntityId and sent lazily by dense index, as the bounds are.
    void SetDrawKey(Id id, uint32_t key)
    {
        draw_keys_[id] = key;
        draw_keys_stale_ = true;
    }
    void ClearDrawKey(Id id)
    {
        if (draw_keys_.erase(id)) draw_keys_stale_ = true;
    }
    // The visible entities (FetchVisible's rule) whose key is below n_keys, sorted by (key, index): batches[k] is the range of `out`
    // that holds key k.  One query on the device, one copy of the listed matrices into their Transform::world.
    bool FetchDrawBatches(SceneT& scene, const float planes[][4], size_t n, uint32_t n_keys, std::vector<bge_draw_batch>& batches,
                          std::vector<Id>& out)
    {
        out.clear();
        batches.clear();
        if (!ok() || !UploadBounds() || !UploadDrawKeys()) return false;
        bge_cull_desc desc{};
        desc.struct_size = sizeof desc;
        desc.n_planes = static_cast<uint32_t>(n);
        if (n > BGE_CULL_MAX_PLANES) return Log("FetchDrawBatches: more than 16 planes");
        if (n_keys == 0 || n_keys > BGE_DRAW_MAX_KEYS) return Log("FetchDrawBatches: n_keys outside [1, 65536]");
        if (n) std::memcpy(desc.planes, planes, n * 16);
        const size_t cap = ids_.size();
        index_list_.resize(cap);
        batches.resize(n_keys);
        if (!down_.resize(cap * 16 + 1)) return Log("bge_host_alloc");
        uint64_t total = 0;
        if (bge_world_draw_batches(world_, &desc, n_keys, batches.data(), index_list_.data(), down_.data(), nullptr, cap, &total) != BGE_OK) {
            batches.clear();
            return Log("bge_world_draw_batches");
        }
        out.reserve(total);
        for (uint64_t k = 0; k < total; ++k) { // (every listed entity owns a Transform: out[k] is record k)
            const Id id = ids_[index_list_[k]];
            if (auto* t = scene.GetTransform(id)) std::memcpy(t->world, &down_[16 * k], 64);
            out.push_back(id);
        }
        return true;
    }

    // --- TransformSystem::Update(Scene&)
    bool UpdateTransforms(SceneT& scene)
    {
        if (!ok() || !RefreshTopology(scene) || !UploadDirtyTransforms(scene) || !UploadBounds() || !UploadDrawKeys()) return false;
        if (bge_world_tick(world_, 0.0f, gravity, BGE_TICK_TRANSFORMS) != BGE_OK) return Log("bge_world_tick");
        const size_t n = ids_.size();
        if (resident) {
            limbo_.resize(n);
            if (n && bge_world_download_dirty(world_, 0, n, limbo_.data()) != BGE_OK) return Log("bge_world_download_dirty");
            for (auto& kv : scene.GetTransforms()) {
                const uint32_t i = index_of_[kv.first];
                if (limbo_[i]) continue;
                kv.second.dirty = false;
                written_[i] = 0;
            }
            return true;
        }
        if (!down_.resize(n * 16 + 1)) return Log("bge_host_alloc");
        if (n && bge_world_download_world(world_, 0, n, down_.data()) != BGE_OK) return Log("bge_world_download_world");
        limbo_.resize(n);
        if (n && bge_world_download_dirty(world_, 0, n, limbo_.data()) != BGE_OK) return Log("bge_world_download_dirty");
        for (auto& kv : scene.GetTransforms()) {
            const uint32_t i = index_of_[kv.first];
            if (limbo_[i]) continue; // inside a parent cycle: the reference never reaches it, it stays dirty
            std::memcpy(kv.second.world, &down_[16 * static_cast<size_t>(i)], 64);
            kv.second.dirty = false;
            written_[i] = 0;
        }
        return true;
    }

    // --- rigid-body slice of PhysicsSystem::Update(Scene&, camera, input, dt)
    // How UpdatePhysics steps the world: Bullet's stepSimulation(dt, max_sub_steps, fixed_step) (PhysicsSystem.cpp:855-863).
    // max_sub_steps < 0: exactly one step of dt per call (no clock) — identical while the caller passes dt == fixed_step.
    int max_sub_steps = 4;
    float fixed_step = 1.0f / 120.0f;
    int last_sub_steps = 0; // stepSimulation's return value of the last call
    int ground_plane_state = 1; // what the world was last told (GpuPhysicsSystem keeps it in step with its own switch)

    bool UpdatePhysics(SceneT& scene, double dt)
    {
        if (!ok() || !RefreshTopology(scene) || !UploadBodies(scene) || !UploadDirtyTransforms(scene)) return false;
        if (!FlushImpulses()) return false; // (what ApplyImpulse .. queued since the last Update, before the step)
        uint32_t flags = BGE_TICK_PHYSICS;
        if (bullet_basis) flags |= BGE_TICK_BULLET_BASIS;
        bool triggers = false;
        if constexpr (detail::has_trigger_volumes<SceneT>::value) {
            if (!UploadTriggers(scene, triggers)) return false;
            if (triggers) flags |= BGE_TICK_BROADPHASE; // the ghost overlaps come out of the broadphase step
        }
        if (max_sub_steps < 0) {
            last_sub_steps = 1;
            if (bge_world_tick(world_, static_cast<float>(dt), gravity, flags) != BGE_OK) return Log("bge_world_tick");
        } else if (bge_world_step_simulation(world_, dt, max_sub_steps, fixed_step, gravity, flags, &last_sub_steps) != BGE_OK) {
            return Log("bge_world_step_simulation");
        }
        trigger_events_.clear();
        if constexpr (detail::has_trigger_volumes<SceneT>::value) {
            if (triggers && !FetchTriggerEvents(scene)) return false;
        }
        // SyncRigidBodiesFromPhysics: Dynamic bodies only (PhysicsSystem.cpp:926-948)
        index_list_.clear();
        for (auto& kv : scene.GetRigidBodies()) {
            auto it = index_of_.find(kv.first);
            if (it == index_of_.end() || !body_[it->second].exists) continue;
            if (static_cast<int>(kv.second.type) == 1) index_list_.push_back(it->second);
        }
        const size_t m = index_list_.size();
        if (!down_.resize(m * 6 + 1)) return Log("bge_host_alloc");
        if (m && bge_world_download_pose_indexed(world_, m, index_list_.data(), down_.data(), down_.data() + 3 * m) != BGE_OK) {
            return Log("bge_world_download_pose_indexed");
        }
        for (size_t k = 0; k < m; ++k) {
            const uint32_t i = index_list_[k];
            auto* t = scene.GetTransform(ids_[i]);
            if (!t) continue;
            std::memcpy(static_cast<void*>(&t->position), &down_[3 * k], 12);
            std::memcpy(static_cast<void*>(&t->rotationEuler), &down_[3 * m + 3 * k], 12);
            t->MarkDirty();
            std::memcpy(&last_pose_[6 * static_cast<size_t>(i)], &down_[3 * k], 12);
            std::memcpy(&last_pose_[6 * static_cast<size_t>(i) + 3], &down_[3 * m + 3 * k], 12);
            written_[i] = 1;
        }
        return true;
    }

    // what LogStats prints as "bodies": m_world->getNumCollisionObjects() (PhysicsSystem.cpp:1332) — rigid bodies, active trigger
    // ghosts and, while it is in the world, the ground plane's object (:149-166)
    int CollisionObjectCount()
    {
        bge_world_info info{};
        if (!ok() || bge_world_get_info(world_, &info) != BGE_OK) return 0;
        int n = static_cast<int>(info.n_bodies) + (ground_plane_state ? 1 : 0);
        for (uint8_t a : t_active_) n += a ? 1 : 0;
        return n;
    }

    // Enter / Stay / Exit of the last UpdatePhysics (what ProcessTriggerEvents publishes, PhysicsSystem.cpp:1017-1074)
    const std::vector<GpuTriggerEvent>& TriggerEvents() const { return trigger_events_; }

    // PhysicsSystem::Raycast / RaycastAll (src/physics/PhysicsSystem.cpp:1076-1146) on the device world as the last Update left it
    // (include/bge_world.h states what a ray sees).  One launch pair and one small read-back per call.  HitT has the members of the
    // reference's PhysicsRaycastHit (src/physics/PhysicsAPI.h:12-18): entity, point, normal, distance.
    template <class Vec3, class HitT>
    bool Raycast(const Vec3& origin, const Vec3& direction, float maxDistance, uint32_t layerMask, HitT& outHit)
    {
        if (!ok() || !(maxDistance > 0.0f) || layerMask == 0u) return false;
        const bge_ray ray = MakeRay(origin, direction, maxDistance, layerMask);
        bge_ray_hit h{};
        if (bge_world_raycast(world_, 1, &ray, &h) != BGE_OK) return Log("bge_world_raycast");
        if (h.kind == BGE_RAY_MISS) return false;
        FillHit(h, outHit);
        return true;
    }
    template <class HitT, class Vec3>
    std::vector<HitT> RaycastAll(const Vec3& origin, const Vec3& direction, float maxDistance, uint32_t layerMask)
    {
        std::vector<HitT> hits;
        if (!ok() || !(maxDistance > 0.0f) || layerMask == 0u) return hits;
        const bge_ray ray = MakeRay(origin, direction, maxDistance, layerMask);
        uint64_t total = 0;
        if (bge_world_raycast_all(world_, 1, &ray, nullptr, 0, nullptr, &total) != BGE_OK) {
            Log("bge_world_raycast_all");
            return hits;
        }
        ray_hits_.resize(total);
        if (total && bge_world_raycast_all(world_, 1, &ray, ray_hits_.data(), total, nullptr, &total) != BGE_OK) {
            Log("bge_world_raycast_all");
            return hits;
        }
        hits.resize(total);
        for (uint64_t i = 0; i < total; ++i) FillHit(ray_hits_[i], hits[i]);
        return hits;
    }

    // EXTENSIONS without a reference counterpart: a sphere swept along origin + direction * maxDistance and a sphere at rest
    // against the world the ray queries see (include/bge_world.h "Sphere queries") — the two primitives of a character
    // controller.  HitT as for Raycast: point is the contact point on the shape, normal points from it to the sphere's centre.
    template <class Vec3, class HitT>
    bool SphereCast(const Vec3& origin, const Vec3& direction, float maxDistance, float radius, uint32_t layerMask, HitT& outHit)
    {
        if (!ok() || !(maxDistance > 0.0f) || !(radius >= 0.0f) || layerMask == 0u) return false;
        const bge_sphere_cast cast = MakeCast(origin, direction, maxDistance, radius, layerMask);
        bge_ray_hit h{};
        if (bge_world_sphere_cast(world_, 1, &cast, &h) != BGE_OK) return Log("bge_world_sphere_cast");
        if (h.kind == BGE_RAY_MISS) return false;
        FillHit(h, outHit);
        return true;
    }
    template <class HitT, class Vec3>
    std::vector<HitT> SphereCastAll(const Vec3& origin, const Vec3& direction, float maxDistance, float radius, uint32_t layerMask)
    {
        std::vector<HitT> hits;
        if (!ok() || !(maxDistance > 0.0f) || !(radius >= 0.0f) || layerMask == 0u) return hits;
        const bge_sphere_cast cast = MakeCast(origin, direction, maxDistance, radius, layerMask);
        uint64_t total = 0;
        if (bge_world_sphere_cast_all(world_, 1, &cast, nullptr, 0, nullptr, &total) != BGE_OK) {
            Log("bge_world_sphere_cast_all");
            return hits;
        }
        ray_hits_.resize(total);
        if (total && bge_world_sphere_cast_all(world_, 1, &cast, ray_hits_.data(), total, nullptr, &total) != BGE_OK) {
            Log("bge_world_sphere_cast_all");
            return hits;
        }
        hits.resize(total);
        for (uint64_t i = 0; i < total; ++i) FillHit(ray_hits_[i], hits[i]);
        return hits;
    }
    // every object within radius of center: bodies in ascending entity index, then trigger ghosts, then the plane
    template <class Vec3> std::vector<GpuOverlapHit> OverlapSphere(const Vec3& center, float radius, uint32_t layerMask)
    {
        std::vector<GpuOverlapHit> out;
        if (!ok() || !(radius >= 0.0f) || layerMask == 0u) return out;
        bge_sphere s{};
        s.center[0] = center.x, s.center[1] = center.y, s.center[2] = center.z;
        s.radius = radius;
        s.layer_mask = layerMask;
        uint64_t total = 0;
        if (bge_world_overlap_sphere(world_, 1, &s, nullptr, 0, nullptr, &total) != BGE_OK) {
            Log("bge_world_overlap_sphere");
            return out;
        }
        overlap_hits_.resize(total);
        if (total && bge_world_overlap_sphere(world_, 1, &s, overlap_hits_.data(), total, nullptr, &total) != BGE_OK) {
            Log("bge_world_overlap_sphere");
            return out;
        }
        out.resize(total);
        for (uint64_t i = 0; i < total; ++i) {
            const bge_overlap_hit& h = overlap_hits_[i];
            const bool has = h.entity != BGE_RAY_NO_ENTITY && h.entity < ids_.size();
            out[i].entity = has ? ids_[h.entity] : Id{0};
            out[i].trigger = h.kind == BGE_RAY_TRIGGER;
            out[i].distance = h.distance;
        }
        return out;
    }

    // EXTENSION: collide-and-slide moves of a batch of spheres (include/bge_world.h "Sphere moves"): each is moved by its
    // displacement, stopped at what it hits, slid along it, and probed for ground.  One call, no round trip per sphere or per
    // slide.  Nothing is written into a Transform: the caller applies result.position where it wants it.  false when there is
    // no world or the call failed; results[i].valid tells an invalid mover.
    template <class Vec3> bool MoveSpheres(const std::vector<GpuSphereMover<Vec3>>& movers, std::vector<GpuSphereMoveResult<Vec3>>& results)
    {
        results.assign(movers.size(), GpuSphereMoveResult<Vec3>{});
        for (size_t i = 0; i < movers.size(); ++i) results[i].position = movers[i].position;
        if (!ok()) return false;
        if (movers.empty()) return true;
        moves_.resize(movers.size());
        move_results_.resize(movers.size());
        for (size_t i = 0; i < movers.size(); ++i) {
            const GpuSphereMover<Vec3>& m = movers[i];
            bge_sphere_move& o = moves_[i];
            o = bge_sphere_move{};
            o.position[0] = m.position.x, o.position[1] = m.position.y, o.position[2] = m.position.z;
            o.displacement[0] = m.displacement.x, o.displacement[1] = m.displacement.y, o.displacement[2] = m.displacement.z;
            o.radius = m.radius;
            o.skin = m.skin;
            o.probe_distance = m.probeDistance;
            o.min_ground_ny = std::cos(m.maxSlopeRad);
            o.layer_mask = m.layerMask;
        }
        if (bge_world_sphere_move(world_, moves_.size(), moves_.data(), move_results_.data()) != BGE_OK) return Log("bge_world_sphere_move");
        for (size_t i = 0; i < movers.size(); ++i) {
            const bge_sphere_move_result& r = move_results_[i];
            GpuSphereMoveResult<Vec3>& o = results[i];
            o.position.x = r.position[0], o.position.y = r.position[1], o.position.z = r.position[2];
            o.remaining.x = r.remaining[0], o.remaining.y = r.remaining[1], o.remaining.z = r.remaining[2];
            o.valid = (r.flags & BGE_MOVE_INVALID) == 0u;
            o.grounded = (r.flags & BGE_MOVE_GROUNDED) != 0u;
            o.probeHit = (r.flags & BGE_MOVE_PROBE_HIT) != 0u;
            o.outOfSlides = (r.flags & BGE_MOVE_OUT_OF_SLIDES) != 0u;
            o.hits = r.n_hits;
            o.hitEntity = r.hit_entity != BGE_RAY_NO_ENTITY && r.hit_entity < ids_.size() ? ids_[r.hit_entity] : Id{0};
            o.hitTrigger = r.hit_kind == BGE_RAY_TRIGGER;
            o.hitNormal.x = r.hit_normal[0], o.hitNormal.y = r.hit_normal[1], o.hitNormal.z = r.hit_normal[2];
            o.groundEntity = r.ground_entity != BGE_RAY_NO_ENTITY && r.ground_entity < ids_.size() ? ids_[r.ground_entity] : Id{0};
            o.groundTrigger = r.ground_kind == BGE_RAY_TRIGGER;
            o.groundDistance = r.ground_distance;
            o.groundNormal.x = r.ground_normal[0], o.groundNormal.y = r.ground_normal[1], o.groundNormal.z = r.ground_normal[2];
        }
        return true;
    }
    // one sphere: true when it was moved (a valid mover on a world)
    template <class Vec3>
    bool MoveSphere(const Vec3& position, const Vec3& displacement, float radius, float skin, float probeDistance, float maxSlopeRad,
                    uint32_t layerMask, GpuSphereMoveResult<Vec3>& result)
    {
        std::vector<GpuSphereMover<Vec3>> one(1);
        one[0].position = position;
        one[0].displacement = displacement;
        one[0].radius = radius;
        one[0].skin = skin;
        one[0].probeDistance = probeDistance;
        one[0].maxSlopeRad = maxSlopeRad;
        one[0].layerMask = layerMask;
        std::vector<GpuSphereMoveResult<Vec3>> out;
        const bool done = MoveSpheres(one, out);
        result = out[0];
        return done && result.valid;
    }

    // EXTENSION: the same moves, stepping up over low obstacles (include/bge_world.h "Sphere step moves"): where the first thing
    // met is not walkable, the sphere is tried stepHeight higher, and the result is taken if it lands on walkable ground further
    // along.  One call, no round trip per sphere or per stage.  false when there is no world or the call failed.
    template <class Vec3>
    bool StepMoveSpheres(const std::vector<GpuSphereStepMover<Vec3>>& movers, std::vector<GpuSphereStepResult<Vec3>>& results)
    {
        results.assign(movers.size(), GpuSphereStepResult<Vec3>{});
        for (size_t i = 0; i < movers.size(); ++i) results[i].position = movers[i].position;
        if (!ok()) return false;
        if (movers.empty()) return true;
        step_moves_.resize(movers.size());
        step_results_.resize(movers.size());
        for (size_t i = 0; i < movers.size(); ++i) {
            const GpuSphereStepMover<Vec3>& m = movers[i];
            bge_sphere_step_move& o = step_moves_[i];
            o = bge_sphere_step_move{};
            o.position[0] = m.position.x, o.position[1] = m.position.y, o.position[2] = m.position.z;
            o.displacement[0] = m.displacement.x, o.displacement[1] = m.displacement.y, o.displacement[2] = m.displacement.z;
            o.radius = m.radius;
            o.skin = m.skin;
            o.probe_distance = m.probeDistance;
            o.min_ground_ny = std::cos(m.maxSlopeRad);
            o.layer_mask = m.layerMask;
            o.step_height = m.stepHeight;
        }
        if (bge_world_sphere_step_move(world_, step_moves_.size(), step_moves_.data(), step_results_.data()) != BGE_OK) {
            return Log("bge_world_sphere_step_move");
        }
        for (size_t i = 0; i < movers.size(); ++i) {
            const bge_sphere_step_result& r = step_results_[i];
            GpuSphereStepResult<Vec3>& o = results[i];
            o.position.x = r.position[0], o.position.y = r.position[1], o.position.z = r.position[2];
            o.remaining.x = r.remaining[0], o.remaining.y = r.remaining[1], o.remaining.z = r.remaining[2];
            o.valid = (r.flags & BGE_MOVE_INVALID) == 0u;
            o.grounded = (r.flags & BGE_MOVE_GROUNDED) != 0u;
            o.probeHit = (r.flags & BGE_MOVE_PROBE_HIT) != 0u;
            o.outOfSlides = (r.flags & BGE_MOVE_OUT_OF_SLIDES) != 0u;
            o.stepTried = (r.flags & BGE_MOVE_STEP_TRIED) != 0u;
            o.stepped = (r.flags & BGE_MOVE_STEPPED) != 0u;
            o.stepRise = r.step_rise;
            o.hits = r.n_hits;
            o.hitEntity = r.hit_entity != BGE_RAY_NO_ENTITY && r.hit_entity < ids_.size() ? ids_[r.hit_entity] : Id{0};
            o.hitTrigger = r.hit_kind == BGE_RAY_TRIGGER;
            o.hitNormal.x = r.hit_normal[0], o.hitNormal.y = r.hit_normal[1], o.hitNormal.z = r.hit_normal[2];
            o.groundEntity = r.ground_entity != BGE_RAY_NO_ENTITY && r.ground_entity < ids_.size() ? ids_[r.ground_entity] : Id{0};
            o.groundTrigger = r.ground_kind == BGE_RAY_TRIGGER;
            o.groundDistance = r.ground_distance;
            o.groundNormal.x = r.ground_normal[0], o.groundNormal.y = r.ground_normal[1], o.groundNormal.z = r.ground_normal[2];
        }
        return true;
    }
    // one sphere: true when it was moved (a valid mover on a world)
    template <class Vec3>
    bool StepMoveSphere(const Vec3& position, const Vec3& displacement, float radius, float skin, float probeDistance, float maxSlopeRad,
                        uint32_t layerMask, float stepHeight, GpuSphereStepResult<Vec3>& result)
    {
        std::vector<GpuSphereStepMover<Vec3>> one(1);
        one[0].position = position;
        one[0].displacement = displacement;
        one[0].radius = radius;
        one[0].skin = skin;
        one[0].probeDistance = probeDistance;
        one[0].maxSlopeRad = maxSlopeRad;
        one[0].layerMask = layerMask;
        one[0].stepHeight = stepHeight;
        std::vector<GpuSphereStepResult<Vec3>> out;
        const bool done = StepMoveSpheres(one, out);
        result = out[0];
        return done && result.valid;
    }

    // EXTENSION: the object that reaches deepest into a sphere at rest, with the depth and the way out (include/bge_world.h
    // "Sphere penetration and recovery"); false when nothing touches the sphere.
    template <class Vec3> bool SpherePenetration(const Vec3& center, float radius, uint32_t layerMask, GpuPenetrationHit<Vec3>& outHit)
    {
        if (!ok() || !(radius >= 0.0f) || layerMask == 0u) return false;
        bge_sphere s{};
        s.center[0] = center.x, s.center[1] = center.y, s.center[2] = center.z;
        s.radius = radius;
        s.layer_mask = layerMask;
        bge_penetration_hit h{};
        if (bge_world_sphere_penetration(world_, 1, &s, &h) != BGE_OK) return Log("bge_world_sphere_penetration");
        if (h.kind == BGE_RAY_MISS) return false;
        outHit.entity = h.entity != BGE_RAY_NO_ENTITY && h.entity < ids_.size() ? ids_[h.entity] : Id{0};
        outHit.trigger = h.kind == BGE_RAY_TRIGGER;
        outHit.depth = h.depth;
        outHit.point.x = h.point[0], outHit.point.y = h.point[1], outHit.point.z = h.point[2];
        outHit.normal.x = h.normal[0], outHit.normal.y = h.normal[1], outHit.normal.z = h.normal[2];
        return true;
    }

    // EXTENSION: a batch of spheres pushed out of what they touch or penetrate, before they are moved (recover, then
    // MoveSpheres).  One call, no round trip per sphere or per push.  Nothing is written into a Transform.  false when there is
    // no world or the call failed; results[i].valid tells an invalid record.
    template <class Vec3>
    bool RecoverSpheres(const std::vector<GpuSphereRecover<Vec3>>& spheres, std::vector<GpuSphereRecoverResult<Vec3>>& results)
    {
        results.assign(spheres.size(), GpuSphereRecoverResult<Vec3>{});
        for (size_t i = 0; i < spheres.size(); ++i) results[i].position = spheres[i].position;
        if (!ok()) return false;
        if (spheres.empty()) return true;
        recovers_.resize(spheres.size());
        recover_results_.resize(spheres.size());
        for (size_t i = 0; i < spheres.size(); ++i) {
            const GpuSphereRecover<Vec3>& m = spheres[i];
            bge_sphere_recover& o = recovers_[i];
            o = bge_sphere_recover{};
            o.position[0] = m.position.x, o.position[1] = m.position.y, o.position[2] = m.position.z;
            o.radius = m.radius;
            o.skin = m.skin;
            o.layer_mask = m.layerMask;
        }
        if (bge_world_sphere_recover(world_, recovers_.size(), recovers_.data(), recover_results_.data()) != BGE_OK) {
            return Log("bge_world_sphere_recover");
        }
        for (size_t i = 0; i < spheres.size(); ++i) {
            const bge_sphere_recover_result& r = recover_results_[i];
            GpuSphereRecoverResult<Vec3>& o = results[i];
            o.position.x = r.position[0], o.position.y = r.position[1], o.position.z = r.position[2];
            o.pushed.x = r.pushed[0], o.pushed.y = r.pushed[1], o.pushed.z = r.pushed[2];
            o.valid = (r.flags & BGE_RECOVER_INVALID) == 0u;
            o.moved = (r.flags & BGE_RECOVER_MOVED) != 0u;
            o.stuck = (r.flags & BGE_RECOVER_STUCK) != 0u;
            o.pushes = r.n_pushes;
            o.hitEntity = r.hit_entity != BGE_RAY_NO_ENTITY && r.hit_entity < ids_.size() ? ids_[r.hit_entity] : Id{0};
            o.hitTrigger = r.hit_kind == BGE_RAY_TRIGGER;
            o.hitNormal.x = r.hit_normal[0], o.hitNormal.y = r.hit_normal[1], o.hitNormal.z = r.hit_normal[2];
            o.hitDepth = r.hit_depth;
            o.remainingDepth = r.remaining_depth;
        }
        return true;
    }
    // one sphere: true when it was recovered (a valid record on a world)
    template <class Vec3>
    bool RecoverSphere(const Vec3& position, float radius, float skin, uint32_t layerMask, GpuSphereRecoverResult<Vec3>& result)
    {
        std::vector<GpuSphereRecover<Vec3>> one(1);
        one[0].position = position;
        one[0].radius = radius;
        one[0].skin = skin;
        one[0].layerMask = layerMask;
        std::vector<GpuSphereRecoverResult<Vec3>> out;
        const bool done = RecoverSpheres(one, out);
        result = out[0];
        return done && result.valid;
    }

    // EXTENSION: the scene's characters (include/bge_world.h "Characters"): a set of sphere characters that lives on the device;
    // one UpdateCharacters runs a frame's sub-steps for all of them, one SyncCharacters brings the states back.  The device's set is
    // replaced as a whole, so adding a character re-creates it on the next UpdateCharacters: the others keep their position as of
    // the last SyncCharacters and are, like the new one, at rest and not grounded.
    bool AddCharacter(SceneT& scene, Id entity, const GpuCharacterKnobs& k)
    {
        auto* t = scene.GetTransform(entity);
        if (!t || char_index_.count(entity)) return false;
        bge_character_desc d{};
        d.position[0] = t->position.x, d.position[1] = t->position.y, d.position[2] = t->position.z;
        d.radius = k.radius;
        d.skin = k.skin;
        d.step_height = k.stepHeight;
        d.min_ground_ny = std::cos(k.maxSlopeRad);
        d.probe_distance = k.probeDistance;
        d.gravity = k.gravity;
        d.jump_speed = k.jumpSpeed;
        d.fall_speed = k.fallSpeed;
        d.layer_mask = k.layerMask;
        for (size_t i = 0; i < char_states_.size() && i < char_descs_.size(); ++i) std::memcpy(char_descs_[i].position, char_states_[i].position, 12);
        char_index_[entity] = static_cast<uint32_t>(char_ids_.size());
        char_ids_.push_back(entity);
        char_descs_.push_back(d);
        char_inputs_.push_back(bge_character_input{});
        chars_stale_ = true;
        return true;
    }
    void RemoveCharacters()
    {
        char_ids_.clear();
        char_index_.clear();
        char_descs_.clear();
        char_inputs_.clear();
        char_states_.clear();
        chars_stale_ = char_inputs_stale_ = false;
        char_trig_watching_ = char_trig_pending_ = false; // (creating the set turns the device's watch off)
        char_trigger_events_.clear();
        char_ride_applied_ = 0u; // (and riding)
        char_rides_.clear();
        char_crowd_applied_ = false; // (and the crowd)
        char_crowd_hits_.clear();
        if (ok() && bge_world_characters_create(world_, 0, nullptr) != BGE_OK) Log("bge_world_characters_create");
    }
    // EXTENSION: trigger events for the characters (include/bge_world.h "Character trigger events"), off by default: every
    // UpdateCharacters makes the Enter / Stay / Exit list of the characters against the trigger volumes on the device, SyncCharacters
    // fetches it.  `other` of an event is the character's EntityId.  TriggerEvents() is untouched.
    void SetCharacterTriggerEvents(bool on)
    {
        if (on == char_trig_on_) return;
        char_trig_on_ = on;
        if (!on) char_trigger_events_.clear();
    }
    // the list of the last UpdateCharacters, as of the last SyncCharacters, in the device's order
    const std::vector<GpuTriggerEvent>& CharacterTriggerEvents() const { return char_trigger_events_; }
    // EXTENSION: characters ride moving platforms (include/bge_world.h "Character platform riding"), off by default: every
    // UpdateCharacters begins by moving each grounded character with the Static or Kinematic body it stood on (with dynamicBodies
    // a Dynamic one too).  Applied by the next UpdateCharacters; re-creating the set loses no anchor worth keeping, since
    // re-created characters are not grounded.
    void SetCharacterPlatformRiding(bool on, bool dynamicBodies = false)
    {
        char_ride_want_ = 0u;
        if (on) char_ride_want_ = static_cast<uint32_t>(BGE_CHAR_RIDE_ON) | (dynamicBodies ? static_cast<uint32_t>(BGE_CHAR_RIDE_DYNAMIC) : 0u);
        if (!on) char_rides_.clear();
    }
    // carried, turn and the platform of the last UpdateCharacters, as of the last SyncCharacters; false while riding is off
    template <class Vec3> bool GetCharacterRide(Id entity, GpuCharacterRide<Vec3>& out) const
    {
        auto it = char_index_.find(entity);
        if (it == char_index_.end() || it->second >= char_rides_.size()) return false;
        const bge_character_ride& r = char_rides_[it->second];
        out = GpuCharacterRide<Vec3>{};
        out.carried = (r.flags & BGE_CHAR_RIDE_CARRIED) != 0u;
        out.lost = (r.flags & BGE_CHAR_RIDE_LOST) != 0u;
        out.platform = r.entity != BGE_RAY_NO_ENTITY && r.entity < ids_.size() ? ids_[r.entity] : Id{0};
        out.carriedBy.x = r.carried[0], out.carriedBy.y = r.carried[1], out.carriedBy.z = r.carried[2];
        for (int k = 0; k < 4; ++k) out.turn[k] = r.turn[k];
        return true;
    }
    // EXTENSION: characters push each other apart (include/bge_world.h "Crowd separation"), off by default: every step of
    // UpdateCharacters begins by moving each character away from the character that overlaps it deepest, by half the overlap and
    // at most maxPush (0 = no limit).  Every character is of group 1 and sees all.  Applied by the next UpdateCharacters, and
    // again whenever AddCharacter re-creates the set.
    void SetCharacterCrowd(bool on, float maxPush = 0.0f)
    {
        char_crowd_want_ = on;
        char_crowd_max_push_ = on ? maxPush : 0.0f;
        if (!on) char_crowd_hits_.clear();
    }
    // what the last step of the last UpdateCharacters found, as of the last SyncCharacters; false while the crowd is off
    template <class Vec3> bool GetCharacterCrowd(Id entity, GpuCharacterCrowd<Vec3>& out) const
    {
        auto it = char_index_.find(entity);
        if (it == char_index_.end() || it->second >= char_crowd_hits_.size()) return false;
        const bge_crowd_hit& h = char_crowd_hits_[it->second];
        out = GpuCharacterCrowd<Vec3>{};
        out.pushed = (h.flags & BGE_CROWD_PUSHED) != 0u;
        out.clamped = (h.flags & BGE_CROWD_CLAMPED) != 0u;
        out.other = h.other != BGE_RAY_NO_ENTITY && h.other < char_ids_.size() ? char_ids_[h.other] : Id{0};
        out.overlaps = h.n_overlaps;
        out.depth = h.depth;
        out.push.x = h.push[0], out.push.y = h.push[1], out.push.z = h.push[2];
        return true;
    }
    // EXTENSION: characters push the Dynamic bodies they walk into (include/bge_world.h "Character push"), off by default: every
    // step of UpdateCharacters ends by giving the body hit an impulse of force * dt, level, away from the character.  Applied by
    // the next UpdateCharacters, and again whenever AddCharacter re-creates the set.
    void SetCharacterPush(bool on, float force = 0.0f, float maxNormalY = 0.5f)
    {
        char_push_want_ = bge_character_push_desc{on ? static_cast<uint32_t>(BGE_CHAR_PUSH_ON) : 0u, on ? force : 0.0f, on ? maxNormalY : 0.0f,
                                                  on ? 0xffffffffu : 0u};
    }
    // EXTENSION: impulses on Dynamic bodies (include/bge_world.h "Impulses"): Bullet's applyImpulse / applyCentralImpulse /
    // applyTorqueImpulse + activate().  Queued here, in call order, and applied as one batch at the head of the next UpdatePhysics,
    // after that frame's uploads and before its step.  An entity that has no Dynamic body by then is skipped.
    void QueueImpulse(Id entity, uint32_t flags, const float impulse[3], const float point[3])
    {
        bge_impulse r{};
        r.flags = flags;
        std::memcpy(r.impulse, impulse, 12);
        std::memcpy(r.point, point, 12);
        impulse_ids_.push_back(entity);
        impulses_.push_back(r);
    }
    size_t QueuedImpulses() const { return impulses_.size(); }
    // EXTENSION: the query index (include/bge_world.h "Query index"), off by default: every query, move, recovery and character
    // step visits only the bodies near it instead of all of them; every answer keeps its bytes.  cellEdge = 0: the library's.
    bool SetQueryIndex(bool on, float cellEdge = 0.0f)
    {
        bge_query_index_desc d{};
        d.mode = on ? 1u : 0u;
        d.cell_edge = cellEdge;
        d.min_work = BGE_QUERY_INDEX_MIN_WORK_DEFAULT;
        return bge_world_set_query_index(world_, &d) == BGE_OK || Log("bge_world_set_query_index");
    }
    // what the last call that queried did with it (synchronises the world's stream)
    bool GetQueryIndexStats(bge_query_index_stats& out) const
    {
        return bge_world_query_index_stats(world_, &out) == BGE_OK || Log("bge_world_query_index_stats");
    }
    size_t CharacterCount() const { return char_ids_.size(); }
    bool SetCharacterWalk(Id entity, float dx, float dz)
    {
        auto it = char_index_.find(entity);
        if (it == char_index_.end()) return false;
        char_inputs_[it->second].walk_x = dx;
        char_inputs_[it->second].walk_z = dz;
        char_inputs_stale_ = true;
        return true;
    }
    bool CharacterJump(Id entity) // the edge; the device jumps only a character that stands on ground
    {
        auto it = char_index_.find(entity);
        if (it == char_index_.end()) return false;
        char_inputs_[it->second].buttons |= BGE_CHAR_BUTTON_JUMP;
        char_inputs_stale_ = true;
        return true;
    }
    template <class Vec3> bool WarpCharacter(Id entity, const Vec3& position)
    {
        auto it = char_index_.find(entity);
        if (it == char_index_.end()) return false;
        const float p[3] = {position.x, position.y, position.z};
        if (it->second < char_states_.size()) std::memcpy(char_states_[it->second].position, p, 12);
        if (chars_stale_) { // not on the device yet: it will be created there
            std::memcpy(char_descs_[it->second].position, p, 12);
            return true;
        }
        if (!ok()) return false;
        if (bge_world_characters_warp(world_, 1, &it->second, p) != BGE_OK) return Log("bge_world_characters_warp");
        return true;
    }
    // `steps` steps of length dt for every character, enqueued; nothing is read back (SyncCharacters does that)
    bool UpdateCharacters(float dt, uint32_t steps)
    {
        if (!ok()) return false;
        if (char_ids_.empty() || steps == 0u) return true; // (a frame without a sub-step: the walk and a pending jump wait for the next)
        if (chars_stale_) {
            // Re-creating the set forgets which volume each character stands in: read that before and put it back after (the
            // indices of the characters that were there do not change), so that nobody Enters a volume again because another
            // character was added
            char_overlaps_.clear();
            if (char_trig_watching_) {
                uint64_t total = 0;
                if (bge_world_characters_trigger_overlaps(world_, 0, nullptr, &total) != BGE_OK) return Log("bge_world_characters_trigger_overlaps");
                char_overlaps_.resize(2 * total);
                if (total && bge_world_characters_trigger_overlaps(world_, total, char_overlaps_.data(), &total) != BGE_OK) {
                    return Log("bge_world_characters_trigger_overlaps");
                }
            }
            if (bge_world_characters_create(world_, char_descs_.size(), char_descs_.data()) != BGE_OK) return Log("bge_world_characters_create");
            chars_stale_ = false;
            char_inputs_stale_ = true;
            char_trig_watching_ = false;
            char_ride_applied_ = 0u; // (creating the set switched riding off)
            char_crowd_applied_ = false; // (and the crowd)
            char_push_applied_ = bge_character_push_desc{0u, 0.0f, 0.0f, 0u}; // (and push)
        }
        if (char_crowd_want_ != char_crowd_applied_ || (char_crowd_want_ && char_crowd_max_push_ != char_crowd_applied_push_)) {
            if (bge_world_characters_crowd(world_, char_crowd_want_ ? static_cast<uint32_t>(BGE_CHAR_CROWD_ON) : 0u, char_crowd_max_push_,
                                           char_crowd_want_ ? char_descs_.size() : 0, nullptr, nullptr) != BGE_OK) {
                return Log("bge_world_characters_crowd");
            }
            char_crowd_applied_ = char_crowd_want_;
            char_crowd_applied_push_ = char_crowd_max_push_;
        }
        if (std::memcmp(&char_push_want_, &char_push_applied_, sizeof char_push_want_) != 0) {
            if (bge_world_characters_push(world_, &char_push_want_) != BGE_OK) return Log("bge_world_characters_push");
            char_push_applied_ = char_push_want_;
        }
        if (char_ride_want_ != char_ride_applied_) {
            if (bge_world_characters_ride(world_, char_ride_want_) != BGE_OK) return Log("bge_world_characters_ride");
            char_ride_applied_ = char_ride_want_;
        }
        if (char_trig_on_ != char_trig_watching_) {
            if (bge_world_characters_watch_triggers(world_, char_trig_on_ ? char_descs_.size() : 0, nullptr, nullptr, BGE_CHAR_TRIGGER_STAY_EVENTS, 0) !=
                BGE_OK) {
                return Log("bge_world_characters_watch_triggers");
            }
            char_trig_watching_ = char_trig_on_;
            if (char_trig_on_ && !char_overlaps_.empty() &&
                bge_world_characters_set_trigger_overlaps(world_, char_overlaps_.size() / 2, char_overlaps_.data()) != BGE_OK) {
                return Log("bge_world_characters_set_trigger_overlaps");
            }
            char_overlaps_.clear();
        }
        if (char_inputs_stale_) {
            if (bge_world_characters_set_input(world_, 0, char_inputs_.size(), char_inputs_.data()) != BGE_OK) return Log("bge_world_characters_set_input");
            char_inputs_stale_ = false;
        }
        if (bge_world_characters_update(world_, dt, steps) != BGE_OK) return Log("bge_world_characters_update");
        for (bge_character_input& in : char_inputs_) in.buttons &= ~static_cast<uint32_t>(BGE_CHAR_BUTTON_JUMP); // (the update consumed the edges)
        char_trig_pending_ = char_trig_watching_;
        return true;
    }
    // One download; each character's position goes into its Transform, as SyncRigidBodiesFromPhysics does for bodies
    bool SyncCharacters(SceneT& scene)
    {
        if (!ok()) return false;
        if (char_ids_.empty() || chars_stale_) return true;
        char_states_.resize(char_ids_.size());
        if (bge_world_characters_download(world_, 0, char_states_.size(), char_states_.data()) != BGE_OK) return Log("bge_world_characters_download");
        for (size_t i = 0; i < char_ids_.size(); ++i) {
            auto* t = scene.GetTransform(char_ids_[i]);
            if (!t) continue;
            std::memcpy(static_cast<void*>(&t->position), char_states_[i].position, 12);
            t->MarkDirty();
        }
        char_rides_.resize(char_ride_applied_ ? char_ids_.size() : 0);
        if (!char_rides_.empty() && bge_world_characters_rides(world_, 0, char_rides_.size(), char_rides_.data()) != BGE_OK) {
            char_rides_.clear();
            return Log("bge_world_characters_rides");
        }
        char_crowd_hits_.resize(char_crowd_applied_ ? char_ids_.size() : 0);
        if (!char_crowd_hits_.empty() && bge_world_characters_crowd_hits(world_, 0, char_crowd_hits_.size(), char_crowd_hits_.data()) != BGE_OK) {
            char_crowd_hits_.clear();
            return Log("bge_world_characters_crowd_hits");
        }
        return FetchCharacterTriggerEvents(scene);
    }
    bool CharacterOnGround(Id entity) const
    {
        auto it = char_index_.find(entity);
        return it != char_index_.end() && it->second < char_states_.size() && (char_states_[it->second].flags & BGE_CHAR_GROUNDED) != 0u;
    }
    template <class Vec3> bool GetCharacterState(Id entity, GpuCharacterState<Vec3>& out) const
    {
        auto it = char_index_.find(entity);
        if (it == char_index_.end() || it->second >= char_states_.size()) return false;
        const bge_character_state& s = char_states_[it->second];
        out = GpuCharacterState<Vec3>{};
        out.position.x = s.position[0], out.position.y = s.position[1], out.position.z = s.position[2];
        out.verticalVelocity = s.vertical_velocity;
        out.valid = (s.flags & BGE_CHAR_INVALID) == 0u;
        out.grounded = (s.flags & BGE_CHAR_GROUNDED) != 0u;
        out.jumped = (s.flags & BGE_CHAR_JUMPED) != 0u;
        out.landed = (s.flags & BGE_CHAR_LANDED) != 0u;
        out.headBump = (s.flags & BGE_CHAR_HEAD_BUMP) != 0u;
        out.recovered = (s.flags & BGE_CHAR_RECOVERED) != 0u;
        out.stuck = (s.flags & BGE_CHAR_STUCK) != 0u;
        out.stepped = (s.flags & BGE_CHAR_STEPPED) != 0u;
        out.outOfSlides = (s.flags & BGE_CHAR_OUT_OF_SLIDES) != 0u;
        out.groundEntity = s.ground_entity != BGE_RAY_NO_ENTITY && s.ground_entity < ids_.size() ? ids_[s.ground_entity] : Id{0};
        out.groundTrigger = s.ground_kind == BGE_RAY_TRIGGER;
        out.groundNormal.x = s.ground_normal[0], out.groundNormal.y = s.ground_normal[1], out.groundNormal.z = s.ground_normal[2];
        out.hitEntity = s.hit_entity != BGE_RAY_NO_ENTITY && s.hit_entity < ids_.size() ? ids_[s.hit_entity] : Id{0};
        out.hitTrigger = s.hit_kind == BGE_RAY_TRIGGER;
        out.hitNormal.x = s.hit_normal[0], out.hitNormal.y = s.hit_normal[1], out.hitNormal.z = s.hit_normal[2];
        out.stepRise = s.step_rise;
        out.recoveredBy.x = s.recovered[0], out.recoveredBy.y = s.recovered[1], out.recoveredBy.z = s.recovered[2];
        out.steps = s.steps;
        return true;
    }

    // CollectDebugLines + debugDrawWorld(DBG_DrawContactPoints) (PhysicsSystem.cpp:857-873, 1148-1175) on the device world as
    // the last Update left it: the count, then the lines (include/bge_world.h states what is drawn and in which order)
    bool DebugLines(const bge_debug_desc& desc, DebugLineBuffer& out)
    {
        out.clear();
        if (!ok()) return false;
        uint64_t total = 0;
        if (bge_world_debug_lines(world_, &desc, nullptr, 0, &total) != BGE_OK) return Log("bge_world_debug_lines");
        out.resize(total);
        if (total == 0) return true;
        if (bge_world_debug_lines(world_, &desc, out.data(), total, &total) != BGE_OK) {
            out.clear();
            return Log("bge_world_debug_lines");
        }
        out.resize(total);
        return true;
    }

private:
    // EnsureTrigger (PhysicsSystem.cpp:523-590): the trigger set is re-sent when a TriggerVolume appeared, vanished or
    // changed; remembered overlaps survive on the device side for unchanged triggers
    bool UploadTriggers(SceneT& scene, bool& any)
    {
        auto& vols = scene.GetTriggerVolumes();
        t_entity_.clear(); t_shape_.clear(); t_size_.clear(); t_layer_.clear(); t_mask_.clear(); t_oneshot_.clear(); t_active_.clear();
        bool dirty = false;
        seen_trigger_.assign(ids_.size(), 0);
        // ProcessTriggerEvents' loop order matters once a one-shot trigger overlaps another trigger (bge_world.h): the world walks
        // the uploaded array, the reference an unordered_map (unspecified order) — ascending EntityId here, as in the oracle
        t_order_.clear();
        for (auto& kv : vols) t_order_.push_back(kv.first);
        std::sort(t_order_.begin(), t_order_.end());
        for (const auto id : t_order_) {
            auto vit = vols.find(id);
            auto& kv = *vit;
            auto it = index_of_.find(kv.first);
            uint32_t index;
            bool without_transform = false;
            if (it != index_of_.end()) {
                index = it->second;
            } else {
                // a trigger needs a Transform to be created or re-posed (PhysicsSystem.cpp:530-534) — but a ghost whose entity lost
                // its Transform stays in the world where it was: the entity's index was kept for it (RefreshTopology)
                auto o = orphan_of_.find(kv.first);
                if (o == orphan_of_.end() || !has_trigger_[o->second]) continue;
                index = o->second;
                without_transform = true;
            }
            seen_trigger_[index] = 1;
            has_trigger_[index] = 1;
            auto& tv = kv.second;
            t_entity_.push_back(index);
            t_shape_.push_back(static_cast<uint8_t>(static_cast<int>(tv.shape)));
            t_size_.push_back(tv.size.x); t_size_.push_back(tv.size.y); t_size_.push_back(tv.size.z);
            t_layer_.push_back(tv.layer);
            t_mask_.push_back(tv.mask);
            t_oneshot_.push_back(tv.oneShot ? 1 : 0);
            t_active_.push_back(tv.active ? 1 : 0);
            if (!without_transform) { // (EnsureTrigger does not reach the other ones: their dirty flag waits)
                dirty = dirty || tv.dirty;
                tv.dirty = false;
            }
        }
        for (uint32_t i = 0; i < ids_.size(); ++i) {
            if (has_trigger_[i] && !seen_trigger_[i]) { // the component is gone
                has_trigger_[i] = 0;
                RetireIfNothingLeft(i);
            }
        }
        any = !t_entity_.empty();
        // signature of the set: everything that reaches the device
        std::vector<uint32_t> sig;
        sig.reserve(t_entity_.size() * 8);
        for (size_t k = 0; k < t_entity_.size(); ++k) {
            uint32_t sz[3];
            std::memcpy(sz, &t_size_[3 * k], 12);
            sig.insert(sig.end(), {t_entity_[k], t_shape_[k], sz[0], sz[1], sz[2], t_layer_[k], t_mask_[k],
                                   static_cast<uint32_t>(t_oneshot_[k] | (t_active_[k] << 1))});
        }
        if (!dirty && sig == t_signature_) return true;
        t_signature_ = sig;
        if (bge_world_upload_triggers(world_, t_entity_.size(), t_entity_.data(), t_shape_.data(), t_size_.data(), t_layer_.data(),
                                      t_mask_.data(), t_oneshot_.data(), t_active_.data()) != BGE_OK) {
            return Log("bge_world_upload_triggers");
        }
        return true;
    }

    // The list of the last UpdateCharacters, once.  A one-shot volume with an Enter in it is switched off in the scene, so the next
    // trigger upload takes its ghost out of the world (PhysicsSystem.cpp:1062-1072) and it reports nothing further.
    bool FetchCharacterTriggerEvents(SceneT& scene)
    {
        char_trigger_events_.clear();
        if (!char_trig_pending_) return true;
        char_trig_pending_ = false;
        uint64_t total = 0;
        if (bge_world_characters_trigger_events(world_, nullptr, 0, &total) != BGE_OK) return Log("bge_world_characters_trigger_events");
        raw_char_events_.resize(total);
        if (total && bge_world_characters_trigger_events(world_, raw_char_events_.data(), total, &total) != BGE_OK) {
            return Log("bge_world_characters_trigger_events");
        }
        for (const bge_character_trigger_event& e : raw_char_events_) {
            if (e.trigger >= ids_.size() || e.character >= char_ids_.size()) continue;
            char_trigger_events_.push_back(GpuTriggerEvent{static_cast<GpuTriggerEvent::Type>(e.type), ids_[e.trigger], char_ids_[e.character]});
            if (e.type == BGE_CHAR_TRIGGER_ENTER) {
                if (auto* tv = scene.GetTriggerVolume(ids_[e.trigger])) {
                    if (tv->oneShot && tv->active) tv->active = false;
                }
            }
        }
        return true;
    }

    bool FetchTriggerEvents(SceneT& scene)
    {
        uint64_t total = 0;
        if (bge_world_trigger_events(world_, nullptr, 0, &total) != BGE_OK) return Log("bge_world_trigger_events");
        raw_events_.resize(total);
        if (bge_world_trigger_events(world_, raw_events_.data(), total, &total) != BGE_OK) return Log("bge_world_trigger_events");
        for (const bge_trigger_event& e : raw_events_) {
            trigger_events_.push_back(GpuTriggerEvent{static_cast<GpuTriggerEvent::Type>(e.type), last_ids_[e.trigger], last_ids_[e.other]});
        }
        // one-shot triggers that fired are now inactive (PhysicsSystem.cpp:1062-1071)
        if (!t_entity_.empty()) {
            t_active_.resize(t_entity_.size());
            if (bge_world_trigger_active(world_, t_entity_.size(), t_entity_.data(), t_active_.data()) != BGE_OK) return Log("bge_world_trigger_active");
            for (size_t k = 0; k < t_entity_.size(); ++k) {
                if (auto* tv = scene.GetTriggerVolume(ids_[t_entity_[k]])) {
                    if (tv->active && !t_active_[k]) tv->active = false;
                }
            }
        }
        return true;
    }

    struct BodyState {
        bool exists = false;
    };
    struct Bounds {
        float v[6]; // centre, half extents
    };

    // bounds the device should hold per index against what it was last sent: only the rows that differ travel
    bool UploadBounds()
    {
        if (!bounds_stale_) return true;
        static constexpr float kNoBounds[6] = {0.0f, 0.0f, 0.0f, -1.0f, -1.0f, -1.0f}; // a negative half extent: not renderable
        const size_t n = ids_.size();
        bounds_want_.resize(n * 6);
        for (size_t i = 0; i < n; ++i) std::memcpy(&bounds_want_[6 * i], kNoBounds, 24);
        for (const auto& kv : bounds_) {
            auto it = index_of_.find(kv.first);
            if (it != index_of_.end()) std::memcpy(&bounds_want_[6 * static_cast<size_t>(it->second)], kv.second.v, 24);
        }
        const size_t had = bounds_sent_.size() / 6;
        bounds_sent_.resize(n * 6);
        for (size_t i = had; i < n; ++i) std::memcpy(&bounds_sent_[6 * i], kNoBounds, 24); // (a new index has none on the device either)
        index_list_.clear();
        stage_.clear();
        repack_.clear();
        for (size_t i = 0; i < n; ++i) {
            if (std::memcmp(&bounds_want_[6 * i], &bounds_sent_[6 * i], 24) == 0) continue;
            index_list_.push_back(static_cast<uint32_t>(i));
            stage_.insert(stage_.end(), &bounds_want_[6 * i], &bounds_want_[6 * i] + 3);
            repack_.insert(repack_.end(), &bounds_want_[6 * i] + 3, &bounds_want_[6 * i] + 6);
        }
        if (!index_list_.empty() &&
            bge_world_upload_bounds_indexed(world_, index_list_.size(), index_list_.data(), stage_.data(), repack_.data()) != BGE_OK) {
            return Log("bge_world_upload_bounds_indexed");
        }
        bounds_sent_.swap(bounds_want_);
        bounds_stale_ = false;
        return true;
    }

    // the same for the draw keys
    bool UploadDrawKeys()
    {
        if (!draw_keys_stale_) return true;
        const size_t n = ids_.size();
        draw_keys_want_.assign(n, BGE_NO_DRAW_KEY);
        for (const auto& kv : draw_keys_) {
            auto it = index_of_.find(kv.first);
            if (it != index_of_.end()) draw_keys_want_[it->second] = kv.second;
        }
        draw_keys_sent_.resize(n, BGE_NO_DRAW_KEY); // (a new index has none on the device either)
        index_list_.clear();
        draw_keys_stage_.clear();
        for (size_t i = 0; i < n; ++i) {
            if (draw_keys_want_[i] == draw_keys_sent_[i]) continue;
            index_list_.push_back(static_cast<uint32_t>(i));
            draw_keys_stage_.push_back(draw_keys_want_[i]);
        }
        if (!index_list_.empty() &&
            bge_world_upload_draw_keys_indexed(world_, index_list_.size(), index_list_.data(), draw_keys_stage_.data()) != BGE_OK) {
            return Log("bge_world_upload_draw_keys_indexed");
        }
        draw_keys_sent_.swap(draw_keys_want_);
        draw_keys_stale_ = false;
        return true;
    }

    bool Log(const char* what) const
    {
        std::fprintf(stderr, "[GPU] %s failed: %s\n", what, bge_last_error());
        return false;
    }

    // Stable dense indices: an entity keeps its index while it owns a Transform; freed indices are reused.
    bool RefreshTopology(SceneT& scene)
    {
        auto& transforms = scene.GetTransforms();
        bool changed = transforms.size() != live_ || topology_stale_;
        topology_stale_ = false;
        if (!changed) {
            for (auto& kv : transforms) {
                auto it = index_of_.find(kv.first);
                if (it == index_of_.end() || parent_[it->second] != ParentIndex(scene, kv.first)) {
                    changed = true;
                    break;
                }
            }
        }
        if (!changed) return true;

        // drop entities that lost their Transform; remember which index each id had, because the reference reuses
        // EntityIds (Scene.cpp:24-27) and everything keyed by id there (e.g. a trigger's remembered overlaps) is keyed
        // by index here: a re-created id gets its old index back
        for (auto it = index_of_.begin(); it != index_of_.end();) {
            if (!scene.HasTransform(it->first)) {
                has_tf_[it->second] = 0;
                const bool body_lives_on = body_[it->second].exists && scene.GetRigidBody(it->first) && scene.GetCollider(it->first);
                const bool ghost_lives_on = has_trigger_[it->second] && scene.GetTriggerVolume(it->first);
                if (!body_lives_on && body_[it->second].exists) {
                    gone_bodies_.push_back(it->second); // (its components went with the Transform)
                    body_[it->second] = BodyState{};
                }
                if (body_lives_on || ghost_lives_on) {
                    // The entity lost its Transform but keeps its body components: the reference keeps stepping the Bullet body
                    // (EnsureRigidBody returns before it looks at the runtime, PhysicsSystem.cpp:389-393), and a trigger ghost stays where
                    // it was (EnsureTrigger returns early too).  The index stays the entity's — the world keeps body and ghost on
                    // it — until the components go (UploadBodies / UploadTriggers) or the Transform returns.
                    orphan_of_[it->first] = it->second;
                } else {
                    // (the world keeps the body of an index that merely loses its Transform: one whose components went too —
                    //  a destroyed entity — is taken out explicitly, while its slot still exists)
                    if (body_[it->second].exists) gone_bodies_.push_back(it->second);
                    ids_[it->second] = 0;
                    has_trigger_[it->second] = 0;
                    body_[it->second] = BodyState{};
                    free_.push_back(it->second);
                    is_free_[it->second] = 1;
                    retired_[it->first] = it->second;
                }
                it = index_of_.erase(it);
            } else {
                ++it;
            }
        }
        if (!gone_bodies_.empty()) {
            const std::vector<uint8_t> none(gone_bodies_.size(), BGE_BODY_NONE);
            if (bge_world_upload_bodies_indexed(world_, gone_bodies_.size(), gone_bodies_.data(), none.data(), nullptr, nullptr, nullptr, nullptr,
                                                nullptr) != BGE_OK) {
                return Log("bge_world_upload_bodies_indexed (bodies of entities that are gone)");
            }
            gone_bodies_.clear();
        }
        // first the ids that come back, so that nobody else takes their index
        for (auto& kv : transforms) {
            if (index_of_.count(kv.first)) continue;
            auto o = orphan_of_.find(kv.first);
            if (o != orphan_of_.end()) { // the Transform returns to a body that lived on without one: same index, body state kept
                const uint32_t i = o->second;
                has_tf_[i] = 1;
                written_[i] = 0;
                index_of_[kv.first] = i;
                orphan_of_.erase(o);
                continue;
            }
            auto r = retired_.find(kv.first);
            if (r == retired_.end() || !is_free_[r->second]) continue;
            const uint32_t i = r->second;
            is_free_[i] = 0;
            ids_[i] = kv.first;
            last_ids_[i] = kv.first;
            has_tf_[i] = 1;
            written_[i] = 0;
            index_of_[kv.first] = i;
            fresh_.push_back(i);
        }
        // New entities take their indices in ASCENDING ENTITY ID (the store is an unordered_map): where the device orders entities — the
        // lowest four obstacles of a body, body A of a pair of Dynamic boxes, the bodies and manifolds of a simulation island — it
        // orders by index, the oracle by entity id; for entities that first appear together (a loaded scene) the two agree.  A reused
        // index (free list) can break the agreement: results stay deterministic, the solver's row order is then another one.
        new_ids_.clear();
        for (auto& kv : transforms) {
            if (!index_of_.count(kv.first)) new_ids_.push_back(kv.first);
        }
        std::sort(new_ids_.begin(), new_ids_.end());
        for (const Id new_id : new_ids_) {
            struct { Id first; } kv{new_id};
            uint32_t i;
            while (!free_.empty() && !is_free_[free_.back()]) free_.pop_back(); // taken back above
            if (!free_.empty()) {
                i = free_.back();
                free_.pop_back();
                is_free_[i] = 0;
            } else {
                i = static_cast<uint32_t>(ids_.size());
                ids_.push_back(0);
                last_ids_.push_back(0);
                has_tf_.push_back(0);
                parent_.push_back(BGE_NO_PARENT);
                body_.emplace_back();
                is_free_.push_back(0);
                has_trigger_.push_back(0);
                written_.push_back(0);
                last_pose_.resize(last_pose_.size() + 6, 0.0f);
                last_scale_.resize(last_scale_.size() + 3, 0.0f);
            }
            ids_[i] = kv.first;
            last_ids_[i] = kv.first; // survives the entity: an Exit event may name a body that was destroyed
            has_tf_[i] = 1;
            written_[i] = 0;
            index_of_[kv.first] = i;
            fresh_.push_back(i);
        }
        for (auto& kv : transforms) parent_[index_of_[kv.first]] = ParentIndex(scene, kv.first);
        // (an index whose entity lost its Transform keeps the parent it had: to the device that entity's place in the
        //  hierarchy has not changed, so nothing below it is taken for re-parented)
        live_ = transforms.size();
        bounds_stale_ = true; // an entity may sit on another index now
        draw_keys_stale_ = true;
        if (bge_world_set_topology(world_, ids_.size(), parent_.data(), has_tf_.data()) != BGE_OK) return Log("bge_world_set_topology");
        // the device has just cleared the per-index rows from ids_.size() on: what was "last sent" beyond it is gone as well, so a
        // later regrowth sends those rows again even when no upload ran in between
        if (bounds_sent_.size() > ids_.size() * 6) bounds_sent_.resize(ids_.size() * 6);
        if (draw_keys_sent_.size() > ids_.size()) draw_keys_sent_.resize(ids_.size());
        // a reused index must not inherit the previous owner's device state: force a full upload
        for (uint32_t i : fresh_) {
            if (auto* t = scene.GetTransform(ids_[i])) t->dirty = true;
        }
        fresh_.clear();
        return true;
    }

    // An index kept for an entity without a Transform (its body and / or its trigger ghost live on) is given up when neither is left.
    void RetireIfNothingLeft(uint32_t i)
    {
        if (has_tf_[i] || ids_[i] == 0 || body_[i].exists || has_trigger_[i]) return;
        orphan_of_.erase(ids_[i]);
        retired_[ids_[i]] = i;
        ids_[i] = 0;
        free_.push_back(i);
        is_free_[i] = 1;
        topology_stale_ = true;
    }

    uint32_t ParentIndex(SceneT& scene, Id id)
    {
        const Id p = scene.GetParent(id);
        if (p == 0) return BGE_NO_PARENT;
        if (!scene.HasTransform(p)) {
            // The child is a root (Scene.cpp:528).  If the parent entity owned a Transform before, the device is told the SAME
            // parent index (has_transform = 0 there) for as long as nobody else has taken it: bge_world_set_topology then sees
            // an unchanged parent entity that lost its Transform — it neither marks the child dirty nor recomputes its world
            // matrix, as the reference does not (Scene::RemoveTransform marks nobody) — instead of a changed parent.
            auto o = orphan_of_.find(p);
            if (o != orphan_of_.end()) return o->second; // (its body still holds the index)
            auto r = retired_.find(p);
            return (r != retired_.end() && is_free_[r->second]) ? r->second : BGE_NO_PARENT;
        }
        auto it = index_of_.find(p);
        return it == index_of_.end() ? 0xfffffffeu /* not indexed yet: forces a refresh */ : it->second;
    }

    bool UploadDirtyTransforms(SceneT& scene)
    {
        index_list_.clear();
        stage_.clear();
        for (auto& kv : scene.GetTransforms()) {
            auto& t = kv.second;
            if (!t.dirty) continue;
            const uint32_t i = index_of_[kv.first];
            if (written_[i] && std::memcmp(&t.position, &last_pose_[6 * static_cast<size_t>(i)], 12) == 0 &&
                std::memcmp(&t.rotationEuler, &last_pose_[6 * static_cast<size_t>(i) + 3], 12) == 0 &&
                std::memcmp(&t.scale, &last_scale_[3 * static_cast<size_t>(i)], 12) == 0) {
                continue; // dirty only because the physics write-back marked it: the device already has these values
            }
            // (the scale is compared too: a scale edit + MarkDirty between PhysicsSystem::Update and
            //  TransformSystem::Update must reach the device — the reference recomputes `local` from it in that frame)
            std::memcpy(&last_scale_[3 * static_cast<size_t>(i)], &t.scale, 12);
            index_list_.push_back(i);
            const float* p = &t.position.x;
            stage_.insert(stage_.end(), p, p + 9); // position, rotationEuler, scale are contiguous (Transform.h:14-16)
        }
        const size_t m = index_list_.size();
        if (!m) return true;
        // repack [pos|euler|scale] rows into three arrays
        repack_.resize(m * 9);
        for (size_t k = 0; k < m; ++k) {
            std::memcpy(&repack_[3 * k], &stage_[9 * k], 12);
            std::memcpy(&repack_[3 * m + 3 * k], &stage_[9 * k + 3], 12);
            std::memcpy(&repack_[6 * m + 3 * k], &stage_[9 * k + 6], 12);
        }
        if (bge_world_upload_trs_indexed(world_, m, index_list_.data(), repack_.data(), repack_.data() + 3 * m,
                                         repack_.data() + 6 * m) != BGE_OK) {
            return Log("bge_world_upload_trs_indexed");
        }
        for (uint32_t i : index_list_) written_[i] = 0;
        return true;
    }

    // EnsureRigidBody / prune loops (PhysicsSystem.cpp:1222-1260, 382-499): a body exists where RigidBody, Collider
    // and Transform all do; it is (re)created when RigidBody.dirty or Collider.dirty is set.
    bool UploadBodies(SceneT& scene)
    {
        index_list_.clear();
        b_type_.clear(); b_mass_.clear(); b_shape_.clear(); b_size_.clear(); b_layer_.clear(); b_mask_.clear(); b_friction_.clear(); b_restitution_.clear();
        seen_.assign(ids_.size(), 0);
        for (auto& kv : scene.GetRigidBodies()) {
            auto it = index_of_.find(kv.first);
            auto* col = scene.GetCollider(kv.first);
            if (it == index_of_.end()) {
                // no Transform: nothing is (re)created (its dirty flags wait); a body that lives on without one stays as it is
                auto o = orphan_of_.find(kv.first);
                if (o != orphan_of_.end() && col) seen_[o->second] = 1;
                continue;
            }
            if (!col) continue;
            const uint32_t i = it->second;
            seen_[i] = 1;
            auto& rb = kv.second;
            if (body_[i].exists && !rb.dirty && !col->dirty) continue;
            index_list_.push_back(i);
            b_type_.push_back(static_cast<uint8_t>(static_cast<int>(rb.type)));
            b_mass_.push_back(rb.mass);
            b_shape_.push_back(static_cast<uint8_t>(static_cast<int>(col->shape)));
            b_size_.push_back(col->size.x); b_size_.push_back(col->size.y); b_size_.push_back(col->size.z);
            b_layer_.push_back(rb.layer);
            b_mask_.push_back(rb.mask);
            b_friction_.push_back(rb.friction); // info.m_friction = body.friction (PhysicsSystem.cpp:437)
            b_restitution_.push_back(rb.restitution); // info.m_restitution = body.restitution (:438)
            body_[i].exists = true;
            rb.dirty = false;   // PhysicsSystem.cpp:476
            col->dirty = false; // PhysicsSystem.cpp:403
        }
        for (uint32_t i = 0; i < ids_.size(); ++i) {
            if (body_[i].exists && !seen_[i]) { // component removed: RemoveRigidBody (PhysicsSystem.cpp:1230-1233)
                index_list_.push_back(i);
                b_type_.push_back(BGE_BODY_NONE);
                b_mass_.push_back(0.0f);
                b_shape_.push_back(0);
                b_size_.insert(b_size_.end(), {0.5f, 0.5f, 0.5f});
                b_layer_.push_back(1);
                b_mask_.push_back(0xffffffffu);
                b_friction_.push_back(0.5f);
                b_restitution_.push_back(0.0f);
                body_[i].exists = false;
                RetireIfNothingLeft(i);
            }
        }
        if (index_list_.empty()) return true;
        if (bge_world_upload_bodies_indexed(world_, index_list_.size(), index_list_.data(), b_type_.data(), b_mass_.data(),
                                            b_shape_.data(), b_size_.data(), b_layer_.data(), b_mask_.data()) != BGE_OK) {
            return Log("bge_world_upload_bodies_indexed");
        }
        if (bge_world_upload_friction_indexed(world_, index_list_.size(), index_list_.data(), b_friction_.data()) != BGE_OK) {
            return Log("bge_world_upload_friction_indexed");
        }
        if (bge_world_upload_restitution_indexed(world_, index_list_.size(), index_list_.data(), b_restitution_.data()) != BGE_OK) {
            return Log("bge_world_upload_restitution_indexed");
        }
        return true;
    }

    bge_world* world_ = nullptr;
    std::vector<Id> ids_;                       // dense index -> EntityId (0 = free)
    std::vector<Id> last_ids_;                  // dense index -> the id it last belonged to
    std::unordered_map<Id, uint32_t> index_of_;
    std::vector<uint32_t> parent_, free_, fresh_, index_list_, gone_bodies_;
    std::vector<Id> new_ids_;
    std::vector<uint8_t> has_tf_, written_, limbo_, seen_, is_free_, has_trigger_, seen_trigger_;
    std::unordered_map<Id, uint32_t> retired_;  // last index of ids that lost their Transform
    std::unordered_map<Id, uint32_t> orphan_of_; // ids without a Transform whose body lives on, on the index they had
    bool topology_stale_ = false;               // an index was given up outside RefreshTopology
    std::vector<BodyState> body_;
    std::unordered_map<Id, Bounds> bounds_;     // what SetBounds was given, per EntityId
    std::vector<float> bounds_want_, bounds_sent_; // per dense index: the row the device should hold / was last sent
    bool bounds_stale_ = false;
    std::unordered_map<Id, uint32_t> draw_keys_; // what SetDrawKey was given, per EntityId
    std::vector<uint32_t> draw_keys_want_, draw_keys_sent_, draw_keys_stage_; // per dense index: wanted / last sent; the rows that travel
    bool draw_keys_stale_ = false;
    std::vector<float> last_pose_;              // position + euler the physics write-back stored (6 floats per index)
    std::vector<float> last_scale_;             // scale as last uploaded (3 floats per index)
    std::vector<float> stage_, repack_;
    // Destination of the downloads: page-locked (bge_host_alloc), so the copies run at the PCIe rate instead of the
    // pageable ~10 GB/s; grow-only.
    struct PinnedFloats {
        float* p = nullptr;
        size_t cap = 0;
        ~PinnedFloats() { bge_host_free(p); }
        PinnedFloats() = default;
        PinnedFloats(const PinnedFloats&) = delete;
        PinnedFloats& operator=(const PinnedFloats&) = delete;
        float* resize(size_t n)
        {
            if (n > cap) {
                bge_host_free(p);
                p = nullptr;
                cap = 0;
                void* q = nullptr;
                const size_t want = n + n / 4;
                if (bge_host_alloc(want * sizeof(float), &q) == BGE_OK) {
                    p = static_cast<float*>(q);
                    cap = want;
                }
            }
            return p;
        }
        float& operator[](size_t i) { return p[i]; }
        float* data() { return p; }
    } down_;
    std::vector<uint8_t> b_type_, b_shape_;
    std::vector<float> b_mass_, b_size_, b_friction_, b_restitution_;
    std::vector<uint32_t> b_layer_, b_mask_;
    size_t live_ = 0;
    std::vector<uint32_t> t_entity_, t_layer_, t_mask_, t_signature_;
    std::vector<uint8_t> t_shape_, t_oneshot_, t_active_;
    std::vector<float> t_size_;
    std::vector<uint32_t> t_order_; // EntityIds of the scene's TriggerVolumes, ascending
    std::vector<bge_trigger_event> raw_events_;
    std::vector<GpuTriggerEvent> trigger_events_;
    std::vector<bge_ray_hit> ray_hits_;
    std::vector<bge_overlap_hit> overlap_hits_;
    std::vector<bge_sphere_move> moves_;
    std::vector<bge_sphere_move_result> move_results_;
    std::vector<bge_sphere_step_move> step_moves_;
    std::vector<bge_sphere_step_result> step_results_;
    std::vector<bge_sphere_recover> recovers_;
    std::vector<bge_sphere_recover_result> recover_results_;
    // characters: the set in the order it was added; the descs and inputs as the device should hold them, the states as last synced
    std::vector<Id> char_ids_;
    std::unordered_map<Id, uint32_t> char_index_;
    std::vector<bge_character_desc> char_descs_;
    std::vector<bge_character_input> char_inputs_;
    std::vector<bge_character_state> char_states_;
    bool chars_stale_ = false, char_inputs_stale_ = false;
    // character trigger events: wanted, on on the device, an UpdateCharacters' list waits for SyncCharacters
    bool char_trig_on_ = false, char_trig_watching_ = false, char_trig_pending_ = false;
    std::vector<uint32_t> char_overlaps_; // (trigger entity, character) pairs carried over a re-creation of the set
    std::vector<bge_character_trigger_event> raw_char_events_;
    std::vector<GpuTriggerEvent> char_trigger_events_;
    // character platform riding: the flags wanted, the flags the device has, the records as last synced
    uint32_t char_ride_want_ = 0u, char_ride_applied_ = 0u;
    std::vector<bge_character_ride> char_rides_;
    bool char_crowd_want_ = false, char_crowd_applied_ = false;
    float char_crowd_max_push_ = 0.0f, char_crowd_applied_push_ = 0.0f;
    std::vector<bge_crowd_hit> char_crowd_hits_;
    // character push: the desc wanted and the desc the device has (all zeros = off)
    bge_character_push_desc char_push_want_{0u, 0.0f, 0.0f, 0u}, char_push_applied_{0u, 0.0f, 0.0f, 0u};
    // impulses queued since the last UpdatePhysics, in call order, and whom they are for
    std::vector<Id> impulse_ids_;
    std::vector<bge_impulse> impulses_;

    // the queue as one batch; an entity the mirror does not know gets BGE_RAY_NO_ENTITY, which no world carries
    bool FlushImpulses()
    {
        if (impulses_.empty()) return true;
        if (ids_.empty()) { // (an empty scene has no world to apply them to)
            impulses_.clear();
            impulse_ids_.clear();
            return true;
        }
        for (size_t k = 0; k < impulses_.size(); ++k) {
            auto it = index_of_.find(impulse_ids_[k]);
            impulses_[k].entity = it == index_of_.end() ? BGE_RAY_NO_ENTITY : it->second;
        }
        const int rc = bge_world_apply_impulses(world_, impulses_.size(), impulses_.data(), nullptr);
        impulses_.clear();
        impulse_ids_.clear();
        return rc == BGE_OK || Log("bge_world_apply_impulses");
    }

    template <class Vec3> static bge_sphere_cast MakeCast(const Vec3& o, const Vec3& d, float maxDistance, float radius, uint32_t layerMask)
    {
        bge_sphere_cast c{};
        c.origin[0] = o.x, c.origin[1] = o.y, c.origin[2] = o.z;
        c.direction[0] = d.x, c.direction[1] = d.y, c.direction[2] = d.z;
        c.max_distance = maxDistance;
        c.radius = radius;
        c.layer_mask = layerMask;
        return c;
    }
    template <class Vec3> static bge_ray MakeRay(const Vec3& o, const Vec3& d, float maxDistance, uint32_t layerMask)
    {
        bge_ray r{};
        r.origin[0] = o.x;
        r.origin[1] = o.y;
        r.origin[2] = o.z;
        r.direction[0] = d.x;
        r.direction[1] = d.y;
        r.direction[2] = d.z;
        r.max_distance = maxDistance;
        r.layer_mask = layerMask;
        return r;
    }
    // entity index -> EntityId through the mirror's map; the plane (the reference's Ground object) has no entity: kInvalidEntity (0)
    template <class HitT> void FillHit(const bge_ray_hit& h, HitT& out) const
    {
        const bool has = h.entity != BGE_RAY_NO_ENTITY && h.entity < ids_.size();
        out.entity = static_cast<decltype(out.entity)>(has ? ids_[h.entity] : Id{0});
        out.point.x = h.point[0];
        out.point.y = h.point[1];
        out.point.z = h.point[2];
        out.normal.x = h.normal[0];
        out.normal.y = h.normal[1];
        out.normal.z = h.normal[2];
        out.distance = h.distance;
    }
};

// One mirror per Scene object, found by address (TransformSystem::Update is a static function without state,
// src/ecs/TransformSystem.h:5-9).  OnSceneReloaded drops it (the reference move-assigns the whole Scene on
// reload, src/scene/SceneLoader.cpp:742).
template <class SceneT> class GpuMirrors {
public:
    static GpuSceneMirror<SceneT>& Of(SceneT& scene)
    {
        auto& slot = Table()[&scene];
        if (!slot) slot = std::make_unique<GpuSceneMirror<SceneT>>();
        return *slot;
    }
    static void Drop(SceneT& scene) { Table().erase(&scene); }

private:
    static std::unordered_map<const void*, std::unique_ptr<GpuSceneMirror<SceneT>>>& Table()
    {
        static std::unordered_map<const void*, std::unique_ptr<GpuSceneMirror<SceneT>>> t;
        return t;
    }
};

template <class SceneT> class GpuTransformSystem {
public:
    static void Update(SceneT& scene) { GpuMirrors<SceneT>::Of(scene).UpdateTransforms(scene); }
};

template <class SceneT> class GpuPhysicsSystem {
public:
    // ---- PhysicsSystem's public surface for this path (src/physics/PhysicsSystem.h:43-48, 77)
    void SetConfigPath(std::filesystem::path path)
    {
        configPath_ = std::move(path);
        hasLastWriteTime_ = false;
    }
    // EnsureWorld (PhysicsSystem.cpp:108-120): the device world of a scene is created on its first Update; here the
    // GPU is probed once so that a missing device is reported at start-up, as a failed Bullet set-up would be
    void Initialize()
    {
        GpuSceneMirror<SceneT> probe;
        if (!probe.ok()) std::fprintf(stderr, "[GPU] Initialize: no usable device — %s\n", bge_last_error());
    }
    void OnSceneReloaded(SceneT& scene) // the mirror (and its clock) is rebuilt by the next Update
    {
        GpuMirrors<SceneT>::Drop(scene);
        if (lastScene_ == &scene) lastScene_ = nullptr;
    }
    // mtime poll of the config file, every frame (PhysicsSystem.cpp:216-240)
    bool ReloadConfigIfNeeded(SceneT& scene)
    {
        if (configPath_.empty()) return false;
        std::error_code ec;
        const auto currentTime = std::filesystem::last_write_time(configPath_, ec);
        if (ec) return false;
        if (!hasLastWriteTime_ || currentTime != lastWriteTime_) {
            lastWriteTime_ = currentTime;
            hasLastWriteTime_ = true;
            config_ = LoadConfigFromDisk();
            (void)scene; // ApplyConfig's scene work is the character controllers' (out of scope); gravity reaches the world on the next Update
            return true;
        }
        return false;
    }
    // rigid-body slice of PhysicsSystem::Update(Scene&, const Camera&, const InputSystem&, double) (PhysicsSystem.cpp:1208-1328);
    // camera and input feed the character controller, which is not part of this path
    template <class CameraT, class InputT> void Update(SceneT& scene, const CameraT&, const InputT&, double dt) { Step(scene, dt); }
    void Update(SceneT& scene, double dt) { Step(scene, dt); }
    // PhysicsSystem.cpp:1330-1341
    void LogStats() const
    {
        std::printf("[Physics] bodies=%d characters=%zu stepTime=%.4fms substeps=%d fixedStep=%.4f actualDt=%.4f\n", lastBodies_,
                    lastScene_ ? GpuMirrors<SceneT>::Of(*lastScene_).CharacterCount() : static_cast<size_t>(0), lastStepDurationMs_, lastStepSubsteps_, config_.fixedStep, lastStepDt_);
    }
    double GetFixedStep() const { return config_.fixedStep; }

    // ---- additions
    void SetGravity(float g) { config_.gravity = g; }
    // Bullet's own orientation scheme for every Dynamic body (include/bge_world.h, BGE_TICK_BULLET_BASIS); choose before
    // the first Update of a scene
    void SetBulletBasis(bool on) { bulletBasis_ = on; }
    // the static ground plane every reference world has (on by default); off = free bodies
    void SetGroundPlane(bool on) { groundPlane_ = on; }
    int LastSubSteps() const { return lastStepSubsteps_; }
    // trigger events of the last Update (publish them on the engine's EventBus, src/core/EventBus.h)
    const std::vector<GpuTriggerEvent>& TriggerEvents(SceneT& scene) const { return GpuMirrors<SceneT>::Of(scene).TriggerEvents(); }

    // PhysicsSystem::Raycast / RaycastAll (src/physics/PhysicsSystem.h:66-75): the world of the scene of the last Update, as that
    // Update left it — call after Update and before the next one uploads new poses, as Application::Update does
    // (src/core/Application.cpp:256-281).  false / empty before the first Update, as the reference without m_world.
    template <class Vec3, class HitT>
    bool Raycast(const Vec3& origin, const Vec3& direction, float maxDistance, uint32_t layerMask, HitT& outHit) const
    {
        return lastScene_ && GpuMirrors<SceneT>::Of(*lastScene_).Raycast(origin, direction, maxDistance, layerMask, outHit);
    }
    template <class HitT, class Vec3>
    std::vector<HitT> RaycastAll(const Vec3& origin, const Vec3& direction, float maxDistance, uint32_t layerMask) const
    {
        if (!lastScene_) return {};
        return GpuMirrors<SceneT>::Of(*lastScene_).template RaycastAll<HitT>(origin, direction, maxDistance, layerMask);
    }

    // EXTENSIONS, not in the reference's PhysicsSystem: sphere casts and a sphere overlap against the same world, under the same
    // call order as Raycast (include/bge_world.h "Sphere queries"); false / empty before the first Update.
    template <class Vec3, class HitT>
    bool SphereCast(const Vec3& origin, const Vec3& direction, float maxDistance, float radius, uint32_t layerMask, HitT& outHit) const
    {
        return lastScene_ && GpuMirrors<SceneT>::Of(*lastScene_).SphereCast(origin, direction, maxDistance, radius, layerMask, outHit);
    }
    template <class HitT, class Vec3>
    std::vector<HitT> SphereCastAll(const Vec3& origin, const Vec3& direction, float maxDistance, float radius, uint32_t layerMask) const
    {
        if (!lastScene_) return {};
        return GpuMirrors<SceneT>::Of(*lastScene_).template SphereCastAll<HitT>(origin, direction, maxDistance, radius, layerMask);
    }
    template <class Vec3> std::vector<GpuOverlapHit> OverlapSphere(const Vec3& center, float radius, uint32_t layerMask) const
    {
        if (!lastScene_) return {};
        return GpuMirrors<SceneT>::Of(*lastScene_).OverlapSphere(center, radius, layerMask);
    }

    // EXTENSION: collide-and-slide moves of spheres against the same world, under the same call order as Raycast
    // (include/bge_world.h "Sphere moves"); false before the first Update, with every position echoed.
    template <class Vec3>
    bool MoveSphere(const Vec3& position, const Vec3& displacement, float radius, float skin, float probeDistance, float maxSlopeRad,
                    uint32_t layerMask, GpuSphereMoveResult<Vec3>& result) const
    {
        if (!lastScene_) {
            result = GpuSphereMoveResult<Vec3>{};
            result.position = position;
            return false;
        }
        return GpuMirrors<SceneT>::Of(*lastScene_).MoveSphere(position, displacement, radius, skin, probeDistance, maxSlopeRad, layerMask, result);
    }
    template <class Vec3> bool MoveSpheres(const std::vector<GpuSphereMover<Vec3>>& movers, std::vector<GpuSphereMoveResult<Vec3>>& results) const
    {
        if (!lastScene_) {
            results.assign(movers.size(), GpuSphereMoveResult<Vec3>{});
            for (size_t i = 0; i < movers.size(); ++i) results[i].position = movers[i].position;
            return false;
        }
        return GpuMirrors<SceneT>::Of(*lastScene_).MoveSpheres(movers, results);
    }

    // EXTENSION: the same moves, stepping up over low obstacles (include/bge_world.h "Sphere step moves"); false before the first
    // Update, with every position echoed.
    template <class Vec3>
    bool StepMoveSphere(const Vec3& position, const Vec3& displacement, float radius, float skin, float probeDistance, float maxSlopeRad,
                        uint32_t layerMask, float stepHeight, GpuSphereStepResult<Vec3>& result) const
    {
        if (!lastScene_) {
            result = GpuSphereStepResult<Vec3>{};
            result.position = position;
            return false;
        }
        return GpuMirrors<SceneT>::Of(*lastScene_).StepMoveSphere(position, displacement, radius, skin, probeDistance, maxSlopeRad, layerMask,
                                                                  stepHeight, result);
    }
    template <class Vec3>
    bool StepMoveSpheres(const std::vector<GpuSphereStepMover<Vec3>>& movers, std::vector<GpuSphereStepResult<Vec3>>& results) const
    {
        if (!lastScene_) {
            results.assign(movers.size(), GpuSphereStepResult<Vec3>{});
            for (size_t i = 0; i < movers.size(); ++i) results[i].position = movers[i].position;
            return false;
        }
        return GpuMirrors<SceneT>::Of(*lastScene_).StepMoveSpheres(movers, results);
    }

    // EXTENSION: sphere penetration and recovery against the same world, under the same call order as Raycast
    // (include/bge_world.h "Sphere penetration and recovery"); false before the first Update, with every position echoed.
    template <class Vec3> bool SpherePenetration(const Vec3& center, float radius, uint32_t layerMask, GpuPenetrationHit<Vec3>& outHit) const
    {
        return lastScene_ && GpuMirrors<SceneT>::Of(*lastScene_).SpherePenetration(center, radius, layerMask, outHit);
    }
    template <class Vec3>
    bool RecoverSphere(const Vec3& position, float radius, float skin, uint32_t layerMask, GpuSphereRecoverResult<Vec3>& result) const
    {
        if (!lastScene_) {
            result = GpuSphereRecoverResult<Vec3>{};
            result.position = position;
            return false;
        }
        return GpuMirrors<SceneT>::Of(*lastScene_).RecoverSphere(position, radius, skin, layerMask, result);
    }
    template <class Vec3>
    bool RecoverSpheres(const std::vector<GpuSphereRecover<Vec3>>& spheres, std::vector<GpuSphereRecoverResult<Vec3>>& results) const
    {
        if (!lastScene_) {
            results.assign(spheres.size(), GpuSphereRecoverResult<Vec3>{});
            for (size_t i = 0; i < spheres.size(); ++i) results[i].position = spheres[i].position;
            return false;
        }
        return GpuMirrors<SceneT>::Of(*lastScene_).RecoverSpheres(spheres, results);
    }

    // EXTENSION: sphere characters on the device (include/bge_world.h "Characters") in the place of the reference's
    // btKinematicCharacterController (PhysicsSystem.cpp:709-846).  The surface follows the reference's use of Bullet's controller;
    // the shape is a sphere of the capsule's radius, and capsules are not done; pushing Dynamic bodies and riding platforms are
    // opt-in (SetCharacterPush, SetCharacterPlatformRiding below).
    // Per frame, after Update: SetCharacterWalk / CharacterJump from the input, UpdateCharacters(fixed step, the Update's
    // sub-steps), SyncCharacters.  They act on the scene of the last Update and return false before it.
    // AddCharacter: the position is the entity's Transform's; radius, step height, max slope, jump speed and gravity are the
    // Config's, as EnsureCharacter takes them (:735-760); the fall speed is |gravity| * 3 (:761).  The ground probe reaches 0.1 below the
    // character: a descending character within that of walkable ground is put on it, so a longer probe would end a jump early.
    bool AddCharacter(typename GpuSceneMirror<SceneT>::Id entity)
    {
        if (!lastScene_) return false;
        GpuCharacterKnobs k;
        k.radius = config_.capsuleRadius;
        k.stepHeight = std::max(config_.stepHeight, 0.0f);
        k.maxSlopeRad = config_.maxSlopeDeg * 0.017453292f;
        k.probeDistance = 0.1f;
        k.gravity = std::max(-config_.gravity, 0.0f);
        k.jumpSpeed = std::max(config_.jumpImpulse, 0.0f);
        k.fallSpeed = std::max(std::fabs(config_.gravity) * 3.0f, 1.0f);
        return GpuMirrors<SceneT>::Of(*lastScene_).AddCharacter(*lastScene_, entity, k);
    }
    void RemoveCharacters()
    {
        if (lastScene_) GpuMirrors<SceneT>::Of(*lastScene_).RemoveCharacters();
    }
    // the level displacement of one step: what setWalkDirection takes (:827)
    bool SetCharacterWalk(typename GpuSceneMirror<SceneT>::Id entity, float dx, float dz)
    {
        return lastScene_ && GpuMirrors<SceneT>::Of(*lastScene_).SetCharacterWalk(entity, dx, dz);
    }
    // jump.pressed (:834): sets the edge; "only on the ground" (:840) is applied on the device
    bool CharacterJump(typename GpuSceneMirror<SceneT>::Id entity) { return lastScene_ && GpuMirrors<SceneT>::Of(*lastScene_).CharacterJump(entity); }
    template <class Vec3> bool WarpCharacter(typename GpuSceneMirror<SceneT>::Id entity, const Vec3& position)
    {
        return lastScene_ && GpuMirrors<SceneT>::Of(*lastScene_).WarpCharacter(entity, position);
    }
    bool UpdateCharacters(float dt, uint32_t steps)
    {
        if (!lastScene_) return false;
        GpuMirrors<SceneT>::Of(*lastScene_).SetCharacterTriggerEvents(characterTriggerEvents_);
        GpuMirrors<SceneT>::Of(*lastScene_).SetCharacterPlatformRiding(characterRiding_, characterRidingDynamic_);
        GpuMirrors<SceneT>::Of(*lastScene_).SetCharacterCrowd(characterCrowd_, characterCrowdMaxPush_);
        GpuMirrors<SceneT>::Of(*lastScene_).SetCharacterPush(characterPush_, characterPushForce_, characterPushMaxNormalY_);
        return GpuMirrors<SceneT>::Of(*lastScene_).UpdateCharacters(dt, steps);
    }
    bool SyncCharacters(SceneT& scene) { return GpuMirrors<SceneT>::Of(scene).SyncCharacters(scene); }
    // EXTENSION: Enter / Stay / Exit of the characters against the trigger volumes (include/bge_world.h "Character trigger
    // events"), off by default.  UpdateCharacters makes the list on the device, SyncCharacters fetches it and switches off a one-shot
    // volume that a character Entered; `other` of an event is the character's EntityId.  TriggerEvents() stays as it is.
    void SetCharacterTriggerEvents(bool on)
    {
        characterTriggerEvents_ = on;
        if (lastScene_) GpuMirrors<SceneT>::Of(*lastScene_).SetCharacterTriggerEvents(on);
    }
    const std::vector<GpuTriggerEvent>& CharacterTriggerEvents() const
    {
        static const std::vector<GpuTriggerEvent> none;
        return lastScene_ ? GpuMirrors<SceneT>::Of(*lastScene_).CharacterTriggerEvents() : none;
    }
    // EXTENSION: characters ride moving platforms (include/bge_world.h "Character platform riding"), off by default.  With it on,
    // a character that stands on a Static or Kinematic body (with dynamicBodies on a Dynamic one too) is moved with that body at the
    // start of every UpdateCharacters; a game that moves platforms through their Transforms need not keep Bullet for that.  The
    // carry is a teleport (no sweep) and leaves no velocity behind when the character steps off.
    void SetCharacterPlatformRiding(bool on, bool dynamicBodies = false)
    {
        characterRiding_ = on;
        characterRidingDynamic_ = on && dynamicBodies;
        if (lastScene_) GpuMirrors<SceneT>::Of(*lastScene_).SetCharacterPlatformRiding(characterRiding_, characterRidingDynamic_);
    }
    // what the last UpdateCharacters' carry did and the platform stood on, as of the last SyncCharacters
    template <class Vec3> bool GetCharacterRide(typename GpuSceneMirror<SceneT>::Id entity, GpuCharacterRide<Vec3>& out) const
    {
        return lastScene_ && GpuMirrors<SceneT>::Of(*lastScene_).GetCharacterRide(entity, out);
    }
    // EXTENSION: characters push each other apart (include/bge_world.h "Crowd separation"), off by default.  In the reference the
    // character ghosts block each other's sweeps; here every step begins by parting overlapping characters by half their overlap
    // (at most maxPush per step; 0 = no limit), level, away from the deepest neighbour.  A push, not a cast: two characters may
    // overlap by what one step walked.
    void SetCharacterCrowd(bool on, float maxPush = 0.0f)
    {
        characterCrowd_ = on;
        characterCrowdMaxPush_ = on ? maxPush : 0.0f;
        if (lastScene_) GpuMirrors<SceneT>::Of(*lastScene_).SetCharacterCrowd(characterCrowd_, characterCrowdMaxPush_);
    }
    // what the last step of the last UpdateCharacters found around the character, as of the last SyncCharacters
    template <class Vec3> bool GetCharacterCrowd(typename GpuSceneMirror<SceneT>::Id entity, GpuCharacterCrowd<Vec3>& out) const
    {
        return lastScene_ && GpuMirrors<SceneT>::Of(*lastScene_).GetCharacterCrowd(entity, out);
    }
    // EXTENSION: characters push the Dynamic bodies they walk into (include/bge_world.h "Character push"), off by default.  In the
    // reference the character's ghost is a fixed body to the solver and a crate is pushed out of it; here the body a step's slide
    // hit gets force * dt, level, away from the character, unless the hit is steeper than maxNormalY (a character standing on a
    // crate does not push it).  No reaction on the character, no spin.
    void SetCharacterPush(bool on, float force = 0.0f, float maxNormalY = 0.5f)
    {
        characterPush_ = on;
        characterPushForce_ = on ? force : 0.0f;
        characterPushMaxNormalY_ = maxNormalY;
        if (lastScene_) GpuMirrors<SceneT>::Of(*lastScene_).SetCharacterPush(characterPush_, characterPushForce_, characterPushMaxNormalY_);
    }
    // EXTENSION: impulses (include/bge_world.h "Impulses"): btRigidBody::applyImpulse / applyCentralImpulse / applyTorqueImpulse,
    // each with activate(), on the body of `entity` in the scene of the last Update.  Queued, and applied in call order as one batch
    // at the head of the next Update, before its step; ActivateBody only wakes.  false before the first Update.
    template <class Vec3> bool ApplyImpulse(typename GpuSceneMirror<SceneT>::Id entity, const Vec3& impulse, const Vec3& relPos)
    {
        return QueueImpulse(entity, BGE_IMPULSE_AT_POINT, impulse.x, impulse.y, impulse.z, relPos.x, relPos.y, relPos.z);
    }
    template <class Vec3> bool ApplyCentralImpulse(typename GpuSceneMirror<SceneT>::Id entity, const Vec3& impulse)
    {
        return QueueImpulse(entity, BGE_IMPULSE_CENTRAL, impulse.x, impulse.y, impulse.z, 0.0f, 0.0f, 0.0f);
    }
    template <class Vec3> bool ApplyTorqueImpulse(typename GpuSceneMirror<SceneT>::Id entity, const Vec3& torque)
    {
        return QueueImpulse(entity, BGE_IMPULSE_TORQUE, torque.x, torque.y, torque.z, 0.0f, 0.0f, 0.0f);
    }
    bool ActivateBody(typename GpuSceneMirror<SceneT>::Id entity) { return QueueImpulse(entity, BGE_IMPULSE_CENTRAL, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f); }
    // EXTENSION: the query index (include/bge_world.h "Query index"), off by default.  With it on, Raycast .. UpdateCharacters
    // visit only the bodies near each query instead of every body; every answer keeps its bytes.  cellEdge = 0: the library's
    // choice.  Handed to the scene's mirror here and by every Update.
    void SetQueryIndex(bool on, float cellEdge = 0.0f)
    {
        queryIndexSet_ = true;
        queryIndex_ = on;
        queryIndexEdge_ = on ? cellEdge : 0.0f;
        if (lastScene_) GpuMirrors<SceneT>::Of(*lastScene_).SetQueryIndex(queryIndex_, queryIndexEdge_);
    }
    // what the last call that queried did with the index (synchronises the world's stream)
    bool GetQueryIndexStats(bge_query_index_stats& out) const
    {
        return lastScene_ && GpuMirrors<SceneT>::Of(*lastScene_).GetQueryIndexStats(out);
    }
    // as of the last SyncCharacters
    bool CharacterOnGround(typename GpuSceneMirror<SceneT>::Id entity) const
    {
        return lastScene_ && GpuMirrors<SceneT>::Of(*lastScene_).CharacterOnGround(entity);
    }
    template <class Vec3> bool GetCharacterState(typename GpuSceneMirror<SceneT>::Id entity, GpuCharacterState<Vec3>& out) const
    {
        return lastScene_ && GpuMirrors<SceneT>::Of(*lastScene_).GetCharacterState(entity, out);
    }
    // The walk displacement of one step from the camera's yaw, the MoveForward and MoveRight axes, Sprint, the walk speed and dt, with
    // the arithmetic of HandleCharacterInput (:797-832): no walk unless the direction's squared length exceeds 1e-5; the sprint
    // multiplier is the reference's 1.8.
    static void CharacterWalkFromInput(float yaw, float moveForward, float moveRight, bool sprint, float walkSpeed, double dt, float& dx, float& dz)
    {
        const float forwardX = std::cos(yaw);
        const float forwardZ = std::sin(yaw);
        const float rightX = forwardZ;
        const float rightZ = -forwardX;
        const float multiplier = sprint ? 1.8f : 1.0f;
        float x = forwardX * moveForward + rightX * moveRight;
        float z = forwardZ * moveForward + rightZ * moveRight;
        dx = dz = 0.0f;
        const float length2 = x * x + z * z;
        if (length2 > 1e-5f) {
            const float inv = 1.0f / std::sqrt(length2); // btVector3::normalize
            x *= inv;
            z *= inv;
            const float speed = walkSpeed * multiplier;
            dx = x * speed * static_cast<float>(dt);
            dz = z * speed * static_cast<float>(dt);
        }
    }

    // The debug overlay (src/physics/PhysicsSystem.h:77-82, bound to a key at src/core/Application.cpp:173; the renderer gets
    // GetDebugLines() every frame, :359).  While it is on, Update refills the buffer after the step (one bge_world_debug_lines
    // query on the scene's mirror); while it is off GetDebugLines() is empty and Update does nothing for it.
    void ToggleDebugOverlay() { SetDebugOverlayEnabled(!debugDrawEnabled_); }
    void SetDebugOverlayEnabled(bool enabled)
    {
        if (debugDrawEnabled_ == enabled) return;
        debugDrawEnabled_ = enabled;
        if (!enabled) debugLines_.clear();
        std::printf("[PhysicsDebug] overlay %s\n", enabled ? "ON" : "OFF");
    }
    bool IsDebugOverlayEnabled() const { return debugDrawEnabled_; }
    const DebugLineBuffer& GetDebugLines() const { return debugDrawEnabled_ ? debugLines_ : emptyDebugLines_; }
    // Not in the reference: draw only the bodies, ghosts and contact points inside the closed box [min, max] (the plane always) —
    // what makes the overlay usable in a world of 10^6 bodies
    template <class Vec3> void SetDebugRegion(const Vec3& mn, const Vec3& mx)
    {
        debugDesc_.use_region = 1u;
        debugDesc_.region_min[0] = mn.x, debugDesc_.region_min[1] = mn.y, debugDesc_.region_min[2] = mn.z;
        debugDesc_.region_max[0] = mx.x, debugDesc_.region_max[1] = mx.y, debugDesc_.region_max[2] = mx.z;
    }
    void ClearDebugRegion() { debugDesc_.use_region = 0u; }

    // PhysicsSystem::Config (src/physics/PhysicsSystem.h:85-95); AddCharacter takes the character fields (capsuleHeight has no use
    // for a sphere; walkSpeed is the caller's, for CharacterWalkFromInput)
    struct Config {
        float gravity = -9.81f;
        float fixedStep = 1.0f / 120.0f;
        float stepHeight = 0.35f;
        float maxSlopeDeg = 50.0f;
        float capsuleHeight = 1.7f;
        float capsuleRadius = 0.35f;
        float walkSpeed = 3.5f;
        float jumpImpulse = 5.0f;
    };
    const Config& GetConfig() const { return config_; }

private:
    // LoadConfigFromDisk (PhysicsSystem.cpp:242-282): missing keys keep the current value, an unreadable or malformed
    // file keeps the whole current config, a non-positive fixedStep becomes 1/120
    Config LoadConfigFromDisk() const
    {
        Config cfg = config_;
        std::ifstream file(configPath_);
        if (!file.is_open()) {
            std::fprintf(stderr, "[Physics] Failed to open config: %s\n", configPath_.string().c_str());
            return cfg;
        }
        std::stringstream ss;
        ss << file.rdbuf();
        const std::string text = ss.str();
        json::Value data;
        std::string err;
        json::Parser parser(text);
        if (!parser.parse(data, &err) || data.kind != json::Value::Object) {
            std::fprintf(stderr, "[Physics] Failed to parse config: %s\n", err.c_str());
            return cfg;
        }
        cfg.gravity = detail::read_float(data, "gravity", cfg.gravity);
        cfg.fixedStep = detail::read_float(data, "fixedStep", cfg.fixedStep);
        cfg.stepHeight = detail::read_float(data, "stepHeight", cfg.stepHeight);
        cfg.maxSlopeDeg = detail::read_float(data, "maxSlopeDeg", cfg.maxSlopeDeg);
        cfg.walkSpeed = detail::read_float(data, "walkSpeed", cfg.walkSpeed);
        cfg.jumpImpulse = detail::read_float(data, "jumpImpulse", cfg.jumpImpulse);
        if (const json::Value* capsule = data.find("capsule"); capsule && capsule->kind == json::Value::Object) {
            cfg.capsuleHeight = detail::read_float(*capsule, "height", cfg.capsuleHeight);
            cfg.capsuleRadius = detail::read_float(*capsule, "radius", cfg.capsuleRadius);
        }
        if (!(cfg.fixedStep > 0.0f)) cfg.fixedStep = 1.0f / 120.0f;
        return cfg;
    }

    void Step(SceneT& scene, double dt)
    {
        auto& m = GpuMirrors<SceneT>::Of(scene);
        lastScene_ = &scene;
        if (queryIndexSet_) m.SetQueryIndex(queryIndex_, queryIndexEdge_); // (until SetQueryIndex is called the world keeps its default: off)
        m.gravity[0] = 0.0f;
        m.gravity[1] = config_.gravity; // m_world->setGravity(btVector3(0, m_config.gravity, 0)), PhysicsSystem.cpp:130, 292
        m.gravity[2] = 0.0f;
        m.bullet_basis = bulletBasis_;
        if (m.ground_plane_state != static_cast<int>(groundPlane_)) {
            m.SetGroundPlane(groundPlane_);
            m.ground_plane_state = static_cast<int>(groundPlane_);
        }
        m.max_sub_steps = 4;                                        // PhysicsSystem.cpp:863
        m.fixed_step = std::max(config_.fixedStep, 1.0f / 240.0f); // kMinStep, PhysicsSystem.cpp:33, 855
        const auto start = std::chrono::high_resolution_clock::now();
        m.UpdatePhysics(scene, dt);
        const auto end = std::chrono::high_resolution_clock::now();
        lastStepDurationMs_ = std::chrono::duration<double, std::milli>(end - start).count(); // includes the pose download
        lastStepDt_ = dt;
        lastStepSubsteps_ = m.last_sub_steps;
        lastBodies_ = m.CollisionObjectCount();
        if (debugDrawEnabled_) m.DebugLines(debugDesc_, debugLines_); // debugDrawWorld + CollectDebugLines, PhysicsSystem.cpp:866-870
    }

    bool QueueImpulse(typename GpuSceneMirror<SceneT>::Id entity, uint32_t flags, float ix, float iy, float iz, float px, float py, float pz)
    {
        if (!lastScene_) return false;
        const float impulse[3] = {ix, iy, iz}, point[3] = {px, py, pz};
        GpuMirrors<SceneT>::Of(*lastScene_).QueueImpulse(entity, flags, impulse, point);
        return true;
    }

    std::filesystem::path configPath_;
    std::filesystem::file_time_type lastWriteTime_{};
    bool hasLastWriteTime_ = false;
    Config config_{};
    bool bulletBasis_ = false;
    bool groundPlane_ = true;
    SceneT* lastScene_ = nullptr; // the scene whose world the ray queries read
    bool characterTriggerEvents_ = false; // SetCharacterTriggerEvents: handed to the scene's mirror by UpdateCharacters
    bool characterRiding_ = false, characterRidingDynamic_ = false; // SetCharacterPlatformRiding: the same
    bool characterCrowd_ = false;                                   // SetCharacterCrowd: the same
    float characterCrowdMaxPush_ = 0.0f;
    bool characterPush_ = false;                                    // SetCharacterPush: the same
    float characterPushForce_ = 0.0f, characterPushMaxNormalY_ = 0.5f;
    bool queryIndexSet_ = false, queryIndex_ = false; // SetQueryIndex: handed to the scene's mirror by Step
    float queryIndexEdge_ = 0.0f;
    bool debugDrawEnabled_ = false;
    bge_debug_desc debugDesc_{static_cast<uint32_t>(sizeof(bge_debug_desc)), BGE_DEBUG_ALL, 0u, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
    DebugLineBuffer debugLines_;
    DebugLineBuffer emptyDebugLines_; // (stays empty)
    double lastStepDurationMs_ = 0.0, lastStepDt_ = 0.0;
    int lastStepSubsteps_ = 0, lastBodies_ = 0;
};

} // namespace bge
