/*
 * bge_world.h — C ABI of the MI355X-native ECS world tick (libbge_world.so).
 *
 * The reference (Skeletus/BangGameEngine) has no plugin/FFI layer: the per-frame world update is
 * three C++ call sites inside Application::Update (src/core/Application.cpp:256, :283-285).  This
 * header is the boundary a maintainer binds instead (INTEGRATION.md shows the C++ adapter that keeps
 * the reference's call shapes on top of it).  Each entry point cites the reference code it replaces.
 *
 * Model
 *   - A `bge_world` is a device-resident mirror of one reference `Scene` (src/ecs/Scene.h:97-105):
 *     Transform / RigidBody / Collider components as structure-of-arrays in HBM, plus the parent→child
 *     hierarchy flattened into 256-slot tiles ordered by depth.
 *   - Entities are addressed by a dense ENTITY INDEX in [0, n) chosen by the caller (the adapter maps
 *     the reference's sparse EntityId — src/ecs/Entity.h:4-5 — onto it).
 *   - Matrices are 16 floats, row-major, row-vector convention, translation in elements 12..14, exactly
 *     as `Transform::world` (src/ecs/Transform.h:18-19).
 *   - Not thread-safe: one host thread per world (the reference is single-threaded).
 *   - Every function returns BGE_OK (0) or a negative error code and never throws; the message of the
 *     last failure on the calling thread is available from bge_last_error().
 *   - All work is enqueued on the world's HIP stream (bge_world_desc.stream, or a private stream);
 *     download functions synchronise that stream before returning.
 */
#ifndef BGE_WORLD_H
#define BGE_WORLD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BGE_API __attribute__((visibility("default")))

#define BGE_NO_PARENT 0xffffffffu

enum bge_status {
    BGE_OK = 0,
    BGE_ERR_INVALID = -1,     /* bad argument */
    BGE_ERR_HIP = -2,         /* a HIP runtime call failed */
    BGE_ERR_OOM = -3,         /* host or device allocation failed */
    BGE_ERR_STATE = -4,       /* call order (e.g. upload before set_topology) */
    BGE_ERR_UNSUPPORTED = -5  /* feature not built */
};

/* RigidBodyType (src/ecs/PhysicsComponents.h:20-25) + "entity has no rigid body" */
enum bge_body_type { BGE_BODY_STATIC = 0, BGE_BODY_DYNAMIC = 1, BGE_BODY_KINEMATIC = 2, BGE_BODY_NONE = 255 };
/* Bullet's activation states (btCollisionObject.h), as the reference's bodies carry them:
 * Dynamic bodies are created ACTIVE_TAG, Kinematic ones DISABLE_DEACTIVATION (src/physics/PhysicsSystem.cpp:454-463). */
enum bge_activation {
    BGE_ACTIVATION_NONE = 0,
    BGE_ACTIVE_TAG = 1,
    BGE_ISLAND_SLEEPING = 2,
    BGE_WANTS_DEACTIVATION = 3,
    BGE_DISABLE_DEACTIVATION = 4
};
/* ColliderShape (src/ecs/PhysicsComponents.h:7-11) */
enum bge_shape { BGE_SHAPE_BOX = 0, BGE_SHAPE_CAPSULE = 1 };

/* What one bge_world_tick does. */
enum bge_tick_flags {
    BGE_TICK_PHYSICS = 1u,    /* rigid-body slice of PhysicsSystem::Update (src/physics/PhysicsSystem.cpp:1208-1328) */
    BGE_TICK_TRANSFORMS = 2u, /* TransformSystem::Update (src/ecs/TransformSystem.cpp:40-46) */
    BGE_TICK_BROADPHASE = 4u, /* AABB update + overlapping pairs (Bullet updateAabbs/calculateOverlappingPairs) */
    BGE_TICK_ALL = 3u,        /* Application::Update's physics + transform steps (src/core/Application.cpp:256,284) */
    BGE_TICK_GATHER_ROOTS = 8u, /* after the tick: bge_world_gather_roots (needs bge_world_comm_init) */
    BGE_TICK_NORMAL_MATRICES = 16u, /* with TRANSFORMS: also write transpose(inverse(world)) per entity, the normalMtx
                                      Renderer::BeginFrame computes on the CPU per mesh (src/render/Renderer.cpp:633-636) */
    BGE_TICK_AABBS = 32u,     /* with PHYSICS: update the AABBs (Bullet updateAabbs) without the local pair search —
                                 the sharded broadphase (bge_world_bp_*) searches them across ranks instead */
    BGE_TICK_BULLET_BASIS = 64u /* with PHYSICS: Bullet's own orientation scheme for every Dynamic body, spinning or not —
                                 each step its basis goes through btMatrix3x3::getRotation, btTransformUtil::integrateTransform's
                                 exponential map + safeNormalize and setRotation, and SyncRigidBodiesFromPhysics
                                 (src/physics/PhysicsSystem.cpp:925-950) rewrites Transform::rotationEuler from it.  Without the
                                 flag a body whose angular velocity is exactly zero keeps its orientation and euler triple bit
                                 for bit (within 1e-5 relative of this mode; 44 bytes per body and tick cheaper).
                                 Use one mode for the whole life of a world. */
};

enum bge_device_array {
    BGE_ARRAY_WORLD = 0,          /* float[n_slots][16], slot order; READ-ONLY to consumers: a tick rewrites only the
                                     translation row of a matrix whose rotation rows it knows to be current,
                                     so a value written here into rows 0..2 may persist.  Asking for this pointer (or for
                                     BGE_ARRAY_POSITION) PINS the world: a tick of a flat scene otherwise leaves the
                                     translation row of such a matrix unstored (it is a copy of the position; downloads, the
                                     visible list, draw batches and bge_world_pack_roots compose it).  The call stores what
                                     is outstanding, waits for it, and no later tick of this world defers a row, so the
                                     memory behind the pointer is complete after every tick, at the cost of that store
                                     (about three times the time of a flat tick at 1 M bodies).  Consumers
                                     that can use bge_world_visible_device / bge_world_draw_batches_device /
                                     bge_world_pack_roots instead keep the cheaper tick. */
    BGE_ARRAY_ROOT_WORLDS = 1,    /* float[n_roots][16], filled by bge_world_pack_roots */
    BGE_ARRAY_SLOT_OF_ENTITY = 2, /* uint32[n_entities], BGE_NO_PARENT where the entity has no Transform */
    BGE_ARRAY_POSITION = 3,       /* float[n_slots][3]; pins the world like BGE_ARRAY_WORLD (a write through this pointer
                                     must not reach a matrix before the next tick) */
    BGE_ARRAY_PAIRS = 4,          /* uint32[pair_capacity][2], entity indices */
    BGE_ARRAY_NORMAL = 5          /* float[n_slots][16] normal matrices, slot order (after a NORMAL_MATRICES tick) */
};

typedef struct bge_world bge_world;

typedef struct bge_world_desc {
    uint32_t struct_size; /* sizeof(bge_world_desc) */
    int32_t device;       /* HIP device ordinal, or -1 for the current device */
    void* stream;         /* hipStream_t to enqueue on, or NULL for a private non-blocking stream */
    uint64_t pair_capacity; /* max overlapping pairs kept per tick (0 = 8 x entities); emission is split over 64 shards */
} bge_world_desc;

typedef struct bge_world_info {
    uint64_t n_entities;
    uint64_t n_transforms; /* entities that own a Transform */
    uint64_t n_slots;      /* n_tiles * 256 */
    uint64_t n_tiles;      /* tiles that are ticked */
    uint64_t n_passes;     /* dependent launches per transform pass (1 unless a subtree exceeds a tile) */
    uint64_t n_roots;
    uint64_t n_limbo;      /* transforms inside a parent cycle: never updated, stay dirty */
    uint64_t n_bodies;
    uint64_t max_depth;
} bge_world_info;

BGE_API const char* bge_last_error(void);
BGE_API uint32_t bge_version(void);

/* Scene lifetime: `Application` owning a `Scene` + `PhysicsSystem` (src/core/Application.h:39-42). */
BGE_API int bge_world_create(const bge_world_desc* desc, bge_world** out);
BGE_API void bge_world_destroy(bge_world* world);

/*
 * Hierarchy: replaces Scene::m_parents / m_children and the root scan of
 * Scene::ForEachRootTransform (src/ecs/Scene.cpp:354-393, 523-533).
 *   parent[i]         entity index of i's parent, or BGE_NO_PARENT
 *   has_transform[i]  0/1, NULL = all 1.  An entity whose parent has no Transform is a root
 *                     (Scene.cpp:528); an entity without a Transform gets no slot.
 * Entities in a parent cycle are never reached by the reference's DFS; they are kept, never updated,
 * and stay dirty.  Calling this again re-flattens and keeps all component state of surviving indices.
 * All Transforms start dirty with TRS = (0, 0, 1) as a default-constructed Transform (Transform.h:14-16).
 * On a live world the call also does what the reference's scene edits do to what stays:
 *   - a changed parent ENTITY marks the child's subtree dirty, through Transform-less entities too (Scene::SetParent ->
 *     MarkHierarchyDirty, Scene.cpp:354-393, 535-550).  "Changed" is read off the two arrays: a child moved away and back
 *     between two calls (two SetParent calls in the reference, each marking it) shows nothing here — mark it with
 *     bge_world_mark_dirty, as an adapter that forwards Transform::dirty does anyway;
 *   - a clean Transform whose parent entity stays but lost its Transform becomes a root WITHOUT being marked, and keeps its
 *     world matrix until something marks it (Scene::RemoveTransform marks nobody; TransformSystem::Update recomputes a node
 *     only when it or an ancestor is dirty);
 *   - an entity that loses its Transform while its body is in the world (uploaded, and a physics tick has run since) keeps
 *     the body: it is stepped, collides and enters trigger volumes as before, is never re-posed or re-created, nothing is
 *     written back, and uploads of Transform or body data to it are ignored — except BGE_BODY_NONE, which removes it
 *     (PhysicsSystem::EnsureRigidBody returns before it looks at the runtime of an entity without a Transform,
 *     PhysicsSystem.cpp:389-393, and only the RigidBody component's removal takes the body out).  A caller that drops an
 *     entity altogether uploads BGE_BODY_NONE for it before the call;
 *   - a trigger volume whose entity loses its Transform stays in the world with the box it was last posed to (EnsureTrigger
 *     returns early as well) until the trigger is removed from the uploaded set or the Transform returns.
 */
BGE_API int bge_world_set_topology(bge_world* world, uint64_t n, const uint32_t* parent, const uint8_t* has_transform);

/*
 * Transform components: position / rotationEuler (radians) / scale as packed xyz triples
 * (src/ecs/Transform.h:14-16).  Any array may be NULL (left unchanged).  Marks the range dirty
 * (Transform::MarkDirty, src/ecs/Transform.cpp:13-16).
 */
BGE_API int bge_world_upload_trs(bge_world* world, uint64_t first, uint64_t count, const float* pos3,
                                 const float* euler3, const float* scale3);
BGE_API int bge_world_mark_dirty(bge_world* world, uint64_t first, uint64_t count);
/* Sparse form: row i belongs to entity entity_index[i] (what an adapter uploads after scanning for Transform::dirty). */
BGE_API int bge_world_upload_trs_indexed(bge_world* world, uint64_t count, const uint32_t* entity_index,
                                         const float* pos3, const float* euler3, const float* scale3);

/*
 * RigidBody + Collider components (src/ecs/PhysicsComponents.h:13-37) for a range of entities.
 *   type[i]   bge_body_type; BGE_BODY_NONE removes the body.  A body exists only where the entity also has
 *             a Transform (PhysicsSystem.cpp:389-393).
 *   mass      RigidBody::mass (Dynamic: max(mass, 0.01), else 0 — PhysicsSystem.cpp:426-429); NULL = 1
 *   shape     bge_shape, NULL = box;   size3: Collider::size, NULL = (.5,.5,.5)
 *   layer / mask   NULL = 1 / 0xffffffff; layer 0 is treated as 1 (PhysicsSystem.cpp:407)
 * Marks RigidBody.dirty and Collider.dirty: on the next physics tick the body is (re)created from its
 * Transform with zero velocity (PhysicsSystem.cpp:398-477).
 */
BGE_API int bge_world_upload_bodies(bge_world* world, uint64_t first, uint64_t count, const uint8_t* type,
                                    const float* mass, const uint8_t* shape, const float* size3,
                                    const uint32_t* layer, const uint32_t* mask);
BGE_API int bge_world_upload_bodies_indexed(bge_world* world, uint64_t count, const uint32_t* entity_index,
                                            const uint8_t* type, const float* mass, const uint8_t* shape,
                                            const float* size3, const uint32_t* layer, const uint32_t* mask);
/*
 * Extension (no reference API): overwrite linear / angular velocity without touching dirty flags.
 * The reference's bodies only ever gain velocity from gravity and contacts; synthetic workloads seed it.
 * An angular velocity then stays constant: Bullet's gyroscopic impulse (zero at rest, hence zero for every body the
 * reference can create without contacts) is not part of the path.
 */
BGE_API int bge_world_set_velocities(bge_world* world, uint64_t first, uint64_t count, const float* linvel3,
                                     const float* angvel3);

/*
 * One fixed-step tick = Application::Update's data-parallel part (src/core/Application.cpp:256, 284):
 *   BGE_TICK_PHYSICS     re-pose dirty bodies from their Transform (zeroing Dynamic velocities,
 *                        PhysicsSystem.cpp:952-989), one Bullet sub-step for free bodies
 *                        (v += g*dt; x += v*dt; exponential-map rotation), write position/rotationEuler back
 *                        and mark Dynamic transforms dirty (PhysicsSystem.cpp:916-950)
 *   BGE_TICK_TRANSFORMS  local = mtxSRT(S,R,T); world = parentWorld * local (root: world = local); clear dirty
 *   BGE_TICK_BROADPHASE  (with PHYSICS) feed AABBs and collect overlapping pairs
 * dt is seconds (the reference narrows its double once, PhysicsSystem.cpp:863); gravity is 3 floats
 * (the reference uses (0, config.gravity, 0), PhysicsSystem.cpp:130).
 */
BGE_API int bge_world_tick(bge_world* world, float dt, const float gravity[3], uint32_t flags);
/*
 * Enqueue `ticks` identical ticks back to back (the catch-up loop of Application::Run, Application.cpp:96-101).
 * Nothing can observe the state between the ticks of one call, and the library uses that: in a flat scene (one pass, no frozen
 * root) ticked with PHYSICS | TRANSFORMS alone, the ticks go out in groups of BGE_FUSE_TICKS launches (environment, read per
 * call; default 8; 1 = off), and a wave of 64 bodies whose tick is known to be lane-local arithmetic runs the ticks that remain of
 * its group in one launch.  The intermediate ticks of a call are then never materialised in memory for those bodies; after the
 * call every array holds what `ticks` single calls would have left, bit for bit.  There is still one launch per tick on the
 * stream, groups never span calls, and an event pair per tick (bge_world_profile_enable(2)) switches the grouping off.
 * Solo groups: where EVERY tile of the scene is flat (no hierarchy at all, no frozen root), a group is ONE launch in which every
 * wave runs the group's ticks itself, one after the other, and the group's other ticks launch nothing; they still count as ticks
 * everywhere (bge_world_profile_read, the bodies' birth rule).  The default group is then 512 ticks (BGE_FUSE_TICKS sets it for both
 * schemes).  BGE_SOLO_GROUPS=0 (environment, read per call; default on) keeps one launch per tick.
 * If a launch of the call fails, bodies may be left at different ticks: the world is not usable after a failed tick call.
 */
BGE_API int bge_world_tick_many(bge_world* world, uint32_t ticks, float dt, const float gravity[3], uint32_t flags);
/*
 * PhysicsSystem::StepSimulation (src/physics/PhysicsSystem.cpp:848-875) = Bullet's
 *     m_world->stepSimulation(static_cast<btScalar>(dt), 4, max(config.fixedStep, 1/240))
 * around the world's ticks: the world keeps Bullet's clock m_localTime (binary32).  Every call adds dt to it;
 * n = int(m_localTime / fixed_step) sub-steps of fixed_step are due (0 while the clock is below fixed_step), all n are
 * taken off the clock, min(n, max_sub_steps) are simulated; *sub_steps (may be NULL) receives n, stepSimulation's return
 * value.  With dt == fixed_step — what Application::Run passes (src/core/Application.cpp:96-101, 326) — that is exactly
 * one sub-step per call and identical to bge_world_tick(world, fixed_step, gravity, flags).  max_sub_steps == 0 is Bullet's
 * variable-step mode: one step of dt.
 *   flags   as for bge_world_tick; BGE_TICK_PHYSICS is required.  The teleport rule (re-pose of dirty bodies) is applied
 *           once, before the first sub-step (SyncKinematicBodiesToPhysics runs before stepSimulation); AABBs / pairs /
 *           trigger events / world matrices / the root gather are produced once, from the state after the last sub-step
 *           (trigger ghosts are posed from the Transforms as they were before the first).
 *   n == 0  nothing is simulated, but what PhysicsSystem::Update does around the step still happens: dirty bodies are
 *           re-posed, every Dynamic body's Transform is marked dirty again (SyncRigidBodiesFromPhysics), and every
 *           remembered trigger overlap is reported as Stay (the ghosts' pair caches did not change).
 * bge_world_reset_clock zeroes m_localTime (a new btDiscreteDynamicsWorld, e.g. after OnSceneReloaded of a new world).
 */
BGE_API int bge_world_step_simulation(bge_world* world, double dt, int max_sub_steps, float fixed_step, const float gravity[3],
                                      uint32_t flags, int* sub_steps);
BGE_API int bge_world_reset_clock(bge_world* world);
BGE_API int bge_world_sync(bge_world* world);
/*
 * Kernel timing with HIP events on the world's stream (the reference times its step with chrono around
 * stepSimulation, src/physics/PhysicsSystem.cpp:862-866).
 *   enable = 1  one event pair around each bge_world_tick_many call (all its launches, gaps included) — no
 *               markers between back-to-back kernels, so it does not perturb what it measures
 *   enable = 2  one pair around every tick's tick-kernel launches (excludes broadphase / collective work that
 *               is interleaved on the stream; costs a few microseconds per tick)
 *   enable = 0  off
 * bge_world_profile_read synchronises the stream and returns the summed time and the number of ticks covered
 * since the last read.
 */
BGE_API int bge_world_profile_enable(bge_world* world, int enable);
BGE_API int bge_world_profile_read(bge_world* world, double* tick_kernel_ms, uint64_t* ticks);

/* Page-locked host buffers for the upload / download entry points: copies to and from them run at the PCIe rate
 * (pageable memory: roughly a fifth of it).  Optional — every entry point accepts any host pointer. */
BGE_API int bge_host_alloc(uint64_t bytes, void** out);
BGE_API int bge_host_free(void* p);
/* What the library itself holds in this process, over all worlds: the number of live blocks and their bytes (device memory and the
 * few page-locked blocks of the worlds; bge_host_alloc memory belongs to the caller and is not counted).  Both are 0 once every
 * world is destroyed.  Either pointer may be NULL.  Costs two atomic loads; safe from any thread. */
BGE_API void bge_device_memory(uint64_t* allocations, uint64_t* bytes);

/* Results.  `Transform::world` after TransformSystem::Update; position/rotationEuler after PhysicsSystem::Update. */
BGE_API int bge_world_download_world(bge_world* world, uint64_t first, uint64_t count, float* out16);
BGE_API int bge_world_download_pose(bge_world* world, uint64_t first, uint64_t count, float* pos3, float* euler3);
/* normalMtx per entity of the last BGE_TICK_NORMAL_MATRICES tick (16 floats, bx::mtxTranspose(bx::mtxInverse(world))). */
BGE_API int bge_world_download_normal(bge_world* world, uint64_t first, uint64_t count, float* out16);
BGE_API int bge_world_download_world_indexed(bge_world* world, uint64_t count, const uint32_t* entity_index, float* out16);
BGE_API int bge_world_download_pose_indexed(bge_world* world, uint64_t count, const uint32_t* entity_index, float* pos3,
                                            float* euler3);
BGE_API int bge_world_download_bodies(bge_world* world, uint64_t first, uint64_t count, float* linvel3,
                                      float* angvel3, float* quat4, float* aabb6);
BGE_API int bge_world_download_dirty(bge_world* world, uint64_t first, uint64_t count, uint8_t* dirty);
/* Deactivation ("sleeping") of free bodies, inside stepSimulation (src/physics/PhysicsSystem.cpp:863): a Dynamic body
 * whose |v| stays below 0.8 and |w| below 1.0 for more than 2 s goes WANTS_DEACTIVATION at the end of that step and
 * ISLAND_SLEEPING in the next one (a free body is an island of its own); asleep it takes no gravity, is not integrated,
 * and its velocities are zeroed every step.  Body (re)creation wakes it, and so does an impulse ("Impulses" below: the extension's
 * activate(); the reference never calls it).
 * state[i] receives a bge_activation; time[i] btCollisionObject::m_deactivationTime while the body is ACTIVE_TAG and 0
 * otherwise (Bullet keeps a stale value there that nothing reads).  Either pointer may be NULL. */
BGE_API int bge_world_download_activation(bge_world* world, uint64_t first, uint64_t count, uint8_t* state, float* time);
/* Thresholds of the above (Bullet's defaults 0.8, 1.0, 2.0 — the reference never changes them).
 * seconds == 0 disables sleeping (Bullet: gDeactivationTime == 0). */
BGE_API int bge_world_set_sleeping(bge_world* world, float linear_threshold, float angular_threshold, float seconds);
/*
 * The static ground plane of the reference's physics world, with Bullet's contact handling for it (SURVEY.md section 8(f)
 * rank 4).  PhysicsSystem::EnsureGround (src/physics/PhysicsSystem.cpp:149-166) adds btStaticPlaneShape((0,1,0), 0) with
 * friction 1 and restitution 0 to every world, in group StaticFilter (2) with mask AllFilter; stepSimulation (:863) then runs
 * btConvexPlaneCollisionAlgorithm and btSequentialImpulseConstraintSolver for every Dynamic body at the plane:
 *   per sub-step ONE contact at the collider's support vertex, kept in a 4-point persistent manifold; contact + friction
 *   rows with warm starting, split impulse below -0.04, 10 iterations; the implicit gyroscopic impulse of a spinning body.
 * A body dropped on the plane comes to rest on it and falls asleep (bge_world_download_activation).  Bodies still do not
 * collide with EACH OTHER on this path (no convex-convex narrowphase): a body is an island of its own.
 *   bge_world_set_ground_plane   0 (default) = free bodies, what BASELINE's workloads are; 1 = the reference's world.
 *                                A body whose mask lacks bit 1 (value 2) passes through, as in Bullet.
 *   bge_world_upload_friction    RigidBody::friction (default 0.5, src/ecs/PhysicsComponents.h:32); the plane's is 1.
 *   bge_world_download_contacts  n_points[i] in 0..4 and, per body, 4 x (localA.xyz, appliedImpulse, localB.x, distance,
 *                                localB.z, appliedImpulseLateral1; localB.y is exactly 0) — inspection (the reference exposes no contacts).
 */
BGE_API int bge_world_set_ground_plane(bge_world* world, int enabled);
BGE_API int bge_world_upload_friction(bge_world* world, uint64_t first, uint64_t count, const float* friction);
BGE_API int bge_world_upload_friction_indexed(bge_world* world, uint64_t count, const uint32_t* entity_index, const float* friction);
BGE_API int bge_world_download_contacts(bge_world* world, uint64_t first, uint64_t count, uint8_t* n_points, float* points32);

/*
 * Dynamic boxes on the Static / Kinematic BOX colliders of the scene (round 3).  The reference
 * creates every RigidBody — Static ones too — as a Bullet body with its btBoxShape / btCapsuleShape
 * (src/physics/PhysicsSystem.cpp:421-474, CreateShape :686-707) and its default dispatcher collides Dynamic bodies with them
 * (:122-128, 863): a body dropped over assets/scenes/demo.json:67-91's "Ground", a 50 x 1 x 50 box, rests on the box's top.
 *   bge_world_set_static_contacts  0 (default) = off, as BASELINE's free bodies need; 1 = every Dynamic body with a BOX collider
 *       collides with every Static / Kinematic body with a BOX collider whose fed AABB overlaps its own and whose layer / mask
 *       pass both ways: Bullet's btBoxBoxDetector (15-axis separating-axis test, face clipping, the four-point cull) into a
 *       4-point persistent manifold per pair, all of a body's manifolds (the plane's too) in ONE sequential-impulse island per
 *       body — a static body merges no islands.  Combined friction = product of both frictions clamped to +-10, combined
 *       restitution = product of both restitutions (btManifoldResult), so RigidBody::restitution (:438) is live here.
 *       Not built: capsules against boxes (GJK / EPA); Dynamic against Dynamic is bge_world_set_dynamic_contacts.  A body holds at most 4 such manifolds (lowest
 *       entity indices); the Dynamic body is always the pair's body A — Bullet orders a pair by proxy creation, which the
 *       reference leaves to an unordered_map's iteration order (oracle/boxbox_ref.h states every such choice).
 *       Switching OFF (1 -> 0) ends every pair with an obstacle at the call: afterwards no body holds a box manifold —
 *       bge_world_download_box_contacts reports 0 manifolds for every body at once, sleeping ones included — a tick is safe,
 *       a sleeping body stays asleep where it is (nothing else of any body changes), and a later switch to 1 starts from empty
 *       manifolds.  The call waits for the world's stream.
 *   bge_world_upload_restitution  RigidBody::restitution per entity (default 0, src/ecs/PhysicsComponents.h:33).
 *   bge_world_download_box_contacts  per queried entity: n_manifolds[i] in 0..4, header8 = 4 x (other entity index or
 *       0xffffffff, points 0..4) in ascending entity index, points192 = 4 manifolds x 4 points x (localA.xyz, localB.xyz,
 *       normalWorldOnB.xyz, distance, appliedImpulse, appliedImpulseLateral1).  Any of the three may be NULL.
 */
BGE_API int bge_world_set_static_contacts(bge_world* world, int enabled);
BGE_API int bge_world_upload_restitution(bge_world* world, uint64_t first, uint64_t count, const float* restitution);
BGE_API int bge_world_upload_restitution_indexed(bge_world* world, uint64_t count, const uint32_t* entity_index, const float* restitution);
BGE_API int bge_world_download_box_contacts(bge_world* world, uint64_t first, uint64_t count, uint8_t* n_manifolds, uint32_t* header8,
                                            float* points192);
/*
 * Dynamic boxes against EACH OTHER (round 3, after SURVEY.md section 8(f) rank 4).  In the reference every RigidBody is a
 * btRigidBody of one btDiscreteDynamicsWorld (src/physics/PhysicsSystem.cpp:122-131, 421-474): two Dynamic boxes collide, rest on
 * each other, and bodies whose AABBs overlap form ONE simulation island that is solved together and sleeps / wakes together.
 *   bge_world_set_dynamic_contacts  0 (default) = off; 1 = every pair of Dynamic bodies with BOX colliders whose fed AABBs overlap
 *       and whose layer / mask pass both ways is a pair of the cache (body A = the lower entity index): btBoxBoxDetector into a 4-point
 *       persistent manifold per pair; btSimulationIslandManager's rule — the bodies of every pair are united, touching or not; an
 *       island sleeps only when none of its bodies is ACTIVE_TAG, otherwise its sleeping bodies turn WANTS_DEACTIVATION (timer 0,
 *       no gravity until the stepSimulation call ends) — and btSequentialImpulseConstraintSolver over all manifolds of an island
 *       (the bodies in ascending entity index, each body's plane manifold, its manifolds with Static / Kinematic boxes, its pairs
 *       with Dynamic boxes of higher index: oracle/island_ref.h states why this order and not Bullet's pool order).  One device
 *       thread solves a small island, a workgroup a big one (rows that share no body side by side, level by level: the sequence's
 *       results exactly); the sub-step reads two counters back (pairs, island bodies).  Capsules take no part (GJK / EPA).
 *       Works with or without the plane and the static contacts.  The sub-step's pair search (all bodies, Static ones too) keeps
 *       pair_capacity pairs when bge_world_create was given one — more is BGE_ERR_INVALID, never a silent drop — and otherwise starts at
 *       8 per entity and doubles by itself whenever a sub-step finds more.
 *       Islands live inside ONE world: a scene sharded over several worlds (bge_partition_subtrees) does not collide bodies of
 *       different shards with each other.
 *   bge_world_download_dynamic_pairs  the pair cache after the last tick in ascending (lower, higher) entity index: *total pairs;
 *       for the first `cap`: header3 = lower index, higher index, points; points48 = 4 x (localA.xyz, localB.xyz, normalWorldOnB.xyz,
 *       distance, appliedImpulse, appliedImpulseLateral1).  header3 / points48 may be NULL.
 */
BGE_API int bge_world_set_dynamic_contacts(bge_world* world, int enabled);
BGE_API int bge_world_download_dynamic_pairs(bge_world* world, uint64_t cap, uint32_t* header3, float* points48, uint64_t* total);
/* Scene::CountDirtyTransforms (src/ecs/Scene.cpp:435-446): a device-side wave-reduced count. */
BGE_API int bge_world_dirty_count(bge_world* world, uint64_t* out);
/* Overlapping pairs of the last BROADPHASE tick as (a, b) entity indices, a < b, unordered list.
 * *total receives the number found on the device (at most cap are copied).  Fails with BGE_ERR_INVALID when the
 * device had to drop pairs (pair_capacity too small); pairs2 = NULL just queries the count. */
BGE_API int bge_world_pairs(bge_world* world, uint32_t* pairs2, uint64_t cap, uint64_t* total);

/*
 * Trigger volumes: TriggerVolume components (src/ecs/PhysicsComponents.h:39-48) and the
 * Enter / Stay / Exit events of PhysicsSystem::ProcessTriggerEvents (src/physics/PhysicsSystem.cpp:1017-1074).
 *   bge_world_upload_triggers replaces the world's whole trigger set (count may be 0).  Per trigger: the entity it
 *       sits on (needs a Transform), shape/size as for colliders, layer (0 is treated as 4, kDefaultTriggerLayer), mask,
 *       oneShot, active.  Triggers that were present before keep their remembered overlaps unless layer/mask changed.
 *   Every BGE_TICK_BROADPHASE tick then (a) poses each active trigger's ghost box from its entity's Transform as it is
 *       BEFORE the step (EnsureTrigger, PhysicsSystem.cpp:575), (b) tests it on the device against the fed AABB of every
 *       registered collision object — every rigid body, Static ones included, and every other active trigger ghost (each
 *       of two overlapping ghosts then reports the other) — with the filter (groupT & maskO) && (groupO & maskT): the
 *       content of Bullet's pair cache for the ghost (btGhostPairCallback, PhysicsSystem.cpp:132-133; the reference gives
 *       Bullet custom groups, :473,577, so no static-static exclusion applies; the ghost's own entity is skipped, :1033),
 *       (c) diffs the overlap set with the previous tick's — on the device, see bge_world_set_trigger_stay_events below; the host
 *       keeps the sets and takes over whenever it changed them itself —: Enter (0) / Stay (1) / Exit (2).  A one-shot trigger
 *       turns inactive after its first non-empty set, forgets it, and leaves the world at once: triggers processed AFTER
 *       it in the same tick no longer list it (:1062-1072).  The triggers are processed IN THE ORDER OF THE UPLOADED ARRAY
 *       (the reference walks a std::unordered_map — an order the language leaves open; the C++ adapter and the oracle use
 *       ascending EntityId).  With triggers present such a tick synchronises the stream (the events are for host code).
 *       A tick may find at most 2^20 overlaps (trigger, body) and (trigger, trigger) together; one that finds more fails with
 *       BGE_ERR_OOM and a message naming both numbers.  A tick that fails this way reports no events and leaves every
 *       remembered set as it was before it; the next successful tick is diffed against those sets.
 *   bge_world_trigger_events returns (and clears) the events accumulated since the previous call.
 *   bge_world_trigger_active reports TriggerVolume::active per queried entity (0 after a one-shot fired, or no trigger).
 *   With more than 64 triggers (BGE_TRIGGER_GRID_MIN overrides the number) step (b) changes: a ghost whose box covers at
 *       most 8192 cells of the broadphase grid looks up the bodies sorted into those cells (plus the bodies too wide for the
 *       grid) instead of being tested against every body; wider ghosts keep the all-bodies test.  The overlap sets are the
 *       same either way.  bge_world_trigger_query_stats reports how the last tick split the ghosts that are in the world.
 */
typedef struct bge_trigger_event {
    uint32_t type;    /* 0 Enter, 1 Stay, 2 Exit (PhysicsSystem::TriggerEvent::Type, src/physics/PhysicsSystem.h:50-62) */
    uint32_t trigger; /* entity index of the trigger */
    uint32_t other;   /* entity index of the body or of the other trigger */
} bge_trigger_event;
BGE_API int bge_world_upload_triggers(bge_world* world, uint64_t count, const uint32_t* entity_index, const uint8_t* shape,
                                      const float* size3, const uint32_t* layer, const uint32_t* mask,
                                      const uint8_t* one_shot, const uint8_t* active);
BGE_API int bge_world_trigger_events(bge_world* world, bge_trigger_event* out, uint64_t cap, uint64_t* total);
/* Stay events.  PhysicsSystem::ProcessTriggerEvents (src/physics/PhysicsSystem.cpp:1017-1074) reports Stay for every remembered
 * overlap on every tick, and so does bge_world_trigger_events by default.  With many volumes that list is the cost of the trigger
 * pass (92,000 records a tick at 4 M bodies x 1000 volumes): the Enter / Exit difference itself is taken on the device (a table of
 * last tick's overlaps stays there; only the changes travel).  enabled = 0 leaves the Stay records out — Enter and Exit still come,
 * in the same order — and bge_world_trigger_diff_stats counts what was left out.
 * device_ticks / host_ticks: how many ticks took their difference on the device / on the host (the first tick after the volumes or
 * their activation changed, ticks with a one-shot volume in the world, a tick with more than 65,536 changes; BGE_TRIGGER_DEVICE_DIFF=0
 * in the environment keeps every tick on the host). */
BGE_API int bge_world_set_trigger_stay_events(bge_world* world, int enabled);
BGE_API int bge_world_trigger_diff_stats(bge_world* world, uint64_t* device_ticks, uint64_t* host_ticks, uint64_t* stay_suppressed);

BGE_API int bge_world_trigger_active(bge_world* world, uint64_t count, const uint32_t* entity_index, uint8_t* active);
BGE_API int bge_world_trigger_query_stats(bge_world* world, uint32_t* through_grid, uint32_t* against_all_bodies);

/*
 * Ray queries: PhysicsSystem::Raycast / RaycastAll (src/physics/PhysicsSystem.cpp:1076-1146), i.e. Bullet's rayTest with a
 * ClosestRayResultCallback / AllHitsRayResultCallback of group -1 and mask layer_mask, for a batch of rays at once.
 * Parity with the reference's compiled caster is NOT pinned for this path; the rules below are the specification.
 *   Segment   from = origin, to = origin + direction * max_distance (direction is not normalised, as in the reference); a hit
 *             has fraction f in [0, 1], point = from + (to - from) * f, distance = f * max_distance (the reference's definition,
 *             not the Euclidean length), normal = outward unit normal of the surface hit, world space.
 *   No hit    when !(max_distance > 0), layer_mask == 0, direction == (0, 0, 0), or any input is not finite (NaN, inf).
 *   Filter    an object is a candidate when (objGroup & layer_mask) != 0 && objMask != 0.
 *   Objects   - every rigid body (Static, Dynamic, Kinematic; asleep or awake) at the pose Bullet holds after the last physics
 *               tick: position + quaternion (bge_world_download_pose / _bodies).  A box is the SHARP box of its half extents
 *               with margin (max(size, 0.01)); a capsule is Bullet's Y-axis capsule (radius, half height).  Bodies uploaded
 *               since the last physics tick (Bullet creates them in the next Update) and removed bodies are not in the world.
 *             - every trigger ghost that is in the world at the pose the last BGE_TICK_BROADPHASE tick gave it (EnsureTrigger poses it
 *               from the Transform as it was before the step): the entity is the trigger's.  Inactive ghosts, ghosts of fired
 *               one-shots and ghosts never posed (or not posed since the last bge_world_upload_triggers) are not hit.
 *             - the ground plane when bge_world_set_ground_plane is on: group StaticFilter (2), mask all-ones, hit from either side
 *               (btTriangleRaycastCallback without back-face filtering): normal +y from above, -y from below; a segment that does
 *               not cross y = 0 strictly (parallel, or an end point on the plane) does not hit it.  entity = BGE_RAY_NO_ENTITY.
 *   Closest   smallest f; ties go to the lowest object code: bodies by entity index, then ghosts by entity index, then the plane.
 *   All hits  one record per object crossed, each ray's list sorted by (f, object code) (Bullet's order is its dbvt traversal
 *             order, which depends on history: this order is a specification choice).
 *   Choices   - a ray that starts inside or on the surface of a box or capsule does not hit that shape;
 *             - boxes are sharp: Bullet's GJK caster rounds a box's edges by its 0.04 margin, so a ray grazing within 0.04 of an
 *               edge may differ from the reference;
 *             - Bullet also culls bodies whose fed AABB of the last sub-step misses the ray; here the shape at its current pose
 *               alone decides.
 *   Call order  the query reads the device state as it is: call it after a physics tick and before new poses are uploaded, as
 *             Application::Update does (src/core/Application.cpp:256-281).  A Transform uploaded between the tick and the query
 *             moves the body's position for the query (its orientation stays the one the tick left).
 *   Range     everything is binary32.  An answer is the exact answer of a world whose shapes are moved by at most
 *               B = 2e-6 * (|from|_1 + |to - from|_1 + |body origin|_1 + the body's bounding radius [+ the cast's radius]),
 *             about 4e-6 of the distance from the world's origin for a query from nearby: 0.005 at 1,000 units, 0.04 at 10,000,
 *             0.4 at 100,000 (one binary32 spacing there is 0.008).  A feature thinner than B (a body, a gap, an offset from a
 *             face) is not resolved: a query may report or miss it either way.  Supported, and tested, are bodies whose smallest
 *             half extent or radius is at least 30 B, that is 1.2e-4 of |origin|_1: 0.12 at 1,000 units, 1.2 at 10,000, 12 at
 *             100,000.  Smaller bodies that far out are still found by overlaps and penetrations, whose distances are good to
 *             the same B; for rays and casts at them keep the world within that range of its origin, or move the origin.
 *             This holds for the sphere queries, the sphere moves and the recovery below as well.
 *   bge_world_raycast         hits[i] for rays[i]; a miss is kind BGE_RAY_MISS, entity BGE_RAY_NO_ENTITY, all floats 0.
 *                             Synchronises the world's stream.
 *   bge_world_raycast_all     offsets[0..n_rays] (offsets[i + 1] - offsets[i] hits of ray i at hits[offsets[i]..]) and *total,
 *                             the convention of bge_world_pairs: hits = NULL queries only the counts (offsets may be NULL too);
 *                             BGE_ERR_INVALID when cap < *total, *total (and offsets) still filled in.
 *   bge_world_raycast_device  device pointers: rays_device = bge_ray[n_rays], hits_device = bge_ray_hit[n_rays]; enqueued on the
 *                             world's stream, no synchronisation (the caller orders its own use of hits_device after it).
 *   n_rays = 0 is a no-op.  The entity indices of the world must stay below 2^30.
 */
typedef struct bge_ray {
    float origin[3];
    float direction[3];
    float max_distance;
    uint32_t layer_mask;
} bge_ray; /* 32 bytes */
enum bge_ray_kind { BGE_RAY_MISS = 0, BGE_RAY_BODY = 1, BGE_RAY_TRIGGER = 2, BGE_RAY_GROUND = 3 };
#define BGE_RAY_NO_ENTITY 0xffffffffu
typedef struct bge_ray_hit {
    uint32_t kind;   /* bge_ray_kind */
    uint32_t entity; /* entity index of the body or trigger; BGE_RAY_NO_ENTITY for the plane and for a miss */
    float fraction;
    float distance;
    float point[3];
    float normal[3];
} bge_ray_hit; /* 40 bytes */
BGE_API int bge_world_raycast(bge_world* world, uint64_t n_rays, const bge_ray* rays, bge_ray_hit* hits);
BGE_API int bge_world_raycast_all(bge_world* world, uint64_t n_rays, const bge_ray* rays, bge_ray_hit* hits, uint64_t cap,
                                  uint64_t* offsets, uint64_t* total);
BGE_API int bge_world_raycast_device(bge_world* world, uint64_t n_rays, const void* rays_device, void* hits_device);

/*
 * Sphere queries: a sphere swept along a segment (cast) and a sphere at rest (overlap) against the world the ray queries see, for a
 * batch at once.  NOT in the reference's PhysicsSystem: they are the two primitives its btKinematicCharacterController is made of
 * (a convex sweep, an overlap test; src/physics/PhysicsSystem.cpp:762) for the one shape that is exact in closed form against
 * every shape of the world.  The rules below are the specification.
 *   Objects, poses, Filter, tie order, Call order   those of the ray queries above, word for word: every rigid body in the world
 *             at the pose the last physics tick left, every live posed trigger ghost, the plane when it is on; an object is a
 *             candidate when (objGroup & layer_mask) != 0 && objMask != 0; object code = bodies by entity index, then ghosts by
 *             entity index, then the plane.
 *   Distance  dist(c, S) is the Euclidean distance from the point c to the solid shape S, 0 inside it.  Box: the sharp box of its
 *             half extents with margin (as for rays).  Capsule: the points within its radius R of its Y segment, so
 *             dist = max(0, |c - closest point of the segment| - R).  Plane: |c.y|.
 *   Cast      the centre moves along c(f) = origin + direction * max_distance * f, f in [0, 1] (direction is not normalised).
 *             Object S is hit at the smallest f with dist(c(f), S) = radius, provided dist(c(0), S) > radius: a sphere that
 *             STARTS TOUCHING OR OVERLAPPING a shape does not hit that shape (the ray rule "starts inside or on";
 *             bge_world_overlap_sphere finds those).  Said otherwise, the ray of the centre against the shape grown by radius: a
 *             capsule of radius R + radius; the ROUNDED box (sharp box + ball); the planes y = +-radius (from above: hit iff
 *             origin.y > radius and end.y < radius, f = (origin.y - radius) / (origin.y - end.y); mirrored from below;
 *             |origin.y| <= radius hits nothing).
 *   Hit       the record is bge_ray_hit: fraction = f, distance = f * max_distance (the ray definition), point = the point of S
 *             closest to c(f) (the contact point on the surface), normal = normalise(c(f) - point): on a box face the face
 *             normal, on an edge or a corner the rounded direction; for the plane point = (c.x, 0, c.z), normal +-y.
 *   No hit    the ray conditions (!(max_distance > 0), layer_mask == 0, direction == (0, 0, 0), any input not finite) and
 *             !(radius >= 0).  radius == 0 is a legal cast; it agrees with the ray query to rounding (not bit for bit: on an exact
 *             edge hit the box normal is defined differently).
 *   Closest   smallest f, ties to the lowest object code.   All hits: one record per object, each cast's list in (f, object code) order.
 *   Overlap   object S is reported iff dist(center, S) <= radius (plane: |center.y| <= radius), with that distance; each sphere's
 *             list in ascending object code.  A sphere with a non-finite input, radius < 0 or layer_mask == 0 reports nothing.
 *   bge_world_sphere_cast         hits[i] for casts[i]; a miss as for bge_world_raycast.  Synchronises the world's stream.
 *   bge_world_sphere_cast_all     count / cap / offsets / hits = NULL / BGE_ERR_INVALID when cap < *total: as bge_world_raycast_all.
 *   bge_world_sphere_cast_device  device pointers: casts_device = bge_sphere_cast[n], hits_device = bge_ray_hit[n]; enqueued on the
 *                                 world's stream, no synchronisation.
 *   bge_world_overlap_sphere      the list convention of bge_world_raycast_all with bge_overlap_hit records.
 *   n = 0 is a no-op.  The entity indices of the world must stay below 2^30.
 */
typedef struct bge_sphere_cast {
    float origin[3];
    float direction[3];
    float max_distance;
    float radius;
    uint32_t layer_mask;
    uint32_t reserved; /* 0 */
} bge_sphere_cast; /* 40 bytes */
typedef struct bge_sphere {
    float center[3];
    float radius;
    uint32_t layer_mask;
} bge_sphere; /* 20 bytes */
typedef struct bge_overlap_hit {
    uint32_t kind;   /* bge_ray_kind: BGE_RAY_BODY, BGE_RAY_TRIGGER or BGE_RAY_GROUND */
    uint32_t entity; /* entity index of the body or trigger; BGE_RAY_NO_ENTITY for the plane */
    float distance;  /* from the centre to the shape, 0 when the centre is inside it */
} bge_overlap_hit; /* 12 bytes */
BGE_API int bge_world_sphere_cast(bge_world* world, uint64_t n, const bge_sphere_cast* casts, bge_ray_hit* hits);
BGE_API int bge_world_sphere_cast_all(bge_world* world, uint64_t n, const bge_sphere_cast* casts, bge_ray_hit* hits, uint64_t cap,
                                      uint64_t* offsets, uint64_t* total);
BGE_API int bge_world_sphere_cast_device(bge_world* world, uint64_t n, const void* casts_device, void* hits_device);
BGE_API int bge_world_overlap_sphere(bge_world* world, uint64_t n, const bge_sphere* spheres, bge_overlap_hit* hits, uint64_t cap,
                                     uint64_t* offsets, uint64_t* total);

/*
 * Sphere moves: the core of a kinematic controller for a batch of spheres at once — move the sphere by a displacement, stop at
 * what it hits, slide what is left along the surface, probe for ground.  NOT in the reference's PhysicsSystem (its character is
 * Bullet's btKinematicCharacterController on a capsule, src/physics/PhysicsSystem.cpp:709-846).  A move is BGE_MOVE_SLIDES
 * rounds of bge_world_sphere_cast plus one probe cast, all on the device with no host round trip in between.  The rule below is
 * the specification.  All arithmetic is binary32, each line evaluated left to right with one rounding per
 * operation; j runs over x, y, z.
 *   Sees      Objects, poses, Filter, tie order and Call order are those of bge_world_sphere_cast, word for word: the mover sees
 *             the world only through that cast.
 *   Valid     a mover is valid iff every float of it is finite, radius >= 0, skin > 0, probe_distance >= 0 and layer_mask != 0.
 *             An invalid mover returns flags = BGE_MOVE_INVALID, position echoed, the kinds BGE_RAY_MISS, the entities
 *             BGE_RAY_NO_ENTITY, everything else 0.
 *   State     p = position, r = displacement, d0 = displacement, no previous normal, not finished.
 *   Rounds    for each of the BGE_MOVE_SLIDES rounds, unless finished:
 *             1. L2 = (r.x*r.x + r.y*r.y) + r.z*r.z.  If !(L2 > 1e-12f): r = 0, finished.
 *             2. Take the closest hit of the cast {origin p, direction r, max_distance 1, radius, layer_mask}.  On a miss:
 *                p_j = p_j + r_j, r = 0, finished.
 *             3. On a hit with fraction f and normal n:
 *                  L = sqrtf(L2)
 *                  a = -(((r.x*n.x + r.y*n.y) + r.z*n.z) / L);   if !(a >= 0.0625f) then a = 0.0625f
 *                  g = f - skin / (a * L);                       if !(g > 0) then g = 0
 *                  p_j = p_j + r_j * g
 *                n_hits += 1; hit_kind, hit_entity and hit_normal take the hit's kind, entity and normal.
 *             4. Leftover:  w = 1 - f;  l_j = r_j * w;  dn = (l.x*n.x + l.y*n.y) + l.z*n.z;  s_j = l_j - n_j * dn.
 *             5. Crease.  If there is a previous normal m and ((s.x*m.x + s.y*m.y) + s.z*m.z) < 0:
 *                  c = (m.y*n.z - m.z*n.y, m.z*n.x - m.x*n.z, m.x*n.y - m.y*n.x);  cc = (c.x*c.x + c.y*c.y) + c.z*c.z
 *                  if !(cc > 1e-12f): s = 0;  otherwise t = ((l.x*c.x + l.y*c.y) + l.z*c.z) / cc and s_j = c_j * t.
 *             6. A slide never turns against the asked direction: if !(((s.x*d0.x + s.y*d0.y) + s.z*d0.z) > 0): s = 0.
 *             7. r = s; the previous normal becomes n.
 *   After     if (r.x*r.x + r.y*r.y) + r.z*r.z > 1e-12f, BGE_MOVE_OUT_OF_SLIDES is set and remaining = r; otherwise remaining = 0.
 *             position = p.
 *   Probe     if probe_distance > 0, the cast {origin p, direction (0, -1, 0), max_distance probe_distance, radius, layer_mask}.
 *             On a hit BGE_MOVE_PROBE_HIT is set, ground_kind, ground_entity and ground_normal take the hit and ground_distance
 *             is the hit's distance; BGE_MOVE_GROUNDED is set iff additionally ground_normal[1] >= min_ground_ny.
 *   Skin      the cast ignores a shape the sphere starts touching, so a mover must never come to rest at distance radius from
 *             anything: it would fall through it in the next call.  The back-off by skin / a along the path keeps a gap of skin
 *             to a flat surface (a is the cosine of the approach).  The clamp at a = 1/16 bounds the back-off at grazing angles to
 *             16 skins of path, where the gap kept is then smaller than skin, never negative.  Choose skin well above the
 *             binary32 spacing at the scene's extent (1e-3 .. 1e-2 for a scene of a few hundred units).
 *   Not done  capsule or box movers; moving platforms; the result is not written into any Transform.  Stepping up over a kerb or a
 *             stair is bge_world_sphere_step_move ("Sphere step moves" below).  A sphere that STARTS touching or inside a shape is
 *             not this query's business (the cast does not see what it starts in): bge_world_sphere_recover below pushes it
 *             out first, so the order per frame is recover, then move.
 *   The query changes no world state.  n = 0 is a no-op.  A NULL argument with n > 0 is BGE_ERR_INVALID.  Before
 *   bge_world_set_topology it returns what bge_world_sphere_cast returns there.
 *   bge_world_sphere_move         results[i] for moves[i].  Synchronises the world's stream.
 *   bge_world_sphere_move_device  device pointers: moves_device = bge_sphere_move[n], results_device = bge_sphere_move_result[n],
 *                                 both 4-byte aligned (a misaligned pointer is BGE_ERR_INVALID); enqueued on the world's stream,
 *                                 no synchronisation.
 */
#define BGE_MOVE_SLIDES 4
typedef struct bge_sphere_move {
    float position[3];     /* centre before the move */
    float displacement[3]; /* asked motion of this call (the caller folds in walk direction, gravity, dt) */
    float radius;
    float skin;            /* > 0: the gap kept to what was hit */
    float probe_distance;  /* >= 0: length of the ground probe straight down after the move; 0 = no probe */
    float min_ground_ny;   /* GROUNDED needs ground normal.y >= this (cos of the max slope) */
    uint32_t layer_mask;
    uint32_t reserved;     /* 0 */
} bge_sphere_move; /* 48 bytes */
enum bge_move_flags { BGE_MOVE_INVALID = 1u, BGE_MOVE_GROUNDED = 2u, BGE_MOVE_OUT_OF_SLIDES = 4u, BGE_MOVE_PROBE_HIT = 8u };
typedef struct bge_sphere_move_result {
    float position[3];  /* centre after the move */
    float remaining[3]; /* displacement left unspent (zero unless OUT_OF_SLIDES) */
    uint32_t flags;     /* bge_move_flags */
    uint32_t n_hits;    /* rounds that hit something, 0 .. BGE_MOVE_SLIDES */
    uint32_t hit_kind;  /* last hit of the slides: bge_ray_kind; BGE_RAY_MISS / BGE_RAY_NO_ENTITY / 0 if none */
    uint32_t hit_entity;
    float hit_normal[3];
    uint32_t ground_kind; /* the probe's hit, same convention */
    uint32_t ground_entity;
    float ground_distance;
    float ground_normal[3];
    uint32_t reserved; /* 0 */
} bge_sphere_move_result; /* 80 bytes */
BGE_API int bge_world_sphere_move(bge_world* world, uint64_t n, const bge_sphere_move* moves, bge_sphere_move_result* results);
BGE_API int bge_world_sphere_move_device(bge_world* world, uint64_t n, const void* moves_device, void* results_device);

/*
 * Sphere step moves: a sphere move that steps up over low obstacles — what a caller of bge_world_sphere_move composes from an up
 * move, a forward move and a down move, done once on the device with no host round trip.  NOT in the reference's
 * PhysicsSystem.  The rule below is the specification.  All arithmetic is binary32, one rounding per operation, left to right, as
 * in "Sphere moves".
 *   Slide(p, d)  the State and the rounds 1-7 of "Sphere moves", word for word, run for BGE_MOVE_SLIDES rounds from p with
 *             r = d0 = d and no previous normal.  It yields p', r' (zero unless (r'.x*r'.x + r'.y*r'.y) + r'.z*r'.z > 1e-12f, then
 *             OUT_OF_SLIDES), n_hits, the last hit, and the normal n1 of the first round's hit.
 *   Cast      the closest hit of bge_world_sphere_cast with the mover's radius and layer_mask: Objects, poses, Filter, tie order,
 *             start rule and Call order are the cast's by construction.
 *   Valid     a mover is valid iff it is a valid bge_sphere_move and step_height is finite and >= 0.  An invalid mover returns the
 *             INVALID record of "Sphere moves", with step_rise = 0.
 *   Plain     P = Slide(position, displacement).
 *   Gate      BGE_MOVE_STEP_TRIED is set, and the stages below are run, iff step_height > 0, P.n_hits >= 1,
 *             n1.y < min_ground_ny (the first thing met is not walkable ground) and
 *             displacement.x*displacement.x + displacement.z*displacement.z > 1e-12f.
 *   Up        Cast {position, (0, 1, 0), max_distance step_height}.  Miss: u = step_height.  Hit at distance t: u = t - skin.
 *             If !(u > 0) the step fails.  q = (position.x, position.y + u, position.z).
 *   Forward   F = Slide(q, (displacement.x, 0, displacement.z)).
 *   Down      m = u + probe_distance.  Cast {F.p, (0, -1, 0), max_distance m}.  A miss fails the step; a hit whose normal.y is not
 *             >= min_ground_ny fails the step.  Otherwise e = distance - skin; if !(e > 0) then e = 0;
 *             S = (F.p.x, F.p.y - e, F.p.z).  The back-off is vertical, so the gap kept to a slope is skin * normal.y > 0.
 *   Gain      gs = (S.x - position.x)*displacement.x + (S.z - position.z)*displacement.z, and gp the same with P.p for S.  The
 *             step fails unless gs > gp.
 *   Result    if the step did not fail: BGE_MOVE_STEPPED is set, position = S; remaining, OUT_OF_SLIDES, n_hits and hit_* are
 *             those of F; step_rise = u.  Otherwise every field is that of P, and step_rise = 0.
 *   Probe     one probe from the chosen position, by the Probe rule of "Sphere moves": ground_*, PROBE_HIT and GROUNDED.
 *   Hence     with STEP_TRIED masked off, a record without STEPPED equals, byte for byte, what bge_world_sphere_move returns for
 *             the same 48 bytes read as a bge_sphere_move (whose reserved word it does not look at); step_height == 0 is
 *             therefore exactly the plain move.  A stepped result is reproducible from public calls: bge_world_sphere_cast up,
 *             bge_world_sphere_move with probe 0 forward, bge_world_sphere_cast down.  A low fence is hopped only when
 *             probe_distance reaches the ground behind it: Down looks u + probe_distance below F.p, and the fence was cleared by u.
 *   Example   radius 0.5, skin 0.01, min_ground_ny cos 45 degrees, plane on.  A Static box with half extents (2, 0.3, 2) at
 *             (3, 0.3, 0): top y = 0.6, near face x = 1.  Mover at (0, 0.51, 0), displacement (2, 0, 0), step_height 0.7, probe
 *             0.1.  Plain: the face head-on, P.p = (0.49, 0.51, 0), n1 = (-1, 0, 0): the gate passes.  Up: free, u = 0.7,
 *             q = (0, 1.21, 0).  Forward: the underside at 0.71 > 0.6 is free, F.p = (2, 1.21, 0).  Down: m = 0.8, the top is
 *             touched at centre y = 1.1, distance 0.11, normal (0, 1, 0): e = 0.10, S = (2, 1.11, 0).  Gain: gs = 4 > gp = 0.98.
 *             Result: position (2, 1.11, 0), flags STEP_TRIED | STEPPED | GROUNDED | PROBE_HIT, n_hits 0, hit_kind MISS,
 *             ground_kind BODY, entity 0, ground_distance 0.01, step_rise 0.7.
 *   Not done  capsule and box movers, moving platforms, writing into a Transform.
 *   The query changes no world state.  n = 0 is a no-op.  A NULL argument with n > 0 is BGE_ERR_INVALID.  n is at most 2^30 - 1
 *   (a pass asks two casts per mover).  Before bge_world_set_topology it returns what bge_world_sphere_cast returns there.
 *   bge_world_sphere_step_move         results[i] for moves[i].  Synchronises the world's stream.
 *   bge_world_sphere_step_move_device  device pointers: moves_device = bge_sphere_step_move[n], results_device =
 *                                      bge_sphere_step_result[n], both 4-byte aligned (a misaligned pointer is BGE_ERR_INVALID);
 *                                      enqueued on the world's stream, no synchronisation.
 */
typedef struct bge_sphere_step_move { /* bge_sphere_move with step_height where its reserved word is */
    float position[3];
    float displacement[3];
    float radius;
    float skin;
    float probe_distance;
    float min_ground_ny;
    uint32_t layer_mask;
    float step_height; /* >= 0: how far the sphere may rise to get over an obstacle; 0 = plain move */
} bge_sphere_step_move; /* 48 bytes */
enum bge_step_move_flags { BGE_MOVE_STEP_TRIED = 16u, BGE_MOVE_STEPPED = 32u }; /* two more bits of the result's flags word */
typedef struct bge_sphere_step_result { /* bge_sphere_move_result with step_rise where its reserved word is */
    float position[3];
    float remaining[3];
    uint32_t flags; /* bge_move_flags | bge_step_move_flags */
    uint32_t n_hits;
    uint32_t hit_kind;
    uint32_t hit_entity;
    float hit_normal[3];
    uint32_t ground_kind;
    uint32_t ground_entity;
    float ground_distance;
    float ground_normal[3];
    float step_rise; /* u of the Up stage when STEPPED, otherwise 0 */
} bge_sphere_step_result; /* 80 bytes */
BGE_API int bge_world_sphere_step_move(bge_world* world, uint64_t n, const bge_sphere_step_move* moves, bge_sphere_step_result* results);
BGE_API int bge_world_sphere_step_move_device(bge_world* world, uint64_t n, const void* moves_device, void* results_device);

/*
 * Sphere penetration and recovery: by how much and in which direction a sphere at rest reaches into the world
 * (bge_world_sphere_penetration), and the iteration that pushes it out (bge_world_sphere_recover) — what a mover needs when a crate
 * fell onto it, a platform moved into it or it was teleported, since bge_world_sphere_move does not see what it starts in.  NOT in
 * the reference's PhysicsSystem (Bullet's btKinematicCharacterController::recoverFromPenetration plays this part there).  The rules
 * below are the specification.  All arithmetic is binary32 with one rounding per operation; j runs over x, y, z.
 *   Sees      Objects, poses, Filter, object codes, tie order and Call order are those of bge_world_sphere_cast, word for word:
 *             rigid bodies at the pose of the last physics tick, live posed trigger ghosts, the plane when it is on; an object is
 *             a candidate iff (objGroup & layer_mask) != 0 && objMask != 0.
 *   Signed distance sd(c, S) and outward direction n(c, S).  q is c in the shape's frame, obtained as for dist(c, S) above.
 *             Box (the sharp box of the half extents with margin, h):
 *               if any |q_j| > h_j (outside): sd = dist(c, S), the value bge_world_overlap_sphere reports, bit for bit;
 *                 n = (q - closest point of the box) / sd, taken through the pose.
 *               otherwise (inside or on the surface): sd = -min_j (h_j - |q_j|); n is the box axis j of that minimum taken through
 *                 the pose, ties to the lowest j, with the sign of q_j (q_j == 0, either zero, counts as +).
 *             Capsule (radius R, Y segment): a = |q - closest point of the segment|, sd = a - R, n = (q - closest) / a through the
 *               pose; when !(a > 0), n is the capsule's local +x axis through the pose (and sd = -R).
 *             Plane (two-sided, as the casts treat it): sd = |c.y|; n = (0, 1, 0) when c.y >= 0 (so -0 goes up), otherwise
 *               (0, -1, 0): a centre below the plane is pushed further down.  The plane has no inside.
 *   Penetration   object S penetrates the sphere (center, radius) iff sd(center, S) <= radius: exactly the objects
 *             bge_world_overlap_sphere reports, whose distance is max(sd, 0).  depth = radius - sd (one subtraction; a zero depth
 *             is +0), so depth >= 0.  The answer is the object of the LARGEST depth, ties to the lowest object code: kind and
 *             entity as bge_overlap_hit, normal = n(center, S), point_j = center_j - normal_j * sd (on the surface).
 *   No hit    the conditions of bge_world_overlap_sphere: a non-finite input, radius < 0, layer_mask == 0, or no object
 *             penetrating.  The miss record has kind = BGE_RAY_MISS, entity = BGE_RAY_NO_ENTITY and every other word 0.
 *   Recover   A record is valid iff every float of it is finite, radius >= 0, skin > 0 and layer_mask != 0.  An invalid record
 *             returns flags = BGE_RECOVER_INVALID, position echoed, the kind BGE_RAY_MISS, the entity BGE_RAY_NO_ENTITY,
 *             everything else 0.
 *             State   p = position, not finished, n_pushes = 0.
 *             Rounds  for each of the BGE_RECOVER_ROUNDS rounds, unless finished:
 *                     1. Take the penetration query {p, radius, layer_mask}.
 *                     2. On a miss: finished.
 *                     3. On a hit with depth e and normal n:  t = e + skin;  p_j = p_j + n_j * t;  n_pushes += 1;  hit_kind,
 *                        hit_entity, hit_normal and hit_depth take the hit's kind, entity, normal and depth.
 *             After   if not finished, one more penetration query at p: a hit sets BGE_RECOVER_STUCK and remaining_depth is its
 *                     depth (hit_* stay those of the last push).
 *             Result  pushed_j = p_j - position_j; BGE_RECOVER_MOVED iff n_pushes > 0; position = p.
 *             A sphere clear of everything comes back unchanged with flags 0.  After one push against a flat surface the gap is
 *             skin, so the cast sees that surface again.  A wedge or a slot narrower than the sphere may end STUCK; the result
 *             is deterministic either way.  (Bullet's character controller also recovers in at most 4 iterations.)
 *   The queries change no world state.  n = 0 is a no-op.  A NULL argument with n > 0 is BGE_ERR_INVALID.  Before
 *   bge_world_set_topology they return what bge_world_overlap_sphere returns there.
 *   bge_world_sphere_penetration         hits[i] for spheres[i].  Synchronises the world's stream.
 *   bge_world_sphere_penetration_device  device pointers: spheres_device = bge_sphere[n], hits_device = bge_penetration_hit[n],
 *                                        both 4-byte aligned (a misaligned pointer is BGE_ERR_INVALID); enqueued on the world's
 *                                        stream, no synchronisation.
 *   bge_world_sphere_recover             results[i] for records[i].  Synchronises the world's stream.
 *   bge_world_sphere_recover_device      device pointers: records_device = bge_sphere_recover[n], results_device =
 *                                        bge_sphere_recover_result[n], aligned, enqueued and not synchronised likewise.
 */
#define BGE_RECOVER_ROUNDS 4
typedef struct bge_penetration_hit {
    uint32_t kind;     /* bge_ray_kind: BGE_RAY_BODY, BGE_RAY_TRIGGER or BGE_RAY_GROUND; BGE_RAY_MISS when nothing penetrates */
    uint32_t entity;   /* entity index of the body or trigger; BGE_RAY_NO_ENTITY for the plane and for a miss */
    float depth;       /* radius - sd, >= 0 */
    float point[3];    /* center - normal * sd: on the surface */
    float normal[3];   /* n(center, S), unit: the way out */
    uint32_t reserved; /* 0 */
} bge_penetration_hit; /* 40 bytes */
typedef struct bge_sphere_recover {
    float position[3];
    float radius;
    float skin;        /* > 0: the gap left to what it was pushed out of */
    uint32_t layer_mask;
    uint32_t reserved; /* 0 */
} bge_sphere_recover; /* 28 bytes */
enum bge_recover_flags { BGE_RECOVER_INVALID = 1u, BGE_RECOVER_MOVED = 2u, BGE_RECOVER_STUCK = 4u };
typedef struct bge_sphere_recover_result {
    float position[3];     /* centre after the recovery */
    float pushed[3];       /* position after - position before */
    uint32_t flags;        /* bge_recover_flags */
    uint32_t n_pushes;     /* 0 .. BGE_RECOVER_ROUNDS */
    uint32_t hit_kind;     /* the last push: bge_ray_kind; BGE_RAY_MISS / BGE_RAY_NO_ENTITY / 0 if none */
    uint32_t hit_entity;
    float hit_normal[3];
    float hit_depth;
    float remaining_depth; /* with BGE_RECOVER_STUCK: the depth still found after the last round; otherwise 0 */
    uint32_t reserved;     /* 0 */
} bge_sphere_recover_result; /* 64 bytes */
BGE_API int bge_world_sphere_penetration(bge_world* world, uint64_t n, const bge_sphere* spheres, bge_penetration_hit* hits);
BGE_API int bge_world_sphere_penetration_device(bge_world* world, uint64_t n, const void* spheres_device, void* hits_device);
BGE_API int bge_world_sphere_recover(bge_world* world, uint64_t n, const bge_sphere_recover* records, bge_sphere_recover_result* results);
BGE_API int bge_world_sphere_recover_device(bge_world* world, uint64_t n, const void* records_device, void* results_device);

/*
 * Characters: a set of sphere characters that lives on the device between frames — position, vertical velocity and whether the
 * character stands on ground — with gravity, jump, the fall-speed clamp, the snap that keeps a walker on a downward slope, and one
 * call that runs a frame, or several sub-steps, for all of them with no host round trip.  An extension, as every
 * sphere mover: the reference drives one btKinematicCharacterController on a capsule (src/physics/PhysicsSystem.cpp:709-846); the
 * surface here (walk displacement, jump, on-ground, warp, gravity, jump speed, fall speed, max slope, step height) and the meaning
 * of its knobs follow that use, the shape is a sphere, and the rule below is the specification.  All arithmetic is binary32, one
 * rounding per operation, left to right.
 *   Recover, StepMove  are bge_world_sphere_recover and bge_world_sphere_step_move, word for word.  The character sees the world
 *             only through them, so Objects, poses (the last physics tick), Filter and tie order are theirs by construction.
 *   One step of length dt, per character:
 *   Input     walk_x and walk_z are the level displacement of this step (what setWalkDirection takes: direction * speed * dt).
 *             BGE_CHAR_BUTTON_JUMP is an edge: the first step of an update call reads it and clears it, whether or not it led to
 *             a jump; the further steps of that call see it clear.
 *   Valid     the step is valid iff walk_x and walk_z are finite and neither the recovery nor the step move below comes back
 *             INVALID.  An invalid step sets BGE_CHAR_INVALID, leaves position, vertical_velocity and GROUNDED as they were before
 *             the step and clears every other flag; ground_* and hit_* take the miss convention (BGE_RAY_MISS, BGE_RAY_NO_ENTITY,
 *             0), step_rise and recovered are 0, steps += 1.
 *   Recover   R = Recover{position, radius, skin, layer_mask}.  p = R.position.  RECOVERED iff R is MOVED, STUCK iff R is STUCK,
 *             recovered = R.pushed.
 *   Vertical  was = GROUNDED before the step.  jumped = JUMP && was.
 *             If jumped: vv = jump_speed.  Else if was: vv = 0, the character is walking and dy = 0.
 *             When not walking:  vv = vv - gravity*dt;  if vv > jump_speed then vv = jump_speed;
 *                                if vv < -fall_speed then vv = -fall_speed;  dy = vv*dt.
 *   Move      M = StepMove{p, (walk_x, dy, walk_z), radius, skin, probe_distance, min_ground_ny, layer_mask,
 *             step_height if walking else 0}.  q = M.position.
 *   Ground    grounded = M.GROUNDED && !(vv > 0).  If grounded: e = M.ground_distance - skin; if !(e > 0) then e = 0;
 *             q.y = q.y - e; vv = 0.  This is the vertical back-off of the step move's Down stage, so the gap kept to a slope is
 *             skin * normal.y > 0.  LANDED iff grounded && !was.
 *   Head      if vv > 0 && M.n_hits >= 1 && M.hit_normal[1] < 0: vv = 0 and HEAD_BUMP is set.
 *   State     position = q, vertical_velocity = vv; the flags GROUNDED, JUMPED, LANDED, HEAD_BUMP, RECOVERED, STUCK, and STEPPED and
 *             OUT_OF_SLIDES from M; ground_kind, ground_entity and ground_normal from M's probe (its miss convention where it
 *             found nothing); hit_kind, hit_entity, hit_normal and step_rise from M; recovered; steps += 1.
 *   Hence     a walker stays on a downward slope only while probe_distance covers the drop of one step: a walker moves level, the
 *             probe finds the slope below and Ground brings it down; where the probe misses, GROUNDED is lost and the character
 *             falls from the next step on.  probe_distance = 0 never grounds.  Step-up happens only while walking (a character in
 *             the air asks step_height 0, the plain move).  A character that walks off an edge loses GROUNDED without JUMPED.
 *             A kerb is stepped in the step whose walk brings the centre far enough over its edge that the Down stage lands on
 *             walkable ground (within radius * sqrt(1 - min_ground_ny^2) of the edge, level): a walk much shorter than that per
 *             step rests at the kerb's face.  A sphere whose radius exceeds the kerb's height meets its upper edge, not its face,
 *             and may roll over it by the plain slide.
 *   Example   radius 0.5, skin 0.01, gravity 9.81, jump_speed 5, fall_speed 30, probe_distance 0.1, dt = 1/60 (0.0166667), plane
 *             on.  A character GROUNDED at (0, 0.51, 0) with JUMP set and no walk.  Step 1: jumped, vv = 5 - 9.81 dt = 4.8365,
 *             dy = 0.0806083, nothing is met: position y = 0.5906083; the probe finds the plane 0.0906 below but vv > 0: not
 *             grounded; flags JUMPED.  Step 2: vv = 4.673, dy = 0.0778833, y = 0.6684917, flags 0.  Step 3: vv = 4.5095,
 *             dy = 0.0751583, y = 0.74365.  vv turns negative in step 31; in step 60 the move ends 0.02325 above the touching
 *             height, the probe finds the plane at that distance, e = 0.01325: y = 0.51, vv = 0, flags GROUNDED | LANDED.
 *             The kerb of "Sphere step moves" (min_ground_ny cos 45 degrees, step_height 0.7): a character GROUNDED at
 *             (0, 0.51, 0) with walk (2, 0): walking, dy = 0, M is that example's result: position (2, 1.11, 0), ground_distance
 *             0.01, e = 0: flags GROUNDED | STEPPED, step_rise 0.7, ground_kind BODY, entity 0.
 *   Not done  capsule characters; writing into a Transform on the device (the adapter does that on the host).  Dynamic bodies are
 *             pushed only once "Character push" below is switched on, and what remains open there is a reaction on the character
 *             and a push at the contact point.  A platform that moves INTO a character pushes it out through Recover; one that moves away from or along
 *             under a grounded character carries it only once "Character platform riding" below is switched on, and what remains
 *             open there is a swept carry and inherited velocity.  Trigger volumes report characters through "Character trigger events" below,
 *             with what remains open there: the box is the sphere's, not a capsule's; the world's own bge_world_trigger_events
 *             still does not see characters; characters do not report each other.
 *   Characters are not bodies: no query sees them, they see each other only through "Crowd separation" below once it is switched on
 *   (a push; they do not block each other's sweeps), and no call here changes any other world state — except that, once
 *   "Character push" below is switched on, an update call changes the velocities and the activation of the Dynamic bodies pushed.
 *   bge_world_characters_create   replaces the set with n characters made from descs; n = 0 removes it (descs may then be NULL).
 *                                 Every desc is checked on the host: every float finite, radius >= 0, skin > 0, step_height >= 0,
 *                                 probe_distance >= 0, gravity >= 0, jump_speed >= 0, fall_speed > 0, layer_mask != 0; a bad desc is
 *                                 BGE_ERR_INVALID with its index in bge_last_error, and the set is left as it was.  Characters start
 *                                 at desc.position, not grounded, vertical_velocity 0, steps 0, inputs zero.  n is at most 2^30 - 1
 *                                 (the step move's bound).  May be called before bge_world_set_topology.
 *   bge_world_characters_set_input         inputs[0 .. count) for characters first .. first + count (host memory).
 *   bge_world_characters_set_input_device  the same from a device pointer, 4-byte aligned (a misaligned pointer is
 *                                 BGE_ERR_INVALID); enqueued on the world's stream, no synchronisation.  A range outside the set is
 *                                 BGE_ERR_INVALID for both.
 *   bge_world_characters_warp     for k < count: character index[k] takes position3[3k ..], vertical_velocity 0 and loses GROUNDED,
 *                                 as warp does in the reference (:1315).  Positions must be finite and indices inside the set.
 *   bge_world_characters_update   dt finite and > 0 and steps >= 1, otherwise BGE_ERR_INVALID.  Enqueues `steps` steps on the
 *                                 world's stream: no synchronisation and nothing read in between.  With no characters it is a
 *                                 no-op; with characters before bge_world_set_topology it returns what bge_world_sphere_cast returns
 *                                 there.  A step is 5 penetration passes and 7 sphere-cast passes over the world
 *                                 (4 of them over two casts per character).
 *   bge_world_characters_download states[0 .. count) of characters first .. first + count.  Synchronises the world's stream.
 *   bge_world_characters_state_device  the resident bge_character_state[n] (NULL and 0 without characters), valid until the next
 *                                 bge_world_characters_create; reads must be ordered after the world's stream.
 */
typedef struct bge_character_desc {
    float position[3];    /* where the character starts */
    float radius;
    float skin;           /* > 0 */
    float step_height;    /* >= 0: the kerb a walking character gets over; 0 = none */
    float min_ground_ny;  /* GROUNDED needs ground normal.y >= this (cos of the max slope) */
    float probe_distance; /* >= 0: how far below itself the character looks for ground; 0 never grounds */
    float gravity;        /* >= 0, downwards */
    float jump_speed;     /* >= 0: vertical_velocity after a jump, and its upper clamp */
    float fall_speed;     /* > 0: vertical_velocity is never below -fall_speed */
    uint32_t layer_mask;
} bge_character_desc; /* 48 bytes */
enum bge_character_buttons { BGE_CHAR_BUTTON_JUMP = 1u };
typedef struct bge_character_input {
    float walk_x, walk_z; /* level displacement of one step */
    uint32_t buttons;     /* bge_character_buttons: edges, cleared by the step that reads them */
    uint32_t reserved;    /* 0 */
} bge_character_input; /* 16 bytes */
enum bge_character_flags {
    BGE_CHAR_INVALID = 1u, BGE_CHAR_GROUNDED = 2u, BGE_CHAR_JUMPED = 4u, BGE_CHAR_LANDED = 8u, BGE_CHAR_HEAD_BUMP = 16u,
    BGE_CHAR_RECOVERED = 32u, BGE_CHAR_STUCK = 64u, BGE_CHAR_STEPPED = 128u, BGE_CHAR_OUT_OF_SLIDES = 256u
};
typedef struct bge_character_state {
    float position[3];
    float vertical_velocity;
    uint32_t flags;        /* bge_character_flags of the last step (GROUNDED is also state) */
    uint32_t ground_kind;  /* the last step's ground probe: bge_ray_kind; BGE_RAY_MISS / BGE_RAY_NO_ENTITY / 0 if none */
    uint32_t ground_entity;
    float ground_normal[3];
    uint32_t hit_kind;     /* the last hit of the last step's slides, same convention */
    uint32_t hit_entity;
    float hit_normal[3];
    float step_rise;       /* with STEPPED: how far the last step rose */
    float recovered[3];    /* what the last step's recovery pushed the character by */
    uint32_t steps;        /* steps run since the set was created */
} bge_character_state; /* 80 bytes */
BGE_API int bge_world_characters_create(bge_world* world, uint64_t n, const bge_character_desc* descs);
BGE_API int bge_world_characters_set_input(bge_world* world, uint64_t first, uint64_t count, const bge_character_input* inputs);
BGE_API int bge_world_characters_set_input_device(bge_world* world, uint64_t first, uint64_t count, const void* inputs_device);
BGE_API int bge_world_characters_warp(bge_world* world, uint64_t count, const uint32_t* index, const float* position3);
BGE_API int bge_world_characters_update(bge_world* world, float dt, uint32_t steps);
BGE_API int bge_world_characters_download(bge_world* world, uint64_t first, uint64_t count, bge_character_state* states);
BGE_API int bge_world_characters_state_device(bge_world* world, void** states_device, uint64_t* n);

/*
 * Character trigger events: Enter / Stay / Exit of the device's characters against the trigger volumes, made on the device once
 * per bge_world_characters_update call.  In the reference the character is a btPairCachingGhostObject of group
 * kDefaultCharacterLayer = 2 and mask all (src/physics/PhysicsSystem.cpp:741-766), every trigger ghost's pair cache lists it and
 * ProcessTriggerEvents (:1017-1074) publishes its events once per frame.  Opt-in: until bge_world_characters_watch_triggers turns
 * the watch on, every other call does what it did without this section.  The rule below is the specification.
 *   Character box  for a character at p with radius r, on axis a: lower corner (p[a] - r) - 0.02f, upper corner (p[a] + r) + 0.02f;
 *             binary32, one rounding per operation, left to right: the sphere's AABB plus updateSingleAabb's contact threshold.
 *   Trigger box    the fed AABB of the trigger as the last BGE_TICK_BROADPHASE tick posed it; for a ghost whose entity lost its
 *             Transform, the frozen box.  bge_world_trigger_boxes returns these boxes.
 *   Overlap   on every axis tmin <= cmax && tmax >= cmin: closed intervals (the test of the world's own trigger pass).
 *   Filter    (trigger.layer & char.mask) != 0 && (char.group & trigger.mask) != 0.  Group and mask are per character; NULL arrays
 *             mean group 2 and mask 0xffffffff.  A character with group 0 overlaps nothing.
 *   When      once per bge_world_characters_update call, after its last step, from the positions that step left (not per step: a
 *             volume crossed inside one call is not reported).  A BGE_CHAR_INVALID character is tested where it stands.
 *   Which     exactly the ghosts the queries see at that call: active, and posed by a tick or frozen.  A trigger that is not among
 *             them during a call is skipped: it is not tested, produces no event, and its remembered overlaps stay as they are.
 *   Events    for each such trigger, in the order of the uploaded trigger array, with cur = overlapping now and prev = remembered:
 *             first, in ascending character index, BGE_CHAR_TRIGGER_ENTER for cur & ~prev and BGE_CHAR_TRIGGER_STAY for cur & prev;
 *             then, in ascending character index, BGE_CHAR_TRIGGER_EXIT for prev & ~cur; then remembered := cur.  Without
 *             BGE_CHAR_TRIGGER_STAY_EVENTS the Stay records are left out and nothing else changes.  (The reference's order inside
 *             one trigger is that of an unordered_set; this fixes one.)  record.trigger is the trigger's entity index,
 *             record.character the index in the set.
 *   The list  is that of the last update call: each call replaces it, fetching does not clear it.
 *   one_shot  has no effect here, and no call of this section changes the trigger set or any other world state: consuming a
 *             one-shot trigger is the caller's job (the adapter does it).
 *   bge_world_upload_triggers     a trigger that was present before with the same entity, layer and mask keeps its remembered
 *                                 characters, any other starts empty; no Exit is reported for a removed trigger (the rule for
 *                                 remembered bodies).  With the watch on it synchronises the world's stream.
 *   bge_world_characters_create   turns the watch off and forgets the remembered sets and the list.
 *   bge_world_characters_warp     does nothing special: the next update call reports what the new position gives.
 *   Not done  the box is the sphere's, not a capsule's; characters stay invisible to the world's own bge_world_trigger_events;
 *             characters do not report each other.
 *   bge_world_characters_watch_triggers  n must equal the set's size; n = 0 turns the watch off (group and mask may be NULL).
 *                                 event_capacity = 0 picks n + 1024.  Calling it again replaces the filters and keeps the remembered
 *                                 sets and the list (the list's capacity only grows).  BGE_ERR_INVALID for a wrong n or unknown flag
 *                                 bits.  BGE_ERR_UNSUPPORTED where a bitmap, triggers x ceil(n / 64) 64-bit words, would exceed 2^28
 *                                 words, or with more than 65535 * 64 triggers; bge_world_upload_triggers answers the same, before
 *                                 it changes anything, for a trigger array that would.  Synchronises the world's stream.
 *   bge_world_characters_trigger_events  the list of the last update call into out[0 .. cap), and its length in total (out = NULL
 *                                 asks for total only).  Synchronises the world's stream.  If the call found more events than the
 *                                 device list holds, the list is grown and made again from the two bitmaps: nothing is lost, and the
 *                                 new capacity stays.  More than 2^32 - 2 events in one call is BGE_ERR_UNSUPPORTED.  total is 0
 *                                 while the watch is off.
 *   bge_world_characters_trigger_events_device  the resident list, its 4-byte count and the list's capacity in records, for a
 *                                 consumer on the device (NULL, NULL, 0 while the watch is off).  count may exceed capacity: records
 *                                 beyond capacity are not written.  Valid until the next bge_world_characters_watch_triggers,
 *                                 bge_world_characters_create, bge_world_upload_triggers or a host fetch that grows the list; reads
 *                                 must be ordered after the world's stream.
 *   bge_world_characters_trigger_overlaps      the remembered set as pairs2[2k] = trigger entity, pairs2[2k + 1] = character
 *                                 index, sorted by trigger array order and then by character; at most cap pairs are written, total
 *                                 is their number.  Synchronises the world's stream.
 *   bge_world_characters_set_trigger_overlaps  replaces the remembered set by `count` such pairs (any order).  A pair naming an
 *                                 entity that carries no trigger or an index outside the set (every index while the watch is off)
 *                                 is BGE_ERR_INVALID, and the set is left as it was.  For save / load and re-creating the set.
 *   bge_world_trigger_boxes       aabb6[6k ..] = the fed AABB (min xyz, max xyz) of the trigger on entity_index[k] and listed[k] = 1
 *                                 where that trigger is in the queries' ghost list now; otherwise listed[k] = 0 and the empty box
 *                                 (+inf x 3, -inf x 3).  Read-only; synchronises the world's stream.  aabb6 or listed may be NULL.
 */
enum bge_character_trigger_event_type { BGE_CHAR_TRIGGER_ENTER = 0, BGE_CHAR_TRIGGER_STAY = 1, BGE_CHAR_TRIGGER_EXIT = 2 };
enum bge_character_trigger_flags { BGE_CHAR_TRIGGER_STAY_EVENTS = 1u };
typedef struct bge_character_trigger_event {
    uint32_t type;      /* bge_character_trigger_event_type */
    uint32_t trigger;   /* the trigger's entity index */
    uint32_t character; /* index in the character set */
} bge_character_trigger_event; /* 12 bytes */
BGE_API int bge_world_characters_watch_triggers(bge_world* world, uint64_t n, const uint32_t* group, const uint32_t* mask, uint32_t flags,
                                                uint64_t event_capacity);
BGE_API int bge_world_characters_trigger_events(bge_world* world, bge_character_trigger_event* out, uint64_t cap, uint64_t* total);
BGE_API int bge_world_characters_trigger_events_device(bge_world* world, void** events, void** count, uint64_t* capacity);
BGE_API int bge_world_characters_trigger_overlaps(bge_world* world, uint64_t cap, uint32_t* pairs2, uint64_t* total);
BGE_API int bge_world_characters_set_trigger_overlaps(bge_world* world, uint64_t count, const uint32_t* pairs2);
BGE_API int bge_world_trigger_boxes(bge_world* world, uint64_t count, const uint32_t* entity_index, float* aabb6, uint8_t* listed);

/*
 * Character platform riding: a character that stands on a body moves with it.  Each character remembers the body
 * it stood on when the last bge_world_characters_update call ended and that body's pose (the anchor); the next call begins by
 * putting the character where it was in that body's frame.  Opt-in: until bge_world_characters_ride switches it on, every other
 * call does byte for byte what it did without this section.  The rule below is the specification.  All arithmetic is binary32, one
 * rounding per operation, in the order written.
 *   Pose      of a body: its position and its quaternion (xyzw) as the queries see them at that call: the position is what
 *             bge_world_download_pose returns, the quaternion what bge_world_download_bodies returns.
 *   Present   a body is present exactly when the queries' body pass would load it: its type is not BGE_BODY_NONE and it has not
 *             been uploaded since the last physics tick.
 *   Rideable  a present body is rideable when it is Static or Kinematic; with BGE_CHAR_RIDE_DYNAMIC a Dynamic body is rideable too.
 *   Carry     once per bge_world_characters_update call, before its first step.  The stages run in order and the first that applies
 *             decides:
 *             1. flags = 0, carried = 0, turn = (0, 0, 0, 1).
 *             2. If the character is not GROUNDED or entity == BGE_RAY_NO_ENTITY: nothing more.  (A warp clears GROUNDED, so a
 *                warped character is never carried.)
 *             3. If the anchor body is no longer present or no longer rideable: flags = BGE_CHAR_RIDE_LOST, the position stays.
 *             4. If the body's current pose equals the anchor pose word for word (7 words): nothing more.  A world that did not move
 *                stays byte-identical to one with riding off.
 *             5. Otherwise, with p the character's position, (a_p, a_q) the anchor pose and (c_p, c_q) the current pose:
 *                  l = rot(conj(a_q), p - a_p);  t = c_p + rot(c_q, l);  carried = t - p;  turn = mul(c_q, conj(a_q))
 *                If every component of t is finite: position = t, flags = BGE_CHAR_RIDE_CARRIED; vertical_velocity and the state's
 *                flags stay.  Otherwise flags = BGE_CHAR_RIDE_LOST, the position stays, carried stays 0 and turn the identity.
 *             conj negates x, y and z.  rot(q, v) is
 *                  tx = (q.y*v.z - q.z*v.y)*2;  ty = (q.z*v.x - q.x*v.z)*2;  tz = (q.x*v.y - q.y*v.x)*2;
 *                  r.x = (v.x + q.w*tx) + (q.y*tz - q.z*ty);
 *                  r.y = (v.y + q.w*ty) + (q.z*tx - q.x*tz);
 *                  r.z = (v.z + q.w*tz) + (q.x*ty - q.y*tx)
 *             and mul(p, q) is
 *                  x = ((p.w*q.x + p.x*q.w) + p.y*q.z) - p.z*q.y
 *                  y = ((p.w*q.y + p.y*q.w) + p.z*q.x) - p.x*q.z
 *                  z = ((p.w*q.z + p.z*q.w) + p.x*q.y) - p.y*q.x
 *                  w = ((p.w*q.w - p.x*q.x) - p.y*q.y) - p.z*q.z
 *             The steps then run as in "Characters"; the first step's Recover resolves whatever the carry put the character into.
 *   Anchor    once per call, after its last step and before the trigger events.  If the state is GROUNDED, ground_kind is
 *             BGE_RAY_BODY and that body is rideable: entity = ground_entity and the anchor pose is that body's pose now.  Otherwise
 *             entity = BGE_RAY_NO_ENTITY and the anchor words are 0.  (An INVALID last step leaves ground_kind MISS: no anchor.)
 *   Hence     the plane and trigger ghosts are never ridden.  A character that jumped or walked off is not carried, and the platform
 *             leaves without it.  The character keeps no horizontal velocity when it leaves a platform.  turn is for the caller's
 *             facing: the device keeps none.
 *   Example   a level box with its top at y = 1, a character of radius 0.5 and skin 0.01 GROUNDED on it at (1, 1.51, 0), anchor
 *             pose ((0, 0.5, 0), identity).  The box moves to (0.25, 0.5, 0): l = (1, 1.01, 0), t = (1.25, 1.51, 0), carried =
 *             (0.25, 0, 0), turn the identity.  The box instead turns by pi/8 about y, c_q = (0, 0.19509, 0, 0.98079): t =
 *             (0.92388, 1.51, -0.38268), turn = c_q.
 *   Forgetting  bge_world_characters_create switches riding off and drops the records.  bge_world_set_topology clears every anchor.
 *             bge_world_upload_bodies over entities [first, first + count) clears the anchors whose entity lies in that range
 *             (bge_world_upload_bodies_indexed: the entities of its list, run by run of consecutive indices; a list of more than
 *             16 runs is taken as the span from its lowest to its highest index): an entity index that gets a new body must not
 *             carry anyone by the difference between two unrelated poses.  Both clears are enqueued on the world's stream.
 *   Not done  a swept carry: Carry is a teleport, so a carry longer than a wall is thick passes through the wall; inherited
 *             velocity; capsule characters; pushing Dynamic bodies.
 *   bge_world_characters_ride     flags = BGE_CHAR_RIDE_ON, optionally | BGE_CHAR_RIDE_DYNAMIC; 0 switches riding off and drops the
 *                                 records.  Unknown bits, DYNAMIC without ON, and ON with no character set are BGE_ERR_INVALID.
 *                                 Switching on allocates the records and clears them (no anchor); calling it again while riding is
 *                                 on changes only the flags and keeps the anchors.  With riding on an update call makes two more
 *                                 launches (not two more per step); nothing is read back.
 *   bge_world_characters_rides    out[0 .. count) = the records of characters first .. first + count.  Synchronises the world's
 *                                 stream.  A range outside the set is BGE_ERR_INVALID, and so is any count > 0 while riding is off.
 *   bge_world_characters_rides_device  the resident bge_character_ride[n] (NULL and 0 while riding is off), valid until the next
 *                                 bge_world_characters_ride(0) or bge_world_characters_create; reads must be ordered after the
 *                                 world's stream.
 */
enum bge_character_ride_mode { BGE_CHAR_RIDE_ON = 1u, BGE_CHAR_RIDE_DYNAMIC = 2u };
enum bge_character_ride_flags { BGE_CHAR_RIDE_CARRIED = 1u, BGE_CHAR_RIDE_LOST = 2u };
typedef struct bge_character_ride {
    uint32_t flags;           /* bge_character_ride_flags of the last update call */
    uint32_t entity;          /* the anchor: the body stood on when the last call ended; BGE_RAY_NO_ENTITY if none */
    float anchor_position[3]; /* that body's pose as that call saw it */
    float anchor_rotation[4]; /* xyzw */
    float carried[3];         /* what Carry added to the position in the last call; 0 if nothing */
    float turn[4];            /* xyzw: the body's rotation since the anchor, cur * conj(anchor); (0, 0, 0, 1) if nothing */
} bge_character_ride; /* 64 bytes, 4-byte aligned, moved word by word like every character record */
BGE_API int bge_world_characters_ride(bge_world* world, uint32_t flags);
BGE_API int bge_world_characters_rides(bge_world* world, uint64_t first, uint64_t count, bge_character_ride* out);
BGE_API int bge_world_characters_rides_device(bge_world* world, void** rides, uint64_t* n);

/*
 * Crowd separation: spheres of a batch push each other apart, and so do the device's characters once switched on (DESIGN.md
 * 4.23).  In the reference every character's ghost is in the Bullet world with group 2 and mask all, so the sweeps of
 * btKinematicCharacterController see the other characters and characters block each other; here the characters part by a level
 * push at the head of every step.  The rule below is the specification.  All arithmetic is binary32, one rounding per operation,
 * left to right, as in "Sphere moves"; sqrtf and / are the correctly rounded ones.
 *   Crowd query  a stateless query over a batch of n spheres against EACH OTHER: of the world it uses only the stream and the device.
 *   Valid     a sphere is valid iff its four floats are finite and radius >= 0.  An invalid sphere gets flags = BGE_CROWD_INVALID,
 *             other = BGE_RAY_NO_ENTITY and every other word 0, and it is not there for the others.
 *   Pair      for i != j, both valid: a candidate iff (group_i & mask_j) != 0 && (group_j & mask_i) != 0.  Then
 *                  d[k] = c_i[k] - c_j[k];  d2 = (d.x*d.x + d.y*d.y) + d.z*d.z;  R = r_i + r_j;  depth = R - sqrtf(d2)
 *             and the pair overlaps iff depth > 0.  Both ends compute the same depth, bit for bit.
 *   Answer    for i: n_overlaps = the number of overlapping j; other = the j of the LARGEST depth, ties to the lowest j (the rule of
 *             bge_world_sphere_penetration); depth = that depth.  With no overlap: flags 0, other = BGE_RAY_NO_ENTITY, the rest 0.
 *   Push      is level, so a crowd never climbs onto itself.  With d taken against `other`:
 *                  hl2 = d.x*d.x + d.z*d.z
 *                  if hl2 > 1e-12f:  hl = sqrtf(hl2);  m = (d.x / hl, 0, d.z / hl)
 *                  otherwise         m = (i < other ? 1 : -1, 0, 0)      coincident or stacked centres part by index
 *                  t = depth * 0.5f;  if max_push > 0 && t > max_push:  t = max_push and BGE_CROWD_CLAMPED is set
 *                  push = (m.x*t, +0, m.z*t) and BGE_CROWD_PUSHED is set
 *   Hence     the answer depends on nothing but the batch: not on the search structure and not on the order in which candidates
 *             are met.  Every field is a maximum with a stated tie or an integer count.  The same call gives the same bytes every
 *             time.
 *   Example   spheres of radius 0.5 at (0, 0, 0) and (0.6, 0, 0): d2 = 0.36, depth = 1 - 0.6 = 0.4, t = 0.2; sphere 0 gets other 1,
 *             push (-0.2, 0, 0), sphere 1 gets other 0, push (0.2, 0, 0); applied, the centres are 1 apart: touching.
 *   bge_world_crowd_query         hits[0 .. n) for spheres[0 .. n) (host memory).  max_push must be finite and >= 0, otherwise
 *                                 BGE_ERR_INVALID; 0 means no limit.  n = 0 is a no-op; NULL with n > 0 is BGE_ERR_INVALID; n is at
 *                                 most 2^30 - 1.  Synchronises the world's stream.  Changes no world state and works before
 *                                 bge_world_set_topology.
 *   bge_world_crowd_query_device  the same from and to device pointers, 4-byte aligned (a misaligned pointer is BGE_ERR_INVALID);
 *                                 enqueued on the world's stream, no synchronisation, nothing read back.
 *   BGE_CROWD_GRID_MIN            (environment, read per call; default 256) batches of fewer spheres are answered by all pairs, larger
 *                                 ones through a hashed grid.  Both give the same bytes.
 * Characters.  Opt-in: until bge_world_characters_crowd switches it on, every call does byte for byte what it does without this
 * section.
 *   Separate  with the crowd on, every step of bge_world_characters_update begins with the stage Separate, before Recover: the crowd
 *             query over {state.position, desc.radius, group, mask} of ALL characters as they stand (in the first step that is
 *             after the riding Carry).  A BGE_CHAR_INVALID character still stands where it is and takes part.
 *   Apply     for a character whose hit is PUSHED: position.x = position.x + push.x, position.z = position.z + push.z, and nothing
 *             else of the state changes.  A character that is not PUSHED is not touched at all: a set in which nobody overlaps gives
 *             the same bytes as with the crowd off, a -0 coordinate included.  The step then runs as in "Characters" from that
 *             position.
 *   Ordering  Separate comes first, so the step's own Recover and Move have the last word: a character pushed into a wall is pushed
 *             out of it in the same step, and after an update call no character is inside the world; two may still overlap each
 *             other by what the last step walked.  Ride anchors and trigger events see the positions the last step left, as before.
 *   Records   the hit records kept are those of the call's last step.
 *   bge_world_characters_crowd    flags = BGE_CHAR_CROWD_ON, or 0 = off (which drops the records; n, group and mask are then
 *                                 ignored).  With ON, n must equal the set's size; group and mask are per character, NULL means
 *                                 group 1 and mask 0xffffffff.  Unknown flag bits, a max_push that is not finite and >= 0, a wrong n
 *                                 and ON without a set are BGE_ERR_INVALID.  Calling it again replaces the filters and max_push.  All
 *                                 arrays are allocated here: an update call allocates nothing and reads nothing back.  Synchronises
 *                                 the world's stream.
 *   bge_world_characters_crowd_hits  out[0 .. count) = the records of characters first .. first + count as the last update call's
 *                                 last step left them (all words 0 before the first update).  Synchronises the world's stream.  A
 *                                 range outside the set is BGE_ERR_INVALID, and so is any count > 0 while the crowd is off.
 *   bge_world_characters_crowd_hits_device  the resident bge_crowd_hit[n] (NULL and 0 while the crowd is off), valid until the next
 *                                 bge_world_characters_crowd(0) or bge_world_characters_create; reads must be ordered after the
 *                                 world's stream.
 *   bge_world_characters_create   switches the crowd off and drops the records.  bge_world_characters_warp does nothing special.
 *   Not done  characters do not block each other's SWEEPS: this is a push, not a cast, so two characters may overlap by what one
 *             step walked; vertical stacking (the push is level: a character standing on another is parted sideways); more than
 *             the deepest neighbour per step (a character between several others moves away from the deepest only, and the steps
 *             after it deal with the rest).
 */
typedef struct bge_crowd_sphere {
    float center[3];
    float radius;
    uint32_t group;
    uint32_t mask;
} bge_crowd_sphere; /* 24 bytes */
enum bge_crowd_flags { BGE_CROWD_INVALID = 1u, BGE_CROWD_PUSHED = 2u, BGE_CROWD_CLAMPED = 4u };
enum bge_character_crowd_mode { BGE_CHAR_CROWD_ON = 1u };
typedef struct bge_crowd_hit {
    uint32_t flags;      /* bge_crowd_flags */
    uint32_t other;      /* index of the deepest overlapping sphere; BGE_RAY_NO_ENTITY if none */
    uint32_t n_overlaps; /* how many spheres of the batch overlap this one */
    float depth;         /* of `other`; 0 if none */
    float push[3];       /* push[1] is always +0 */
    uint32_t reserved;   /* 0 */
} bge_crowd_hit; /* 32 bytes, 4-byte aligned, moved word by word */
BGE_API int bge_world_crowd_query(bge_world* world, uint64_t n, const bge_crowd_sphere* spheres, float max_push, bge_crowd_hit* hits);
BGE_API int bge_world_crowd_query_device(bge_world* world, uint64_t n, const void* spheres_device, float max_push, void* hits_device);
BGE_API int bge_world_characters_crowd(bge_world* world, uint32_t flags, float max_push, uint64_t n, const uint32_t* group,
                                       const uint32_t* mask);
BGE_API int bge_world_characters_crowd_hits(bge_world* world, uint64_t first, uint64_t count, bge_crowd_hit* out);
BGE_API int bge_world_characters_crowd_hits_device(bge_world* world, void** hits, uint64_t* n);

/*
 * Impulses: a batch of impulse records applied to Dynamic bodies on the device.  An extension: the reference never
 * calls them, but they are Bullet's btRigidBody::applyImpulse / applyCentralImpulse / applyTorqueImpulse, each followed by
 * btCollisionObject::activate(), and the rule below is the specification.  All arithmetic is binary32, one rounding per operation,
 * in the stated order.
 *   Record    bge_impulse {entity, flags, impulse[3], point[3]}.  The low two bits of flags are the kind:
 *               BGE_IMPULSE_AT_POINT (0)  point is Bullet's rel_pos: relative to the body's origin, in world axes
 *               BGE_IMPULSE_CENTRAL  (1)  point is ignored
 *               BGE_IMPULSE_TORQUE   (2)  impulse is a torque impulse, point is ignored
 *             BGE_IMPULSE_WORLD_POINT (4), with AT_POINT only: point is a world position and r[k] = point[k] - origin[k], origin
 *             being the body's position in memory.  Kind 3, WORLD_POINT with another kind and any other bit are unknown flags.
 *   Valid     a record is valid iff its flags are known, every float its kind reads is finite (impulse; point too for AT_POINT),
 *             entity < the world's entity count, and that entity carries a Dynamic body at the time of the call: it has a slot
 *             and the slot's type is Dynamic (a body kept without a Transform counts; so does one whose RigidBody or Collider is
 *             dirty — see Wake).  Every other record is skipped and changes nothing.
 *   Apply     per body, its valid records in ASCENDING RECORD INDEX, as if Bullet's calls were made one after the other, on the
 *             velocities in memory (v, w):
 *               AT_POINT, CENTRAL   v[k] = v[k] + impulse[k] * inv_mass                                    k = x, y, z
 *               AT_POINT            t = cross3(r, impulse);  w = w + mat_vec(invI_world, t)
 *               TORQUE              t = impulse;             w = w + mat_vec(invI_world, t)
 *             cross3(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x); mat_vec row r = (m[r][0]*t.x + m[r][1]*t.y)
 *             + m[r][2]*t.z; w = w + u adds component by component.  inv_mass is the value the tick uses (1 / mass as uploaded).
 *             invI_world is the contact solver's, computed once per body and call from the pose in memory, so it does not change
 *             between the records of a call.  Records of different bodies do not meet.
 *   Inertia   mass = max(mass as uploaded, 0.01); inv_mass = 1 / mass.  Box: he = the collider's half extents with margin (for
 *             sizes >= 0.4: (size - 0.04f) + 0.04f per axis), l = 2 * he, m12 = mass * 0.0833333358168602f,
 *             I = (m12*(l.y*l.y + l.z*l.z), m12*(l.x*l.x + l.z*l.z), m12*(l.x*l.x + l.y*l.y)).  Capsule (radius r, half height
 *             hh): l = 2 * (r, r + hh, r), sm = mass * 0.08333333f, I likewise with sm.  il[k] = I[k] != 0 ? 1 / I[k] : 0.
 *             basis B = btMatrix3x3(q) of the stored quaternion q, the same under both orientation schemes:
 *             d = ((q.x*q.x + q.y*q.y) + q.z*q.z) + q.w*q.w; s = 2 / d; xs, ys, zs = q.x*s, q.y*s, q.z*s; wx = q.w*xs ..; xx = q.x*xs ..;
 *             B = [1 - (yy + zz), xy - wz, xz + wy; xy + wz, 1 - (xx + zz), yz - wx; xz - wy, yz + wx, 1 - (xx + yy)].
 *             invI_world[r][c] = ((B[r][0]*il.x)*B[c][0] + (B[r][1]*il.y)*B[c][1]) + (B[r][2]*il.z)*B[c][2].
 *   Wake      a body with at least one valid record is activated as activate() does it: its state becomes ACTIVE_TAG and
 *             m_deactivationTime 0, whether it was asleep, wanted to sleep or was awake with a running timer.  A valid record
 *             whose impulse is all zeros still wakes: that is the caller's activate().  Cached contacts (the plane's manifold,
 *             the box manifolds, the pair cache of Dynamic-against-Dynamic contacts) are not touched: a woken body warm-starts
 *             from what it held.  With Dynamic-against-Dynamic contacts on, the next tick finds an island that is no longer all
 *             asleep: its other sleeping bodies go WANTS_DEACTIVATION with timer 0 (Bullet's buildIslands) and the island is
 *             collided and solved again.  A body whose RigidBody or Collider is
 *             dirty is re-created by the next tick with zero velocity, as after any upload: the impulse is lost with the old body.
 *   Status    optional, one word per record: BGE_IMPULSE_APPLIED (1) on every valid record; BGE_IMPULSE_WOKE (2) in addition on
 *             the lowest-index valid record of a body that was not ACTIVE_TAG with timer 0 before the call;
 *             BGE_IMPULSE_INVALID (4) alone for unknown flags or a non-finite float (whatever the entity is); otherwise
 *             BGE_IMPULSE_NO_BODY (8) alone for an entity out of range or without a Dynamic body.
 *   Hence     the result is the same bytes every time, however many records name one body and however the batch is ordered
 *             among different bodies: no sum is taken across records other than the one the order states.
 *   Example   a 1 kg box of half extents 0.5 at rest at the origin, unrotated, ISLAND_SLEEPING.  I_local = (1/6, 1/6, 1/6),
 *             invI_world = diag(6).  Record 0: AT_POINT, impulse (0, 0, 2), point (0.5, 0, 0): v = (0, 0, 2), t = (0, -1, 0),
 *             w = (0, -6, 0).  Record 1 on the same body: CENTRAL, impulse (1, 0, 0): v = (1, 0, 2).  The body is ACTIVE_TAG with
 *             timer 0; status = {APPLIED | WOKE, APPLIED}.
 *   bge_world_apply_impulses         records[0 .. n) from host memory; status[0 .. n) or NULL.  n = 0 is a no-op; records NULL
 *                                    with n > 0 is BGE_ERR_INVALID; n is at most 2^30 - 1.  Before bge_world_set_topology it
 *                                    returns what bge_world_sphere_cast returns there.  Synchronises the world's stream.
 *   bge_world_apply_impulses_device  the same from and to device pointers, 4-byte aligned (a misaligned pointer is
 *                                    BGE_ERR_INVALID); status_device may be NULL.  Enqueued on the world's stream, no
 *                                    synchronisation, nothing read back; the records must stay as they are until the stream has
 *                                    passed the call.
 */
enum bge_impulse_flags { BGE_IMPULSE_AT_POINT = 0u, BGE_IMPULSE_CENTRAL = 1u, BGE_IMPULSE_TORQUE = 2u, BGE_IMPULSE_WORLD_POINT = 4u };
enum bge_impulse_status { BGE_IMPULSE_APPLIED = 1u, BGE_IMPULSE_WOKE = 2u, BGE_IMPULSE_INVALID = 4u, BGE_IMPULSE_NO_BODY = 8u };
typedef struct bge_impulse {
    uint32_t entity;
    uint32_t flags;   /* bge_impulse_flags */
    float impulse[3]; /* N s; for BGE_IMPULSE_TORQUE a torque impulse, N m s */
    float point[3];   /* AT_POINT: rel_pos, or a world position with BGE_IMPULSE_WORLD_POINT; otherwise ignored */
} bge_impulse; /* 32 bytes, 4-byte aligned, moved word by word */
BGE_API int bge_world_apply_impulses(bge_world* world, uint64_t n, const bge_impulse* records, uint32_t* status);
BGE_API int bge_world_apply_impulses_device(bge_world* world, uint64_t n, const void* records_device, void* status_device);

/*
 * Character push: the device's characters shove the Dynamic bodies they walk into.  In the reference the
 * character's ghost is a fixed body to the solver and a crate is pushed out of it; here the step's hit becomes an impulse record.
 * Opt-in: until bge_world_characters_push switches it on, every call does byte for byte what it does without this section.
 *   Push      with push on, every step of bge_world_characters_update ends with the stage Push, after State.  For character i the
 *             record is empty (entity = BGE_RAY_NO_ENTITY, every other word 0) unless all of these hold for the state the step
 *             left: the step was valid (no BGE_CHAR_INVALID); hit_kind == BGE_RAY_BODY; hit_entity carries a Dynamic body (as
 *             "Impulses" Valid); that body's collision group & body_mask != 0; |hit_normal.y| <= max_normal_y.  Then, with
 *             n = hit_normal:
 *                  h = sqrtf(n.x*n.x + n.z*n.z);  d = (-n.x / h, 0, -n.z / h);  m = force * dt;  impulse = (d.x*m, d.y*m, d.z*m)
 *             kind BGE_IMPULSE_CENTRAL, entity = hit_entity, point 0.  max_normal_y < 1 makes h > 0 for a unit normal; a record
 *             whose impulse is not finite is skipped by Apply like any other.
 *   Apply     the n records then go through "Impulses" Apply and Wake, record index = character index: two characters against
 *             one crate in one step add in character order, and a pushed body wakes.  No status is kept.
 *   Hence     bodies do not move between the steps of one update call, so every step of a call pushes; the push is central, so
 *             it produces no spin; a character standing on a crate does not push it (its hit normal is vertical, and the ground
 *             probe is not a hit); there is no reaction on the character.
 *   Example   force 30, dt = 1/60, a character walking along +x into the face of a 1 kg crate: hit_normal = (-1, 0, 0), h = 1,
 *             d = (1, 0, 0), m = 0.5: the crate's v.x grows by 0.5 in that step, and it is ACTIVE_TAG with timer 0.
 *   Records   the push records kept are those of the call's last step.
 *   bge_world_characters_push     desc->flags = BGE_CHAR_PUSH_ON, or 0 = off (which drops the records; the other members are then
 *                                 ignored).  Unknown flag bits, a force that is not finite and >= 0, a max_normal_y that is not
 *                                 finite and in [0, 1), a NULL desc and ON without a set are BGE_ERR_INVALID.  Calling it again
 *                                 replaces the desc.  All arrays are allocated here: an update call allocates nothing and reads
 *                                 nothing back.  Synchronises the world's stream.
 *   bge_world_characters_push_records  out[0 .. count) = the records of characters first .. first + count as the last update
 *                                 call's last step left them (empty before the first update).  Synchronises the world's stream.
 *                                 A range outside the set is BGE_ERR_INVALID, and so is any count > 0 while push is off.
 *   bge_world_characters_push_records_device  the resident bge_impulse[n] (NULL and 0 while push is off), valid until the next
 *                                 bge_world_characters_push(off) or bge_world_characters_create; reads must be ordered after the
 *                                 world's stream.
 *   bge_world_characters_create   switches push off and drops the records.
 *   Not done  a reaction on the character; a push at the contact point (spin); radial impulses; forces accumulated over a step.
 */
enum bge_character_push_mode { BGE_CHAR_PUSH_ON = 1u };
typedef struct bge_character_push_desc {
    uint32_t flags;     /* bge_character_push_mode */
    float force;        /* newtons, finite, >= 0 */
    float max_normal_y; /* finite, in [0, 1): steeper hits (|hit_normal.y| above it) do not push */
    uint32_t body_mask; /* a body is pushed iff its collision group & body_mask != 0 */
} bge_character_push_desc; /* 16 bytes */
BGE_API int bge_world_characters_push(bge_world* world, const bge_character_push_desc* desc);
BGE_API int bge_world_characters_push_records(bge_world* world, uint64_t first, uint64_t count, bge_impulse* out);
BGE_API int bge_world_characters_push_records_device(bge_world* world, void** records, uint64_t* n);

/*
 * Query index.  Opt-in; off by default, and while it is off every call enqueues exactly what it enqueues without this section.
 * Every ray, sphere cast, overlap and penetration query — and so every move, step move, recovery and character step, which are
 * made of them — tests bodies against queries in one body pass.  Without the index that pass tests EVERY body against EVERY
 * query.  With it, a spatial hash of the bodies' cull spheres at their current poses is built on the device at the head of the
 * call, and a query's body pass visits only the cells its extent touches.  The index only chooses WHICH bodies a query looks at:
 * every body it looks at goes through the same cull and the same exact test, operation for operation, a closest hit is a minimum
 * with a stated tie and a list is sorted by a total order, so every answer is THE SAME BYTES as with the index off.  Ghosts and
 * the ground plane are not indexed (they are handled per query as before).  The rule below is the specification; h is the cell
 * edge in force, cell(x) = clamp(floor(x / h), -2^20, 2^20) per axis, computed in float.
 *   1 Members     exactly the bodies the queries can see at all: a body of any type that is in the world (not uploaded since the
 *                 last physics tick, not removed) with group != 0 and mask != 0.  A member's cull sphere has the body's position
 *                 c as centre and rb = rad * 1.0001 + 1e-5 * (|c.x| + |c.y| + |c.z|) + 1e-6 as radius (rad: capsule radius +
 *                 half height; box |half extents with margin|), each operation rounded to float — the queries' own expression.
 *   2 Wide list   a member whose rb is not finite or exceeds h / 2 is on the wide list; every other member is in the cell of c.
 *                 Every indexed query tests the whole wide list.  A large ground box is such a body; so is one at 1e30.  A
 *                 non-finite pose needs no special case: its cull fails as it does without the index.
 *   3 Far queries the extent of a query is the box of its segment (ray, sphere cast: origin and origin + direction * max_distance)
 *                 or its centre (overlap, penetration: the point form), and its growth what its cull adds to rb: slack for a
 *                 ray, radius * 1.0001 + slack for the others, slack the kind's own 1e-5 * (sum of magnitudes) term.  With
 *                 reach = (h / 2 + growth) * 1.0625 the query visits the cells cell(lo - reach) .. cell(hi + reach) per axis.  It
 *                 goes FAR instead when that is more than max_cells cells, or more than 1024 on one axis (a member's record
 *                 carries the low 10 bits of its cell per axis, which is what tells visited cells apart), or when lo - reach,
 *                 hi + reach or reach is not finite, or reach > 1e18.  Far queries run the all-bodies pass, over the far
 *                 queries alone.  A long diagonal ray is therefore far; a 3-D line walk through the cells is not built.
 *   4 Coverage    for every (query, member) pair the cull passes, the member is visited: in its own cell, or on the wide list,
 *                 or because the query is far (DESIGN.md 4.24 has the argument for the margin 1.0625 over float rounding).
 *   5 No double visits  a member is accepted only on the visit of its own cell, by the key bits in its record: a bucket shared by
 *                 two visited cells, or a hash collision, puts no object twice into a list of all hits.
 *   6 Freshness   the index is built once per public call that queries, before its first pass, from the poses of that moment,
 *                 and all passes of the call share it (the passes of one bge_world_characters_update, the slides of a move, the
 *                 casts of a step move).  Nothing is kept across calls.  No query call synchronises or reads anything back for it.
 *   bge_world_set_query_index    desc = NULL or mode = 0: off.  mode = 1: on, with cell_edge (0 = chosen by the library: 4.0),
 *                 max_cells (0 = default: 256) and min_work: a call of n queries against a world of n_slots slots builds and uses
 *                 the index when n * n_slots >= min_work (for a move, step move and character update n is the casts of one
 *                 pass) and takes the all-bodies pass otherwise; 0 = every call.  BGE_QUERY_INDEX_MIN_WORK_DEFAULT (2^30: about
 *                 1,000 queries against a million slots, the measured crossover of DESIGN.md 4.24) is the library's choice.  mode > 1, a negative or non-finite cell_edge or reserved != 0 is BGE_ERR_INVALID and
 *                 changes nothing.  An edge below 1e-18 counts as 1e-18.
 *   bge_world_query_index_stats  what the last call that queried did: whether it built the index, members in cells and on the
 *                 wide list, queries that walked cells and queries that went far (summed over the passes of that call; a list
 *                 that outgrew its capacity runs its pass twice), the cell edge and table size, and builds since the world's
 *                 creation.  Synchronises the stream once and reads a few words.
 * The environment gives the default desc of a NEW world, read once in bge_world_create: BGE_QUERY_INDEX=1 (mode = 1) and
 * BGE_QUERY_INDEX_MIN_WORK=<n>.  They change no result.
 */
#define BGE_QUERY_INDEX_MIN_WORK_DEFAULT ((uint64_t)1 << 30)
typedef struct bge_query_index_desc {
    uint32_t mode;      /* 0 off, 1 on */
    float cell_edge;    /* 0 = chosen by the library */
    uint32_t max_cells; /* most cells one query may visit; 0 = default */
    uint32_t reserved;  /* 0 */
    uint64_t min_work;  /* n_queries * n_slots below it: the all-bodies pass */
} bge_query_index_desc; /* 24 bytes */
typedef struct bge_query_index_stats {
    uint32_t built;           /* 1: the last call that queried built and used the index */
    uint32_t table_size;      /* buckets */
    uint64_t bodies_indexed;  /* members in cells */
    uint64_t bodies_wide;     /* members on the wide list */
    uint64_t queries_indexed; /* queries that walked their cells */
    uint64_t queries_far;     /* queries that took the all-bodies pass */
    float cell_edge;
    uint32_t reserved;
    uint64_t builds;          /* since bge_world_create */
    uint64_t reserved2;
} bge_query_index_stats; /* 64 bytes */
BGE_API int bge_world_set_query_index(bge_world* world, const bge_query_index_desc* desc);
BGE_API int bge_world_query_index_stats(bge_world* world, bge_query_index_stats* out);

/*
 * The physics debug overlay: what PhysicsSystem::GetDebugLines hands to the renderer while the overlay is on
 * (src/physics/PhysicsSystem.cpp:857-873, 1148-1175; src/physics/BulletDebugDrawer.cpp) — every collision object's shape as
 * wireframe lines in one colour, then one short red line per contact point — made on the device from the state the last tick
 * left.  The query reads that state and changes nothing.  The rules below are the specification.
 *   Shapes    (BGE_DEBUG_SHAPES) exactly the objects the ray queries see, at the same poses; the layer / mask play no part:
 *             - every rigid body of any type, asleep or awake, that is in the world (not uploaded since the last physics tick,
 *               not removed) at position + quaternion as held after the last physics tick, with the collider as Bullet holds it
 *               (box: half extents with margin; capsule: radius, half height);
 *             - every trigger ghost that is in the world and posed (as for rays);
 *             - the ground plane when bge_world_set_ground_plane is on.
 *   Lines     box      12: the corners (-x-y-z, +x-y-z, +x+y-z, -x+y-z, then the same four at +z) through the pose, edges
 *                          0,1 1,2 2,3 3,0  4,5 5,6 6,7 7,4  0,4 1,5 2,6 3,7 (DrawBox).
 *             capsule 120: up axis Y, the axes the NORMALISED columns of the basis; 24 segments x (top ring, bottom ring, side
 *                          line) = 72 lines, then 12 hemisphere steps x (top, bottom in the plane of the basis' Z column, top,
 *                          bottom in the plane of its X column) = 48 (DrawCapsule; ring angle i / 24 * 2 pi measured from the Z
 *                          column towards the X column, as there).
 *             plane    12: the square (-25,0,25) (-25,0,-25) (25,0,-25) (25,0,25) as 4 border lines, then for i = 1..4, t = i / 5
 *                          the two grid lines lerp(c0,c3,t)-lerp(c1,c2,t) and lerp(c0,c1,t)-lerp(c3,c2,t) (DrawStaticPlane with
 *                          btPlaneSpace1's u = (-1,0,0), v = (0,0,1)).
 *   Colours   abgr: 0xffff00ff trigger ghosts; 0xff7f7f7f Static bodies and the plane; 0xff00ffff Dynamic AND Kinematic bodies (the
 *             reference's Kinematic bodies end up without CF_STATIC_OBJECT, PhysicsSystem.cpp:443-465); 0xff0000ff contacts.
 *   Order     of the shapes section — fixed, so that a caller finds an entity's lines from counts alone: (1) the plane's 12
 *             lines, if on; (2) bodies in ascending ENTITY index, 12 lines per box, 120 per capsule; (3) ghosts in the order of
 *             the uploaded trigger array.  (The reference's order is that of an unordered_map and of Bullet's object array: this
 *             order is a specification choice.)
 *   Contacts  (BGE_DEBUG_CONTACTS) behind the shapes: one line per contact point that bge_world_download_contacts (while the
 *             plane is on), bge_world_download_box_contacts (while the static contacts are on) and
 *             bge_world_download_dynamic_pairs (while the dynamic contacts are on) report at the time of the call:
 *             from = body B's pose x localB, where B is the plane (its frame is the world's: (localB.x, 0, localB.z)), the
 *             obstacle box, or the higher entity of a pair; to = from + 0.25 x normalise(normalWorldOnB), (0, 1, 0) for the plane
 *             and for a normal of squared length below FLT_EPSILON.  (Bullet draws the m_positionWorldOnB cached by the last
 *             narrowphase; for a Dynamic B that differs from "current pose x localB" by one integration step — a stated choice.)
 *             The ORDER inside the contact section is unspecified: every point exactly once, the same multiset for the same state.
 *   Region    with use_region a body or ghost is drawn when its origin lies in the closed box region_min <= origin <= region_max
 *             (plain binary32 compares; all of its lines or none), a contact when its `from` point does, the plane always.  A
 *             region with a NaN or with min > max on an axis draws only the plane.
 *   Call order  as for rays: after a physics tick, before new poses are uploaded.
 *   bge_world_debug_lines         the convention of bge_world_pairs: lines = NULL only counts; cap < *total is BGE_ERR_INVALID
 *                                 with *total filled in and nothing written.  desc = NULL means BGE_DEBUG_ALL, whole world.
 *                                 Synchronises the world's stream.
 *   bge_world_debug_lines_device  device pointers: lines_device = bge_debug_line[cap] (4-byte aligned; may be NULL when cap = 0),
 *                                 total_device = one uint64_t.  Enqueued on the world's stream, no synchronisation.  Lines beyond
 *                                 cap are not written; *total_device still counts them (a renderer can draw from the buffer with
 *                                 an indirect draw).
 *   More than 2^32 - 1 lines is BGE_ERR_UNSUPPORTED, decided before anything is written.  No lines at all is not an error.
 */
typedef struct bge_debug_line {
    float from[3];
    float to[3];
    uint32_t abgr;
} bge_debug_line; /* 28 bytes: the reference's PhysicsDebugLine (src/physics/PhysicsDebugDraw.h) */
enum bge_debug_flags { BGE_DEBUG_SHAPES = 1u, BGE_DEBUG_CONTACTS = 2u, BGE_DEBUG_ALL = 3u };
typedef struct bge_debug_desc {
    uint32_t struct_size; /* sizeof(bge_debug_desc) */
    uint32_t flags;       /* bge_debug_flags; the reference's overlay is BGE_DEBUG_ALL */
    uint32_t use_region;  /* 0: the whole world */
    float region_min[3], region_max[3];
} bge_debug_desc;
BGE_API int bge_world_debug_lines(bge_world* world, const bge_debug_desc* desc, bge_debug_line* lines, uint64_t cap, uint64_t* total);
BGE_API int bge_world_debug_lines_device(bge_world* world, const bge_debug_desc* desc, void* lines_device, uint64_t cap,
                                         void* total_device);

/*
 * Frustum culling: which entities a view sees, with their matrices packed for an instanced or indirect draw.  An EXTENSION: the
 * reference's renderer submits every MeshRenderer whose Transform is clean (src/render/Renderer.cpp:606-665).  The world and
 * normal matrices are the render feed the tick ends in; this is its last step, made where they live.  The rules below are the
 * specification.
 *   Bounds    bge_world_upload_bounds / _indexed: the model-space box of the entity's mesh, a centre and half extents, three
 *             floats each.  Stored per ENTITY (not per slot).  An entity is RENDERABLE once it has bounds whose three half extents
 *             are finite and >= 0 and whose centre is finite; a negative, infinite or NaN half extent or a non-finite centre takes
 *             it out again.  Bounds are component state: bge_world_set_topology keeps them for surviving indices, as it keeps
 *             bodies (an index beyond the old entity count starts without bounds).  Uploading bounds marks nothing dirty.
 *   Rule      binary32, each line evaluated left to right with one rounding per operation.  For entity e with slot s, world
 *             matrix m = world[s] (translation in m[12..14]), centre c and half extents h:
 *                 cw[j] = ((c.x*m[j] + c.y*m[4+j]) + c.z*m[8+j]) + m[12+j]                      j = 0, 1, 2
 *             and for every plane (a, b, c4, d):
 *                 e_i = (a*m[4i] + b*m[4i+1]) + c4*m[4i+2]                                      i = 0, 1, 2
 *                 r   = (|e_0|*h.x + |e_1|*h.y) + |e_2|*h.z
 *                 sd  = ((a*cw.x + b*cw.y) + c4*cw.z) + d
 *             The entity is VISIBLE iff it is renderable, owns a Transform, is not dirty (bge_world_download_dirty reports 0:
 *             it has been through a transforms tick since it was last marked; an entity inside a parent cycle stays dirty and is
 *             never drawn, as the renderer skips transform->dirty) and sd >= -r is TRUE for every plane — so a NaN anywhere
 *             culls.  Planes point inwards and need not be normalised.  n_planes = 0 lists every renderable, clean entity.
 *             This is the usual oriented-box test: exact per plane, conservative at the corners of a frustum.
 *   Order     ascending ENTITY index; record k of every output array belongs to the same entity.  world16[k] equals
 *             bge_world_download_world_indexed of that entity bit for bit, normal16[k] bge_world_download_normal's.
 *   bge_world_visible         the convention of bge_world_pairs / bge_world_debug_lines: with all three outputs NULL it only
 *                             counts; cap < *total is BGE_ERR_INVALID with *total filled in and nothing written; any of the three
 *                             outputs may be NULL.  Synchronises the world's stream.
 *   bge_world_visible_device  device pointers (entities 4-byte, the matrices 16-byte aligned; any may be NULL) and one device
 *                             uint64_t for the total.  Enqueued on the world's stream, no synchronisation.  Records beyond cap
 *                             are not written and are still counted: a renderer can feed an indirect draw from the buffers.
 *   normal16  before a BGE_TICK_NORMAL_MATRICES tick (or after a bge_world_set_topology that grew the world, before the next
 *             one) asking for it is BGE_ERR_STATE, as bge_world_download_normal.
 *   n_planes > 16 is BGE_ERR_INVALID.  More than 2^32 - 1 records is BGE_ERR_UNSUPPORTED (a world holds fewer entities than that).
 *   The query changes no world state.
 *   bge_frustum_planes   host only: the six planes of a view-projection matrix in the bx row-vector convention,
 *             clip_j = sum_i v_i * m[4i+j], in the order w+x, w-x, w+y, w-y, near, w-z, where near is z (depth 0..1), or w+z with
 *             homogeneous_depth (depth -1..1).  Plane k is planes24[4k..4k+3] = (a, b, c4, d); each coefficient is ONE binary32
 *             add or subtract of two matrix elements (or the element itself).
 */
#define BGE_CULL_MAX_PLANES 16
typedef struct bge_cull_desc {
    uint32_t struct_size; /* sizeof(bge_cull_desc) */
    uint32_t n_planes;    /* 0 .. BGE_CULL_MAX_PLANES */
    float planes[BGE_CULL_MAX_PLANES][4];
} bge_cull_desc;
BGE_API int bge_world_upload_bounds(bge_world* world, uint64_t first, uint64_t count, const float* center3, const float* half3);
BGE_API int bge_world_upload_bounds_indexed(bge_world* world, uint64_t count, const uint32_t* entity_index, const float* center3,
                                            const float* half3);
BGE_API int bge_world_visible(bge_world* world, const bge_cull_desc* desc, uint32_t* entities, float* world16, float* normal16,
                              uint64_t cap, uint64_t* total);
BGE_API int bge_world_visible_device(bge_world* world, const bge_cull_desc* desc, void* entities_device, void* world16_device,
                                     void* normal16_device, uint64_t cap, void* total_device);
BGE_API int bge_frustum_planes(const float viewproj16[16], int homogeneous_depth, float planes24[24]);

/*
 * Draw batches: the visible entities grouped by draw key, so that one instanced or indirect draw per key can be issued straight
 * from the buffers.  An EXTENSION on top of the frustum culling above (the reference's renderer walks MeshRenderer { mesh,
 * material } per entity, src/render/Renderer.cpp:606-700).  The rules below are the specification.
 *   Keys      bge_world_upload_draw_keys / _indexed: one uint32_t per entity, the caller's id for a mesh + material combination.
 *             Stored per ENTITY (not per slot), as the bounds are.  Every entity starts with BGE_NO_DRAW_KEY.  Any 32-bit value
 *             may be uploaded.  bge_world_set_topology keeps the keys of surviving indices; an index beyond the old entity count
 *             (also one that was removed and is reused after growth) starts without a key.  Uploading keys marks nothing dirty.
 *   Members   entity e is in the result iff it is VISIBLE by the rule of bge_world_visible for the same desc (renderable, owns a
 *             Transform, clean, sd >= -r on every plane) and key[e] < n_keys.  Entities whose key is >= n_keys, BGE_NO_DRAW_KEY
 *             included, are left out and not counted.  With n_keys = 1 and every key 0 the result equals bge_world_visible's,
 *             record for record.
 *   Order     records are sorted by (key, entity index), both ascending.  batches[k].instance_count is the number of records
 *             with key k; batches[k].first_instance is the sum of the counts of the keys below k, for empty batches too, so all
 *             n_keys entries are defined.  *total is the sum of all counts.  Record i of entities, world16 and normal16 belongs to
 *             the same entity; the matrices equal bge_world_download_world_indexed / bge_world_download_normal bit for bit.  The
 *             same state gives the same bytes on every call.
 *   bge_world_draw_batches         the convention of bge_world_visible; synchronises the world's stream.  batches, when not NULL,
 *                                  has n_keys entries and is always filled, whatever cap is.  With the three record outputs NULL
 *                                  the call only counts.  cap < *total is BGE_ERR_INVALID with *total and batches filled in and no
 *                                  record written.
 *   bge_world_draw_batches_device  device pointers (batches and entities 4-byte, the matrices 16-byte, total 8-byte aligned; all
 *                                  but total may be NULL; a misaligned pointer is BGE_ERR_INVALID).  Enqueued on the world's
 *                                  stream, no synchronisation.  Records at positions >= cap are not written and are still counted;
 *                                  batches always holds the full counts.
 *   n_keys == 0 or n_keys > BGE_DRAW_MAX_KEYS is BGE_ERR_INVALID; n_planes > 16 and a wrong struct_size as for bge_world_visible;
 *   normal16 before a BGE_TICK_NORMAL_MATRICES tick is BGE_ERR_STATE; so is a call before bge_world_set_topology.  An indexed
 *   upload with an index outside the world is BGE_ERR_INVALID and uploads nothing.
 *   The query changes no world state, and does not change what the next bge_world_visible returns (nor the other way round).
 */
#define BGE_NO_DRAW_KEY 0xffffffffu
#define BGE_DRAW_MAX_KEYS 65536u
typedef struct bge_draw_batch {
    uint32_t first_instance;
    uint32_t instance_count;
} bge_draw_batch; /* 8 bytes */
BGE_API int bge_world_upload_draw_keys(bge_world* world, uint64_t first, uint64_t count, const uint32_t* key);
BGE_API int bge_world_upload_draw_keys_indexed(bge_world* world, uint64_t count, const uint32_t* entity_index, const uint32_t* key);
BGE_API int bge_world_draw_batches(bge_world* world, const bge_cull_desc* desc, uint32_t n_keys, bge_draw_batch* batches,
                                   uint32_t* entities, float* world16, float* normal16, uint64_t cap, uint64_t* total);
BGE_API int bge_world_draw_batches_device(bge_world* world, const bge_cull_desc* desc, uint32_t n_keys, void* batches_device,
                                          void* entities_device, void* world16_device, void* normal16_device, uint64_t cap,
                                          void* total_device);

/* Multi-GPU support: compact the world matrices of all roots (entity order) into one buffer that the
 * caller all-gathers across ranks (one collective per frame).  dst = NULL packs into the world's own
 * BGE_ARRAY_ROOT_WORLDS buffer; otherwise dst is a device pointer with room for n_roots*16 floats. */
BGE_API int bge_world_pack_roots(bge_world* world, void* dst_device);
BGE_API int bge_world_device_array(bge_world* world, int which, void** device_ptr, uint64_t* elements);

/*
 * Native collective (RCCL over xGMI), one process per GPU.  The reference has no distributed layer; this is
 * the only exchange of the sharded tick (BASELINE.json configs[4]): every rank contributes the world matrices
 * of its roots and receives everybody's.
 *   bge_comm_unique_id   rank 0 fills a 128-byte id and distributes it by any means (the bench uses
 *                        torch.distributed's store); wraps ncclGetUniqueId.
 *   bge_world_comm_init  joins the communicator (ncclCommInitRank) and allocates a ring of 8 send/receive buffer
 *                        pairs of `rows_per_rank` rows (ranks pad to the largest root count) plus a side stream for
 *                        the collective.  A row on the wire is BGE_ROOT_ROW_FLOATS = 12 floats: the root's world matrix
 *                        without its fourth column, which is exactly (0, 0, 0, 1) for a root (world = local =
 *                        bx::mtxSRT, src/ecs/Transform.cpp:32-35) — elements 0,1,2, 4,5,6, 8,9,10, 12,13,14.
 *   bge_world_gather_roots   packs this rank's roots on the world's stream and enqueues ONE gather on the side
 *                        stream; buffers rotate per frame, so frame t's gather runs under the following ticks.
 *                        *table_device (may be NULL) receives the device pointer of the table being filled:
 *                        nranks x rows_per_rank x 12 floats, rank-major.  bge_world_download_gathered returns full
 *                        4x4 matrices.
 *   bge_world_comm_wait  makes the world's stream wait for every outstanding gather.
 * librccl.so.1 is loaded at run time (dlopen); BGE_ERR_UNSUPPORTED when it cannot be found.
 */
#define BGE_ROOT_ROW_FLOATS 12
BGE_API int bge_comm_unique_id(void* out128);
BGE_API int bge_world_comm_init(bge_world* world, int nranks, int rank, const void* id128, uint64_t rows_per_rank);
BGE_API int bge_world_gather_roots(bge_world* world, void** table_device);
BGE_API int bge_world_comm_wait(bge_world* world);
/* How the frame's root table travels: one ncclAllGather (default), or DIRECT — one ncclSend + ncclRecv per peer in one
 * group, every rank pushing its block to each peer over its own xGMI link (the node is a full mesh).  Same table either
 * way; call on every rank.  bench.py times both on the node it runs on and keeps the faster one. */
enum bge_gather_mode { BGE_GATHER_ALLGATHER = 0, BGE_GATHER_DIRECT = 1 };
BGE_API int bge_world_comm_set_mode(bge_world* world, int mode);
/* Copy the most recently gathered table to the host (waits for it): nranks x rows_per_rank x 16 floats. */
BGE_API int bge_world_download_gathered(bge_world* world, float* out, uint64_t floats);
BGE_API int bge_world_comm_destroy(bge_world* world);

/*
 * Sharded broadphase: the GLOBAL pair set of a scene whose bodies live on several GPUs.
 * The reference has one Bullet world, hence one pair cache over all bodies (src/physics/PhysicsSystem.cpp:124, 863);
 * bge_partition_subtrees shards by subtree, so a per-world BGE_TICK_BROADPHASE only sees the pairs inside one shard.
 * For the pair search the bodies are re-partitioned into slabs along one axis, one slab per rank
 * (slab s = [cuts[s], cuts[s+1]), cuts[0] = -inf, cuts[nranks] = +inf, interior cuts non-decreasing):
 *   bge_world_set_global_ids   id reported for each local entity index (default: the index itself)
 *   bge_world_aabb_bounds      min / max corner over the body AABBs of the last BGE_TICK_AABBS / BGE_TICK_BROADPHASE
 *                              tick, so that ranks can agree on cuts
 *   bge_world_bp_route         counts[d] = records this world sends to slab d: one per slab the body's extent touches
 *   bge_world_bp_pack          the 48-byte records grouped by slab (slab d at record offset sum(counts[0..d))) into
 *                              device memory the caller exchanges (all-to-all: RCCL, torch.distributed, hipMemcpyPeer)
 *   bge_world_bp_find          pair search over the records a rank received; a pair is kept only where the lower end
 *                              of its overlap interval along `axis`, max(min_a, min_b), lies in [window_lo, window_hi)
 *                              = the rank's own slab, so the union over ranks is the global set without duplicates.
 *                              Afterwards bge_world_pairs returns these pairs (global ids) until the next
 *                              BGE_TICK_BROADPHASE tick.
 *   bge_world_bp_exchange      all of the above over the world's RCCL communicator (bge_world_comm_init): all-reduced
 *                              extent and histogram -> balanced cuts, one all-gather of counts, one send/recv per peer.
 * Record layout (float4 x 3): min.xyz | global id,  max.xyz | 0,  group | mask | static flag | 0.
 */
#define BGE_BP_RECORD_BYTES 48
BGE_API int bge_world_set_global_ids(bge_world* world, uint64_t first, uint64_t count, const uint32_t* ids);
BGE_API int bge_world_aabb_bounds(bge_world* world, float min3[3], float max3[3], uint64_t* n_bodies);
/* hist[b] = bodies whose AABB min corner along `axis` falls into bin b of `bins` (<= 4096) equal bins over [lo, hi]
 * (out-of-range values land in the first / last bin).  Summed over ranks it yields balanced cuts: */
BGE_API int bge_world_axis_histogram(bge_world* world, uint32_t axis, float lo, float hi, uint32_t bins, uint64_t* hist);
/* Host only: cuts[0..nranks] with cuts[k] = upper edge of the first bin at which k/nranks of the bodies are reached. */
BGE_API int bge_balanced_cuts(const uint64_t* hist, uint32_t bins, float lo, float hi, uint32_t nranks, float* cuts);
BGE_API int bge_world_bp_route(bge_world* world, uint32_t axis, uint32_t nranks, const float* cuts, uint64_t* counts);
BGE_API int bge_world_bp_pack(bge_world* world, void* send_device);
BGE_API int bge_world_bp_find(bge_world* world, const void* records_device, uint64_t n_records, uint32_t axis,
                              float window_lo, float window_hi);
BGE_API int bge_world_bp_exchange(bge_world* world, uint32_t axis);
BGE_API int bge_world_get_info(bge_world* world, bge_world_info* info);

/*
 * Host-side helpers (no GPU needed).
 * bge_flatten_topology: the tile/pass layout bge_world_set_topology would build — for inspection and tests.
 *   slot_of_entity[n], level_of_entity[n] (depth inside its tile), pass_of_entity[n]; any may be NULL.
 * bge_partition_subtrees: assign every entity to one of `nranks` shards, whole subtrees only, balancing
 *   node counts greedily (largest subtree first); rank_of_entity[n].  Entities in cycles go to rank 0.
 */
BGE_API int bge_flatten_topology(uint64_t n, const uint32_t* parent, const uint8_t* has_transform,
                                 uint32_t* slot_of_entity, uint8_t* level_of_entity, uint32_t* pass_of_entity,
                                 bge_world_info* info);
BGE_API int bge_partition_subtrees(uint64_t n, const uint32_t* parent, const uint8_t* has_transform,
                                   uint32_t nranks, uint32_t* rank_of_entity, uint64_t* nodes_per_rank);

#ifdef __cplusplus
}
#endif
#endif /* BGE_WORLD_H */
