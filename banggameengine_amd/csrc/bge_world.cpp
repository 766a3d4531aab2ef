// bge_world.cpp — implementation of the C ABI declared in include/bge_world.h.
//
// Host-side plumbing only: device allocation, the entity-index <-> slot maps, staging of uploads and
// downloads, and kernel launches on the world's stream.  All arithmetic of the hot path is in
// bge_kernels.hip; there is no CPU fallback — every entry point that needs the GPU fails with
// BGE_ERR_HIP when no device is usable.
#include "../../include/bge_world.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "bge_device_buffer.hpp"
#include "bge_broadphase.hpp"
#include "bge_route.hpp"
#include "bge_comm.hpp"
#include "bge_batch.hpp"
#include "bge_cull.hpp"
#include "bge_debug.hpp"
#include "bge_flatten.hpp"
#include "bge_epochs.hpp"
#include "bge_tick_plan.hpp"
#include "bge_kernels.hpp"
#include "bge_move.hpp"
#include "bge_step.hpp"
#include "bge_recover.hpp"
#include "bge_character.hpp"
#include "bge_chartrig.hpp"
#include "bge_ride.hpp"
#include "bge_crowd.hpp"
#include "bge_impulse.hpp"
#include "bge_impulse_math.hpp"
#include "bge_qindex.hpp"
#include "bge_qindex_math.hpp"
#include "bge_query.hpp"

namespace {

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

// include/bge_world.h promises that no entry point throws: every `int bge_*` function is a function-try-block that ends
// in this handler list (host containers can throw std::bad_alloc; an exception must not unwind into a C caller).
#define BGE_CATCH_ALL(name)                                                                              \
    catch (const std::bad_alloc&) { return fail(BGE_ERR_OOM, "%s: host allocation failed", name); }      \
    catch (const std::exception& e) { return fail(BGE_ERR_STATE, "%s: unexpected exception: %s", name, e.what()); } \
    catch (...) { return fail(BGE_ERR_STATE, "%s: unexpected exception", name); }

#define HIP_TRY(expr)                                                                                      \
    do {                                                                                                   \
        const hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) {                                                                            \
            return fail(e_ == hipErrorOutOfMemory ? BGE_ERR_OOM : BGE_ERR_HIP, "%s failed: %s (%s:%d)", #expr, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                        \
        }                                                                                                  \
    } while (0)

// Every device block of the world is a DevBuf, every page-locked one a PinnedBuf (bge_device_buffer.hpp): members and the
// temporaries of one call alike free themselves (an early HIP_TRY return must not leak them).
using bge::DevBuf;
using bge::PinnedBuf;

// A per-slot device array and its format, set once where the member is declared: upload, download, allocation and the carry of
// bge_world_set_topology read it from here.
struct SlotBuf : DevBuf {
    static constexpr int kNoFill = -1;
    const uint32_t words;        // 32-bit words per slot
    const bool vel_blocks;       // per-wave velocity blocks (bge_device_math.hpp vel_word) instead of rows of `words`
    const int fill;              // the byte a fresh store is filled with; kNoFill: k_init_slots and the uploads write every row
    const bool* const feature[2]; // optional store: made when one of these is first switched on, then kept; none = always there
    explicit SlotBuf(uint32_t words, bool vel_blocks = false, int fill = kNoFill, const bool* f0 = nullptr, const bool* f1 = nullptr)
        : words(words), vel_blocks(vel_blocks), fill(fill), feature{f0, f1} {}
    size_t bytes_for(uint64_t slots) const { return slots * words * 4; }
    // has a store in every layout: always, or exists already, or its feature is on
    bool wanted() const { return !feature[0] || p || *feature[0] || (feature[1] && *feature[1]); }
};

// A device array in ENTITY order (a re-flattening moves slots, not entities): allocated with the first upload, a row of all ones
// (NaNs) = nothing uploaded, rows >= n_entities once it exists.
struct EntityBuf : DevBuf {
    const uint32_t words; // per entity
    uint64_t rows = 0;
    explicit EntityBuf(uint32_t words) : words(words) {}
    int first_use(uint64_t n_entities, hipStream_t stream)
    {
        if (p) return BGE_OK;
        const uint64_t n = std::max<uint64_t>(n_entities, 1);
        HIP_TRY(ensure(n * words * 4));
        HIP_TRY(hipMemsetAsync(p, 0xff, n * words * 4, stream));
        rows = n;
        return BGE_OK;
    }
    // a topology of n entities after one of old_n: surviving indices keep their row, indices that went or are new have none
    int follow_topology(uint64_t n, uint64_t old_n, hipStream_t stream)
    {
        if (!p) return BGE_OK;
        const size_t row = words * 4;
        if (n > rows) {
            DevBuf grown;
            HIP_TRY(grown.ensure(n * row));
            HIP_TRY(hipMemsetAsync(grown.p, 0xff, n * row, stream));
            const uint64_t keep = std::min(old_n, rows);
            if (keep) HIP_TRY(hipMemcpyAsync(grown.p, p, keep * row, hipMemcpyDeviceToDevice, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            std::swap<DevBuf>(*this, grown);
            rows = n;
        } else if (n < old_n) {
            HIP_TRY(hipMemsetAsync(static_cast<char*>(p) + n * row, 0xff, (std::min(old_n, rows) - n) * row, stream));
        }
        return BGE_OK;
    }
};

// Collider size -> AABB half extents in the collider's frame.
// Box: btBoxShape ctor (implicit = he - 0.04), setSafeMargin (margin = min(0.04, 0.1*min he) through
// btBoxShape::setMargin), btTransformAabb adds the margin back.  Capsule (up axis Y): (r, r+h/2, r).
// Reference clamps: src/physics/PhysicsSystem.cpp:692-703.
void collider_half_extents(uint8_t shape, const float* size, float* out)
{
    if (shape == BGE_SHAPE_CAPSULE) {
        const float radius = std::max(size[0], 0.01f);
        const float half_height = std::max(size[1], 0.0f);
        const float h = 0.5f * (half_height * 2.0f);
        out[0] = radius;
        out[1] = radius + h;
        out[2] = radius;
        return;
    }
    const float hx = std::max(size[0], 0.01f), hy = std::max(size[1], 0.01f), hz = std::max(size[2], 0.01f);
    const float m0 = 0.04f;
    float ix = hx - m0, iy = hy - m0, iz = hz - m0;
    const float min_dim = std::min(hx, std::min(hy, hz));
    const float safe = 0.1f * min_dim;
    float margin = m0;
    if (safe < margin) {
        ix = (ix + m0) - safe;
        iy = (iy + m0) - safe;
        iz = (iz + m0) - safe;
        margin = safe;
    }
    out[0] = ix + margin;
    out[1] = iy + margin;
    out[2] = iz + margin;
}

} // namespace

struct bge_world {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint64_t pair_capacity_req = 0;

    bge::Flattened flat;
    std::vector<uint32_t> parent_entity; // entity-level parents (Scene::m_parents) as of the last set_topology
    DevBuf frozen;                       // WorldView::frozen (allocated with the first frozen root)
    bool any_frozen = false;
    bge::TileShape shape;                // of the first pass's tile headers; refresh_shape() wherever a header changes
    void refresh_shape()
    {
        shape = flat.pass_tile_begin.size() < 2 ? bge::TileShape{} : bge::TileShape::of(flat.tile_hdr.data(), flat.pass_tile_begin[0], flat.pass_tile_begin[1]);
    }
    std::vector<uint8_t> body_type_host; // bge_body_type per entity index as last uploaded (BGE_BODY_NONE = no body)
    std::vector<uint8_t> orphan_host;    // 1: the entity lost its Transform while it had a body; the body kept its slot (kValid clear)
    // A body exists in the reference's world from the first PhysicsSystem::Update that sees its components AND a Transform
    // (EnsureRigidBody); an entity that loses its Transform before that has no body to keep.  body_since[e]: the value of
    // physics_updates when the body of entity e was (last) uploaded onto a slot with a Transform; it exists once a later update ran.
    std::vector<uint64_t> body_since;
    uint64_t physics_updates = 0;
    bool has_topology = false;
    bool maybe_dirty = true;
    float local_time = 0.0f; // btDiscreteDynamicsWorld::m_localTime (bge_world_step_simulation)

    // device arrays
    DevBuf parent, tile_hdr, slot_of_entity, entity_of_slot, root_slots, root_index;
    DevBuf root_worlds, counter, stage, stage2, mass_palette, filter_table, grav_palette;
    // Per-slot arrays that are not carried as rows: flags are merged on the host; normal is allocated by the first tick that asks
    // for it and not carried (cull_params relies on its size staying stale after growth).
    SlotBuf flags{1}, normal{16};
    // Per-slot component state.  `carried` below is the one place that enumerates these.
    SlotBuf pos{3}, euler{3}, scale{3}, world{16}, vel{3, true}, angvel{3}, quat{4}, inv_mass{1}, deact{1}, filter_class{1};
    SlotBuf half_extent{3}, group{1}, mask{1}, aabb{6};
    SlotBuf cshape{4}, cmass{1}, cfriction{1}, cinfo{1}; // ground contact (bge_contact.hip)
    SlotBuf manifold{32, false, 0x00, &ground_plane};    // ... its four points per slot, from the first time the plane is switched on
    SlotBuf crestitution{1};                             // RigidBody::restitution per slot (k_init_slots writes the component default, 0)
    // kBoxManifolds manifold rows per slot, every row free (bge::kBoxNone) until a contact takes it.  A body of an island collides
    // its own pairs through contact_body, which keeps the obstacle manifold rows of its slot tidy whether or not there are
    // obstacles: the store exists from the first bge_world_set_static_contacts(1) or bge_world_set_dynamic_contacts(1) on.
    SlotBuf bmanifold{bge::kBoxManifolds * bge::kBoxManifoldWords, false, 0xff, &static_contacts, &dynamic_contacts};
    // What bge_world_set_topology carries over to the new layout, allocates for it and (the optional stores) fills, in this order.
    // An optional store follows every layout from its first use on, feature on or off: the carry scatters its rows to the NEW slot
    // indices, and the kernels index it by slot as soon as the feature is back.
    SlotBuf* const carried[21] = {&pos,   &euler, &scale, &world,  &vel,   &angvel,    &quat,  &inv_mass, &deact,        &filter_class, &half_extent,
                                  &group, &mask,  &aabb,  &cshape, &cmass, &cfriction, &cinfo, &manifold, &crestitution, &bmanifold};
    uint64_t slot_rows() const { return std::max<uint64_t>(flat.n_slots, bge::kTile); } // arrays are allocated for whole tiles
    DevBuf ground_list, ground_count;                 // slots k_ground_select hands to the solver; count + ticket words
    // The tick kernel's per-wave words (WorldView::rs_word: "rotation rows current", "at rest", and the flag value with its epoch: four
    // per wave64, zeroed with every layout) and the epochs they are compared with (bge_epochs.hpp).  Every call that can write pos,
    // euler, scale, world, quat, velocities, deactivation records, contact words, body types or flags moves BOTH epochs on (epochs_edit), which invalidates all
    // words.  A tick whose launches include another kernel that writes euler, scale, world or quat moves the rows epoch alone; a tick
    // of a variant without the rest path moves the rest epoch alone.
    DevBuf rs_word;
    bge::PathEpochs epochs;
    // The deferred translation row (bge_epochs.hpp Row3State): a tick with TickParams::defer_row3 leaves row 3 of the
    // translation-row waves unstored.  ensure_row3_current() stores them (k_row3_sync) and runs BEFORE the rows epoch moves, before the
    // words are zeroed and before anything but a translation-row tick writes pos or world — words_clear() and epochs_edit() see to
    // the first two themselves; a call that writes pos before its epochs_edit() (upload_trs, bge_world_set_topology) and a tick
    // without the translation-row path call it first.  Readers that run every frame compose instead (row3_view()).
    // Fused ticks (bge_epochs.hpp FuseClock): one word per wave64, zeroed with every layout, and the serials of the
    // launches it is compared with.  No host call but tick_impl and the layout touches either.
    DevBuf adv;
    bge::FuseClock fuse;
    bge::Row3State row3;
    bge::Row3View row3_view() const { return bge::Row3View{view.rs_word, view.pos, row3.pending}; }
    hipError_t ensure_row3_current()
    {
        const uint32_t due = row3.take_sync();
        if (due == 0u || !rs_word.p) return hipSuccess;
        return bge::launch_row3_sync(stream, view, flat.n_tiles_ticked, due);
    }
    void words_clear()
    {
        (void)ensure_row3_current();
        if (rs_word.p) (void)hipMemsetAsync(rs_word.p, 0, rs_word.bytes, stream);
    }
    void epochs_edit()
    {
        (void)ensure_row3_current();
        if (epochs.host_edit()) words_clear();
    }
    // Dynamic boxes on the Static / Kinematic box colliders of the scene (round 3, bge_contact.hip): off by default, like the plane
    bool static_contacts = false;
    DevBuf obstacle_slots, obstacle_gen, obstacles, obstacle_grid, box_list, box_count;
    bool obstacle_grid_on = true; // BGE_OBSTACLE_GRID=0: every body tests every obstacle (measurements)
    uint32_t n_obstacles = 0;
    bool obstacles_stale = true;                      // the compact list of Static / Kinematic box bodies must be rebuilt
    std::vector<uint8_t> body_shape_host;             // bge_shape per entity index as last uploaded
    std::vector<uint32_t> body_gen_host;              // how often the entity's body was (re)created: a re-created box is a new pair
    std::vector<std::vector<uint32_t>> trig_scratch;  // process_trigger_pairs: this tick's body overlaps per trigger (capacity kept)
    std::vector<std::vector<uint32_t>> trig_scratch_ghosts; // ... and the ghosts met, as trigger indices
    std::vector<uint32_t> trig_union;                 // ... and the union being diffed
    std::vector<uint32_t> trig_pairs_host;            // ... and the downloaded (trigger, entity) hit list
    bool ground_plane = false; // the reference's static plane y = 0 (PhysicsSystem.cpp:149-166); off: free bodies (BASELINE's workloads)
    DevBuf bp_partials; // per-wave bounds / count / widest extent written by the tick kernel for the broadphase (32 B per wave)
    float grav_cached[3] = {0.0f, 0.0f, 0.0f};
    bool grav_palette_stale = true; // the mass palette or the gravity vector changed since the table was built
    // Collision-filter palette: scenes use a handful of (layer, mask, static) combinations, so the broadphase's sorted
    // records carry an 8-bit class instead of two 32-bit words (32-byte records instead of 48).  Class 0 = (1, ~0, not
    // static), the component defaults; with more than 255 combinations the broadphase falls back to full records.
    struct FilterKey {
        uint32_t group, mask, is_static;
        bool operator==(const FilterKey& o) const { return group == o.group && mask == o.mask && is_static == o.is_static; }
    };
    std::vector<FilterKey> filter_palette{FilterKey{1u, 0xffffffffu, 0u}};
    bool filter_overflow = false;
    bool filter_table_stale = true;
    uint32_t filter_class_of(uint32_t group, uint32_t mask, bool is_static)
    {
        const FilterKey k{group, mask, is_static ? 1u : 0u};
        for (size_t c = 0; c < filter_palette.size(); ++c) {
            if (filter_palette[c] == k) return static_cast<uint32_t>(c);
        }
        if (filter_palette.size() >= 255) {
            filter_overflow = true;
            return 0;
        }
        filter_palette.push_back(k);
        filter_table_stale = true;
        return static_cast<uint32_t>(filter_palette.size() - 1);
    }
    // Bullet's defaults (btRigidBodyConstructionInfo: 0.8 / 1.0; gDeactivationTime 2 s) — the reference never changes them
    float sleep_lin = 0.8f, sleep_ang = 1.0f, sleep_time = 2.0f;
    void fill_sleep(bge::TickParams& p) const
    {
        p.sleep_lin = sleep_lin;
        p.sleep_lin2 = sleep_lin * sleep_lin;
        p.sleep_ang2 = sleep_ang * sleep_ang;
        p.sleep_time = sleep_time;
    }
    std::vector<float> palette_inv_mass;            // class -> inv_mass (class 0 = 0: Static / Kinematic)
    std::unordered_map<uint32_t, uint32_t> palette_class; // inv_mass bits -> class
    bge::Broadphase broadphase;
    // sharded broadphase (bge_route.hip): records routed to spatial slabs, pair search over what was received
    bge::ShardRouter router;
    bge::Broadphase slab_broadphase;
    // Dynamic boxes against each other (bge_island.hip): a broadphase of its own over the sub-step's fed AABBs (the tick's
    // pair list and the trigger query keep theirs), the sorted pair cache with its manifolds in two generations, per-slot scratch
    bool dynamic_contacts = false;
    bool static_contacts_ever = false; // bge_world_set_static_contacts(1) was called: bodies may hold manifolds with obstacles
    bge::Broadphase island_bp;
    DevBuf isl_slot_words, isl_counts, isl_identity, isl_gen, isl_keys_raw, isl_keys[2], isl_man[2], isl_body_keys_raw, isl_body_slot_raw,
        isl_body_keys, isl_body_slot, isl_solver_bodies, isl_rows, isl_sort_tmp, isl_big_list, isl_body_words, isl_ints;
    PinnedBuf isl_counts_host;
    int isl_cur = 0;
    uint32_t isl_n_prev = 0;
    uint64_t isl_identity_n = 0;
    bool isl_gen_stale = true;
    uint32_t isl_last_pairs = 0, isl_last_bodies = 0;
    uint32_t isl_big_points = 128; // islands with more contact points go to the workgroup solver (BGE_ISLAND_BIG_POINTS: tests force it)
    bool bp_shared = false; // this sub-step's island phases ran `broadphase` on the boxes the tick would run it on: the tick skips its run
    uint64_t isl_pair_cap = 0; // pair capacity of island_bp (grows by itself unless bge_world_create fixed pair_capacity)
    bool pairs_from_slab = false;          // bge_world_pairs reads the slab search (global ids) instead of the local one
    std::vector<uint32_t> global_id_host;  // per entity index; empty = identity
    DevBuf global_of_slot, bp_send, bp_recv, bp_small, bp_hist;
    bool global_of_slot_stale = true;
    bge::RootComm comm;
    bge::WorldView view{};

    // trigger volumes: host runtime (what PhysicsSystem keeps in m_triggerRuntime) + device mirrors
    struct Trigger {
        uint32_t entity = 0;
        uint8_t shape = 0;
        float size[3] = {0.5f, 0.5f, 0.5f};
        uint32_t layer = 4, mask = 0xffffffffu;
        bool one_shot = false;
        bool component_active = true; // TriggerVolume::active
        bool runtime_active = false;  // ghost is in the world
        bool posed = false;           // ... and a tick has posed it on the device since
        // The entity lost its Transform: EnsureTrigger returns before it touches the ghost (PhysicsSystem.cpp:530-534) and nothing
        // removes it, so the ghost stays in the world where it last was and keeps reporting overlaps.
        bool frozen = false;
        float frozen_aabb[6] = {0, 0, 0, 0, 0, 0};
        float frozen_pose[8] = {0, 0, 0, 0, 0, 0, 0, 1}; // ... and the pose (origin, 0, quaternion) the ray queries see it at
        std::vector<uint32_t> overlaps;       // sorted entity indices of the previous tick: the union of the two lists below
        std::vector<uint32_t> overlap_bodies; // ... met as rigid bodies (of any type: the pair cache pairs a ghost with Static bodies too)
        std::vector<uint32_t> overlap_ghosts; // ... met as other trigger ghosts (each of two overlapping ghosts lists the other)
        void clear_overlaps()
        {
            overlaps.clear();
            overlap_bodies.clear();
            overlap_ghosts.clear();
        }
    };
    bool owns_transform(uint32_t e) const
    {
        return e < flat.slot_of_entity.size() && flat.slot_of_entity[e] != bge::kNone && !(e < orphan_host.size() && orphan_host[e]);
    }
    std::vector<Trigger> triggers; // in upload order = the order ProcessTriggerEvents' loop walks them (bge_world.h)
    std::unordered_map<uint32_t, uint32_t> trig_index_of_entity;
    std::vector<bge_trigger_event> trigger_events; // since the last bge_world_trigger_events
    bool triggers_device_stale = true;
    bool trig_list_on_device = false; // the device arrays are indexed like `triggers` (false between an upload of the list and the next sync)
    DevBuf trig_slot, trig_entity, trig_he, trig_group, trig_mask, trig_active, trig_aabb, trig_pairs, trig_count, trig_lists;
    DevBuf trig_pose; // [triggers][8] ghost pose written beside the box by k_trigger_aabb (ray queries)
    // queries (bge_query.hip): staging for the host entry points, the per-query keys (all ones between calls), the all-hits
    // list, and the ghosts the queries see (rebuilt from `triggers` per query, uploaded when it changed)
    DevBuf query_in, query_out, query_keys, query_all, query_all_count, query_ghosts;
    uint64_t query_keys_n = 0;
    // the query index (bge_qindex.hip; include/bge_world.h "Query index"): the desc in force, the buffers of a build (grow-only),
    // and what the last call that queried did
    bge_query_index_desc qi_desc{0u, 0.0f, 0u, 0u, BGE_QUERY_INDEX_MIN_WORK_DEFAULT};
    DevBuf qi_count, qi_start, qi_cell, qi_rec_a, qi_rec_b, qi_rec_c, qi_scan, qi_words, qi_far;
    uint32_t qi_scan_table = 0;
    size_t qi_scan_bytes = 0;
    bool qi_last_built = false;
    float qi_last_edge = 0.0f;
    uint32_t qi_last_table = 0;
    uint64_t qi_builds = 0;
    uint32_t query_all_cap = 0;
    std::vector<bge::QueryGhost> query_ghosts_host, query_ghosts_dev;
    // sphere moves (bge_move.hip): staging for the host entry point, the per-mover state, and the cast / hit records of the passes
    DevBuf move_in, move_out, move_state, move_casts, move_hits;
    // sphere step moves (bge_step.hip): the same, its own; the cast / hit records hold two lanes per mover
    DevBuf step_in, step_out, step_state, step_casts, step_hits;
    // sphere recovery (bge_recover.hip): the same for its passes, and its own (k_move_step relies on being the only writer of move_casts)
    DevBuf recover_in, recover_out, recover_state, recover_queries, recover_hits;
    // characters (bge_character.hip): the resident desc / input / state records of the set, the records its steps hand to the
    // recovery and the step move and get back, and the step's scratch
    DevBuf char_desc, char_input, char_state, char_recover_in, char_recover_out, char_step_in, char_step_out, char_scratch;
    uint64_t n_characters = 0;
    // character platform riding (bge_ride.hip): the resident bge_character_ride records of the set while riding is on
    DevBuf char_ride;
    bool ride_on = false;
    uint32_t ride_flags = 0;
    // crowd separation (bge_crowd.hip): staging for the host entry point, the snapshot records, the grid path's per-sphere
    // {bucket, rank}, bucket counts / offsets, scan storage and r_max word; the resident bge_crowd_hit records and filters of the
    // character set while its crowd is on
    DevBuf crowd_in, crowd_out, crowd_rec_a, crowd_rec_b, crowd_cell, crowd_count, crowd_start, crowd_scan, crowd_rmax;
    uint32_t crowd_scan_table = 0; // the table size crowd_scan is sized for
    size_t crowd_scan_bytes = 0;
    DevBuf char_crowd_hits, char_crowd_group, char_crowd_mask;
    bool char_crowd_on = false;
    float char_crowd_max_push = 0.0f;
    float char_r_max = 0.0f; // the largest desc.radius of the set
    // impulses (bge_impulse.hip): staging for the host entry point, the (slot, record index) pairs before and after the sort and
    // hipcub's storage (grow-only, sized for imp_cap records); the resident push records of the character set while push is on
    DevBuf imp_in, imp_status, imp_keys[2], imp_vals[2], imp_sort;
    uint64_t imp_cap = 0, imp_sort_n = 0; // records the pair arrays hold; the n imp_sort_need was asked for
    size_t imp_sort_need = 0;
    DevBuf char_push_records;
    bool char_push_on = false;
    bge_character_push_desc char_push_desc{0u, 0.0f, 0.0f, 0u};
    // character trigger events (bge_chartrig.hip): the per-character filters, the two [triggers][ceil(n / 64)] bitmaps
    // (ct_bits[ct_rem] = remembered, the other = remembered before the last update call), the per-(ghost, word) counts / offsets, the
    // per-ghost totals, bases and {trigger, entity} of the last call, the event list and its count
    DevBuf ct_group, ct_mask, ct_bits[2], ct_counts, ct_row_total, ct_row_base, ct_ghost_rec, ct_events, ct_count, ct_src_row;
    bool ct_on = false;
    uint32_t ct_flags = 0;
    int ct_rem = 0;
    uint64_t ct_rows = 0, ct_words = 0, ct_cap = 0;
    uint32_t ct_last_ghosts = 0; // ghosts of the last update call: with ct_bits and the offsets, what makes its list again
    // debug overlay (bge_debug.hip): per-workgroup line counts and their offsets, the host entry point's line buffer and total
    DevBuf dbg_block_sum, dbg_block_off, dbg_lines, dbg_total;
    // frustum culling (bge_cull.hip): the model-space bounds per ENTITY (a row of NaNs = no bounds), the pass's ballots / counts /
    // offsets, the host entry point's records and total
    EntityBuf bounds{6};
    DevBuf cull_ballots, cull_block_sum, cull_block_off, cull_out, cull_total;
    // draw batches (bge_batch.hip): the draw key per ENTITY (all ones = no key), the sort's ping-pong records and digit tables, the
    // host entry point's batches
    EntityBuf draw_keys{1};
    DevBuf batch_sort, batch_hist, batch_out;
    uint32_t trigger_grid_min = 64;       // more ghosts than this: the broadphase grid answers for the small ones
    // Enter / Exit taken on the device (bge_kernels.hpp TriggerDiff): two key tables (this tick's, last tick's), header + deltas in
    // one device buffer with a page-locked copy.  The overlap sets above stay the truth; `trig_mirror_valid` says that last tick's
    // table holds exactly them — it is rebuilt from them after every tick that went the long way or changed them on the host.
    DevBuf trig_tab[2], trig_delta_dev, trig_keys_dev;
    uint32_t trig_tab_log2 = 0;
    PinnedBuf trig_delta_host;
    bool trig_mirror_valid = false;
    bool trig_device_diff = true;         // BGE_TRIGGER_DEVICE_DIFF=0 keeps every tick on the host's path (A/B, tests)
    bool trig_stay_events = true;         // bge_world_set_trigger_stay_events
    uint64_t trig_stay_suppressed = 0;    // Stay events not materialised since the last bge_world_trigger_events
    uint64_t trig_fast_ticks = 0, trig_slow_ticks = 0;
    double trig_wait_ms = 0.0, trig_apply_ms = 0.0; // BGE_TRIGGER_PROFILE=1: time until the deltas are on the host / spent applying them
    uint64_t trig_deltas_seen = 0;
    std::vector<uint64_t> trig_keys_host;
    std::vector<uint32_t> trig_exits, trig_touched;
    std::vector<uint8_t> trig_was;
    uint64_t trig_total_overlaps = 0;     // sum of the sets' sizes over the volumes in the world (kept by the short way, recounted by the long one)
    uint32_t trig_through_grid = 0, trig_against_all = 0; // how the last tick split them
    bge::TriggerView trigger_view() const
    {
        bge::TriggerView t{};
        t.slot = trig_slot.as<uint32_t>();
        t.entity = trig_entity.as<uint32_t>();
        t.half_extent = trig_he.as<float>();
        t.group = trig_group.as<uint32_t>();
        t.mask = trig_mask.as<uint32_t>();
        t.active = trig_active.as<uint8_t>();
        t.aabb = trig_aabb.as<float>();
        t.pose = trig_pose.as<float>();
        return t;
    }

    // optional event-pair timing of the tick kernels
    int profiling = 0;                   // 0 off, 1 one pair per tick_many call, 2 one pair per tick
    std::vector<hipEvent_t> prof_events; // start/stop pairs
    size_t prof_used = 0;                // events recorded since the last read
    std::vector<uint32_t> prof_ticks_pending; // ticks covered by each recorded pair
    double prof_ms_carry = 0.0;          // time of pairs folded in when the ring wrapped
    uint64_t prof_ticks_carry = 0;

    void rebuild_view()
    {
        view.flags = flags.as<uint32_t>();
        view.parent = parent.as<uint32_t>();
        view.tile_hdr = tile_hdr.as<uint32_t>();
        view.pos = pos.as<float>();
        view.euler = euler.as<float>();
        view.scale = scale.as<float>();
        view.world = world.as<float>();
        view.vel = vel.as<float>();
        view.angvel = angvel.as<float>();
        view.quat = quat.as<float>();
        view.inv_mass = inv_mass.as<float>();
        view.half_extent = half_extent.as<float>();
        view.group = group.as<uint32_t>();
        view.mask = mask.as<uint32_t>();
        view.aabb = aabb.as<float>();
        view.mass_palette = mass_palette.as<float2>();
        view.grav_palette = grav_palette.as<float4>();
        view.deact = deact.as<uint32_t>();
        view.filter_class = filter_class.as<uint32_t>();
        view.root_index = root_index.as<uint32_t>();
        view.normal = normal.as<float>();
        view.cshape = cshape.as<float4>();
        view.cmass = cmass.as<float>();
        view.cfriction = cfriction.as<float>();
        view.cinfo = cinfo.as<uint32_t>();
        view.manifold = manifold.as<float>();
        view.crestitution = crestitution.as<float>();
        view.bmanifold = bmanifold.as<uint32_t>();
        view.frozen = frozen.as<uint32_t>();
        view.rs_word = rs_word.as<uint32_t>();
        view.adv = adv.as<uint32_t>();
    }
    // What is not memory; every buffer above frees itself after this body.  The caller has set the world's device and destroys
    // the world's own stream afterwards (bge_world_destroy).
    ~bge_world()
    {
        comm.destroy();
        for (hipEvent_t e : prof_events) (void)hipEventDestroy(e);
    }
};

namespace {

// Mass class of an inverse mass: scenes use a handful of distinct masses, so the kernel reads (inv_mass, mass)
// from a 64-entry palette instead of 4 B per body; the 63rd distinct value onwards uses the per-slot array.
uint32_t mass_class(bge_world* w, float inv_mass, bool& palette_changed)
{
    uint32_t bits;
    std::memcpy(&bits, &inv_mass, 4);
    auto it = w->palette_class.find(bits);
    if (it != w->palette_class.end()) return it->second;
    if (w->palette_inv_mass.size() >= bge::kMassClassArray) return bge::kMassClassArray;
    const uint32_t cls = static_cast<uint32_t>(w->palette_inv_mass.size());
    w->palette_inv_mass.push_back(inv_mass);
    w->palette_class[bits] = cls;
    palette_changed = true;
    return cls;
}

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

int check_range(const bge_world* w, uint64_t first, uint64_t count)
{
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (!w->has_topology) return fail(BGE_ERR_STATE, "bge_world_set_topology has not been called");
    if (first > w->flat.n_entities || count > w->flat.n_entities - first) {
        return fail(BGE_ERR_INVALID, "entity range [%llu, +%llu) outside [0, %llu)", (unsigned long long)first,
                    (unsigned long long)count, (unsigned long long)w->flat.n_entities);
    }
    return BGE_OK;
}

// device copy of an explicit entity-index list (validated against n_entities), or null for a range call
int stage_index(bge_world* w, uint64_t count, const uint32_t* index, const uint32_t** dev)
{
    *dev = nullptr;
    if (!index) return BGE_OK;
    for (uint64_t i = 0; i < count; ++i) {
        if (index[i] >= w->flat.n_entities) {
            return fail(BGE_ERR_INVALID, "entity_index[%llu] = %u outside [0, %llu)", (unsigned long long)i, index[i],
                        (unsigned long long)w->flat.n_entities);
        }
    }
    HIP_TRY(w->stage2.ensure(count * 4));
    HIP_TRY(hipMemcpyAsync(w->stage2.p, index, count * 4, hipMemcpyHostToDevice, w->stream));
    *dev = w->stage2.as<uint32_t>();
    return BGE_OK;
}

// What an X(first, count, ...) / X_indexed(count, entity_index, ...) pair of entry points was called with
struct Entities {
    uint64_t first, count;
    const uint32_t* index; // the host's list (X_indexed)
    bool indexed;
    static Entities range(uint64_t first, uint64_t count) { return {first, count, nullptr, false}; }
    static Entities list(uint64_t count, const uint32_t* index) { return {0, count, index, true}; }
};
constexpr int kNothingToDo = 1; // what `pre` answers for count == 0: BGE_OK, and nothing more happens

// The prologue those entry points share.  `pre()` holds what differs before the list is staged: the payload's NULL tests and the
// count == 0 exit, in the entry point's own order; then `body(device index list or null)` runs.
template <class Pre, class Body>
int with_entities(bge_world* w, const Entities& e, Pre pre, Body body, const char* null_index = "entity_index is NULL")
{
    if (int rc = e.indexed ? check_range(w, 0, 0) : check_range(w, e.first, e.count)) return rc;
    if (e.indexed && e.count && !e.index) return fail(BGE_ERR_INVALID, "%s", null_index);
    DeviceGuard guard(w->device);
    if (int rc = pre()) return rc == kNothingToDo ? BGE_OK : rc;
    const uint32_t* di = nullptr;
    if (int rc = stage_index(w, e.count, e.index, &di)) return rc;
    return body(di);
}

// upload one host array of `count` rows into a per-slot device array
int upload_rows(bge_world* w, uint64_t first, uint64_t count, const void* host, SlotBuf& dst, uint32_t or_bits,
                const uint32_t* dev_index = nullptr, uint32_t need_bits = 0)
{
    const size_t bytes = dst.bytes_for(count);
    HIP_TRY(w->stage.ensure(bytes));
    HIP_TRY(hipMemcpyAsync(w->stage.p, host, bytes, hipMemcpyHostToDevice, w->stream));
    HIP_TRY(bge::launch_scatter_rows(w->stream, w->slot_of_entity.as<uint32_t>(), first, count, dst.words, w->stage.p, dst.p,
                                     w->flags.as<uint32_t>(), or_bits, dev_index, need_bits, dst.vel_blocks));
    // the staging buffer is reused by the next call
    HIP_TRY(hipStreamSynchronize(w->stream));
    return BGE_OK;
}

// (the velocity blocks are not rows of `words` words: always through the gather kernel)
int download_rows(bge_world* w, uint64_t first, uint64_t count, const SlotBuf& src, void* host, const uint32_t* dev_index = nullptr)
{
    const size_t bytes = src.bytes_for(count);
    if (&src == &w->world && w->row3.pending != 0u) {
        // translation rows are deferred: the gather composes them (a frame that ticks and downloads does not pay for the store as well)
        HIP_TRY(w->stage.ensure(bytes));
        HIP_TRY(bge::launch_gather_world(w->stream, w->slot_of_entity.as<uint32_t>(), first, count, w->view, w->row3_view(), w->stage.p, dev_index));
        HIP_TRY(hipMemcpyAsync(host, w->stage.p, bytes, hipMemcpyDeviceToHost, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream));
        return BGE_OK;
    }
    if (w->flat.identity && !dev_index && !src.vel_blocks) {
        // flat scene: slot == entity index, the rows are already contiguous in entity order
        HIP_TRY(hipMemcpyAsync(host, src.as<char>() + src.bytes_for(first), bytes, hipMemcpyDeviceToHost, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream));
        return BGE_OK;
    }
    HIP_TRY(w->stage.ensure(bytes));
    HIP_TRY(bge::launch_gather_rows(w->stream, w->slot_of_entity.as<uint32_t>(), first, count, src.words, src.p, w->stage.p, dev_index,
                                    src.vel_blocks));
    HIP_TRY(hipMemcpyAsync(host, w->stage.p, bytes, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return BGE_OK;
}

// Make an optional store exist for the current layout when its feature is switched on.  bge_world_set_topology keeps an existing
// store sized for the layout, so a smaller one cannot survive — checked by size all the same: the kernels load and store
// a[words * slot ..] for every slot of the layout.  (synced: the caller has just waited for the stream)
int make_store(bge_world* w, SlotBuf& a, bool synced = false)
{
    if (!w->has_topology || a.bytes >= a.bytes_for(w->slot_rows())) return BGE_OK;
    if (!synced) HIP_TRY(hipStreamSynchronize(w->stream));
    HIP_TRY(a.ensure(a.bytes_for(w->slot_rows())));
    HIP_TRY(hipMemsetAsync(a.p, a.fill, a.bytes, w->stream));
    w->rebuild_view();
    return BGE_OK;
}

} // namespace

namespace {
constexpr uint32_t kTriggerPairCap = 1u << 20;

// device mirrors of the trigger set (slots follow the current topology)
int sync_triggers_to_device(bge_world* w)
{
    const size_t n = w->triggers.size();
    if (n == 0) return BGE_OK;
    std::vector<uint32_t> slot(n), entity(n), group(n), mask(n);
    std::vector<float> he(3 * n);
    std::vector<uint8_t> active(n);
    for (size_t i = 0; i < n; ++i) {
        const bge_world::Trigger& t = w->triggers[i];
        entity[i] = t.entity;
        slot[i] = w->owns_transform(t.entity) ? w->flat.slot_of_entity[t.entity] : bge::kNone;
        collider_half_extents(t.shape, t.size, &he[3 * i]);
        group[i] = t.layer;
        mask[i] = t.mask;
        active[i] = t.runtime_active && slot[i] != bge::kNone ? 1 : 0;
        if (t.runtime_active && t.frozen) {
            slot[i] = bge::kFrozenGhost; // k_trigger_aabb leaves its box alone
            active[i] = 1;
        }
    }
    HIP_TRY(w->trig_slot.ensure(n * 4));
    HIP_TRY(w->trig_entity.ensure(n * 4));
    HIP_TRY(w->trig_he.ensure(n * 12));
    HIP_TRY(w->trig_group.ensure(n * 4));
    HIP_TRY(w->trig_mask.ensure(n * 4));
    HIP_TRY(w->trig_active.ensure(n));
    HIP_TRY(w->trig_aabb.ensure(n * 24));
    HIP_TRY(w->trig_pose.ensure(n * 32));
    HIP_TRY(w->trig_pairs.ensure(static_cast<size_t>(kTriggerPairCap) * 8));
    HIP_TRY(w->trig_count.ensure(64));
    HIP_TRY(hipMemcpyAsync(w->trig_slot.p, slot.data(), n * 4, hipMemcpyHostToDevice, w->stream));
    HIP_TRY(hipMemcpyAsync(w->trig_entity.p, entity.data(), n * 4, hipMemcpyHostToDevice, w->stream));
    HIP_TRY(hipMemcpyAsync(w->trig_he.p, he.data(), n * 12, hipMemcpyHostToDevice, w->stream));
    HIP_TRY(hipMemcpyAsync(w->trig_group.p, group.data(), n * 4, hipMemcpyHostToDevice, w->stream));
    HIP_TRY(hipMemcpyAsync(w->trig_mask.p, mask.data(), n * 4, hipMemcpyHostToDevice, w->stream));
    HIP_TRY(hipMemcpyAsync(w->trig_active.p, active.data(), n, hipMemcpyHostToDevice, w->stream));
    for (size_t i = 0; i < n; ++i) {
        const bge_world::Trigger& t = w->triggers[i];
        if (t.runtime_active && t.frozen) {
            HIP_TRY(hipMemcpyAsync(static_cast<char*>(w->trig_aabb.p) + 24 * i, t.frozen_aabb, 24, hipMemcpyHostToDevice, w->stream));
            HIP_TRY(hipMemcpyAsync(static_cast<char*>(w->trig_pose.p) + 32 * i, t.frozen_pose, 32, hipMemcpyHostToDevice, w->stream));
        }
    }
    HIP_TRY(hipStreamSynchronize(w->stream)); // the host vectors die here
    w->triggers_device_stale = false;
    w->trig_list_on_device = true;
    return BGE_OK;
}

// EnsureTrigger's activation rule, before the step (PhysicsSystem.cpp:573-590)
void ensure_triggers(bge_world* w)
{
    for (bge_world::Trigger& t : w->triggers) {
        const bool has_tf = w->owns_transform(t.entity);
        if (!has_tf && t.runtime_active && t.frozen) continue; // EnsureTrigger returns before it touches the ghost
        if (has_tf && t.frozen) {                              // the Transform is back: posed from it again
            t.frozen = false;
            w->triggers_device_stale = true;
        }
        const bool want = t.component_active && has_tf;
        if (want != t.runtime_active) {
            t.runtime_active = want;
            t.posed = false;
            t.clear_overlaps();
            w->triggers_device_stale = true;
            w->trig_mirror_valid = false;
        }
    }
}

// One trip of ProcessTriggerEvents' loop (PhysicsSystem.cpp:1019-1073) for trigger t: `bodies` = entities met as rigid bodies
// (sorted), `ghosts` = other triggers met, as indices into w->triggers (any order).  A ghost that has left the world since the
// lists were made — a one-shot trigger that fired EARLIER in this loop (:1062-1072 removes it at once, and the pair cache takes
// it out of every other ghost's list) — no longer counts.  An entity met both ways counts once (:1026 std::unordered_set).
void diff_and_commit_trigger(bge_world* w, bge_world::Trigger& t, std::vector<uint32_t>& bodies, std::vector<uint32_t>& ghosts)
{
    size_t kept = 0;
    for (uint32_t j : ghosts) {
        if (j < w->triggers.size() && w->triggers[j].runtime_active) ghosts[kept++] = w->triggers[j].entity;
    }
    ghosts.resize(kept);
    std::sort(ghosts.begin(), ghosts.end());
    std::vector<uint32_t>& cur = w->trig_union;
    cur.resize(bodies.size() + ghosts.size());
    cur.erase(std::set_union(bodies.begin(), bodies.end(), ghosts.begin(), ghosts.end(), cur.begin()), cur.end());
    // (both sets are sorted, so Enter / Stay / Exit come out of two linear merges — with a binary search per overlap the host
    //  side of 92,000 overlaps a tick took 2.7 ms)
    const std::vector<uint32_t>& prev = t.overlaps;
    size_t at = 0;
    for (uint32_t other : cur) {
        while (at < prev.size() && prev[at] < other) ++at;
        const bool was = at < prev.size() && prev[at] == other;
        if (was && !w->trig_stay_events) {
            ++w->trig_stay_suppressed;
            continue;
        }
        w->trigger_events.push_back(bge_trigger_event{was ? 1u : 0u, t.entity, other});
    }
    at = 0;
    for (uint32_t previous : prev) {
        while (at < cur.size() && cur[at] < previous) ++at;
        if (!(at < cur.size() && cur[at] == previous)) w->trigger_events.push_back(bge_trigger_event{2u, t.entity, previous});
    }
    t.overlaps.swap(cur);
    t.overlap_bodies.swap(bodies);
    t.overlap_ghosts.swap(ghosts);
    if (t.one_shot && !t.overlaps.empty()) {
        t.component_active = false;
        t.runtime_active = false; // out of the world, and out of every list, from here on
        t.clear_overlaps();
        w->triggers_device_stale = true;
    }
}

// ProcessTriggerEvents on the hit list the device produced for this tick: (trigger, body entity) from the all-bodies pass and
// the grid look-up, (trigger | kGhostHit, other trigger) from the ghost-against-ghost pass
int process_trigger_pairs(bge_world* w)
{
    uint32_t counters[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(counters, w->trig_count.p, 12, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    const uint32_t n_pairs = counters[0];
    w->trig_against_all = counters[1];
    w->trig_through_grid = counters[2];
    if (n_pairs > kTriggerPairCap) return fail(BGE_ERR_OOM, "%u trigger overlaps in one tick exceed the buffer of %u", n_pairs, kTriggerPairCap);
    std::vector<uint32_t>& pairs = w->trig_pairs_host; // (kept between ticks: no 0.7 MB value-initialisation per tick)
    if (pairs.size() < 2 * static_cast<size_t>(n_pairs)) pairs.resize(2 * static_cast<size_t>(n_pairs));
    if (n_pairs) {
        HIP_TRY(hipMemcpyAsync(pairs.data(), w->trig_pairs.p, 2 * static_cast<size_t>(n_pairs) * 4, hipMemcpyDeviceToHost, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream));
    }
    // (the per-trigger lists keep their capacity from tick to tick)
    std::vector<std::vector<uint32_t>>& bodies = w->trig_scratch;
    std::vector<std::vector<uint32_t>>& ghosts = w->trig_scratch_ghosts;
    const size_t n_trig = w->triggers.size();
    if (bodies.size() < n_trig) bodies.resize(n_trig);
    if (ghosts.size() < n_trig) ghosts.resize(n_trig);
    for (size_t i = 0; i < n_trig; ++i) {
        bodies[i].clear();
        ghosts[i].clear();
    }
    for (uint32_t k = 0; k < n_pairs; ++k) {
        const uint32_t a = pairs[2 * k], b = pairs[2 * k + 1];
        const uint32_t i = a & ~bge::kGhostHit;
        if (i >= n_trig) continue;
        if (a & bge::kGhostHit) ghosts[i].push_back(b);
        else bodies[i].push_back(b);
    }
    w->trigger_events.reserve(w->trigger_events.size() + n_pairs + n_pairs / 4);
    for (size_t i = 0; i < n_trig; ++i) {
        bge_world::Trigger& t = w->triggers[i];
        if (!t.runtime_active) continue;
        std::sort(bodies[i].begin(), bodies[i].end());
        diff_and_commit_trigger(w, t, bodies[i], ghosts[i]);
    }
    return BGE_OK;
}

// ---- the short way: Enter / Exit come from the device (bge_kernels.hpp TriggerDiff), the sets are updated by them
constexpr uint32_t kTrigDeltaCap = 1u << 16;       // deltas fetched with the header in one copy; more than that in a tick: the long way
constexpr uint32_t kTrigHeaderWords = 8;

inline void sorted_insert(std::vector<uint32_t>& v, uint32_t e)
{
    auto it = std::lower_bound(v.begin(), v.end(), e);
    if (it == v.end() || *it != e) v.insert(it, e);
}
inline void sorted_erase(std::vector<uint32_t>& v, uint32_t e)
{
    auto it = std::lower_bound(v.begin(), v.end(), e);
    if (it != v.end() && *it == e) v.erase(it);
}
inline bool sorted_has(const std::vector<uint32_t>& v, uint32_t e) { return std::binary_search(v.begin(), v.end(), e); }

// (Re)build last tick's table from the host's sets: after a tick on the long way, an upload of the trigger list, a (de)activation
int rebuild_trigger_mirror(bge_world* w)
{
    std::vector<uint64_t>& keys = w->trig_keys_host;
    keys.clear();
    w->trig_total_overlaps = 0;
    for (size_t i = 0; i < w->triggers.size(); ++i) {
        const bge_world::Trigger& t = w->triggers[i];
        if (!t.runtime_active) continue;
        w->trig_total_overlaps += t.overlaps.size();
        for (uint32_t e : t.overlap_bodies) keys.push_back((static_cast<uint64_t>(i) << 33) | e);
        for (uint32_t e : t.overlap_ghosts) {
            auto it = w->trig_index_of_entity.find(e);
            if (it != w->trig_index_of_entity.end()) keys.push_back((static_cast<uint64_t>(i) << 33) | (1ull << 32) | it->second);
        }
    }
    uint32_t log2 = 12;
    while ((1ull << log2) < 4 * std::max<uint64_t>(keys.size(), w->trig_pairs_host.size() / 2)) ++log2;
    if (log2 > 26) return fail(BGE_ERR_OOM, "%llu remembered trigger overlaps", (unsigned long long)keys.size());
    if (log2 > w->trig_tab_log2) w->trig_tab_log2 = log2;
    const size_t bytes = sizeof(uint64_t) << w->trig_tab_log2;
    for (DevBuf& b : w->trig_tab) HIP_TRY(b.ensure(bytes));
    HIP_TRY(w->trig_delta_dev.ensure(kTrigHeaderWords * 4 + static_cast<size_t>(kTrigDeltaCap) * 8));
    HIP_TRY(w->trig_delta_host.ensure(kTrigHeaderWords * 4 + static_cast<size_t>(kTrigDeltaCap) * 8));
    HIP_TRY(hipMemsetAsync(w->trig_tab[0].p, 0xff, bytes, w->stream)); // this tick's table for the next diff
    HIP_TRY(hipMemsetAsync(w->trig_tab[1].p, 0xff, bytes, w->stream)); // last tick's
    HIP_TRY(hipMemsetAsync(w->trig_delta_dev.p, 0, kTrigHeaderWords * 4, w->stream));
    if (!keys.empty()) {
        HIP_TRY(w->trig_keys_dev.ensure(keys.size() * 8));
        HIP_TRY(hipMemcpyAsync(w->trig_keys_dev.p, keys.data(), keys.size() * 8, hipMemcpyHostToDevice, w->stream));
        HIP_TRY(bge::launch_trigger_table_build(w->stream, w->trig_tab[1].as<uint64_t>(), w->trig_tab_log2, w->trig_keys_dev.as<uint64_t>(),
                                                static_cast<uint32_t>(keys.size()), w->trig_delta_dev.as<uint32_t>()));
        uint32_t overflow = 0;
        HIP_TRY(hipMemcpyAsync(&overflow, w->trig_delta_dev.as<uint32_t>() + 2, 4, hipMemcpyDeviceToHost, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream)); // (`keys` is read by the copy above)
        if (overflow) return fail(BGE_ERR_HIP, "trigger mirror table overflowed at %llu keys", (unsigned long long)keys.size());
    }
    w->trig_mirror_valid = true;
    return BGE_OK;
}

// One tick's trigger events from the device's deltas.  Returns 1 when the tick has to go the long way after all (too many changes,
// a table overflow), 0 when done, a negative error otherwise.
int process_trigger_pairs_fast(bge_world* w)
{
    const auto t0 = std::chrono::steady_clock::now();
    bge::TriggerDiff d{};
    d.cur = w->trig_tab[0].as<uint64_t>();
    d.prev = w->trig_tab[1].as<uint64_t>();
    d.log2_cap = w->trig_tab_log2;
    d.header = w->trig_delta_dev.as<uint32_t>();
    d.deltas = reinterpret_cast<uint64_t*>(w->trig_delta_dev.as<uint32_t>() + kTrigHeaderWords);
    d.delta_cap = kTrigDeltaCap;
    d.pairs = static_cast<const uint2*>(w->trig_pairs.p);
    d.count = w->trig_count.as<uint32_t>();
    d.pair_cap = kTriggerPairCap;
    HIP_TRY(hipMemsetAsync(d.header, 0, kTrigHeaderWords * 4, w->stream));
    HIP_TRY(bge::launch_trigger_diff(w->stream, d));
    // the header and the first 1,024 deltas in one copy; a tick with more changes fetches the rest in a second one
    constexpr uint32_t kFirst = 1024;
    uint32_t* host = w->trig_delta_host.as<uint32_t>();
    HIP_TRY(hipMemcpyAsync(host, w->trig_delta_dev.p, kTrigHeaderWords * 4 + kFirst * 8, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    const uint32_t n_delta = host[0], n_pairs = host[3];
    w->trig_against_all = host[4];
    w->trig_through_grid = host[5];
    if (n_pairs > kTriggerPairCap) {
        // k_trigger_diff_cur has put this tick's keys into trig_tab[0] already: both tables are rebuilt from the host's sets, which
        // this tick leaves as they were, before the next difference is taken (bge_world.h: a tick that fails this way)
        w->trig_mirror_valid = false;
        return fail(BGE_ERR_OOM, "%u trigger overlaps in one tick exceed the buffer of %u", n_pairs, kTriggerPairCap);
    }
    if (host[2] || n_delta > kTrigDeltaCap || (static_cast<uint64_t>(host[1]) << 1) > (1ull << w->trig_tab_log2)) {
        w->trig_mirror_valid = false; // (both tables are rebuilt, larger, after the long way)
        if (w->trig_pairs_host.size() < 2 * static_cast<size_t>(n_pairs)) w->trig_pairs_host.resize(2 * static_cast<size_t>(n_pairs));
        return 1;
    }
    if (n_delta > kFirst) {
        HIP_TRY(hipMemcpyAsync(host + kTrigHeaderWords + 2 * kFirst, reinterpret_cast<const uint64_t*>(w->trig_delta_dev.as<uint32_t>() + kTrigHeaderWords) + kFirst,
                               static_cast<size_t>(n_delta - kFirst) * 8, hipMemcpyDeviceToHost, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream));
    }
    // this tick's table becomes last tick's; the other one is cleared for the next diff (in stream order, behind the kernels)
    std::swap(w->trig_tab[0], w->trig_tab[1]);
    HIP_TRY(hipMemsetAsync(w->trig_tab[0].p, 0xff, sizeof(uint64_t) << w->trig_tab_log2, w->stream));
    const auto t1 = std::chrono::steady_clock::now();
    uint64_t* deltas = reinterpret_cast<uint64_t*>(host + kTrigHeaderWords);
    std::sort(deltas, deltas + n_delta, [](uint64_t a, uint64_t b) { return (a & ~bge::kTrigKeyExit) < (b & ~bge::kTrigKeyExit); });
    const size_t n_trig = w->triggers.size();
    std::vector<uint32_t>& enters = w->trig_union; // (scratch: the entities that entered the trigger at hand, ascending)
    std::vector<uint32_t>& exits = w->trig_exits;
    std::vector<uint32_t>& touched = w->trig_touched;
    std::vector<uint8_t>& was = w->trig_was;
    uint32_t at = 0;
    uint64_t all_enters = 0;
    // with Stay records every volume in the world is reported; without them only the volumes the deltas name are visited
    for (size_t i = 0; i < n_trig; ++i) {
        if (!w->trig_stay_events) {
            if (at >= n_delta) break;
            i = static_cast<size_t>((deltas[at] & ~bge::kTrigKeyExit) >> 33);
            if (i >= n_trig) break;
        }
        bge_world::Trigger& t = w->triggers[i];
        enters.clear();
        exits.clear();
        touched.clear();
        const uint32_t first = at;
        while (at < n_delta && ((deltas[at] & ~bge::kTrigKeyExit) >> 33) == i) ++at;
        if (!t.runtime_active) continue; // (the device skips a ghost that is not in the world: nothing can be listed for it)
        if (at > first) {
            // the entities whose membership may change, and whether they are members now
            for (uint32_t k = first; k < at; ++k) {
                const uint64_t key = deltas[k] & ~bge::kTrigKeyExit;
                const uint32_t other = static_cast<uint32_t>(key);
                const bool ghost = (key >> 32) & 1ull;
                if (ghost && other >= n_trig) continue;
                touched.push_back(ghost ? w->triggers[other].entity : other);
            }
            std::sort(touched.begin(), touched.end());
            touched.erase(std::unique(touched.begin(), touched.end()), touched.end());
            was.resize(touched.size());
            for (size_t k = 0; k < touched.size(); ++k) was[k] = sorted_has(t.overlaps, touched[k]);
            for (uint32_t k = first; k < at; ++k) {
                const bool exit = (deltas[k] & bge::kTrigKeyExit) != 0;
                const uint64_t key = deltas[k] & ~bge::kTrigKeyExit;
                const uint32_t other = static_cast<uint32_t>(key);
                const bool ghost = (key >> 32) & 1ull;
                if (ghost && other >= n_trig) continue;
                std::vector<uint32_t>& set = ghost ? t.overlap_ghosts : t.overlap_bodies;
                const uint32_t e = ghost ? w->triggers[other].entity : other;
                if (exit) sorted_erase(set, e);
                else sorted_insert(set, e);
            }
            for (size_t k = 0; k < touched.size(); ++k) {
                const uint32_t e = touched[k];
                const bool is = sorted_has(t.overlap_bodies, e) || sorted_has(t.overlap_ghosts, e); // (met both ways counts once)
                if (is && !was[k]) {
                    sorted_insert(t.overlaps, e);
                    enters.push_back(e);
                } else if (!is && was[k]) {
                    sorted_erase(t.overlaps, e);
                    exits.push_back(e);
                }
            }
            w->trig_total_overlaps += enters.size();
            w->trig_total_overlaps -= exits.size();
            all_enters += enters.size();
        }
        // ProcessTriggerEvents' report for this trigger: Enter / Stay over the current set in ascending entity order, then Exit
        if (w->trig_stay_events) {
            size_t en = 0;
            for (uint32_t e : t.overlaps) {
                const bool entered = en < enters.size() && enters[en] == e;
                if (entered) ++en;
                w->trigger_events.push_back(bge_trigger_event{entered ? 0u : 1u, t.entity, e});
            }
        } else {
            for (uint32_t e : enters) w->trigger_events.push_back(bge_trigger_event{0u, t.entity, e});
        }
        for (uint32_t e : exits) w->trigger_events.push_back(bge_trigger_event{2u, t.entity, e});
    }
    if (!w->trig_stay_events) w->trig_stay_suppressed += w->trig_total_overlaps - all_enters;
    ++w->trig_fast_ticks;
    w->trig_wait_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
    w->trig_apply_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    w->trig_deltas_seen += n_delta;
    return 0;
}

// ... and in a call that simulates nothing: no collision detection ran, every ghost's list is last call's — minus the ghosts
// that are no longer in the world (deactivated by EnsureTrigger since, or fired as one-shot earlier in this loop); a volume
// that was made one-shot since fires on what it remembers (PhysicsSystem.cpp:1062-1072)
void process_triggers_without_a_step(bge_world* w)
{
    w->trig_mirror_valid = false; // (a ghost that left the world drops out of the others' lists here, on the host)
    std::vector<uint32_t> bodies, ghosts;
    for (bge_world::Trigger& t : w->triggers) {
        if (!t.runtime_active) continue;
        bodies = t.overlap_bodies;
        ghosts.clear();
        for (uint32_t e : t.overlap_ghosts) {
            auto it = w->trig_index_of_entity.find(e);
            if (it != w->trig_index_of_entity.end()) ghosts.push_back(it->second);
        }
        diff_and_commit_trigger(w, t, bodies, ghosts);
    }
}

// The compact list of what a Dynamic box can rest on — every Static / Kinematic body with a box collider, ascending entity index,
// with the generation of its btRigidBody — and the buffers of the box-contact path (bge_contact.hip); rebuilt after body uploads
// and re-topologies only.
int prepare_obstacles(bge_world* w, uint64_t n_slots)
{
    if (w->box_list.bytes < n_slots * 4 || !w->box_count.p) {
        HIP_TRY(w->box_list.ensure(std::max<uint64_t>(n_slots, 1) * 4));
        HIP_TRY(w->box_count.ensure(64));
        HIP_TRY(hipMemsetAsync(w->box_count.p, 0, 64, w->stream));
    }
    if (!w->obstacles_stale) return BGE_OK;
    std::vector<uint32_t> slots, gens;
    for (uint64_t e = 0; e < w->flat.n_entities && e < w->body_type_host.size(); ++e) {
        const uint8_t t = w->body_type_host[e];
        if (t != BGE_BODY_STATIC && t != BGE_BODY_KINEMATIC) continue;
        if (e < w->body_shape_host.size() && w->body_shape_host[e] == BGE_SHAPE_CAPSULE) continue;
        const uint32_t sl = w->flat.slot_of_entity[e];
        if (sl == bge::kNone) continue;
        slots.push_back(sl);
        gens.push_back(e < w->body_gen_host.size() ? w->body_gen_host[e] : 0u);
    }
    w->n_obstacles = static_cast<uint32_t>(slots.size());
    const size_t n = std::max<size_t>(slots.size(), 1);
    HIP_TRY(hipStreamSynchronize(w->stream)); // (a kernel of the previous tick may still read the old list)
    HIP_TRY(w->obstacle_slots.ensure(n * 4));
    HIP_TRY(w->obstacle_gen.ensure(n * 4));
    HIP_TRY(w->obstacles.ensure(n * sizeof(bge::ObstacleRec)));
    // (an obstacle on the grid covers at most 64 cells: 64 items each is a capacity that cannot overflow)
    if (w->n_obstacles > bge::kObstacleGridMin) HIP_TRY(w->obstacle_grid.ensure((bge::kObstacleGridItems + 64ull * n) * 4));
    if (!slots.empty()) {
        HIP_TRY(hipMemcpy(w->obstacle_slots.p, slots.data(), slots.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(w->obstacle_gen.p, gens.data(), gens.size() * 4, hipMemcpyHostToDevice));
    }
    w->obstacles_stale = false;
    return BGE_OK;
}

// the world's collision-filter palette as the broadphase takes it (uploads the table when it changed)
int filter_palette_of(bge_world* w, bge::FilterPalette* out)
{
    if (w->filter_table_stale && !w->filter_overflow) {
        std::vector<uint32_t> tab(256 * 4, 0u);
        for (size_t c = 0; c < w->filter_palette.size(); ++c) {
            tab[4 * c] = w->filter_palette[c].group;
            tab[4 * c + 1] = w->filter_palette[c].mask;
            tab[4 * c + 2] = w->filter_palette[c].is_static;
        }
        HIP_TRY(hipMemcpyAsync(w->filter_table.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream)); // `tab` is a local
        w->filter_table_stale = false;
    }
    *out = bge::FilterPalette{w->filter_overflow ? nullptr : w->filter_class.as<uint32_t>(), w->filter_overflow ? nullptr : w->filter_table.as<uint4>(),
                              static_cast<uint32_t>(w->filter_palette.size())};
    return BGE_OK;
}

// One sub-step's collision detection and constraint solving for the Dynamic boxes that touch each other (bge_island.hip;
// oracle/physics_ref.h CollideDynamicPairs / StepIsland).  Runs before k_ground_select; two small read-backs (pairs, island bodies)
// size the sorts between its phases.
int island_substep(bge_world* w, bge::GroundParams& gp, uint64_t n_slots, bool bullet_basis, bool later_sub_step, bool tick_wants_pairs)
{
    const uint64_t n_entities = std::max<uint64_t>(w->flat.n_entities, 1);
    HIP_TRY(w->isl_slot_words.ensure(std::max<uint64_t>(n_slots, 1) * 16));
    if (!w->isl_counts.p) {
        HIP_TRY(w->isl_counts.ensure(64));
        HIP_TRY(hipMemsetAsync(w->isl_counts.p, 0, 64, w->stream));
    }
    HIP_TRY(w->isl_counts_host.ensure(64));
    const uint32_t* const counts_host = w->isl_counts_host.as<uint32_t>();
    if (w->isl_identity_n < n_slots) {
        std::vector<uint32_t> iota(n_slots);
        for (uint64_t i = 0; i < n_slots; ++i) iota[i] = static_cast<uint32_t>(i);
        HIP_TRY(hipStreamSynchronize(w->stream));
        HIP_TRY(w->isl_identity.ensure(n_slots * 4));
        HIP_TRY(hipMemcpy(w->isl_identity.p, iota.data(), n_slots * 4, hipMemcpyHostToDevice));
        w->isl_identity_n = n_slots;
    }
    if (w->isl_gen_stale || w->isl_gen.bytes < n_entities * 4) {
        std::vector<uint32_t> gens(n_entities, 0u);
        for (uint64_t e = 0; e < n_entities && e < w->body_gen_host.size(); ++e) gens[e] = w->body_gen_host[e];
        HIP_TRY(hipStreamSynchronize(w->stream));
        HIP_TRY(w->isl_gen.ensure(n_entities * 4));
        HIP_TRY(hipMemcpy(w->isl_gen.p, gens.data(), n_entities * 4, hipMemcpyHostToDevice));
        w->isl_gen_stale = false;
    }
    // pair_capacity: what bge_world_create was given, or — left to the world — 8 pairs per entity to begin with, doubled whenever a
    // sub-step finds more (the pair search reports Dynamic-Static pairs too: a dropped pair would be two bodies passing through each other)
    if (w->isl_pair_cap == 0) w->isl_pair_cap = w->pair_capacity_req ? w->pair_capacity_req : std::max<uint64_t>(8 * w->flat.n_entities, 4096);
    if (!w->pair_capacity_req) w->isl_pair_cap = std::max<uint64_t>(w->isl_pair_cap, std::max<uint64_t>(8 * w->flat.n_entities, 4096));

    bge::IslandParams ip{};
    ip.dt = gp.dt;
    ip.gx = gp.gx;
    ip.gy = gp.gy;
    ip.gz = gp.gz;
    ip.n_slots = n_slots;
    ip.repose = gp.repose;
    ip.entity_of_slot = w->entity_of_slot.as<uint32_t>();
    ip.slot_of_entity = w->slot_of_entity.as<uint32_t>();
    ip.gen_of_entity = w->isl_gen.as<uint32_t>();
    ip.counts = w->isl_counts.as<uint32_t>();
    ip.parent = w->isl_slot_words.as<uint32_t>();
    ip.member = ip.parent + n_slots;
    ip.active = ip.member + n_slots;
    ip.index_of_slot = ip.active + n_slots;
    gp.entity_of_slot = w->entity_of_slot.as<uint32_t>();

    HIP_TRY(hipMemsetAsync(w->isl_counts.p, 0, 12, w->stream)); // (word 3, the error bits, stays: the solver's are read with the NEXT sub-step's counts)
    HIP_TRY(hipMemsetAsync(w->isl_counts.as<uint32_t>() + 4, 0, 16, w->stream));
    if (w->static_contacts) HIP_TRY(bge::launch_obstacles(w->stream, w->view, gp));
    gp.obstacles_ready = 1u;
    HIP_TRY(bge::launch_island_begin(w->stream, w->view, gp, ip, bullet_basis));
    gp.repose = 0u; // (done: k_ground_select must not derive the quaternions a second time from the angles k_island_begin wrote)
    bge::FilterPalette palette{};
    if (int prc = filter_palette_of(w, &palette)) return prc;
    // The tick's own broadphase (BGE_TICK_BROADPHASE: pairs for the caller, the trigger query) sees exactly these boxes after k_tick — the
    // fed AABBs of the sub-step's start — so when it is asked for, it runs HERE, once, and the tick skips its run (bp_shared).  Its
    // capacity is the world's; should it drop pairs, the island path repeats the search with its own instance, which grows.
    bool shared = tick_wants_pairs;
    w->bp_shared = false;
    for (;;) {
        bge::Broadphase& bp = shared ? w->broadphase : w->island_bp;
        const uint64_t cap = shared ? (w->pair_capacity_req ? w->pair_capacity_req : std::max<uint64_t>(8 * w->flat.n_entities, 4096)) : w->isl_pair_cap;
        int rc = bp.configure(std::max<uint64_t>(w->flat.n_slots, bge::kTile), cap);
        if (rc != BGE_OK) return fail(rc, "broadphase allocation failed: %s", bp.error());
        HIP_TRY(w->isl_keys_raw.ensure(cap * 8));
        ip.keys_raw = w->isl_keys_raw.as<uint64_t>();
        ip.pair_cap = static_cast<uint32_t>(std::min<uint64_t>(cap, 0xffffffffu));
        ip.bp_ids_are_entities = shared ? 1u : 0u;
        rc = bp.run(w->stream, w->view, n_slots, shared ? w->entity_of_slot.as<uint32_t>() : w->isl_identity.as<uint32_t>(), nullptr, &palette, nullptr);
        if (rc != BGE_OK) return fail(rc, "broadphase failed: %s", bp.error());
        const bge::PairSlices sl = bp.slices();
        ip.bp_stage = sl.stage;
        ip.bp_counts = sl.counts;
        ip.bp_shard_cap = sl.shard_cap;
        ip.bp_shards = sl.shards;
        HIP_TRY(bge::launch_island_pair_keys(w->stream, w->view, ip));
        HIP_TRY(hipMemcpyAsync(w->isl_counts_host.p, w->isl_counts.p, 16, hipMemcpyDeviceToHost, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream));
        if (counts_host[3] & 5u) {
            HIP_TRY(hipMemsetAsync(w->isl_counts.p, 0, 64, w->stream));
            return fail(BGE_ERR_HIP, "internal error in the island solver of the previous sub-step (bits %#x): row pool exhausted or an obstacle record missing",
                        counts_host[3]);
        }
        if (!(counts_host[3] & 2u) && counts_host[0] <= ip.pair_cap) {
            w->bp_shared = shared;
            break;
        }
        HIP_TRY(hipMemsetAsync(w->isl_counts.p, 0, 64, w->stream));
        if (shared) { // (the tick's run will report what the world's capacity does to ITS pair list; the islands need every pair)
            shared = false;
            continue;
        }
        if (w->pair_capacity_req || cap >= (1ull << 31)) {
            return fail(BGE_ERR_INVALID, "more overlapping body pairs than pair_capacity (%llu) holds: create the world with a larger pair_capacity",
                        (unsigned long long)cap);
        }
        w->isl_pair_cap = cap * 2; // (the pair search is repeated on the same boxes: nothing else of the sub-step has run yet)
    }
    const uint32_t n_pairs = counts_host[0];
    w->isl_last_pairs = n_pairs;
    w->isl_last_bodies = 0;
    const int cur = w->isl_cur, prev = cur ^ 1;
    if (n_pairs) {
        HIP_TRY(w->isl_keys[cur].ensure(static_cast<size_t>(n_pairs) * 8));
        HIP_TRY(w->isl_man[cur].ensure(static_cast<size_t>(n_pairs) * bge::kBoxManifoldWords * 4));
        size_t tmp_bytes = 0;
        HIP_TRY(bge::island_sort_keys(w->stream, nullptr, tmp_bytes, ip.keys_raw, w->isl_keys[cur].as<uint64_t>(), n_pairs));
        HIP_TRY(w->isl_sort_tmp.ensure(std::max<size_t>(tmp_bytes, 16)));
        HIP_TRY(bge::island_sort_keys(w->stream, w->isl_sort_tmp.p, tmp_bytes, ip.keys_raw, w->isl_keys[cur].as<uint64_t>(), n_pairs));
    }
    ip.keys = w->isl_keys[cur].as<uint64_t>();
    ip.man = w->isl_man[cur].as<uint32_t>();
    ip.n_pairs = n_pairs;
    ip.prev_keys = w->isl_keys[prev].as<uint64_t>();
    ip.prev_man = w->isl_man[prev].as<uint32_t>();
    ip.n_prev = w->isl_n_prev;
    const uint64_t body_cap = std::max<uint64_t>(n_slots, 1);
    HIP_TRY(w->isl_body_keys_raw.ensure(body_cap * 8));
    HIP_TRY(w->isl_body_slot_raw.ensure(body_cap * 4));
    ip.body_keys_raw = w->isl_body_keys_raw.as<uint64_t>();
    ip.body_slot_raw = w->isl_body_slot_raw.as<uint32_t>();
    ip.body_cap = static_cast<uint32_t>(body_cap);
    w->isl_cur = prev; // (this sub-step's list is the next one's "previous", also when the rest finds nothing to do)
    w->isl_n_prev = n_pairs;
    if (n_pairs == 0 && !later_sub_step) return BGE_OK;
    HIP_TRY(bge::launch_island_build(w->stream, w->view, ip, later_sub_step));
    HIP_TRY(hipMemcpyAsync(w->isl_counts_host.p, w->isl_counts.p, 16, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    const uint32_t n_bodies = counts_host[1];
    w->isl_last_bodies = n_bodies;
    if (n_bodies == 0) return BGE_OK;
    HIP_TRY(w->isl_body_keys.ensure(static_cast<size_t>(n_bodies) * 8));
    HIP_TRY(w->isl_body_slot.ensure(static_cast<size_t>(n_bodies) * 4));
    {
        size_t tmp_bytes = 0;
        HIP_TRY(bge::island_sort_pairs(w->stream, nullptr, tmp_bytes, ip.body_keys_raw, w->isl_body_keys.as<uint64_t>(), ip.body_slot_raw,
                                       w->isl_body_slot.as<uint32_t>(), n_bodies));
        HIP_TRY(w->isl_sort_tmp.ensure(std::max<size_t>(tmp_bytes, 16)));
        HIP_TRY(bge::island_sort_pairs(w->stream, w->isl_sort_tmp.p, tmp_bytes, ip.body_keys_raw, w->isl_body_keys.as<uint64_t>(), ip.body_slot_raw,
                                       w->isl_body_slot.as<uint32_t>(), n_bodies));
    }
    ip.body_keys = w->isl_body_keys.as<uint64_t>();
    ip.body_slot = w->isl_body_slot.as<uint32_t>();
    ip.n_bodies = n_bodies;
    // every point the manifolds can hold: 4 on the plane + 4 x 4 on obstacles per body (where those are on), 4 per pair; two rows a point
    const uint64_t own_points = (w->ground_plane ? 4ull : 0ull) + (w->static_contacts_ever ? 4ull * bge::kBoxManifolds : 0ull); // (a capacity: switching off ends every obstacle pair, so the rows are only needed while on)
    const uint64_t row_cap = 2ull * (own_points * n_bodies + 4ull * n_pairs) + 2;
    HIP_TRY(w->isl_solver_bodies.ensure(static_cast<size_t>(n_bodies) * bge::kIslBodyBytes));
    HIP_TRY(w->isl_rows.ensure(static_cast<size_t>(row_cap) * bge::kIslRowBytes + static_cast<size_t>(row_cap / 2 + 1) * bge::kIslRowColdBytes));
    ip.solver_bodies = w->isl_solver_bodies.p;
    ip.rows = w->isl_rows.p;
    ip.rows_cold = static_cast<char*>(w->isl_rows.p) + static_cast<size_t>(row_cap) * bge::kIslRowBytes;
    ip.row_cap = static_cast<uint32_t>(std::min<uint64_t>(row_cap, 0xffffffffu));
    // islands a workgroup solves level by level (k_island_solve_big): the list of them, two words per body, four per point for the levels
    const uint64_t int_cap = 2ull * row_cap + 8ull * n_bodies + 64;
    HIP_TRY(w->isl_big_list.ensure(static_cast<size_t>(n_bodies) * 16)); // (two lists: big islands, mid islands)
    HIP_TRY(w->isl_body_words.ensure(static_cast<size_t>(n_bodies) * 20 + 16)); // (two words a body for the workgroup solver, pair_first, row_count, row_first)
    const size_t scan_bytes = bge::island_scan_bytes(n_bodies);
    HIP_TRY(w->isl_sort_tmp.ensure(std::max<size_t>(scan_bytes, 16)));
    HIP_TRY(w->isl_ints.ensure(static_cast<size_t>(int_cap) * 4));
    ip.big_list = w->isl_big_list.as<uint32_t>();
    ip.mid_list = ip.big_list + 2ull * n_bodies;
    ip.body_words = w->isl_body_words.as<uint32_t>();
    ip.pair_first = ip.body_words + 2ull * n_bodies;
    ip.row_count = ip.pair_first + n_bodies;
    ip.row_first = ip.row_count + n_bodies;
    ip.scan_tmp = w->isl_sort_tmp.p;
    ip.scan_tmp_bytes = scan_bytes;
    ip.ints = w->isl_ints.as<uint32_t>();
    ip.int_cap = static_cast<uint32_t>(std::min<uint64_t>(int_cap, 0xffffffffu));
    ip.big_points = w->isl_big_points;
    ip.iterations = 10u;
    HIP_TRY(bge::launch_island_solve(w->stream, w->view, gp, ip, bullet_basis));
    return BGE_OK;
}

// sum the recorded event pairs into the carry (synchronises the stream)
int fold_profile(bge_world* w)
{
    HIP_TRY(hipStreamSynchronize(w->stream));
    for (size_t k = 0; k + 1 < w->prof_used; k += 2) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, w->prof_events[k], w->prof_events[k + 1]));
        w->prof_ms_carry += ms;
        w->prof_ticks_carry += (k / 2 < w->prof_ticks_pending.size()) ? w->prof_ticks_pending[k / 2] : 1u;
    }
    w->prof_used = 0;
    w->prof_ticks_pending.clear();
    return BGE_OK;
}
} // namespace

extern "C" {

int bge_world_gather_roots(bge_world* w, void** table_device);

const char* bge_last_error(void) { return g_last_error.c_str(); }
uint32_t bge_version(void) { return 0x00010000u; }

int bge_world_create(const bge_world_desc* desc, bge_world** out)
try {
    if (!out) return fail(BGE_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (desc && desc->struct_size != 0 && desc->struct_size < sizeof(bge_world_desc)) {
        return fail(BGE_ERR_INVALID, "bge_world_desc.struct_size %u < %zu", desc->struct_size, sizeof(bge_world_desc));
    }
    int ndev = 0;
    {
        const hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev <= 0) {
            return fail(BGE_ERR_HIP, "no usable HIP device (hipGetDeviceCount: %s, count %d) — this library has no CPU path",
                        hipGetErrorString(e), ndev);
        }
    }
    int device = desc ? desc->device : -1;
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    if (device >= ndev) return fail(BGE_ERR_INVALID, "device %d out of range (count %d)", device, ndev);

    bge_world* w = new (std::nothrow) bge_world();
    if (!w) return fail(BGE_ERR_OOM, "host allocation failed");
    w->device = device;
    if (const char* e = std::getenv("BGE_TRIGGER_GRID_MIN")) w->trigger_grid_min = static_cast<uint32_t>(std::strtoul(e, nullptr, 10));
    if (const char* e = std::getenv("BGE_TRIGGER_DEVICE_DIFF")) w->trig_device_diff = std::strtoul(e, nullptr, 10) != 0;
    if (const char* e = std::getenv("BGE_OBSTACLE_GRID")) w->obstacle_grid_on = std::strtoul(e, nullptr, 10) != 0;
    if (const char* e = std::getenv("BGE_QUERY_INDEX")) w->qi_desc.mode = std::strtoul(e, nullptr, 10) != 0 ? 1u : 0u;
    if (const char* e = std::getenv("BGE_QUERY_INDEX_MIN_WORK")) w->qi_desc.min_work = std::strtoull(e, nullptr, 10);
    DeviceGuard guard(device);
    if (desc && desc->stream) {
        w->stream = static_cast<hipStream_t>(desc->stream);
    } else {
        const hipError_t e = hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete w;
            return fail(BGE_ERR_HIP, "hipStreamCreateWithFlags failed: %s", hipGetErrorString(e));
        }
        w->own_stream = true;
    }
    w->pair_capacity_req = desc ? desc->pair_capacity : 0;
    *out = w;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_create")

void bge_world_destroy(bge_world* w)
{
    if (!w) return;
    DeviceGuard guard(w->device);
    (void)hipStreamSynchronize(w->stream);
    if (w->trig_fast_ticks && std::getenv("BGE_TRIGGER_PROFILE"))
        std::fprintf(stderr, "[bge] trigger diff on the device: %llu ticks, %.3f ms per tick until the deltas were on the host, %.3f ms applying %.0f of them\n",
                     (unsigned long long)w->trig_fast_ticks, w->trig_wait_ms / w->trig_fast_ticks, w->trig_apply_ms / w->trig_fast_ticks,
                     double(w->trig_deltas_seen) / w->trig_fast_ticks);
    const hipStream_t own = w->own_stream ? w->stream : nullptr;
    delete w; // frees every buffer, inside the guard
    if (own) (void)hipStreamDestroy(own);
}

// Character platform riding: the anchors on entities [first, first + count) are cleared, on the stream (bge_world_set_topology: all
// of them; bge_world_upload_bodies: an entity index that gets a new body carries nobody by the difference of two unrelated poses)
static int ride_forget(bge_world* w, uint64_t first, uint64_t count)
{
    if (!w->ride_on || w->n_characters == 0) return BGE_OK;
    HIP_TRY(bge::launch_char_ride_forget(w->stream, w->char_ride.p, static_cast<uint32_t>(w->n_characters), first, count));
    return BGE_OK;
}

int bge_world_set_topology(bge_world* w, uint64_t n, const uint32_t* parent, const uint8_t* has_transform)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (n >= 0xfffffff0ull) return fail(BGE_ERR_INVALID, "too many entities (%llu)", (unsigned long long)n);
    DeviceGuard guard(w->device);
    HIP_TRY(w->ensure_row3_current()); // (the carry below moves stored matrices to new slots, and the words are zeroed)

    // An entity that loses its Transform while its body exists keeps a slot for the body (kValid clear): the reference keeps
    // stepping that Bullet body (PhysicsSystem.cpp:389-393).  To the hierarchy it is an entity without a Transform: it is
    // nobody's effective parent and has none itself.
    std::vector<uint8_t> orphan(n, 0);
    bool any_orphan = false;
    if (w->has_topology && has_transform) {
        const uint64_t lim = std::min<uint64_t>(n, w->flat.n_entities);
        for (uint64_t i = 0; i < lim; ++i) {
            const bool was_orphan = i < w->orphan_host.size() && w->orphan_host[i];
            const bool created = was_orphan || (i < w->body_since.size() && w->physics_updates > w->body_since[i]);
            if (!has_transform[i] && w->flat.slot_of_entity[i] != bge::kNone && i < w->body_type_host.size() &&
                w->body_type_host[i] != BGE_BODY_NONE && created) {
                orphan[i] = 1;
                any_orphan = true;
            }
        }
    }
    // A trigger ghost whose entity loses its Transform stays in the world where it was last posed (EnsureTrigger returns before
    // it touches the ghost, PhysicsSystem.cpp:530-534): its box is fetched now, while the device arrays still describe it.
    if (w->has_topology && has_transform && !w->triggers.empty()) {
        for (size_t k = 0; k < w->triggers.size(); ++k) {
            bge_world::Trigger& t = w->triggers[k];
            const bool keeps_transform = t.entity < n && has_transform[t.entity];
            if (keeps_transform || t.frozen || !t.runtime_active) continue;
            if (t.posed && w->trig_list_on_device && w->trig_aabb.p) {
                HIP_TRY(hipStreamSynchronize(w->stream));
                HIP_TRY(hipMemcpy(t.frozen_aabb, static_cast<const char*>(w->trig_aabb.p) + 24 * k, 24, hipMemcpyDeviceToHost));
                if (w->trig_pose.p) HIP_TRY(hipMemcpy(t.frozen_pose, static_cast<const char*>(w->trig_pose.p) + 32 * k, 32, hipMemcpyDeviceToHost));
                t.frozen = true;
            } else {
                t.runtime_active = false; // (never posed: there is no ghost to keep)
                t.clear_overlaps();
            }
        }
    }
    std::vector<uint32_t> parent_flat;
    std::vector<uint8_t> tf_flat;
    if (any_orphan) {
        parent_flat.assign(n, bge::kNone);
        tf_flat.assign(n, 0);
        for (uint64_t i = 0; i < n; ++i) {
            tf_flat[i] = (has_transform[i] || orphan[i]) ? 1 : 0;
            const uint32_t p = parent ? parent[i] : bge::kNone;
            if (!orphan[i] && p != bge::kNone && p < n && !orphan[p]) parent_flat[i] = p;
        }
    }
    bge::Flattened nf;
    try {
        bge::flatten_topology(n, any_orphan ? parent_flat.data() : parent, any_orphan ? tf_flat.data() : has_transform, nf);
    } catch (const std::bad_alloc&) {
        return fail(BGE_ERR_OOM, "host allocation failed while flattening %llu entities", (unsigned long long)n);
    }
    if (any_orphan) {
        for (uint64_t i = 0; i < n; ++i) {
            if (orphan[i]) nf.flags[nf.slot_of_entity[i]] &= ~bge::kValid;
        }
    }

    // ---- carry component state of surviving entity indices over to the new layout
    const bool carry = w->has_topology && w->flat.n_slots > 0;
    const uint64_t n_keep = carry ? std::min<uint64_t>(n, w->flat.n_entities) : 0;
    struct Carry {
        SlotBuf* buf;
        DevBuf tmp;
    };
    std::vector<Carry> carries;
    DevBuf old_flags_tmp;
    if (n_keep) {
        for (SlotBuf* a : w->carried) {
            if (a->p) carries.push_back(Carry{a, DevBuf{}}); // (an optional store that was never made has nothing to carry)
        }
        for (Carry& c : carries) {
            HIP_TRY(c.tmp.ensure(c.buf->bytes_for(n_keep)));
            HIP_TRY(bge::launch_gather_rows(w->stream, w->slot_of_entity.as<uint32_t>(), 0, n_keep, c.buf->words, c.buf->p, c.tmp.p, nullptr,
                                            c.buf->vel_blocks));
        }
        HIP_TRY(old_flags_tmp.ensure(n_keep * 4));
        HIP_TRY(bge::launch_gather_rows(w->stream, w->slot_of_entity.as<uint32_t>(), 0, n_keep, 1, w->flags.p, old_flags_tmp.p));
        HIP_TRY(hipStreamSynchronize(w->stream));
    }
    std::vector<uint32_t> old_flags(n_keep);
    if (n_keep) HIP_TRY(hipMemcpy(old_flags.data(), old_flags_tmp.p, n_keep * 4, hipMemcpyDeviceToHost));
    // roots that still keep their stored world matrix (the kernel clears a bit when its root turns dirty), per entity
    std::vector<uint8_t> was_frozen(n_keep, 0);
    if (n_keep && w->any_frozen) {
        std::vector<uint32_t> bits((w->flat.n_slots + 31) / 32);
        HIP_TRY(hipMemcpy(bits.data(), w->frozen.p, bits.size() * 4, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n_keep; ++i) {
            const uint32_t s = w->flat.slot_of_entity[i];
            if (s != bge::kNone && ((bits[s >> 5] >> (s & 31u)) & 1u)) was_frozen[i] = 1;
        }
    }

    // ---- which surviving transforms became dirty through the hierarchy.  Scene::SetParent (Scene.cpp:354-393) works on
    // ENTITIES: a changed parent — whether or not either parent owns a Transform — ends in MarkHierarchyDirty(child), which walks
    // the children lists (through Transform-less entities too) and marks every Transform on the way (Scene.cpp:535-550).  A
    // Transform that merely gained or lost an effective parent because that parent's Transform came or went is NOT marked.
    std::vector<uint8_t> keep_mask(n_keep, 0); // 1 = carried over, 2 = carried over but hierarchy-dirty
    std::vector<uint32_t> raw_new(n, bge::kNone);
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t p = parent ? parent[i] : bge::kNone;
        if (p != bge::kNone && p < n) raw_new[i] = p; // (SetParent ignores a parent that is not alive)
    }
    if (n_keep) {
        std::vector<uint32_t> order; // BFS over the new entity forest so that dirtiness flows parent -> child
        order.reserve(n);
        std::vector<uint32_t> child_begin(n + 1, 0), child_list;
        for (uint64_t i = 0; i < n; ++i) {
            if (raw_new[i] != bge::kNone) child_begin[raw_new[i] + 1]++;
        }
        for (uint64_t i = 0; i < n; ++i) child_begin[i + 1] += child_begin[i];
        child_list.resize(child_begin[n]);
        {
            std::vector<uint32_t> cur(child_begin.begin(), child_begin.end() - 1);
            for (uint64_t i = 0; i < n; ++i) {
                if (raw_new[i] != bge::kNone) child_list[cur[raw_new[i]]++] = static_cast<uint32_t>(i);
            }
        }
        std::vector<uint8_t> hdirty(n, 0);
        for (uint64_t i = 0; i < n; ++i) {
            if (raw_new[i] == bge::kNone) order.push_back(static_cast<uint32_t>(i));
        }
        for (size_t h = 0; h < order.size(); ++h) { // (entities inside a parent cycle are never reached: nothing marks them)
            const uint32_t u = order[h];
            bool d = u >= w->parent_entity.size() || w->parent_entity[u] != raw_new[u];
            if (raw_new[u] != bge::kNone && hdirty[raw_new[u]]) d = true;
            hdirty[u] = d ? 1 : 0;
            for (uint32_t c = child_begin[u]; c < child_begin[u + 1]; ++c) order.push_back(child_list[c]);
        }
        for (uint64_t i = 0; i < n_keep; ++i) {
            if (nf.slot_of_entity[i] == bge::kNone || w->flat.slot_of_entity[i] == bge::kNone) continue;
            keep_mask[i] = hdirty[i] ? 2 : 1;
        }
    }
    // A clean Transform whose parent ENTITY stays but no longer owns a Transform becomes a root without being marked dirty:
    // TransformSystem::Update will not recompute it (UpdateNode recomputes a node only when it or an ancestor is dirty,
    // TransformSystem.cpp:18-40), so its world matrix stays parent * local until something dirties it.  Such roots — and the
    // ones that were already in that state and still have no Transform above them — are listed for the kernel.
    std::vector<uint32_t> frozen_bits;
    bool any_frozen = false;
    for (uint64_t i = 0; i < n_keep; ++i) {
        if (keep_mask[i] != 1 || (old_flags[i] & bge::kTDirty)) continue;
        if (orphan[i]) continue;                    // (a body without a Transform has no world matrix to keep)
        const uint32_t p = raw_new[i];
        const bool parent_owns_transform = p != bge::kNone && nf.slot_of_entity[p] != bge::kNone && !orphan[p];
        if (p == bge::kNone || parent_owns_transform) continue; // no parent entity, or it owns a Transform (again)
        const bool parent_had_transform = p < w->flat.n_entities && w->flat.slot_of_entity[p] != bge::kNone &&
                                          !(p < w->orphan_host.size() && w->orphan_host[p]);
        if (!parent_had_transform && !was_frozen[i]) continue;
        if (frozen_bits.empty()) frozen_bits.assign((std::max<uint64_t>(nf.n_slots, bge::kTile) + 31) / 32, 0u);
        const uint32_t sl = nf.slot_of_entity[i];
        frozen_bits[sl >> 5] |= 1u << (sl & 31u);
        nf.tile_hdr[sl / bge::kTile] |= bge::kHdrFrozen;
        any_frozen = true;
    }
    w->parent_entity.swap(raw_new);

    // ---- (re)allocate for the new layout
    const uint64_t S = std::max<uint64_t>(nf.n_slots, bge::kTile);
    const uint64_t T = std::max<uint32_t>(nf.n_tiles_total, 1);
    HIP_TRY(w->flags.ensure(S * 4));
    HIP_TRY(w->parent.ensure(S * 4));
    HIP_TRY(w->tile_hdr.ensure(T * 4));
    HIP_TRY(w->rs_word.ensure(T * 64));
    HIP_TRY(hipMemsetAsync(w->rs_word.p, 0, T * 64, w->stream));
    HIP_TRY(w->adv.ensure(T * 16));
    HIP_TRY(hipMemsetAsync(w->adv.p, 0, T * 16, w->stream));
    w->epochs_edit();
    HIP_TRY(w->slot_of_entity.ensure(std::max<uint64_t>(n, 1) * 4));
    HIP_TRY(w->entity_of_slot.ensure(S * 4));
    HIP_TRY(w->root_index.ensure(S * 4));
    HIP_TRY(w->root_slots.ensure(std::max<size_t>(nf.root_slots.size(), 1) * 4));
    for (SlotBuf* a : w->carried) { // (k_init_slots writes the defaults, the carry below the surviving values)
        if (a == &w->half_extent) HIP_TRY(w->filter_table.ensure(256 * 16)); // (its place in the order of first allocations)
        if (!a->wanted()) continue;
        HIP_TRY(a->ensure(a->bytes_for(S)));
        if (a->fill != SlotBuf::kNoFill) HIP_TRY(hipMemsetAsync(a->p, a->fill, a->bytes, w->stream));
    }
    w->obstacles_stale = true; // slots moved
    HIP_TRY(w->root_worlds.ensure(std::max<size_t>(nf.root_slots.size(), 1) * 64));
    HIP_TRY(w->counter.ensure(64));
    HIP_TRY(w->mass_palette.ensure(256 * sizeof(float2)));
    HIP_TRY(w->grav_palette.ensure(256 * sizeof(float4)));
    w->grav_palette_stale = true;
    w->rebuild_view();

    if (nf.n_slots) {
        HIP_TRY(hipMemcpyAsync(w->parent.p, nf.parent_field.data(), nf.n_slots * 4, hipMemcpyHostToDevice, w->stream));
        HIP_TRY(hipMemcpyAsync(w->entity_of_slot.p, nf.entity_of_slot.data(), nf.n_slots * 4, hipMemcpyHostToDevice, w->stream));
        HIP_TRY(hipMemcpyAsync(w->tile_hdr.p, nf.tile_hdr.data(), static_cast<size_t>(nf.n_tiles_total) * 4,
                               hipMemcpyHostToDevice, w->stream));
        // structural flags travel through the staging buffer, k_init_slots merges them
        HIP_TRY(w->stage.ensure(nf.n_slots * 4));
        HIP_TRY(hipMemcpyAsync(w->stage.p, nf.flags.data(), nf.n_slots * 4, hipMemcpyHostToDevice, w->stream));
        HIP_TRY(bge::launch_init_slots(w->stream, nf.n_slots, w->stage.as<uint32_t>(), w->view));
    }
    if (n) HIP_TRY(hipMemcpyAsync(w->slot_of_entity.p, nf.slot_of_entity.data(), n * 4, hipMemcpyHostToDevice, w->stream));
    std::vector<uint32_t> root_index_host;
    if (!nf.root_slots.empty()) {
        HIP_TRY(hipMemcpyAsync(w->root_slots.p, nf.root_slots.data(), nf.root_slots.size() * 4, hipMemcpyHostToDevice, w->stream));
        root_index_host.assign(nf.n_slots, 0);
        for (size_t k = 0; k < nf.root_slots.size(); ++k) root_index_host[nf.root_slots[k]] = static_cast<uint32_t>(k);
        HIP_TRY(hipMemcpyAsync(w->root_index.p, root_index_host.data(), nf.n_slots * 4, hipMemcpyHostToDevice, w->stream));
    }
    HIP_TRY(hipStreamSynchronize(w->stream));

    if (n_keep) {
        // entities that lost or gained their Transform restart from defaults: route them to "no slot"
        std::vector<uint32_t> carry_map(n_keep, bge::kNone);
        for (uint64_t i = 0; i < n_keep; ++i) {
            if (keep_mask[i]) carry_map[i] = nf.slot_of_entity[i];
        }
        DevBuf map_dev;
        HIP_TRY(map_dev.ensure(n_keep * 4));
        HIP_TRY(hipMemcpyAsync(map_dev.p, carry_map.data(), n_keep * 4, hipMemcpyHostToDevice, w->stream));
        for (Carry& c : carries) {
            HIP_TRY(bge::launch_scatter_rows(w->stream, map_dev.as<uint32_t>(), 0, n_keep, c.buf->words, c.tmp.p, c.buf->p, nullptr, 0, nullptr, 0,
                                             c.buf->vel_blocks));
        }
        // flags: keep body type / dirty / spin / shape bits of the old word, structure from the new one
        std::vector<uint32_t> merged(nf.flags);
        const uint32_t keep_bits = bge::kTypeMask | bge::kTDirty | bge::kBDirty | bge::kSpin | bge::kMassMask | bge::kDrowsy;
        for (uint64_t s = 0; s < nf.n_slots; ++s) {
            if (merged[s] & bge::kValid) merged[s] |= bge::kTDirty;
        }
        for (uint64_t i = 0; i < n_keep; ++i) {
            if (!keep_mask[i]) continue;
            const uint32_t s = nf.slot_of_entity[i];
            uint32_t f = (nf.flags[s] & ~keep_bits) | (old_flags[i] & keep_bits);
            if (keep_mask[i] == 2) f |= bge::kTDirty;
            if (orphan[i]) f &= ~(bge::kValid | bge::kTDirty); // the body's slot: no Transform here, nothing to be dirty
            merged[s] = f;
        }
        HIP_TRY(hipMemcpyAsync(w->flags.p, merged.data(), nf.n_slots * 4, hipMemcpyHostToDevice, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream));
        for (Carry& c : carries) c.tmp.release();
        old_flags_tmp.release();
        map_dev.release();
    }

    if (any_frozen) {
        HIP_TRY(w->frozen.ensure(frozen_bits.size() * 4));
        HIP_TRY(hipMemcpy(w->frozen.p, frozen_bits.data(), frozen_bits.size() * 4, hipMemcpyHostToDevice));
        w->rebuild_view();
    }
    if (int rc = w->bounds.follow_topology(n, w->flat.n_entities, w->stream)) return rc;
    if (int rc = w->draw_keys.follow_topology(n, w->flat.n_entities, w->stream)) return rc;
    w->any_frozen = any_frozen;
    w->flat = std::move(nf);
    w->refresh_shape();
    w->orphan_host.swap(orphan);
    w->body_type_host.resize(n, BGE_BODY_NONE); // surviving indices keep their body, new ones have none
    for (uint64_t i = 0; i < n; ++i) {
        if (w->flat.slot_of_entity[i] == bge::kNone) w->body_type_host[i] = BGE_BODY_NONE; // no Transform, no body
    }
    w->has_topology = true;
    w->maybe_dirty = true;
    w->triggers_device_stale = true; // slots moved
    w->global_of_slot_stale = true;
    w->pairs_from_slab = false;
    return ride_forget(w, 0, ~0ull); // (slots moved and entity indices may mean other entities: nobody rides across this)
}
BGE_CATCH_ALL("bge_world_set_topology")

static int upload_trs(bge_world* w, const Entities& e, const float* pos3, const float* euler3, const float* scale3)
{
    return with_entities(
        w, e, [&] { return e.count ? BGE_OK : kNothingToDo; },
        [&](const uint32_t* di) -> int {
            // (Transform::world keeps the old translation until the next TransformSystem::Update: stored before pos is overwritten)
            HIP_TRY(w->ensure_row3_current());
            for (auto [host, dst] : {std::pair{pos3, &w->pos}, {euler3, &w->euler}, {scale3, &w->scale}}) {
                if (!host) continue;
                if (int rc = upload_rows(w, e.first, e.count, host, *dst, 0, di, bge::kValid)) return rc;
            }
            HIP_TRY(bge::launch_scatter_rows(w->stream, w->slot_of_entity.as<uint32_t>(), e.first, e.count, 0, nullptr, nullptr,
                                             w->flags.as<uint32_t>(), bge::kTDirty, di, bge::kValid));
            HIP_TRY(hipStreamSynchronize(w->stream));
            w->maybe_dirty = true;
            w->epochs_edit();
            return BGE_OK;
        });
}

int bge_world_upload_trs(bge_world* w, uint64_t first, uint64_t count, const float* pos3, const float* euler3,
                         const float* scale3)
try {
    return upload_trs(w, Entities::range(first, count), pos3, euler3, scale3);
}
BGE_CATCH_ALL("bge_world_upload_trs")

int bge_world_upload_trs_indexed(bge_world* w, uint64_t count, const uint32_t* entity_index, const float* pos3,
                                 const float* euler3, const float* scale3)
try {
    return upload_trs(w, Entities::list(count, entity_index), pos3, euler3, scale3);
}
BGE_CATCH_ALL("bge_world_upload_trs_indexed")

int bge_world_mark_dirty(bge_world* w, uint64_t first, uint64_t count)
try {
    if (int rc = check_range(w, first, count)) return rc;
    if (count == 0) return BGE_OK;
    DeviceGuard guard(w->device);
    HIP_TRY(bge::launch_scatter_rows(w->stream, w->slot_of_entity.as<uint32_t>(), first, count, 0, nullptr, nullptr,
                                     w->flags.as<uint32_t>(), bge::kTDirty, nullptr, bge::kValid));
    w->maybe_dirty = true;
    w->epochs_edit();
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_mark_dirty")

// (the body of bge_world_upload_bodies / _indexed once with_entities has staged the list: di)
static int upload_bodies(bge_world* w, uint64_t first, uint64_t count, const uint32_t* index, const uint32_t* di, const uint8_t* type,
                         const float* mass, const uint8_t* shape, const float* size3, const uint32_t* layer, const uint32_t* mask)
{
    // host: component values -> device parameters (PhysicsSystem.cpp:398-477, 686-707)
    bool palette_changed = w->palette_inv_mass.empty();
    if (palette_changed) {
        w->palette_inv_mass.push_back(0.0f);
        w->palette_class[0u] = 0;
    }
    std::vector<uint32_t> words(count * 13);
    float* cdims = reinterpret_cast<float*>(words.data() + 8 * count); // collider as Bullet holds it (ground contact)
    float* cmass = reinterpret_cast<float*>(words.data() + 11 * count);
    uint32_t* cbits = words.data() + 12 * count;
    uint32_t* type_bits = words.data();
    float* inv_mass = reinterpret_cast<float*>(words.data() + count);
    float* he = reinterpret_cast<float*>(words.data() + 2 * count);
    uint32_t* group = words.data() + 5 * count;
    uint32_t* msk = words.data() + 6 * count;
    uint32_t* fclass = words.data() + 7 * count;
    for (uint64_t i = 0; i < count; ++i) {
        const uint8_t t = type[i];
        if (t != BGE_BODY_NONE && t > BGE_BODY_KINEMATIC) return fail(BGE_ERR_INVALID, "type[%llu] = %u", (unsigned long long)i, t);
        const uint8_t sh = shape ? shape[i] : BGE_SHAPE_BOX;
        const float default_size[3] = {0.5f, 0.5f, 0.5f};
        const float* sz = size3 ? size3 + 3 * i : default_size;
        if (t == BGE_BODY_NONE) {
            type_bits[i] = 0;
            inv_mass[i] = 0.0f;
        } else {
            float m = 0.0f;
            if (t == BGE_BODY_DYNAMIC) m = std::max(mass ? mass[i] : 1.0f, 0.01f);
            inv_mass[i] = m != 0.0f ? 1.0f / m : 0.0f;
            type_bits[i] = (static_cast<uint32_t>(t) + 1u) | bge::kBDirty | (mass_class(w, inv_mass[i], palette_changed) << bge::kMassShift);
        }
        {
            const uint64_t e = index ? index[i] : first + i;
            const bool orphan = e < w->orphan_host.size() && w->orphan_host[e];
            if (e < w->body_type_host.size() && !(orphan && t != BGE_BODY_NONE)) {
                const uint8_t now = w->flat.slot_of_entity[e] == bge::kNone ? BGE_BODY_NONE : t;
                if (w->body_type_host[e] == BGE_BODY_NONE && now != BGE_BODY_NONE) {
                    if (w->body_since.size() < w->body_type_host.size()) w->body_since.resize(w->body_type_host.size(), 0);
                    w->body_since[e] = w->physics_updates; // not in the reference's world before the next update
                }
                w->body_type_host[e] = now;
                if (w->body_shape_host.size() < w->body_type_host.size()) w->body_shape_host.resize(w->body_type_host.size(), BGE_SHAPE_BOX);
                if (w->body_gen_host.size() < w->body_type_host.size()) w->body_gen_host.resize(w->body_type_host.size(), 0u);
                w->body_shape_host[e] = sh;
                w->body_gen_host[e] += 1u; // EnsureRigidBody re-creates the btRigidBody: its pairs and their manifolds are gone
                w->isl_gen_stale = true;
                w->obstacles_stale = true;
            }
        }
        collider_half_extents(sh, sz, he + 3 * i);
        const uint32_t l = layer ? layer[i] : 1u;
        group[i] = l ? l : 1u;
        msk[i] = mask ? mask[i] : 0xffffffffu;
        if (sh == BGE_SHAPE_CAPSULE) {
            // btCapsuleShape(radius, 2 * halfHeight): m_implicitShapeDimensions = (radius, 0.5 * height, radius)
            cdims[3 * i] = std::max(sz[0], 0.01f);
            cdims[3 * i + 1] = 0.5f * (std::max(sz[1], 0.0f) * 2.0f);
            cdims[3 * i + 2] = cdims[3 * i];
        } else {
            std::memcpy(cdims + 3 * i, he + 3 * i, 12); // btBoxShape::getHalfExtentsWithMargin() is what the AABB uses too
        }
        cmass[i] = t == BGE_BODY_DYNAMIC ? std::max(mass ? mass[i] : 1.0f, 0.01f) : 0.0f;
        // the ground is in group StaticFilter (2) with mask AllFilter: it reaches the bodies whose mask has bit 1
        cbits[i] = (sh == BGE_SHAPE_CAPSULE ? bge::kCiCapsule : 0u) | ((msk[i] & 2u) ? bge::kCiGroundMask : 0u);
        fclass[i] = t == BGE_BODY_NONE ? 0u : w->filter_class_of(group[i], msk[i], t == BGE_BODY_STATIC);
    }
    if (palette_changed) {
        std::vector<float2> pal(256, float2{0.0f, 0.0f});
        for (size_t k = 0; k < w->palette_inv_mass.size(); ++k) {
            const float im = w->palette_inv_mass[k];
            pal[k] = float2{im, im != 0.0f ? 1.0f / im : 0.0f}; // same IEEE divide the kernel's fallback path performs
        }
        w->grav_palette_stale = true;
        HIP_TRY(hipMemcpyAsync(w->mass_palette.p, pal.data(), pal.size() * sizeof(float2), hipMemcpyHostToDevice, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream));
    }
    {
        // tile headers: "every valid slot carries a Dynamic body" lets the tick kernel load velocities without waiting for flags
        std::vector<uint32_t> dyn_in_tile(w->flat.n_tiles_total, 0);
        for (uint64_t e = 0; e < w->flat.n_entities; ++e) {
            const uint32_t sl = w->flat.slot_of_entity[e];
            if (sl != bge::kNone && w->body_type_host[e] == BGE_BODY_DYNAMIC) dyn_in_tile[sl / bge::kTile]++;
        }
        bool changed = false;
        for (uint32_t t = 0; t < w->flat.n_tiles_total; ++t) {
            const uint32_t count = (w->flat.tile_hdr[t] >> bge::kHdrCountShift) & bge::kHdrCountMask;
            const uint32_t want = (count != 0 && dyn_in_tile[t] == count) ? bge::kHdrAllDynamic : 0u;
            if ((w->flat.tile_hdr[t] & bge::kHdrAllDynamic) != want) {
                w->flat.tile_hdr[t] = (w->flat.tile_hdr[t] & ~bge::kHdrAllDynamic) | want;
                changed = true;
            }
        }
        if (changed) {
            w->refresh_shape();
            HIP_TRY(hipStreamSynchronize(w->stream));
            HIP_TRY(hipMemcpy(w->tile_hdr.p, w->flat.tile_hdr.data(), static_cast<size_t>(w->flat.n_tiles_total) * 4, hipMemcpyHostToDevice));
        }
    }
    if (w->ride_on) {
        // character platform riding: nobody keeps an anchor on an entity whose body is replaced.  The indexed form forgets run by
        // run of consecutive indices; a list of more than kRuns runs is taken as its span.
        constexpr size_t kRuns = 16;
        std::vector<std::pair<uint64_t, uint64_t>> runs; // first, count
        if (!index) {
            runs.emplace_back(first, count);
        } else {
            std::vector<uint32_t> sorted(index, index + count);
            std::sort(sorted.begin(), sorted.end());
            for (uint32_t e : sorted) {
                if (!runs.empty() && e < runs.back().first + runs.back().second) continue; // (listed twice)
                if (!runs.empty() && e == runs.back().first + runs.back().second) runs.back().second += 1;
                else runs.emplace_back(e, 1);
            }
            if (runs.size() > kRuns) runs.assign(1, {sorted.front(), uint64_t(sorted.back()) - sorted.front() + 1u});
        }
        for (const auto& run : runs) {
            if (int rc = ride_forget(w, run.first, run.second)) return rc;
        }
    }
    const size_t bytes = words.size() * 4;
    HIP_TRY(w->stage.ensure(bytes));
    HIP_TRY(hipMemcpyAsync(w->stage.p, words.data(), bytes, hipMemcpyHostToDevice, w->stream));
    const uint32_t* d = w->stage.as<uint32_t>();
    HIP_TRY(bge::launch_scatter_bodies(w->stream, w->slot_of_entity.as<uint32_t>(), first, count, d,
                                       reinterpret_cast<const float*>(d + count), reinterpret_cast<const float*>(d + 2 * count),
                                       d + 5 * count, d + 6 * count, d + 7 * count, w->view, di,
                                       reinterpret_cast<const float*>(d + 8 * count), reinterpret_cast<const float*>(d + 11 * count),
                                       d + 12 * count));
    HIP_TRY(hipStreamSynchronize(w->stream));
    w->maybe_dirty = true;
    w->epochs_edit();
    return BGE_OK;
}

static int upload_bodies(bge_world* w, const Entities& e, const uint8_t* type, const float* mass, const uint8_t* shape, const float* size3,
                         const uint32_t* layer, const uint32_t* mask)
{
    return with_entities(
        w, e,
        [&]() -> int {
            if (!type) return fail(BGE_ERR_INVALID, "type is NULL");
            return e.count ? BGE_OK : kNothingToDo;
        },
        [&](const uint32_t* di) -> int { return upload_bodies(w, e.first, e.count, e.index, di, type, mass, shape, size3, layer, mask); });
}

int bge_world_upload_bodies(bge_world* w, uint64_t first, uint64_t count, const uint8_t* type, const float* mass,
                            const uint8_t* shape, const float* size3, const uint32_t* layer, const uint32_t* mask)
try {
    return upload_bodies(w, Entities::range(first, count), type, mass, shape, size3, layer, mask);
}
BGE_CATCH_ALL("bge_world_upload_bodies")

int bge_world_upload_bodies_indexed(bge_world* w, uint64_t count, const uint32_t* entity_index, const uint8_t* type,
                                    const float* mass, const uint8_t* shape, const float* size3, const uint32_t* layer,
                                    const uint32_t* mask)
try {
    return upload_bodies(w, Entities::list(count, entity_index), type, mass, shape, size3, layer, mask);
}
BGE_CATCH_ALL("bge_world_upload_bodies_indexed")

int bge_world_set_velocities(bge_world* w, uint64_t first, uint64_t count, const float* linvel3, const float* angvel3)
try {
    if (int rc = check_range(w, first, count)) return rc;
    if (count == 0 || (!linvel3 && !angvel3)) return BGE_OK;
    DeviceGuard guard(w->device);
    const size_t rows = static_cast<size_t>(count) * 12;
    HIP_TRY(w->stage.ensure(rows * 2));
    float* dl = w->stage.as<float>();
    float* da = reinterpret_cast<float*>(static_cast<char*>(w->stage.p) + rows);
    if (linvel3) HIP_TRY(hipMemcpyAsync(dl, linvel3, rows, hipMemcpyHostToDevice, w->stream));
    if (angvel3) HIP_TRY(hipMemcpyAsync(da, angvel3, rows, hipMemcpyHostToDevice, w->stream));
    HIP_TRY(bge::launch_scatter_velocities(w->stream, w->slot_of_entity.as<uint32_t>(), first, count, linvel3 ? dl : nullptr,
                                           angvel3 ? da : nullptr, w->view));
    HIP_TRY(hipStreamSynchronize(w->stream));
    w->epochs_edit();
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_set_velocities")

namespace {
// How one enqueued tick relates to PhysicsSystem::Update's stepSimulation call (bge_world_step_simulation):
struct SubStep {
    bool no_repose = false;    // a later sub-step of the same call: the teleport rule ran before the first one
    bool ghosts_posed = false; // the trigger ghosts were posed (and their activation rule applied) before the first sub-step
};
int tick_impl(bge_world* w, uint32_t ticks, float dt, const float gravity[3], uint32_t flags, SubStep sub);
uint64_t ticked_slots(const bge_world* w) { return static_cast<uint64_t>(w->flat.n_tiles_ticked) * bge::kTile; }
} // namespace

int bge_world_tick_many(bge_world* w, uint32_t ticks, float dt, const float gravity[3], uint32_t flags)
try {
    return tick_impl(w, ticks, dt, gravity, flags, SubStep{});
}
BGE_CATCH_ALL("bge_world_tick_many")

namespace {
// The sub-step's contacts (ground plane, obstacles, Dynamic pairs).  Bullet's order inside PhysicsSystem::Update: teleport dirty
// bodies (before stepSimulation), then per sub-step collision detection + solver, then integrateTransforms — so k_ground_select
// re-poses them (once per stepSimulation call) and picks the bodies at the ground, k_ground collides and solves those, and the
// tick kernel integrates.
int contact_substep(bge_world* w, bge::TickParams& p, float dt, const float gravity[3], uint32_t flags, SubStep sub)
{
    const uint64_t n_slots = ticked_slots(w);
    // the solver's work list: slots + its count and ticket words (left at zero by every k_ground)
    const uint64_t shard_cap = bge::ground_shard_cap(n_slots);
    const size_t list_bytes = shard_cap * bge::kGroundShards * 4, count_bytes = (bge::kGroundShards + 1) * 64;
    if (w->ground_list.bytes < list_bytes || !w->ground_count.p) {
        HIP_TRY(w->ground_list.ensure(list_bytes));
        HIP_TRY(w->ground_count.ensure(count_bytes));
        HIP_TRY(hipMemsetAsync(w->ground_count.p, 0, count_bytes, w->stream));
    }
    bge::GroundParams gp{};
    gp.repose = sub.no_repose ? 0u : 1u; // (the teleport rule is part of k_ground_select)
    gp.list = w->ground_list.as<uint32_t>();
    gp.list_count = w->ground_count.as<uint32_t>();
    gp.shard_cap = shard_cap;
    gp.dt = dt;
    gp.gx = gravity[0];
    gp.gy = gravity[1];
    gp.gz = gravity[2];
    gp.n_slots = n_slots;
    gp.want_aabb = (flags & (BGE_TICK_BROADPHASE | BGE_TICK_AABBS)) ? 1u : 0u;
    gp.plane = w->ground_plane ? 1u : 0u;
    if (w->static_contacts) {
        if (int rc = prepare_obstacles(w, n_slots)) return rc;
        gp.obstacle_slots = w->obstacle_slots.as<uint32_t>();
        gp.obstacle_gen = w->obstacle_gen.as<uint32_t>();
        gp.obstacles = w->obstacles.as<bge::ObstacleRec>();
        gp.n_obstacles = w->n_obstacles;
        if (w->obstacle_grid_on && w->n_obstacles > bge::kObstacleGridMin) {
            gp.obstacle_grid = w->obstacle_grid.as<uint32_t>();
            gp.obstacle_grid_cap = 64u * w->n_obstacles;
        }
        gp.entity_of_slot = w->entity_of_slot.as<uint32_t>();
        gp.box_list = w->box_list.as<uint32_t>();
        gp.box_count = w->box_count.as<uint32_t>();
    }
    if (w->dynamic_contacts) {
        if (int rc = island_substep(w, gp, n_slots, (flags & BGE_TICK_BULLET_BASIS) != 0, sub.no_repose != 0, (flags & BGE_TICK_BROADPHASE) != 0)) return rc;
    }
    HIP_TRY(bge::launch_ground(w->stream, w->view, gp, (flags & BGE_TICK_BULLET_BASIS) != 0));
    p.no_repose = 1u;
    p.cinfo_in = w->cinfo.as<uint32_t>();
    return BGE_OK;
}

// The trigger ghosts' boxes from the Transforms as they are before the step
int pose_ghosts(bge_world* w)
{
    ensure_triggers(w);
    if (w->triggers_device_stale) {
        if (int rc = sync_triggers_to_device(w)) return rc;
    }
    HIP_TRY(bge::launch_trigger_aabb(w->stream, static_cast<uint32_t>(w->triggers.size()), w->trigger_view(), w->view));
    for (bge_world::Trigger& tg : w->triggers) tg.posed = tg.posed || (tg.runtime_active && !tg.frozen);
    return BGE_OK;
}

// Is a one-shot volume in the world?
bool any_one_shot(const bge_world* w)
{
    for (const bge_world::Trigger& t : w->triggers) {
        if (t.one_shot && t.runtime_active) return true;
    }
    return false;
}

// The tick's broadphase after the tick kernel, and the trigger volumes' overlaps with the new boxes
int broadphase_and_triggers(bge_world* w, bool with_triggers)
{
    // buffers are sized on first use: a world that never asks for pairs does not pay for them
    const uint64_t cap = w->pair_capacity_req ? w->pair_capacity_req : std::max<uint64_t>(8 * w->flat.n_entities, 4096);
    int rc = BGE_OK;
    if (!(w->dynamic_contacts && w->bp_shared)) rc = w->broadphase.configure(std::max<uint64_t>(w->flat.n_slots, bge::kTile), cap);
    if (rc != BGE_OK) return fail(rc, "broadphase allocation failed: %s", w->broadphase.error());
    bge::FilterPalette palette{};
    if (int prc = filter_palette_of(w, &palette)) return prc;
    if (!(w->dynamic_contacts && w->bp_shared)) { // (else: island_substep ran it on these very boxes)
        rc = w->broadphase.run(w->stream, w->view, ticked_slots(w), w->entity_of_slot.as<uint32_t>(), nullptr, &palette, w->bp_partials.as<float4>());
        if (rc != BGE_OK) return fail(rc, "broadphase failed: %s", w->broadphase.error());
    }
    w->bp_shared = false;
    w->pairs_from_slab = false;
    if (with_triggers) {
        // counters: [0] overlaps found, [1] ghosts left to the all-bodies pass, [2] ghosts walked through the grid
        HIP_TRY(hipMemsetAsync(w->trig_count.p, 0, 12, w->stream));
        const uint32_t n_trig = static_cast<uint32_t>(w->triggers.size());
        const uint32_t* big_list = nullptr;
        if (n_trig > w->trigger_grid_min) {
            // many ghosts: the ones that cover few cells look their bodies up in the broadphase's sorted grid
            // (n_bodies x n_triggers box tests otherwise: 4 M bodies x 1000 ghosts = 4 G tests a tick)
            HIP_TRY(w->trig_lists.ensure(static_cast<size_t>(n_trig) * 8));
            const bge::TriggerView tv = w->trigger_view();
            const bge::BoxQuery q{n_trig, tv.aabb, tv.group, tv.mask, tv.entity, w->trig_count.as<uint32_t>(),
                                  w->trig_lists.as<uint32_t>(), w->trig_lists.as<uint32_t>() + n_trig,
                                  static_cast<uint2*>(w->trig_pairs.p), kTriggerPairCap};
            rc = w->broadphase.query_boxes(w->stream, w->view, w->entity_of_slot.as<uint32_t>(), &palette, q);
            if (rc != BGE_OK) return fail(rc, "trigger query failed: %s", w->broadphase.error());
            big_list = w->trig_lists.as<uint32_t>();
        }
        HIP_TRY(bge::launch_trigger_pairs(w->stream, ticked_slots(w), n_trig,
                                          w->trigger_view(), w->view, w->entity_of_slot.as<uint32_t>(), w->trig_count.as<uint32_t>(),
                                          w->trig_pairs.p, kTriggerPairCap, big_list,
                                          big_list ? w->trig_count.as<uint32_t>() + 1 : nullptr));
        HIP_TRY(bge::launch_trigger_ghost_pairs(w->stream, n_trig, w->trigger_view(), w->trig_count.as<uint32_t>(), w->trig_pairs.p,
                                                kTriggerPairCap));
        // The short way needs last tick's table to hold exactly the host's sets and no one-shot volume in the world (one that
        // fires leaves the world in the middle of ProcessTriggerEvents' loop and takes itself out of the later ghosts' lists:
        // that order dependence stays on the host)
        int how = 1;
        if (w->trig_device_diff && w->trig_mirror_valid && !any_one_shot(w)) {
            how = process_trigger_pairs_fast(w);
            if (how < 0) return how;
        }
        if (how == 1) {
            if (int rc2 = process_trigger_pairs(w)) return rc2;
            ++w->trig_slow_ticks;
            w->trig_mirror_valid = false;
            if (w->trig_device_diff && !any_one_shot(w)) {
                if (int rc2 = rebuild_trigger_mirror(w)) return rc2;
            }
        }
    }
    return BGE_OK;
}

int tick_impl(bge_world* w, uint32_t ticks, float dt, const float gravity[3], uint32_t flags, SubStep sub)
{
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (!w->has_topology) return fail(BGE_ERR_STATE, "bge_world_set_topology has not been called");
    if ((flags & (BGE_TICK_PHYSICS | BGE_TICK_TRANSFORMS)) == 0) return fail(BGE_ERR_INVALID, "tick flags select nothing");
    if ((flags & (BGE_TICK_BROADPHASE | BGE_TICK_AABBS)) && !(flags & BGE_TICK_PHYSICS)) {
        return fail(BGE_ERR_INVALID, "BGE_TICK_BROADPHASE / BGE_TICK_AABBS need BGE_TICK_PHYSICS (the AABBs come from the physics step)");
    }
    if ((flags & BGE_TICK_BULLET_BASIS) && !(flags & BGE_TICK_PHYSICS)) {
        return fail(BGE_ERR_INVALID, "BGE_TICK_BULLET_BASIS needs BGE_TICK_PHYSICS (it selects how the physics step carries orientations)");
    }
    if ((flags & BGE_TICK_PHYSICS) && !gravity) return fail(BGE_ERR_INVALID, "gravity is NULL");
    if ((flags & BGE_TICK_NORMAL_MATRICES) && !(flags & BGE_TICK_TRANSFORMS)) {
        return fail(BGE_ERR_INVALID, "BGE_TICK_NORMAL_MATRICES needs BGE_TICK_TRANSFORMS (they are derived from the new world matrices)");
    }
    DeviceGuard guard(w->device);
    if ((flags & BGE_TICK_NORMAL_MATRICES) && w->normal.bytes < w->normal.bytes_for(w->slot_rows())) {
        HIP_TRY(hipStreamSynchronize(w->stream));
        HIP_TRY(w->normal.ensure(w->normal.bytes_for(w->slot_rows())));
        HIP_TRY(hipMemsetAsync(w->normal.p, 0, w->normal.bytes, w->stream));
        w->rebuild_view();
    }
    const bool phys = (flags & BGE_TICK_PHYSICS) != 0;
    const bool xform = (flags & BGE_TICK_TRANSFORMS) != 0;
    if (phys) w->physics_updates += ticks; // (bodies uploaded before this call are in the world from now on)
    if (phys && (w->grav_palette_stale || gravity[0] != w->grav_cached[0] || gravity[1] != w->grav_cached[1] ||
                 gravity[2] != w->grav_cached[2] || std::memcmp(gravity, w->grav_cached, 12) != 0)) {
        // btRigidBody::setGravity: m_gravity = acceleration / m_inverseMass, one IEEE division per component (the same
        // correctly rounded binary32 division on the host as the kernel's fallback path performs on the device)
        std::vector<float> tab(256 * 4, 0.0f);
        for (size_t k = 0; k < w->palette_inv_mass.size() && k < 256; ++k) {
            const float im = w->palette_inv_mass[k];
            if (im != 0.0f) {
                tab[4 * k] = gravity[0] / im;
                tab[4 * k + 1] = gravity[1] / im;
                tab[4 * k + 2] = gravity[2] / im;
            }
            tab[4 * k + 3] = im;
        }
        HIP_TRY(hipStreamSynchronize(w->stream)); // ticks in flight still read the old table
        HIP_TRY(hipMemcpy(w->grav_palette.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
        std::memcpy(w->grav_cached, gravity, 12);
        w->grav_palette_stale = false;
    }
    if (w->profiling) {
        // room for every pair of this call, so that no mid-run synchronisation is needed
        const size_t need = w->prof_used + 2 * static_cast<size_t>(w->profiling == 2 ? ticks : 1);
        while (w->prof_events.size() < need && w->prof_events.size() < (1u << 20)) {
            hipEvent_t e = nullptr;
            HIP_TRY(hipEventCreate(&e));
            w->prof_events.push_back(e);
        }
    }
    const size_t n_passes = w->flat.pass_tile_begin.size() - 1;
    const bge::TickScene scene{w->flat.n_slots, n_passes, w->any_frozen, w->ground_plane || w->static_contacts || w->dynamic_contacts,
                               w->shape.all_flat, w->shape.any_flat_all_dynamic, w->profiling};
    const bge::TickPlan plan = bge::TickPlan::of(flags, scene, bge::TickKnobs::from_env(), w->row3);
    bge::TickGroups groups(plan, ticks);
    for (uint32_t t = 0; t < ticks; ++t) {
        if (!phys && !w->maybe_dirty && !(flags & BGE_TICK_NORMAL_MATRICES)) {
            // TransformSystem::Update with nothing dirty: a no-op scan — only the kernel launches are skipped.  The
            // collective is NOT: a peer rank may have dirty transforms and issue its gather, and a rank that stayed
            // away would leave it hanging (and let the ranks' ring frame counters drift apart).  The unchanged roots are
            // packed from the world array and gathered like any other frame.
            if (flags & BGE_TICK_GATHER_ROOTS) {
                if (int rc = bge_world_gather_roots(w, nullptr)) return rc;
            }
            continue;
        }
        bge::TickParams p{};
        p.dt = dt;
        p.gx = gravity ? gravity[0] : 0.0f;
        p.gy = gravity ? gravity[1] : 0.0f;
        p.gz = gravity ? gravity[2] : 0.0f;
        p.nt_out = plan.nt_out ? 1u : 0u;
        p.no_repose = sub.no_repose ? 1u : 0u;
        p.flag_word = plan.flag_word ? 1u : 0u;
        const bge::TickGroups::Tick group = groups.next(t, w->fuse);
        if (group.clear_adv) HIP_TRY(hipMemsetAsync(w->adv.p, 0, w->adv.bytes, w->stream));
        p.serial = group.serial;
        p.n_left = group.n_left;
        p.n_solo = group.n_solo;
        // (a tick without the translation-row path may write pos or world from any of its kernels, and moves the rows epoch)
        if (!plan.rows_path) HIP_TRY(w->ensure_row3_current());
        if (plan.rows_path) p.rs_epoch = w->epochs.rows;
        else if (w->epochs.tick_without_rows()) w->words_clear();
        if (plan.defer_row3) {
            p.defer_row3 = 1u;
            w->row3.deferred(w->epochs.rows);
        }
        if (plan.rest_path) p.rest_epoch = w->epochs.rest;
        else if (w->epochs.tick_without_rest()) w->words_clear();
        w->fill_sleep(p);
        const bool with_triggers = (flags & BGE_TICK_BROADPHASE) && !w->triggers.empty();
        if (with_triggers && !sub.ghosts_posed) {
            if (int rc = pose_ghosts(w)) return rc;
        }
        if (flags & BGE_TICK_BROADPHASE) {
            // the broadphase takes its grid from per-wave partials the tick kernel writes beside the AABBs
            const size_t need = std::max<size_t>(w->flat.n_tiles_total, 1) * 4 * 32;
            if (w->bp_partials.bytes < need) {
                HIP_TRY(hipStreamSynchronize(w->stream));
                HIP_TRY(w->bp_partials.ensure(need));
            }
            p.bp_partial = w->bp_partials.as<float4>();
        }
        if (plan.contacts) {
            if (int rc = contact_substep(w, p, dt, gravity, flags, sub)) return rc;
        }
        // BGE_TICK_GATHER_ROOTS with a transform pass: the roots write the all-gather's send buffer themselves
        const bool fused_gather = (flags & BGE_TICK_GATHER_ROOTS) && xform;
        if (flags & BGE_TICK_GATHER_ROOTS) {
            if (!w->comm.ready()) return fail(BGE_ERR_STATE, "BGE_TICK_GATHER_ROOTS needs bge_world_comm_init");
            if (w->flat.root_slots.size() > w->comm.rows_per_rank()) {
                return fail(BGE_ERR_INVALID, "%zu roots but the communicator was sized for %llu rows per rank",
                            w->flat.root_slots.size(), (unsigned long long)w->comm.rows_per_rank());
            }
        }
        if (fused_gather) {
            float* send = nullptr;
            if (w->comm.begin_frame(w->stream, &send) != BGE_OK) return fail(BGE_ERR_HIP, "%s", w->comm.error());
            p.root_out = send;
        }
        const bool pair_begins = w->profiling == 2 || (w->profiling == 1 && t == 0);
        const bool pair_ends = w->profiling == 2 || (w->profiling == 1 && t + 1 == ticks);
        if (pair_begins) {
            if (w->prof_used + 2 > w->prof_events.size()) {
                if (int rc = fold_profile(w)) return rc;
            }
            HIP_TRY(hipEventRecord(w->prof_events[w->prof_used], w->stream));
        }
        for (size_t pass = 0; pass < n_passes && group.launch; ++pass) { // (a later tick of a solo group: its work is in the group's launch)
            p.tile_begin = w->flat.pass_tile_begin[pass];
            const uint32_t n_tiles = w->flat.pass_tile_begin[pass + 1] - p.tile_begin;
            HIP_TRY(bge::launch_tick(w->stream, w->view, p, n_tiles, flags));
        }
        if (pair_ends) {
            HIP_TRY(hipEventRecord(w->prof_events[w->prof_used + 1], w->stream));
            w->prof_used += 2;
            w->prof_ticks_pending.push_back(w->profiling == 2 ? 1u : ticks);
        }
        if (flags & BGE_TICK_BROADPHASE) {
            if (int rc = broadphase_and_triggers(w, with_triggers)) return rc;
        }
        w->maybe_dirty = phys && !xform;
        if (fused_gather) {
            if (w->comm.gather(w->stream, nullptr) != BGE_OK) return fail(BGE_ERR_HIP, "%s", w->comm.error());
        } else if (flags & BGE_TICK_GATHER_ROOTS) {
            if (int rc = bge_world_gather_roots(w, nullptr)) return rc;
        }
    }
    return BGE_OK;
}
} // namespace

// Bullet's btDiscreteDynamicsWorld::stepSimulation(timeStep, maxSubSteps, fixedTimeStep) around the world's ticks, as
// PhysicsSystem::StepSimulation calls it (src/physics/PhysicsSystem.cpp:855-863): the clock m_localTime accumulates
// timeStep; floor(m_localTime / fixedTimeStep) sub-steps are due and ALL of them are taken off the clock, but at most
// maxSubSteps are simulated; maxSubSteps == 0 is Bullet's variable-step mode (one step of timeStep, none when it is ~0).
// All arithmetic in binary32, as in the reference's single-precision Bullet build.
int bge_world_step_simulation(bge_world* w, double dt, int max_sub_steps, float fixed_step, const float gravity[3],
                              uint32_t flags, int* sub_steps)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (!(flags & BGE_TICK_PHYSICS)) return fail(BGE_ERR_INVALID, "bge_world_step_simulation needs BGE_TICK_PHYSICS");
    if (max_sub_steps < 0) return fail(BGE_ERR_INVALID, "max_sub_steps %d < 0", max_sub_steps);
    if (max_sub_steps > 0 && !(fixed_step > 0.0f)) return fail(BGE_ERR_INVALID, "fixed_step must be positive");
    const float time_step = static_cast<float>(dt); // stepSimulation(static_cast<btScalar>(dt), ...), PhysicsSystem.cpp:863
    int due = 0;
    float step = fixed_step;
    if (max_sub_steps > 0) {
        w->local_time = w->local_time + time_step;
        if (w->local_time >= fixed_step) {
            due = static_cast<int>(w->local_time / fixed_step);
            w->local_time = w->local_time - static_cast<float>(due) * fixed_step;
        }
    } else {
        // variable time step: m_localTime = m_latencyMotionStateInterpolation ? 0 : timeStep (not observable here);
        // btFuzzyZero(timeStep) ? 0 : 1 sub-step of timeStep
        step = time_step;
        due = std::fabs(time_step) < 1.1920928955078125e-07f ? 0 : 1;
        max_sub_steps = 1;
    }
    if (sub_steps) *sub_steps = due; // what stepSimulation returns (and LogStats prints as "substeps")
    const int run = std::min(due, max_sub_steps);
    const bool triggers = (flags & BGE_TICK_BROADPHASE) && !w->triggers.empty();
    SubStep sub{};
    if (triggers) {
        if (!w->has_topology) return fail(BGE_ERR_STATE, "bge_world_set_topology has not been called");
        // EnsureTrigger / SyncTriggersToPhysics pose the ghosts from the Transforms as they are BEFORE stepSimulation
        DeviceGuard guard(w->device);
        if (int rc = pose_ghosts(w)) return rc;
        sub.ghosts_posed = true;
    }
    if (run == 0) {
        w->physics_updates += 1; // EnsureRigidBody runs in every PhysicsSystem::Update, sub-steps or not
        // no sub-step: no collision detection, no integration — but the calls around stepSimulation still run
        if (!w->has_topology) return fail(BGE_ERR_STATE, "bge_world_set_topology has not been called");
        DeviceGuard guard(w->device);
        HIP_TRY(w->ensure_row3_current());
        HIP_TRY(bge::launch_pose_only(w->stream, w->view, ticked_slots(w), (flags & BGE_TICK_BULLET_BASIS) != 0));
        w->maybe_dirty = true;
        w->epochs_edit(); // (k_pose_only re-poses: it writes quat, euler, velocities, and marks every Dynamic Transform dirty)
        if (triggers) {
            process_triggers_without_a_step(w);
        }
        const uint32_t rest = flags & (BGE_TICK_TRANSFORMS | BGE_TICK_NORMAL_MATRICES | BGE_TICK_GATHER_ROOTS);
        if (rest & BGE_TICK_TRANSFORMS) return tick_impl(w, 1, step, gravity, rest, sub);
        if (rest & BGE_TICK_GATHER_ROOTS) return bge_world_gather_roots(w, nullptr); // the collective is never skipped
        return BGE_OK;
    }
    // sub-steps before the last one: physics only (AABBs, pairs, world matrices and the gather are observable only after
    // the call); the teleport rule belongs to the first
    const uint32_t inner = flags & (BGE_TICK_PHYSICS | BGE_TICK_BULLET_BASIS);
    if (run >= 2) {
        if (int rc = tick_impl(w, 1, step, gravity, inner, sub)) return rc;
        sub.no_repose = true;
        if (run > 2) {
            if (int rc = tick_impl(w, static_cast<uint32_t>(run - 2), step, gravity, inner, sub)) return rc;
        }
    }
    return tick_impl(w, 1, step, gravity, flags, sub);
}
BGE_CATCH_ALL("bge_world_step_simulation")

int bge_world_reset_clock(bge_world* w)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    w->local_time = 0.0f;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_reset_clock")

int bge_world_set_ground_plane(bge_world* w, int enabled)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    DeviceGuard guard(w->device);
    const bool on = enabled != 0;
    if (int rc = on ? make_store(w, w->manifold) : BGE_OK) return rc;
    w->ground_plane = on;
    w->epochs_edit();
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_set_ground_plane")

int bge_world_set_static_contacts(bge_world* w, int enabled)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    DeviceGuard guard(w->device);
    const bool on = enabled != 0;
    if (int rc = on ? make_store(w, w->bmanifold) : BGE_OK) return rc;
    if (!on && w->static_contacts && w->has_topology && w->bmanifold.p && w->bmanifold.bytes >= w->bmanifold.bytes_for(w->slot_rows())) {
        // switching off ends every pair with an obstacle here and now: no body keeps a manifold row or kCiBoxes (contact_substep hands
        // the kernels no obstacle list and no box list while the switch is off, so nothing may still ask for them)
        HIP_TRY(hipStreamSynchronize(w->stream));
        HIP_TRY(bge::launch_end_obstacle_pairs(w->stream, w->view, w->slot_rows()));
    }
    w->static_contacts = on;
    w->static_contacts_ever = w->static_contacts_ever || on;
    w->obstacles_stale = true;
    w->epochs_edit();
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_set_static_contacts")

int bge_world_set_dynamic_contacts(bge_world* w, int enabled)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    DeviceGuard guard(w->device);
    HIP_TRY(hipStreamSynchronize(w->stream));
    if (int rc = enabled ? make_store(w, w->bmanifold, true) : BGE_OK) return rc;
    if (const char* e = std::getenv("BGE_ISLAND_BIG_POINTS")) w->isl_big_points = static_cast<uint32_t>(std::strtoul(e, nullptr, 10));
    w->dynamic_contacts = enabled != 0;
    w->isl_n_prev = 0; // (off and on again: the pair cache starts empty)
    w->isl_gen_stale = true;
    w->epochs_edit();
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_set_dynamic_contacts")

int bge_world_download_dynamic_pairs(bge_world* w, uint64_t cap, uint32_t* header3, float* points48, uint64_t* total)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (!total) return fail(BGE_ERR_INVALID, "total is NULL");
    DeviceGuard guard(w->device);
    HIP_TRY(hipStreamSynchronize(w->stream));
    const uint32_t n = w->dynamic_contacts ? w->isl_n_prev : 0u;
    *total = n;
    const uint64_t take = std::min<uint64_t>(n, cap);
    if (take == 0 || (!header3 && !points48)) return BGE_OK;
    const int at = w->isl_cur ^ 1; // (island_substep flipped the generations)
    std::vector<uint64_t> keys(take);
    std::vector<uint32_t> man(take * bge::kBoxManifoldWords);
    HIP_TRY(hipMemcpy(keys.data(), w->isl_keys[at].p, take * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(man.data(), w->isl_man[at].p, take * bge::kBoxManifoldWords * 4, hipMemcpyDeviceToHost));
    for (uint64_t k = 0; k < take; ++k) {
        const uint32_t* m = man.data() + k * bge::kBoxManifoldWords;
        if (header3) {
            header3[3 * k] = static_cast<uint32_t>(keys[k] >> 32);
            header3[3 * k + 1] = static_cast<uint32_t>(keys[k]);
            header3[3 * k + 2] = m[0];
        }
        if (points48) {
            float* o = points48 + 48 * k;
            for (uint32_t j = 0; j < 4; ++j) {
                for (uint32_t q = 0; q < 12; ++q) o[12 * j + q] = j < m[0] ? reinterpret_cast<const float*>(m + 4)[12 * j + q] : 0.0f;
            }
        }
    }
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_download_dynamic_pairs")

// RigidBody::restitution / ::friction: one float per entity into its per-slot array
static int upload_scalar(bge_world* w, const Entities& e, const float* value, const char* name, SlotBuf* dst)
{
    return with_entities(
        w, e,
        [&]() -> int {
            if (e.count == 0) return kNothingToDo;
            return value ? BGE_OK : fail(BGE_ERR_INVALID, "%s is NULL", name);
        },
        [&](const uint32_t* di) -> int { return upload_rows(w, e.first, e.count, value, *dst, 0, di); });
}

int bge_world_upload_restitution(bge_world* w, uint64_t first, uint64_t count, const float* restitution)
try {
    return upload_scalar(w, Entities::range(first, count), restitution, "restitution", w ? &w->crestitution : nullptr);
}
BGE_CATCH_ALL("bge_world_upload_restitution")

int bge_world_upload_restitution_indexed(bge_world* w, uint64_t count, const uint32_t* entity_index, const float* restitution)
try {
    return upload_scalar(w, Entities::list(count, entity_index), restitution, "restitution", w ? &w->crestitution : nullptr);
}
BGE_CATCH_ALL("bge_world_upload_restitution_indexed")

int bge_world_download_box_contacts(bge_world* w, uint64_t first, uint64_t count, uint8_t* n_manifolds, uint32_t* header8, float* points192)
try {
    if (int rc = check_range(w, first, count)) return rc;
    if (count == 0) return BGE_OK;
    DeviceGuard guard(w->device);
    std::vector<uint32_t> ci(count);
    if (int rc = download_rows(w, first, count, w->cinfo, ci.data())) return rc;
    const uint32_t kWords = w->bmanifold.words;
    std::vector<uint32_t> rows;
    if (w->bmanifold.p) {
        rows.resize(count * kWords);
        if (int rc = download_rows(w, first, count, w->bmanifold, rows.data())) return rc;
    }
    for (uint64_t i = 0; i < count; ++i) {
        // the device keeps a body's rows in no particular order: ascending entity of the other box here
        uint32_t order[bge::kBoxManifolds];
        uint32_t n = 0;
        if (w->bmanifold.p && (ci[i] & bge::kCiBoxes)) {
            for (uint32_t e = 0; e < bge::kBoxManifolds; ++e) {
                if (rows[i * kWords + e * bge::kBoxManifoldWords] != bge::kBoxNone) order[n++] = e;
            }
            std::sort(order, order + n, [&](uint32_t a, uint32_t b) {
                return rows[i * kWords + a * bge::kBoxManifoldWords] < rows[i * kWords + b * bge::kBoxManifoldWords];
            });
        }
        if (n_manifolds) n_manifolds[i] = static_cast<uint8_t>(n);
        for (uint32_t k = 0; k < bge::kBoxManifolds; ++k) {
            const uint32_t* src = k < n ? &rows[i * kWords + order[k] * bge::kBoxManifoldWords] : nullptr;
            if (header8) {
                header8[8 * i + 2 * k] = src ? src[0] : bge::kBoxNone;
                header8[8 * i + 2 * k + 1] = src ? src[1] : 0u;
            }
            if (points192) {
                float* dst = points192 + 192 * i + 48 * k;
                if (src) {
                    std::memcpy(dst, src + 4, 48 * 4);
                    for (uint32_t j = src[1]; j < 4; ++j) std::memset(dst + 12 * j, 0, 48); // (points beyond the count: whatever the row held)
                } else {
                    std::memset(dst, 0, 48 * 4);
                }
            }
        }
    }
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_download_box_contacts")

int bge_world_upload_friction(bge_world* w, uint64_t first, uint64_t count, const float* friction)
try {
    return upload_scalar(w, Entities::range(first, count), friction, "friction", w ? &w->cfriction : nullptr);
}
BGE_CATCH_ALL("bge_world_upload_friction")

int bge_world_upload_friction_indexed(bge_world* w, uint64_t count, const uint32_t* entity_index, const float* friction)
try {
    return upload_scalar(w, Entities::list(count, entity_index), friction, "friction", w ? &w->cfriction : nullptr);
}
BGE_CATCH_ALL("bge_world_upload_friction_indexed")

int bge_world_download_contacts(bge_world* w, uint64_t first, uint64_t count, uint8_t* n_points, float* points32)
try {
    if (int rc = check_range(w, first, count)) return rc;
    if (count == 0) return BGE_OK;
    DeviceGuard guard(w->device);
    std::vector<uint32_t> ci(count);
    if (int rc = download_rows(w, first, count, w->cinfo, ci.data())) return rc;
    if (n_points) {
        for (uint64_t i = 0; i < count; ++i) n_points[i] = w->manifold.p ? static_cast<uint8_t>((ci[i] >> bge::kCiCountShift) & 7u) : 0;
    }
    if (points32) {
        if (!w->manifold.p) {
            std::memset(points32, 0, w->manifold.bytes_for(count));
        } else if (int rc = download_rows(w, first, count, w->manifold, points32)) {
            return rc;
        }
    }
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_download_contacts")

int bge_world_tick(bge_world* w, float dt, const float gravity[3], uint32_t flags)
try {
    return bge_world_tick_many(w, 1, dt, gravity, flags);
}
BGE_CATCH_ALL("bge_world_tick")

int bge_world_profile_enable(bge_world* w, int enable)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    DeviceGuard guard(w->device);
    if (enable && w->prof_events.empty()) {
        w->prof_events.resize(2048);
        for (hipEvent_t& e : w->prof_events) {
            e = nullptr;
            HIP_TRY(hipEventCreate(&e));
        }
    }
    if (int rc = fold_profile(w)) return rc;
    w->prof_ms_carry = 0.0;
    w->prof_ticks_carry = 0;
    w->profiling = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_profile_enable")

int bge_world_profile_read(bge_world* w, double* tick_kernel_ms, uint64_t* ticks)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    DeviceGuard guard(w->device);
    if (int rc = fold_profile(w)) return rc;
    if (tick_kernel_ms) *tick_kernel_ms = w->prof_ms_carry;
    if (ticks) *ticks = w->prof_ticks_carry;
    w->prof_ms_carry = 0.0;
    w->prof_ticks_carry = 0;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_profile_read")

int bge_world_sync(bge_world* w)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    DeviceGuard guard(w->device);
    HIP_TRY(hipStreamSynchronize(w->stream));
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_sync")

int bge_world_download_world(bge_world* w, uint64_t first, uint64_t count, float* out16)
try {
    if (int rc = check_range(w, first, count)) return rc;
    if (!out16) return fail(BGE_ERR_INVALID, "out16 is NULL");
    if (count == 0) return BGE_OK;
    DeviceGuard guard(w->device);
    return download_rows(w, first, count, w->world, out16);
}
BGE_CATCH_ALL("bge_world_download_world")

int bge_world_download_world_indexed(bge_world* w, uint64_t count, const uint32_t* entity_index, float* out16)
try {
    return with_entities(
        w, Entities::list(count, entity_index),
        [&]() -> int {
            if (count == 0) return kNothingToDo;
            return out16 ? BGE_OK : fail(BGE_ERR_INVALID, "NULL argument");
        },
        [&](const uint32_t* di) -> int { return download_rows(w, 0, count, w->world, out16, di); }, "NULL argument");
}
BGE_CATCH_ALL("bge_world_download_world_indexed")

static int download_pose(bge_world* w, const Entities& e, float* pos3, float* euler3)
{
    return with_entities(
        w, e, [&] { return e.count ? BGE_OK : kNothingToDo; },
        [&](const uint32_t* di) -> int {
            for (auto [src, host] : {std::pair{&w->pos, pos3}, {&w->euler, euler3}}) {
                if (!host) continue;
                if (int rc = download_rows(w, e.first, e.count, *src, host, di)) return rc;
            }
            return BGE_OK;
        });
}

int bge_world_download_pose_indexed(bge_world* w, uint64_t count, const uint32_t* entity_index, float* pos3, float* euler3)
try {
    return download_pose(w, Entities::list(count, entity_index), pos3, euler3);
}
BGE_CATCH_ALL("bge_world_download_pose_indexed")

int bge_world_download_normal(bge_world* w, uint64_t first, uint64_t count, float* out16)
try {
    if (int rc = check_range(w, first, count)) return rc;
    if (!out16) return fail(BGE_ERR_INVALID, "out16 is NULL");
    if (!w->normal.p) return fail(BGE_ERR_STATE, "no tick with BGE_TICK_NORMAL_MATRICES has run");
    if (count == 0) return BGE_OK;
    DeviceGuard guard(w->device);
    return download_rows(w, first, count, w->normal, out16);
}
BGE_CATCH_ALL("bge_world_download_normal")

int bge_world_download_pose(bge_world* w, uint64_t first, uint64_t count, float* pos3, float* euler3)
try {
    return download_pose(w, Entities::range(first, count), pos3, euler3);
}
BGE_CATCH_ALL("bge_world_download_pose")

int bge_world_download_bodies(bge_world* w, uint64_t first, uint64_t count, float* linvel3, float* angvel3, float* quat4,
                              float* aabb6)
try {
    if (int rc = check_range(w, first, count)) return rc;
    if (count == 0) return BGE_OK;
    DeviceGuard guard(w->device);
    if (linvel3) {
        if (int rc = download_rows(w, first, count, w->vel, linvel3)) return rc;
    }
    if (angvel3) {
        if (int rc = download_rows(w, first, count, w->angvel, angvel3)) return rc;
    }
    if (quat4) {
        if (int rc = download_rows(w, first, count, w->quat, quat4)) return rc;
    }
    if (aabb6) {
        if (int rc = download_rows(w, first, count, w->aabb, aabb6)) return rc;
    }
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_download_bodies")

int bge_world_download_activation(bge_world* w, uint64_t first, uint64_t count, uint8_t* state, float* time)
try {
    if (int rc = check_range(w, first, count)) return rc;
    if (count == 0) return BGE_OK;
    DeviceGuard guard(w->device);
    std::vector<uint32_t> rec(count), fl(count);
    if (int rc = download_rows(w, first, count, w->deact, rec.data())) return rc;
    if (int rc = download_rows(w, first, count, w->flags, fl.data())) return rc;
    for (uint64_t i = 0; i < count; ++i) {
        const uint32_t type = fl[i] & bge::kTypeMask; // download_rows zero-fills entities without a slot
        const uint32_t r = (fl[i] & bge::kDrowsy) ? rec[i] : 0u;
        uint8_t s = BGE_ACTIVATION_NONE;
        float t = 0.0f;
        if (type == 1u) s = BGE_ISLAND_SLEEPING;           // addRigidBody puts static objects to sleep
        else if (type == 3u) s = BGE_DISABLE_DEACTIVATION; // PhysicsSystem.cpp:457
        else if (type == 2u) {
            if (r == bge::kDeactSleeping) s = BGE_ISLAND_SLEEPING;
            else if (r == bge::kDeactWants) s = BGE_WANTS_DEACTIVATION;
            else {
                s = BGE_ACTIVE_TAG;
                std::memcpy(&t, &r, 4);
            }
        }
        if (state) state[i] = s;
        if (time) time[i] = t;
    }
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_download_activation")

int bge_world_set_sleeping(bge_world* w, float linear_threshold, float angular_threshold, float seconds)
try {
    if (!w) return fail(BGE_ERR_INVALID, "NULL argument");
    if (!(linear_threshold >= 0.0f) || !(angular_threshold >= 0.0f) || !(seconds >= 0.0f))
        return fail(BGE_ERR_INVALID, "sleeping thresholds must be >= 0");
    DeviceGuard guard(w->device);
    w->sleep_lin = linear_threshold;
    w->sleep_ang = angular_threshold;
    w->sleep_time = seconds;
    w->epochs_edit(); // (what decides a body's deactivation state changed)
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_set_sleeping")

// Page-locked host memory: transfers to and from it run at the full PCIe rate (~55 GB/s against ~10 GB/s pageable).
int bge_host_alloc(uint64_t bytes, void** out)
try {
    if (!out) return fail(BGE_ERR_INVALID, "NULL argument");
    *out = nullptr;
    void* p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? BGE_ERR_OOM : BGE_ERR_HIP, "hipHostMalloc(%llu): %s", (unsigned long long)bytes,
                                     hipGetErrorString(e));
    *out = p;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_host_alloc")

int bge_host_free(void* p)
try {
    if (!p) return BGE_OK;
    const hipError_t e = hipHostFree(p);
    if (e != hipSuccess) return fail(BGE_ERR_HIP, "hipHostFree: %s", hipGetErrorString(e));
    return BGE_OK;
}
BGE_CATCH_ALL("bge_host_free")

void bge_device_memory(uint64_t* allocations, uint64_t* bytes)
{
    if (allocations) *allocations = bge::live_memory().allocations.load(std::memory_order_relaxed);
    if (bytes) *bytes = bge::live_memory().bytes.load(std::memory_order_relaxed);
}

int bge_world_download_dirty(bge_world* w, uint64_t first, uint64_t count, uint8_t* dirty)
try {
    if (int rc = check_range(w, first, count)) return rc;
    if (!dirty) return fail(BGE_ERR_INVALID, "dirty is NULL");
    if (count == 0) return BGE_OK;
    DeviceGuard guard(w->device);
    HIP_TRY(w->stage.ensure(count));
    HIP_TRY(bge::launch_dirty_bytes(w->stream, w->slot_of_entity.as<uint32_t>(), first, count, w->flags.as<uint32_t>(),
                                    w->stage.as<uint8_t>()));
    HIP_TRY(hipMemcpyAsync(dirty, w->stage.p, count, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_download_dirty")

int bge_world_dirty_count(bge_world* w, uint64_t* out)
try {
    if (!w || !out) return fail(BGE_ERR_INVALID, "NULL argument");
    if (!w->has_topology) return fail(BGE_ERR_STATE, "bge_world_set_topology has not been called");
    DeviceGuard guard(w->device);
    HIP_TRY(hipMemsetAsync(w->counter.p, 0, 8, w->stream));
    HIP_TRY(bge::launch_count_dirty(w->stream, w->flat.n_slots, w->flags.as<uint32_t>(), w->counter.as<unsigned long long>()));
    unsigned long long v = 0;
    HIP_TRY(hipMemcpyAsync(&v, w->counter.p, 8, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    *out = v;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_dirty_count")

int bge_world_pairs(bge_world* w, uint32_t* pairs2, uint64_t cap, uint64_t* total)
try {
    if (!w || !total) return fail(BGE_ERR_INVALID, "NULL argument");
    if (!w->has_topology) return fail(BGE_ERR_STATE, "bge_world_set_topology has not been called");
    DeviceGuard guard(w->device);
    bge::Broadphase& bp = w->pairs_from_slab ? w->slab_broadphase : w->broadphase;
    const int rc = bp.download(w->stream, pairs2, cap, total);
    if (rc != BGE_OK) return fail(rc, "pair download failed: %s", bp.error());
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_pairs")

// ---------------------------------------------------------------- sharded broadphase (bge_route.hip)
namespace {
int refresh_global_of_slot(bge_world* w)
{
    if (!w->global_of_slot_stale && w->global_of_slot.p) return BGE_OK;
    const uint64_t S = std::max<uint64_t>(w->flat.n_slots, 1);
    std::vector<uint32_t> g(S, bge::kNone);
    for (uint64_t s = 0; s < w->flat.n_slots; ++s) {
        const uint32_t e = w->flat.entity_of_slot[s];
        if (e != bge::kNone) g[s] = e < w->global_id_host.size() ? w->global_id_host[e] : e;
    }
    HIP_TRY(w->global_of_slot.ensure(S * 4));
    HIP_TRY(hipMemcpyAsync(w->global_of_slot.p, g.data(), S * 4, hipMemcpyHostToDevice, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    w->global_of_slot_stale = false;
    return BGE_OK;
}
} // namespace

int bge_world_set_global_ids(bge_world* w, uint64_t first, uint64_t count, const uint32_t* ids)
try {
    if (int rc = check_range(w, first, count)) return rc;
    if (count && !ids) return fail(BGE_ERR_INVALID, "ids is NULL");
    if (w->global_id_host.size() < w->flat.n_entities) {
        const size_t old = w->global_id_host.size();
        w->global_id_host.resize(w->flat.n_entities);
        for (size_t i = old; i < w->global_id_host.size(); ++i) w->global_id_host[i] = static_cast<uint32_t>(i);
    }
    for (uint64_t i = 0; i < count; ++i) w->global_id_host[first + i] = ids[i];
    w->global_of_slot_stale = true;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_set_global_ids")

int bge_world_aabb_bounds(bge_world* w, float mn[3], float mx[3], uint64_t* n_bodies)
try {
    if (!w || !mn || !mx) return fail(BGE_ERR_INVALID, "NULL argument");
    if (!w->has_topology) return fail(BGE_ERR_STATE, "bge_world_set_topology has not been called");
    DeviceGuard guard(w->device);
    const int rc = w->router.bounds(w->stream, w->view, ticked_slots(w), mn, mx, n_bodies);
    if (rc != BGE_OK) return fail(rc, "%s", w->router.error());
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_aabb_bounds")

int bge_world_axis_histogram(bge_world* w, uint32_t axis, float lo, float hi, uint32_t bins, uint64_t* hist)
try {
    if (!w || !hist) return fail(BGE_ERR_INVALID, "NULL argument");
    if (!w->has_topology) return fail(BGE_ERR_STATE, "bge_world_set_topology has not been called");
    DeviceGuard guard(w->device);
    const int rc = w->router.histogram(w->stream, w->view, ticked_slots(w), axis, lo, hi, bins, hist);
    if (rc != BGE_OK) return fail(rc, "%s", w->router.error());
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_axis_histogram")

int bge_balanced_cuts(const uint64_t* hist, uint32_t bins, float lo, float hi, uint32_t nranks, float* cuts)
try {
    if (!hist || !cuts || bins == 0 || nranks == 0) return fail(BGE_ERR_INVALID, "bad argument");
    uint64_t total = 0;
    for (uint32_t b = 0; b < bins; ++b) total += hist[b];
    const double width = (static_cast<double>(hi) - static_cast<double>(lo)) / bins;
    cuts[0] = lo;
    cuts[nranks] = hi;
    uint64_t cum = 0;
    uint32_t b = 0;
    for (uint32_t k = 1; k < nranks; ++k) {
        // smallest bin whose inclusive prefix reaches k/nranks of the bodies; the cut is that bin's upper edge
        const uint64_t target = (total * k + nranks - 1) / nranks;
        while (b < bins && cum + hist[b] < target) cum += hist[b++];
        const uint32_t edge = b < bins ? b + 1 : bins;
        cuts[k] = (hi >= lo) ? static_cast<float>(static_cast<double>(lo) + width * edge) : lo;
        if (k > 1 && cuts[k] < cuts[k - 1]) cuts[k] = cuts[k - 1];
    }
    return BGE_OK;
}
BGE_CATCH_ALL("bge_balanced_cuts")

int bge_world_bp_route(bge_world* w, uint32_t axis, uint32_t nranks, const float* cuts, uint64_t* counts)
try {
    if (!w || !counts) return fail(BGE_ERR_INVALID, "NULL argument");
    if (!w->has_topology) return fail(BGE_ERR_STATE, "bge_world_set_topology has not been called");
    if (nranks > 1 && !cuts) return fail(BGE_ERR_INVALID, "cuts is NULL");
    DeviceGuard guard(w->device);
    const float none[2] = {0.0f, 0.0f};
    const int rc = w->router.count(w->stream, w->view, ticked_slots(w), axis, nranks, cuts ? cuts : none, counts);
    if (rc != BGE_OK) return fail(rc, "%s", w->router.error());
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_bp_route")

int bge_world_bp_pack(bge_world* w, void* send_device)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (!w->has_topology) return fail(BGE_ERR_STATE, "bge_world_set_topology has not been called");
    DeviceGuard guard(w->device);
    if (int rc = refresh_global_of_slot(w)) return rc;
    const int rc = w->router.pack(w->stream, w->view, ticked_slots(w), w->global_of_slot.as<uint32_t>(), send_device);
    if (rc != BGE_OK) return fail(rc, "%s", w->router.error());
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_bp_pack")

int bge_world_bp_find(bge_world* w, const void* records_device, uint64_t n_records, uint32_t axis, float window_lo, float window_hi)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (n_records && !records_device) return fail(BGE_ERR_INVALID, "records_device is NULL");
    if (axis > 2) return fail(BGE_ERR_INVALID, "axis %u", axis);
    if (n_records > 0x7fff0000ull) return fail(BGE_ERR_INVALID, "%llu records exceed the 32-bit record index", (unsigned long long)n_records);
    DeviceGuard guard(w->device);
    bge::WorldView view{};
    const uint32_t* ids = nullptr;
    int rc = w->router.unpack(w->stream, records_device, n_records, &view, &ids);
    if (rc != BGE_OK) return fail(rc, "%s", w->router.error());
    // the number of records a slab receives changes from tick to tick: grow with 25 % headroom, never shrink
    uint64_t want_slots = std::max<uint64_t>(n_records, bge::kTile);
    if (want_slots > w->slab_broadphase.configured_slots()) want_slots += want_slots / 4;
    const uint64_t cap = std::max<uint64_t>(w->pair_capacity_req ? w->pair_capacity_req : std::max<uint64_t>(8 * want_slots, 4096),
                                            w->slab_broadphase.capacity());
    rc = w->slab_broadphase.configure(std::max<uint64_t>(want_slots, w->slab_broadphase.configured_slots()), cap);
    if (rc != BGE_OK) return fail(rc, "broadphase allocation failed: %s", w->slab_broadphase.error());
    const bge::PairWindow win{axis, window_lo, window_hi};
    rc = w->slab_broadphase.run(w->stream, view, n_records, ids, &win);
    if (rc != BGE_OK) return fail(rc, "broadphase failed: %s", w->slab_broadphase.error());
    w->pairs_from_slab = true;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_bp_find")

// The whole exchange over the world's RCCL communicator: common bounds (one all-reduce), uniform cuts along `axis`,
// counts (one all-gather), records (one grouped send/recv per peer), slab search.
int bge_world_bp_exchange(bge_world* w, uint32_t axis)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (!w->has_topology) return fail(BGE_ERR_STATE, "bge_world_set_topology has not been called");
    if (!w->comm.ready()) return fail(BGE_ERR_STATE, "bge_world_comm_init has not been called");
    if (axis > 2) return fail(BGE_ERR_INVALID, "axis %u", axis);
    const uint32_t N = static_cast<uint32_t>(w->comm.nranks());
    const uint32_t me = static_cast<uint32_t>(w->comm.rank());
    if (N > bge::kMaxSlabs) return fail(BGE_ERR_UNSUPPORTED, "at most %u ranks", bge::kMaxSlabs);
    DeviceGuard guard(w->device);
    float mn[3], mx[3];
    int rc = w->router.bounds(w->stream, w->view, ticked_slots(w), mn, mx, nullptr);
    if (rc != BGE_OK) return fail(rc, "%s", w->router.error());
    // max-reduce of (-min, max) along the axis
    HIP_TRY(w->bp_small.ensure(8 * static_cast<size_t>(N) * (N + 1) + 64));
    float ext[2] = {-mn[axis], mx[axis]};
    HIP_TRY(hipMemcpyAsync(w->bp_small.p, ext, sizeof ext, hipMemcpyHostToDevice, w->stream));
    if (w->comm.all_reduce_max(w->stream, w->bp_small.as<float>(), 2) != BGE_OK) return fail(BGE_ERR_HIP, "%s", w->comm.error());
    HIP_TRY(hipMemcpyAsync(ext, w->bp_small.p, sizeof ext, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    // balanced cuts: all-reduced histogram of the min corners -> quantiles; every rank evaluates the same code on the
    // same reduced data, so the cuts are identical everywhere
    const float lo = -ext[0], hi = ext[1];
    std::vector<float> cuts(N + 1, 0.0f);
    if (hi >= lo) {
        std::vector<uint64_t> hist(bge::kMaxHistBins, 0);
        rc = w->router.histogram(w->stream, w->view, ticked_slots(w), axis, lo, hi, bge::kMaxHistBins, hist.data());
        if (rc != BGE_OK) return fail(rc, "%s", w->router.error());
        HIP_TRY(w->bp_hist.ensure(bge::kMaxHistBins * 8));
        HIP_TRY(hipMemcpyAsync(w->bp_hist.p, hist.data(), bge::kMaxHistBins * 8, hipMemcpyHostToDevice, w->stream));
        if (w->comm.all_reduce_sum_u64(w->stream, w->bp_hist.as<uint64_t>(), bge::kMaxHistBins) != BGE_OK)
            return fail(BGE_ERR_HIP, "%s", w->comm.error());
        HIP_TRY(hipMemcpyAsync(hist.data(), w->bp_hist.p, bge::kMaxHistBins * 8, hipMemcpyDeviceToHost, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream));
        if (int rc2 = bge_balanced_cuts(hist.data(), bge::kMaxHistBins, lo, hi, N, cuts.data())) return rc2;
    }
    std::vector<uint64_t> send_counts(N, 0), table(static_cast<size_t>(N) * N, 0), recv_counts(N, 0);
    rc = w->router.count(w->stream, w->view, ticked_slots(w), axis, N, cuts.data(), send_counts.data());
    if (rc != BGE_OK) return fail(rc, "%s", w->router.error());
    uint64_t* dev_counts = reinterpret_cast<uint64_t*>(w->bp_small.as<char>() + 64);
    HIP_TRY(hipMemcpyAsync(dev_counts, send_counts.data(), 8ull * N, hipMemcpyHostToDevice, w->stream));
    if (w->comm.all_gather_bytes(w->stream, dev_counts, dev_counts + N, 8ull * N) != BGE_OK) return fail(BGE_ERR_HIP, "%s", w->comm.error());
    HIP_TRY(hipMemcpyAsync(table.data(), dev_counts + N, 8ull * N * N, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    uint64_t n_send = 0, n_recv = 0;
    for (uint32_t p = 0; p < N; ++p) {
        recv_counts[p] = table[static_cast<size_t>(p) * N + me]; // what rank p routes to my slab
        n_send += send_counts[p];
        n_recv += recv_counts[p];
    }
    HIP_TRY(w->bp_send.ensure(std::max<uint64_t>(n_send, 1) * bge::kRecordBytes));
    HIP_TRY(w->bp_recv.ensure(std::max<uint64_t>(n_recv, 1) * bge::kRecordBytes));
    if (int rc2 = refresh_global_of_slot(w)) return rc2;
    rc = w->router.pack(w->stream, w->view, ticked_slots(w), w->global_of_slot.as<uint32_t>(), w->bp_send.p);
    if (rc != BGE_OK) return fail(rc, "%s", w->router.error());
    if (w->comm.all_to_all_v(w->stream, w->bp_send.p, send_counts.data(), w->bp_recv.p, recv_counts.data(), bge::kRecordBytes) != BGE_OK)
        return fail(BGE_ERR_HIP, "%s", w->comm.error());
    const float wlo = me == 0 ? -INFINITY : cuts[me];
    const float whi = me + 1 == N ? INFINITY : cuts[me + 1];
    return bge_world_bp_find(w, w->bp_recv.p, n_recv, axis, wlo, whi);
}
BGE_CATCH_ALL("bge_world_bp_exchange")

// ---------------------------------------------------------------- character trigger events: state (bge_chartrig.hip)
namespace {

constexpr uint64_t kCharTrigMaxWords = 1ull << 28;              // 64-bit words of one bitmap
constexpr uint64_t kCharTrigMaxRows = 65535ull * bge::kCharTrigChunk; // (one grid row per chunk of ghosts)

// NULL, or why a watch over `rows` triggers and n characters cannot be kept
const char* chartrig_bound_fault(uint64_t rows, uint64_t n)
{
    const uint64_t words = (n + 63u) / 64u;
    if (rows > kCharTrigMaxRows) return "more than 65535 * 64 triggers";
    if (words != 0 && rows > kCharTrigMaxWords / words) return "triggers x ceil(n / 64) exceeds 2^28 words";
    return nullptr;
}

// The arrays whose size follows the trigger array, for `rows` triggers.  Their contents are lost: only after chartrig_settle.
int chartrig_size_rows(bge_world* w, uint64_t rows)
{
    const uint64_t r = std::max<uint64_t>(rows, 1);
    HIP_TRY(w->ct_counts.ensure(r * w->ct_words * 8));
    HIP_TRY(w->ct_row_total.ensure(r * 8));
    HIP_TRY(w->ct_row_base.ensure(r * 8));
    HIP_TRY(w->ct_ghost_rec.ensure(r * 8));
    HIP_TRY(w->ct_src_row.ensure(r * 4));
    return BGE_OK;
}

// the passes' parameters: `cur` is ct_bits[cur_buf], `prev` the other
bge::CharTrigParams chartrig_params(bge_world* w, int cur_buf, uint32_t n_ghosts)
{
    bge::CharTrigParams p{};
    p.state = w->char_state.p;
    p.desc = w->char_desc.p;
    p.group = w->ct_group.as<uint32_t>();
    p.mask = w->ct_mask.as<uint32_t>();
    p.n = static_cast<uint32_t>(w->n_characters);
    p.words = static_cast<uint32_t>(w->ct_words);
    p.ghosts = w->query_ghosts.as<bge::QueryGhost>();
    p.n_ghosts = n_ghosts;
    p.aabb = w->trig_aabb.as<float>();
    p.prev = w->ct_bits[1 - cur_buf].as<unsigned long long>();
    p.cur = w->ct_bits[cur_buf].as<unsigned long long>();
    p.counts = w->ct_counts.as<unsigned long long>();
    p.row_total = w->ct_row_total.as<unsigned long long>();
    p.row_base = w->ct_row_base.as<unsigned long long>();
    p.ghost_rec = w->ct_ghost_rec.as<uint2>();
    p.count = w->ct_count.as<uint32_t>();
    p.events = w->ct_events.p;
    p.cap = w->ct_cap;
    p.stay = (w->ct_flags & BGE_CHAR_TRIGGER_STAY_EVENTS) ? 1u : 0u;
    return p;
}

// Waits for the stream, reads the last call's count and makes the device list hold all of it (and at least min_cap records): where
// the call found more than the list holds, the list grows and is made again from the two bitmaps and the offsets the call left.
// After this the list no longer depends on the bitmaps.
int chartrig_settle(bge_world* w, uint64_t min_cap, uint32_t* count_out)
{
    HIP_TRY(hipStreamSynchronize(w->stream));
    uint32_t count = 0;
    if (w->ct_on) HIP_TRY(hipMemcpy(&count, w->ct_count.p, 4, hipMemcpyDeviceToHost));
    if (count_out) *count_out = count;
    if (!w->ct_on) return BGE_OK;
    if (count == 0xffffffffu) return fail(BGE_ERR_UNSUPPORTED, "more than 2^32 - 2 character trigger events in one call");
    const uint64_t need = std::max<uint64_t>(count, min_cap);
    if (need <= w->ct_cap) return BGE_OK;
    DevBuf grown;
    HIP_TRY(grown.ensure(need * sizeof(bge_character_trigger_event)));
    if (count <= w->ct_cap) { // (complete as it is)
        if (count) HIP_TRY(hipMemcpy(grown.p, w->ct_events.p, uint64_t(count) * sizeof(bge_character_trigger_event), hipMemcpyDeviceToDevice));
    }
    std::swap(grown, w->ct_events);
    const bool remake = count > w->ct_cap;
    w->ct_cap = need;
    if (remake) {
        HIP_TRY(bge::launch_chartrig_emit(w->stream, chartrig_params(w, w->ct_rem, w->ct_last_ghosts)));
        HIP_TRY(hipStreamSynchronize(w->stream));
    }
    return BGE_OK;
}

void chartrig_off(bge_world* w)
{
    w->ct_on = false;
    w->ct_flags = 0;
    w->ct_rem = 0;
    w->ct_rows = w->ct_words = w->ct_cap = 0;
    w->ct_last_ghosts = 0;
    for (DevBuf* b : {&w->ct_group, &w->ct_mask, &w->ct_bits[0], &w->ct_bits[1], &w->ct_counts, &w->ct_row_total, &w->ct_row_base, &w->ct_ghost_rec,
                      &w->ct_events, &w->ct_count, &w->ct_src_row}) {
        b->release();
    }
}

// bge_world_characters_update's last enqueue with the watch on, after query_prepare listed the ghosts: no synchronisation, nothing
// read back, no allocation (the arrays were sized when the watch was turned on and when the trigger array was uploaded).
int chartrig_enqueue(bge_world* w, uint32_t n_ghosts)
{
    if (w->ct_rows != w->triggers.size()) return fail(BGE_ERR_STATE, "character trigger bitmaps hold %llu rows for %llu triggers",
                                                       (unsigned long long)w->ct_rows, (unsigned long long)w->triggers.size());
    w->ct_last_ghosts = n_ghosts;
    if (n_ghosts == 0) { // every trigger is skipped: no event, the remembered sets stay
        HIP_TRY(hipMemsetAsync(w->ct_count.p, 0, 4, w->stream));
        return BGE_OK;
    }
    const int cur = 1 - w->ct_rem;
    // the rows of triggers that are not listed carry over; k_ct_test overwrites the listed ones
    HIP_TRY(hipMemcpyAsync(w->ct_bits[cur].p, w->ct_bits[w->ct_rem].p, w->ct_rows * w->ct_words * 8, hipMemcpyDeviceToDevice, w->stream));
    HIP_TRY(bge::launch_chartrig(w->stream, chartrig_params(w, cur, n_ghosts)));
    w->ct_rem = cur;
    return BGE_OK;
}

// bge_world_upload_triggers with the watch on: row i of the remembered bitmap becomes old row src_row[i], or empty.
int chartrig_permute_rows(bge_world* w, const std::vector<uint32_t>& src_row)
{
    DeviceGuard guard(w->device);
    if (int rc = chartrig_settle(w, 0, nullptr)) return rc; // (the last call's list is whole before its bitmaps go)
    const uint64_t rows = src_row.size();
    if (int rc = chartrig_size_rows(w, rows)) return rc;
    const uint64_t bytes = std::max<uint64_t>(rows * w->ct_words * 8, 8);
    DevBuf next;
    HIP_TRY(next.ensure(bytes));
    if (rows) {
        HIP_TRY(hipMemcpyAsync(w->ct_src_row.p, src_row.data(), rows * 4, hipMemcpyHostToDevice, w->stream));
        HIP_TRY(bge::launch_chartrig_gather(w->stream, static_cast<uint32_t>(rows), static_cast<uint32_t>(w->ct_words), w->ct_src_row.as<uint32_t>(),
                                            w->ct_bits[w->ct_rem].as<unsigned long long>(), next.as<unsigned long long>()));
        HIP_TRY(hipStreamSynchronize(w->stream)); // (src_row and the old bitmap die here)
    }
    std::swap(next, w->ct_bits[w->ct_rem]);
    DevBuf& other = w->ct_bits[1 - w->ct_rem];
    if (other.bytes < bytes) HIP_TRY(other.ensure(bytes));
    w->ct_rows = rows;
    w->ct_last_ghosts = 0;
    return BGE_OK;
}

} // namespace

int bge_world_upload_triggers(bge_world* w, uint64_t count, const uint32_t* entity_index, const uint8_t* shape, const float* size3,
                              const uint32_t* layer, const uint32_t* mask, const uint8_t* one_shot, const uint8_t* active)
try {
    if (int rc = check_range(w, 0, 0)) return rc;
    if (count && !entity_index) return fail(BGE_ERR_INVALID, "entity_index is NULL");
    if (w->ct_on) {
        if (const char* what = chartrig_bound_fault(count, w->n_characters)) return fail(BGE_ERR_UNSUPPORTED, "character trigger events: %s", what);
    }
    std::vector<uint32_t> ct_src_row(w->ct_on ? count : 0, bge::kCharTrigNoRow);
    std::unordered_map<uint32_t, size_t> old_index;
    for (size_t i = 0; i < w->triggers.size(); ++i) old_index[w->triggers[i].entity] = i;
    std::vector<bge_world::Trigger> next(count);
    std::unordered_map<uint32_t, bool> seen;
    for (uint64_t i = 0; i < count; ++i) {
        const uint32_t e = entity_index[i];
        if (e >= w->flat.n_entities) return fail(BGE_ERR_INVALID, "entity_index[%llu] = %u outside [0, %llu)", (unsigned long long)i, e,
                                                  (unsigned long long)w->flat.n_entities);
        if (seen.count(e)) return fail(BGE_ERR_INVALID, "entity %u carries two triggers", e);
        seen[e] = true;
        bge_world::Trigger& t = next[i];
        t.entity = e;
        t.shape = shape ? shape[i] : 0;
        if (size3) std::memcpy(t.size, size3 + 3 * i, 12);
        const uint32_t l = layer ? layer[i] : 0u;
        t.layer = l ? l : 4u; // kDefaultTriggerLayer = 1 << 2 (PhysicsSystem.cpp:38, 557)
        t.mask = mask ? mask[i] : 0xffffffffu;
        t.one_shot = one_shot && one_shot[i];
        t.component_active = !active || active[i];
        auto it = old_index.find(e);
        if (it != old_index.end()) {
            bge_world::Trigger& o = w->triggers[it->second];
            // a layer/mask change re-adds the ghost (PhysicsSystem.cpp:560-571): remembered overlaps are dropped
            if (o.layer == t.layer && o.mask == t.mask) {
                t.runtime_active = o.runtime_active;
                t.overlaps.swap(o.overlaps);
                t.overlap_bodies.swap(o.overlap_bodies);
                t.overlap_ghosts.swap(o.overlap_ghosts);
            }
            // (a ghost whose entity has no Transform keeps its place whatever is uploaded: EnsureTrigger does not reach it)
            t.posed = false;
            if (o.frozen && o.runtime_active) {
                t.frozen = true;
                t.runtime_active = true;
                std::memcpy(t.frozen_aabb, o.frozen_aabb, 24);
                std::memcpy(t.frozen_pose, o.frozen_pose, 32);
                t.layer = o.layer;
                t.mask = o.mask;
                if (t.overlaps.empty()) {
                    t.overlaps.swap(o.overlaps);
                    t.overlap_bodies.swap(o.overlap_bodies);
                    t.overlap_ghosts.swap(o.overlap_ghosts);
                }
            }
            // remembered characters follow the same rule: the same entity, layer and mask keep their row
            if (w->ct_on && o.layer == t.layer && o.mask == t.mask) ct_src_row[i] = static_cast<uint32_t>(it->second);
        }
    }
    if (w->ct_on) {
        if (int rc = chartrig_permute_rows(w, ct_src_row)) return rc;
    }
    w->triggers.swap(next);
    w->trig_index_of_entity.clear();
    for (size_t i = 0; i < w->triggers.size(); ++i) w->trig_index_of_entity[w->triggers[i].entity] = static_cast<uint32_t>(i);
    w->triggers_device_stale = true;
    w->trig_list_on_device = false;
    w->trig_mirror_valid = false; // (the keys carry trigger indices)
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_upload_triggers")

int bge_world_trigger_events(bge_world* w, bge_trigger_event* out, uint64_t cap, uint64_t* total)
try {
    if (!w || !total) return fail(BGE_ERR_INVALID, "NULL argument");
    *total = w->trigger_events.size();
    if (out) {
        const uint64_t take = std::min<uint64_t>(cap, w->trigger_events.size());
        if (take) std::memcpy(out, w->trigger_events.data(), take * sizeof(bge_trigger_event));
        w->trigger_events.clear();
    }
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_trigger_events")

int bge_world_set_trigger_stay_events(bge_world* w, int enabled)
try {
    if (!w) return fail(BGE_ERR_INVALID, "NULL world");
    w->trig_stay_events = enabled != 0;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_set_trigger_stay_events")

int bge_world_trigger_diff_stats(bge_world* w, uint64_t* device_ticks, uint64_t* host_ticks, uint64_t* stay_suppressed)
try {
    if (!w) return fail(BGE_ERR_INVALID, "NULL world");
    if (device_ticks) *device_ticks = w->trig_fast_ticks;
    if (host_ticks) *host_ticks = w->trig_slow_ticks;
    if (stay_suppressed) *stay_suppressed = w->trig_stay_suppressed;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_trigger_diff_stats")

int bge_world_trigger_active(bge_world* w, uint64_t count, const uint32_t* entity_index, uint8_t* active)
try {
    if (!w || (count && (!entity_index || !active))) return fail(BGE_ERR_INVALID, "NULL argument");
    std::unordered_map<uint32_t, bool> state;
    for (const bge_world::Trigger& t : w->triggers) state[t.entity] = t.component_active;
    for (uint64_t i = 0; i < count; ++i) {
        auto it = state.find(entity_index[i]);
        active[i] = it != state.end() && it->second ? 1 : 0;
    }
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_trigger_active")

int bge_world_trigger_query_stats(bge_world* w, uint32_t* through_grid, uint32_t* against_all_bodies)
try {
    if (!w) return fail(BGE_ERR_INVALID, "NULL world");
    if (through_grid) *through_grid = w->trig_through_grid;
    if (against_all_bodies) *against_all_bodies = w->trig_against_all;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_trigger_query_stats")

// ---------------------------------------------------------------- the query index: the entry points (bge_qindex.hip)
static_assert(sizeof(bge_query_index_desc) == 24, "bge_query_index_desc is 24 bytes (include/bge_world.h)");
static_assert(sizeof(bge_query_index_stats) == 64, "bge_query_index_stats is 64 bytes (include/bge_world.h)");

int bge_world_set_query_index(bge_world* w, const bge_query_index_desc* desc)
try {
    if (!w) return fail(BGE_ERR_INVALID, "NULL world");
    if (!desc) {
        w->qi_desc.mode = 0u;
        return BGE_OK;
    }
    if (desc->mode > 1u) return fail(BGE_ERR_INVALID, "bge_query_index_desc.mode = %u: 0 (off) or 1 (on)", desc->mode);
    if (!std::isfinite(desc->cell_edge) || desc->cell_edge < 0.0f) {
        return fail(BGE_ERR_INVALID, "bge_query_index_desc.cell_edge = %g: finite and >= 0 (0 = chosen by the library)", double(desc->cell_edge));
    }
    if (desc->reserved != 0u) return fail(BGE_ERR_INVALID, "bge_query_index_desc.reserved = %u: must be 0", desc->reserved);
    w->qi_desc = *desc;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_set_query_index")

int bge_world_query_index_stats(bge_world* w, bge_query_index_stats* out)
try {
    if (!w || !out) return fail(BGE_ERR_INVALID, "NULL argument");
    *out = bge_query_index_stats{};
    out->builds = w->qi_builds;
    if (!w->qi_last_built) return BGE_OK;
    DeviceGuard guard(w->device);
    uint32_t words[bge::kQiWords] = {};
    HIP_TRY(hipMemcpyAsync(words, w->qi_words.p, sizeof(words), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    out->built = 1u;
    out->table_size = w->qi_last_table;
    out->cell_edge = w->qi_last_edge;
    out->bodies_indexed = words[bge::kQiIndexed];
    out->bodies_wide = words[bge::kQiWide];
    out->queries_indexed = words[bge::kQiRoutedIndex];
    out->queries_far = words[bge::kQiRoutedFar];
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_query_index_stats")

// ---------------------------------------------------------------- queries: rays, sphere casts, sphere overlaps (bge_query.hip)
static_assert(sizeof(bge_ray) == 32, "bge_ray is 32 bytes (include/bge_world.h)");
static_assert(sizeof(bge_ray_hit) == 40, "bge_ray_hit is 40 bytes (include/bge_world.h)");
static_assert(sizeof(bge_sphere_cast) == 40, "bge_sphere_cast is 40 bytes (include/bge_world.h)");
static_assert(sizeof(bge_sphere) == 20, "bge_sphere is 20 bytes (include/bge_world.h)");
static_assert(sizeof(bge_overlap_hit) == 12, "bge_overlap_hit is 12 bytes (include/bge_world.h)");
static_assert(sizeof(bge_sphere_move) == 48, "bge_sphere_move is 48 bytes (include/bge_world.h)");
static_assert(sizeof(bge_sphere_move_result) == 80, "bge_sphere_move_result is 80 bytes (include/bge_world.h)");
static_assert(sizeof(bge_sphere_step_move) == 48, "bge_sphere_step_move is 48 bytes (include/bge_world.h)");
static_assert(sizeof(bge_sphere_step_result) == 80, "bge_sphere_step_result is 80 bytes (include/bge_world.h)");
static_assert(sizeof(bge_penetration_hit) == 40, "bge_penetration_hit is 40 bytes (include/bge_world.h)");
static_assert(sizeof(bge_sphere_recover) == 28, "bge_sphere_recover is 28 bytes (include/bge_world.h)");
static_assert(sizeof(bge_sphere_recover_result) == 64, "bge_sphere_recover_result is 64 bytes (include/bge_world.h)");

namespace {

// The trigger ghosts that are in the world for a query (ray and sphere queries, debug overlay): active, posed by a tick into the
// device arrays as they are indexed now, in the order of the uploaded trigger array.  The device copy is sent only when the list
// changed.
int sync_query_ghosts(bge_world* w)
{
    std::vector<bge::QueryGhost>& gh = w->query_ghosts_host;
    gh.clear();
    if (w->trig_list_on_device && w->trig_pose.p) {
        for (size_t i = 0; i < w->triggers.size(); ++i) {
            const bge_world::Trigger& t = w->triggers[i];
            if (!t.runtime_active || !(t.posed || t.frozen)) continue;
            bge::QueryGhost g{};
            if (t.shape == BGE_SHAPE_CAPSULE) {
                g.capsule = 1u;
                g.dims[0] = std::max(t.size[0], 0.01f); // btCapsuleShape(radius, 2 * halfHeight), as for bodies
                g.dims[1] = 0.5f * (std::max(t.size[1], 0.0f) * 2.0f);
                g.dims[2] = g.dims[0];
            } else {
                collider_half_extents(t.shape, t.size, g.dims);
            }
            g.trigger = static_cast<uint32_t>(i);
            g.entity = t.entity;
            g.group = t.layer;
            g.mask = t.mask;
            gh.push_back(g);
        }
    }
    const bool same = gh.size() == w->query_ghosts_dev.size() &&
                      (gh.empty() || std::memcmp(gh.data(), w->query_ghosts_dev.data(), gh.size() * sizeof(bge::QueryGhost)) == 0);
    if (!same) {
        w->query_ghosts_dev = gh;
        if (!gh.empty()) {
            HIP_TRY(w->query_ghosts.ensure(gh.size() * sizeof(bge::QueryGhost)));
            HIP_TRY(hipMemcpyAsync(w->query_ghosts.p, w->query_ghosts_dev.data(), gh.size() * sizeof(bge::QueryGhost), hipMemcpyHostToDevice,
                                   w->stream));
            HIP_TRY(hipStreamSynchronize(w->stream)); // (the list changes when the trigger set does, not per query)
        }
    }
    return BGE_OK;
}

// Builds the query index for a call of n queries (include/bge_world.h "Query index": once per public call, all its passes share
// it) and names it in p.qi; or leaves p.qi.on = 0: the index is off, the batch is below min_work, or there is no slot.  Buffers
// are sized here, before the first launch of the call.
int query_index_prepare(bge_world* w, uint64_t n, bge::QueryCall& p)
{
    w->qi_last_built = false;
    const bge_query_index_desc& d = w->qi_desc;
    const uint64_t slots = p.n_slots;
    if (d.mode == 0u || n == 0 || slots == 0 || slots > 0x7fffffffull) return BGE_OK;
    if (n * slots < d.min_work) return BGE_OK; // (n < 2^31, slots < 2^31)
    const uint32_t table = bge::qindex_table_size(slots);
    if (w->qi_scan_table != table) {
        w->qi_scan_bytes = bge::qindex_scan_bytes(table);
        w->qi_scan_table = table;
    }
    HIP_TRY(w->qi_count.ensure(size_t(table) * 4));
    HIP_TRY(w->qi_start.ensure(size_t(table) * 4));
    HIP_TRY(w->qi_cell.ensure(slots * 8));
    HIP_TRY(w->qi_rec_a.ensure(slots * 16));
    HIP_TRY(w->qi_rec_b.ensure(slots * 16));
    HIP_TRY(w->qi_rec_c.ensure(slots * 16));
    HIP_TRY(w->qi_scan.ensure(std::max<size_t>(w->qi_scan_bytes, 16)));
    HIP_TRY(w->qi_words.ensure(bge::kQiWords * 4));
    HIP_TRY(w->qi_far.ensure(n * 4));
    bge::QIndexView& v = p.qi;
    v.on = 1u;
    v.table = table;
    v.h = bge::qindex::edge(d.cell_edge);
    v.max_cells = d.max_cells ? d.max_cells : bge::qindex::kMaxCellsDefault;
    v.n_rec = static_cast<uint32_t>(slots);
    v.start = w->qi_start.as<uint32_t>();
    v.count = w->qi_count.as<uint32_t>();
    v.rec_a = w->qi_rec_a.as<float4>();
    v.rec_b = w->qi_rec_b.as<float4>();
    v.rec_c = w->qi_rec_c.as<uint4>();
    v.words = w->qi_words.as<uint32_t>();
    v.far_list = w->qi_far.as<uint32_t>();
    bge::QIndexBuild b{};
    b.count = w->qi_count.as<uint32_t>();
    b.start = w->qi_start.as<uint32_t>();
    b.cell = w->qi_cell.as<uint32_t>();
    b.rec_a = w->qi_rec_a.as<float4>();
    b.rec_b = w->qi_rec_b.as<float4>();
    b.rec_c = w->qi_rec_c.as<uint4>();
    b.scan_tmp = w->qi_scan.p;
    b.scan_bytes = w->qi_scan_bytes;
    HIP_TRY(bge::launch_qindex_build(w->stream, p, b));
    w->qi_last_built = true;
    w->qi_last_edge = v.h;
    w->qi_last_table = table;
    w->qi_builds += 1;
    return BGE_OK;
}

// What every query needs: the ghosts the queries see, the per-query keys, the body arrays, the query index when it is on.
int query_prepare(bge_world* w, uint64_t n, bge::QueryCall& p)
{
    if (!w->has_topology) return fail(BGE_ERR_STATE, "bge_world_set_topology has not been called");
    if (n > 0x7fffffffull) return fail(BGE_ERR_INVALID, "n_rays = %llu: at most 2^31 - 1 rays per batch", (unsigned long long)n);
    if (w->flat.n_entities > bge::kQueryEntityMask) {
        return fail(BGE_ERR_UNSUPPORTED, "ray queries need entity indices below 2^30 (world has %llu)", (unsigned long long)w->flat.n_entities);
    }
    if (int rc = sync_query_ghosts(w)) return rc;
    if (n > w->query_keys_n) {
        HIP_TRY(w->query_keys.ensure(n * 8));
        HIP_TRY(hipMemsetAsync(w->query_keys.p, 0xff, n * 8, w->stream));
        w->query_keys_n = n;
    }
    p = bge::QueryCall{};
    p.n_queries = static_cast<uint32_t>(n);
    p.n_slots = w->flat.n_slots;
    p.flags = w->view.flags;
    p.pos = w->view.pos;
    p.quat = w->view.quat;
    p.cshape = w->view.cshape;
    p.cinfo = w->view.cinfo;
    p.group = w->view.group;
    p.mask = w->view.mask;
    p.entity_of_slot = w->entity_of_slot.as<uint32_t>();
    p.slot_of_entity = w->slot_of_entity.as<uint32_t>();
    p.ghosts = w->query_ghosts.as<bge::QueryGhost>();
    p.n_ghosts = static_cast<uint32_t>(w->query_ghosts_dev.size());
    p.ghost_pose = w->trig_pose.as<float>();
    p.plane = w->ground_plane ? 1u : 0u;
    p.keys = w->query_keys.as<unsigned long long>();
    return query_index_prepare(w, n, p);
}

// the batch's query records (bge_ray, bge_sphere_cast, bge_sphere) into the staging buffer
int query_upload(bge_world* w, uint64_t bytes, const void* records, bge::QueryCall& p)
{
    HIP_TRY(w->query_in.ensure(bytes));
    HIP_TRY(hipMemcpyAsync(w->query_in.p, records, bytes, hipMemcpyHostToDevice, w->stream));
    p.records = w->query_in.p;
    return BGE_OK;
}

// Runs an all-hits launch and brings its list back sorted by query, then by (f, object code) or, for the overlap, by object code
// alone: a total order, so the result does not depend on the order of the appends.  The list's capacity grows to what a batch
// found: a second run of the same batch fits.
int query_collect(bge_world* w, bge::QueryKind kind, bge::QueryCall& p, std::vector<bge::QueryRec>& rec)
{
    HIP_TRY(w->query_all_count.ensure(4));
    p.all_count = w->query_all_count.as<uint32_t>();
    uint32_t found = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        const uint64_t want = std::max<uint64_t>({w->query_all_cap, 4096u, 4ull * p.n_queries});
        if (want > 0x7fffffffull) return fail(BGE_ERR_OOM, "ray hit list of %llu records", (unsigned long long)want);
        HIP_TRY(w->query_all.ensure(want * sizeof(bge::QueryRec)));
        w->query_all_cap = static_cast<uint32_t>(want);
        p.all = w->query_all.as<bge::QueryRec>();
        p.all_cap = w->query_all_cap;
        HIP_TRY(hipMemsetAsync(w->query_all_count.p, 0, 4, w->stream));
        HIP_TRY(bge::launch_query(w->stream, kind, p, true));
        HIP_TRY(hipMemcpyAsync(&found, w->query_all_count.p, 4, hipMemcpyDeviceToHost, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream));
        if (found <= w->query_all_cap) break;
        w->query_all_cap = found;
    }
    if (found > w->query_all_cap) return fail(BGE_ERR_STATE, "ray hit list overflowed twice");
    rec.resize(found);
    if (found) {
        HIP_TRY(hipMemcpyAsync(rec.data(), w->query_all.p, found * sizeof(bge::QueryRec), hipMemcpyDeviceToHost, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream));
    }
    const bool by_fraction = kind != bge::QueryKind::SphereOverlap;
    auto key = [by_fraction](const bge::QueryRec& r) {
        uint32_t fb = 0;
        if (by_fraction) std::memcpy(&fb, &r.f, 4);
        return std::make_pair(static_cast<uint64_t>(r.query) << 32 | fb, r.code);
    };
    std::sort(rec.begin(), rec.end(), [&](const bge::QueryRec& a, const bge::QueryRec& b) { return key(a) < key(b); });
    return BGE_OK;
}

// offsets[0 .. n] of a sorted list: the records of query i are [offsets[i], offsets[i + 1])
void query_offsets(const std::vector<bge::QueryRec>& rec, uint64_t n, uint64_t* offsets)
{
    size_t at = 0;
    for (uint64_t r = 0; r <= n; ++r) {
        while (at < rec.size() && rec[at].query < r) ++at;
        offsets[r] = at;
    }
}

// An object code as the public records name it
void decode_code(uint32_t code, uint32_t& kind, uint32_t& entity)
{
    const uint32_t k = code >> 30;
    kind = k == 0u ? BGE_RAY_BODY : (k == 1u ? BGE_RAY_TRIGGER : BGE_RAY_GROUND);
    entity = k == 2u ? BGE_RAY_NO_ENTITY : (code & bge::kQueryEntityMask);
}

// Closest hit per query (rays, sphere casts; the deepest of a penetration), host records to host hits of 40 bytes each
int query_closest(bge_world* w, bge::QueryKind kind, uint64_t n, size_t record_bytes, const void* records, void* hits)
{
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (n == 0) return BGE_OK;
    if (!records || !hits) return fail(BGE_ERR_INVALID, "NULL argument");
    DeviceGuard guard(w->device);
    bge::QueryCall p;
    if (int rc = query_prepare(w, n, p)) return rc;
    if (int rc = query_upload(w, n * record_bytes, records, p)) return rc;
    HIP_TRY(w->query_out.ensure(n * sizeof(bge_ray_hit)));
    p.hits = w->query_out.p;
    HIP_TRY(bge::launch_query(w->stream, kind, p, false));
    HIP_TRY(hipMemcpyAsync(hits, w->query_out.p, n * sizeof(bge_ray_hit), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return BGE_OK;
}

// The same between device buffers, enqueued on the world's stream
int query_closest_device(bge_world* w, bge::QueryKind kind, uint64_t n, const void* records_device, void* hits_device)
{
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (n == 0) return BGE_OK;
    if (!records_device || !hits_device) return fail(BGE_ERR_INVALID, "NULL argument");
    DeviceGuard guard(w->device);
    bge::QueryCall p;
    if (int rc = query_prepare(w, n, p)) return rc;
    p.records = records_device;
    p.hits = hits_device;
    HIP_TRY(bge::launch_query(w->stream, kind, p, false));
    return BGE_OK;
}

// A batch of sphere moves between device buffers (include/bge_world.h "Sphere moves"): begin, BGE_MOVE_SLIDES rounds of a
// closest-hit sphere-cast pass and a step, the probe's pass, finish — all enqueued, nothing read in between.  q comes from
// query_prepare(w, n, q), which holds the checks of the batch (topology, n, entity range) for both entry points.
int move_enqueue(bge_world* w, bge::QueryCall q, uint64_t n, const void* moves_device, void* results_device)
{
    HIP_TRY(w->move_state.ensure(n * bge::kMoveStateBytes));
    HIP_TRY(w->move_casts.ensure(n * sizeof(bge_sphere_cast)));
    HIP_TRY(w->move_hits.ensure(n * sizeof(bge_ray_hit)));
    q.records = w->move_casts.p;
    q.hits = w->move_hits.p;
    bge::MoveParams m{};
    m.moves = moves_device;
    m.results = results_device;
    m.state = w->move_state.as<float4>();
    m.casts = w->move_casts.p;
    m.hits = w->move_hits.p;
    m.n = static_cast<uint32_t>(n);
    HIP_TRY(bge::launch_move_begin(w->stream, m));
    for (uint32_t round = 0; round < BGE_MOVE_SLIDES; ++round) {
        HIP_TRY(bge::launch_query(w->stream, bge::QueryKind::SphereCast, q, false));
        HIP_TRY(bge::launch_move_step(w->stream, m, round));
    }
    HIP_TRY(bge::launch_query(w->stream, bge::QueryKind::SphereCast, q, false));
    HIP_TRY(bge::launch_move_finish(w->stream, m));
    return BGE_OK;
}

// A batch of sphere step moves between device buffers (include/bge_world.h "Sphere step moves"; the schedule is DESIGN.md 4.19's):
// begin, then BGE_MOVE_SLIDES passes over both lanes (2n casts: the plain slide at i, the step at n + i), two passes over the step's
// half alone (its last Forward round, its Down cast), the selection, the probe's pass over the first half, finish — all enqueued,
// nothing read in between.  q comes from query_prepare(w, 2 * n, q).  The scratch is the step mover's own.
int step_enqueue(bge_world* w, bge::QueryCall q, uint64_t n, const void* moves_device, void* results_device)
{
    HIP_TRY(w->step_state.ensure(n * bge::kStepStateBytes));
    HIP_TRY(w->step_casts.ensure(2 * n * sizeof(bge_sphere_cast)));
    HIP_TRY(w->step_hits.ensure(2 * n * sizeof(bge_ray_hit)));
    bge::StepParams m{};
    m.moves = moves_device;
    m.results = results_device;
    m.state = w->step_state.as<float4>();
    m.casts = w->step_casts.p;
    m.hits = w->step_hits.p;
    m.n = static_cast<uint32_t>(n);
    bge::QueryCall both = q, step_half = q, plain_half = q;
    both.records = plain_half.records = w->step_casts.p;
    both.hits = plain_half.hits = w->step_hits.p;
    step_half.records = static_cast<const char*>(w->step_casts.p) + n * sizeof(bge_sphere_cast);
    step_half.hits = static_cast<char*>(w->step_hits.p) + n * sizeof(bge_ray_hit);
    step_half.n_queries = plain_half.n_queries = static_cast<uint32_t>(n);
    HIP_TRY(bge::launch_step_begin(w->stream, m));
    for (uint32_t stage = 1; stage <= bge::kStepStages; ++stage) {
        HIP_TRY(bge::launch_query(w->stream, bge::QueryKind::SphereCast, stage <= BGE_MOVE_SLIDES ? both : step_half, false));
        HIP_TRY(bge::launch_step_advance(w->stream, m, stage));
    }
    HIP_TRY(bge::launch_query(w->stream, bge::QueryKind::SphereCast, plain_half, false));
    HIP_TRY(bge::launch_step_finish(w->stream, m));
    return BGE_OK;
}

// A batch of sphere recoveries between device buffers (include/bge_world.h "Sphere penetration and recovery"): begin,
// BGE_RECOVER_ROUNDS rounds of a penetration pass and a step, the final check's pass, finish — all enqueued, nothing read in
// between.  q comes from query_prepare(w, n, q).  The scratch is the recovery's own, not the mover's.
int recover_enqueue(bge_world* w, bge::QueryCall q, uint64_t n, const void* records_device, void* results_device)
{
    HIP_TRY(w->recover_state.ensure(n * bge::kRecoverStateBytes));
    HIP_TRY(w->recover_queries.ensure(n * sizeof(bge_sphere)));
    HIP_TRY(w->recover_hits.ensure(n * sizeof(bge_penetration_hit)));
    q.records = w->recover_queries.p;
    q.hits = w->recover_hits.p;
    bge::RecoverParams r{};
    r.records = records_device;
    r.results = results_device;
    r.state = w->recover_state.as<float4>();
    r.queries = w->recover_queries.p;
    r.hits = w->recover_hits.p;
    r.n = static_cast<uint32_t>(n);
    HIP_TRY(bge::launch_recover_begin(w->stream, r));
    for (uint32_t round = 0; round < BGE_RECOVER_ROUNDS; ++round) {
        HIP_TRY(bge::launch_query(w->stream, bge::QueryKind::SpherePenetration, q, false));
        HIP_TRY(bge::launch_recover_step(w->stream, r));
    }
    HIP_TRY(bge::launch_query(w->stream, bge::QueryKind::SpherePenetration, q, false));
    HIP_TRY(bge::launch_recover_finish(w->stream, r));
    return BGE_OK;
}

// One list entry point: its names in the error texts, its record sizes, and fill(hit, sorted record, the caller's record of its query)
struct QueryList {
    bge::QueryKind kind;
    const char* what;
    const char* records_name;
    size_t record_bytes, hit_bytes;
    void (*fill)(void* hit, const bge::QueryRec& r, const void* record);
};

// Every hit per query: *total and offsets always, the hits when there is room for them
int query_list(bge_world* w, const QueryList& q, uint64_t n, const void* records, void* hits, uint64_t cap, uint64_t* offsets, uint64_t* total)
{
    if (!w || !total) return fail(BGE_ERR_INVALID, "NULL argument");
    *total = 0;
    if (n == 0) {
        if (offsets) offsets[0] = 0;
        return BGE_OK;
    }
    if (!records) return fail(BGE_ERR_INVALID, "%s is NULL", q.records_name);
    DeviceGuard guard(w->device);
    bge::QueryCall p;
    if (int rc = query_prepare(w, n, p)) return rc;
    if (int rc = query_upload(w, n * q.record_bytes, records, p)) return rc;
    std::vector<bge::QueryRec> rec;
    if (int rc = query_collect(w, q.kind, p, rec)) return rc;
    *total = rec.size();
    if (offsets) query_offsets(rec, n, offsets);
    if (!hits) return BGE_OK;
    if (cap < rec.size()) return fail(BGE_ERR_INVALID, "%s: %zu hits, room for %llu", q.what, rec.size(), (unsigned long long)cap);
    for (size_t i = 0; i < rec.size(); ++i) {
        q.fill(static_cast<char*>(hits) + i * q.hit_bytes, rec[i], static_cast<const char*>(records) + rec[i].query * q.record_bytes);
    }
    return BGE_OK;
}

// The fills' point arithmetic is the device's (bge_query.hip: the descriptions' prep and point), operation for operation: the
// first record of a query's list equals its closest hit bit for bit.
void fill_ray_hit(void* hit, const bge::QueryRec& r, const void* record)
{
    bge_ray_hit& h = *static_cast<bge_ray_hit*>(hit);
    const bge_ray& ray = *static_cast<const bge_ray*>(record);
    decode_code(r.code, h.kind, h.entity);
    h.fraction = r.f;
    h.distance = r.f * ray.max_distance;
    for (int a = 0; a < 3; ++a) {
        const float delta = ray.direction[a] * ray.max_distance;
        h.point[a] = ray.origin[a] + delta * r.f;
        h.normal[a] = r.n[a];
    }
}

void fill_sphere_cast_hit(void* hit, const bge::QueryRec& r, const void* record)
{
    bge_ray_hit& h = *static_cast<bge_ray_hit*>(hit);
    const bge_sphere_cast& c = *static_cast<const bge_sphere_cast*>(record);
    decode_code(r.code, h.kind, h.entity);
    h.fraction = r.f;
    h.distance = r.f * c.max_distance;
    for (int a = 0; a < 3; ++a) {
        const float delta = c.direction[a] * c.max_distance;
        const float centre = c.origin[a] + delta * r.f;
        h.point[a] = centre - c.radius * r.n[a];
        h.normal[a] = r.n[a];
    }
    if (h.kind == BGE_RAY_GROUND) h.point[1] = 0.0f;
}

void fill_overlap_hit(void* hit, const bge::QueryRec& r, const void*)
{
    bge_overlap_hit& h = *static_cast<bge_overlap_hit*>(hit);
    decode_code(r.code, h.kind, h.entity);
    h.distance = r.f;
}

const QueryList kRaycastAll{bge::QueryKind::Ray, "raycast_all", "rays", sizeof(bge_ray), sizeof(bge_ray_hit), fill_ray_hit};
const QueryList kSphereCastAll{bge::QueryKind::SphereCast, "sphere_cast_all", "casts", sizeof(bge_sphere_cast), sizeof(bge_ray_hit), fill_sphere_cast_hit};
const QueryList kOverlapSphere{bge::QueryKind::SphereOverlap, "overlap_sphere", "spheres", sizeof(bge_sphere), sizeof(bge_overlap_hit), fill_overlap_hit};

} // namespace

int bge_world_raycast(bge_world* w, uint64_t n_rays, const bge_ray* rays, bge_ray_hit* hits)
try {
    return query_closest(w, bge::QueryKind::Ray, n_rays, sizeof(bge_ray), rays, hits);
}
BGE_CATCH_ALL("bge_world_raycast")

int bge_world_raycast_device(bge_world* w, uint64_t n_rays, const void* rays_device, void* hits_device)
try {
    return query_closest_device(w, bge::QueryKind::Ray, n_rays, rays_device, hits_device);
}
BGE_CATCH_ALL("bge_world_raycast_device")

int bge_world_raycast_all(bge_world* w, uint64_t n_rays, const bge_ray* rays, bge_ray_hit* hits, uint64_t cap, uint64_t* offsets,
                          uint64_t* total)
try {
    return query_list(w, kRaycastAll, n_rays, rays, hits, cap, offsets, total);
}
BGE_CATCH_ALL("bge_world_raycast_all")

int bge_world_sphere_cast(bge_world* w, uint64_t n, const bge_sphere_cast* casts, bge_ray_hit* hits)
try {
    return query_closest(w, bge::QueryKind::SphereCast, n, sizeof(bge_sphere_cast), casts, hits);
}
BGE_CATCH_ALL("bge_world_sphere_cast")

int bge_world_sphere_cast_device(bge_world* w, uint64_t n, const void* casts_device, void* hits_device)
try {
    return query_closest_device(w, bge::QueryKind::SphereCast, n, casts_device, hits_device);
}
BGE_CATCH_ALL("bge_world_sphere_cast_device")

int bge_world_sphere_cast_all(bge_world* w, uint64_t n, const bge_sphere_cast* casts, bge_ray_hit* hits, uint64_t cap, uint64_t* offsets,
                              uint64_t* total)
try {
    return query_list(w, kSphereCastAll, n, casts, hits, cap, offsets, total);
}
BGE_CATCH_ALL("bge_world_sphere_cast_all")

int bge_world_sphere_move(bge_world* w, uint64_t n, const bge_sphere_move* moves, bge_sphere_move_result* results)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (n == 0) return BGE_OK;
    if (!moves || !results) return fail(BGE_ERR_INVALID, "NULL argument");
    DeviceGuard guard(w->device);
    bge::QueryCall q;
    if (int rc = query_prepare(w, n, q)) return rc; // (before the staging is sized: it refuses a batch that is too large)
    HIP_TRY(w->move_in.ensure(n * sizeof(bge_sphere_move)));
    HIP_TRY(w->move_out.ensure(n * sizeof(bge_sphere_move_result)));
    HIP_TRY(hipMemcpyAsync(w->move_in.p, moves, n * sizeof(bge_sphere_move), hipMemcpyHostToDevice, w->stream));
    if (int rc = move_enqueue(w, q, n, w->move_in.p, w->move_out.p)) return rc;
    HIP_TRY(hipMemcpyAsync(results, w->move_out.p, n * sizeof(bge_sphere_move_result), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_sphere_move")

int bge_world_sphere_move_device(bge_world* w, uint64_t n, const void* moves_device, void* results_device)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (n == 0) return BGE_OK;
    if (!moves_device || !results_device) return fail(BGE_ERR_INVALID, "NULL argument");
    if ((reinterpret_cast<uintptr_t>(moves_device) | reinterpret_cast<uintptr_t>(results_device)) & 3u) {
        return fail(BGE_ERR_INVALID, "moves_device and results_device must be 4-byte aligned");
    }
    DeviceGuard guard(w->device);
    bge::QueryCall q;
    if (int rc = query_prepare(w, n, q)) return rc;
    return move_enqueue(w, q, n, moves_device, results_device);
}
BGE_CATCH_ALL("bge_world_sphere_move_device")

int bge_world_sphere_step_move(bge_world* w, uint64_t n, const bge_sphere_step_move* moves, bge_sphere_step_result* results)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (n == 0) return BGE_OK;
    if (!moves || !results) return fail(BGE_ERR_INVALID, "NULL argument");
    if (n > 0x3fffffffull) return fail(BGE_ERR_INVALID, "n = %llu: a step move asks 2 n casts per pass, at most 2^31 - 1", (unsigned long long)n);
    DeviceGuard guard(w->device);
    bge::QueryCall q;
    if (int rc = query_prepare(w, 2 * n, q)) return rc; // (before the staging is sized: it refuses a batch that is too large)
    HIP_TRY(w->step_in.ensure(n * sizeof(bge_sphere_step_move)));
    HIP_TRY(w->step_out.ensure(n * sizeof(bge_sphere_step_result)));
    HIP_TRY(hipMemcpyAsync(w->step_in.p, moves, n * sizeof(bge_sphere_step_move), hipMemcpyHostToDevice, w->stream));
    if (int rc = step_enqueue(w, q, n, w->step_in.p, w->step_out.p)) return rc;
    HIP_TRY(hipMemcpyAsync(results, w->step_out.p, n * sizeof(bge_sphere_step_result), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_sphere_step_move")

int bge_world_sphere_step_move_device(bge_world* w, uint64_t n, const void* moves_device, void* results_device)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (n == 0) return BGE_OK;
    if (!moves_device || !results_device) return fail(BGE_ERR_INVALID, "NULL argument");
    if ((reinterpret_cast<uintptr_t>(moves_device) | reinterpret_cast<uintptr_t>(results_device)) & 3u) {
        return fail(BGE_ERR_INVALID, "moves_device and results_device must be 4-byte aligned");
    }
    if (n > 0x3fffffffull) return fail(BGE_ERR_INVALID, "n = %llu: a step move asks 2 n casts per pass, at most 2^31 - 1", (unsigned long long)n);
    DeviceGuard guard(w->device);
    bge::QueryCall q;
    if (int rc = query_prepare(w, 2 * n, q)) return rc;
    return step_enqueue(w, q, n, moves_device, results_device);
}
BGE_CATCH_ALL("bge_world_sphere_step_move_device")

int bge_world_overlap_sphere(bge_world* w, uint64_t n, const bge_sphere* spheres, bge_overlap_hit* hits, uint64_t cap, uint64_t* offsets,
                             uint64_t* total)
try {
    return query_list(w, kOverlapSphere, n, spheres, hits, cap, offsets, total);
}
BGE_CATCH_ALL("bge_world_overlap_sphere")

int bge_world_sphere_penetration(bge_world* w, uint64_t n, const bge_sphere* spheres, bge_penetration_hit* hits)
try {
    static_assert(sizeof(bge_penetration_hit) == sizeof(bge_ray_hit), "the closest-hit records of every kind are 40 bytes");
    return query_closest(w, bge::QueryKind::SpherePenetration, n, sizeof(bge_sphere), spheres, hits);
}
BGE_CATCH_ALL("bge_world_sphere_penetration")

int bge_world_sphere_penetration_device(bge_world* w, uint64_t n, const void* spheres_device, void* hits_device)
try {
    if (n > 0 && ((reinterpret_cast<uintptr_t>(spheres_device) | reinterpret_cast<uintptr_t>(hits_device)) & 3u)) {
        return fail(BGE_ERR_INVALID, "spheres_device and hits_device must be 4-byte aligned");
    }
    return query_closest_device(w, bge::QueryKind::SpherePenetration, n, spheres_device, hits_device);
}
BGE_CATCH_ALL("bge_world_sphere_penetration_device")

int bge_world_sphere_recover(bge_world* w, uint64_t n, const bge_sphere_recover* records, bge_sphere_recover_result* results)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (n == 0) return BGE_OK;
    if (!records || !results) return fail(BGE_ERR_INVALID, "NULL argument");
    DeviceGuard guard(w->device);
    bge::QueryCall q;
    if (int rc = query_prepare(w, n, q)) return rc; // (before the staging is sized: it refuses a batch that is too large)
    HIP_TRY(w->recover_in.ensure(n * sizeof(bge_sphere_recover)));
    HIP_TRY(w->recover_out.ensure(n * sizeof(bge_sphere_recover_result)));
    HIP_TRY(hipMemcpyAsync(w->recover_in.p, records, n * sizeof(bge_sphere_recover), hipMemcpyHostToDevice, w->stream));
    if (int rc = recover_enqueue(w, q, n, w->recover_in.p, w->recover_out.p)) return rc;
    HIP_TRY(hipMemcpyAsync(results, w->recover_out.p, n * sizeof(bge_sphere_recover_result), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_sphere_recover")

int bge_world_sphere_recover_device(bge_world* w, uint64_t n, const void* records_device, void* results_device)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (n == 0) return BGE_OK;
    if (!records_device || !results_device) return fail(BGE_ERR_INVALID, "NULL argument");
    if ((reinterpret_cast<uintptr_t>(records_device) | reinterpret_cast<uintptr_t>(results_device)) & 3u) {
        return fail(BGE_ERR_INVALID, "records_device and results_device must be 4-byte aligned");
    }
    DeviceGuard guard(w->device);
    bge::QueryCall q;
    if (int rc = query_prepare(w, n, q)) return rc;
    return recover_enqueue(w, q, n, records_device, results_device);
}
BGE_CATCH_ALL("bge_world_sphere_recover_device")

// ---------------------------------------------------------------- characters (bge_character.hip)
static_assert(sizeof(bge_character_desc) == 48, "bge_character_desc is 48 bytes (include/bge_world.h)");
static_assert(sizeof(bge_character_input) == 16, "bge_character_input is 16 bytes (include/bge_world.h)");
static_assert(sizeof(bge_character_state) == 80, "bge_character_state is 80 bytes (include/bge_world.h)");

namespace {

void char_crowd_off(bge_world* w)
{
    w->char_crowd_on = false;
    w->char_crowd_max_push = 0.0f;
    for (DevBuf* b : {&w->char_crowd_hits, &w->char_crowd_group, &w->char_crowd_mask}) b->release();
}

void char_push_off(bge_world* w)
{
    w->char_push_on = false;
    w->char_push_desc = bge_character_push_desc{0u, 0.0f, 0.0f, 0u};
    w->char_push_records.release();
}

int check_character_range(const bge_world* w, uint64_t first, uint64_t count)
{
    if (first > w->n_characters || count > w->n_characters - first) {
        return fail(BGE_ERR_INVALID, "character range [%llu, +%llu) outside [0, %llu)", (unsigned long long)first, (unsigned long long)count,
                    (unsigned long long)w->n_characters);
    }
    return BGE_OK;
}

// What is wrong with a desc, or NULL
const char* character_desc_fault(const bge_character_desc& d)
{
    const float floats[] = {d.position[0], d.position[1], d.position[2], d.radius, d.skin, d.step_height, d.min_ground_ny, d.probe_distance,
                            d.gravity, d.jump_speed, d.fall_speed};
    for (float v : floats) {
        if (!std::isfinite(v)) return "a value is not finite";
    }
    if (!(d.radius >= 0.0f)) return "radius < 0";
    if (!(d.skin > 0.0f)) return "skin <= 0";
    if (!(d.step_height >= 0.0f)) return "step_height < 0";
    if (!(d.probe_distance >= 0.0f)) return "probe_distance < 0";
    if (!(d.gravity >= 0.0f)) return "gravity < 0";
    if (!(d.jump_speed >= 0.0f)) return "jump_speed < 0";
    if (!(d.fall_speed > 0.0f)) return "fall_speed <= 0";
    if (d.layer_mask == 0u) return "layer_mask == 0";
    return nullptr;
}

} // namespace

int bge_world_characters_create(bge_world* w, uint64_t n, const bge_character_desc* descs)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (n > 0 && !descs) return fail(BGE_ERR_INVALID, "descs is NULL");
    if (n > 0x3fffffffull) return fail(BGE_ERR_INVALID, "n = %llu: a character's step move asks 2 n casts per pass, at most 2^31 - 1", (unsigned long long)n);
    for (uint64_t i = 0; i < n; ++i) {
        if (const char* what = character_desc_fault(descs[i])) return fail(BGE_ERR_INVALID, "character desc %llu: %s", (unsigned long long)i, what);
    }
    DeviceGuard guard(w->device);
    HIP_TRY(hipStreamSynchronize(w->stream)); // (an update of the old set may still be running on its buffers)
    w->n_characters = 0;
    chartrig_off(w); // (the watch belongs to the set: its filters and bitmaps are per character)
    w->ride_on = false; // (and so do the ride records)
    w->ride_flags = 0;
    w->char_ride.release();
    char_crowd_off(w); // (and the crowd's filters and hit records)
    char_push_off(w);  // (and the push records)
    w->char_r_max = 0.0f;
    for (uint64_t i = 0; i < n; ++i) w->char_r_max = std::max(w->char_r_max, descs[i].radius);
    if (n == 0) {
        for (DevBuf* b : {&w->char_desc, &w->char_input, &w->char_state, &w->char_recover_in, &w->char_recover_out, &w->char_step_in, &w->char_step_out,
                          &w->char_scratch}) {
            b->release();
        }
        return BGE_OK;
    }
    HIP_TRY(w->char_desc.ensure(n * sizeof(bge_character_desc)));
    HIP_TRY(w->char_input.ensure(n * sizeof(bge_character_input)));
    HIP_TRY(w->char_state.ensure(n * sizeof(bge_character_state)));
    HIP_TRY(w->char_recover_in.ensure(n * sizeof(bge_sphere_recover)));
    HIP_TRY(w->char_recover_out.ensure(n * sizeof(bge_sphere_recover_result)));
    HIP_TRY(w->char_step_in.ensure(n * sizeof(bge_sphere_step_move)));
    HIP_TRY(w->char_step_out.ensure(n * sizeof(bge_sphere_step_result)));
    HIP_TRY(w->char_scratch.ensure(n * sizeof(uint2)));
    std::vector<bge_character_state> states(n);
    for (uint64_t i = 0; i < n; ++i) {
        bge_character_state& s = states[i];
        s = bge_character_state{};
        for (int a = 0; a < 3; ++a) s.position[a] = descs[i].position[a];
        s.ground_kind = s.hit_kind = BGE_RAY_MISS;
        s.ground_entity = s.hit_entity = BGE_RAY_NO_ENTITY;
    }
    HIP_TRY(hipMemcpyAsync(w->char_desc.p, descs, n * sizeof(bge_character_desc), hipMemcpyHostToDevice, w->stream));
    HIP_TRY(hipMemcpyAsync(w->char_state.p, states.data(), n * sizeof(bge_character_state), hipMemcpyHostToDevice, w->stream));
    HIP_TRY(hipMemsetAsync(w->char_input.p, 0, n * sizeof(bge_character_input), w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream)); // (the copies read the caller's and this function's memory)
    w->n_characters = n;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_characters_create")

int bge_world_characters_set_input(bge_world* w, uint64_t first, uint64_t count, const bge_character_input* inputs)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (int rc = check_character_range(w, first, count)) return rc;
    if (count == 0) return BGE_OK;
    if (!inputs) return fail(BGE_ERR_INVALID, "inputs is NULL");
    DeviceGuard guard(w->device);
    HIP_TRY(hipMemcpyAsync(w->char_input.as<bge_character_input>() + first, inputs, count * sizeof(bge_character_input), hipMemcpyHostToDevice,
                           w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream)); // (the caller's memory is free again on return)
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_characters_set_input")

int bge_world_characters_set_input_device(bge_world* w, uint64_t first, uint64_t count, const void* inputs_device)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (int rc = check_character_range(w, first, count)) return rc;
    if (count == 0) return BGE_OK;
    if (!inputs_device) return fail(BGE_ERR_INVALID, "inputs_device is NULL");
    if (reinterpret_cast<uintptr_t>(inputs_device) & 3u) return fail(BGE_ERR_INVALID, "inputs_device must be 4-byte aligned");
    DeviceGuard guard(w->device);
    HIP_TRY(hipMemcpyAsync(w->char_input.as<bge_character_input>() + first, inputs_device, count * sizeof(bge_character_input),
                           hipMemcpyDeviceToDevice, w->stream));
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_characters_set_input_device")

int bge_world_characters_warp(bge_world* w, uint64_t count, const uint32_t* index, const float* position3)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (count == 0) return BGE_OK;
    if (!index || !position3) return fail(BGE_ERR_INVALID, "NULL argument");
    for (uint64_t k = 0; k < count; ++k) {
        if (index[k] >= w->n_characters) {
            return fail(BGE_ERR_INVALID, "warp %llu: character %u outside [0, %llu)", (unsigned long long)k, index[k], (unsigned long long)w->n_characters);
        }
        for (int a = 0; a < 3; ++a) {
            if (!std::isfinite(position3[3 * k + a])) return fail(BGE_ERR_INVALID, "warp %llu: the position is not finite", (unsigned long long)k);
        }
    }
    DeviceGuard guard(w->device);
    // the first five words of a state: position, vertical_velocity, flags (everything but GROUNDED stays: they are the last step's)
    HIP_TRY(hipStreamSynchronize(w->stream));
    for (uint64_t k = 0; k < count; ++k) {
        char* s = w->char_state.as<char>() + uint64_t(index[k]) * sizeof(bge_character_state);
        uint32_t head[5];
        HIP_TRY(hipMemcpy(head, s, sizeof head, hipMemcpyDeviceToHost));
        std::memcpy(head, position3 + 3 * k, 12);
        head[3] = 0u; // vv = +0
        head[4] &= ~uint32_t(BGE_CHAR_GROUNDED);
        HIP_TRY(hipMemcpy(s, head, sizeof head, hipMemcpyHostToDevice));
    }
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_characters_warp")


// ---------------------------------------------------------------- crowd separation (bge_crowd.hip)
static_assert(sizeof(bge_crowd_sphere) == 24, "bge_crowd_sphere is 24 bytes (include/bge_world.h)");
static_assert(sizeof(bge_crowd_hit) == 32, "bge_crowd_hit is 32 bytes (include/bge_world.h)");

namespace {

constexpr uint64_t kCrowdGridMinDefault = 256; // the smallest measured size, and the grid path is ahead there

// Sizes the temporaries for n spheres (both paths: BGE_CROWD_GRID_MIN is read per call) and names them in p
int crowd_reserve(bge_world* w, uint64_t n, bge::CrowdParams& p)
{
    const uint32_t table = bge::crowd_table_size(n);
    if (w->crowd_scan_table != table) {
        w->crowd_scan_bytes = bge::crowd_scan_bytes(table);
        w->crowd_scan_table = table;
    }
    HIP_TRY(w->crowd_rec_a.ensure(n * 16));
    HIP_TRY(w->crowd_rec_b.ensure(n * 16));
    HIP_TRY(w->crowd_cell.ensure(n * 8));
    HIP_TRY(w->crowd_count.ensure(size_t(table) * 4));
    HIP_TRY(w->crowd_start.ensure(size_t(table) * 4));
    HIP_TRY(w->crowd_scan.ensure(std::max<size_t>(w->crowd_scan_bytes, 16)));
    HIP_TRY(w->crowd_rmax.ensure(4));
    p.rec_a = w->crowd_rec_a.p;
    p.rec_b = w->crowd_rec_b.p;
    p.cell = w->crowd_cell.as<uint32_t>();
    p.count = w->crowd_count.as<uint32_t>();
    p.start = w->crowd_start.as<uint32_t>();
    p.scan_tmp = w->crowd_scan.p;
    p.scan_bytes = w->crowd_scan_bytes;
    p.table = table;
    uint64_t grid_min = kCrowdGridMinDefault;
    if (const char* e = std::getenv("BGE_CROWD_GRID_MIN")) grid_min = std::strtoull(e, nullptr, 10);
    p.grid = n >= grid_min ? 1u : 0u;
    return BGE_OK;
}

int crowd_check_max_push(float max_push)
{
    if (!(std::isfinite(max_push) && max_push >= 0.0f)) return fail(BGE_ERR_INVALID, "max_push = %g: must be finite and >= 0", (double)max_push);
    return BGE_OK;
}

int crowd_query_enqueue(bge_world* w, uint64_t n, const void* spheres, float max_push, void* hits)
{
    bge::CrowdParams p{};
    if (int rc = crowd_reserve(w, n, p)) return rc;
    const uint32_t* s = static_cast<const uint32_t*>(spheres);
    p.src = bge::CrowdSource{s, s + 3, s + 4, s + 5, 6u, 6u, 6u, 6u};
    p.n = static_cast<uint32_t>(n);
    p.max_push = max_push;
    p.hits = hits;
    p.r_max_device = w->crowd_rmax.as<uint32_t>();
    HIP_TRY(bge::launch_crowd(w->stream, p));
    return BGE_OK;
}

// Separate of one step: the character set as the batch, the push applied to state.position
int char_crowd_params(bge_world* w, bge::CrowdParams& p)
{
    const uint64_t n = w->n_characters;
    if (int rc = crowd_reserve(w, n, p)) return rc; // (sized by bge_world_characters_crowd: nothing is allocated here)
    uint32_t* state = w->char_state.as<uint32_t>();
    p.src = bge::CrowdSource{state, w->char_desc.as<uint32_t>() + 3, w->char_crowd_group.as<uint32_t>(), w->char_crowd_mask.as<uint32_t>(),
                             20u, 12u, 1u, 1u};
    p.n = static_cast<uint32_t>(n);
    p.max_push = w->char_crowd_max_push;
    p.hits = w->char_crowd_hits.p;
    p.apply_position = state;
    p.r_max_host = w->char_r_max;
    return BGE_OK;
}

// ---- impulses (bge_impulse.hip)
static_assert(sizeof(bge_impulse) == 32, "bge_impulse is 32 bytes (include/bge_world.h)");
static_assert(sizeof(bge_character_push_desc) == 16, "bge_character_push_desc is 16 bytes (include/bge_world.h)");

// Sizes the sort's arrays for n records (grow-only: a call of no more records than one before allocates nothing) and names them in p
int impulse_reserve(bge_world* w, uint64_t n, bge::ImpulseParams& p)
{
    if (n > w->imp_cap) {
        const size_t bytes = bge::impulse::word_array_bytes(n);
        for (DevBuf* b : {&w->imp_keys[0], &w->imp_keys[1], &w->imp_vals[0], &w->imp_vals[1]}) HIP_TRY(b->ensure(bytes));
        w->imp_cap = n;
    }
    if (n != w->imp_sort_n) {
        w->imp_sort_need = bge::impulse_sort_bytes(static_cast<uint32_t>(n));
        w->imp_sort_n = n;
    }
    HIP_TRY(w->imp_sort.ensure(std::max<size_t>(w->imp_sort_need, 16)));
    p.keys_in = w->imp_keys[0].as<uint32_t>();
    p.keys_out = w->imp_keys[1].as<uint32_t>();
    p.vals_in = w->imp_vals[0].as<uint32_t>();
    p.vals_out = w->imp_vals[1].as<uint32_t>();
    p.sort_tmp = w->imp_sort.p;
    p.sort_bytes = w->imp_sort.bytes;
    return BGE_OK;
}

// Valid, Apply and Wake of n records that lie in device memory; the caller has moved the epochs on (epochs_edit)
int impulses_enqueue(bge_world* w, uint64_t n, const void* records, void* status)
{
    bge::ImpulseParams p{};
    if (int rc = impulse_reserve(w, n, p)) return rc;
    p.records = static_cast<const uint32_t*>(records);
    p.status = static_cast<uint32_t*>(status);
    p.n = static_cast<uint32_t>(n);
    p.n_entities = w->flat.n_entities;
    p.slot_of_entity = w->slot_of_entity.as<uint32_t>();
    HIP_TRY(bge::launch_impulses(w->stream, p, w->view));
    return BGE_OK;
}

int impulses_check(const bge_world* w, uint64_t n)
{
    if (!w->has_topology) return fail(BGE_ERR_STATE, "bge_world_set_topology has not been called");
    if (!bge::impulse::count_ok(n)) return fail(BGE_ERR_INVALID, "n = %llu: at most 2^30 - 1 impulse records", (unsigned long long)n);
    return BGE_OK;
}

} // namespace

int bge_world_characters_update(bge_world* w, float dt, uint32_t steps)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (!(std::isfinite(dt) && dt > 0.0f)) return fail(BGE_ERR_INVALID, "dt = %g: must be finite and > 0", (double)dt);
    if (steps < 1u) return fail(BGE_ERR_INVALID, "steps = 0: at least one step");
    const uint64_t n = w->n_characters;
    if (n == 0) return BGE_OK;
    DeviceGuard guard(w->device);
    // Push writes velocities, flags and deactivation records: the tick's per-wave words go, as for bge_world_set_velocities, and a
    // deferred translation row is made current BEFORE query_prepare captures how the queries read row 3
    if (w->char_push_on) w->epochs_edit();
    bge::QueryCall q;
    if (int rc = query_prepare(w, 2 * n, q)) return rc; // (the step move's 2 n casts per pass; the recovery asks n of them)
    bge::QueryCall qr = q;
    qr.n_queries = static_cast<uint32_t>(n);
    bge::CharacterParams c{};
    c.desc = w->char_desc.p;
    c.input = w->char_input.p;
    c.state = w->char_state.p;
    c.recover_in = w->char_recover_in.p;
    c.recover_out = w->char_recover_out.p;
    c.step_in = w->char_step_in.p;
    c.step_out = w->char_step_out.p;
    c.scratch = w->char_scratch.as<uint2>();
    c.dt = dt;
    c.n = static_cast<uint32_t>(n);
    bge::RideParams r{};
    if (w->ride_on) {
        r.state = w->char_state.p;
        r.ride = w->char_ride.p;
        r.n = c.n;
        r.dynamic = (w->ride_flags & BGE_CHAR_RIDE_DYNAMIC) ? 1u : 0u;
        r.n_entities = w->flat.n_entities;
        r.n_slots = q.n_slots;
        r.flags = q.flags;
        r.pos = q.pos;
        r.quat = q.quat;
        r.slot_of_entity = q.slot_of_entity;
        HIP_TRY(bge::launch_char_carry(w->stream, r));
    }
    bge::CrowdParams cp{};
    if (w->char_crowd_on) {
        if (int rc = char_crowd_params(w, cp)) return rc;
    }
    bge::CharPushParams pp{};
    if (w->char_push_on) {
        pp.state = w->char_state.as<uint32_t>();
        pp.records = w->char_push_records.as<uint32_t>();
        pp.n = c.n;
        pp.n_entities = w->flat.n_entities;
        pp.slot_of_entity = w->slot_of_entity.as<uint32_t>();
        pp.force = w->char_push_desc.force;
        pp.dt = dt;
        pp.max_normal_y = w->char_push_desc.max_normal_y;
        pp.body_mask = w->char_push_desc.body_mask;
    }
    for (uint32_t k = 0; k < steps; ++k) {
        if (w->char_crowd_on) {
            HIP_TRY(bge::launch_crowd(w->stream, cp)); // Separate
        }
        HIP_TRY(bge::launch_char_begin(w->stream, c, k == 0 ? 1u : 0u));
        if (int rc = recover_enqueue(w, qr, n, w->char_recover_in.p, w->char_recover_out.p)) return rc;
        HIP_TRY(bge::launch_char_move(w->stream, c));
        if (int rc = step_enqueue(w, q, n, w->char_step_in.p, w->char_step_out.p)) return rc;
        HIP_TRY(bge::launch_char_finish(w->stream, c));
        if (w->char_push_on) {
            HIP_TRY(bge::launch_char_push(w->stream, pp, w->view)); // Push
            if (int rc = impulses_enqueue(w, n, w->char_push_records.p, nullptr)) return rc; // (sized by bge_world_characters_push)
        }
    }
    if (w->ride_on) {
        HIP_TRY(bge::launch_char_anchor(w->stream, r));
    }
    if (w->ct_on) {
        if (int rc = chartrig_enqueue(w, q.n_ghosts)) return rc;
    }
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_characters_update")

int bge_world_characters_download(bge_world* w, uint64_t first, uint64_t count, bge_character_state* states)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (int rc = check_character_range(w, first, count)) return rc;
    if (count == 0) return BGE_OK;
    if (!states) return fail(BGE_ERR_INVALID, "states is NULL");
    DeviceGuard guard(w->device);
    HIP_TRY(hipMemcpyAsync(states, w->char_state.as<bge_character_state>() + first, count * sizeof(bge_character_state), hipMemcpyDeviceToHost,
                           w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_characters_download")

int bge_world_characters_state_device(bge_world* w, void** states_device, uint64_t* n)
try {
    if (!w || !states_device || !n) return fail(BGE_ERR_INVALID, "NULL argument");
    *states_device = w->n_characters ? w->char_state.p : nullptr;
    *n = w->n_characters;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_characters_state_device")

// ---------------------------------------------------------------- character platform riding (bge_ride.hip)
static_assert(sizeof(bge_character_ride) == 64, "bge_character_ride is 64 bytes (include/bge_world.h)");

int bge_world_characters_ride(bge_world* w, uint32_t flags)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (flags & ~uint32_t(BGE_CHAR_RIDE_ON | BGE_CHAR_RIDE_DYNAMIC)) return fail(BGE_ERR_INVALID, "flags = %#x: unknown bits", flags);
    if ((flags & BGE_CHAR_RIDE_DYNAMIC) && !(flags & BGE_CHAR_RIDE_ON)) return fail(BGE_ERR_INVALID, "BGE_CHAR_RIDE_DYNAMIC without BGE_CHAR_RIDE_ON");
    DeviceGuard guard(w->device);
    if (flags == 0u) {
        if (w->ride_on) {
            HIP_TRY(hipStreamSynchronize(w->stream)); // (an update may still be writing the records)
        }
        w->ride_on = false;
        w->ride_flags = 0;
        w->char_ride.release();
        return BGE_OK;
    }
    const uint64_t n = w->n_characters;
    if (n == 0) return fail(BGE_ERR_INVALID, "there is no character set to switch riding on for");
    if (!w->ride_on) {
        // no anchor: entity = BGE_RAY_NO_ENTITY, turn = (0, 0, 0, 1), every other word 0
        std::vector<bge_character_ride> fresh(n);
        for (bge_character_ride& r : fresh) {
            r = bge_character_ride{};
            r.entity = BGE_RAY_NO_ENTITY;
            r.turn[3] = 1.0f;
        }
        HIP_TRY(w->char_ride.ensure(n * sizeof(bge_character_ride)));
        HIP_TRY(hipMemcpyAsync(w->char_ride.p, fresh.data(), n * sizeof(bge_character_ride), hipMemcpyHostToDevice, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream)); // (the copy reads this function's memory)
        w->ride_on = true;
    }
    w->ride_flags = flags;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_characters_ride")

int bge_world_characters_rides(bge_world* w, uint64_t first, uint64_t count, bge_character_ride* out)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (int rc = check_character_range(w, first, count)) return rc;
    DeviceGuard guard(w->device);
    if (count == 0) {
        HIP_TRY(hipStreamSynchronize(w->stream));
        return BGE_OK;
    }
    if (!w->ride_on) return fail(BGE_ERR_INVALID, "character platform riding is off");
    if (!out) return fail(BGE_ERR_INVALID, "out is NULL");
    HIP_TRY(hipMemcpyAsync(out, w->char_ride.as<bge_character_ride>() + first, count * sizeof(bge_character_ride), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_characters_rides")

int bge_world_characters_rides_device(bge_world* w, void** rides, uint64_t* n)
try {
    if (!w || !rides || !n) return fail(BGE_ERR_INVALID, "NULL argument");
    *rides = w->ride_on ? w->char_ride.p : nullptr;
    *n = w->ride_on ? w->n_characters : 0;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_characters_rides_device")


// ---------------------------------------------------------------- crowd separation: the entry points (bge_crowd.hip)
int bge_world_crowd_query(bge_world* w, uint64_t n, const bge_crowd_sphere* spheres, float max_push, bge_crowd_hit* hits)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (int rc = crowd_check_max_push(max_push)) return rc;
    if (n == 0) return BGE_OK;
    if (!spheres || !hits) return fail(BGE_ERR_INVALID, "NULL argument");
    if (n > 0x3fffffffull) return fail(BGE_ERR_INVALID, "n = %llu: at most 2^30 - 1 spheres", (unsigned long long)n);
    DeviceGuard guard(w->device);
    HIP_TRY(w->crowd_in.ensure(n * sizeof(bge_crowd_sphere)));
    HIP_TRY(w->crowd_out.ensure(n * sizeof(bge_crowd_hit)));
    HIP_TRY(hipMemcpyAsync(w->crowd_in.p, spheres, n * sizeof(bge_crowd_sphere), hipMemcpyHostToDevice, w->stream));
    if (int rc = crowd_query_enqueue(w, n, w->crowd_in.p, max_push, w->crowd_out.p)) return rc;
    HIP_TRY(hipMemcpyAsync(hits, w->crowd_out.p, n * sizeof(bge_crowd_hit), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_crowd_query")

int bge_world_crowd_query_device(bge_world* w, uint64_t n, const void* spheres_device, float max_push, void* hits_device)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (int rc = crowd_check_max_push(max_push)) return rc;
    if (n == 0) return BGE_OK;
    if (!spheres_device || !hits_device) return fail(BGE_ERR_INVALID, "NULL argument");
    if ((reinterpret_cast<uintptr_t>(spheres_device) | reinterpret_cast<uintptr_t>(hits_device)) & 3u) {
        return fail(BGE_ERR_INVALID, "spheres_device and hits_device must be 4-byte aligned");
    }
    if (n > 0x3fffffffull) return fail(BGE_ERR_INVALID, "n = %llu: at most 2^30 - 1 spheres", (unsigned long long)n);
    DeviceGuard guard(w->device);
    return crowd_query_enqueue(w, n, spheres_device, max_push, hits_device);
}
BGE_CATCH_ALL("bge_world_crowd_query_device")

int bge_world_characters_crowd(bge_world* w, uint32_t flags, float max_push, uint64_t n, const uint32_t* group, const uint32_t* mask)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (flags & ~uint32_t(BGE_CHAR_CROWD_ON)) return fail(BGE_ERR_INVALID, "flags = %#x: unknown bits", flags);
    DeviceGuard guard(w->device);
    if (flags == 0u) {
        if (w->char_crowd_on) {
            HIP_TRY(hipStreamSynchronize(w->stream)); // (an update may still be writing the records)
        }
        char_crowd_off(w);
        return BGE_OK;
    }
    if (int rc = crowd_check_max_push(max_push)) return rc;
    if (w->n_characters == 0) return fail(BGE_ERR_INVALID, "there is no character set to switch the crowd on for");
    if (n != w->n_characters) {
        return fail(BGE_ERR_INVALID, "n = %llu, the set holds %llu characters", (unsigned long long)n, (unsigned long long)w->n_characters);
    }
    HIP_TRY(hipStreamSynchronize(w->stream)); // (an update may still be reading the filters)
    bge::CrowdParams sized{};
    if (int rc = crowd_reserve(w, n, sized)) return rc;
    HIP_TRY(w->char_crowd_group.ensure(n * 4));
    HIP_TRY(w->char_crowd_mask.ensure(n * 4));
    const std::vector<uint32_t> ones(group ? 0 : n, 1u), all(mask ? 0 : n, 0xffffffffu);
    HIP_TRY(hipMemcpyAsync(w->char_crowd_group.p, group ? group : ones.data(), n * 4, hipMemcpyHostToDevice, w->stream));
    HIP_TRY(hipMemcpyAsync(w->char_crowd_mask.p, mask ? mask : all.data(), n * 4, hipMemcpyHostToDevice, w->stream));
    if (!w->char_crowd_on) {
        HIP_TRY(w->char_crowd_hits.ensure(n * sizeof(bge_crowd_hit)));
        HIP_TRY(hipMemsetAsync(w->char_crowd_hits.p, 0, n * sizeof(bge_crowd_hit), w->stream));
    }
    HIP_TRY(hipStreamSynchronize(w->stream)); // (the copies read the caller's and this function's memory)
    w->char_crowd_on = true;
    w->char_crowd_max_push = max_push;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_characters_crowd")

int bge_world_characters_crowd_hits(bge_world* w, uint64_t first, uint64_t count, bge_crowd_hit* out)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (int rc = check_character_range(w, first, count)) return rc;
    DeviceGuard guard(w->device);
    if (count == 0) {
        HIP_TRY(hipStreamSynchronize(w->stream));
        return BGE_OK;
    }
    if (!w->char_crowd_on) return fail(BGE_ERR_INVALID, "the character crowd is off");
    if (!out) return fail(BGE_ERR_INVALID, "out is NULL");
    HIP_TRY(hipMemcpyAsync(out, w->char_crowd_hits.as<bge_crowd_hit>() + first, count * sizeof(bge_crowd_hit), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_characters_crowd_hits")

int bge_world_characters_crowd_hits_device(bge_world* w, void** hits, uint64_t* n)
try {
    if (!w || !hits || !n) return fail(BGE_ERR_INVALID, "NULL argument");
    *hits = w->char_crowd_on ? w->char_crowd_hits.p : nullptr;
    *n = w->char_crowd_on ? w->n_characters : 0;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_characters_crowd_hits_device")

// ---------------------------------------------------------------- impulses and the characters' push: the entry points (bge_impulse.hip)
int bge_world_apply_impulses(bge_world* w, uint64_t n, const bge_impulse* records, uint32_t* status)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (n == 0) return BGE_OK;
    if (!records) return fail(BGE_ERR_INVALID, "records is NULL");
    if (int rc = impulses_check(w, n)) return rc;
    DeviceGuard guard(w->device);
    HIP_TRY(w->imp_in.ensure(bge::impulse::record_bytes(n)));
    if (status) HIP_TRY(w->imp_status.ensure(bge::impulse::word_array_bytes(n)));
    HIP_TRY(hipMemcpyAsync(w->imp_in.p, records, bge::impulse::record_bytes(n), hipMemcpyHostToDevice, w->stream));
    w->epochs_edit();
    // from here on a copy from or to the caller's memory may be in flight: no return before the stream has passed it
    int rc = impulses_enqueue(w, n, w->imp_in.p, status ? w->imp_status.p : nullptr);
    hipError_t copied = hipSuccess;
    if (rc == BGE_OK && status) copied = hipMemcpyAsync(status, w->imp_status.p, bge::impulse::word_array_bytes(n), hipMemcpyDeviceToHost, w->stream);
    const hipError_t synced = hipStreamSynchronize(w->stream);
    if (rc != BGE_OK) return rc;
    HIP_TRY(copied);
    HIP_TRY(synced);
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_apply_impulses")

int bge_world_apply_impulses_device(bge_world* w, uint64_t n, const void* records_device, void* status_device)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (n == 0) return BGE_OK;
    if (!records_device) return fail(BGE_ERR_INVALID, "records_device is NULL");
    if ((reinterpret_cast<uintptr_t>(records_device) | reinterpret_cast<uintptr_t>(status_device)) & 3u) {
        return fail(BGE_ERR_INVALID, "records_device and status_device must be 4-byte aligned");
    }
    if (int rc = impulses_check(w, n)) return rc;
    DeviceGuard guard(w->device);
    w->epochs_edit();
    return impulses_enqueue(w, n, records_device, status_device);
}
BGE_CATCH_ALL("bge_world_apply_impulses_device")

int bge_world_characters_push(bge_world* w, const bge_character_push_desc* desc)
try {
    if (!w || !desc) return fail(BGE_ERR_INVALID, "NULL argument");
    if (desc->flags & ~uint32_t(BGE_CHAR_PUSH_ON)) return fail(BGE_ERR_INVALID, "bge_character_push_desc::flags = %#x: unknown bits", desc->flags);
    DeviceGuard guard(w->device);
    if (desc->flags == 0u) {
        if (w->char_push_on) {
            HIP_TRY(hipStreamSynchronize(w->stream)); // (an update may still be writing the records)
        }
        char_push_off(w);
        return BGE_OK;
    }
    switch (bge::impulse::push_desc_error(desc->flags, desc->force, desc->max_normal_y)) {
    case 0: break;
    case 2: return fail(BGE_ERR_INVALID, "bge_character_push_desc::force = %g: must be finite and >= 0", (double)desc->force);
    default: return fail(BGE_ERR_INVALID, "bge_character_push_desc::max_normal_y = %g: must be finite and in [0, 1)", (double)desc->max_normal_y);
    }
    const uint64_t n = w->n_characters;
    if (n == 0) return fail(BGE_ERR_INVALID, "there is no character set to switch push on for");
    HIP_TRY(hipStreamSynchronize(w->stream)); // (an update may still be running with the old desc's buffers)
    bge::ImpulseParams sized{};
    if (int rc = impulse_reserve(w, n, sized)) return rc;
    if (!w->char_push_on) {
        // no push yet: entity = BGE_RAY_NO_ENTITY, every other word 0
        std::vector<bge_impulse> fresh(n);
        for (bge_impulse& r : fresh) {
            r = bge_impulse{};
            r.entity = BGE_RAY_NO_ENTITY;
        }
        HIP_TRY(w->char_push_records.ensure(n * sizeof(bge_impulse)));
        HIP_TRY(hipMemcpyAsync(w->char_push_records.p, fresh.data(), n * sizeof(bge_impulse), hipMemcpyHostToDevice, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream)); // (the copy reads this function's memory)
    }
    w->char_push_on = true;
    w->char_push_desc = *desc;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_characters_push")

int bge_world_characters_push_records(bge_world* w, uint64_t first, uint64_t count, bge_impulse* out)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (int rc = check_character_range(w, first, count)) return rc;
    DeviceGuard guard(w->device);
    if (count == 0) {
        HIP_TRY(hipStreamSynchronize(w->stream));
        return BGE_OK;
    }
    if (!w->char_push_on) return fail(BGE_ERR_INVALID, "the character push is off");
    if (!out) return fail(BGE_ERR_INVALID, "out is NULL");
    HIP_TRY(hipMemcpyAsync(out, w->char_push_records.as<bge_impulse>() + first, count * sizeof(bge_impulse), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_characters_push_records")

int bge_world_characters_push_records_device(bge_world* w, void** records, uint64_t* n)
try {
    if (!w || !records || !n) return fail(BGE_ERR_INVALID, "NULL argument");
    *records = w->char_push_on ? w->char_push_records.p : nullptr;
    *n = w->char_push_on ? w->n_characters : 0;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_characters_push_records_device")

// ---------------------------------------------------------------- character trigger events (bge_chartrig.hip)
static_assert(sizeof(bge_character_trigger_event) == 12, "bge_character_trigger_event is 12 bytes (include/bge_world.h)");

int bge_world_characters_watch_triggers(bge_world* w, uint64_t n, const uint32_t* group, const uint32_t* mask, uint32_t flags,
                                        uint64_t event_capacity)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (flags & ~uint32_t(BGE_CHAR_TRIGGER_STAY_EVENTS)) return fail(BGE_ERR_INVALID, "flags = 0x%x: unknown bits", flags);
    if (n != 0 && n != w->n_characters) {
        return fail(BGE_ERR_INVALID, "n = %llu, the set holds %llu characters", (unsigned long long)n, (unsigned long long)w->n_characters);
    }
    DeviceGuard guard(w->device);
    if (n == 0) {
        HIP_TRY(hipStreamSynchronize(w->stream));
        chartrig_off(w);
        return BGE_OK;
    }
    const uint64_t rows = w->triggers.size();
    if (const char* what = chartrig_bound_fault(rows, n)) return fail(BGE_ERR_UNSUPPORTED, "character trigger events: %s", what);
    const uint64_t cap = event_capacity ? event_capacity : n + 1024u;
    if (w->ct_on) {
        if (int rc = chartrig_settle(w, cap, nullptr)) return rc; // (the remembered sets and the list stay; the list only grows)
    } else {
        HIP_TRY(hipStreamSynchronize(w->stream));
        w->ct_words = (n + 63u) / 64u;
        const uint64_t bytes = std::max<uint64_t>(rows * w->ct_words * 8, 8);
        HIP_TRY(w->ct_group.ensure(n * 4));
        HIP_TRY(w->ct_mask.ensure(n * 4));
        HIP_TRY(w->ct_bits[0].ensure(bytes));
        HIP_TRY(w->ct_bits[1].ensure(bytes));
        HIP_TRY(w->ct_events.ensure(cap * sizeof(bge_character_trigger_event)));
        HIP_TRY(w->ct_count.ensure(64));
        if (int rc = chartrig_size_rows(w, rows)) return rc;
        HIP_TRY(hipMemsetAsync(w->ct_bits[0].p, 0, bytes, w->stream));
        HIP_TRY(hipMemsetAsync(w->ct_bits[1].p, 0, bytes, w->stream));
        HIP_TRY(hipMemsetAsync(w->ct_count.p, 0, 64, w->stream));
        w->ct_rows = rows;
        w->ct_cap = cap;
        w->ct_rem = 0;
        w->ct_last_ghosts = 0;
    }
    std::vector<uint32_t> g(n, 2u), m(n, 0xffffffffu); // kDefaultCharacterLayer, mask all (PhysicsSystem.cpp:763)
    if (group) std::memcpy(g.data(), group, n * 4);
    if (mask) std::memcpy(m.data(), mask, n * 4);
    HIP_TRY(hipMemcpyAsync(w->ct_group.p, g.data(), n * 4, hipMemcpyHostToDevice, w->stream));
    HIP_TRY(hipMemcpyAsync(w->ct_mask.p, m.data(), n * 4, hipMemcpyHostToDevice, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream)); // (the vectors die here)
    w->ct_flags = flags;
    w->ct_on = true;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_characters_watch_triggers")

int bge_world_characters_trigger_events(bge_world* w, bge_character_trigger_event* out, uint64_t cap, uint64_t* total)
try {
    if (!w || !total) return fail(BGE_ERR_INVALID, "NULL argument");
    *total = 0;
    if (!w->ct_on) return BGE_OK;
    DeviceGuard guard(w->device);
    uint32_t count = 0;
    if (int rc = chartrig_settle(w, 0, &count)) return rc;
    *total = count;
    const uint64_t take = out ? std::min<uint64_t>(cap, count) : 0;
    if (take) HIP_TRY(hipMemcpy(out, w->ct_events.p, take * sizeof(bge_character_trigger_event), hipMemcpyDeviceToHost));
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_characters_trigger_events")

int bge_world_characters_trigger_events_device(bge_world* w, void** events, void** count, uint64_t* capacity)
try {
    if (!w || !events || !count || !capacity) return fail(BGE_ERR_INVALID, "NULL argument");
    *events = w->ct_on ? w->ct_events.p : nullptr;
    *count = w->ct_on ? w->ct_count.p : nullptr;
    *capacity = w->ct_on ? w->ct_cap : 0;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_characters_trigger_events_device")

int bge_world_characters_trigger_overlaps(bge_world* w, uint64_t cap, uint32_t* pairs2, uint64_t* total)
try {
    if (!w || !total) return fail(BGE_ERR_INVALID, "NULL argument");
    *total = 0;
    if (!w->ct_on || w->ct_rows == 0) return BGE_OK;
    DeviceGuard guard(w->device);
    std::vector<uint64_t> bits(w->ct_rows * w->ct_words);
    HIP_TRY(hipStreamSynchronize(w->stream));
    HIP_TRY(hipMemcpy(bits.data(), w->ct_bits[w->ct_rem].p, bits.size() * 8, hipMemcpyDeviceToHost));
    uint64_t k = 0;
    for (uint64_t r = 0; r < w->ct_rows; ++r) {
        for (uint64_t wd = 0; wd < w->ct_words; ++wd) {
            for (uint64_t word = bits[r * w->ct_words + wd]; word; word &= word - 1) {
                if (pairs2 && k < cap) {
                    pairs2[2 * k] = w->triggers[r].entity;
                    pairs2[2 * k + 1] = static_cast<uint32_t>(64 * wd + static_cast<uint64_t>(__builtin_ctzll(word)));
                }
                ++k;
            }
        }
    }
    *total = k;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_characters_trigger_overlaps")

int bge_world_characters_set_trigger_overlaps(bge_world* w, uint64_t count, const uint32_t* pairs2)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (count && !pairs2) return fail(BGE_ERR_INVALID, "pairs2 is NULL");
    const uint64_t n = w->ct_on ? w->n_characters : 0;
    std::vector<uint64_t> bits(w->ct_on ? w->ct_rows * w->ct_words : 0, 0);
    for (uint64_t k = 0; k < count; ++k) {
        const uint32_t e = pairs2[2 * k], c = pairs2[2 * k + 1];
        auto it = w->trig_index_of_entity.find(e);
        if (it == w->trig_index_of_entity.end()) return fail(BGE_ERR_INVALID, "pair %llu: entity %u carries no trigger", (unsigned long long)k, e);
        if (c >= n) return fail(BGE_ERR_INVALID, "pair %llu: character %u outside [0, %llu)", (unsigned long long)k, c, (unsigned long long)n);
        bits[uint64_t(it->second) * w->ct_words + (c >> 6)] |= 1ull << (c & 63u);
    }
    if (!w->ct_on) return BGE_OK;
    DeviceGuard guard(w->device);
    if (int rc = chartrig_settle(w, 0, nullptr)) return rc; // (the last call's list is whole before its bitmap goes)
    if (!bits.empty()) HIP_TRY(hipMemcpy(w->ct_bits[w->ct_rem].p, bits.data(), bits.size() * 8, hipMemcpyHostToDevice));
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_characters_set_trigger_overlaps")

int bge_world_trigger_boxes(bge_world* w, uint64_t count, const uint32_t* entity_index, float* aabb6, uint8_t* listed)
try {
    if (!w || (count && !entity_index)) return fail(BGE_ERR_INVALID, "NULL argument");
    if (count == 0) return BGE_OK;
    DeviceGuard guard(w->device);
    HIP_TRY(hipStreamSynchronize(w->stream));
    std::vector<float> boxes;
    const bool on_device = w->trig_list_on_device && w->trig_pose.p && w->trig_aabb.p && !w->triggers.empty();
    if (on_device) {
        boxes.resize(6 * w->triggers.size());
        HIP_TRY(hipMemcpy(boxes.data(), w->trig_aabb.p, boxes.size() * 4, hipMemcpyDeviceToHost));
    }
    for (uint64_t k = 0; k < count; ++k) {
        bool is_listed = false;
        auto it = w->trig_index_of_entity.find(entity_index[k]);
        if (on_device && it != w->trig_index_of_entity.end()) { // the rule of sync_query_ghosts
            const bge_world::Trigger& t = w->triggers[it->second];
            is_listed = t.runtime_active && (t.posed || t.frozen);
        }
        if (listed) listed[k] = is_listed ? 1 : 0;
        if (aabb6) {
            for (int a = 0; a < 6; ++a) aabb6[6 * k + a] = is_listed ? boxes[6 * it->second + a] : (a < 3 ? INFINITY : -INFINITY);
        }
    }
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_trigger_boxes")

// ---------------------------------------------------------------- debug overlay (bge_debug.hip)
static_assert(sizeof(bge_debug_line) == 28, "bge_debug_line is 28 bytes (include/bge_world.h)");

namespace {

constexpr uint64_t kDebugMaxLines = 0xffffffffull;

// Enqueues the whole query: *total_device = lines of the state as it is, lines_device[0 .. min(cap, total)) written.
int debug_enqueue(bge_world* w, const bge_debug_desc* desc, void* lines_device, uint64_t cap, void* total_device)
{
    if (!w->has_topology) return fail(BGE_ERR_STATE, "bge_world_set_topology has not been called");
    bge::DebugParams p{};
    p.flags = BGE_DEBUG_ALL;
    if (desc) {
        if (desc->struct_size < sizeof(bge_debug_desc)) return fail(BGE_ERR_INVALID, "bge_debug_desc::struct_size = %u", desc->struct_size);
        if (desc->flags & ~static_cast<uint32_t>(BGE_DEBUG_ALL)) return fail(BGE_ERR_INVALID, "bge_debug_desc::flags = 0x%x", desc->flags);
        p.flags = desc->flags;
        p.use_region = desc->use_region ? 1u : 0u;
        for (int a = 0; a < 3; ++a) {
            p.region_min[a] = desc->region_min[a];
            p.region_max[a] = desc->region_max[a];
        }
    }
    if (cap && !lines_device) return fail(BGE_ERR_INVALID, "lines is NULL");
    if (reinterpret_cast<uintptr_t>(lines_device) & 3u) return fail(BGE_ERR_INVALID, "lines must be 4-byte aligned");
    if (int rc = sync_query_ghosts(w)) return rc;
    const bge::WorldView& v = w->view;
    p.n_entities = w->flat.n_entities;
    p.n_slots = w->flat.n_slots;
    p.slot_of_entity = w->slot_of_entity.as<uint32_t>();
    p.flag_words = v.flags;
    p.pos = v.pos;
    p.quat = v.quat;
    p.cshape = v.cshape;
    p.cinfo = v.cinfo;
    p.ghosts = w->query_ghosts.as<bge::QueryGhost>();
    p.n_ghosts = static_cast<uint32_t>(w->query_ghosts_dev.size());
    p.ghost_pose = w->trig_pose.as<float>();
    p.plane = w->ground_plane ? 1u : 0u;
    if (p.flags & BGE_DEBUG_SHAPES) {
        const uint64_t items = bge::debug_items(p.n_entities, p.n_ghosts);
        const uint64_t blocks = (items + bge::kDebugItemsPerBlock - 1) / bge::kDebugItemsPerBlock;
        if (blocks > 0x7fffffffull) return fail(BGE_ERR_UNSUPPORTED, "debug overlay: %llu items", (unsigned long long)items);
        p.n_blocks = static_cast<uint32_t>(blocks);
        HIP_TRY(w->dbg_block_sum.ensure(blocks * 4));
        HIP_TRY(w->dbg_block_off.ensure(blocks * 8));
        p.block_sum = w->dbg_block_sum.as<uint32_t>();
        p.block_off = w->dbg_block_off.as<uint64_t>();
    }
    if (p.flags & BGE_DEBUG_CONTACTS) {
        // what bge_world_download_contacts / _box_contacts / _dynamic_pairs report while their switch is on
        if (w->ground_plane && w->manifold.p) p.manifold = v.manifold;
        if (w->static_contacts && w->bmanifold.p) p.bmanifold = v.bmanifold;
        if (w->dynamic_contacts && w->isl_n_prev) {
            const int at = w->isl_cur ^ 1; // (island_substep flipped the generations)
            p.pair_keys = w->isl_keys[at].as<uint64_t>();
            p.pair_man = w->isl_man[at].as<uint32_t>();
            p.n_pairs = w->isl_n_prev;
        }
    }
    p.lines = static_cast<float*>(lines_device);
    p.cap = cap;
    p.total = static_cast<unsigned long long*>(total_device);
    HIP_TRY(bge::launch_debug_lines(w->stream, p));
    return BGE_OK;
}

// the count alone (nothing is written anywhere but the world's own counter); synchronises
int debug_count(bge_world* w, const bge_debug_desc* desc, uint64_t* total)
{
    HIP_TRY(w->dbg_total.ensure(8));
    if (int rc = debug_enqueue(w, desc, nullptr, 0, w->dbg_total.p)) return rc;
    HIP_TRY(hipMemcpyAsync(total, w->dbg_total.p, 8, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return BGE_OK;
}

} // namespace

int bge_world_debug_lines(bge_world* w, const bge_debug_desc* desc, bge_debug_line* lines, uint64_t cap, uint64_t* total)
try {
    if (!w || !total) return fail(BGE_ERR_INVALID, "NULL argument");
    *total = 0;
    DeviceGuard guard(w->device);
    uint64_t n = 0;
    if (int rc = debug_count(w, desc, &n)) return rc;
    if (n > kDebugMaxLines) return fail(BGE_ERR_UNSUPPORTED, "debug overlay: %llu lines, at most 2^32 - 1", (unsigned long long)n);
    *total = n;
    if (!lines || n == 0) return BGE_OK;
    if (cap < n) return fail(BGE_ERR_INVALID, "debug_lines: %llu lines, room for %llu", (unsigned long long)n, (unsigned long long)cap);
    HIP_TRY(w->dbg_lines.ensure(n * sizeof(bge_debug_line)));
    if (int rc = debug_enqueue(w, desc, w->dbg_lines.p, n, w->dbg_total.p)) return rc;
    HIP_TRY(hipMemcpyAsync(lines, w->dbg_lines.p, n * sizeof(bge_debug_line), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_debug_lines")

int bge_world_debug_lines_device(bge_world* w, const bge_debug_desc* desc, void* lines_device, uint64_t cap, void* total_device)
try {
    if (!w || !total_device) return fail(BGE_ERR_INVALID, "NULL argument");
    DeviceGuard guard(w->device);
    // a world whose line count could pass 2^32 - 1 is counted first (one synchronisation), so that nothing is written when it does
    const uint64_t most = bge::kDebugPlaneLines + (bge::kDebugCapsuleLines + 4ull + 4ull * bge::kBoxManifolds) * (w->flat.n_entities + w->triggers.size()) +
                    4ull * w->isl_n_prev;
    if (most > kDebugMaxLines) {
        uint64_t n = 0;
        if (int rc = debug_count(w, desc, &n)) return rc;
        if (n > kDebugMaxLines) return fail(BGE_ERR_UNSUPPORTED, "debug overlay: %llu lines, at most 2^32 - 1", (unsigned long long)n);
    }
    return debug_enqueue(w, desc, lines_device, cap, total_device);
}
BGE_CATCH_ALL("bge_world_debug_lines_device")

// ---------------------------------------------------------------- frustum culling (bge_cull.hip)
static_assert(sizeof(bge_cull_desc) == 8 + 4 * 4 * BGE_CULL_MAX_PLANES, "bge_cull_desc layout (include/bge_world.h)");
static_assert(BGE_CULL_MAX_PLANES == bge::kCullMaxPlanes, "plane limit");

namespace {

int upload_bounds(bge_world* w, const Entities& e, const float* center3, const float* half3)
{
    const uint64_t count = e.count;
    return with_entities(
        w, e,
        [&]() -> int {
            if (!center3 || !half3) return fail(BGE_ERR_INVALID, "center3 / half3 is NULL");
            if (count == 0) return kNothingToDo;
            return w->bounds.first_use(w->flat.n_entities, w->stream); // (before the list is staged)
        },
        [&](const uint32_t* di) -> int {
            HIP_TRY(w->stage.ensure(count * 24));
            float* sc = w->stage.as<float>();
            HIP_TRY(hipMemcpyAsync(sc, center3, count * 12, hipMemcpyHostToDevice, w->stream));
            HIP_TRY(hipMemcpyAsync(sc + 3 * count, half3, count * 12, hipMemcpyHostToDevice, w->stream));
            HIP_TRY(bge::launch_cull_scatter_bounds(w->stream, di, e.first, count, sc, sc + 3 * count, w->bounds.as<float>()));
            HIP_TRY(hipStreamSynchronize(w->stream)); // the staging buffers are reused by the next call
            return BGE_OK;
        });
}

// Everything of the pass but its outputs: the desc, the world's arrays, the scratch of the three kernels
int cull_params(bge_world* w, const bge_cull_desc* desc, bool want_normal, bge::CullParams& p)
{
    if (!w->has_topology) return fail(BGE_ERR_STATE, "bge_world_set_topology has not been called");
    if (desc) {
        if (desc->struct_size < sizeof(bge_cull_desc)) return fail(BGE_ERR_INVALID, "bge_cull_desc::struct_size = %u", desc->struct_size);
        if (desc->n_planes > BGE_CULL_MAX_PLANES) return fail(BGE_ERR_INVALID, "bge_cull_desc::n_planes = %u, at most %d", desc->n_planes, BGE_CULL_MAX_PLANES);
        p.n_planes = desc->n_planes;
        std::memcpy(p.planes, desc->planes, sizeof p.planes);
    }
    p.n_entities = w->flat.n_entities;
    p.n_slots = w->flat.n_slots;
    if (p.n_entities > 0xffffffffull) return fail(BGE_ERR_UNSUPPORTED, "visible: %llu entities, at most 2^32 - 1 records", (unsigned long long)p.n_entities);
    if (want_normal) {
        if (!w->normal.p) return fail(BGE_ERR_STATE, "no tick with BGE_TICK_NORMAL_MATRICES has run");
        if (w->normal.bytes < p.n_slots * 64) return fail(BGE_ERR_STATE, "no tick with BGE_TICK_NORMAL_MATRICES has run since the world grew");
        p.normal = w->normal.as<float>();
    }
    p.slot_of_entity = w->slot_of_entity.as<uint32_t>();
    p.flag_words = w->view.flags;
    p.bounds = w->bounds.as<float>();
    p.world = w->view.world;
    p.row3 = w->row3_view();
    const uint64_t blocks = (p.n_entities + bge::kCullEntitiesPerBlock - 1) / bge::kCullEntitiesPerBlock;
    p.n_blocks = static_cast<uint32_t>(blocks);
    HIP_TRY(w->cull_ballots.ensure(std::max<uint64_t>(blocks, 1) * (bge::kCullEntitiesPerBlock / 64) * 8));
    HIP_TRY(w->cull_block_sum.ensure(std::max<uint64_t>(blocks, 1) * 4));
    HIP_TRY(w->cull_block_off.ensure(std::max<uint64_t>(blocks, 1) * 8));
    p.ballots = w->cull_ballots.as<unsigned long long>();
    p.block_sum = w->cull_block_sum.as<uint32_t>();
    p.block_off = w->cull_block_off.as<uint64_t>();
    return BGE_OK;
}

} // namespace

int bge_world_upload_bounds(bge_world* w, uint64_t first, uint64_t count, const float* center3, const float* half3)
try {
    return upload_bounds(w, Entities::range(first, count), center3, half3);
}
BGE_CATCH_ALL("bge_world_upload_bounds")

int bge_world_upload_bounds_indexed(bge_world* w, uint64_t count, const uint32_t* entity_index, const float* center3, const float* half3)
try {
    return upload_bounds(w, Entities::list(count, entity_index), center3, half3);
}
BGE_CATCH_ALL("bge_world_upload_bounds_indexed")

int bge_world_visible(bge_world* w, const bge_cull_desc* desc, uint32_t* entities, float* world16, float* normal16, uint64_t cap,
                      uint64_t* total)
try {
    if (!w || !total) return fail(BGE_ERR_INVALID, "NULL argument");
    *total = 0;
    DeviceGuard guard(w->device);
    bge::CullParams p{};
    if (int rc = cull_params(w, desc, normal16 != nullptr, p)) return rc;
    HIP_TRY(w->cull_total.ensure(8));
    p.total = w->cull_total.as<unsigned long long>();
    HIP_TRY(bge::launch_cull_count(w->stream, p));
    uint64_t n = 0;
    HIP_TRY(hipMemcpyAsync(&n, w->cull_total.p, 8, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    *total = n;
    if ((!entities && !world16 && !normal16) || n == 0) return BGE_OK;
    if (cap < n) return fail(BGE_ERR_INVALID, "visible: %llu records, room for %llu", (unsigned long long)n, (unsigned long long)cap);
    // the records are emitted from the ballots the count left (nothing ran in between) into one buffer: indices | world | normal
    const uint64_t idx_bytes = (n * 4 + 15) & ~15ull;
    HIP_TRY(w->cull_out.ensure(idx_bytes + n * 64 * ((world16 ? 1 : 0) + (normal16 ? 1 : 0))));
    char* out = w->cull_out.as<char>();
    p.out_entities = entities ? reinterpret_cast<uint32_t*>(out) : nullptr;
    p.out_world = world16 ? reinterpret_cast<float*>(out + idx_bytes) : nullptr;
    p.out_normal = normal16 ? reinterpret_cast<float*>(out + idx_bytes + (world16 ? n * 64 : 0)) : nullptr;
    p.cap = n;
    HIP_TRY(bge::launch_cull_emit(w->stream, p));
    if (entities) HIP_TRY(hipMemcpyAsync(entities, p.out_entities, n * 4, hipMemcpyDeviceToHost, w->stream));
    if (world16) HIP_TRY(hipMemcpyAsync(world16, p.out_world, n * 64, hipMemcpyDeviceToHost, w->stream));
    if (normal16) HIP_TRY(hipMemcpyAsync(normal16, p.out_normal, n * 64, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_visible")

int bge_world_visible_device(bge_world* w, const bge_cull_desc* desc, void* entities_device, void* world16_device, void* normal16_device,
                             uint64_t cap, void* total_device)
try {
    if (!w || !total_device) return fail(BGE_ERR_INVALID, "NULL argument");
    if (reinterpret_cast<uintptr_t>(entities_device) & 3u) return fail(BGE_ERR_INVALID, "entities must be 4-byte aligned");
    if ((reinterpret_cast<uintptr_t>(world16_device) | reinterpret_cast<uintptr_t>(normal16_device)) & 15u) {
        return fail(BGE_ERR_INVALID, "world16 / normal16 must be 16-byte aligned");
    }
    if (reinterpret_cast<uintptr_t>(total_device) & 7u) return fail(BGE_ERR_INVALID, "total must be 8-byte aligned");
    DeviceGuard guard(w->device);
    bge::CullParams p{};
    if (int rc = cull_params(w, desc, normal16_device != nullptr, p)) return rc;
    p.out_entities = static_cast<uint32_t*>(entities_device);
    p.out_world = static_cast<float*>(world16_device);
    p.out_normal = static_cast<float*>(normal16_device);
    p.cap = cap;
    p.total = static_cast<unsigned long long*>(total_device);
    HIP_TRY(bge::launch_cull_count(w->stream, p));
    HIP_TRY(bge::launch_cull_emit(w->stream, p));
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_visible_device")

// ---------------------------------------------------------------- draw batches (bge_batch.hip)
static_assert(sizeof(bge_draw_batch) == 8, "bge_draw_batch layout (include/bge_world.h)");
static_assert(BGE_DRAW_MAX_KEYS == bge::kBatchMaxKeys, "key limit");

namespace {

int upload_draw_keys(bge_world* w, const Entities& e, const uint32_t* key)
{
    return with_entities(
        w, e,
        [&]() -> int {
            if (!key) return fail(BGE_ERR_INVALID, "key is NULL");
            return e.count ? BGE_OK : kNothingToDo;
        },
        [&](const uint32_t* di) -> int {
            if (int rc = w->draw_keys.first_use(w->flat.n_entities, w->stream)) return rc; // (after the list is staged)
            HIP_TRY(w->stage.ensure(e.count * 4));
            HIP_TRY(hipMemcpyAsync(w->stage.p, key, e.count * 4, hipMemcpyHostToDevice, w->stream));
            HIP_TRY(bge::launch_batch_scatter_keys(w->stream, di, e.first, e.count, w->stage.as<uint32_t>(), w->draw_keys.as<uint32_t>()));
            HIP_TRY(hipStreamSynchronize(w->stream)); // the staging buffers are reused by the next call
            return BGE_OK;
        });
}

// cull_params plus the keys and the sort's scratch
int batch_params(bge_world* w, const bge_cull_desc* desc, uint32_t n_keys, bool want_normal, bge::BatchParams& p)
{
    if (n_keys == 0 || n_keys > BGE_DRAW_MAX_KEYS) return fail(BGE_ERR_INVALID, "n_keys = %u outside [1, %u]", n_keys, BGE_DRAW_MAX_KEYS);
    if (int rc = cull_params(w, desc, want_normal, p.cull)) return rc;
    p.key = w->draw_keys.as<uint32_t>();
    p.n_keys = n_keys;
    const uint64_t rows = std::max<uint64_t>(p.cull.n_entities, 1);
    const uint64_t tiles = (rows + bge::kBatchTile - 1) / bge::kBatchTile;
    HIP_TRY(w->batch_sort.ensure(rows * 16));
    HIP_TRY(w->batch_hist.ensure(tiles * 256 * 4 * 2));
    uint32_t* rec = w->batch_sort.as<uint32_t>();
    p.sort_key[0] = rec;
    p.sort_key[1] = rec + rows;
    p.sort_entity[0] = rec + 2 * rows;
    p.sort_entity[1] = rec + 3 * rows;
    p.hist = w->batch_hist.as<uint32_t>();
    p.hist_off = p.hist + tiles * 256;
    return BGE_OK;
}

} // namespace

int bge_world_upload_draw_keys(bge_world* w, uint64_t first, uint64_t count, const uint32_t* key)
try {
    return upload_draw_keys(w, Entities::range(first, count), key);
}
BGE_CATCH_ALL("bge_world_upload_draw_keys")

int bge_world_upload_draw_keys_indexed(bge_world* w, uint64_t count, const uint32_t* entity_index, const uint32_t* key)
try {
    return upload_draw_keys(w, Entities::list(count, entity_index), key);
}
BGE_CATCH_ALL("bge_world_upload_draw_keys_indexed")

int bge_world_draw_batches(bge_world* w, const bge_cull_desc* desc, uint32_t n_keys, bge_draw_batch* batches, uint32_t* entities,
                           float* world16, float* normal16, uint64_t cap, uint64_t* total)
try {
    if (!w || !total) return fail(BGE_ERR_INVALID, "NULL argument");
    *total = 0;
    DeviceGuard guard(w->device);
    bge::BatchParams p{};
    if (int rc = batch_params(w, desc, n_keys, normal16 != nullptr, p)) return rc;
    HIP_TRY(w->cull_total.ensure(8));
    p.cull.total = w->cull_total.as<unsigned long long>();
    HIP_TRY(bge::launch_batch_count(w->stream, p));
    const bool records = entities || world16 || normal16;
    if (batches || records) {
        if (batches) {
            HIP_TRY(w->batch_out.ensure(static_cast<size_t>(n_keys) * 8));
            p.batches = w->batch_out.as<uint32_t>();
        }
        HIP_TRY(bge::launch_batch_sort(w->stream, p));
        if (batches) HIP_TRY(hipMemcpyAsync(batches, p.batches, static_cast<size_t>(n_keys) * 8, hipMemcpyDeviceToHost, w->stream));
    }
    uint64_t n = 0;
    HIP_TRY(hipMemcpyAsync(&n, w->cull_total.p, 8, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    *total = n;
    if (!records || n == 0) return BGE_OK;
    if (cap < n) return fail(BGE_ERR_INVALID, "draw batches: %llu records, room for %llu", (unsigned long long)n, (unsigned long long)cap);
    // the records are gathered from the sorted list the sort left (nothing ran in between) into one buffer: indices | world | normal
    const uint64_t idx_bytes = (n * 4 + 15) & ~15ull;
    HIP_TRY(w->cull_out.ensure(idx_bytes + n * 64 * ((world16 ? 1 : 0) + (normal16 ? 1 : 0))));
    char* out = w->cull_out.as<char>();
    p.cull.out_entities = entities ? reinterpret_cast<uint32_t*>(out) : nullptr;
    p.cull.out_world = world16 ? reinterpret_cast<float*>(out + idx_bytes) : nullptr;
    p.cull.out_normal = normal16 ? reinterpret_cast<float*>(out + idx_bytes + (world16 ? n * 64 : 0)) : nullptr;
    p.cull.cap = n;
    HIP_TRY(bge::launch_batch_gather(w->stream, p));
    if (entities) HIP_TRY(hipMemcpyAsync(entities, p.cull.out_entities, n * 4, hipMemcpyDeviceToHost, w->stream));
    if (world16) HIP_TRY(hipMemcpyAsync(world16, p.cull.out_world, n * 64, hipMemcpyDeviceToHost, w->stream));
    if (normal16) HIP_TRY(hipMemcpyAsync(normal16, p.cull.out_normal, n * 64, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_draw_batches")

int bge_world_draw_batches_device(bge_world* w, const bge_cull_desc* desc, uint32_t n_keys, void* batches_device, void* entities_device,
                                  void* world16_device, void* normal16_device, uint64_t cap, void* total_device)
try {
    if (!w || !total_device) return fail(BGE_ERR_INVALID, "NULL argument");
    if ((reinterpret_cast<uintptr_t>(batches_device) | reinterpret_cast<uintptr_t>(entities_device)) & 3u) {
        return fail(BGE_ERR_INVALID, "batches / entities must be 4-byte aligned");
    }
    if ((reinterpret_cast<uintptr_t>(world16_device) | reinterpret_cast<uintptr_t>(normal16_device)) & 15u) {
        return fail(BGE_ERR_INVALID, "world16 / normal16 must be 16-byte aligned");
    }
    if (reinterpret_cast<uintptr_t>(total_device) & 7u) return fail(BGE_ERR_INVALID, "total must be 8-byte aligned");
    DeviceGuard guard(w->device);
    bge::BatchParams p{};
    if (int rc = batch_params(w, desc, n_keys, normal16_device != nullptr, p)) return rc;
    p.batches = static_cast<uint32_t*>(batches_device);
    p.cull.out_entities = static_cast<uint32_t*>(entities_device);
    p.cull.out_world = static_cast<float*>(world16_device);
    p.cull.out_normal = static_cast<float*>(normal16_device);
    p.cull.cap = cap;
    p.cull.total = static_cast<unsigned long long*>(total_device);
    HIP_TRY(bge::launch_batch_count(w->stream, p));
    if (p.batches || (cap && (p.cull.out_entities || p.cull.out_world || p.cull.out_normal))) {
        HIP_TRY(bge::launch_batch_sort(w->stream, p));
        HIP_TRY(bge::launch_batch_gather(w->stream, p));
    }
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_draw_batches_device")

int bge_frustum_planes(const float m[16], int homogeneous_depth, float planes24[24])
try {
    if (!m || !planes24) return fail(BGE_ERR_INVALID, "NULL argument");
    for (int i = 0; i < 4; ++i) { // coefficient i of every plane comes from row i: clip_j = sum_i v_i * m[4i+j]
        const float x = m[4 * i], y = m[4 * i + 1], z = m[4 * i + 2], ww = m[4 * i + 3];
        planes24[0 + i] = ww + x;
        planes24[4 + i] = ww - x;
        planes24[8 + i] = ww + y;
        planes24[12 + i] = ww - y;
        planes24[16 + i] = homogeneous_depth ? ww + z : z;
        planes24[20 + i] = ww - z;
    }
    return BGE_OK;
}
BGE_CATCH_ALL("bge_frustum_planes")

int bge_world_pack_roots(bge_world* w, void* dst_device)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (!w->has_topology) return fail(BGE_ERR_STATE, "bge_world_set_topology has not been called");
    DeviceGuard guard(w->device);
    float* dst = dst_device ? static_cast<float*>(dst_device) : w->root_worlds.as<float>();
    HIP_TRY(bge::launch_pack_roots(w->stream, w->flat.root_slots.size(), w->root_slots.as<uint32_t>(), w->world.as<float>(), w->row3_view(), dst));
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_pack_roots")

int bge_world_device_array(bge_world* w, int which, void** device_ptr, uint64_t* elements)
try {
    if (!w || !device_ptr) return fail(BGE_ERR_INVALID, "NULL argument");
    if (!w->has_topology) return fail(BGE_ERR_STATE, "bge_world_set_topology has not been called");
    uint64_t n = 0;
    void* p = nullptr;
    switch (which) {
    case BGE_ARRAY_WORLD:
    case BGE_ARRAY_POSITION: {
        // A raw pointer sees memory, not a composed row — and a holder of the position pointer could move a body without the world
        // knowing: the deferred rows are stored now and no tick of this world defers again (bge_epochs.hpp Row3State::pinned)
        DeviceGuard guard(w->device);
        w->row3.pinned = true;
        HIP_TRY(w->ensure_row3_current());
        HIP_TRY(hipStreamSynchronize(w->stream));
        p = which == BGE_ARRAY_WORLD ? w->world.p : w->pos.p;
        n = w->flat.n_slots;
        break;
    }
    case BGE_ARRAY_ROOT_WORLDS: p = w->root_worlds.p; n = w->flat.root_slots.size(); break;
    case BGE_ARRAY_SLOT_OF_ENTITY: p = w->slot_of_entity.p; n = w->flat.n_entities; break;
    case BGE_ARRAY_PAIRS: {
        bge::Broadphase& bp = w->pairs_from_slab ? w->slab_broadphase : w->broadphase;
        DeviceGuard guard(w->device);
        if (bp.compact(w->stream) != BGE_OK) return fail(BGE_ERR_HIP, "%s", bp.error());
        p = bp.pairs_device();
        n = bp.capacity();
        break;
    }
    case BGE_ARRAY_NORMAL: p = w->normal.p; n = w->normal.p ? w->flat.n_slots : 0; break;
    default: return fail(BGE_ERR_INVALID, "unknown device array %d", which);
    }
    *device_ptr = p;
    if (elements) *elements = n;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_device_array")

int bge_comm_unique_id(void* out128)
try {
    if (!out128) return fail(BGE_ERR_INVALID, "out128 is NULL");
    std::string err;
    const int rc = bge::RootComm::unique_id(out128, err);
    if (rc != BGE_OK) return fail(rc, "%s", err.c_str());
    return BGE_OK;
}
BGE_CATCH_ALL("bge_comm_unique_id")

int bge_world_comm_init(bge_world* w, int nranks, int rank, const void* id128, uint64_t rows_per_rank)
try {
    if (!w || !id128) return fail(BGE_ERR_INVALID, "NULL argument");
    if (nranks <= 0 || rank < 0 || rank >= nranks) return fail(BGE_ERR_INVALID, "rank %d of %d", rank, nranks);
    DeviceGuard guard(w->device);
    const int rc = w->comm.init(nranks, rank, id128, rows_per_rank);
    if (rc != BGE_OK) return fail(rc, "%s", w->comm.error());
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_comm_init")

int bge_world_gather_roots(bge_world* w, void** table_device)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (!w->has_topology) return fail(BGE_ERR_STATE, "bge_world_set_topology has not been called");
    if (!w->comm.ready()) return fail(BGE_ERR_STATE, "bge_world_comm_init has not been called");
    if (w->flat.root_slots.size() > w->comm.rows_per_rank()) {
        return fail(BGE_ERR_INVALID, "%zu roots but the communicator was sized for %llu rows per rank", w->flat.root_slots.size(),
                    (unsigned long long)w->comm.rows_per_rank());
    }
    DeviceGuard guard(w->device);
    float* send = nullptr;
    int rc = w->comm.begin_frame(w->stream, &send);
    if (rc != BGE_OK) return fail(rc, "%s", w->comm.error());
    HIP_TRY(bge::launch_pack_roots(w->stream, w->flat.root_slots.size(), w->root_slots.as<uint32_t>(), w->world.as<float>(), w->row3_view(), send,
                                   /*compact=*/true));
    rc = w->comm.gather(w->stream, table_device);
    if (rc != BGE_OK) return fail(rc, "%s", w->comm.error());
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_gather_roots")

int bge_world_download_gathered(bge_world* w, float* out, uint64_t floats)
try {
    if (!w || !out) return fail(BGE_ERR_INVALID, "NULL argument");
    if (!w->comm.ready()) return fail(BGE_ERR_STATE, "bge_world_comm_init has not been called");
    DeviceGuard guard(w->device);
    if (w->comm.wait(w->stream) != BGE_OK) return fail(BGE_ERR_HIP, "%s", w->comm.error());
    const void* table = w->comm.last_table();
    if (!table) return fail(BGE_ERR_STATE, "nothing has been gathered yet");
    // the table holds compact rows (12 floats); the caller gets full 4x4 matrices
    const uint64_t rows = w->comm.rows_per_rank() * static_cast<uint64_t>(w->comm.nranks());
    std::vector<float> compact(rows * bge::RootComm::kRowFloats);
    HIP_TRY(hipMemcpyAsync(compact.data(), table, compact.size() * 4, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    const uint64_t take = std::min<uint64_t>(floats / 16, rows);
    for (uint64_t r = 0; r < take; ++r) {
        const float* c = &compact[r * bge::RootComm::kRowFloats];
        float* m = out + 16 * r;
        for (int row = 0; row < 4; ++row) {
            m[4 * row] = c[3 * row];
            m[4 * row + 1] = c[3 * row + 1];
            m[4 * row + 2] = c[3 * row + 2];
            m[4 * row + 3] = row == 3 ? 1.0f : 0.0f;
        }
    }
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_download_gathered")

int bge_world_comm_set_mode(bge_world* w, int mode)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    if (mode != BGE_GATHER_ALLGATHER && mode != BGE_GATHER_DIRECT) return fail(BGE_ERR_INVALID, "unknown gather mode %d", mode);
    DeviceGuard guard(w->device);
    if (w->comm.ready() && w->comm.wait(w->stream) != BGE_OK) return fail(BGE_ERR_HIP, "%s", w->comm.error());
    w->comm.set_mode(mode);
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_comm_set_mode")

int bge_world_comm_wait(bge_world* w)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    DeviceGuard guard(w->device);
    const int rc = w->comm.wait(w->stream);
    if (rc != BGE_OK) return fail(rc, "%s", w->comm.error());
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_comm_wait")

int bge_world_comm_destroy(bge_world* w)
try {
    if (!w) return fail(BGE_ERR_INVALID, "world is NULL");
    DeviceGuard guard(w->device);
    (void)hipStreamSynchronize(w->stream);
    w->comm.destroy();
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_comm_destroy")

static void fill_info(const bge::Flattened& f, bge_world_info* info)
{
    info->n_entities = f.n_entities;
    info->n_transforms = f.n_transforms;
    info->n_slots = f.n_slots;
    info->n_tiles = f.n_tiles_ticked;
    info->n_passes = f.pass_tile_begin.size() - 1;
    info->n_roots = f.root_slots.size();
    info->n_limbo = f.n_limbo;
    info->n_bodies = 0;
    info->max_depth = f.max_depth;
}

int bge_world_get_info(bge_world* w, bge_world_info* info)
try {
    if (!w || !info) return fail(BGE_ERR_INVALID, "NULL argument");
    if (!w->has_topology) return fail(BGE_ERR_STATE, "bge_world_set_topology has not been called");
    fill_info(w->flat, info);
    for (uint8_t t : w->body_type_host) info->n_bodies += t != BGE_BODY_NONE ? 1 : 0;
    return BGE_OK;
}
BGE_CATCH_ALL("bge_world_get_info")

int bge_flatten_topology(uint64_t n, const uint32_t* parent, const uint8_t* has_transform, uint32_t* slot_of_entity,
                         uint8_t* level_of_entity, uint32_t* pass_of_entity, bge_world_info* info)
try {
    if (n >= 0xfffffff0ull) return fail(BGE_ERR_INVALID, "too many entities");
    bge::Flattened f;
    try {
        bge::flatten_topology(n, parent, has_transform, f);
    } catch (const std::bad_alloc&) {
        return fail(BGE_ERR_OOM, "host allocation failed");
    }
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t s = f.slot_of_entity[i];
        if (slot_of_entity) slot_of_entity[i] = s;
        if (level_of_entity) level_of_entity[i] = s == bge::kNone ? 0 : static_cast<uint8_t>((f.flags[s] & bge::kLevelMask) >> bge::kLevelShift);
        if (pass_of_entity) pass_of_entity[i] = f.pass_of_entity[i];
    }
    if (info) fill_info(f, info);
    return BGE_OK;
}
BGE_CATCH_ALL("bge_flatten_topology")

int bge_partition_subtrees(uint64_t n, const uint32_t* parent, const uint8_t* has_transform, uint32_t nranks,
                           uint32_t* rank_of_entity, uint64_t* nodes_per_rank)
try {
    if (!rank_of_entity || nranks == 0) return fail(BGE_ERR_INVALID, "bad arguments");
    try {
        bge::partition_subtrees(n, parent, has_transform, nranks, rank_of_entity, nodes_per_rank);
    } catch (const std::bad_alloc&) {
        return fail(BGE_ERR_OOM, "host allocation failed");
    }
    return BGE_OK;
}
BGE_CATCH_ALL("bge_partition_subtrees")

} // extern "C"
