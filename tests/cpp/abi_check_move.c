/* The sphere-move part of the C ABI (include/bge_world.h bge_world_sphere_move*): compiles as C99 (no C++), the records have their
 * stated sizes and offsets, and the entry points link and refuse a NULL world. */
#include <stdio.h>
#include <string.h>

#include "../../include/bge_world.h"

typedef char bge_sphere_move_is_48_bytes[(sizeof(bge_sphere_move) == 48) ? 1 : -1];
typedef char bge_sphere_move_displacement_at_12[(offsetof(bge_sphere_move, displacement) == 12) ? 1 : -1];
typedef char bge_sphere_move_radius_at_24[(offsetof(bge_sphere_move, radius) == 24) ? 1 : -1];
typedef char bge_sphere_move_skin_at_28[(offsetof(bge_sphere_move, skin) == 28) ? 1 : -1];
typedef char bge_sphere_move_probe_at_32[(offsetof(bge_sphere_move, probe_distance) == 32) ? 1 : -1];
typedef char bge_sphere_move_slope_at_36[(offsetof(bge_sphere_move, min_ground_ny) == 36) ? 1 : -1];
typedef char bge_sphere_move_mask_at_40[(offsetof(bge_sphere_move, layer_mask) == 40) ? 1 : -1];
typedef char bge_sphere_move_result_is_80_bytes[(sizeof(bge_sphere_move_result) == 80) ? 1 : -1];
typedef char bge_sphere_move_result_remaining_at_12[(offsetof(bge_sphere_move_result, remaining) == 12) ? 1 : -1];
typedef char bge_sphere_move_result_flags_at_24[(offsetof(bge_sphere_move_result, flags) == 24) ? 1 : -1];
typedef char bge_sphere_move_result_n_hits_at_28[(offsetof(bge_sphere_move_result, n_hits) == 28) ? 1 : -1];
typedef char bge_sphere_move_result_hit_kind_at_32[(offsetof(bge_sphere_move_result, hit_kind) == 32) ? 1 : -1];
typedef char bge_sphere_move_result_hit_normal_at_40[(offsetof(bge_sphere_move_result, hit_normal) == 40) ? 1 : -1];
typedef char bge_sphere_move_result_ground_kind_at_52[(offsetof(bge_sphere_move_result, ground_kind) == 52) ? 1 : -1];
typedef char bge_sphere_move_result_ground_distance_at_60[(offsetof(bge_sphere_move_result, ground_distance) == 60) ? 1 : -1];
typedef char bge_sphere_move_result_ground_normal_at_64[(offsetof(bge_sphere_move_result, ground_normal) == 64) ? 1 : -1];
typedef char bge_move_slides_is_4[(BGE_MOVE_SLIDES == 4) ? 1 : -1];

int main(void)
{
    bge_sphere_move move;
    bge_sphere_move_result result;
    memset(&move, 0, sizeof move);
    move.displacement[1] = -1.0f;
    move.radius = 0.5f;
    move.skin = 0.01f;
    move.layer_mask = 1u;
    if (BGE_MOVE_INVALID != 1 || BGE_MOVE_GROUNDED != 2 || BGE_MOVE_OUT_OF_SLIDES != 4 || BGE_MOVE_PROBE_HIT != 8) return 1;
    if (bge_world_sphere_move(NULL, 1, &move, &result) != BGE_ERR_INVALID) return 2;
    if (bge_world_sphere_move(NULL, 0, NULL, NULL) != BGE_ERR_INVALID) return 3;
    if (bge_world_sphere_move_device(NULL, 1, NULL, NULL) != BGE_ERR_INVALID) return 4;
    if (bge_last_error()[0] == '\0') return 5;
    printf("move abi ok\n");
    return 0;
}
