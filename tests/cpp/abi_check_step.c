/* The sphere-step-move part of the C ABI (include/bge_world.h bge_world_sphere_step_move*): compiles as C99 (no C++), the records
 * have their stated sizes and offsets and lie over the plain move's, and the entry points link and refuse a NULL world. */
#include <stdio.h>
#include <string.h>

#include "../../include/bge_world.h"

typedef char bge_sphere_step_move_is_48_bytes[(sizeof(bge_sphere_step_move) == 48) ? 1 : -1];
typedef char bge_sphere_step_move_displacement_at_12[(offsetof(bge_sphere_step_move, displacement) == 12) ? 1 : -1];
typedef char bge_sphere_step_move_radius_at_24[(offsetof(bge_sphere_step_move, radius) == 24) ? 1 : -1];
typedef char bge_sphere_step_move_skin_at_28[(offsetof(bge_sphere_step_move, skin) == 28) ? 1 : -1];
typedef char bge_sphere_step_move_probe_at_32[(offsetof(bge_sphere_step_move, probe_distance) == 32) ? 1 : -1];
typedef char bge_sphere_step_move_slope_at_36[(offsetof(bge_sphere_step_move, min_ground_ny) == 36) ? 1 : -1];
typedef char bge_sphere_step_move_mask_at_40[(offsetof(bge_sphere_step_move, layer_mask) == 40) ? 1 : -1];
typedef char bge_sphere_step_move_height_at_44[(offsetof(bge_sphere_step_move, step_height) == 44) ? 1 : -1];
typedef char bge_sphere_step_move_height_is_the_reserved_word[(offsetof(bge_sphere_step_move, step_height) == offsetof(bge_sphere_move, reserved)) ? 1 : -1];
typedef char bge_sphere_step_result_is_80_bytes[(sizeof(bge_sphere_step_result) == 80) ? 1 : -1];
typedef char bge_sphere_step_result_remaining_at_12[(offsetof(bge_sphere_step_result, remaining) == 12) ? 1 : -1];
typedef char bge_sphere_step_result_flags_at_24[(offsetof(bge_sphere_step_result, flags) == 24) ? 1 : -1];
typedef char bge_sphere_step_result_n_hits_at_28[(offsetof(bge_sphere_step_result, n_hits) == 28) ? 1 : -1];
typedef char bge_sphere_step_result_hit_kind_at_32[(offsetof(bge_sphere_step_result, hit_kind) == 32) ? 1 : -1];
typedef char bge_sphere_step_result_hit_entity_at_36[(offsetof(bge_sphere_step_result, hit_entity) == 36) ? 1 : -1];
typedef char bge_sphere_step_result_hit_normal_at_40[(offsetof(bge_sphere_step_result, hit_normal) == 40) ? 1 : -1];
typedef char bge_sphere_step_result_ground_kind_at_52[(offsetof(bge_sphere_step_result, ground_kind) == 52) ? 1 : -1];
typedef char bge_sphere_step_result_ground_entity_at_56[(offsetof(bge_sphere_step_result, ground_entity) == 56) ? 1 : -1];
typedef char bge_sphere_step_result_ground_distance_at_60[(offsetof(bge_sphere_step_result, ground_distance) == 60) ? 1 : -1];
typedef char bge_sphere_step_result_ground_normal_at_64[(offsetof(bge_sphere_step_result, ground_normal) == 64) ? 1 : -1];
typedef char bge_sphere_step_result_rise_at_76[(offsetof(bge_sphere_step_result, step_rise) == 76) ? 1 : -1];
typedef char bge_sphere_step_result_rise_is_the_reserved_word[(offsetof(bge_sphere_step_result, step_rise) == offsetof(bge_sphere_move_result, reserved)) ? 1 : -1];

int main(void)
{
    bge_sphere_step_move move;
    bge_sphere_step_result result;
    memset(&move, 0, sizeof move);
    move.displacement[0] = 1.0f;
    move.radius = 0.5f;
    move.skin = 0.01f;
    move.layer_mask = 1u;
    move.step_height = 0.3f;
    if (BGE_MOVE_STEP_TRIED != 16 || BGE_MOVE_STEPPED != 32) return 1;
    if ((BGE_MOVE_STEP_TRIED | BGE_MOVE_STEPPED) & (BGE_MOVE_INVALID | BGE_MOVE_GROUNDED | BGE_MOVE_OUT_OF_SLIDES | BGE_MOVE_PROBE_HIT)) return 6;
    if (bge_world_sphere_step_move(NULL, 1, &move, &result) != BGE_ERR_INVALID) return 2;
    if (bge_world_sphere_step_move(NULL, 0, NULL, NULL) != BGE_ERR_INVALID) return 3;
    if (bge_world_sphere_step_move_device(NULL, 1, NULL, NULL) != BGE_ERR_INVALID) return 4;
    if (bge_last_error()[0] == '\0') return 5;
    printf("step abi ok\n");
    return 0;
}
