/* The penetration and recovery part of the C ABI (include/bge_world.h bge_world_sphere_penetration*, bge_world_sphere_recover*):
 * compiles as C99 (no C++), the records have their stated sizes and offsets, and the entry points link and refuse a NULL world. */
#include <stdio.h>
#include <string.h>

#include "../../include/bge_world.h"

typedef char bge_penetration_hit_is_40_bytes[(sizeof(bge_penetration_hit) == 40) ? 1 : -1];
typedef char bge_penetration_hit_entity_at_4[(offsetof(bge_penetration_hit, entity) == 4) ? 1 : -1];
typedef char bge_penetration_hit_depth_at_8[(offsetof(bge_penetration_hit, depth) == 8) ? 1 : -1];
typedef char bge_penetration_hit_point_at_12[(offsetof(bge_penetration_hit, point) == 12) ? 1 : -1];
typedef char bge_penetration_hit_normal_at_24[(offsetof(bge_penetration_hit, normal) == 24) ? 1 : -1];
typedef char bge_penetration_hit_reserved_at_36[(offsetof(bge_penetration_hit, reserved) == 36) ? 1 : -1];
typedef char bge_sphere_recover_is_28_bytes[(sizeof(bge_sphere_recover) == 28) ? 1 : -1];
typedef char bge_sphere_recover_radius_at_12[(offsetof(bge_sphere_recover, radius) == 12) ? 1 : -1];
typedef char bge_sphere_recover_skin_at_16[(offsetof(bge_sphere_recover, skin) == 16) ? 1 : -1];
typedef char bge_sphere_recover_mask_at_20[(offsetof(bge_sphere_recover, layer_mask) == 20) ? 1 : -1];
typedef char bge_sphere_recover_reserved_at_24[(offsetof(bge_sphere_recover, reserved) == 24) ? 1 : -1];
typedef char bge_sphere_recover_result_is_64_bytes[(sizeof(bge_sphere_recover_result) == 64) ? 1 : -1];
typedef char bge_sphere_recover_result_pushed_at_12[(offsetof(bge_sphere_recover_result, pushed) == 12) ? 1 : -1];
typedef char bge_sphere_recover_result_flags_at_24[(offsetof(bge_sphere_recover_result, flags) == 24) ? 1 : -1];
typedef char bge_sphere_recover_result_n_pushes_at_28[(offsetof(bge_sphere_recover_result, n_pushes) == 28) ? 1 : -1];
typedef char bge_sphere_recover_result_hit_kind_at_32[(offsetof(bge_sphere_recover_result, hit_kind) == 32) ? 1 : -1];
typedef char bge_sphere_recover_result_hit_entity_at_36[(offsetof(bge_sphere_recover_result, hit_entity) == 36) ? 1 : -1];
typedef char bge_sphere_recover_result_hit_normal_at_40[(offsetof(bge_sphere_recover_result, hit_normal) == 40) ? 1 : -1];
typedef char bge_sphere_recover_result_hit_depth_at_52[(offsetof(bge_sphere_recover_result, hit_depth) == 52) ? 1 : -1];
typedef char bge_sphere_recover_result_remaining_at_56[(offsetof(bge_sphere_recover_result, remaining_depth) == 56) ? 1 : -1];
typedef char bge_sphere_recover_result_reserved_at_60[(offsetof(bge_sphere_recover_result, reserved) == 60) ? 1 : -1];
typedef char bge_recover_rounds_is_4[(BGE_RECOVER_ROUNDS == 4) ? 1 : -1];

int main(void)
{
    bge_sphere sphere;
    bge_penetration_hit hit;
    bge_sphere_recover record;
    bge_sphere_recover_result result;
    memset(&sphere, 0, sizeof sphere);
    memset(&record, 0, sizeof record);
    sphere.radius = 0.5f;
    sphere.layer_mask = 1u;
    record.radius = 0.5f;
    record.skin = 0.01f;
    record.layer_mask = 1u;
    if (BGE_RECOVER_INVALID != 1 || BGE_RECOVER_MOVED != 2 || BGE_RECOVER_STUCK != 4) return 1;
    if (bge_world_sphere_penetration(NULL, 1, &sphere, &hit) != BGE_ERR_INVALID) return 2;
    if (bge_world_sphere_penetration_device(NULL, 1, NULL, NULL) != BGE_ERR_INVALID) return 3;
    if (bge_world_sphere_recover(NULL, 1, &record, &result) != BGE_ERR_INVALID) return 4;
    if (bge_world_sphere_recover(NULL, 0, NULL, NULL) != BGE_ERR_INVALID) return 5;
    if (bge_world_sphere_recover_device(NULL, 1, NULL, NULL) != BGE_ERR_INVALID) return 6;
    if (bge_last_error()[0] == '\0') return 7;
    printf("recover abi ok\n");
    return 0;
}
