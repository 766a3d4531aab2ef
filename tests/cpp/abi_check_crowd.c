/* The crowd-separation part of the C ABI (include/bge_world.h bge_world_crowd_query .., bge_world_characters_crowd ..): compiles as
 * C99 (no C++), the two records have their stated sizes and offsets, the flag words their values, and the entry points link and
 * refuse a NULL world. */
#include <stdio.h>
#include <string.h>

#include "../../include/bge_world.h"

typedef char bge_crowd_sphere_is_24_bytes[(sizeof(bge_crowd_sphere) == 24) ? 1 : -1];
typedef char bge_crowd_sphere_center_at_0[(offsetof(bge_crowd_sphere, center) == 0) ? 1 : -1];
typedef char bge_crowd_sphere_radius_at_12[(offsetof(bge_crowd_sphere, radius) == 12) ? 1 : -1];
typedef char bge_crowd_sphere_group_at_16[(offsetof(bge_crowd_sphere, group) == 16) ? 1 : -1];
typedef char bge_crowd_sphere_mask_at_20[(offsetof(bge_crowd_sphere, mask) == 20) ? 1 : -1];
typedef char bge_crowd_hit_is_32_bytes[(sizeof(bge_crowd_hit) == 32) ? 1 : -1];
typedef char bge_crowd_hit_flags_at_0[(offsetof(bge_crowd_hit, flags) == 0) ? 1 : -1];
typedef char bge_crowd_hit_other_at_4[(offsetof(bge_crowd_hit, other) == 4) ? 1 : -1];
typedef char bge_crowd_hit_n_overlaps_at_8[(offsetof(bge_crowd_hit, n_overlaps) == 8) ? 1 : -1];
typedef char bge_crowd_hit_depth_at_12[(offsetof(bge_crowd_hit, depth) == 12) ? 1 : -1];
typedef char bge_crowd_hit_push_at_16[(offsetof(bge_crowd_hit, push) == 16) ? 1 : -1];
typedef char bge_crowd_hit_reserved_at_28[(offsetof(bge_crowd_hit, reserved) == 28) ? 1 : -1];

int main(void)
{
    bge_crowd_sphere sphere;
    bge_crowd_hit hit;
    void* ptr = NULL;
    uint64_t n = 0;
    memset(&sphere, 0, sizeof sphere);
    memset(&hit, 0, sizeof hit);
    if (BGE_CROWD_INVALID != 1 || BGE_CROWD_PUSHED != 2 || BGE_CROWD_CLAMPED != 4) return 1;
    if (BGE_CHAR_CROWD_ON != 1) return 2;
    if (bge_world_crowd_query(NULL, 1, &sphere, 0.0f, &hit) != BGE_ERR_INVALID) return 3;
    if (bge_world_crowd_query_device(NULL, 1, &sphere, 0.0f, &hit) != BGE_ERR_INVALID) return 4;
    if (bge_world_characters_crowd(NULL, BGE_CHAR_CROWD_ON, 0.0f, 1, NULL, NULL) != BGE_ERR_INVALID) return 5;
    if (bge_world_characters_crowd_hits(NULL, 0, 1, &hit) != BGE_ERR_INVALID) return 6;
    if (bge_world_characters_crowd_hits_device(NULL, &ptr, &n) != BGE_ERR_INVALID) return 7;
    if (bge_last_error()[0] == '\0') return 8;
    printf("crowd abi ok\n");
    return 0;
}
