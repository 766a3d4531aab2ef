/* The sphere-query part of the C ABI (include/bge_world.h bge_world_sphere_cast*, bge_world_overlap_sphere): compiles as C99 (no
 * C++), the records have their stated sizes and offsets, and the entry points link and refuse a NULL world. */
#include <stdio.h>
#include <string.h>

#include "../../include/bge_world.h"

typedef char bge_sphere_cast_is_40_bytes[(sizeof(bge_sphere_cast) == 40) ? 1 : -1];
typedef char bge_sphere_cast_radius_at_28[(offsetof(bge_sphere_cast, radius) == 28) ? 1 : -1];
typedef char bge_sphere_cast_mask_at_32[(offsetof(bge_sphere_cast, layer_mask) == 32) ? 1 : -1];
typedef char bge_sphere_is_20_bytes[(sizeof(bge_sphere) == 20) ? 1 : -1];
typedef char bge_sphere_mask_at_16[(offsetof(bge_sphere, layer_mask) == 16) ? 1 : -1];
typedef char bge_overlap_hit_is_12_bytes[(sizeof(bge_overlap_hit) == 12) ? 1 : -1];
typedef char bge_overlap_hit_distance_at_8[(offsetof(bge_overlap_hit, distance) == 8) ? 1 : -1];

int main(void)
{
    bge_sphere_cast cast;
    bge_sphere sphere;
    bge_ray_hit hit;
    bge_overlap_hit found;
    uint64_t offsets[2] = {0, 0}, total = 7;
    memset(&cast, 0, sizeof cast);
    memset(&sphere, 0, sizeof sphere);
    cast.direction[1] = -1.0f;
    cast.max_distance = 200.0f;
    cast.radius = 0.5f;
    cast.layer_mask = 1u;
    sphere.radius = 1.0f;
    sphere.layer_mask = 1u;
    if (bge_world_sphere_cast(NULL, 1, &cast, &hit) != BGE_ERR_INVALID) return 1;
    if (bge_world_sphere_cast_all(NULL, 1, &cast, &hit, 1, offsets, &total) != BGE_ERR_INVALID) return 2;
    if (bge_world_sphere_cast_device(NULL, 1, NULL, NULL) != BGE_ERR_INVALID) return 3;
    if (bge_world_overlap_sphere(NULL, 1, &sphere, &found, 1, offsets, &total) != BGE_ERR_INVALID) return 4;
    if (bge_last_error()[0] == '\0') return 5;
    printf("sphere abi ok\n");
    return 0;
}
