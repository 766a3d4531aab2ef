/* The ray-query part of the C ABI (include/bge_world.h bge_world_raycast*): compiles as C99 (no C++), the records have their
 * stated sizes, and the entry points link and refuse a NULL world. */
#include <stdio.h>
#include <string.h>

#include "../../include/bge_world.h"

typedef char bge_ray_is_32_bytes[(sizeof(bge_ray) == 32) ? 1 : -1];
typedef char bge_ray_hit_is_40_bytes[(sizeof(bge_ray_hit) == 40) ? 1 : -1];
typedef char bge_ray_hit_point_at_16[(offsetof(bge_ray_hit, point) == 16) ? 1 : -1];
typedef char bge_ray_mask_at_28[(offsetof(bge_ray, layer_mask) == 28) ? 1 : -1];

int main(void)
{
    bge_ray ray;
    bge_ray_hit hit;
    uint64_t offsets[2] = {0, 0}, total = 7;
    memset(&ray, 0, sizeof ray);
    ray.direction[1] = -1.0f;
    ray.max_distance = 200.0f;
    ray.layer_mask = 1u;
    if (bge_world_raycast(NULL, 1, &ray, &hit) != BGE_ERR_INVALID) return 1;
    if (bge_world_raycast_all(NULL, 1, &ray, &hit, 1, offsets, &total) != BGE_ERR_INVALID) return 2;
    if (bge_world_raycast_device(NULL, 1, NULL, NULL) != BGE_ERR_INVALID) return 3;
    if (bge_last_error()[0] == '\0') return 4;
    if (BGE_RAY_MISS != 0 || BGE_RAY_BODY != 1 || BGE_RAY_TRIGGER != 2 || BGE_RAY_GROUND != 3 || BGE_RAY_NO_ENTITY != 0xffffffffu) return 5;
    printf("raycast abi ok\n");
    return 0;
}
