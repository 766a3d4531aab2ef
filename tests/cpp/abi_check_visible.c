/* The frustum-culling part of the C ABI (include/bge_world.h bge_world_visible*) seen from C99: the descriptor's layout, the
 * entry points link and refuse a NULL world, and bge_frustum_planes (host only) gives the planes of a matrix in the stated order. */
#include <stddef.h>
#include <stdio.h>

#include "../../include/bge_world.h"

typedef char bge_cull_desc_is_264_bytes[(sizeof(bge_cull_desc) == 264) ? 1 : -1];
typedef char bge_cull_desc_n_planes_at_4[(offsetof(bge_cull_desc, n_planes) == 4) ? 1 : -1];
typedef char bge_cull_desc_planes_at_8[(offsetof(bge_cull_desc, planes) == 8) ? 1 : -1];
typedef char bge_cull_max_planes_is_16[(BGE_CULL_MAX_PLANES == 16) ? 1 : -1];

int main(void)
{
    float c[3] = {0.0f, 0.0f, 0.0f}, h[3] = {1.0f, 1.0f, 1.0f}, m[16], planes[24], world16[16];
    uint32_t index = 0, entity = 0;
    uint64_t total = 7;
    bge_cull_desc desc;
    int i;
    desc.struct_size = (uint32_t)sizeof desc;
    desc.n_planes = 0;
    if (bge_world_upload_bounds(NULL, 0, 1, c, h) != BGE_ERR_INVALID) return 2;
    if (bge_world_upload_bounds_indexed(NULL, 1, &index, c, h) != BGE_ERR_INVALID) return 3;
    if (bge_world_visible(NULL, &desc, &entity, world16, NULL, 1, &total) != BGE_ERR_INVALID) return 4;
    if (bge_world_visible_device(NULL, &desc, NULL, NULL, NULL, 0, NULL) != BGE_ERR_INVALID) return 5;
    if (bge_last_error()[0] == '\0') return 6;
    /* identity: clip = (x, y, z, w) -> w+x = (1, 0, 0, 1), w-x = (-1, 0, 0, 1), ..., near = z = (0, 0, 1, 0), w-z = (0, 0, -1, 1) */
    for (i = 0; i < 16; ++i) m[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    if (bge_frustum_planes(m, 0, planes) != BGE_OK) return 7;
    if (planes[0] != 1.0f || planes[3] != 1.0f || planes[4] != -1.0f || planes[7] != 1.0f) return 8;
    if (planes[9] != 1.0f || planes[13] != -1.0f || planes[18] != 1.0f || planes[19] != 0.0f) return 9;
    if (planes[22] != -1.0f || planes[23] != 1.0f) return 10;
    if (bge_frustum_planes(m, 1, planes) != BGE_OK || planes[18] != 1.0f || planes[19] != 1.0f) return 11;
    if (bge_frustum_planes(NULL, 0, planes) != BGE_ERR_INVALID) return 12;
    printf("visible abi ok\n");
    return 0;
}
