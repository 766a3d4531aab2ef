/* The draw-batch part of the C ABI (include/bge_world.h bge_world_draw_batches*) seen from C99: the record's layout, the two
 * constants, and the entry points link and refuse a NULL world. */
#include <stddef.h>
#include <stdio.h>

#include "../../include/bge_world.h"

typedef char bge_draw_batch_is_8_bytes[(sizeof(bge_draw_batch) == 8) ? 1 : -1];
typedef char bge_draw_batch_count_at_4[(offsetof(bge_draw_batch, instance_count) == 4) ? 1 : -1];
typedef char bge_no_draw_key_is_all_ones[(BGE_NO_DRAW_KEY == 0xffffffffu) ? 1 : -1];
typedef char bge_draw_max_keys_is_65536[(BGE_DRAW_MAX_KEYS == 65536u) ? 1 : -1];

int main(void)
{
    uint32_t key = 0, index = 0, entity = 0;
    uint64_t total = 7;
    float world16[16];
    bge_draw_batch batch;
    bge_cull_desc desc;
    desc.struct_size = (uint32_t)sizeof desc;
    desc.n_planes = 0;
    if (bge_world_upload_draw_keys(NULL, 0, 1, &key) != BGE_ERR_INVALID) return 2;
    if (bge_world_upload_draw_keys_indexed(NULL, 1, &index, &key) != BGE_ERR_INVALID) return 3;
    if (bge_world_draw_batches(NULL, &desc, 1, &batch, &entity, world16, NULL, 1, &total) != BGE_ERR_INVALID) return 4;
    if (bge_world_draw_batches_device(NULL, &desc, 1, NULL, NULL, NULL, NULL, 0, NULL) != BGE_ERR_INVALID) return 5;
    if (bge_last_error()[0] == '\0') return 6;
    printf("batches abi ok\n");
    return 0;
}
