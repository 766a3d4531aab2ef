/* The impulse part of the C ABI (include/bge_world.h bge_world_apply_impulses .., bge_world_characters_push ..): compiles as C99 (no
 * C++), the two records have their stated sizes and offsets, the flag and status words their values, and the entry points link and
 * refuse a NULL world. */
#include <stdio.h>
#include <string.h>

#include "../../include/bge_world.h"

typedef char bge_impulse_is_32_bytes[(sizeof(bge_impulse) == 32) ? 1 : -1];
typedef char bge_impulse_entity_at_0[(offsetof(bge_impulse, entity) == 0) ? 1 : -1];
typedef char bge_impulse_flags_at_4[(offsetof(bge_impulse, flags) == 4) ? 1 : -1];
typedef char bge_impulse_impulse_at_8[(offsetof(bge_impulse, impulse) == 8) ? 1 : -1];
typedef char bge_impulse_point_at_20[(offsetof(bge_impulse, point) == 20) ? 1 : -1];
typedef char bge_character_push_desc_is_16_bytes[(sizeof(bge_character_push_desc) == 16) ? 1 : -1];
typedef char bge_character_push_desc_flags_at_0[(offsetof(bge_character_push_desc, flags) == 0) ? 1 : -1];
typedef char bge_character_push_desc_force_at_4[(offsetof(bge_character_push_desc, force) == 4) ? 1 : -1];
typedef char bge_character_push_desc_max_normal_y_at_8[(offsetof(bge_character_push_desc, max_normal_y) == 8) ? 1 : -1];
typedef char bge_character_push_desc_body_mask_at_12[(offsetof(bge_character_push_desc, body_mask) == 12) ? 1 : -1];

int main(void)
{
    bge_impulse record;
    bge_character_push_desc desc;
    uint32_t status = 0;
    void* ptr = NULL;
    uint64_t n = 0;
    memset(&record, 0, sizeof record);
    memset(&desc, 0, sizeof desc);
    if (BGE_IMPULSE_AT_POINT != 0 || BGE_IMPULSE_CENTRAL != 1 || BGE_IMPULSE_TORQUE != 2 || BGE_IMPULSE_WORLD_POINT != 4) return 1;
    if (BGE_IMPULSE_APPLIED != 1 || BGE_IMPULSE_WOKE != 2 || BGE_IMPULSE_INVALID != 4 || BGE_IMPULSE_NO_BODY != 8) return 2;
    if (BGE_CHAR_PUSH_ON != 1) return 3;
    if (bge_world_apply_impulses(NULL, 1, &record, &status) != BGE_ERR_INVALID) return 4;
    if (bge_world_apply_impulses_device(NULL, 1, &record, &status) != BGE_ERR_INVALID) return 5;
    if (bge_world_characters_push(NULL, &desc) != BGE_ERR_INVALID) return 6;
    if (bge_world_characters_push_records(NULL, 0, 1, &record) != BGE_ERR_INVALID) return 7;
    if (bge_world_characters_push_records_device(NULL, &ptr, &n) != BGE_ERR_INVALID) return 8;
    if (bge_last_error()[0] == '\0') return 9;
    printf("impulse abi ok\n");
    return 0;
}
