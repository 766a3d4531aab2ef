/* The character part of the C ABI (include/bge_world.h bge_world_characters_*): compiles as C99 (no C++), the records have their
 * stated sizes and offsets, the flag words their values, and the entry points link and refuse a NULL world. */
#include <stdio.h>
#include <string.h>

#include "../../include/bge_world.h"

typedef char bge_character_desc_is_48_bytes[(sizeof(bge_character_desc) == 48) ? 1 : -1];
typedef char bge_character_desc_radius_at_12[(offsetof(bge_character_desc, radius) == 12) ? 1 : -1];
typedef char bge_character_desc_skin_at_16[(offsetof(bge_character_desc, skin) == 16) ? 1 : -1];
typedef char bge_character_desc_step_height_at_20[(offsetof(bge_character_desc, step_height) == 20) ? 1 : -1];
typedef char bge_character_desc_slope_at_24[(offsetof(bge_character_desc, min_ground_ny) == 24) ? 1 : -1];
typedef char bge_character_desc_probe_at_28[(offsetof(bge_character_desc, probe_distance) == 28) ? 1 : -1];
typedef char bge_character_desc_gravity_at_32[(offsetof(bge_character_desc, gravity) == 32) ? 1 : -1];
typedef char bge_character_desc_jump_speed_at_36[(offsetof(bge_character_desc, jump_speed) == 36) ? 1 : -1];
typedef char bge_character_desc_fall_speed_at_40[(offsetof(bge_character_desc, fall_speed) == 40) ? 1 : -1];
typedef char bge_character_desc_mask_at_44[(offsetof(bge_character_desc, layer_mask) == 44) ? 1 : -1];
typedef char bge_character_input_is_16_bytes[(sizeof(bge_character_input) == 16) ? 1 : -1];
typedef char bge_character_input_walk_z_at_4[(offsetof(bge_character_input, walk_z) == 4) ? 1 : -1];
typedef char bge_character_input_buttons_at_8[(offsetof(bge_character_input, buttons) == 8) ? 1 : -1];
typedef char bge_character_state_is_80_bytes[(sizeof(bge_character_state) == 80) ? 1 : -1];
typedef char bge_character_state_vv_at_12[(offsetof(bge_character_state, vertical_velocity) == 12) ? 1 : -1];
typedef char bge_character_state_flags_at_16[(offsetof(bge_character_state, flags) == 16) ? 1 : -1];
typedef char bge_character_state_ground_kind_at_20[(offsetof(bge_character_state, ground_kind) == 20) ? 1 : -1];
typedef char bge_character_state_ground_entity_at_24[(offsetof(bge_character_state, ground_entity) == 24) ? 1 : -1];
typedef char bge_character_state_ground_normal_at_28[(offsetof(bge_character_state, ground_normal) == 28) ? 1 : -1];
typedef char bge_character_state_hit_kind_at_40[(offsetof(bge_character_state, hit_kind) == 40) ? 1 : -1];
typedef char bge_character_state_hit_entity_at_44[(offsetof(bge_character_state, hit_entity) == 44) ? 1 : -1];
typedef char bge_character_state_hit_normal_at_48[(offsetof(bge_character_state, hit_normal) == 48) ? 1 : -1];
typedef char bge_character_state_step_rise_at_60[(offsetof(bge_character_state, step_rise) == 60) ? 1 : -1];
typedef char bge_character_state_recovered_at_64[(offsetof(bge_character_state, recovered) == 64) ? 1 : -1];
typedef char bge_character_state_steps_at_76[(offsetof(bge_character_state, steps) == 76) ? 1 : -1];

int main(void)
{
    bge_character_desc desc;
    bge_character_input input;
    bge_character_state state;
    void* ptr = NULL;
    uint64_t n = 0;
    uint32_t index = 0;
    float at[3] = {0.0f, 1.0f, 0.0f};
    memset(&desc, 0, sizeof desc);
    memset(&input, 0, sizeof input);
    desc.radius = 0.5f;
    desc.skin = 0.01f;
    desc.fall_speed = 30.0f;
    desc.layer_mask = 1u;
    input.buttons = BGE_CHAR_BUTTON_JUMP;
    if (BGE_CHAR_INVALID != 1 || BGE_CHAR_GROUNDED != 2 || BGE_CHAR_JUMPED != 4 || BGE_CHAR_LANDED != 8 || BGE_CHAR_HEAD_BUMP != 16) return 1;
    if (BGE_CHAR_RECOVERED != 32 || BGE_CHAR_STUCK != 64 || BGE_CHAR_STEPPED != 128 || BGE_CHAR_OUT_OF_SLIDES != 256) return 2;
    if (BGE_CHAR_BUTTON_JUMP != 1) return 3;
    if (bge_world_characters_create(NULL, 1, &desc) != BGE_ERR_INVALID) return 4;
    if (bge_world_characters_set_input(NULL, 0, 1, &input) != BGE_ERR_INVALID) return 5;
    if (bge_world_characters_set_input_device(NULL, 0, 1, NULL) != BGE_ERR_INVALID) return 6;
    if (bge_world_characters_warp(NULL, 1, &index, at) != BGE_ERR_INVALID) return 7;
    if (bge_world_characters_update(NULL, 0.01f, 1) != BGE_ERR_INVALID) return 8;
    if (bge_world_characters_download(NULL, 0, 1, &state) != BGE_ERR_INVALID) return 9;
    if (bge_world_characters_state_device(NULL, &ptr, &n) != BGE_ERR_INVALID) return 10;
    if (bge_last_error()[0] == '\0') return 11;
    printf("character abi ok\n");
    return 0;
}
