/* The platform-riding part of the C ABI (include/bge_world.h bge_world_characters_ride ..): compiles as C99 (no C++), the record has
 * its stated size and offsets, the flag words their values, and the entry points link and refuse a NULL world. */
#include <stdio.h>
#include <string.h>

#include "../../include/bge_world.h"

typedef char bge_character_ride_is_64_bytes[(sizeof(bge_character_ride) == 64) ? 1 : -1];
typedef char bge_character_ride_flags_at_0[(offsetof(bge_character_ride, flags) == 0) ? 1 : -1];
typedef char bge_character_ride_entity_at_4[(offsetof(bge_character_ride, entity) == 4) ? 1 : -1];
typedef char bge_character_ride_anchor_position_at_8[(offsetof(bge_character_ride, anchor_position) == 8) ? 1 : -1];
typedef char bge_character_ride_anchor_rotation_at_20[(offsetof(bge_character_ride, anchor_rotation) == 20) ? 1 : -1];
typedef char bge_character_ride_carried_at_36[(offsetof(bge_character_ride, carried) == 36) ? 1 : -1];
typedef char bge_character_ride_turn_at_48[(offsetof(bge_character_ride, turn) == 48) ? 1 : -1];

int main(void)
{
    bge_character_ride ride;
    void* ptr = NULL;
    uint64_t n = 0;
    memset(&ride, 0, sizeof ride);
    if (BGE_CHAR_RIDE_ON != 1 || BGE_CHAR_RIDE_DYNAMIC != 2) return 1;
    if (BGE_CHAR_RIDE_CARRIED != 1 || BGE_CHAR_RIDE_LOST != 2) return 2;
    if (bge_world_characters_ride(NULL, BGE_CHAR_RIDE_ON) != BGE_ERR_INVALID) return 3;
    if (bge_world_characters_rides(NULL, 0, 1, &ride) != BGE_ERR_INVALID) return 4;
    if (bge_world_characters_rides_device(NULL, &ptr, &n) != BGE_ERR_INVALID) return 5;
    if (bge_last_error()[0] == '\0') return 6;
    printf("ride abi ok\n");
    return 0;
}
