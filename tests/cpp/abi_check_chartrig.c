/* The character-trigger part of the C ABI (include/bge_world.h "Character trigger events"): compiles as C99 (no C++), the record
 * has its stated size and offsets, the enum and flag words their values, and the entry points link and refuse a NULL world. */
#include <stdio.h>
#include <string.h>

#include "../../include/bge_world.h"

typedef char bge_character_trigger_event_is_12_bytes[(sizeof(bge_character_trigger_event) == 12) ? 1 : -1];
typedef char bge_character_trigger_event_type_at_0[(offsetof(bge_character_trigger_event, type) == 0) ? 1 : -1];
typedef char bge_character_trigger_event_trigger_at_4[(offsetof(bge_character_trigger_event, trigger) == 4) ? 1 : -1];
typedef char bge_character_trigger_event_character_at_8[(offsetof(bge_character_trigger_event, character) == 8) ? 1 : -1];

int main(void)
{
    bge_character_trigger_event event;
    void* events = NULL;
    void* count = NULL;
    uint64_t capacity = 0, total = 0;
    uint32_t group = 2u, mask = 0xffffffffu, entity = 0u, pair[2] = {0u, 0u};
    float box[6];
    uint8_t listed = 0;
    memset(&event, 0, sizeof event);
    if (BGE_CHAR_TRIGGER_ENTER != 0 || BGE_CHAR_TRIGGER_STAY != 1 || BGE_CHAR_TRIGGER_EXIT != 2) return 1;
    if (BGE_CHAR_TRIGGER_STAY_EVENTS != 1) return 2;
    if (bge_world_characters_watch_triggers(NULL, 1, &group, &mask, BGE_CHAR_TRIGGER_STAY_EVENTS, 0) != BGE_ERR_INVALID) return 3;
    if (bge_world_characters_trigger_events(NULL, &event, 1, &total) != BGE_ERR_INVALID) return 4;
    if (bge_world_characters_trigger_events_device(NULL, &events, &count, &capacity) != BGE_ERR_INVALID) return 5;
    if (bge_world_characters_trigger_overlaps(NULL, 1, pair, &total) != BGE_ERR_INVALID) return 6;
    if (bge_world_characters_set_trigger_overlaps(NULL, 1, pair) != BGE_ERR_INVALID) return 7;
    if (bge_world_trigger_boxes(NULL, 1, &entity, box, &listed) != BGE_ERR_INVALID) return 8;
    if (bge_last_error()[0] == '\0') return 9;
    printf("chartrig abi ok\n");
    return 0;
}
