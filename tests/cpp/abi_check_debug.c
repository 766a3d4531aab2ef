/* The debug-overlay part of the C ABI (include/bge_world.h bge_world_debug_lines*) seen from C99: the line record is the
 * reference's 28-byte PhysicsDebugLine, field by field, the flags have their stated values, and the entry points link and
 * refuse a NULL world. */
#include <stddef.h>
#include <stdio.h>

#include "../../include/bge_world.h"

typedef char bge_debug_line_is_28_bytes[(sizeof(bge_debug_line) == 28) ? 1 : -1];
typedef char bge_debug_line_from_at_0[(offsetof(bge_debug_line, from) == 0) ? 1 : -1];
typedef char bge_debug_line_to_at_12[(offsetof(bge_debug_line, to) == 12) ? 1 : -1];
typedef char bge_debug_line_abgr_at_24[(offsetof(bge_debug_line, abgr) == 24) ? 1 : -1];
typedef char bge_debug_desc_is_36_bytes[(sizeof(bge_debug_desc) == 36) ? 1 : -1];

int main(void)
{
    bge_debug_line line;
    uint64_t total = 7;
    if (bge_world_debug_lines(NULL, NULL, &line, 1, &total) != BGE_ERR_INVALID) return 2;
    if (bge_world_debug_lines_device(NULL, NULL, NULL, 0, NULL) != BGE_ERR_INVALID) return 3;
    if (bge_last_error()[0] == '\0') return 4;
    if (BGE_DEBUG_SHAPES != 1 || BGE_DEBUG_CONTACTS != 2 || BGE_DEBUG_ALL != 3) return 1;
    printf("debug abi ok\n");
    return 0;
}
