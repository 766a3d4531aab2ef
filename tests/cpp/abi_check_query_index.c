/* The query-index part of the C ABI (include/bge_world.h "Query index": bge_world_set_query_index, bge_world_query_index_stats):
 * compiles as C99 (no C++), the two structs have their stated sizes and offsets, and the entry points link and refuse a NULL
 * world. */
#include <stdio.h>
#include <string.h>

#include "../../include/bge_world.h"

typedef char desc_is_24_bytes[(sizeof(bge_query_index_desc) == 24) ? 1 : -1];
typedef char desc_mode_at_0[(offsetof(bge_query_index_desc, mode) == 0) ? 1 : -1];
typedef char desc_cell_edge_at_4[(offsetof(bge_query_index_desc, cell_edge) == 4) ? 1 : -1];
typedef char desc_max_cells_at_8[(offsetof(bge_query_index_desc, max_cells) == 8) ? 1 : -1];
typedef char desc_reserved_at_12[(offsetof(bge_query_index_desc, reserved) == 12) ? 1 : -1];
typedef char desc_min_work_at_16[(offsetof(bge_query_index_desc, min_work) == 16) ? 1 : -1];
typedef char stats_is_64_bytes[(sizeof(bge_query_index_stats) == 64) ? 1 : -1];
typedef char stats_built_at_0[(offsetof(bge_query_index_stats, built) == 0) ? 1 : -1];
typedef char stats_table_size_at_4[(offsetof(bge_query_index_stats, table_size) == 4) ? 1 : -1];
typedef char stats_bodies_indexed_at_8[(offsetof(bge_query_index_stats, bodies_indexed) == 8) ? 1 : -1];
typedef char stats_bodies_wide_at_16[(offsetof(bge_query_index_stats, bodies_wide) == 16) ? 1 : -1];
typedef char stats_queries_indexed_at_24[(offsetof(bge_query_index_stats, queries_indexed) == 24) ? 1 : -1];
typedef char stats_queries_far_at_32[(offsetof(bge_query_index_stats, queries_far) == 32) ? 1 : -1];
typedef char stats_cell_edge_at_40[(offsetof(bge_query_index_stats, cell_edge) == 40) ? 1 : -1];
typedef char stats_reserved_at_44[(offsetof(bge_query_index_stats, reserved) == 44) ? 1 : -1];
typedef char stats_builds_at_48[(offsetof(bge_query_index_stats, builds) == 48) ? 1 : -1];
typedef char stats_reserved2_at_56[(offsetof(bge_query_index_stats, reserved2) == 56) ? 1 : -1];

int main(void)
{
    bge_query_index_desc desc;
    bge_query_index_stats stats;
    memset(&desc, 0, sizeof desc);
    memset(&stats, 0, sizeof stats);
    desc.mode = 1;
    desc.min_work = BGE_QUERY_INDEX_MIN_WORK_DEFAULT;
    if (BGE_QUERY_INDEX_MIN_WORK_DEFAULT == 0) return 1;
    if (bge_world_set_query_index(NULL, &desc) != BGE_ERR_INVALID) return 2;
    if (bge_world_set_query_index(NULL, NULL) != BGE_ERR_INVALID) return 3;
    if (bge_world_query_index_stats(NULL, &stats) != BGE_ERR_INVALID) return 4;
    if (bge_last_error()[0] == '\0') return 5;
    printf("query index abi ok\n");
    return 0;
}
