#ifndef IVLN_MAP_SEED_H
#define IVLN_MAP_SEED_H
#include "ivln_hip.h"
#include "ivln_known_lib.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Seeding an iterative mapper (csrc/mapper.hip) - an extension of include/ivln_hip.h, whose declarations are pinned, and
 * the way back from include/ivln_map_build.h: rows of the world cloud are dropped and pre-built points are appended
 * between steps, and the next ivln_mapper_step* maps on top of them.  Together with ivln_mapper_world_export this saves
 * and restores a mapper, and starts a row from a known scene.
 *
 * Order contract (the reference's cloud is a sequence; here it is a bag ordered by rank).  ivln_mapper_rows_clear is
 * clear_completed_episode_data (mapper.py:310-326): survivors keep their ranks.  ivln_mapper_env_append* is a
 * concatenation behind the cloud (mapper.py:871-879): the new points come behind every point now in the cloud, keep the
 * given order among themselves, later calls come behind earlier ones, and all of them come in front of the local points
 * of any later step.  Ties of cell and height in the next keep-highest go to the first in that order.
 *
 * Rank band.  Between complete steps a resident point's rank is its key, < table_cells; a step's local points carry bit
 * 31.  Appended points take ranks from [table_cells, 2^31), handed out by a counter in the handle that only grows and that
 * ivln_mapper_reset rewinds; a call that would leave the band returns IVLN_E_KEYSPACE before any launch (a handle whose
 * table_cells is 2^31 has no band).  The next complete step turns every rank into a key again.  Until then the ranks of
 * appended points are not keys: ivln_mapper_env_export and ivln_known_lib_add_from_mapper answer IVLN_E_UNSUPPORTED for a
 * row that holds any.  ivln_mapper_env_counts and ivln_mapper_world_export report the new state at once.
 *
 * Boxes.  A step takes the cell box of the surviving old cloud from per-env box partials instead of a pass over the
 * cloud, and the multipliers of a key are the extent of that box (quirks Q1 / Q2): a box that is merely large enough
 * changes which points collide.  These calls keep the partials exact - a dropped row's partials become empty, the exact
 * box (cell_index(z), cell_index(x)) of appended points is folded into their row's, other rows are untouched; a handle
 * that has never stepped gets its partials initialised, and a row at or beyond the partials' width widens them.
 *
 * The calls are valid only between complete steps (not between ivln_mapper_step_begin and its _finish), on the stream the
 * steps run on, and must not run while it is capturing.  They leave the arg-max table and the cell winners all zero.
 * Integer work only, no workgroup waits on another: two runs give the same cloud and the same maps.
 * Refused before any launch with nothing written:
 *   IVLN_E_INVALID      NULL m, b outside [0, B_max), B outside [1, B_max], n < 0, NULL keep, NULL xyz / sem with n > 0,
 *                       NULL lib, a scene index that was never added
 *   IVLN_E_UNSUPPORTED  a mapper with a library attached (ivln_mapper_known_attach) or one that holds
 *                       ivln_mapper_load_known points (their ranks are another host counter)
 *   IVLN_E_KEYSPACE     the rank band is exhausted
 *   IVLN_E_CAPACITY     the cloud would exceed world_capacity (ivln_mapper_env_append*: one read-back of the count,
 *                       which synchronises `stream`)
 * ------------------------------------------------------------------------------------------ */

/* Drops every point of a row b with keep[b] == 0 and of every row >= B; keep: device memory, B bytes.  Two launches, no
 * synchronisation. */
int ivln_mapper_rows_clear(ivln_mapper* m, const uint8_t* keep, int B, void* stream);

/* Appends n points - xyz f32 (n, 3) and sem u8 (n), device memory, file order - to row b with meta = b << 8 | label.
 * n == 0 is IVLN_OK and does nothing.  One read-back (synchronises), then two launches whose geometry depends on n and
 * B_max only. */
int ivln_mapper_env_append(ivln_mapper* m, int b, const float* xyz, const uint8_t* sem, int64_t n, void* stream);

/* The same append read from the 16-byte records of scene `scene` of a library (one 16-byte load per point, no host copy of
 * the points).  The scene may have been added after the mapper was created. */
int ivln_mapper_env_append_from_lib(ivln_mapper* m, int b, const ivln_known_lib* lib, int scene, void* stream);

#ifdef __cplusplus
}
#endif
#endif
