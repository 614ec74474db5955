#ifndef IVLN_MAP_BUILD_H
#define IVLN_MAP_BUILD_H
#include "ivln_hip.h"
#include "ivln_known_lib.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Known-map builder: from the cloud an iterative mapper explored to a known scene (csrc/mapper.hip) - an extension of
 * include/ivln_hip.h, whose declarations are pinned.  Known-map mode reads {maps_location}/{scene}.npz (keys xyz,
 * semantics; mapper.py:283-294); these calls produce the arrays of such a file, per env and in the reference's cloud order,
 * or enter them straight into a device-resident scene library (include/ivln_known_lib.h).
 *
 * Order contract.  After a completed step every point of the world cloud carries rank == its key in that step's
 * keep-highest (k_world_select); keys are unique and < table_cells, the env of a point is meta >> 8, and the reference's
 * cloud restricted to one env is ascending rank (what MappingModule.world_cloud() returns by a stable host argsort).  All
 * three calls are defined by that order.
 *
 * Method.  One launch takes per env {count, lowest key, highest key}.  The points of env b then mark their (unique) slot
 * key - lowest in a dense table - the mapper's own arg-max table, which is all zero between steps and is all zero again
 * behind the last launch of the call - , an exclusive scan of the marks gives every point its place, and a last launch
 * moves the points there.  The scan is count tiles / scan the partials / scatter, each level a launch of its own: no
 * workgroup ever waits on another one inside a launch, integer work only, two runs give the same bytes.
 *
 * The calls are valid only between complete steps: after ivln_mapper_step_begin without its _finish the result is
 * undefined (the ranks are not keys yet and the table is in use; memory outside the given buffers is still never
 * written).  They synchronise `stream` once (the read-back of the counts) and must not run while it is capturing.  The
 * first of them allocates the scratch of all three in the mapper handle (the partials of the counts and the scan's levels,
 * about table_cells / 64 bytes; freed by ivln_mapper_destroy).
 * IVLN_E_UNSUPPORTED: the cloud holds points from ivln_mapper_load_known - their ranks are a host counter, not keys.
 * ------------------------------------------------------------------------------------------ */

/* counts_host[b] (host memory, B entries) = points of env b in the current cloud, b < B.  One launch plus one read-back;
 * synchronises `stream`.  IVLN_E_INVALID, before the launch: NULL m / counts_host, B outside [1, B_max]. */
int ivln_mapper_env_counts(ivln_mapper* m, int B, int64_t* counts_host, void* stream);

/* Env b's points in ascending rank, compacted on the device: xyz f32 (max_n, 3) and sem u8 (max_n) are device memory and
 * receive rows [0, n) - already in file order; *n_out (host) = n.
 * Refused before any launch, nothing written: IVLN_E_INVALID for a NULL m / n_out, b outside [0, B_max), max_n < 0, and
 * with max_n > 0 a NULL xyz / sem; IVLN_E_UNSUPPORTED as above.  IVLN_E_CAPACITY: max_n < n - *n_out still receives n,
 * the buffers are not touched. */
int ivln_mapper_env_export(ivln_mapper* m, int b, float* xyz, uint8_t* sem, int64_t max_n, int64_t* n_out, void* stream);

/* The same ordered compaction written as the library's 16-byte records (x, y, z, label as uint32) into `records`
 * (caller-owned device memory of 16 * max_n bytes on a 16-byte boundary that must outlive the library), and the table
 * entry {records, n, present} of scene `scene` written from the device behind them, as ivln_known_lib_add does: no host
 * copy of the points is made, and a graph captured earlier sees the scene on its next replay behind this call.
 * Refused before any launch, nothing written: IVLN_E_INVALID for a NULL lib / m, a scene index ivln_known_lib_add would
 * refuse (outside [0, max_scenes), added before), b outside [0, B_max), max_n < 0, and with max_n > 0 NULL records or
 * records off a 16-byte boundary; IVLN_E_UNSUPPORTED as above.  IVLN_E_CAPACITY: max_n smaller than env b's count
 * (ivln_mapper_env_counts) - nothing is written and the scene is not entered. */
int ivln_known_lib_add_from_mapper(ivln_known_lib* lib, int scene, ivln_mapper* m, int b, void* records, int64_t max_n,
                                   void* stream);

#ifdef __cplusplus
}
#endif
#endif
