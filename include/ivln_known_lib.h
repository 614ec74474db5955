#ifndef IVLN_KNOWN_LIB_H
#define IVLN_KNOWN_LIB_H
#include "ivln_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Known-map mode without copies: a device-resident scene library and a step that can be captured in a hipGraph
 * (csrc/mapper.hip) - an extension of include/ivln_hip.h, whose declarations are pinned: entry points added after that pin
 * are declared in a header of their own.
 * In known-map mode the cloud of a batch row is always exactly one file: a row is cleared when its episode finishes and
 * reloaded from {maps_location}/{env_name}.npz in the same step (mapper.py:851-881), and a row at or above the current batch
 * size is cleared (mapper.py:315-318).  So the device needs each scene once and one latched scene index per row; nothing is
 * copied per step or per reset.  ivln_mapper_known_begin / _load_known / _known_raster (the copy path) stay what they are.
 * No float atomics, no host read inside the step: two runs give the same bytes, and the step replays from a graph.
 * ------------------------------------------------------------------------------------------ */
typedef struct ivln_known_lib ivln_known_lib;

/* A table of max_scenes entries {records, n, present} at a device address that never changes, all entries absent.
 * IVLN_E_INVALID: max_scenes <= 0 or > 2^20, NULL out. */
int ivln_known_lib_create(int max_scenes, ivln_known_lib** out);
/* Frees the table.  The records belong to the caller.  Mappers the library is attached to must not step afterwards. */
int ivln_known_lib_destroy(ivln_known_lib* lib);
/* Packs scene `scene` once: xyz f32 (n, 3) + sem u8 (n) -> records[i] = (x, y, z, label as uint32), 16 bytes each, in file
 * order, and writes the scene's table entry from the device behind them - one launch on `stream`.  `records` is caller-owned
 * device memory of 16 * n bytes on a 16-byte boundary that must outlive the library; xyz / sem may be released once the
 * launch has run.  The table address and the records of older scenes do not move, so a graph captured before this call sees
 * the new scene when it is replayed behind it on the stream.
 * IVLN_E_INVALID, before anything is launched: NULL lib, scene outside [0, max_scenes), a scene that was added before, n < 0,
 * n >= 2^31, and with n > 0 a NULL xyz / sem / records or records off a 16-byte boundary. */
int ivln_known_lib_add(ivln_known_lib* lib, int scene, const float* xyz, const uint8_t* sem, int64_t n, void* records,
                       void* stream);
/* Number of scenes added so far (host-side bookkeeping), or IVLN_E_INVALID for a NULL lib. */
int ivln_known_lib_size(ivln_known_lib* lib);

/* The library this mapper's known steps read; allocates the mapper's latches cur[B_max] (all -1: no scene) on the first
 * call.  The library must outlive the mapper's steps.  Not to be called while a stream is capturing. */
int ivln_mapper_known_attach(ivln_mapper* m, ivln_known_lib* lib);
/* One known-map step, 3 launches whose geometry depends on B and the map size only:
 *   latch     cur[b] = scene_id[b] where not_done[b] == 0 (b < B), cur[b] = -1 for B <= b < B_max (a paused row is cleared);
 *             cur lives in the handle across calls and graph replays, ivln_mapper_reset sets it to -1.  The same launch
 *             derives the ego rotation of row b from orientation[b] (the bits of ivln_mapper_frames) and zeroes occ_out.
 *   raster    grid (workgroups per row, B): row b rasters the records of scene cur[b] with rank = index in the file, so
 *             ties stay last-writer-wins in file order (integer atomicMax per map cell).  cur[b] == -1 rasters nothing.
 *             Any other index without a table entry sets the sticky status IVLN_E_INVALID (ivln_mapper_status) and rasters
 *             nothing for that row; no memory is read through it.
 *   finalise  the per-cell winners -> sem_out.
 * scene_id i32 (B), pose f32 (B, 3), orientation f64 (B, 2) [elevation, heading], not_done u8 (B), occ_out / sem_out u8
 * (B, rows, cols): all device memory.  IVLN_E_INVALID: NULL operand, no library attached, B outside [1, B_max]. */
int ivln_mapper_known_step(ivln_mapper* m, const int32_t* scene_id, const float* pose, const double* orientation,
                           const uint8_t* not_done, int B, uint8_t* occ_out, uint8_t* sem_out, void* stream);
/* Synchronises `stream`; *n = sum over b < B of the sizes of the latched scenes - the world size the copy path reports
 * for the same history (rows with no valid scene count 0). */
int ivln_mapper_known_count(ivln_mapper* m, int B, int64_t* n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
