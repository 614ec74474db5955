#ifndef IVLN_MAPPER_DEBUG_H
#define IVLN_MAPPER_DEBUG_H
#include "ivln_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Test-only view of the iterative mapper's state that outlives a call (csrc/mapper.hip - an extension of
 * include/ivln_hip.h, whose declarations are pinned: entry points added after that pin are declared in a header of their
 * own).  The step's correctness rests on one invariant: between complete calls the keep-highest arg-max table (tab64) and
 * the per-cell raster words (cell) are all zero - the winners of a pass clear their own slots, k_finalize clears the
 * cells, the builder's scatter clears its marks.  Nothing of the product path reads it back; this call does.
 * ------------------------------------------------------------------------------------------ */

/* out[0] = non-zero slots of the arg-max table, out[1] = non-zero raster words, counted behind everything enqueued on
 * `stream` so far.  [0, 0] after every complete call (a step, an export, a reset - also one that raised IVLN_E_KEYSPACE or
 * IVLN_E_CAPACITY); out[0] > 0 between an ivln_mapper_step_begin and its _finish.  Two launches and a 16-byte scratch
 * that is freed before the call returns; synchronises the stream; not to be called under stream capture.
 * IVLN_E_INVALID: a NULL argument. */
int ivln_mapper_debug_nonzero(ivln_mapper* m, int64_t out[2], void* stream);

#ifdef __cplusplus
}
#endif
#endif
