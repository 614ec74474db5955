#ifndef IVLN_TEXT_FEAT_H
#define IVLN_TEXT_FEAT_H
#include "ivln_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Instruction encoder over pre-computed text features: MODEL.INSTRUCTION_ENCODER.sensor_uuid other than "instruction"
 * (csrc/text_feat.hip) - an extension of include/ivln_hip.h, whose declarations are pinned (tests/test_state_rnn_host.py
 * hashes its code): entry points added after that pin are declared in a header of their own.
 * The reference builds no embedding layer for such a sensor and reads observations["rxr_instruction"], a (B, L, E) float
 * tensor (models/encoders/instruction_encoder.py:34-45, 70-78).  All fp32.  No float atomics: two runs give the same bytes.
 * ------------------------------------------------------------------------------------------ */
/* 32-bit words of scratch the front kernel wants for B sequences (2 per sequence: one 8-byte aligned 64-bit word holding
 * row count, difference count and ticket).  The caller zeroes them ONCE; every launch leaves them zero again, so a captured
 * graph replays without a host-side reset.  One launch in flight per scratch buffer. */
int64_t ivln_text_feat_ws_words(int B);
/* Front end of the feature path.  feat (B, L, E) contiguous.
 *   lengths[b] (int32) = the NUMBER of rows t of sequence b with at least one element != 0.0f - the reference's
 *   (x != 0).sum(2) then (. != 0).sum(1) (:77-78): a count, not the index of the last such row.  -0.0f is zero, a NaN
 *   element is non-zero.
 * cache_feat (B, L, E), valid (B) int32, dirty (B) int32: all three given (rollout steps) or all three NULL.  With them
 *   dirty[b] = 1 when valid[b] == 0 or any 32-bit word of sequence b differs bitwise from cache_feat[b]; then cache_feat[b]
 *   takes the new features, valid[b] = 1 and lengths[b] is written.  dirty[b] = 0 otherwise and cache_feat[b] / lengths[b]
 *   keep their bytes - the contract ivln_embed_gates_dirs_f32 has for tokens.
 * A sequence is split over ceil(L / rows-per-workgroup) workgroups (a wave per row); their row counts and difference flags
 * meet in `ws` through one 64-bit integer atomic add each; the workgroup that arrives last writes the sequence's results
 * and re-arms `ws`.
 * 16-byte loads and stores when E % 4 == 0 and feat / cache_feat are 16-byte aligned, else 4-byte ones.
 * IVLN_E_INVALID: NULL feat / lengths / ws, ws not 8-byte aligned, non-positive B / L / E, a partial set of the three cache
 * pointers, a sequence of 2^31 words and more.  Nothing is launched on a refusal. */
int ivln_text_feat_front_f32(const float* feat, int B, int L, int E, int* lengths, float* cache_feat, int* valid, int* dirty,
                             int* ws, void* stream);
/* Gate projection of the feature path: gx[(b*L + t)][g] = feat[b][t] . w[g] + bias[g] for the sequences with dirty[b] != 0
 * (dirty NULL: all of them); rows of the others keep their bytes.  feat (B, L, E), w (G, E), bias (G) or NULL, gx (B*L, G).
 * fp32 in, fp32 out on the fp32 MFMA (ivln_gemm_f32 takes per-image run flags only for NCHW destinations), one launch of
 * 64 x 64 tiles; a tile whose rows all belong to clean sequences returns before its first load.
 * IVLN_E_INVALID: NULL feat / w / gx, non-positive sizes, B * L rows of 2^31 and more. */
int ivln_text_feat_gates_f32(const float* feat, int B, int L, int E, const float* w, const float* bias, int G,
                             const int* dirty, float* gx, void* stream);

#ifdef __cplusplus
}
#endif
#endif
