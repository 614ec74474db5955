#ifndef IVLN_MAP_SIZES_H
#define IVLN_MAP_SIZES_H
#include "ivln_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Egocentric maps other than 64 x 64 cells (EGOCENTRIC_MAPPER.height_meters / width_meters / resolution_meters): the map
 * CNN leaves (rows / 16) * (cols / 16) key positions, the depth encoder keeps its 16, so the two short attentions of the
 * rollout head no longer share one key count - an extension of include/ivln_hip.h, whose declarations are pinned: entry
 * points added after that pin are declared in a header of their own.
 * ------------------------------------------------------------------------------------------ */

/* ivln_attn_small2_f32 with a key count per set: out_s[n, :] = softmax_i(scale * q[n, :Ck_s] . k_s[n, :, i]) . v_s[n, :, i]
 * for the sets s = 0, 1 in ONE launch (csrc/nn_ops.hip k_attn_pair).  The sets share q (rows, ldq) and scale; k_s (rows,
 * Ck_s, I_s) and v_s (rows, Cv_s, I_s) are channel-major with image strides; out_s (rows, Cv_s) is a column slice of rows
 * ldo_s wide.  k1 == NULL: set 0 alone (the other arguments of set 1 are not read).
 * Fixed summation and softmax-reduction orders and no atomics: two runs give the same bytes.
 * IVLN_E_UNSUPPORTED, before anything is launched: rows <= 0, a key count outside [1, 256], Ck_s outside [1, 1024],
 * Cv_s <= 0. */
int ivln_attn_pair_f32(const float* q, int64_t ldq, float scale, int rows, const float* k0, int64_t k0_img_stride,
                       const float* v0, int64_t v0_img_stride, int Ck0, int Cv0, int I0, float* out0, int64_t ldo0,
                       const float* k1, int64_t k1_img_stride, const float* v1, int64_t v1_img_stride, int Ck1, int Cv1,
                       int I1, float* out1, int64_t ldo1, void* stream);

#ifdef __cplusplus
}
#endif
#endif
