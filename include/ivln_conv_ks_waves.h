#ifndef IVLN_CONV_KS_WAVES_H
#define IVLN_CONV_KS_WAVES_H
#include "ivln_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * The wave count of the split-bf16 K-split-over-waves conv kernels (csrc/conv_bf3.hip: k_conv_bf3_ks, the K-split form of
 * k_conv1x1_bf3_ks) - an extension of include/ivln_hip.h, whose declarations are pinned: entry points added after that
 * pin are declared in a header of their own.
 *
 * Both kernels run with eight waves per workgroup (one workgroup per CU) or with four (two co-resident workgroups per CU:
 * the grids of more workgroups than CUs and at most twice as many, which eight waves run as two rounds).  Without a pin the
 * launchers choose (bf3_ks_four_waves); ivln_gemm_desc.tile_override pins the count for tests and tuning, beside the
 * values ivln_hip.h lists: 16 | 17 = k_conv_bf3_ks on its 64-pixel tiles (3x3 and the stacked 2 x 2 transposed form) with
 * 8 | 4 waves, 18 | 19 = the K-split form of k_conv1x1_bf3_ks with 8 | 4 waves (IVLN_E_UNSUPPORTED when not eligible).
 * The sum over K is a fixed-order sum of 8 | 4 partial tiles: the same bytes on every run of one form, not across forms.
 * ------------------------------------------------------------------------------------------ */

/* Launches of the two kernels by wave count since the last reset (host side, at enqueue, like ivln_conv_split_kinds, whose
 * counters [1] and [2] include them): out4 = k_conv_bf3_ks with 8 waves, with 4, k_conv1x1_bf3_ks' K-split form with 8
 * waves, with 4. */
int ivln_conv_ks_waves(long long* out4, int reset);

#ifdef __cplusplus
}
#endif
#endif
