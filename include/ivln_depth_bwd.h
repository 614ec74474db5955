#ifndef IVLN_DEPTH_BWD_H
#define IVLN_DEPTH_BWD_H
#include "ivln_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Backward of the DD-PPO depth ResNet: MODEL.DEPTH_ENCODER.trainable (csrc/depth_bwd.hip) - an extension of
 * include/ivln_hip.h, whose declarations are pinned (tests/test_state_rnn_host.py hashes its code): like
 * include/ivln_rednet_glue.h, entry points added after that pin are declared in a header of their own.
 * The reference sets requires_grad on the encoder's parameters (models/encoders/resnet_encoders.py:31-43), stops feeding
 * cached `depth_features` (:95) and lets autograd train it.  Here the conv gradients are GEMMs (ivln_gemm_f32); these are
 * the kernels between them.  All fp32, NCHW contiguous.  No float atomics: two runs give the same bits.
 * ------------------------------------------------------------------------------------------ */
/* Backward of GroupNorm (+ the ReLU that follows the block).  dy, x (N, C, HW): the upstream gradient and the RAW input
 * the forward normalised; mean / rstd (N * groups) as ivln_groupnorm_f32 saved them; gamma (C); out (N, C, HW) or NULL:
 * the block's activated output - with it dz = dy * (out > 0), without it dz = dy.
 *   xh = (x - mean) * rstd;  dx = rstd * (gamma * dz - mean_g(gamma * dz) - xh * mean_g(gamma * dz * xh))
 *   dgamma[c] = sum_{n,hw} dz * xh;  dbeta[c] = sum_{n,hw} dz
 * (mean_g: over the channels of the group and HW of one image).  dz_out (N, C, HW) or NULL receives dz: a bottleneck tail
 * relu(GN(c3) + GN_ds(ds)) or relu(GN(c3) + identity) needs it three times, the second call takes it as dy with out NULL.
 * One workgroup per (image, group); per-image partials of dgamma / dbeta in ws (>= 2 * N * C floats) are summed over the
 * images in ascending order by a second launch.  16-byte accesses when HW % 4 == 0 and dy / x / out / dx / dz_out are
 * 16-byte aligned, else 4-byte accesses with the same values.  IVLN_E_INVALID: a NULL operand other than out / dz_out,
 * C % groups != 0, non-positive sizes, ws too small; IVLN_E_UNSUPPORTED: more than 1024 channels per group (the sums' LDS
 * arrays) or a group of 2^31 elements and more.  Nothing is launched on a refusal. */
int ivln_groupnorm_bwd_f32(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                           const float* out, int N, int C, int HW, int groups, float* dx, float* dz_out, float* dgamma,
                           float* dbeta, float* ws, int64_t ws_floats, void* stream);
/* Backward of nn.MaxPool2d(3, 2, 1) over `planes` = N * C planes: x (planes, H, W) the saved input, dy (planes, Ho, Wo)
 * with Ho = (H - 1) / 2 + 1 -> dx (planes, H, W).  Gather form: an input pixel sums, in ascending window order, the
 * gradients of the at most 4 windows in which it is the first maximum in row-major order (torch's rule, NaN included). */
int ivln_maxpool3s2_bwd_f32(const float* dy, const float* x, int planes, int H, int W, float* dx, void* stream);
/* W (O, I, KK) -> (I, O, KK), taps in place: the layout the transposed-conv GEMM (IVLN_B_CONVT) reads, so that the input
 * gradient of a stride-2 conv is conv_transpose(dy, W) with output padding 1. */
int ivln_weight_oi_transpose_f32(const float* w, float* wt, int O, int I, int KK, void* stream);

#ifdef __cplusplus
}
#endif
#endif
