#ifndef IVLN_RGB_BWD_H
#define IVLN_RGB_BWD_H
#include "ivln_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Train-mode forward epilogue and backward of the torchvision ResNet-50 RGB encoder: MODEL.RGB_ENCODER.trainable
 * (csrc/rgb_bwd.hip).  Like include/ivln_depth_bwd.h an extension of include/ivln_hip.h, whose declarations are pinned.
 * The reference sets requires_grad on `cnn` and puts it in train mode (models/encoders/resnet_encoders.py:141-143), stops
 * feeding cached `rgb_features` (:194) and lets autograd train it.  Here the conv gradients are GEMMs (ivln_gemm_f32) and
 * the max-pool backward is ivln_maxpool3s2_bwd_f32; these are the kernels between them.  All fp32, NCHW contiguous.
 * No float atomics: every sum runs in a fixed order, two runs give the same bits.  Every entry point returns
 * IVLN_E_INVALID on a NULL required operand or a non-positive size before anything is launched.
 * ------------------------------------------------------------------------------------------ */
/* y = [relu](x * scale[c] + shift[c] [+ r] [+ r2 * scale2[c] + shift2[c]]) over (N, C, HW): BatchNorm applied to a raw conv
 * output with the statistics already folded into scale / shift (train mode: ivln_bn_stats_from_partials_f32 /
 * ivln_bn_train_stats_f32; eval mode: ivln_bn_fold_f32), and a bottleneck's tail relu(bn3(c3) + identity) (r) or
 * relu(bn3(c3) + bn_ds(ds)) (r2, scale2, shift2: all three or none).  16-byte accesses when HW % 4 == 0 and x / r / r2 / y
 * are 16-byte aligned, else 4-byte accesses with the same values. */
int ivln_bn_apply_f32(const float* x, const float* scale, const float* shift, const float* r, const float* r2,
                      const float* scale2, const float* shift2, int N, int C, int HW, int relu, float* y, void* stream);
/* Backward of BatchNorm2d (+ the ReLU behind it).  dy, x (N, C, HW): the upstream gradient and the RAW conv output the
 * forward normalised; gamma (C); out (N, C, HW) or NULL: the activated output - with it dz = dy * (out > 0), without it
 * dz = dy.  M = N * HW, xh = (x - mean[c]) * rstd[c]:
 *   dbeta[c] = sum_{n,hw} dz;  dgamma[c] = sum_{n,hw} dz * xh
 *   train != 0: mean / rstd_or_var (C) are the batch mean and rstd the forward saved;
 *               dx = gamma * rstd * (dz - dbeta / M - xh * dgamma / M)
 *   train == 0: mean / rstd_or_var are running_mean and running_VAR, rstd = 1 / sqrt(var + eps);  dx = gamma * rstd * dz
 * dz_out (N, C, HW) or NULL receives dz (a bottleneck tail needs it three times).  dx may be `out` and dz_out may be `dy`
 * (every element is read before it is written, by the same thread); no other overlap.
 * Three launches: partial sums in double of slices of the images per channel into ws (fixed order), the slices summed in
 * ascending order, the apply pass.  ws holds 4 floats per (channel, slice): >= 4 * C + 2 floats, more lets few channels
 * with large planes spread over more workgroups (4 * C * min(N, 64) + 2 is enough for every split the launcher takes).
 * 16-byte accesses when HW % 4 == 0 and dy / x / out / dx / dz_out are 16-byte aligned, else 4-byte accesses. */
int ivln_bn_bwd_f32(const float* dy, const float* x, const float* mean, const float* rstd_or_var, const float* gamma,
                    const float* out, int N, int C, int HW, int train, float eps, float* dx, float* dz_out, float* dgamma,
                    float* dbeta, float* ws, int64_t ws_floats, void* stream);
/* Backward of ivln_adaptive_avgpool2d_f32: dy (N, C, OH, OW) with image stride dy_img_stride floats (a channel slice of a
 * wider buffer: out_ctot * OH * OW; <= 0: dense) -> dx (N, C, H, W) dense.  Gather form: an input pixel sums, in ascending
 * (oh, ow), dy / window size of every window [floor(o * H / OH), ceil((o + 1) * H / OH)) that covers it. */
int ivln_adaptive_avgpool2d_bwd_f32(const float* dy, int N, int C, int H, int W, int OH, int OW, int64_t dy_img_stride,
                                    float* dx, void* stream);

#ifdef __cplusplus
}
#endif
#endif
