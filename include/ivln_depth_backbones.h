#ifndef IVLN_DEPTH_BACKBONES_H
#define IVLN_DEPTH_BACKBONES_H
#include "ivln_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Depth-encoder backbones other than ResNet-50 (MODEL.DEPTH_ENCODER.backbone: resneXt50, se_resnet50, se_resneXt50,
 * se_resneXt101; habitat-lab v0.1.7 rl/ddppo/policy/resnet.py) need two things the dense kernels do not have: a grouped
 * 3x3 convolution (ResNeXt) and the squeeze-and-excite tail (SE).  csrc/group_conv.hip - an extension of
 * include/ivln_hip.h, whose declarations are pinned: entry points added after that pin are declared in a header of their
 * own.
 * All fp32 in, out and accumulation.  Every sum runs in an order fixed by the shape alone and there are no atomics: two
 * runs give the same bytes.  No entry point allocates or synchronises: safe under stream capture.  A precondition that
 * does not hold is refused with IVLN_E_UNSUPPORTED before anything is launched.
 * ------------------------------------------------------------------------------------------ */

/* Grouped 3x3 convolution, pad 1, stride 1 | 2, Cout == Cin == C, no bias:
 *   y[n][co][oy][ox] = sum_{ci < C/groups, ky, kx}  w[co][ci][ky][kx] * x[n][(co / (C/groups)) * (C/groups) + ci][oy*stride - 1 + ky][ox*stride - 1 + kx]
 * x: NCHW, an image's C planes dense, images x_img_stride floats apart (0: C*H*W).  w: (C, C/groups, 3, 3) dense.
 * y: (N, C, Ho, Wo) dense, Ho = (H - 1) / stride + 1, Wo likewise.  The sum of an output runs over input channels in
 * ascending order, the nine taps of a channel quad (MFMA form) or of a channel (VALU form) innermost.
 * Channels per group that are a multiple of 16 run on the fp32 MFMA (v_mfma_f32_16x16x4_f32: 16 output channels x 16
 * pixels per wave, K = 4 input channels of one tap); every other count from 1 to 64 on the VALU.  Both stage the
 * weights and the input halo of 16 input channels at a time in LDS.
 * IVLN_E_UNSUPPORTED: a NULL pointer, non-positive N / C / H / W / groups, C % groups != 0, C / groups > 64, a stride
 * other than 1 or 2, 0 < x_img_stride < C*H*W, C > 2^20 (MFMA form: C > 16 * 65535), or N*Ho rows / Wo columns beyond the grid (2^31 - 1 tiles). */
int ivln_gconv3x3_f32(const float* x, const float* w, float* y, int N, int C, int H, int W, int groups, int stride,
                      int64_t x_img_stride, void* stream);

/* Squeeze-and-excite gate of a bottleneck, one launch for the whole batch (a workgroup per image):
 *   z       = GroupNorm(x; gamma, beta, groups, eps)              (the block's last GroupNorm, never materialised)
 *   gate[n] = sigmoid(W2 . relu(W1 . mean_hw(z[n]) + b1) + b2)    W1 (Cr, C), b1 (Cr), W2 (C, Cr), b2 (C), gate (N, C)
 * mean_hw(z)[c] = gamma[c] * (mean_hw(x)[c] - mean_g) * rstd_g + beta[c]: per-channel sums of the raw tensor and the
 * group's two-pass statistics (the arithmetic of ivln_groupnorm_f32).
 * x is addressed like ivln_groupnorm_f32's input: element (n, c, p) = sum over z < splits of
 * x[z*slab_stride + n*x_img_stride + c*x_chan_stride + p]  (0 strides: dense NCHW; a split-K conv's slabs otherwise).
 * IVLN_E_UNSUPPORTED: a NULL pointer, non-positive N / C / HW / groups / Cr, C % groups != 0, C > 2048, Cr > 128. */
int ivln_se_gate_f32(const float* x, const float* gamma, const float* beta, int N, int C, int HW, int groups, float eps,
                     int64_t x_img_stride, int64_t x_chan_stride, int splits, int64_t slab_stride, const float* w1,
                     const float* b1, const float* w2, const float* b2, int Cr, float* gate, void* stream);

/* The SE bottleneck's tail:  y = relu(gate[n][c] * GroupNorm(x)[n][c][p] + identity[n][c][p]),  identity = `residual`
 * (an NCHW tensor, images r_img_stride apart) or GroupNorm(x2; gamma2, beta2) with the same groups and eps - the two
 * forms ivln_groupnorm_f32 / ivln_groupnorm2_f32 cover; exactly one of residual / x2.  x and x2 are addressed as above,
 * y is NCHW with images y_img_stride apart (0: C*HW).  A workgroup per (image, group), two-pass statistics.
 * IVLN_E_UNSUPPORTED: a NULL among x / gamma / beta / gate / y, neither or both of residual and x2, x2 without gamma2 /
 * beta2, non-positive N / C / HW / groups, C % groups != 0. */
int ivln_se_apply_f32(const float* x, const float* gamma, const float* beta, const float* gate, const float* residual,
                      float* y, int N, int C, int HW, int groups, float eps, int64_t x_img_stride, int64_t x_chan_stride,
                      int splits, int64_t slab_stride, int64_t y_img_stride, int64_t r_img_stride, const float* x2,
                      const float* gamma2, const float* beta2, int64_t x2_img_stride, int64_t x2_chan_stride, int splits2,
                      int64_t slab_stride2, void* stream);

#ifdef __cplusplus
}
#endif
#endif
