#ifndef IVLN_SEG_TRAIN_H
#define IVLN_SEG_TRAIN_H
#include "ivln_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Segmentation loss and metrics for fine-tuning RedNet (csrc/seg_loss.hip).  Like include/ivln_rgb_bwd.h an extension of
 * include/ivln_hip.h, whose declarations are pinned.  The reference ships no loss for RedNet (rednet.py:224-256 returns
 * five score maps in train mode and nothing consumes them), so the loss is defined here: torch's
 * F.cross_entropy(weight=, ignore_index=, reduction="mean") per score map against the nearest-neighbour down-sampled
 * labels.  The conv gradients behind it are GEMMs (ivln_gemm_f32), the bias gradients ivln_nchw_chansum_f32.
 * No float atomics: every sum runs in a fixed order, in double; two runs give the same bits.  Every entry point returns
 * IVLN_E_INVALID on a NULL required operand or a size out of range before anything is launched.
 *
 * The error word: `err` is one int32 on the device that the caller zeroes once.  A launch that meets a label it cannot
 * take ORs 1 into it and no launch ever clears it (sticky); the kernels that write results read it first and write
 * NOTHING while it is set.  The caller reads it back when it wants the verdict and zeroes it to go on.
 * ------------------------------------------------------------------------------------------ */

/* Pixel cross-entropy over NCHW scores.  scores (N, C, h, w) f32, 2 <= C <= 64; labels u8 (N, h * s, w * s) at full
 * resolution, s >= 1: the target of pixel (i, j) is labels[i * s][j * s] - what F.interpolate(mode="nearest") picks for an
 * integer factor; class_w (C) or NULL (all ones); ignore_label in [0, 255] or -1 for none.  Over the pixels p whose target
 * t_p is not the ignore label:
 *   loss    = sum_p class_w[t_p] * (-log softmax(scores_p)[t_p]) / sum_p class_w[t_p]
 *   dscores = scale * d(loss) / d(scores)      (N, C, h, w), zero at ignored pixels;  NULL: the loss alone
 * When every pixel is ignored (or carries weight 0) the denominator is 0: loss = 0 and dscores = 0 here.  torch gives NaN
 * for that call; a batch without a labelled pixel must not poison the weights, so the two differ on purpose.
 * A target >= C that is not the ignore label sets the error word; `loss` and `dscores` are then left untouched.
 * The per-pixel arithmetic is double (max-subtracted log-sum-exp), rounded to f32 once on the way out.
 * Three launches: per-workgroup partial sums (each lane walks its pixels in ascending order, the lanes meet in a fixed
 * tree), the partials summed in ascending order by one workgroup, the gradient pass.  The grid depends on the shape alone.
 * A lane owns pixels and walks the C classes (class stride h * w): 16-byte accesses when (h * w) % 4 == 0 and scores /
 * dscores are 16-byte aligned, else 4-byte accesses with the same values.
 * ws: >= IVLN_SEG_CE_WS_DOUBLES doubles, 8-byte aligned; ws[0] / ws[1] hold the two sums afterwards. */
#define IVLN_SEG_CE_WS_DOUBLES 2064
int ivln_seg_ce_f32(const float* scores, const uint8_t* labels, const float* class_w, int N, int C, int h, int w, int s,
                    int ignore_label, double scale, float* loss, float* dscores, double* ws, int64_t ws_doubles, int* err,
                    void* stream);

/* Confusion counts: counts[t * C + p] += #{i : truth[i] == t, pred[i] == p} over the n pixels whose truth is not the ignore
 * label (-1: none); counts (C, C) int64, accumulated (the caller zeroes it), C <= 64.  Integer atomics: exact in any order.
 * A truth or a prediction >= C (truth: that is not the ignore label) sets the error word and is not counted. */
int ivln_seg_confusion_u8(const uint8_t* pred, const uint8_t* truth, int64_t n, int C, int ignore_label, int64_t* counts,
                          int* err, void* stream);

#ifdef __cplusplus
}
#endif
#endif
