#ifndef IVLN_SEG_AUGMENT_H
#define IVLN_SEG_AUGMENT_H
#include "ivln_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Training-time augmentation and class statistics for fine-tuning RedNet (csrc/seg_augment.hip).  An extension of
 * include/ivln_seg_train.h with that header's conventions: IVLN_E_INVALID on a NULL required operand or a size out of
 * range before anything is enqueued, a launch grid that depends on the shapes alone, no float atomics.  The reference
 * trains RedNet nowhere, so the arithmetic is defined here (RedNet's own recipe: random scale, crop, flip, HSV jitter).
 * ------------------------------------------------------------------------------------------ */

#define IVLN_SEG_AUGMENT_MAX_B 64      /* images per call: their records travel as one 2 KiB kernel-argument block */
#define IVLN_SEG_AUGMENT_MAX_DIM 32768 /* h, w, H, W: every index and every product below stays inside int32 */
#define IVLN_SEG_AUGMENT_ONE 4096      /* the scale is the rational q / 4096, 2048 <= q <= 8192 */

/* One launch: scale + crop (or pad) + horizontal flip of (rgb, depth, labels) with ONE geometry, the saturation / value
 * jitter of the rgb, and the normalisation RedNet's input takes.
 *   rgb u8 NHWC (B, h, w, 3); depth f32 (B, H, W); labels u8 (B, H, W)
 *   rgb_n f32 (B, 3, H, W)   = ((c' / 255) - mean) / std, as ivln_rgb_resize_normalize_f32 normalises
 *   depth_n f32 (B, 1, H, W) = (d - 0.213) / 0.285;   labels_a u8 (B, H, W)
 * Per image b a record in HOST memory: geom[4 b ..] = {q, oy, ox, flip} int32, photo[4 b ..] = {ks, kv, dv, 0} f32.
 * Geometry, integers only.  Hs = (H * q + 2048) / 4096, Ws likewise: the size of the scaled image.  Output pixel (y, x):
 *   x' = flip ? W - 1 - x : x;  ty = y + oy;  tx = x' + ox;  inside iff 0 <= ty < Hs and 0 <= tx < Ws
 *   ys = min(((2 ty + 1) * 4096) / (2 q), H - 1), xs likewise (the nearest source pixel; integer division)
 * labels and depth are read at (ys, xs): no float decides an index.  rgb, in float: fy = (2 ty + 1) * (2048 / q) - 0.5,
 * taken to the rgb frame (fy + 0.5) * (h / H) - 0.5, clamped to [0, h - 1], x likewise, and the u8 values 0..255 sampled
 * bilinearly with edge-clamped taps there: one sampling of the original image.  An outside pixel gets rgb_n = 0 (the mean
 * colour), depth_n = (0 - 0.213) / 0.285 and the label `ignore_label`.
 * Valid offsets: 0 <= oy <= Hs - H when Hs >= H (a crop), Hs - H <= oy <= 0 when Hs < H (a pad); ox likewise.
 * Photometry, branch-free in RGB (HSV's saturation and value gains without the conversion; no hue): v = max(r, g, b),
 *   c' = clamp(kv * max(v - ks * (v - c), 0) + dv, 0, 255)   per channel c.
 * The identity record {4096, 0, 0, 0 | 1, 1, 0, 0} with (h, w) == (H, W) gives ivln_rgb_resize_normalize_f32's and
 * ivln_affine_f32's bits.
 * IVLN_E_INVALID, before anything is enqueued: B outside [1, 64]; a size outside [1, 32768]; ignore_label outside
 * [-1, 255]; q outside [2048, 8192]; an offset outside its range; flip not 0 / 1; a photo value that is not finite,
 * ks < 0 or kv < 0; a record that pads (Hs < H or Ws < W) while ignore_label == -1.  The records are read by this call and
 * may be reused at once; nothing synchronises the host.
 * A lane owns four consecutive pixels of an output row when W % 4 == 0 and rgb_n, depth_n are 16-byte and labels_a 4-byte
 * aligned (16-byte stores per float plane, one 4-byte store of labels), else one pixel with the same values. */
int ivln_seg_augment_f32(const uint8_t* rgb, const float* depth, const uint8_t* labels, int B, int h, int w, int H, int W,
                         const int32_t* geom, const float* photo, int ignore_label, float* rgb_n, float* depth_n,
                         uint8_t* labels_a, void* stream);

/* Class statistics for median-frequency weights over u8 labels (B, hw), C <= 64, both vectors int64 (C), accumulated
 * (the caller zeroes them):
 *   pixels[c]  += #{pixels of class c}
 *   present[c] += for every image in which c occurs, that image's count of pixels that are neither ignored nor >= C
 * ignore_label in [0, 255] or -1 for none.  `err` is the sticky error word of include/ivln_seg_train.h with the same
 * contract: a label >= C that is not the ignore label sets it and is counted nowhere, and the launch that writes reads it
 * first and writes NOTHING while it is set.  Two launches: every label checked, then one workgroup per image (a 64-bin
 * histogram in LDS).  Integer atomics only: exact in any order. */
int ivln_seg_class_counts_u8(const uint8_t* labels, int B, int64_t hw, int C, int ignore_label, int64_t* pixels,
                             int64_t* present, int* err, void* stream);

#ifdef __cplusplus
}
#endif
#endif
