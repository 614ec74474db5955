#ifndef IVLN_BOXWORLD_H
#define IVLN_BOXWORLD_H
#include "ivln_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Box-world renderer (csrc/boxworld.hip): depth, labels and colour of a room with axis-aligned boxes, ray-cast on the
 * device from the pose by the INVERSE of the mapper's un-projection (core.py:70-171 with the elevation + pi of
 * mapper.py:133-136) - an extension of include/ivln_hip.h with a header of its own, like include/ivln_known_lib.h.
 * The reference renders nothing (Habitat-Sim does), so the arithmetic is defined here; `boxworld.render_reference` is its
 * numpy float32 restatement and equals the kernel bit for bit.
 *
 * Scene.  A room [lo, hi] seen from inside (label 0) and n <= IVLN_BW_MAX_BOXES boxes [lo, hi] with a label 1..12.
 * Camera of row b.  o = cam_pos[b], (s, c) = sincos[b] = (sin h, cos h) rounded once from double.  Pixel (v, u) of an
 * H x W frame with focal lengths (fx, fy), every operation rounded to float32 where it is written:
 *   xs = (((float)u + 0.5f) - (float)(W / 2.0)) / fx      ys = (((float)v + 0.5f) - (float)(H / 2.0)) / fy
 *   d  = (xs * c - s, -ys, -(xs * s) - c)                 = xs * right + ys * down + forward
 * Room.  Per axis a in x, y, z with d_a != 0: t_a = ((d_a > 0 ? hi_a : lo_a) - o_a) / d_a, face 2a + (d_a > 0); the
 * smallest t_a wins, the first one among equals.
 * Box k, in index order.  Per axis a: d_a == 0 -> a miss if o_a < lo_a or o_a > hi_a, else no constraint; otherwise
 * t1 = (lo_a - o_a) / d_a, t2 = (hi_a - o_a) / d_a, near_a = min(t1, t2), far_a = max(t1, t2); t_near = the largest near_a
 * (the first one among equals, face 2a + (d_a < 0)), t_far = the smallest far_a.  A hit needs t_near > 0, t_near <= t_far
 * and t_near < the best t so far (so a camera inside a box does not see it, and a box face flush with a wall loses).
 * Outputs.  depth = min(max((t - dmin) / (dmax - dmin), 0), 1); label u8; p = o + t * d per component;
 *   rgb[c] = (palette[row][c] * shade[face]) >> 8, row = label, and for label 0 row 0 or 13 by the parity of
 *   floor(p_i / 0.5) + floor(p_j / 0.5) over the two axes i < j other than face / 2.
 * ------------------------------------------------------------------------------------------ */
#define IVLN_BW_MAX_BOXES 32
#define IVLN_BW_MAX_DIM 16384 /* H, W, Hr, Wr */

typedef struct ivln_boxworld ivln_boxworld;

/* A device-resident table of max_scenes scene records, all absent.  IVLN_E_INVALID: max_scenes outside [1, 2^16], NULL out. */
int ivln_boxworld_create(int max_scenes, ivln_boxworld** out);
int ivln_boxworld_destroy(ivln_boxworld* bw);
/* Uploads scene `scene` once (host operands; returns after the copy has run).  room f32 [6] = lo xyz, hi xyz; boxes f32
 * [n][6] likewise; labels u8 [n].  IVLN_E_INVALID before anything is copied: NULL handle / room, scene outside the table
 * or added before, n outside [0, 32], NULL boxes / labels with n > 0, a value that is not finite, lo >= hi on any axis,
 * a label outside [1, 12]. */
int ivln_boxworld_add_scene(ivln_boxworld* bw, int scene, const float* room, int n, const float* boxes,
                            const uint8_t* labels, void* stream);
/* Number of scenes added so far, or IVLN_E_INVALID for a NULL handle. */
int ivln_boxworld_size(ivln_boxworld* bw);

/* Renders B rows: one launch of grid (tiles, B) for depth + labels, and one for rgb when Hr > 0 (its own size and focal
 * lengths).  scene_index i32 [B], cam_pos f32 [B][3], sincos f32 [B][2] = (sin h, cos h), depth f32 [B][H][W], labels u8
 * [B][H][W], rgb u8 [B][Hr][Wr][3]: device memory.  A lane renders four horizontally adjacent pixels; depth leaves as one
 * 16-byte store and labels as one 4-byte store where the row offset allows, a row tail takes scalar stores.
 * IVLN_E_INVALID before any launch: NULL handle or operand, B outside [1, 65535], H or W outside [1, 16384], Hr or Wr < 0 or above 16384
 * or only one of them 0, rgb NULL with Hr > 0, dmax <= dmin, a focal length that is not positive.
 * A scene index without a table entry reads nothing through it: the row's depth is written as 1, its labels (and rgb) as
 * 0, and the sticky status IVLN_E_INVALID is set (ivln_boxworld_status). */
int ivln_boxworld_render(ivln_boxworld* bw, const int32_t* scene_index, const float* cam_pos, const float* sincos, int B,
                         int H, int W, float fx, float fy, float dmin, float dmax, float* depth, uint8_t* labels, int Hr,
                         int Wr, float fxr, float fyr, uint8_t* rgb, void* stream);
/* Synchronises `stream` and returns the sticky device status (IVLN_OK / IVLN_E_INVALID); `clear` != 0 resets it. */
int ivln_boxworld_status(ivln_boxworld* bw, int clear, void* stream);

#ifdef __cplusplus
}
#endif
#endif
