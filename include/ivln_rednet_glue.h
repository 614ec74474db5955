/* RedNet encoder glue between its layers (csrc/nn_ops.hip) - an extension of include/ivln_hip.h, whose declarations are
 * pinned (tests/test_state_rnn_host.py hashes its code): entry points added after that pin are declared here. */
#ifndef IVLN_REDNET_GLUE_H
#define IVLN_REDNET_GLUE_H
#include "ivln_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The fusion add at the end of an encoder layer (rednet.py:199-222) and the stride-2 gather in front of the next layer's
 * entry block, in one pass.  x: the stacked batch (2 B, C, H, W), contiguous - RGB branch in images [0, B), depth branch in
 * [B, 2 B).  x[:B] += x[B:] in place at full resolution (one fp32 add per element: ivln_add_f32's arithmetic), and every
 * second pixel of every second row of the WHOLE stacked tensor (the summed first half, the depth half as it is) goes to
 * dst[:, dst_coff : dst_coff + C] of a (2 B, dst_ctot, H / 2, W / 2) tensor.  H even, W a multiple of 8, x and dst on
 * 16-byte boundaries (16-byte loads and stores); anything else returns IVLN_E_INVALID.
 * add = 0: the gather alone - x is a (B, C, H, W) tensor and is only read (the two encoders as separate chains). */
int ivln_add_subsample2_f32(float* x, int B, int C, int H, int W, int add, float* dst, int dst_ctot, int dst_coff, void* stream);

/* ivln_rednet_fwd table entry of the call above: src0 = x, dst = dst, i[0..6] = B, C, H, W, dst_ctot, dst_coff, add. */
enum { IVLN_OP_ADD_SUBSAMPLE2 = 6 };

#ifdef __cplusplus
}
#endif
#endif
