#ifndef IVLN_TOUR_STATE_H
#define IVLN_TOUR_STATE_H
#include "ivln_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * First state encoder of Latent-CMA's `tour_memory_variant` as an LSTM (MODEL.STATE_ENCODER.rnn_type LSTM), with the
 * tour-long memory slot updated INSIDE the masked step (csrc/state_rnn.hip) - an extension of include/ivln_hip.h, whose
 * declarations are pinned (tests/test_state_rnn_host.py hashes its code): entry points added after that pin are declared
 * in a header of their own.
 * The variant feeds the memory slot to the first encoder as the last H columns of its input and max-pools the slot with
 * that encoder's new output (models/latent_cma_policy.py:395-399, 422-425, 433-439), so step t's input depends on step
 * t-1's output and the encoder cannot run as a sequence over a precomputed W_ih x.  The reference has no LSTM form of the
 * pooling (its torch.max broadcasts an (N, 2, H) [h | c] slice into the (N, 1, H) slot and raises); here the slot is
 * pooled with h, the encoder's OUTPUT, which is what the GRU case does ("Latent-CMA with LSTM state encoders").
 * All fp32.  No atomics: two runs give the same bytes.
 * ------------------------------------------------------------------------------------------ */
/* T dependent launches of the step kernel enqueued on `stream` by ONE call: no synchronisation, no allocation, safe under
 * stream capture.  Time-major rows r = t*N + n, I0 = the input columns in front of the memory segment:
 *   m_r   = tour_masks[r] ? (t == 0 ? mem0[n] : max(m_{r-N}, out[r-N])) : 0
 *   gates = gi_base[r] + W_ih[:, I0:I0+H] . m_r + W_hh . (h_prev * ep_masks[r]) + b_hh      (h_prev: h0[n] or out[r-N])
 *   c_r   = s(f) (c_prev * ep_masks[r]) + s(i) tanh(g);   out[r] = s(o) tanh(c_r)
 * gi_base (T*N, 4H) contiguous = W_ih[:, :I0] x_base + b_ih for all rows (the caller's one GEMM); w_ih (4H, I0 + H) is
 * passed WHOLE, its row stride is I0 + H; w_hh (4H, H); b_hh (4H) or NULL.  h0 / c0 / mem0 (N, H) with row strides
 * ld_h0 / ld_c0 / ld_m0 (slices of the (N, L, H) state); ep_masks / tour_masks u8 (T*N).
 * Writes out (T*N, H) row stride ldo; mem_in (T*N, H) row stride ld_mi, m_r - the memory half of the encoder's input,
 * which the dW_ih product of the BPTT and `memory_at_end` read; the last step's h to h_state_out (or NULL), row stride
 * ld_hs; c_state_out (N, H) row stride ld_cs, REQUIRED, holds the cell state from step 0 on (advanced in place) and ends
 * as the last step's c; mem_state_out (N, H) row stride ld_ms = max(m_last, out_last), no mask: the slot the next call
 * starts from.  Optional saves for ivln_lstm_seq_bwd_f32, all five or none: i, f, g, o, c_t, (T*N, H) contiguous each -
 * with x = [x_base | mem_in] that entry point is this one's BPTT (the memory is a constant input, as in the reference,
 * which updates it under no_grad).  T = 1 is the rollout step.
 * A launch reads whole rows of `out` and `mem_in` of the step before (or h0 / mem0) and writes rows of its own step only.
 * h0, c0 and mem0 must therefore not overlap any output: the byte ranges from a view's first to its last element are
 * compared (so slots of ONE (N, L, H) tensor overlap each other), except that c0 may BE c_state_out (same pointer and
 * stride).  16-byte loads when h0 / mem0 / out / mem_in / w_hh / w_ih + I0 and their row strides allow, else 4-byte loads.
 * IVLN_E_INVALID, before any launch: a NULL among the required pointers, a partial set of saves, non-positive T / N / H /
 * I0, H not a multiple of 4, a row stride below H, an overlap as above. */
int ivln_lstm_seq_tour_fwd_f32(const float* gi_base, const float* w_ih, int I0, const float* w_hh, const float* b_hh,
                               const float* h0, int64_t ld_h0, const float* c0, int64_t ld_c0, const float* mem0,
                               int64_t ld_m0, const uint8_t* ep_masks, const uint8_t* tour_masks, float* out, int64_t ldo,
                               float* mem_in, int64_t ld_mi, float* h_state_out, int64_t ld_hs, float* c_state_out,
                               int64_t ld_cs, float* mem_state_out, int64_t ld_ms, int T, int N, int H, float* save_i,
                               float* save_f, float* save_g, float* save_o, float* save_c, void* stream);

#ifdef __cplusplus
}
#endif
#endif
