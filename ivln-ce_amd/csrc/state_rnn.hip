// Masked recurrent state encoders for gfx950: habitat-lab's RNNStateEncoder around nn.GRU / nn.LSTM (one layer), built by
// the reference with rnn_type=model_config.STATE_ENCODER.rnn_type (ivlnce_baselines/models/map_cma_policy.py:183,229) and
// run over the state slices of :290-351 (rollout: one step) and over time-major (T*N rows) trajectory batches under
// base_il_trainer.py:173-219 (update: sequence forward with saved gates, then BPTT).  All fp32.  The cell arithmetic is
// csrc/rnn_cell.h; this file holds the work splits.
//
// 1. One step (k_rnn_step<Cell, LPR, VEC>).  At rollout size (rows <= 8, H = 512) a step streams W_hh once (3-4 MB) and
//    does 6-8 MFLOP: bound by L2 bandwidth and load latency, not a matrix-core problem.  One workgroup per hidden unit j
//    reads the unit's gate rows of W_hh (and W_ih); 32 or 64 lanes share one state row, each lane owns every LPR-th piece
//    of K, so a (row, unit) costs one shuffle reduction and no LDS or barrier (the previous wave-splits-K form spent
//    most of its 13 us in 48 full-wave reductions per block).  H workgroups of 256 threads cover the chip twice at H = 512.
// 2. A sequence as T such launches enqueued back to back from ONE C call (the per-timestep Python -> ctypes round trip,
//    ~15 us, was longer than the 6.5 us kernel), BPTT likewise as one launch per timestep: the carry of step t (a skinny
//    matvec against W_hh^T) fused with the element part of step t-1 on the same hidden unit.  Latent-CMA's
//    `tour_memory_variant` feeds its first encoder a memory pooled with that encoder's previous output, so no W_ih x can
//    be precomputed for that segment: k_rnn_step_tour is the step with the memory update inside it, enqueued the same way.
// 3. The GRU sequence and its BPTT as ONE persistent launch each, inside an envelope (H = 512, N <= 64 / 16); the LSTM has
//    no persistent form.  Design:
//   * 64 workgroups x 256 threads; workgroup b owns hidden units [8 b, 8 b + 8).  A 32-lane group owns one unit and keeps
//     its three W_hh rows (forward) / its W_hh^T row (backward) IN REGISTERS for the whole sequence, split over the lanes
//     exactly like the step kernels split K (lane l owns float4 l, l + 32, ...): 48 floats per lane either way; the 3 MB
//     matrix is read once per launch, not once per timestep.  (16 units per workgroup, 32 x 512, measured slower.)
//   * Per timestep every workgroup needs the WHOLE vector the others produced in the step before (h_{t-1}: N x 512
//     floats forward, dgh_t: N x 1536 backward).  It is exchanged through the kernel's own OUTPUT tensors - `out` rows
//     of step t-1, `dgh` rows of step t - which every step writes to a fresh location: producers store write-through at
//     agent scope (`global_store ... sc1`), drain (`s_waitcnt vmcnt(0)`), arrive on one monotonic counter; consumers
//     poll the counter relaxed from one lane, then read the rows with 16-byte `sc1` (L1-bypassing) buffer loads, all in
//     flight at once, into LDS.  No fences: every exchanged word is write-through stored and sc1 loaded
//     (MI355X_MICROARCH.md, "valid forms").  Stores nobody waits for (saved gates, dgi, hp) and the next step's
//     prefetches are issued between the arrival and the poll.
//   * The counter and a give-up flag live in a caller-provided 256-byte `sync_ws` whose first 192 bytes a memset node
//     zeroes in front of the launch (stream-ordered, so replay-safe); word 48 is the STICKY error word the host reads -
//     several launches share one workspace (four per update), and a flag the next launch's memset erased would hide a
//     timed-out earlier one.  Every spin is bounded: on a timeout the error word is set, all
//     workgroups leave, and `ivln_seq_sync_status` reports it - a lost workgroup can never hang the GPU.
//   * Same lane -> K mapping, fma chains and element formulas as the per-step kernels; the cross-lane sums run on the
//     DPP path in a different association.  The two paths agree to ~2e-7 (tests/test_gpu_kernels.py, bar 1e-6), and the
//     persistent path is bit-reproducible run to run, idle or beside a bandwidth-heavy stream.
//   Measured (MI355X, T = 64, N = 8; tools/gru_seq_bench.py, tools/gru_seq_phases.py; profiles/r03_gru_seq.txt): 4.7 us
//   per forward step and 4.9 us per backward step against 5.8 / 6.5 us for the dependent launches (N = 5: 4.2 / 4.4
//   against 5.7 / 6.3).  Anatomy of a forward step at N = 8: staging the 16 KB of h_{t-1} 0.8 us (one sc1 round trip),
//   matvec + DPP reduction 1.6 us (latency-bound: 0.7 us of it is the 24 x 5 dependent DPP adds, the same with one or
//   two waves per SIMD), element part 0.4 us, drain + arrival 0.5 us, counter wait 1.3 us - three serialised memory
//   round trips per step, which is the floor of this form (tools/barrier_bench prices the bare exchange at 1.9-2.2 us).
//   First version, for the record: 8-byte atomic loads issued one per loop iteration serialised N/2 round trips per
//   step (7.1 us per step, slower than the launches); __shfl_xor reductions (LDS permutes) cost another 0.5 us.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/ivln_hip.h"
#include "../../include/ivln_tour_state.h"
#include "residency.h"
#include "rnn_cell.h"

namespace {

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP)

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---------------------------------------------------------------------------------------------------------------
// One masked step for `rows` states: x (rows, I) against W_ih, or precomputed gi_pre = W_ih x + b_ih when x == nullptr.
// VEC: 16-byte loads (every row of x / h_in / W_ih / W_hh 16-byte aligned), else 4-byte loads with the same lane-strided
// split of K.  LSTM: c_in and c_out may be the same memory (element (row, j) is read and then written by one thread
// only); h_in must not overlap h_out / h_out2 (every workgroup reads whole rows of h_in).  GRU: c_in / c_out / save4 are
// not touched.  Optional saves for BPTT, (rows, H) each: GRU r, z, n, gh_n; LSTM i, f, g, o, c_t.
// ---------------------------------------------------------------------------------------------------------------
template <class Cell, int LPR, bool VEC>
__global__ __launch_bounds__(256) void k_rnn_step(const float* __restrict__ x, int64_t ldx, int I,
                                                  const float* __restrict__ gi_pre, int64_t ldgi,
                                                  const float* __restrict__ h_in, int64_t ldh, const float* c_in,
                                                  int64_t ldc, const uint8_t* __restrict__ mask,
                                                  const float* __restrict__ w_ih, const float* __restrict__ w_hh,
                                                  const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                                  float* __restrict__ h_out, int64_t ldo, float* __restrict__ h_out2,
                                                  int64_t ldo2, float* c_out, int64_t ldco, int rows, int H,
                                                  float* __restrict__ save0, float* __restrict__ save1,
                                                  float* __restrict__ save2, float* __restrict__ save3,
                                                  float* __restrict__ save4) {
    constexpr int NG = Cell::NG;
    constexpr int RPB = 256 / LPR;  // rows per pass
    const int j = blockIdx.x;
    const int l = threadIdx.x % LPR, rr = threadIdx.x / LPR;
    for (int r0 = 0; r0 < rows; r0 += RPB) {
        const int row = r0 + rr;
        const bool row_ok = row < rows;
        const int rowc = row_ok ? row : 0;
        float ai[NG], ah[NG];
        if (x) gate_dots<NG, LPR, VEC>(w_ih, j, H, I, x + (int64_t)rowc * ldx, 1.f, l, ai);
        const float mk = mask ? (mask[rowc] ? 1.f : 0.f) : 1.f;
        gate_dots<NG, LPR, VEC>(w_hh, j, H, H, h_in + (int64_t)rowc * ldh, mk, l, ah);
        lpr_sum_gates<LPR>(ai, x != nullptr, ah);
        if (l == 0 && row_ok) {
            float gi[NG], gh[NG], sv[5];
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if constexpr (Cell::HAS_C) {   // the LSTM's biases may be NULL; the GRU's entry points have always required them
                    gi[g] = x ? ai[g] + (b_ih ? b_ih[g * H + j] : 0.f) : gi_pre[(int64_t)row * ldgi + g * H + j];
                    gh[g] = ah[g] + (b_hh ? b_hh[g * H + j] : 0.f);
                } else {
                    gi[g] = x ? ai[g] + b_ih[g * H + j] : gi_pre[(int64_t)row * ldgi + g * H + j];
                    gh[g] = ah[g] + b_hh[g * H + j];
                }
            }
            const float prev = (Cell::HAS_C ? c_in[(int64_t)row * ldc + j] : h_in[(int64_t)row * ldh + j]) * mk;
            const float hn = Cell::fwd(gi, gh, prev, sv);
            h_out[(int64_t)row * ldo + j] = hn;
            if (h_out2) h_out2[(int64_t)row * ldo2 + j] = hn;
            if constexpr (Cell::HAS_C) c_out[(int64_t)row * ldco + j] = sv[4];
            if (save0) {
                const int64_t e = (int64_t)row * H + j;
                save0[e] = sv[0], save1[e] = sv[1], save2[e] = sv[2], save3[e] = sv[3];
                if constexpr (Cell::NSAVE == 5) save4[e] = sv[4];
            }
        }
    }
}

struct Saves {   // the step's optional saves for BPTT (all or none; GRU uses the first four)
    float* p[5];
};

// rows <= 4: 64 lanes per row, else 32 (8 rows per pass).  The GRU has the 16-byte-load form only (its entry points
// refuse everything else); the LSTM takes the 4-byte form for operands that are not 16-byte aligned.
template <class Cell>
void launch_step(const float* x, int64_t ldx, int I, const float* gi_pre, int64_t ldgi, const float* h_in, int64_t ldh,
                 const float* c_in, int64_t ldc, const uint8_t* mask, const float* w_ih, const float* w_hh,
                 const float* b_ih, const float* b_hh, float* h_out, int64_t ldo, float* h_out2, int64_t ldo2, float* c_out,
                 int64_t ldco, int rows, int H, const Saves& sv, hipStream_t s) {
    bool vec = true;
    if constexpr (Cell::HAS_C)
        vec = al16(h_in) && al16(w_hh) && !(ldh & 3) && (!x || (al16(x) && al16(w_ih) && !(I & 3) && !(ldx & 3)));
#define IVLN_RNN_STEP(LPR, VEC)                                                                                           \
    hipLaunchKernelGGL((k_rnn_step<Cell, LPR, VEC>), dim3(H), dim3(256), 0, s, x, ldx, I, gi_pre, ldgi, h_in, ldh, c_in,  \
                       ldc, mask, w_ih, w_hh, b_ih, b_hh, h_out, ldo, h_out2, ldo2, c_out, ldco, rows, H, sv.p[0], sv.p[1], \
                       sv.p[2], sv.p[3], sv.p[4])
    if constexpr (Cell::HAS_C) {
        if (!vec) {
            if (rows <= 4) IVLN_RNN_STEP(64, false); else IVLN_RNN_STEP(32, false);
            return;
        }
    }
    if (rows <= 4) IVLN_RNN_STEP(64, true); else IVLN_RNN_STEP(32, true);
#undef IVLN_RNN_STEP
}

// the saves of one timestep of a sequence: `off` floats into each tensor, or nothing
Saves saves_at(const Saves& all, int64_t off) {
    Saves sv;
    for (int i = 0; i < 5; ++i) sv.p[i] = all.p[0] && all.p[i] ? all.p[i] + off : nullptr;
    return sv;
}

// ---------------------------------------------------------------------------------------------------------------
// The masked step with Latent-CMA's tour-long memory inside it (include/ivln_tour_state.h): k_rnn_step's work split
// (workgroup j = hidden unit j, LPR lanes per state row, one shuffle reduction per (row, unit)) for an encoder whose
// input ends in a memory segment that depends on its own previous output,
//   m = tour_mask ? (pool ? max(mem_prev, h_in) : mem_prev) : 0        (pool: every step but the first of a call)
//   gi = gi_base + W_ih[:, I0:I0+H] . m                                 (gi_base = W_ih[:, :I0] x + b_ih, precomputed)
// Every workgroup recomputes all H values of m from the rows of the step before (h_in is both the recurrent state and
// what the memory is pooled with: one load serves both); it writes m[j], never reads this step's m_out.  mem_state, when
// given, takes max(m, h_t) - the slot the next call starts from.  c_in / c_out as in k_rnn_step.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float tour_m(float mem, float h, bool keep, bool pool) {
    return keep ? (pool ? fmaxf(mem, h) : mem) : 0.f;
}

// gate_dots for this step: unit j's NG rows of W_hh against h * mk AND of the memory segment of W_ih (w_mem = W_ih + I0,
// row stride ldw) against m, in ONE pass over H with the same lane-strided split; the lanes' partial sums are returned.
template <int NG, int LPR, bool VEC>
__device__ __forceinline__ void tour_gate_dots(const float* __restrict__ w_hh, const float* __restrict__ w_mem, int64_t ldw,
                                               int j, int H, const float* __restrict__ h, float mk,
                                               const float* __restrict__ mem, bool keep, bool pool, int l, float (&am)[NG],
                                               float (&ah)[NG]) {
#pragma unroll
    for (int g = 0; g < NG; ++g) am[g] = ah[g] = 0.f;
    if constexpr (VEC) {
        for (int k = l * 4; k < H; k += LPR * 4) {
            float4 hv = *reinterpret_cast<const float4*>(h + k);
            float4 mv = *reinterpret_cast<const float4*>(mem + k);
            mv.x = tour_m(mv.x, hv.x, keep, pool), mv.y = tour_m(mv.y, hv.y, keep, pool);
            mv.z = tour_m(mv.z, hv.z, keep, pool), mv.w = tour_m(mv.w, hv.w, keep, pool);
            hv.x *= mk, hv.y *= mk, hv.z *= mk, hv.w *= mk;
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                ah[g] = fma4(*reinterpret_cast<const float4*>(w_hh + ((int64_t)g * H + j) * H + k), hv, ah[g]);
                am[g] = fma4(*reinterpret_cast<const float4*>(w_mem + ((int64_t)g * H + j) * ldw + k), mv, am[g]);
            }
        }
    } else {
        for (int k = l; k < H; k += LPR) {
            const float hk = h[k];
            const float mv = tour_m(mem[k], hk, keep, pool), hv = hk * mk;
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                ah[g] = fmaf(w_hh[((int64_t)g * H + j) * H + k], hv, ah[g]);
                am[g] = fmaf(w_mem[((int64_t)g * H + j) * ldw + k], mv, am[g]);
            }
        }
    }
}

template <class Cell, int LPR, bool VEC>
__global__ __launch_bounds__(256) void k_rnn_step_tour(
    const float* __restrict__ gi_base, const float* __restrict__ h_in, int64_t ldh, const float* c_in, int64_t ldc,
    const float* __restrict__ mem_prev, int64_t ldm, int pool, const uint8_t* __restrict__ ep_mask,
    const uint8_t* __restrict__ tour_mask, const float* __restrict__ w_mem, int64_t ldw, const float* __restrict__ w_hh,
    const float* __restrict__ b_hh, float* __restrict__ h_out, int64_t ldo, float* __restrict__ m_out, int64_t ldmo,
    float* __restrict__ h_out2, int64_t ldo2, float* c_out, int64_t ldco, float* __restrict__ mem_state, int64_t ldms,
    int rows, int H, float* __restrict__ save0, float* __restrict__ save1, float* __restrict__ save2,
    float* __restrict__ save3, float* __restrict__ save4) {
    constexpr int NG = Cell::NG;
    constexpr int RPB = 256 / LPR;  // rows per pass
    const int j = blockIdx.x;
    const int l = threadIdx.x % LPR, rr = threadIdx.x / LPR;
    for (int r0 = 0; r0 < rows; r0 += RPB) {
        const int row = r0 + rr;
        const bool row_ok = row < rows;
        const int rowc = row_ok ? row : 0;
        const float mk = ep_mask[rowc] ? 1.f : 0.f;
        const bool keep = tour_mask[rowc] != 0;
        const float* hr = h_in + (int64_t)rowc * ldh;
        const float* mr = mem_prev + (int64_t)rowc * ldm;
        float am[NG], ah[NG];
        tour_gate_dots<NG, LPR, VEC>(w_hh, w_mem, ldw, j, H, hr, mk, mr, keep, pool != 0, l, am, ah);
        lpr_sum_gates<LPR>(am, true, ah);
        if (l == 0 && row_ok) {
            float gi[NG], gh[NG], sv[5];
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                gi[g] = gi_base[(int64_t)row * NG * H + g * H + j] + am[g];
                gh[g] = ah[g] + (b_hh ? b_hh[g * H + j] : 0.f);
            }
            const float hj = hr[j];
            const float mj = tour_m(mr[j], hj, keep, pool != 0);
            const float prev = (Cell::HAS_C ? c_in[(int64_t)row * ldc + j] : hj) * mk;
            const float hn = Cell::fwd(gi, gh, prev, sv);
            h_out[(int64_t)row * ldo + j] = hn;
            m_out[(int64_t)row * ldmo + j] = mj;
            if (h_out2) h_out2[(int64_t)row * ldo2 + j] = hn;
            if (mem_state) mem_state[(int64_t)row * ldms + j] = fmaxf(mj, hn);
            if constexpr (Cell::HAS_C) c_out[(int64_t)row * ldco + j] = sv[4];
            if (save0) {
                const int64_t e = (int64_t)row * H + j;
                save0[e] = sv[0], save1[e] = sv[1], save2[e] = sv[2], save3[e] = sv[3];
                if constexpr (Cell::NSAVE == 5) save4[e] = sv[4];
            }
        }
    }
}

// the bytes from the first to the last element of a (rows, H) view with row stride ld
struct Span {
    uintptr_t lo, hi;
};
inline Span span_of(const void* p, int64_t rows, int64_t ld, int64_t H) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    return {lo, p ? lo + (uintptr_t)(((rows - 1) * ld + H) * (int64_t)sizeof(float)) : lo};
}
inline bool overlap(const Span& a, const Span& b) { return a.lo < b.hi && b.lo < a.hi; }

// A whole sequence of such steps, enqueued back to back (ivln_lstm_seq_fwd_f32's shape).  The load form is chosen ONCE
// for the sequence, so every step runs the same arithmetic.  The caller has validated sizes and overlaps.
template <class Cell>
void launch_tour_seq(const float* gi_base, const float* w_ih, int I0, const float* w_hh, const float* b_hh,
                     const float* h0, int64_t ld_h0, const float* c0, int64_t ld_c0, const float* mem0, int64_t ld_m0,
                     const uint8_t* ep_masks, const uint8_t* tour_masks, float* out, int64_t ldo, float* mem_in,
                     int64_t ld_mi, float* h_state_out, int64_t ld_hs, float* c_state_out, int64_t ld_cs,
                     float* mem_state_out, int64_t ld_ms, int T, int N, int H, const Saves& all, hipStream_t s) {
    const float* w_mem = w_ih + I0;
    const int64_t ldw = (int64_t)I0 + H;
    const bool vec = al16(h0) && al16(mem0) && al16(out) && al16(mem_in) && al16(w_hh) && al16(w_mem) &&
                     !((ld_h0 | ld_m0 | ldo | ld_mi | ldw) & 3);
    for (int t = 0; t < T; ++t) {
        const int64_t r0 = (int64_t)t * N;
        const bool last = t == T - 1;
        const float* h_in = t == 0 ? h0 : out + (r0 - N) * ldo;
        const float* m_prev = t == 0 ? mem0 : mem_in + (r0 - N) * ld_mi;
        const Saves sv = saves_at(all, r0 * H);
#define IVLN_TOUR_STEP(LPR, VEC)                                                                                          \
    hipLaunchKernelGGL((k_rnn_step_tour<Cell, LPR, VEC>), dim3(H), dim3(256), 0, s, gi_base + r0 * Cell::NG * H, h_in,    \
                       t == 0 ? ld_h0 : ldo, t == 0 ? c0 : c_state_out, t == 0 ? ld_c0 : ld_cs, m_prev,                   \
                       t == 0 ? ld_m0 : ld_mi, t == 0 ? 0 : 1, ep_masks + r0, tour_masks + r0, w_mem, ldw, w_hh, b_hh,    \
                       out + r0 * ldo, ldo, mem_in + r0 * ld_mi, ld_mi, last ? h_state_out : nullptr, ld_hs, c_state_out,  \
                       ld_cs, last ? mem_state_out : nullptr, ld_ms, N, H, sv.p[0], sv.p[1], sv.p[2], sv.p[3], sv.p[4])
        if (vec) {
            if (N <= 4) IVLN_TOUR_STEP(64, true); else IVLN_TOUR_STEP(32, true);
        } else {
            if (N <= 4) IVLN_TOUR_STEP(64, false); else IVLN_TOUR_STEP(32, false);
        }
#undef IVLN_TOUR_STEP
    }
}

// ---------------------------------------------------------------------------------------------------------------
// GRU BPTT, one launch per timestep.  k_gru_bwd_elem: the element part of one step (rows = N sequences of step t), the
// matvec dh_prev = dgh . W_hh then runs through k_linear_skinny_ex (train_ops.hip) with a (+dhz) * mask epilogue.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gru_bwd_elem(const float* __restrict__ dout, int64_t ld_dout,
                                                      const float* __restrict__ dh_carry,
                                                      const float* __restrict__ r, const float* __restrict__ z,
                                                      const float* __restrict__ n, const float* __restrict__ ghn,
                                                      const float* __restrict__ h_prev, int64_t ldh,
                                                      const uint8_t* __restrict__ mask, int rows, int H,
                                                      float* __restrict__ dgi, float* __restrict__ dgh,
                                                      float* __restrict__ dhz, float* __restrict__ hp_out) {
    int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * H) return;
    int row = idx / H, j = idx % H;
    float dh = dout[(int64_t)row * ld_dout + j] + (dh_carry ? dh_carry[idx] : 0.f);
    float mk = mask[row] ? 1.f : 0.f;
    float hp = h_prev[(int64_t)row * ldh + j] * mk;
    const float rg = r[idx];
    const GruBwd b = gru_cell_bwd(dh, hp, rg, z[idx], n[idx], ghn[idx]);
    int64_t o = (int64_t)row * 3 * H + j;
    dgi[o] = b.dr_pre;
    dgi[o + H] = b.dz_pre;
    dgi[o + 2 * H] = b.dn_pre;
    dgh[o] = b.dr_pre;
    dgh[o + H] = b.dz_pre;
    dgh[o + 2 * H] = b.dn_pre * rg;
    dhz[idx] = b.dhz;
    hp_out[idx] = hp;
}

// One BPTT step of the masked GRU in ONE launch: block j first finishes step t for hidden unit j,
//   dh_prev[row][j] = (W_hh^T[j] . dgh_t[row] + dhz[row][j]) * mask_t[row]
// and, since the element part of step t-1 for unit j needs nothing but that value, runs it right away.  Halves the
// launches of the BPTT chain (2 x 126 per GRU per update).  32 lanes per row, 8 rows per pass.
__global__ __launch_bounds__(256) void k_gru_bwd_step(
    const float* __restrict__ dgh_t, int64_t ld_dgh, const float* __restrict__ Wt, const uint8_t* __restrict__ mask_t,
    const float* __restrict__ dout_p, int64_t ld_dout, const float* __restrict__ r, const float* __restrict__ z,
    const float* __restrict__ n, const float* __restrict__ ghn, const float* __restrict__ h_pp, int64_t ldh,
    const uint8_t* __restrict__ mask_p, int rows, int H, float* __restrict__ dhz, float* __restrict__ dgi_p,
    float* __restrict__ dgh_p, float* __restrict__ hp_p) {
    const int j = blockIdx.x;
    const int l = threadIdx.x & 31, rr = threadIdx.x >> 5;
    const int K = 3 * H;
    const float* wr = Wt + (int64_t)j * K;
    for (int r0 = 0; r0 < rows; r0 += 8) {
        const int row = r0 + rr;
        const bool row_ok = row < rows;
        const int rowc = row_ok ? row : 0;
        const float* xr = dgh_t + (int64_t)rowc * ld_dgh;
        // the element part's inputs do not depend on the matvec: fetch them first, under its loads
        const int idx = rowc * H + j;
        const float e_dout = dout_p[(int64_t)rowc * ld_dout + j], e_dhz = dhz[idx];
        const float e_h = h_pp[(int64_t)rowc * ldh + j];
        const float rg = r[idx], zg = z[idx], ng = n[idx], gh = ghn[idx];
        const bool e_mt = mask_t[rowc] != 0, e_mp = mask_p[rowc] != 0;
        float v = skinny_dot32(wr, xr, K, l);
        if (l == 0 && row_ok) {
            v = e_mt ? v + e_dhz : 0.f;  // dh carried into step t-1
            const float hp = e_mp ? e_h : 0.f;
            const GruBwd b = gru_cell_bwd(e_dout + v, hp, rg, zg, ng, gh);
            const int64_t o = (int64_t)row * 3 * H + j;
            dgi_p[o] = b.dr_pre;
            dgi_p[o + H] = b.dz_pre;
            dgi_p[o + 2 * H] = b.dn_pre;
            dgh_p[o] = b.dr_pre;
            dgh_p[o + H] = b.dz_pre;
            dgh_p[o + 2 * H] = b.dn_pre * rg;
            dhz[idx] = b.dhz;
            hp_p[idx] = hp;
        }
    }
}

// One LSTM BPTT step in one launch, workgroup j = hidden unit j (k_gru_bwd_step's work split).
// CARRY: what step t sends back into unit j of the previous state,
//   dh_prev[row][j] = mask_t[row] ? Wt[j] . dgi_t[row] : 0      (Wt = W_hh^T, (H, 4H))
//   dc_prev[row][j] = mask_t[row] ? dcf[row][j] : 0             (dcf = dc_t * f_t, left there by step t's element part)
// ELEM: the element part of step p = t - 1 on the same unit (lstm_cell_bwd with dh = d_out_p + dh_prev), which needs
// nothing else; hp_p = h_{p-1} * mask_p.  Without ELEM (after step 0) the carry is the gradient of the initial state:
// dh0 = dh_prev, dcf (= dc0) = dc_prev.
template <bool CARRY, bool ELEM>
__global__ __launch_bounds__(256) void k_lstm_bwd_step(
    const float* __restrict__ dgi_t, const float* __restrict__ Wt, const uint8_t* __restrict__ mask_t,
    const float* __restrict__ dout_p, int64_t ld_dout, const float* __restrict__ gi, const float* __restrict__ gf,
    const float* __restrict__ gg, const float* __restrict__ go, const float* __restrict__ c_p,
    const float* __restrict__ c_pp, int64_t ldc, const float* __restrict__ h_pp, int64_t ldh,
    const uint8_t* __restrict__ mask_p, int rows, int H, float* __restrict__ dcf, int64_t ld_dcf,
    float* __restrict__ dgi_p, float* __restrict__ hp_p, float* __restrict__ dh0, int64_t ld_dh0) {
    const int j = blockIdx.x;
    const int l = threadIdx.x & 31, rr = threadIdx.x >> 5;
    const int K = 4 * H;
    for (int r0 = 0; r0 < rows; r0 += 8) {
        const int row = r0 + rr;
        const bool row_ok = row < rows;
        const int rowc = row_ok ? row : 0;
        const int64_t idx = (int64_t)rowc * H + j;
        // the element part's inputs do not depend on the matvec: fetch them first, under its loads
        float e_dout = 0.f, e_c = 0.f, e_cpp = 0.f, e_h = 0.f, ig = 0.f, fg = 0.f, g_ = 0.f, og = 0.f;
        bool e_mp = false;
        if constexpr (ELEM) {
            e_dout = dout_p[(int64_t)rowc * ld_dout + j];
            e_c = c_p[idx], e_cpp = c_pp[(int64_t)rowc * ldc + j], e_h = h_pp[(int64_t)rowc * ldh + j];
            ig = gi[idx], fg = gf[idx], g_ = gg[idx], og = go[idx];
            e_mp = mask_p[rowc] != 0;
        }
        float dh_prev = 0.f, dc_prev = 0.f;
        if constexpr (CARRY) {
            const float e_dcf = dcf[(int64_t)rowc * ld_dcf + j];
            const bool e_mt = mask_t[rowc] != 0;
            const float v = skinny_dot32(Wt + (int64_t)j * K, dgi_t + (int64_t)rowc * K, K, l);
            dh_prev = e_mt ? v : 0.f;  // a masked step sends nothing into the previous state
            dc_prev = e_mt ? e_dcf : 0.f;
        }
        if (l == 0 && row_ok) {
            if constexpr (ELEM) {
                const LstmBwd b = lstm_cell_bwd(e_dout + dh_prev, dc_prev, e_mp ? e_cpp : 0.f, e_c, ig, fg, g_, og);
                const int64_t o = (int64_t)row * K + j;
#pragma unroll
                for (int g = 0; g < 4; ++g) dgi_p[o + g * H] = b.dgi[g];
                dcf[(int64_t)row * ld_dcf + j] = b.dcf;
                hp_p[idx] = e_mp ? e_h : 0.f;
            } else {
                dh0[(int64_t)row * ld_dh0 + j] = dh_prev;
                dcf[(int64_t)row * ld_dcf + j] = dc_prev;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Persistent sequence GRU
// ---------------------------------------------------------------------------------------------------------------
constexpr int HH = 512;          // hidden size these kernels are built for
constexpr int LPU = 32;          // lanes per unit
constexpr int SEQ_UPB = 8;       // hidden units per workgroup: 64 workgroups x 256 threads, one wave per SIMD
constexpr unsigned SPIN_MAX = 1u << 21;

typedef unsigned long long u64;

#ifdef GRU_SEQ_TIMING  // tools/gru_seq_phases.py: per-workgroup phase stamps of the forward kernel (100 MHz wall clock)
__device__ u64 g_seq_stamp[64 * 256 * 8];
#define SEQ_STAMP(t, k)                                                                             \
    do {                                                                                            \
        if (threadIdx.x == 0 && (t) < 256) g_seq_stamp[(blockIdx.x * 256 + (t)) * 8 + (k)] = wall_clock64(); \
    } while (0)
#else
#define SEQ_STAMP(t, k)
#endif

// 16-byte L1-bypassing (sc1) load through a buffer descriptor: a builtin, so the compiler tracks it in vmcnt and every
// load of a staging pass is in flight before the first wait (an 8-byte atomic load per iteration serialised N/2 memory
// round trips per step: 7.1 us per step, slower than the launches it replaced).
typedef int v4i __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld_pub16(__amdgpu_buffer_rsrc_t rsrc, unsigned byte_off) {
    const v4i x = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)byte_off, 0, /*aux: sc1*/ 16);
    return make_float4(__int_as_float(x.x), __int_as_float(x.y), __int_as_float(x.z), __int_as_float(x.w));
}

// sum over the 32 lanes of a unit's group on the DPP cross-lane path (VALU; __shfl_xor is an LDS permute per step):
// after the four row steps every lane of a 16-lane row holds the row's sum, row_bcast:15 then adds the lower row's
// sum into the upper row - the group total lives in lanes 16..31 of the group.
__device__ __forceinline__ float group_sum_hi(float v) {
#define IVLN_DPP_ADD(ctrl, row_mask)                                                                                   \
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, row_mask, 0xf, false))
    IVLN_DPP_ADD(0xB1, 0xf);   // quad_perm [1,0,3,2]
    IVLN_DPP_ADD(0x4E, 0xf);   // quad_perm [2,3,0,1]
    IVLN_DPP_ADD(0x141, 0xf);  // row_half_mirror
    IVLN_DPP_ADD(0x140, 0xf);  // row_mirror
    IVLN_DPP_ADD(0x142, 0xa);  // row_bcast:15 -> rows 1, 3 (the upper half of each 32-lane group)
#undef IVLN_DPP_ADD
    return v;
}

// The exchange in two halves, so that stores nobody waits for (the saved gates) and the next step's prefetches can be
// issued between them.  grid_arrive: every wave drains its write-through stores, one lane bumps the counter.
// (Gathering a workgroup's slice through LDS into a few 16-byte sc1 stores from one wave was measured and is not
// faster: 4.65 vs 4.71 us per forward step, 5.06 vs 4.94 backward - the extra barrier costs what the wide stores save.)
__device__ __forceinline__ void grid_arrive(unsigned* sync_ws) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave drains its write-through stores
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(&sync_ws[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// grid_wait: one lane polls (relaxed, bounded) until `target` arrivals; false on timeout (error word set).
__device__ __forceinline__ bool grid_wait(unsigned* sync_ws, unsigned target, int* s_fail) {
    if (threadIdx.x == 0) {
        bool ok = false;
        for (unsigned spins = 0; spins < SPIN_MAX; ++spins) {
            if (__hip_atomic_load(&sync_ws[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target) { ok = true; break; }
            if (__hip_atomic_load(&sync_ws[32], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;  // someone gave up
            __builtin_amdgcn_s_sleep(1);
        }
        if (!ok) {
            __hip_atomic_store(&sync_ws[32], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // this launch: everybody out
            __hip_atomic_store(&sync_ws[48], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // sticky: what the host reads
        }
        *s_fail = ok ? 0 : 1;
    }
    __syncthreads();
    return *s_fail == 0;
}

template <int UPB>
__global__ void __launch_bounds__(UPB * LPU)
k_gru_seq_fwd(const float* __restrict__ gi, const float* __restrict__ h0, int64_t ld_h0,
              const uint8_t* __restrict__ masks, const float* __restrict__ w_hh, const float* __restrict__ b_hh,
              float* out, int64_t ldo, float* __restrict__ state_out, int64_t ld_so, int T, int N,
              float* __restrict__ save_r, float* __restrict__ save_z, float* __restrict__ save_n,
              float* __restrict__ save_ghn, unsigned* sync_ws) {
    extern __shared__ __attribute__((aligned(16))) float s_h[];   // N x 512: h_{t-1} * mask_t, then one flag word
    int* s_fail_p = reinterpret_cast<int*>(s_h + N * HH);         // (no static LDS: the dynamic base stays 16-B aligned)
    if (sync_ws[49] != 0 && blockIdx.x == 1) return;  // test hook (word 49): this workgroup "is not resident" - the others' waits time out
    constexpr int NT = UPB * LPU, NWG = HH / UPB;
    const int tid = threadIdx.x, u = tid / LPU, l = tid % LPU;
    const int j = blockIdx.x * UPB + u;
    // the unit's three W_hh rows, lane slice (k = 4 l + 128 i), resident for the whole sequence
    float4 w[3][4];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            w[g][i] = *reinterpret_cast<const float4*>(w_hh + ((int64_t)g * HH + j) * HH + l * 4 + 128 * i);
    float bh[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) bh[g] = b_hh[g * HH + j];
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(
        out, 0, (int)((int64_t)T * N * ldo * sizeof(float)), 0x00020000);

    for (int t = 0; t < T; ++t) {
        const int64_t r0 = (int64_t)t * N;
        SEQ_STAMP(t, 0);
        // ---- stage h_{t-1} * mask_t into LDS (t == 0: the caller's h0, written before this launch) ----
        for (int e0 = 0; e0 < N * (HH / 4); e0 += NT * 4) {   // up to four 16-byte loads per thread in flight
            float4 v[4];
            const int last = N * (HH / 4) - 1;
            if (t == 0) {   // (uniform branch; the loads themselves are unconditional on clamped indices, so that the
                            // compiler issues all four before the first wait)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int e = min(e0 + q * NT + tid, last);
                    v[q] = *reinterpret_cast<const float4*>(h0 + (int64_t)(e / (HH / 4)) * ld_h0 + (e % (HH / 4)) * 4);
                }
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int e = min(e0 + q * NT + tid, last);
                    v[q] = ld_pub16(rs_out, (unsigned)(((r0 - N + e / (HH / 4)) * ldo + (e % (HH / 4)) * 4) * 4));
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = e0 + q * NT + tid;
                if (e <= last) {
                    const float mk = masks[r0 + e / (HH / 4)] ? 1.f : 0.f;
                    v[q].x *= mk, v[q].y *= mk, v[q].z *= mk, v[q].w *= mk;
                    *reinterpret_cast<float4*>(s_h + e * 4) = v[q];
                }
            }
        }
        __syncthreads();
        SEQ_STAMP(t, 1);
        float d_h = 0.f, d_sv[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        for (int nb = 0; nb < N; nb += 8) {
            // lane 16 + q of the group finishes row nb + q of the unit (the DPP reduction leaves the totals in the upper
            // half of the group): fetch its gate inputs under the matvec
            const int row = nb + l - 16;
            const bool mine = l >= 16 && l < 24 && row < N;
            float gin[3] = {0.f, 0.f, 0.f};
            if (mine) {
#pragma unroll
                for (int g = 0; g < 3; ++g) gin[g] = gi[(r0 + row) * 3 * HH + g * HH + j];
            }
            float acc[8][3];
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                acc[n][0] = acc[n][1] = acc[n][2] = 0.f;
                if (nb + n < N) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float4 hv = *reinterpret_cast<const float4*>(s_h + (nb + n) * HH + l * 4 + 128 * i);
#pragma unroll
                        for (int g = 0; g < 3; ++g) acc[n][g] = fma4(w[g][i], hv, acc[n][g]);
                    }
                }
            }
#pragma unroll
            for (int n = 0; n < 8; ++n)
#pragma unroll
                for (int g = 0; g < 3; ++g) acc[n][g] = group_sum_hi(acc[n][g]);
            SEQ_STAMP(t, 2);
            // lane 16 + q takes row nb + q (a select chain, not a dynamic register index)
            float ah[3] = {acc[0][0], acc[0][1], acc[0][2]};
#pragma unroll
            for (int n = 1; n < 8; ++n)
                if (l == 16 + n) { ah[0] = acc[n][0]; ah[1] = acc[n][1]; ah[2] = acc[n][2]; }
            if (mine) {
                const float gh[3] = {ah[0] + bh[0], ah[1] + bh[1], ah[2] + bh[2]};
                float sv[5];
                const float hn = gru_cell_fwd(gin, gh, s_h[row * HH + j], sv);
                st_pub(out + (r0 + row) * ldo + j, hn);   // the only store the other workgroups wait for
                if (N <= 8) {   // one row block: everything else is stored after the arrival (nobody waits for it)
                    d_h = hn;
#pragma unroll
                    for (int q = 0; q < 4; ++q) d_sv[q] = sv[q];
                } else {
                    if (state_out && t == T - 1) state_out[(int64_t)row * ld_so + j] = hn;
                    if (save_r) {
                        const int64_t o = (r0 + row) * HH + j;
                        save_r[o] = sv[0], save_z[o] = sv[1], save_n[o] = sv[2], save_ghn[o] = sv[3];
                    }
                }
            }
        }
        SEQ_STAMP(t, 3);
        if (t + 1 < T) grid_arrive(sync_ws);
        SEQ_STAMP(t, 4);
        if (N <= 8) {
            const int row = l - 16;
            if (l >= 16 && l < 24 && row < N) {
                if (state_out && t == T - 1) state_out[(int64_t)row * ld_so + j] = d_h;
                if (save_r) {
                    const int64_t o = (r0 + row) * HH + j;
                    save_r[o] = d_sv[0], save_z[o] = d_sv[1], save_n[o] = d_sv[2], save_ghn[o] = d_sv[3];
                }
            }
        }
        if (t + 1 < T && !grid_wait(sync_ws, (unsigned)NWG * (unsigned)(t + 1), s_fail_p)) return;
        SEQ_STAMP(t, 5);
    }
}

// backward (BPTT): element part of step T-1, then for t = T-1 .. 1 the carry of step t + the element part of t-1
struct ElemIn {
    float dout, h, r, z, n, ghn;
    bool mask;
};

struct ElemOut {   // what only later kernels read: stored after the arrival
    float dr, dz, dn, hp;
};

// The element part written out here, not through gru_cell_bwd: with the shared function the compiler pairs and orders the
// (1 - z) / (1 - r) / (1 - n^2) factors differently around the write-through stores, and the persistent BPTT measured
// 315-316 us against 312 at T = 64, N = 8 (profiles/state_rnn_refactor_ab.txt).  Same formulas, same association.
__device__ __forceinline__ ElemOut bwd_elem(const ElemIn& e, float carry, int64_t row, int j, float* dgh, float& dhz) {
    const float dh = e.dout + carry;
    const float hp = e.mask ? e.h : 0.f;
    const float dn = dh * (1.f - e.z);
    const float dz = dh * (hp - e.n);
    const float dn_pre = dn * (1.f - e.n * e.n);
    const float dz_pre = dz * e.z * (1.f - e.z);
    const float dr_pre = dn_pre * e.ghn * e.r * (1.f - e.r);
    const int64_t o = row * 3 * HH + j;
    st_pub(dgh + o, dr_pre);               // dgh rows are what the next step's matvec reads on every workgroup
    st_pub(dgh + o + HH, dz_pre);
    st_pub(dgh + o + 2 * HH, dn_pre * e.r);
    dhz = dh * e.z;
    return {dr_pre, dz_pre, dn_pre, hp};
}
__device__ __forceinline__ void bwd_store(const ElemOut& v, int64_t row, int j, float* __restrict__ dgi,
                                          float* __restrict__ hp_out) {
    const int64_t o = row * 3 * HH + j;
    dgi[o] = v.dr;
    dgi[o + HH] = v.dz;
    dgi[o + 2 * HH] = v.dn;
    hp_out[row * HH + j] = v.hp;
}

template <int UPB>
__global__ void __launch_bounds__(UPB * LPU)
k_gru_seq_bwd(const float* __restrict__ d_out, int64_t ld_dout, const float* __restrict__ r, const float* __restrict__ z,
              const float* __restrict__ n, const float* __restrict__ ghn, const float* __restrict__ out, int64_t ld_out,
              const float* __restrict__ h0, int64_t ld_h0, const uint8_t* __restrict__ masks,
              const float* __restrict__ whh_t, int T, int N, float* __restrict__ dgi, float* dgh,
              float* __restrict__ hp, unsigned* sync_ws) {
    extern __shared__ __attribute__((aligned(16))) float s_g[];   // N x 1536: dgh_t, then one flag word
    int* s_fail_p = reinterpret_cast<int*>(s_g + N * 3 * HH);
    if (sync_ws[49] != 0 && blockIdx.x == 1) return;  // test hook (word 49): this workgroup "is not resident" - the others' waits time out
    constexpr int K = 3 * HH, NT = UPB * LPU, NWG = HH / UPB;
    const int tid = threadIdx.x, u = tid / LPU, l = tid % LPU;
    const int j = blockIdx.x * UPB + u;
    float4 w[12];   // W_hh^T row j, lane slice
#pragma unroll
    for (int i = 0; i < 12; ++i) w[i] = *reinterpret_cast<const float4*>(whh_t + (int64_t)j * K + l * 4 + 128 * i);
    const int lr = l - 16;               // lane 16 + q of the group finishes row q of the unit (N <= 16)
    const bool mine = lr >= 0 && lr < N;
    const __amdgpu_buffer_rsrc_t rs_dgh = __builtin_amdgcn_make_buffer_rsrc(
        dgh, 0, (int)((int64_t)T * N * K * sizeof(float)), 0x00020000);
    auto load_elem = [&](int t) {   // inputs of the element part of step t for (row lr, unit j)
        ElemIn e;
        const int64_t row = (int64_t)t * N + lr, idx = row * HH + j;
        e.dout = d_out[row * ld_dout + j];
        e.h = t == 0 ? h0[(int64_t)lr * ld_h0 + j] : out[(row - N) * ld_out + j];
        e.r = r[idx], e.z = z[idx], e.n = n[idx], e.ghn = ghn[idx];
        e.mask = masks[row] != 0;
        return e;
    };
    float dhz = 0.f;
    ElemOut pend = {0.f, 0.f, 0.f, 0.f};
    if (mine) pend = bwd_elem(load_elem(T - 1), 0.f, (int64_t)(T - 1) * N + lr, j, dgh, dhz);
    unsigned epoch = 0;
    for (int t = T - 1; t > 0; --t) {
        grid_arrive(sync_ws);
        ElemIn e;
        bool mask_t = false;
        if (mine) {   // nothing here depends on the exchange: store / fetch it while the others arrive
            bwd_store(pend, (int64_t)t * N + lr, j, dgi, hp);
            e = load_elem(t - 1);
            mask_t = masks[(int64_t)t * N + lr] != 0;
        }
        if (!grid_wait(sync_ws, (unsigned)NWG * ++epoch, s_fail_p)) return;
        // ---- stage dgh_t (N x 1536) into LDS: 16-byte sc1 loads, six per thread in flight at N = 8 ----
        const unsigned src_off = (unsigned)((int64_t)t * N * K * 4);
        for (int e0 = 0; e0 < N * (K / 4); e0 += NT * 6) {
            float4 v[6];
            const int last = N * (K / 4) - 1;
#pragma unroll
            for (int q = 0; q < 6; ++q)   // unconditional loads on clamped indices: all six in flight before the first wait
                v[q] = ld_pub16(rs_dgh, src_off + (unsigned)min(e0 + q * NT + tid, last) * 16u);
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const int e = e0 + q * NT + tid;
                if (e <= last) *reinterpret_cast<float4*>(s_g + e * 4) = v[q];
            }
        }
        __syncthreads();
        float acc[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            acc[q] = 0.f;
            if (q < N) {
                float a0 = 0.f, a1 = 0.f;
#pragma unroll
                for (int i = 0; i < 12; ++i) fma4x2(w[i], *reinterpret_cast<const float4*>(s_g + q * K + l * 4 + 128 * i), a0, a1);
                acc[q] = a0 + a1;
            }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = group_sum_hi(acc[q]);
        float v = acc[0];
#pragma unroll
        for (int q = 1; q < 16; ++q)
            if (lr == q) v = acc[q];
        if (mine) {
            v = mask_t ? v + dhz : 0.f;   // dh carried into step t-1
            pend = bwd_elem(e, v, (int64_t)(t - 1) * N + lr, j, dgh, dhz);
        }
        __syncthreads();   // s_g is rewritten next step
    }
    if (mine) bwd_store(pend, (int64_t)lr, j, dgi, hp);   // step 0
}

// The persistent kernels spin on counters that every workgroup of the grid feeds: the whole grid has to be resident at
// once.  On a partitioned device (CPX: 32 CUs), a CU-masked stream or a large N (up to 128 KB of LDS per workgroup)
// it may not be - then the caller runs the per-step launches (IVLN_E_UNSUPPORTED), instead of every grid_wait spinning
// to its bound (csrc/residency.h: the answer is cached per device, kernel and LDS bytes).  Sets the kernel's dynamic-LDS
// limit once, zeroes the counters with a memset node, launches.
template <class... KArgs, class... Args>
int launch_persistent(void (*kernel)(KArgs...), bool& attr_set, int max_lds, size_t lds, void* sync_ws, hipStream_t s,
                      Args... args) {
    const void* fn = reinterpret_cast<const void*>(kernel);
    if (!attr_set) {
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds) != hipSuccess) return IVLN_E_HIP;
        attr_set = true;
    }
    if (ivln_resident_blocks(fn, SEQ_UPB * LPU, lds) < HH / SEQ_UPB) return IVLN_E_UNSUPPORTED;
    if (hipMemsetAsync(sync_ws, 0, 192, s) != hipSuccess) return IVLN_E_HIP;
    hipLaunchKernelGGL(kernel, dim3(HH / SEQ_UPB), dim3(SEQ_UPB * LPU), lds, s, args..., (unsigned*)sync_ws);
    return LAUNCH_OK();
}

int gru_seq_fwd_persistent(const float* gi, const float* h0, int64_t ld_h0, const uint8_t* masks, const float* w_hh,
                           const float* b_hh, float* out, int64_t ldo, float* state_out, int64_t ld_so, int T, int N,
                           float* save_r, float* save_z, float* save_n, float* save_ghn, void* sync_ws, hipStream_t s) {
    if ((int64_t)T * N * ldo * (int64_t)sizeof(float) >= (int64_t)1 << 31) return IVLN_E_UNSUPPORTED;  // 32-bit buffer offsets
    // the exchange reads `out` / h0 with 16-byte buffer loads
    if (!al16(out) || !al16(h0) || (ldo & 3) || (ld_h0 & 3)) return IVLN_E_UNSUPPORTED;
    static bool attr_set = false;
    return launch_persistent(k_gru_seq_fwd<SEQ_UPB>, attr_set, 64 * HH * (int)sizeof(float) + 16,
                             (size_t)N * HH * sizeof(float) + 16, sync_ws, s, gi, h0, ld_h0, masks, w_hh, b_hh, out, ldo,
                             state_out, ld_so, T, N, save_r, save_z, save_n, save_ghn);
}

int gru_seq_bwd_persistent(const float* d_out, int64_t ld_dout, const float* r, const float* z, const float* n,
                           const float* ghn, const float* out, int64_t ld_out, const float* h0, int64_t ld_h0,
                           const uint8_t* masks, const float* whh_t, int T, int N, float* dgi, float* dgh, float* hp,
                           void* sync_ws, hipStream_t s) {
    if ((int64_t)T * N * 3 * HH * (int64_t)sizeof(float) >= (int64_t)1 << 31) return IVLN_E_UNSUPPORTED;
    if (!al16(dgh)) return IVLN_E_UNSUPPORTED;  // (16-byte buffer loads of the exchanged dgh rows)
    static bool attr_set = false;
    return launch_persistent(k_gru_seq_bwd<SEQ_UPB>, attr_set, 16 * 3 * HH * (int)sizeof(float) + 16,
                             (size_t)N * 3 * HH * sizeof(float) + 16, sync_ws, s, d_out, ld_dout, r, z, n, ghn, out, ld_out,
                             h0, ld_h0, masks, whh_t, T, N, dgi, dgh, hp);
}

}  // namespace

extern "C" {

int ivln_gru_step_f32(const float* x, int64_t ldx, int I, const float* gi_pre, int64_t ldgi, const float* h_in,
                      int64_t ldh, const uint8_t* mask, const float* w_ih, const float* w_hh, const float* b_ih,
                      const float* b_hh, float* h_out, int64_t ldo, float* h_out2, int64_t ldo2, int rows, int H,
                      float* save_r, float* save_z, float* save_n, float* save_ghn, void* stream) {
    if (rows <= 0 || (H & 3) || (x && (I & 3)) || (ldh & 3) || (x && (ldx & 3))) return IVLN_E_INVALID;
    // every operand of the dot products is read with 16-byte loads and the kernel has no scalar form
    if (!al16(h_in) || !al16(w_hh) || (x && (!al16(x) || !al16(w_ih)))) return IVLN_E_INVALID;
    launch_step<GruCell>(x, ldx, I, gi_pre, ldgi, h_in, ldh, nullptr, 0, mask, w_ih, w_hh, b_ih, b_hh, h_out, ldo, h_out2,
                         ldo2, nullptr, 0, rows, H, {{save_r, save_z, save_n, save_ghn, nullptr}}, (hipStream_t)stream);
    return LAUNCH_OK();
}

/* 1 when ivln_cma_seq_fwd_f32 / _bwd_f32 take the single-launch path for this shape (given a sync_ws). */
int ivln_cma_seq_persistent_ok(int N, int H, int backward) {
    return H == HH && N >= 1 && N <= (backward ? 16 : 64);
}

/* Zeroes a sync workspace (256 bytes), including the sticky error word that the launches never clear. */
int ivln_seq_sync_init(void* sync_ws, void* stream) {
    if (!sync_ws) return IVLN_E_INVALID;
    return hipMemsetAsync(sync_ws, 0, 256, (hipStream_t)stream) == hipSuccess ? IVLN_OK : IVLN_E_HIP;
}

/* Synchronises `stream` and reads the error word of a sync workspace: IVLN_OK, or IVLN_E_HIP when a spin of the
 * last persistent launch timed out (its outputs are then undefined). */
/* (word 49 of a sync workspace: test hook, see the kernels; cleared by ivln_seq_sync_init like everything else) */
int ivln_seq_sync_status(const void* sync_ws, void* stream) {
    unsigned err = 0;
    if (hipMemcpyAsync(&err, (const unsigned*)sync_ws + 48, sizeof(err), hipMemcpyDeviceToHost, (hipStream_t)stream) !=
        hipSuccess)
        return IVLN_E_HIP;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return IVLN_E_HIP;
    return err ? IVLN_E_HIP : IVLN_OK;
}

/* GRU over a whole time-major sequence batch in ONE call: one persistent launch inside the envelope, else T dependent
 * step launches.  gi = W_ih x + b_ih for all T*N rows (one GEMM, done by the caller). */
int ivln_cma_seq_fwd_f32(const float* gi, const float* h0, int64_t ld_h0, const uint8_t* masks, const float* w_hh,
                         const float* b_hh, float* out, int64_t ldo, float* state_out, int64_t ld_so, int T, int N,
                         int H, float* save_r, float* save_z, float* save_n, float* save_ghn, void* sync_ws,
                         void* stream) {
    if (!gi || !h0 || !masks || !w_hh || !b_hh || !out || T <= 0 || N <= 0 || (H & 3) || (ld_h0 & 3) || (ldo & 3))
        return IVLN_E_INVALID;
    if (sync_ws && T > 1 && ivln_cma_seq_persistent_ok(N, H, 0)) {
        const int rc = gru_seq_fwd_persistent(gi, h0, ld_h0, masks, w_hh, b_hh, out, ldo, state_out, ld_so, T, N, save_r,
                                              save_z, save_n, save_ghn, sync_ws, (hipStream_t)stream);
        if (rc != IVLN_E_UNSUPPORTED) return rc;
    }
    const Saves all = {{save_r, save_z, save_n, save_ghn, nullptr}};
    for (int t = 0; t < T; ++t) {
        const int64_t r0 = (int64_t)t * N;
        launch_step<GruCell>(nullptr, 0, 0, gi + r0 * 3 * H, (int64_t)3 * H, t == 0 ? h0 : out + (r0 - N) * ldo,
                             t == 0 ? ld_h0 : ldo, nullptr, 0, masks + r0, nullptr, w_hh, nullptr, b_hh, out + r0 * ldo, ldo,
                             t == T - 1 ? state_out : nullptr, ld_so, nullptr, 0, N, H, saves_at(all, r0 * H), (hipStream_t)stream);
    }
    return LAUNCH_OK();
}

int ivln_gru_bwd_elem_f32(const float* dout, int64_t ld_dout, const float* dh_carry, const float* r, const float* z,
                          const float* n, const float* ghn, const float* h_prev, int64_t ldh, const uint8_t* mask,
                          int rows, int H, float* dgi, float* dgh, float* dhz, float* hp_out, void* stream) {
    hipLaunchKernelGGL(k_gru_bwd_elem, dim3((unsigned)(((int64_t)rows * H + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       dout, ld_dout, dh_carry, r, z, n, ghn, h_prev, ldh, mask, rows, H, dgi, dgh, dhz, hp_out);
    return LAUNCH_OK();
}

int ivln_gru_bwd_step_f32(const float* dgh_t, int64_t ld_dgh, const float* whh_t, const uint8_t* mask_t,
                          const float* dout_prev, int64_t ld_dout, const float* r, const float* z, const float* n,
                          const float* ghn, const float* h_prev, int64_t ldh, const uint8_t* mask_prev, int rows, int H,
                          float* dhz, float* dgi_prev, float* dgh_prev, float* hp_prev, void* stream) {
    if ((H & 3) || (ld_dgh & 3) || rows <= 0) return IVLN_E_INVALID;
    hipLaunchKernelGGL(k_gru_bwd_step, dim3(H), dim3(256), 0, (hipStream_t)stream, dgh_t, ld_dgh, whh_t, mask_t,
                       dout_prev, ld_dout, r, z, n, ghn, h_prev, ldh, mask_prev, rows, H, dhz, dgi_prev, dgh_prev,
                       hp_prev);
    return LAUNCH_OK();
}

/* BPTT of ivln_cma_seq_fwd_f32 in one call: one persistent launch inside the envelope, else the element part of step
 * T-1, then T-1 fused (carry of step t + element part of step t-1) launches.  whh_t = W_hh^T (H, 3H).  Outputs dgi / dgh
 * (T*N, 3H), hp = h_prev * mask (T*N, H); dhz (N, H) is scratch. */
int ivln_cma_seq_bwd_f32(const float* d_out, int64_t ld_dout, const float* r, const float* z, const float* n,
                         const float* ghn, const float* out, int64_t ld_out, const float* h0, int64_t ld_h0,
                         const uint8_t* masks, const float* whh_t, int T, int N, int H, float* dgi, float* dgh, float* hp,
                         float* dhz, void* sync_ws, void* stream) {
    if (!d_out || !r || !out || !h0 || !masks || !whh_t || !dgi || !dgh || !hp || !dhz || T <= 0 || N <= 0 || (H & 3))
        return IVLN_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (sync_ws && T > 1 && ivln_cma_seq_persistent_ok(N, H, 1)) {
        const int rc = gru_seq_bwd_persistent(d_out, ld_dout, r, z, n, ghn, out, ld_out, h0, ld_h0, masks, whh_t, T, N, dgi,
                                              dgh, hp, sync_ws, s);
        if (rc != IVLN_E_UNSUPPORTED) return rc;
    }
    auto hprev = [&](int t, int64_t& ld) -> const float* {  // hidden state entering step t
        ld = t == 0 ? ld_h0 : ld_out;
        return t == 0 ? h0 : out + (int64_t)(t - 1) * N * ld_out;
    };
    {
        const int64_t r0 = (int64_t)(T - 1) * N;
        int64_t ld;
        const float* hpv = hprev(T - 1, ld);
        hipLaunchKernelGGL(k_gru_bwd_elem, dim3((unsigned)(((int64_t)N * H + 255) / 256)), dim3(256), 0, s,
                           d_out + r0 * ld_dout, ld_dout, (const float*)nullptr, r + r0 * H, z + r0 * H, n + r0 * H,
                           ghn + r0 * H, hpv, ld, masks + r0, N, H, dgi + r0 * 3 * H, dgh + r0 * 3 * H, dhz, hp + r0 * H);
    }
    for (int t = T - 1; t > 0; --t) {
        const int64_t rt = (int64_t)t * N, rp = (int64_t)(t - 1) * N;
        int64_t ld;
        const float* hpp = hprev(t - 1, ld);
        hipLaunchKernelGGL(k_gru_bwd_step, dim3(H), dim3(256), 0, s, dgh + rt * 3 * H, (int64_t)3 * H, whh_t, masks + rt,
                           d_out + rp * ld_dout, ld_dout, r + rp * H, z + rp * H, n + rp * H, ghn + rp * H, hpp, ld,
                           masks + rp, N, H, dhz, dgi + rp * 3 * H, dgh + rp * 3 * H, hp + rp * H);
    }
    return LAUNCH_OK();
}

int ivln_lstm_step_f32(const float* x, int64_t ldx, int I, const float* gi_pre, int64_t ldgi, const float* h_in,
                       int64_t ldh, const float* c_in, int64_t ldc, const uint8_t* mask, const float* w_ih,
                       const float* w_hh, const float* b_ih, const float* b_hh, float* h_out, int64_t ldo, float* h_out2,
                       int64_t ldo2, float* c_out, int64_t ldco, int rows, int H, float* save_i, float* save_f,
                       float* save_g, float* save_o, float* save_c, void* stream) {
    if (rows <= 0 || H <= 0 || (H & 3) || !h_in || !c_in || !w_hh || !h_out || !c_out) return IVLN_E_INVALID;
    if ((x != nullptr) == (gi_pre != nullptr)) return IVLN_E_INVALID;  // exactly one of the two input forms
    if (x && (!w_ih || I <= 0)) return IVLN_E_INVALID;
    if (save_i && (!save_f || !save_g || !save_o || !save_c)) return IVLN_E_INVALID;
    launch_step<LstmCell>(x, ldx, I, gi_pre, ldgi, h_in, ldh, c_in, ldc, mask, w_ih, w_hh, b_ih, b_hh, h_out, ldo, h_out2,
                          ldo2, c_out, ldco, rows, H, {{save_i, save_f, save_g, save_o, save_c}}, (hipStream_t)stream);
    return LAUNCH_OK();
}

int ivln_lstm_seq_fwd_f32(const float* gi, const float* h0, int64_t ld_h0, const float* c0, int64_t ld_c0,
                          const uint8_t* masks, const float* w_hh, const float* b_hh, float* out, int64_t ldo,
                          float* h_state_out, int64_t ld_hs, float* c_state_out, int64_t ld_cs, int T, int N, int H,
                          float* save_i, float* save_f, float* save_g, float* save_o, float* save_c, void* stream) {
    if (!gi || !h0 || !c0 || !masks || !w_hh || !out || !c_state_out || T <= 0 || N <= 0 || H <= 0 || (H & 3))
        return IVLN_E_INVALID;
    if (save_i && (!save_f || !save_g || !save_o || !save_c)) return IVLN_E_INVALID;
    const Saves all = {{save_i, save_f, save_g, save_o, save_c}};
    for (int t = 0; t < T; ++t) {
        const int64_t r0 = (int64_t)t * N;
        // the cell state lives in c_state_out from step 0 on and is advanced in place
        launch_step<LstmCell>(nullptr, 0, 0, gi + r0 * 4 * H, (int64_t)4 * H, t == 0 ? h0 : out + (r0 - N) * ldo,
                              t == 0 ? ld_h0 : ldo, t == 0 ? c0 : c_state_out, t == 0 ? ld_c0 : ld_cs, masks + r0, nullptr,
                              w_hh, nullptr, b_hh, out + r0 * ldo, ldo, t == T - 1 ? h_state_out : nullptr, ld_hs,
                              c_state_out, ld_cs, N, H, saves_at(all, r0 * H), (hipStream_t)stream);
    }
    return LAUNCH_OK();
}

int ivln_lstm_seq_tour_fwd_f32(const float* gi_base, const float* w_ih, int I0, const float* w_hh, const float* b_hh,
                               const float* h0, int64_t ld_h0, const float* c0, int64_t ld_c0, const float* mem0,
                               int64_t ld_m0, const uint8_t* ep_masks, const uint8_t* tour_masks, float* out, int64_t ldo,
                               float* mem_in, int64_t ld_mi, float* h_state_out, int64_t ld_hs, float* c_state_out,
                               int64_t ld_cs, float* mem_state_out, int64_t ld_ms, int T, int N, int H, float* save_i,
                               float* save_f, float* save_g, float* save_o, float* save_c, void* stream) {
    if (!gi_base || !w_ih || !w_hh || !h0 || !c0 || !mem0 || !ep_masks || !tour_masks || !out || !mem_in || !c_state_out ||
        !mem_state_out || T <= 0 || N <= 0 || H <= 0 || (H & 3) || I0 <= 0)
        return IVLN_E_INVALID;
    if (save_i && (!save_f || !save_g || !save_o || !save_c)) return IVLN_E_INVALID;
    if (ld_h0 < H || ld_c0 < H || ld_m0 < H || ldo < H || ld_mi < H || ld_cs < H || ld_ms < H || (h_state_out && ld_hs < H))
        return IVLN_E_INVALID;
    // every workgroup reads whole rows of h0 / mem0 (and element (n, j) of c0) while others write: no output may overlap them
    const int64_t TN = (int64_t)T * N;
    const Span outs[] = {span_of(out, TN, ldo, H),          span_of(mem_in, TN, ld_mi, H),
                         span_of(h_state_out, N, ld_hs, H), span_of(c_state_out, N, ld_cs, H),
                         span_of(mem_state_out, N, ld_ms, H), span_of(save_i, TN, H, H),
                         span_of(save_f, TN, H, H),         span_of(save_g, TN, H, H),
                         span_of(save_o, TN, H, H),         span_of(save_c, TN, H, H)};
    const Span ins[] = {span_of(h0, N, ld_h0, H), span_of(mem0, N, ld_m0, H), span_of(c0, N, ld_c0, H)};
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 10; ++b) {
            if (a == 2 && b == 3 && c0 == c_state_out && ld_c0 == ld_cs) continue;  // the cell state advanced in place
            if (overlap(ins[a], outs[b])) return IVLN_E_INVALID;
        }
    launch_tour_seq<LstmCell>(gi_base, w_ih, I0, w_hh, b_hh, h0, ld_h0, c0, ld_c0, mem0, ld_m0, ep_masks, tour_masks, out,
                              ldo, mem_in, ld_mi, h_state_out, ld_hs, c_state_out, ld_cs, mem_state_out, ld_ms, T, N, H,
                              {{save_i, save_f, save_g, save_o, save_c}}, (hipStream_t)stream);
    return LAUNCH_OK();
}

int ivln_lstm_seq_bwd_f32(const float* d_out, int64_t ld_dout, const float* save_i, const float* save_f,
                          const float* save_g, const float* save_o, const float* save_c, const float* out, int64_t ld_out,
                          const float* h0, int64_t ld_h0, const float* c0, int64_t ld_c0, const uint8_t* masks,
                          const float* whh_t, int T, int N, int H, float* dgi, float* hp, float* dh0, int64_t ld_dh0,
                          float* dc0, int64_t ld_dc0, void* stream) {
    if (!d_out || !save_i || !save_f || !save_g || !save_o || !save_c || !out || !h0 || !c0 || !masks || !whh_t || !dgi ||
        !hp || !dh0 || !dc0 || T <= 0 || N <= 0 || H <= 0 || (H & 3))
        return IVLN_E_INVALID;
    if (!al16(whh_t) || !al16(dgi)) return IVLN_E_INVALID;  // rows of 4H floats, read with 16-byte loads
    hipStream_t s = (hipStream_t)stream;
    const int64_t G = (int64_t)4 * H;
    auto elem_args = [&](int p, const float*& cpp, int64_t& ldc, const float*& hpp, int64_t& ldh) {  // state entering step p
        cpp = p == 0 ? c0 : save_c + (int64_t)(p - 1) * N * H;
        ldc = p == 0 ? ld_c0 : H;
        hpp = p == 0 ? h0 : out + (int64_t)(p - 1) * N * ld_out;
        ldh = p == 0 ? ld_h0 : ld_out;
    };
    const float *cpp, *hpp;
    int64_t ldc, ldh;
    {   // step T-1: nothing is carried into it; dc0 is the running dc * f from here on
        const int64_t r0 = (int64_t)(T - 1) * N;
        elem_args(T - 1, cpp, ldc, hpp, ldh);
        hipLaunchKernelGGL((k_lstm_bwd_step<false, true>), dim3(H), dim3(256), 0, s, (const float*)nullptr,
                           (const float*)nullptr, (const uint8_t*)nullptr, d_out + r0 * ld_dout, ld_dout, save_i + r0 * H,
                           save_f + r0 * H, save_g + r0 * H, save_o + r0 * H, save_c + r0 * H, cpp, ldc, hpp, ldh,
                           masks + r0, N, H, dc0, ld_dc0, dgi + r0 * G, hp + r0 * H, (float*)nullptr, (int64_t)0);
    }
    for (int t = T - 1; t > 0; --t) {
        const int64_t rt = (int64_t)t * N, rp = (int64_t)(t - 1) * N;
        elem_args(t - 1, cpp, ldc, hpp, ldh);
        hipLaunchKernelGGL((k_lstm_bwd_step<true, true>), dim3(H), dim3(256), 0, s, dgi + rt * G, whh_t, masks + rt,
                           d_out + rp * ld_dout, ld_dout, save_i + rp * H, save_f + rp * H, save_g + rp * H,
                           save_o + rp * H, save_c + rp * H, cpp, ldc, hpp, ldh, masks + rp, N, H, dc0, ld_dc0,
                           dgi + rp * G, hp + rp * H, (float*)nullptr, (int64_t)0);
    }
    // what step 0 sends into the initial state
    hipLaunchKernelGGL((k_lstm_bwd_step<true, false>), dim3(H), dim3(256), 0, s, dgi, whh_t, masks, (const float*)nullptr,
                       (int64_t)0, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr,
                       (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (int64_t)0,
                       (const float*)nullptr, (int64_t)0, (const uint8_t*)nullptr, N, H, dc0, ld_dc0, (float*)nullptr,
                       (float*)nullptr, dh0, ld_dh0);
    return LAUNCH_OK();
}

#ifdef GRU_SEQ_TIMING
int ivln_gru_seq_stamps(void* host, int bytes) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_seq_stamp), bytes) == hipSuccess ? 0 : -1;
}
#endif

}  // extern "C"
