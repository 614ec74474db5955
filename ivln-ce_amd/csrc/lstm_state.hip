// Masked LSTM state encoder for gfx950 (STATE_ENCODER.rnn_type LSTM): one step, the time-major sequence and its BPTT.
// habitat-lab's RNNStateEncoder wrapping nn.LSTM(input, hidden, num_layers=1), built by the reference with
// rnn_type=model_config.STATE_ENCODER.rnn_type (ivlnce_baselines/models/map_cma_policy.py:183,229) and run over the
// state slices of :290-351.  Gate order is torch's: i, f, g, o.  All fp32 in, out and accumulation.
//
//   h' = h * mask, c' = c * mask;  gates = W_ih x + b_ih + W_hh h' + b_hh
//   c_t = s(f) c' + s(i) tanh(g);  h_t = s(o) tanh(c_t)
//
// Work split (the masked GRU step's, csrc/nn_ops.hip k_gru_step): at rollout size (rows <= 8, H = 512) a step streams
// W_hh once (4 MB) and does 8 MFLOP - bound by HBM/L2 bandwidth and by load latency, not a matrix-core problem.  One
// workgroup per hidden unit j reads the four gate rows of W_hh (and W_ih) for that unit; 32 or 64 lanes share one state
// row, each lane owns every LPR-th float4 of K, so a (row, unit) costs one shuffle reduction and no LDS or barrier.  H
// workgroups of 256 threads cover the chip twice at H = 512.  A sequence is T such launches enqueued back to back from
// one C call; there is no single-launch (persistent) form of this encoder.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/ivln_hip.h"

namespace {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP)

__device__ __forceinline__ float fma4(const float4 w, const float4 v, float a) {
    a = fmaf(w.x, v.x, a);
    a = fmaf(w.y, v.y, a);
    a = fmaf(w.z, v.z, a);
    return fmaf(w.w, v.w, a);
}

// One masked step for `rows` states.  VEC: 16-byte loads (every row of x / h_in / W_ih / W_hh 16-byte aligned), else
// 4-byte loads with the same lane-strided split of K.  c_in and c_out may be the same memory (element (row, j) is read
// and then written by one thread only); h_in must not overlap h_out / h_out2 (every workgroup reads whole rows of h_in).
template <int LPR, bool VEC>
__global__ __launch_bounds__(256) void k_lstm_step(const float* __restrict__ x, int64_t ldx, int I,
                                                   const float* __restrict__ gi_pre, int64_t ldgi,
                                                   const float* __restrict__ h_in, int64_t ldh, const float* c_in,
                                                   int64_t ldc, const uint8_t* __restrict__ mask,
                                                   const float* __restrict__ w_ih, const float* __restrict__ w_hh,
                                                   const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                                   float* __restrict__ h_out, int64_t ldo, float* __restrict__ h_out2,
                                                   int64_t ldo2, float* c_out, int64_t ldco, int rows, int H,
                                                   float* __restrict__ save_i, float* __restrict__ save_f,
                                                   float* __restrict__ save_g, float* __restrict__ save_o,
                                                   float* __restrict__ save_c) {
    constexpr int RPB = 256 / LPR;  // rows per pass
    const int j = blockIdx.x;
    const int l = threadIdx.x % LPR, rr = threadIdx.x / LPR;
    for (int r0 = 0; r0 < rows; r0 += RPB) {
        const int row = r0 + rr;
        const bool row_ok = row < rows;
        const int rowc = row_ok ? row : 0;
        float ai[4] = {0.f, 0.f, 0.f, 0.f}, ah[4] = {0.f, 0.f, 0.f, 0.f};
        if (x) {
            const float* xr = x + (int64_t)rowc * ldx;
            if constexpr (VEC) {
                for (int k = l * 4; k < I; k += LPR * 4) {
                    const float4 xv = *reinterpret_cast<const float4*>(xr + k);
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        ai[g] = fma4(*reinterpret_cast<const float4*>(w_ih + ((int64_t)g * H + j) * I + k), xv, ai[g]);
                }
            } else {
                for (int k = l; k < I; k += LPR) {
                    const float xv = xr[k];
#pragma unroll
                    for (int g = 0; g < 4; ++g) ai[g] = fmaf(w_ih[((int64_t)g * H + j) * I + k], xv, ai[g]);
                }
            }
        }
        const float mk = mask ? (mask[rowc] ? 1.f : 0.f) : 1.f;
        const float* hr = h_in + (int64_t)rowc * ldh;
        if constexpr (VEC) {
            for (int k = l * 4; k < H; k += LPR * 4) {
                float4 hv = *reinterpret_cast<const float4*>(hr + k);
                hv.x *= mk, hv.y *= mk, hv.z *= mk, hv.w *= mk;
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    ah[g] = fma4(*reinterpret_cast<const float4*>(w_hh + ((int64_t)g * H + j) * H + k), hv, ah[g]);
            }
        } else {
            for (int k = l; k < H; k += LPR) {
                const float hv = hr[k] * mk;
#pragma unroll
                for (int g = 0; g < 4; ++g) ah[g] = fmaf(w_hh[((int64_t)g * H + j) * H + k], hv, ah[g]);
            }
        }
#pragma unroll
        for (int off = LPR / 2; off > 0; off >>= 1) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (x) ai[g] += __shfl_xor(ai[g], off, 64);
                ah[g] += __shfl_xor(ah[g], off, 64);
            }
        }
        if (l == 0 && row_ok) {
            float pre[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float gi = x ? ai[g] + (b_ih ? b_ih[g * H + j] : 0.f) : gi_pre[(int64_t)row * ldgi + g * H + j];
                pre[g] = gi + (ah[g] + (b_hh ? b_hh[g * H + j] : 0.f));
            }
            const float cp = c_in[(int64_t)row * ldc + j] * mk;
            const float ig = sigmoidf_(pre[0]), fg = sigmoidf_(pre[1]), gg = tanhf(pre[2]), og = sigmoidf_(pre[3]);
            const float ct = fg * cp + ig * gg;
            const float ht = og * tanhf(ct);
            h_out[(int64_t)row * ldo + j] = ht;
            if (h_out2) h_out2[(int64_t)row * ldo2 + j] = ht;
            c_out[(int64_t)row * ldco + j] = ct;
            if (save_i) {
                const int64_t e = (int64_t)row * H + j;
                save_i[e] = ig, save_f[e] = fg, save_g[e] = gg, save_o[e] = og, save_c[e] = ct;
            }
        }
    }
}

// One BPTT step in one launch, workgroup j = hidden unit j (the masked GRU's k_gru_bwd_step, csrc/train_ops.hip).
// CARRY: what step t sends back into unit j of the previous state,
//   dh_prev[row][j] = mask_t[row] ? Wt[j] . dgi_t[row] : 0      (Wt = W_hh^T, (H, 4H))
//   dc_prev[row][j] = mask_t[row] ? dcf[row][j] : 0             (dcf = dc_t * f_t, left there by step t's element part)
// ELEM: the element part of step p = t - 1 on the same unit, which needs nothing else:
//   dh = d_out_p + dh_prev;  dc = dc_prev + dh o (1 - tanh(c_p)^2)
//   dgi_p = [dc g i(1-i), dc c'_{p-1} f(1-f), dc i (1-g^2), dh tanh(c_p) o(1-o)];  dcf = dc f;  hp_p = h_{p-1} * mask_p
// without ELEM (after step 0) the carry is the gradient of the initial state: dh0 = dh_prev, dcf (= dc0) = dc_prev.
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
            const float* wr = Wt + (int64_t)j * K;
            const float* xr = dgi_t + (int64_t)rowc * K;
            float a0 = 0.f, a1 = 0.f;
            for (int k = l * 4; k < K; k += 128) {
                const float4 wv = *reinterpret_cast<const float4*>(wr + k);
                const float4 xv = *reinterpret_cast<const float4*>(xr + k);
                a0 = fmaf(wv.x, xv.x, a0);
                a1 = fmaf(wv.y, xv.y, a1);
                a0 = fmaf(wv.z, xv.z, a0);
                a1 = fmaf(wv.w, xv.w, a1);
            }
            float v = a0 + a1;
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            dh_prev = e_mt ? v : 0.f;  // a masked step sends nothing into the previous state
            dc_prev = e_mt ? e_dcf : 0.f;
        }
        if (l == 0 && row_ok) {
            if constexpr (ELEM) {
                const float dh = e_dout + dh_prev;
                const float tc = tanhf(e_c);
                const float dc = dc_prev + dh * og * (1.f - tc * tc);
                const float cp = e_mp ? e_cpp : 0.f;
                const int64_t o = (int64_t)row * K + j;
                dgi_p[o] = dc * g_ * ig * (1.f - ig);
                dgi_p[o + H] = dc * cp * fg * (1.f - fg);
                dgi_p[o + 2 * H] = dc * ig * (1.f - g_ * g_);
                dgi_p[o + 3 * H] = dh * tc * og * (1.f - og);
                dcf[(int64_t)row * ld_dcf + j] = dc * fg;
                hp_p[idx] = e_mp ? e_h : 0.f;
            } else {
                dh0[(int64_t)row * ld_dh0 + j] = dh_prev;
                dcf[(int64_t)row * ld_dcf + j] = dc_prev;
            }
        }
    }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int launch_step(const float* x, int64_t ldx, int I, const float* gi_pre, int64_t ldgi, const float* h_in, int64_t ldh,
                const float* c_in, int64_t ldc, const uint8_t* mask, const float* w_ih, const float* w_hh,
                const float* b_ih, const float* b_hh, float* h_out, int64_t ldo, float* h_out2, int64_t ldo2, float* c_out,
                int64_t ldco, int rows, int H, float* si, float* sf, float* sg, float* so, float* sc, hipStream_t s) {
    const bool vec = al16(h_in) && al16(w_hh) && !(ldh & 3) && (!x || (al16(x) && al16(w_ih) && !(I & 3) && !(ldx & 3)));
#define IVLN_LSTM_STEP(LPR, VEC)                                                                                          \
    hipLaunchKernelGGL((k_lstm_step<LPR, VEC>), dim3(H), dim3(256), 0, s, x, ldx, I, gi_pre, ldgi, h_in, ldh, c_in, ldc,  \
                       mask, w_ih, w_hh, b_ih, b_hh, h_out, ldo, h_out2, ldo2, c_out, ldco, rows, H, si, sf, sg, so, sc)
    if (rows <= 4) {
        if (vec) IVLN_LSTM_STEP(64, true); else IVLN_LSTM_STEP(64, false);
    } else {
        if (vec) IVLN_LSTM_STEP(32, true); else IVLN_LSTM_STEP(32, false);
    }
#undef IVLN_LSTM_STEP
    return IVLN_OK;
}

}  // namespace

extern "C" {

int ivln_lstm_step_f32(const float* x, int64_t ldx, int I, const float* gi_pre, int64_t ldgi, const float* h_in,
                       int64_t ldh, const float* c_in, int64_t ldc, const uint8_t* mask, const float* w_ih,
                       const float* w_hh, const float* b_ih, const float* b_hh, float* h_out, int64_t ldo, float* h_out2,
                       int64_t ldo2, float* c_out, int64_t ldco, int rows, int H, float* save_i, float* save_f,
                       float* save_g, float* save_o, float* save_c, void* stream) {
    if (rows <= 0 || H <= 0 || (H & 3) || !h_in || !c_in || !w_hh || !h_out || !c_out) return IVLN_E_INVALID;
    if ((x != nullptr) == (gi_pre != nullptr)) return IVLN_E_INVALID;  // exactly one of the two input forms
    if (x && (!w_ih || I <= 0)) return IVLN_E_INVALID;
    if (save_i && (!save_f || !save_g || !save_o || !save_c)) return IVLN_E_INVALID;
    launch_step(x, ldx, I, gi_pre, ldgi, h_in, ldh, c_in, ldc, mask, w_ih, w_hh, b_ih, b_hh, h_out, ldo, h_out2, ldo2,
                c_out, ldco, rows, H, save_i, save_f, save_g, save_o, save_c, (hipStream_t)stream);
    return LAUNCH_OK();
}

int ivln_lstm_seq_fwd_f32(const float* gi, const float* h0, int64_t ld_h0, const float* c0, int64_t ld_c0,
                          const uint8_t* masks, const float* w_hh, const float* b_hh, float* out, int64_t ldo,
                          float* h_state_out, int64_t ld_hs, float* c_state_out, int64_t ld_cs, int T, int N, int H,
                          float* save_i, float* save_f, float* save_g, float* save_o, float* save_c, void* stream) {
    if (!gi || !h0 || !c0 || !masks || !w_hh || !out || !c_state_out || T <= 0 || N <= 0 || H <= 0 || (H & 3))
        return IVLN_E_INVALID;
    if (save_i && (!save_f || !save_g || !save_o || !save_c)) return IVLN_E_INVALID;
    for (int t = 0; t < T; ++t) {
        const int64_t r0 = (int64_t)t * N;
        const float* h_in = t == 0 ? h0 : out + (r0 - N) * ldo;
        const int64_t ldh = t == 0 ? ld_h0 : ldo;
        // the cell state lives in c_state_out from step 0 on and is advanced in place
        const float* c_in = t == 0 ? c0 : c_state_out;
        const int64_t ldc = t == 0 ? ld_c0 : ld_cs;
        launch_step(nullptr, 0, 0, gi + r0 * 4 * H, (int64_t)4 * H, h_in, ldh, c_in, ldc, masks + r0, nullptr, w_hh, nullptr,
                    b_hh, out + r0 * ldo, ldo, t == T - 1 ? h_state_out : nullptr, ld_hs, c_state_out, ld_cs, N, H,
                    save_i ? save_i + r0 * H : nullptr, save_i ? save_f + r0 * H : nullptr,
                    save_i ? save_g + r0 * H : nullptr, save_i ? save_o + r0 * H : nullptr,
                    save_i ? save_c + r0 * H : nullptr, (hipStream_t)stream);
    }
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

}  // extern "C"
