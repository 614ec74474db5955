// Device-side pieces of the masked GRU / LSTM state encoders (habitat-lab RNNStateEncoder around nn.GRU / nn.LSTM, one
// layer), each written ONCE and used by the step / sequence / BPTT kernels of state_rnn.hip and by the fused rollout
// head of cma_step.hip.  All fp32.  Every formula keeps the association it always had: the callers are held to the same
// bytes, not to a tolerance ("State encoders: what is shared").
//
//   GRU  (gates r, z, n):     r = s(gi_r + gh_r)  z = s(gi_z + gh_z)  n = tanh(gi_n + r gh_n)  h_t = (1 - z) n + z h'
//   LSTM (gates i, f, g, o):  pre = gi + gh;  c_t = s(f) c' + s(i) tanh(g);  h_t = s(o) tanh(c_t)
//   gi = W_ih x + b_ih,  gh = W_hh h' + b_hh,  h' = h * mask, c' = c * mask (the mask is applied BEFORE the state is used)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// one sequential chain over a 16-byte piece
__device__ __forceinline__ float fma4(const float4 w, const float4 v, float a) {
    a = fmaf(w.x, v.x, a);
    a = fmaf(w.y, v.y, a);
    a = fmaf(w.z, v.z, a);
    return fmaf(w.w, v.w, a);
}
// two interleaved chains over a 16-byte piece (the BPTT matvecs)
__device__ __forceinline__ void fma4x2(const float4 w, const float4 v, float& a0, float& a1) {
    a0 = fmaf(w.x, v.x, a0);
    a1 = fmaf(w.y, v.y, a1);
    a0 = fmaf(w.z, v.z, a0);
    a1 = fmaf(w.w, v.w, a1);
}

// Write-through 4-byte store at agent scope (`global_store ... sc1`) for values that workgroups on other XCDs read next:
// neighbouring outputs share 128-byte lines, and a write-through store leaves no partially-updated copy of the line
// behind in the producing XCD's L2 (MI355X_MICROARCH.md, inter-workgroup visibility).
__device__ __forceinline__ void st_pub(float* p, float v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// LPR lanes share one batch row and split K; 256 / LPR rows are in flight per pass.  A (row, output) dot product then
// needs one log2(LPR)-step shuffle reduction and no LDS.
template <int LPR>
__device__ __forceinline__ float lpr_sum(float v) {
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the same for the input-side (only when `with_a`) and hidden-side partial sums of N gates at once, level by level: up to
// 2 N independent shuffles in flight per level
template <int LPR, int N>
__device__ __forceinline__ void lpr_sum_gates(float (&a)[N], bool with_a, float (&b)[N]) {
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) {
#pragma unroll
        for (int g = 0; g < N; ++g) {
            if (with_a) a[g] += __shfl_xor(a[g], o, 64);
            b[g] += __shfl_xor(b[g], o, 64);
        }
    }
}

// The NG gate rows of unit j (rows g * H + j of the (NG * H, K) matrix w) against one row x scaled by mk (the mask of an
// incoming state, 1 for an input): ONE pass over K, lane l of LPR owns every LPR-th piece, each piece of x loaded once
// for the NG rows, one sequential fmaf chain per gate.  VEC: 16-byte pieces (x, w 16-byte aligned, K a multiple of 4),
// else 4-byte pieces with the same lane-strided split.  The lanes' partial sums are returned: reduce with lpr_sum.
template <int NG, int LPR, bool VEC>
__device__ __forceinline__ void gate_dots(const float* __restrict__ w, int j, int H, int K, const float* __restrict__ x,
                                          float mk, int l, float (&a)[NG]) {
#pragma unroll
    for (int g = 0; g < NG; ++g) a[g] = 0.f;
    if constexpr (VEC) {
        for (int k = l * 4; k < K; k += LPR * 4) {
            float4 xv = *reinterpret_cast<const float4*>(x + k);
            xv.x *= mk, xv.y *= mk, xv.z *= mk, xv.w *= mk;
#pragma unroll
            for (int g = 0; g < NG; ++g) a[g] = fma4(*reinterpret_cast<const float4*>(w + ((int64_t)g * H + j) * K + k), xv, a[g]);
        }
    } else {
        for (int k = l; k < K; k += LPR) {
            const float xv = x[k] * mk;
#pragma unroll
            for (int g = 0; g < NG; ++g) a[g] = fmaf(w[((int64_t)g * H + j) * K + k], xv, a[g]);
        }
    }
}

// W[o] . x over 32 lanes of one row (lane l owns float4 l, l + 32, ...), two fmaf chains per lane; every lane returns the sum
__device__ __forceinline__ float skinny_dot32(const float* __restrict__ wr, const float* __restrict__ xr, int K, int l) {
    float a0 = 0.f, a1 = 0.f;
    for (int k = l * 4; k < K; k += 128)
        fma4x2(*reinterpret_cast<const float4*>(wr + k), *reinterpret_cast<const float4*>(xr + k), a0, a1);
    return lpr_sum<32>(a0 + a1);
}

// ---- forward cells: pre-activations (biases included) and the masked previous state element in, new state out ----
// sv: what BPTT needs of the step - GRU (r, z, n, gh_n), LSTM (i, f, g, o, c_t)
__device__ __forceinline__ float gru_cell_fwd(const float (&gi)[3], const float (&gh)[3], float hp, float (&sv)[5]) {
    const float rg = sigmoidf_(gi[0] + gh[0]);
    const float zg = sigmoidf_(gi[1] + gh[1]);
    const float ng = tanhf(gi[2] + rg * gh[2]);
    sv[0] = rg, sv[1] = zg, sv[2] = ng, sv[3] = gh[2];
    return (1.f - zg) * ng + zg * hp;
}
__device__ __forceinline__ float lstm_cell_fwd(const float (&gi)[4], const float (&gh)[4], float cp, float (&sv)[5]) {
    const float ig = sigmoidf_(gi[0] + gh[0]), fg = sigmoidf_(gi[1] + gh[1]), gg = tanhf(gi[2] + gh[2]),
                og = sigmoidf_(gi[3] + gh[3]);
    const float ct = fg * cp + ig * gg;
    sv[0] = ig, sv[1] = fg, sv[2] = gg, sv[3] = og, sv[4] = ct;
    return og * tanhf(ct);
}

// What a kernel needs to know of a cell: its gate count, which state element the formula carries (GRU: h, LSTM: c),
// how many values it saves for BPTT, and the formula.
struct GruCell {
    static constexpr int NG = 3, NSAVE = 4;
    static constexpr bool HAS_C = false;
    static __device__ __forceinline__ float fwd(const float (&gi)[3], const float (&gh)[3], float prev, float (&sv)[5]) {
        return gru_cell_fwd(gi, gh, prev, sv);
    }
};
struct LstmCell {
    static constexpr int NG = 4, NSAVE = 5;
    static constexpr bool HAS_C = true;   // sv[4] is the new cell state
    static __device__ __forceinline__ float fwd(const float (&gi)[4], const float (&gh)[4], float prev, float (&sv)[5]) {
        return lstm_cell_fwd(gi, gh, prev, sv);
    }
};

// ---- BPTT, element part of one step ----
// GRU: dh = the gradient arriving at h_t, hp = h_{t-1} * mask_t.
//   dn = dh (1 - z);  dz = dh (hp - n);  dn_pre = dn (1 - n^2);  dz_pre = dz z (1 - z);  dr_pre = dn_pre gh_n r (1 - r)
//   dgi = [dr_pre, dz_pre, dn_pre];  dgh = [dr_pre, dz_pre, dn_pre r] (the caller's product);  dhz = dh z (the direct path into h_{t-1})
struct GruBwd {
    float dr_pre, dz_pre, dn_pre, dhz;
};
__device__ __forceinline__ GruBwd gru_cell_bwd(float dh, float hp, float rg, float zg, float ng, float ghn) {
    const float dn = dh * (1.f - zg);
    const float dz = dh * (hp - ng);
    const float dn_pre = dn * (1.f - ng * ng);
    const float dz_pre = dz * zg * (1.f - zg);
    const float dr_pre = dn_pre * ghn * rg * (1.f - rg);
    return {dr_pre, dz_pre, dn_pre, dh * zg};
}
// LSTM: dh as above, dc_prev = what step t + 1 sent into c_t, cp = c_{t-1} * mask_t, c = c_t.
//   dc = dc_prev + dh o (1 - tanh(c)^2);  dgi = [dc g i(1-i), dc cp f(1-f), dc i (1-g^2), dh tanh(c) o(1-o)];  dcf = dc f
struct LstmBwd {
    float dgi[4], dcf;
};
__device__ __forceinline__ LstmBwd lstm_cell_bwd(float dh, float dc_prev, float cp, float c, float ig, float fg, float g_,
                                                 float og) {
    const float tc = tanhf(c);
    const float dc = dc_prev + dh * og * (1.f - tc * tc);
    return {{dc * g_ * ig * (1.f - ig), dc * cp * fg * (1.f - fg), dc * ig * (1.f - g_ * g_), dh * tc * og * (1.f - og)},
            dc * fg};
}
