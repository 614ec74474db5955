// GRU instruction encoder for gfx950 (MODEL.INSTRUCTION_ENCODER.rnn_type GRU, bidirectional or not): the length-masked
// recurrence over packed sequences and its BPTT.  The reference builds nn.GRU or nn.LSTM from the config
// (ivlnce_baselines/models/encoders/instruction_encoder.py:27-32), runs it over pack_padded_sequence and returns
// pad_packed_sequence(...).permute(0, 2, 1) (:84-94).  The LSTM cell of the same encoder is k_lstm_bidir (nn_ops.hip) /
// k_lstm_bidir_bwd (train_ops.hip); this file is its GRU twin, with the same work split.  Gate order is torch's: r, z, n.
//
//   r = s(gi_r + W_hr h + b_hr)   z = s(gi_z + W_hz h + b_hz)   n = tanh(gi_n + r * (W_hn h + b_hn))
//   h' = (1 - z) * n + z * h
//
// gi = W_ih x + b_ih of every position comes from the GEMM (update pass) or from the folded token table (rollout,
// ivln_embed_gates_cached_f32 with G = 3H).  All fp32.  Plain launches: nothing persistent, no spinning, no tickets.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/ivln_hip.h"

namespace {

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP)

// DPP quad permutation of a float (ctrl = p0 | p1<<2 | p2<<4 | p3<<6: lane i of each quad reads lane p_i)
template <int CTRL>
__device__ __forceinline__ float quad_perm(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}

// Barrier that orders LDS traffic only (see nn_ops.hip: __syncthreads() would also wait for the per-step global stores).
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

typedef float v2f __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------
// Forward.  grid nd * B: one workgroup per (sequence, direction), item = dir * B + b; 4H = 512 threads.  The quad of hidden
// unit j keeps the split of k_lstm_bidir: lane q multiplies ITS quarter of h with the unit's THREE gate rows (3 x H/4 = 96
// weights in registers, statically indexed), the quad adds the partial sums by DPP so every lane holds all three
// W_h* h products.  Lanes 0 and 1 activate r and z (one fast exp each, in the same instruction), the quad exchanges them
// by DPP, then every lane computes n and the new h redundantly (h lives in a register; LDS holds it only for the matvec).
// Lane q < 3 fetches the gate input of row q (prefetched four steps ahead as in k_lstm_bidir); lane 3 mirrors lane 2's
// addresses so that no lane branches around a load.  One LDS-only barrier per step.
// out (B, nd*H, L), exactly zero for t >= min(lengths[b], L).  save (optional) (B, nd, L, 4, H): r, z, n, W_hn h + b_hn.
// ------------------------------------------------------------------------------------------
template <int H>
__global__ __launch_bounds__(4 * H) void k_gru_dirs(const float* __restrict__ gx_f, const float* __restrict__ gx_r,
                                                    const float* __restrict__ whh_f, const float* __restrict__ whh_r,
                                                    const float* __restrict__ bhh_f, const float* __restrict__ bhh_r,
                                                    const int* __restrict__ lengths, int L, int nd,
                                                    float* __restrict__ out, float* __restrict__ save, int B,
                                                    const int* __restrict__ dirty) {
    constexpr int G = 3 * H;
    const int item = blockIdx.x;
    const int b = item % B, dir = item / B, tid = threadIdx.x;
    if (dirty && !dirty[b]) return;  // (per-episode cache, k_embed_gates: this row's output of last step stands)
    constexpr int HQ = H / 4, HQP = HQ + 4;  // +4 words per quarter: the 4 quarters hit different banks
    __shared__ __attribute__((aligned(16))) float hs[2][4 * HQP];  // double-buffered: one barrier per step
    const int q = tid & 3, j = tid >> 2;
    const int g = (q < 3 ? q : 2) * H + j;  // the gate row whose input and bias this lane fetches (order r, z, n)
    const float* gx = (dir == 0 ? gx_f : gx_r) + (int64_t)b * L * G;
    const float* whh = (dir == 0 ? whh_f : whh_r);
    const float bias = (dir == 0 ? bhh_f : bhh_r)[g];
    const float bhn = quad_perm<0xAA>(bias);
    v2f w[3][HQ / 2];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < HQ / 2; ++k) {
            const float* wp = whh + (int64_t)(r * H + j) * H + q * HQ + 2 * k;
            w[r][k] = v2f{wp[0], wp[1]};
        }
    const int hslot = (j / HQ) * HQP + j % HQ;
    if (q == 0) hs[0][hslot] = 0.f;
    float h = 0.f;
    lds_barrier();
    int len = lengths[b];
    if (len > L) len = L;
    if (len < 0) len = 0;
    float* orow = out + ((int64_t)b * nd * H + dir * H + j) * L;
    float* srow = save ? save + (((int64_t)b * nd + dir) * L * 4 + q) * H + j : nullptr;
    auto gx_at = [&](int s) -> float {
        return s < len ? gx[(int64_t)(dir == 0 ? s : len - 1 - s) * G + g] : 0.f;
    };
    auto step = [&](int s, float gxv) {
        const int t = dir == 0 ? s : len - 1 - s;
        const float* hcur = hs[s & 1];
        v2f p[3] = {v2f{0.f, 0.f}, v2f{0.f, 0.f}, v2f{0.f, 0.f}};
#pragma unroll
        for (int k = 0; k < HQ; k += 4) {
            const float4 hv = *reinterpret_cast<const float4*>(&hcur[q * HQP + k]);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                p[r] = __builtin_elementwise_fma(w[r][k / 2], v2f{hv.x, hv.y}, p[r]);
                p[r] = __builtin_elementwise_fma(w[r][k / 2 + 1], v2f{hv.z, hv.w}, p[r]);
            }
        }
        float ps[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            float v = p[r].x + p[r].y;
            v += quad_perm<0xB1>(v);  // lanes 1,0,3,2
            v += quad_perm<0x4E>(v);  // lanes 2,3,0,1
            ps[r] = v;
        }
        const float gin = quad_perm<0xAA>(gxv);
        const float hn = ps[2] + bhn;
        // lanes 0 / 1: r / z (lanes 2, 3 compute a value nobody reads);  sigmoid / tanh through one fast exp each
        const float acc = gxv + bias + (q == 0 ? ps[0] : ps[1]);
        const float a = __builtin_amdgcn_rcpf(1.f + __expf(-acc));
        const float rg = quad_perm<0x00>(a), zg = quad_perm<0x55>(a);
        const float ng = 2.f * __builtin_amdgcn_rcpf(1.f + __expf(-2.f * (gin + rg * hn))) - 1.f;
        h = (1.f - zg) * ng + zg * h;
        if (srow) srow[(int64_t)t * 4 * H] = q == 0 ? rg : (q == 1 ? zg : (q == 2 ? ng : hn));
        if (q == 0) {
            hs[(s + 1) & 1][hslot] = h;
            orow[t] = h;
        }
        lds_barrier();
    };
    float g0 = gx_at(0), g1 = gx_at(1), g2 = gx_at(2), g3 = gx_at(3);
    for (int s = 0; s < len; s += 4) {
        step(s, g0);
        g0 = gx_at(s + 4);
        if (s + 1 >= len) break;
        step(s + 1, g1);
        g1 = gx_at(s + 5);
        if (s + 2 >= len) break;
        step(s + 2, g2);
        g2 = gx_at(s + 6);
        if (s + 3 >= len) break;
        step(s + 3, g3);
        g3 = gx_at(s + 7);
    }
    if (q == 0)
        for (int t = len; t < L; ++t) orow[t] = 0.f;
}

// ------------------------------------------------------------------------------------------
// BPTT of the above.  grid (B, nd); 512 threads.  Work split of k_lstm_bidir_bwd with 3H gate rows: threads 0..H-1 own a
// hidden unit each for the element part; for dh_prev[k] = sum_g W_hh[g][k] dgh[g] thread (ko = tid / 16, ig = tid % 16)
// owns the outputs k = 4ko..4ko+3 and the 24 gate rows g = 24ig..24ig+23 (96 weights in registers), reads only its 24 gate
// gradients from LDS and the 16 lanes of an output add up by shuffles.  The direct path dh * z stays in the unit's
// register.  Two LDS-only barriers per timestep; the element part's inputs are fetched one timestep ahead.
//   dn = dh (1 - z);  dz = dh (h_prev - n);  a_n = dn (1 - n^2);  a_z = dz z (1 - z);  a_r = a_n ghn r (1 - r)
//   dgi = [a_r, a_z, a_n];  dgh = [a_r, a_z, a_n r];  dh_prev = dh z + W_hh^T dgh
// dgi / dgh (B*L, 3H) and hprev (B*L, H) per direction, exactly zero for t >= len; dout there is never read.
// ------------------------------------------------------------------------------------------
template <int H>
__global__ __launch_bounds__(4 * H) void k_gru_dirs_bwd(const float* __restrict__ dout, const float* __restrict__ out,
                                                        const float* __restrict__ save, const float* __restrict__ whh_f,
                                                        const float* __restrict__ whh_r, const int* __restrict__ lengths,
                                                        int L, int nd, float* __restrict__ dgi_f, float* __restrict__ dgi_r,
                                                        float* __restrict__ dgh_f, float* __restrict__ dgh_r,
                                                        float* __restrict__ hprev_f, float* __restrict__ hprev_r) {
    constexpr int G = 3 * H;
    constexpr int RG = 24, GS = RG + 4;  // rows per lane group; LDS stride of a group (+4 words: groups spread over the banks)
    static_assert(H == 128 && G == 16 * RG, "mapping below assumes 512 threads and 384 gate rows");
    __shared__ __attribute__((aligned(16))) float dg[16 * GS];
    __shared__ float dhc[H];
    const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
    const int ig = tid & 15, ko = tid >> 4;
    const float* whh = dir == 0 ? whh_f : whh_r;
    float* dgi = (dir == 0 ? dgi_f : dgi_r) + (int64_t)b * L * G;
    float* dgh = (dir == 0 ? dgh_f : dgh_r) + (int64_t)b * L * G;
    float* hprev = (dir == 0 ? hprev_f : hprev_r) + (int64_t)b * L * H;
    float w[4][RG];
#pragma unroll
    for (int g = 0; g < RG; ++g) {
        const float4 v = *reinterpret_cast<const float4*>(whh + (int64_t)(ig * RG + g) * H + ko * 4);
        w[0][g] = v.x, w[1][g] = v.y, w[2][g] = v.z, w[3][g] = v.w;
    }
    if (tid < H) dhc[tid] = 0.f;
    int len = lengths[b];
    if (len > L) len = L;
    if (len < 0) len = 0;
    {
        const int k = tid % H, pq = tid / H;
        for (int t = len + pq; t < L; t += 4) {  // padded positions carry no gradient
#pragma unroll
            for (int g = k; g < G; g += H) dgi[(int64_t)t * G + g] = 0.f, dgh[(int64_t)t * G + g] = 0.f;
            hprev[(int64_t)t * H + k] = 0.f;
        }
    }
    lds_barrier();
    const float* sv = save + ((int64_t)b * nd + dir) * L * 4 * H;
    const int j = tid;  // element part: threads 0..H-1 own hidden unit j
    const int64_t orow = ((int64_t)b * nd * H + dir * H + (j < H ? j : 0)) * L;
    float dhz = 0.f;  // dh * z carried to the previous timestep (register: only thread j touches it)
    float n_r = 0.f, n_z = 0.f, n_n = 0.f, n_gh = 0.f, n_hp = 0.f, n_do = 0.f;
    auto fetch = [&](int s) {
        if (j < H && s >= 0) {
            const int t = dir == 0 ? s : len - 1 - s, tp = dir == 0 ? t - 1 : t + 1;
            const float* p = sv + (int64_t)t * 4 * H + j;
            n_r = p[0], n_z = p[H], n_n = p[2 * H], n_gh = p[3 * H];
            n_hp = s > 0 ? out[orow + tp] : 0.f;
            n_do = dout[orow + t];
        }
    };
    fetch(len - 1);
    for (int s = len - 1; s >= 0; --s) {
        const int t = dir == 0 ? s : len - 1 - s;  // time index of processing step s
        const float rg = n_r, zg = n_z, ng = n_n, gh = n_gh, hp = n_hp, dov = n_do;
        fetch(s - 1);  // next timestep's inputs, in flight under this one
        if (j < H) {
            const float dh = dov + dhc[j] + dhz;
            const float a_n = dh * (1.f - zg) * (1.f - ng * ng);
            const float a_z = dh * (hp - ng) * zg * (1.f - zg);
            const float a_r = a_n * gh * rg * (1.f - rg);
            const float a_hn = a_n * rg;
            dhz = dh * zg;
            // gate row q*H + j lives in group (q*H + j) / RG, slot (q*H + j) % RG
            dg[((0 * H + j) / RG) * GS + (0 * H + j) % RG] = a_r;
            dg[((1 * H + j) / RG) * GS + (1 * H + j) % RG] = a_z;
            dg[((2 * H + j) / RG) * GS + (2 * H + j) % RG] = a_hn;
            dgi[(int64_t)t * G + j] = a_r;
            dgi[(int64_t)t * G + H + j] = a_z;
            dgi[(int64_t)t * G + 2 * H + j] = a_n;
            dgh[(int64_t)t * G + j] = a_r;
            dgh[(int64_t)t * G + H + j] = a_z;
            dgh[(int64_t)t * G + 2 * H + j] = a_hn;
            hprev[(int64_t)t * H + j] = hp;
        }
        lds_barrier();
        float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
#pragma unroll
        for (int g = 0; g < RG; g += 4) {
            const float4 v = *reinterpret_cast<const float4*>(&dg[ig * GS + g]);
            p0 = fmaf(w[0][g], v.x, p0), p1 = fmaf(w[1][g], v.x, p1), p2 = fmaf(w[2][g], v.x, p2), p3 = fmaf(w[3][g], v.x, p3);
            p0 = fmaf(w[0][g + 1], v.y, p0), p1 = fmaf(w[1][g + 1], v.y, p1), p2 = fmaf(w[2][g + 1], v.y, p2),
            p3 = fmaf(w[3][g + 1], v.y, p3);
            p0 = fmaf(w[0][g + 2], v.z, p0), p1 = fmaf(w[1][g + 2], v.z, p1), p2 = fmaf(w[2][g + 2], v.z, p2),
            p3 = fmaf(w[3][g + 2], v.z, p3);
            p0 = fmaf(w[0][g + 3], v.w, p0), p1 = fmaf(w[1][g + 3], v.w, p1), p2 = fmaf(w[2][g + 3], v.w, p2),
            p3 = fmaf(w[3][g + 3], v.w, p3);
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {  // the 16 lanes of an output group are consecutive
            p0 += __shfl_xor(p0, off, 64);
            p1 += __shfl_xor(p1, off, 64);
            p2 += __shfl_xor(p2, off, 64);
            p3 += __shfl_xor(p3, off, 64);
        }
        if (ig == 0) {  // dhc of this step was consumed before the first barrier: safe to overwrite
            dhc[ko * 4] = p0;
            dhc[ko * 4 + 1] = p1;
            dhc[ko * 4 + 2] = p2;
            dhc[ko * 4 + 3] = p3;
        }
        lds_barrier();
    }
}

}  // namespace

extern "C" {

int ivln_gru_dirs_fwd_f32(const float* gx_f, const float* gx_r, const float* whh_f, const float* whh_r, const float* bhh_f,
                          const float* bhh_r, const int* lengths, int B, int L, int H, int ndir, float* out, float* save,
                          const int* dirty, void* stream) {
    if (H != 128) return IVLN_E_UNSUPPORTED;
    if (B <= 0 || L <= 0 || (ndir != 1 && ndir != 2)) return IVLN_E_INVALID;
    if (!gx_f || !whh_f || !bhh_f || !lengths || !out || (ndir == 2 && (!gx_r || !whh_r || !bhh_r))) return IVLN_E_INVALID;
    if (ndir == 1) gx_r = gx_f, whh_r = whh_f, bhh_r = bhh_f;  // (never read: every item is a forward one)
    hipLaunchKernelGGL((k_gru_dirs<128>), dim3(ndir * B), dim3(512), 0, (hipStream_t)stream, gx_f, gx_r, whh_f, whh_r, bhh_f,
                       bhh_r, lengths, L, ndir, out, save, B, dirty);
    return LAUNCH_OK();
}

int ivln_gru_dirs_bwd_f32(const float* dout, const float* out, const float* save, const float* whh_f, const float* whh_r,
                          const int* lengths, int B, int L, int H, int ndir, float* dgi_f, float* dgi_r, float* dgh_f,
                          float* dgh_r, float* hprev_f, float* hprev_r, void* stream) {
    if (H != 128) return IVLN_E_UNSUPPORTED;
    if (B <= 0 || L <= 0 || (ndir != 1 && ndir != 2)) return IVLN_E_INVALID;
    if (!dout || !out || !save || !whh_f || !lengths || !dgi_f || !dgh_f || !hprev_f) return IVLN_E_INVALID;
    if (ndir == 2 && (!whh_r || !dgi_r || !dgh_r || !hprev_r)) return IVLN_E_INVALID;
    if (ndir == 1) whh_r = whh_f, dgi_r = dgi_f, dgh_r = dgh_f, hprev_r = hprev_f;  // (never used: grid (B, 1))
    hipLaunchKernelGGL((k_gru_dirs_bwd<128>), dim3(B, ndir), dim3(512), 0, (hipStream_t)stream, dout, out, save, whh_f, whh_r,
                       lengths, L, ndir, dgi_f, dgi_r, dgh_f, dgh_r, hprev_f, hprev_r);
    return LAUNCH_OK();
}

}  // extern "C"
