// Instruction encoder over pre-computed text features (include/ivln_text_feat.h): MODEL.INSTRUCTION_ENCODER.sensor_uuid
// "rxr_instruction" - the reference reads a (B, L, E) float tensor and builds no embedding layer
// (models/encoders/instruction_encoder.py:34-45, 70-78).  Two kernels in front of the recurrences of instr_rnn.hip:
//   k_text_feat_front   row counts ("lengths") + the per-episode cache's compare-and-copy, a sequence spread over many
//                       workgroups, its partial results combined by one 64-bit integer atomic add per workgroup
//   k_text_feat_gates   gx = feat . W_ih^T + b_ih on the fp32 MFMA for the sequences the front kernel flagged
// All fp32; plain and 16-byte vector stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ivln_text_feat.h"

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP)

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// (a float is "zero" when it compares equal to 0.0f: +0 and -0; NaN and denormals are not)
__device__ __forceinline__ bool word_nonzero(uint32_t w) { return (w & 0x7fffffffu) != 0u; }

// Workgroup (b, c) of the grid takes rows [c * R, min(L, (c + 1) * R)) of sequence b, a wave per row.  A word of the cache
// is stored only where it differs (or the row was never valid): equal chunks of a dirty sequence need no copy.
// ws: one 64-bit word per sequence (row count, difference count, ticket) - zero on entry, zero again when the last
// workgroup of the sequence has read it.
template <bool VEC>
__global__ __launch_bounds__(256) void k_text_feat_front(const float* __restrict__ feat, int L, int E, int R, int S,
                                                         int* __restrict__ lengths, float* __restrict__ cache,
                                                         int* __restrict__ valid, int* __restrict__ dirty, int* __restrict__ ws) {
    const int b = blockIdx.x / S, c = blockIdx.x - b * S;
    const int t1 = min(L, (c + 1) * R);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool cached = cache != nullptr;
    const bool stale = cached && valid[b] == 0;  // (uniform; `valid[b]` is rewritten only behind every workgroup's ticket)
    int count = 0;
    bool diff = false;
    for (int t = c * R + wave; t < t1; t += 4) {
        const int64_t off = ((int64_t)b * L + t) * E;
        bool nz = false;
        if (VEC) {
            const uint4* src = reinterpret_cast<const uint4*>(feat + off);
            uint4* dst = cached ? reinterpret_cast<uint4*>(cache + off) : nullptr;
            const int E4 = E >> 2;
            for (int i0 = lane; i0 < E4; i0 += 256) {  // four 16-byte loads per operand in flight per lane
                uint4 v[4], o[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = i0 + 64 * u;
                    v[u] = make_uint4(0u, 0u, 0u, 0u);
                    if (i < E4) v[u] = src[i];
                    o[u] = v[u];
                    if (cached && i < E4) o[u] = dst[i];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = i0 + 64 * u;
                    nz |= word_nonzero(v[u].x | v[u].y | v[u].z | v[u].w);
                    const bool d = ((v[u].x ^ o[u].x) | (v[u].y ^ o[u].y) | (v[u].z ^ o[u].z) | (v[u].w ^ o[u].w)) != 0u;
                    if (cached && i < E4 && (d || stale)) dst[i] = v[u];
                    diff |= d;
                }
            }
        } else {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(feat + off);
            uint32_t* dst = cached ? reinterpret_cast<uint32_t*>(cache + off) : nullptr;
            for (int i = lane; i < E; i += 64) {
                const uint32_t v = src[i];
                nz |= word_nonzero(v);
                if (cached) {
                    const bool d = v != dst[i];
                    if (d || stale) dst[i] = v;
                    diff |= d;
                }
            }
        }
        if (__any(nz)) ++count;  // (the same in every lane of the wave)
    }
    diff = __any(diff);
    __shared__ int s_cnt[4], s_diff[4];
    if (lane == 0) s_cnt[wave] = count, s_diff[wave] = diff ? 1 : 0;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int cnt = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
    const int d = (s_diff[0] | s_diff[1] | s_diff[2] | s_diff[3]) | (stale ? 1 : 0);
    // ONE 64-bit integer add per workgroup: [row count : 32 | difference count : 16 | ticket : 16].  Adds commute, so the
    // totals do not depend on the order the workgroups arrive in, and the add that draws the last ticket returns them:
    // no fence, no second word to order against.  That workgroup re-arms the word for the next launch.
    unsigned long long* w = reinterpret_cast<unsigned long long*>(ws) + b;
    const unsigned long long mine = ((unsigned long long)cnt << 32) | ((unsigned long long)d << 16) | 1ull;
    const unsigned long long all = atomicAdd(w, mine) + mine;
    if ((int)(all & 0xffffull) != S) return;
    atomicExch(w, 0ull);
    const int total = (int)(all >> 32), any = (int)((all >> 16) & 0xffffull);
    if (!cached) {
        lengths[b] = total;
    } else {
        dirty[b] = any ? 1 : 0;
        if (any) lengths[b] = total, valid[b] = 1;
    }
}

// D[r][g] = sum_k feat[r][k] * w[g][k] + bias[g]: w is the MFMA's row operand (a lane then holds four consecutive g of one
// row r: one 16-byte store), feat the column operand.  64 x 64 tile, four waves of 32 x 32, K in LDS slices of 32.
constexpr int TF_BM = 64, TF_BN = 64, TF_BK = 32, TF_LD = TF_BK + 1;

template <bool VEC>
__device__ __forceinline__ void load8(const float* __restrict__ base, bool ok, int64_t off, int k, int E, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    if (!ok) return;
    if (VEC) {  // E % 4 == 0: a quad is inside the row or outside it
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (k + 4 * h < E) {
                const float4 q = *reinterpret_cast<const float4*>(base + off + k + 4 * h);
                v[4 * h] = q.x, v[4 * h + 1] = q.y, v[4 * h + 2] = q.z, v[4 * h + 3] = q.w;
            }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (k + j < E) v[j] = base[off + k + j];
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_text_feat_gates(const float* __restrict__ feat, int rows, int L, int E,
                                                         const float* __restrict__ w, const float* __restrict__ bias, int G,
                                                         const int* __restrict__ dirty, float* __restrict__ gx, int vec_out) {
    const int n0 = blockIdx.x * TF_BN, m0 = blockIdx.y * TF_BM;
    if (dirty) {  // (uniform, before the first barrier and the first load) every sequence of the tile's rows is clean
        const int last = min(rows, n0 + TF_BN) - 1;
        bool run = false;
        for (int i = n0 / L; i <= last / L; ++i)
            if (dirty[i]) { run = true; break; }
        if (!run) return;
    }
    __shared__ float As[TF_BM * TF_LD], Bs[TF_BN * TF_LD];
    const int tid = threadIdx.x, lr = tid >> 2, kc = (tid & 3) * 8;
    const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
    const int tm = wave & 1, tn = wave >> 1;
    const bool a_ok = m0 + lr < G, b_ok = n0 + lr < rows;
    const int64_t a_off = (int64_t)(m0 + lr) * E, b_off = (int64_t)(n0 + lr) * E;
    f32x16 acc;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    for (int k0 = 0; k0 < E; k0 += TF_BK) {
        float av[8], bv[8];
        load8<VEC>(w, a_ok, a_off, k0 + kc, E, av);
        load8<VEC>(feat, b_ok, b_off, k0 + kc, E, bv);
        __syncthreads();  // (the previous slice has been read)
#pragma unroll
        for (int j = 0; j < 8; ++j) As[lr * TF_LD + kc + j] = av[j], Bs[lr * TF_LD + kc + j] = bv[j];
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < TF_BK; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(tm * 32 + l31) * TF_LD + kk + half],
                                                       Bs[(tn * 32 + l31) * TF_LD + kk + half], acc, 0, 0, 0);
    }
    // lane (l31, half): row r = n0 + 32 tn + l31; registers 4q .. 4q+3 = gates m0 + 32 tm + 8q + 4 half + {0..3}
    const int r = n0 + tn * 32 + l31;
    if (r >= rows || (dirty && !dirty[r / L])) return;
    float* out = gx + (int64_t)r * G;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int m = m0 + tm * 32 + 8 * q + 4 * half;
        if (vec_out) {  // G % 4 == 0: the four gates are in or out together
            if (m >= G) continue;
            float4 v = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
            if (bias) v.x += bias[m], v.y += bias[m + 1], v.z += bias[m + 2], v.w += bias[m + 3];
            *reinterpret_cast<float4*>(out + m) = v;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (m + i < G) out[m + i] = acc[4 * q + i] + (bias ? bias[m + i] : 0.f);
        }
    }
}

}  // namespace

extern "C" int64_t ivln_text_feat_ws_words(int B) { return B > 0 ? 2 * (int64_t)B : 0; }

extern "C" int ivln_text_feat_front_f32(const float* feat, int B, int L, int E, int* lengths, float* cache_feat, int* valid,
                                        int* dirty, int* ws, void* stream) {
    if (!feat || !lengths || !ws || B <= 0 || L <= 0 || E <= 0) return IVLN_E_INVALID;
    const int given = (cache_feat != nullptr) + (valid != nullptr) + (dirty != nullptr);
    if (given != 0 && given != 3) return IVLN_E_INVALID;
    if ((int64_t)L * E >= (int64_t)1 << 31) return IVLN_E_INVALID;
    // rows per workgroup: about 4096 words (16 KB of features), a multiple of the four waves, and at most 32768
    // workgroups per sequence (the ticket's 16 bits)
    int64_t R = ((4096 / E + 3) / 4) * 4;
    if (R < 4) R = 4;
    if (R * 32768 < L) R = (((int64_t)L + 32767) / 32768 + 3) / 4 * 4;
    if (R > L) R = L;
    const int S = (int)((L + R - 1) / R);
    if ((int64_t)B * S >= (int64_t)1 << 31 || ((uintptr_t)ws & 7) != 0) return IVLN_E_INVALID;
    const bool vec = (E & 3) == 0 && (((uintptr_t)feat | (uintptr_t)cache_feat) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(k_text_feat_front<true>, dim3(B * S), dim3(256), 0, (hipStream_t)stream, feat, L, E, (int)R, S, lengths,
                           cache_feat, valid, dirty, ws);
    else
        hipLaunchKernelGGL(k_text_feat_front<false>, dim3(B * S), dim3(256), 0, (hipStream_t)stream, feat, L, E, (int)R, S, lengths,
                           cache_feat, valid, dirty, ws);
    return LAUNCH_OK();
}

extern "C" int ivln_text_feat_gates_f32(const float* feat, int B, int L, int E, const float* w, const float* bias, int G,
                                        const int* dirty, float* gx, void* stream) {
    if (!feat || !w || !gx || B <= 0 || L <= 0 || E <= 0 || G <= 0) return IVLN_E_INVALID;
    if ((int64_t)B * L >= (int64_t)1 << 31) return IVLN_E_INVALID;
    const int rows = B * L;
    const int64_t gy = (G + TF_BM - 1) / TF_BM;
    if (gy > 65535) return IVLN_E_INVALID;
    const bool vec = (E & 3) == 0 && (((uintptr_t)feat | (uintptr_t)w) & 15) == 0;
    const int vec_out = (G & 3) == 0 && ((uintptr_t)gx & 15) == 0;
    const dim3 grid((rows + TF_BN - 1) / TF_BN, (unsigned)gy);
    if (vec)
        hipLaunchKernelGGL(k_text_feat_gates<true>, grid, dim3(256), 0, (hipStream_t)stream, feat, rows, L, E, w, bias, G,
                           dirty, gx, vec_out);
    else
        hipLaunchKernelGGL(k_text_feat_gates<false>, grid, dim3(256), 0, (hipStream_t)stream, feat, rows, L, E, w, bias, G,
                           dirty, gx, vec_out);
    return LAUNCH_OK();
}
