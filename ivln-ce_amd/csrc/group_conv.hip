// Depth-encoder backbones beyond ResNet-50 (include/ivln_depth_backbones.h): the grouped 3x3 convolution of the ResNeXt
// bottlenecks and the squeeze-and-excite tail of the SE bottlenecks (habitat-lab v0.1.7 rl/ddppo/policy/resnet.py).
//   k_gconv3x3_mfma   channels per group a multiple of 16: v_mfma_f32_16x16x4_f32, a wave = 16 output channels x 16 pixels
//   k_gconv3x3_valu   every other count from 1 to 64: a thread = one pixel x up to 4 output channels
//   k_se_gate         gate = sigmoid(W2 relu(W1 mean_hw(GroupNorm(x)) + b1) + b2), a workgroup per image
//   k_se_apply        relu(gate * GroupNorm(x) + identity), a workgroup per (image, group)
// All fp32, fixed summation orders, plain stores only, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/ivln_depth_backbones.h"

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP)

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------------
// Grouped 3x3 convolution.  Both kernels work on the same tile: 64 output pixels = TH "virtual rows" x TW columns, TW =
// 4 | 8 | 16 by the plane's width, where virtual row vr = n * Ho + oy runs over the whole batch (a 4 x 4 plane fills a
// tile with four images instead of leaving three quarters of it empty).  Rows of a tile may belong to different images,
// so every output row stages its own three input rows: in[ic][r][ky][TWin], TWin = (TW - 1) * stride + 3, zero where the
// input is padding, the row is past the batch or the channel past the chunk.  16 input channels are staged at a time.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int GC_THREADS = 256, GC_PIX = 64, GC_IC = 16, GC_OC = 16;
constexpr int GC_IN_STRIDE_MAX = 464;  // largest per-channel stride: 16 rows x 3 x 9 (TW 4, stride 2) = 432, padded

struct GcArgs {
    const float* x;
    const float* w;
    float* y;
    int N, C, H, W, Ho, Wo, cpg, stride;
    int64_t x_img_stride;
    int tw_shift;   // TW = 1 << tw_shift, TH = 64 >> tw_shift
    int tiles_x;    // column tiles of a row of tiles
    int in_stride;  // floats between staged channels (== 16 mod 32: the four channels of an MFMA k-step on other banks)
    int multi;      // VALU form: 16 % cpg == 0, a workgroup covers the 16 / cpg groups of 16 consecutive channels
    int cpg_shift;  // log2(cpg) when multi
};

__device__ __forceinline__ void gc_stage_input(const GcArgs& a, float* __restrict__ in, int cbase, int nch, int vr0, int ox0) {
    const int TW = 1 << a.tw_shift, TH = GC_PIX >> a.tw_shift;
    const int twin = (TW - 1) * a.stride + 3;
    const int per = TH * 3 * twin;
    const int R = a.N * a.Ho;
    for (int idx = threadIdx.x; idx < GC_IC * per; idx += GC_THREADS) {
        const int ic = idx / per, rem = idx - ic * per;
        const int r = rem / (3 * twin), rem2 = rem - r * 3 * twin;
        const int ky = rem2 / twin, xl = rem2 - ky * twin;
        const int vr = vr0 + r;
        float v = 0.f;
        if (ic < nch && vr < R) {
            const int n = vr / a.Ho, oy = vr - n * a.Ho;
            const int iy = oy * a.stride - 1 + ky, ix = ox0 * a.stride - 1 + xl;
            if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                v = a.x[(int64_t)n * a.x_img_stride + ((int64_t)(cbase + ic) * a.H + iy) * a.W + ix];
        }
        in[ic * a.in_stride + rem] = v;
    }
}

__global__ __launch_bounds__(GC_THREADS) void k_gconv3x3_mfma(GcArgs a) {
    __shared__ float in[GC_IC * GC_IN_STRIDE_MAX];
    __shared__ float wl[9 * GC_IC * GC_OC];  // [tap][ic][oc]: the 64 lanes of an A fragment read 64 consecutive floats
    const int TW = 1 << a.tw_shift;
    const int twin = (TW - 1) * a.stride + 3;
    const int tile_r = blockIdx.x / a.tiles_x, tile_c = blockIdx.x - tile_r * a.tiles_x;
    const int vr0 = tile_r * (GC_PIX >> a.tw_shift), ox0 = tile_c * TW;
    const int oc0 = blockIdx.y * GC_OC;
    const int cin0 = (oc0 / a.cpg) * a.cpg;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, kq = lane >> 4;
    const int p = wave * 16 + col;
    const int r = p >> a.tw_shift, tx = p & (TW - 1);
    const int b_base = kq * a.in_stride + r * 3 * twin + tx * a.stride;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int ch = 0; ch < a.cpg / GC_IC; ++ch) {
        __syncthreads();  // (the previous chunk's fragments have been read)
        gc_stage_input(a, in, cin0 + ch * GC_IC, GC_IC, vr0, ox0);
        for (int idx = threadIdx.x; idx < GC_OC * GC_IC * 9; idx += GC_THREADS) {
            const int oc = idx / (GC_IC * 9), rem = idx - oc * (GC_IC * 9);
            const int ic = rem / 9, tap = rem - ic * 9;
            wl[(tap * GC_IC + ic) * GC_OC + oc] = a.w[((int64_t)(oc0 + oc) * a.cpg + ch * GC_IC + ic) * 9 + tap];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < GC_IC / 4; ++q) {
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int tap = ky * 3 + kx;
                    const float av = wl[(tap * GC_IC + 4 * q + kq) * GC_OC + col];
                    const float bv = in[4 * q * a.in_stride + b_base + ky * twin + kx];
                    // two accumulators: a dependent v_mfma_f32_16x16x4_f32 waits 40 cycles, an independent one issues after 32
                    if ((q * 9 + tap) & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc1, 0, 0, 0);
                    else acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc0, 0, 0, 0);
                }
            }
        }
    }
    const int vr = vr0 + r, ox = ox0 + tx;
    if (vr < a.N * a.Ho && ox < a.Wo) {
        const int n = vr / a.Ho, oy = vr - n * a.Ho;
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // C/D layout: column = lane & 15 (pixel), row = 4 * (lane >> 4) + i (output channel)
            const int oc = oc0 + kq * 4 + i;
            a.y[(((int64_t)n * a.C + oc) * a.Ho + oy) * a.Wo + ox] = acc0[i] + acc1[i];
        }
    }
}

__global__ __launch_bounds__(GC_THREADS) void k_gconv3x3_valu(GcArgs a) {
    __shared__ float in[GC_IC * GC_IN_STRIDE_MAX];
    __shared__ float wl[GC_OC * GC_IC * 9];  // [oc][ic][tap]: a wave reads one address at a time (broadcast)
    const int TW = 1 << a.tw_shift;
    const int twin = (TW - 1) * a.stride + 3;
    const int tile_r = blockIdx.x / a.tiles_x, tile_c = blockIdx.x - tile_r * a.tiles_x;
    const int vr0 = tile_r * (GC_PIX >> a.tw_shift), ox0 = tile_c * TW;
    int oc0, n_oc, cin0, chunks;
    if (a.multi) {  // 16 consecutive channels = whole groups: the input channels they read are the same 16
        oc0 = blockIdx.y * GC_OC;
        n_oc = min(GC_OC, a.C - oc0);
        cin0 = oc0;
        chunks = 1;
    } else {
        const int bpg = (a.cpg + GC_OC - 1) / GC_OC;
        const int g = blockIdx.y / bpg, ob = blockIdx.y - g * bpg;
        oc0 = g * a.cpg + ob * GC_OC;
        n_oc = min(GC_OC, a.cpg - ob * GC_OC);
        cin0 = g * a.cpg;
        chunks = (a.cpg + GC_IC - 1) / GC_IC;
    }
    const int p = threadIdx.x & 63, sub = threadIdx.x >> 6;  // (sub is uniform over a wave)
    const int r = p >> a.tw_shift, tx = p & (TW - 1);
    const int b_base = r * 3 * twin + tx * a.stride;
    const int shift = a.multi ? a.cpg_shift : 4;  // staged channel c belongs to local group c >> shift (always 0 when not multi)
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ch = 0; ch < chunks; ++ch) {
        const int nch = a.multi ? n_oc : min(GC_IC, a.cpg - ch * GC_IC);  // staged input channels
        const int icn = a.multi ? a.cpg : nch;                             // input channels of a weight row in this chunk
        __syncthreads();
        gc_stage_input(a, in, cin0 + ch * GC_IC, nch, vr0, ox0);
        for (int idx = threadIdx.x; idx < n_oc * icn * 9; idx += GC_THREADS) {
            const int oc = idx / (icn * 9), rem = idx - oc * (icn * 9);
            const int ic = rem / 9, tap = rem - ic * 9;
            wl[(oc * GC_IC + ic) * 9 + tap] = a.w[((int64_t)(oc0 + oc) * a.cpg + ch * GC_IC + ic) * 9 + tap];
        }
        __syncthreads();
        for (int c = 0; c < nch; ++c) {
            float v[9];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) v[ky * 3 + kx] = in[c * a.in_stride + b_base + ky * twin + kx];
            const int cg = c >> shift, icl = c - (cg << shift);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ocl = sub + 4 * j;
                if (ocl < n_oc && (a.multi ? ocl >> shift : 0) == cg) {
                    const float* wr = &wl[(ocl * GC_IC + icl) * 9];
#pragma unroll
                    for (int t = 0; t < 9; ++t) acc[j] = fmaf(v[t], wr[t], acc[j]);
                }
            }
        }
    }
    const int vr = vr0 + r, ox = ox0 + tx;
    if (vr < a.N * a.Ho && ox < a.Wo) {
        const int n = vr / a.Ho, oy = vr - n * a.Ho;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ocl = sub + 4 * j;
            if (ocl < n_oc) a.y[(((int64_t)n * a.C + oc0 + ocl) * a.Ho + oy) * a.Wo + ox] = acc[j];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Squeeze-and-excite
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {  // butterfly: every lane ends with the same sum, same order every run
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sum over a workgroup of `nw` waves; every thread returns the same value.  `red` is free again on return.
__device__ __forceinline__ float block_sum(float v, float* red, int nw) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < nw; ++i) s += red[i];
    __syncthreads();
    return s;
}

// element (c, p) of an image: the sum of its split-K slabs (one slab: the tensor itself)
__device__ __forceinline__ float se_load(const float* __restrict__ xp, int c, int p, int64_t chan_stride, int splits,
                                         int64_t slab_stride) {
    const float* q = xp + (int64_t)c * chan_stride + p;
    float v = *q;
    for (int z = 1; z < splits; ++z) v += q[(int64_t)z * slab_stride];
    return v;
}

// four consecutive pixels of channel c from pixel p on (p % 4 == 0): the sum of the slabs, four independent loads in flight
__device__ __forceinline__ float4 se_load4(const float* __restrict__ xp, int c, int p, int64_t chan_stride, int splits,
                                           int64_t slab_stride) {
    const float* q = xp + (int64_t)c * chan_stride + p;
    float4 v = *reinterpret_cast<const float4*>(q);
    int z = 1;
    for (; z + 3 < splits; z += 4) {
        const float4 w0 = *reinterpret_cast<const float4*>(q + (int64_t)z * slab_stride);
        const float4 w1 = *reinterpret_cast<const float4*>(q + (int64_t)(z + 1) * slab_stride);
        const float4 w2 = *reinterpret_cast<const float4*>(q + (int64_t)(z + 2) * slab_stride);
        const float4 w3 = *reinterpret_cast<const float4*>(q + (int64_t)(z + 3) * slab_stride);
        v.x += (w0.x + w1.x) + (w2.x + w3.x);
        v.y += (w0.y + w1.y) + (w2.y + w3.y);
        v.z += (w0.z + w1.z) + (w2.z + w3.z);
        v.w += (w0.w + w1.w) + (w2.w + w3.w);
    }
    for (; z < splits; ++z) {
        const float4 w = *reinterpret_cast<const float4*>(q + (int64_t)z * slab_stride);
        v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
    }
    return v;
}

constexpr int SE_GATE_THREADS = 1024, SE_MAX_C = 2048, SE_MAX_CR = 128;

// Statistics: per channel its sum and M2_c = sum (v - mean_c)^2, then per group (Chan's combination, every term >= 0)
//   mean_g = sum_c sum_c / n,   var_g = sum_c [M2_c + HW (mean_c - mean_g)^2] / n.
// `lpc_shift` >= 0 (the launcher's: HW % 4 == 0, HW <= 1024, 16-byte aligned pointer and strides): a channel is read ONCE, as
// float4s by 1 << lpc_shift lanes that keep up to four of them in registers - a wave covers 64 >> lpc_shift channels per
// round with every load in flight at once (one workgroup has to pull the whole image through one CU: what it costs is
// round trips).  -1: 4-byte loads, two reads of the channel.
__global__ __launch_bounds__(SE_GATE_THREADS) void k_se_gate(
    const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta, int C, int HW, int groups,
    float eps, int64_t x_img_stride, int64_t x_chan_stride, int splits, int64_t slab_stride, const float* __restrict__ w1,
    const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2, int Cr,
    float* __restrict__ gate, int lpc_shift) {
    __shared__ float chs[SE_MAX_C];  // per-channel sum
    __shared__ float chq[SE_MAX_C];  // per-channel M2; then mean_hw(z)
    __shared__ float gm[SE_MAX_C];   // group mean
    __shared__ float gr[SE_MAX_C];   // group rstd
    __shared__ float hid[SE_MAX_CR];
    const int img = blockIdx.x;
    const int cpg = C / groups;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int NW = SE_GATE_THREADS / 64;
    const float* xp = x + (int64_t)img * x_img_stride;
    const float inv_n = 1.f / (float)((int64_t)cpg * HW), inv_hw = 1.f / (float)HW;
    if (lpc_shift >= 0) {
        const int lpc = 1 << lpc_shift, cpw = 64 >> lpc_shift, q4 = HW >> 2;
        const int li = lane & (lpc - 1), sub = lane >> lpc_shift;
        for (int c0 = wave * cpw; c0 < C; c0 += NW * cpw) {  // (uniform over the wave: the shuffles below see all 64 lanes)
            const int c = c0 + sub;
            float4 v[4];
            bool ok[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                ok[k] = c < C && li + k * lpc < q4;
                v[k] = ok[k] ? se_load4(xp, c, (li + k * lpc) * 4, x_chan_stride, splits, slab_stride) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += (v[k].x + v[k].y) + (v[k].z + v[k].w);
            for (int o = lpc >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
            const float m = s * inv_hw;
            float q = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ok[k]) {
                    const float d0 = v[k].x - m, d1 = v[k].y - m, d2 = v[k].z - m, d3 = v[k].w - m;
                    q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
                }
            for (int o = lpc >> 1; o > 0; o >>= 1) q += __shfl_xor(q, o);
            if (li == 0 && c < C) chs[c] = s, chq[c] = q;
        }
    } else {
        for (int c = wave; c < C; c += NW) {
            float s = 0.f;
            for (int p = lane; p < HW; p += 64) s += se_load(xp, c, p, x_chan_stride, splits, slab_stride);
            s = wave_sum(s);
            const float m = s * inv_hw;
            float q = 0.f;
            for (int p = lane; p < HW; p += 64) {
                const float d = se_load(xp, c, p, x_chan_stride, splits, slab_stride) - m;
                q = fmaf(d, d, q);
            }
            q = wave_sum(q);
            if (lane == 0) chs[c] = s, chq[c] = q;
        }
    }
    __syncthreads();
    for (int g = threadIdx.x; g < groups; g += SE_GATE_THREADS) {
        float s = 0.f;
        for (int k = 0; k < cpg; ++k) s += chs[g * cpg + k];
        const float mg = s * inv_n;
        float q = 0.f;
        for (int k = 0; k < cpg; ++k) {
            const float d = chs[g * cpg + k] * inv_hw - mg;
            q += chq[g * cpg + k] + (float)HW * d * d;
        }
        gm[g] = mg;
        gr[g] = rsqrtf(q * inv_n + eps);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += SE_GATE_THREADS) {
        const int g = c / cpg;
        chq[c] = fmaf(gamma[c], (chs[c] * inv_hw - gm[g]) * gr[g], beta[c]);
    }
    __syncthreads();
    for (int j = wave; j < Cr; j += NW) {
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s = fmaf(w1[(int64_t)j * C + c], chq[c], s);
        s = wave_sum(s);
        if (lane == 0) hid[j] = fmaxf(s + b1[j], 0.f);
    }
    __syncthreads();
    for (int c = wave; c < C; c += NW) {
        float s = 0.f;
        for (int j = lane; j < Cr; j += 64) s = fmaf(w2[(int64_t)c * Cr + j], hid[j], s);
        s = wave_sum(s);
        if (lane == 0) gate[(int64_t)img * C + c] = 1.f / (1.f + expf(-(s + b2[c])));
    }
}

constexpr int SE_APPLY_THREADS = 256, SE_CACHE = 8192;

__global__ __launch_bounds__(SE_APPLY_THREADS) void k_se_apply(
    const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ gate, const float* __restrict__ residual, float* __restrict__ y, int C, int HW, int groups,
    float eps, int64_t x_img_stride, int64_t x_chan_stride, int splits, int64_t slab_stride, int64_t y_img_stride,
    int64_t r_img_stride, const float* __restrict__ x2, const float* __restrict__ gamma2, const float* __restrict__ beta2,
    int64_t x2_img_stride, int64_t x2_chan_stride, int splits2, int64_t slab_stride2) {
    __shared__ float cache[SE_CACHE];  // the group's reduced slabs (the backbones' groups hold exactly 8192 values)
    __shared__ float red[SE_APPLY_THREADS / 64];
    constexpr int NW = SE_APPLY_THREADS / 64;
    const int img = blockIdx.x / groups, g = blockIdx.x - img * groups;
    const int cpg = C / groups;
    const int n = cpg * HW;
    const bool cached = n <= SE_CACHE;
    const float* xp = x + (int64_t)img * x_img_stride + (int64_t)g * cpg * x_chan_stride;
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += SE_APPLY_THREADS) {
        const int c = i / HW;
        const float v = se_load(xp, c, i - c * HW, x_chan_stride, splits, slab_stride);
        if (cached) cache[i] = v;
        s += v;
    }
    const float mean = block_sum(s, red, NW) / (float)n;
    float q = 0.f;
    for (int i = threadIdx.x; i < n; i += SE_APPLY_THREADS) {
        const int c = i / HW;
        const float d = (cached ? cache[i] : se_load(xp, c, i - c * HW, x_chan_stride, splits, slab_stride)) - mean;
        q = fmaf(d, d, q);
    }
    const float rstd = rsqrtf(block_sum(q, red, NW) / (float)n + eps);
    const float* x2p = x2 ? x2 + (int64_t)img * x2_img_stride + (int64_t)g * cpg * x2_chan_stride : nullptr;
    float mean2 = 0.f, rstd2 = 0.f;
    if (x2p) {
        float s2 = 0.f;
        for (int i = threadIdx.x; i < n; i += SE_APPLY_THREADS) {
            const int c = i / HW;
            s2 += se_load(x2p, c, i - c * HW, x2_chan_stride, splits2, slab_stride2);
        }
        mean2 = block_sum(s2, red, NW) / (float)n;
        float q2 = 0.f;
        for (int i = threadIdx.x; i < n; i += SE_APPLY_THREADS) {
            const int c = i / HW;
            const float d = se_load(x2p, c, i - c * HW, x2_chan_stride, splits2, slab_stride2) - mean2;
            q2 = fmaf(d, d, q2);
        }
        rstd2 = rsqrtf(block_sum(q2, red, NW) / (float)n + eps);
    }
    float* yp = y + (int64_t)img * y_img_stride + (int64_t)g * n;
    const float* rp = residual ? residual + (int64_t)img * r_img_stride + (int64_t)g * n : nullptr;
    const float* gp = gate + (int64_t)img * C + g * cpg;
    for (int i = threadIdx.x; i < n; i += SE_APPLY_THREADS) {
        const int cl = i / HW, c = g * cpg + cl, pp = i - cl * HW;
        const float v = cached ? cache[i] : se_load(xp, cl, pp, x_chan_stride, splits, slab_stride);
        const float ga = gamma[c] * rstd, be = beta[c] - mean * ga;
        const float z = fmaf(v, ga, be);
        float idv;
        if (rp) {
            idv = rp[i];
        } else {
            const float ga2 = gamma2[c] * rstd2, be2 = beta2[c] - mean2 * ga2;
            idv = fmaf(se_load(x2p, cl, pp, x2_chan_stride, splits2, slab_stride2), ga2, be2);
        }
        yp[i] = fmaxf(fmaf(gp[cl], z, idv), 0.f);
    }
}

}  // namespace

extern "C" {

int ivln_gconv3x3_f32(const float* x, const float* w, float* y, int N, int C, int H, int W, int groups, int stride,
                      int64_t x_img_stride, void* stream) {
    if (!x || !w || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0 || groups <= 0) return IVLN_E_UNSUPPORTED;
    if (C % groups || C / groups > 64 || C > (1 << 20) || (stride != 1 && stride != 2)) return IVLN_E_UNSUPPORTED;
    if (x_img_stride == 0) x_img_stride = (int64_t)C * H * W;
    if (x_img_stride < (int64_t)C * H * W) return IVLN_E_UNSUPPORTED;
    GcArgs a;
    a.x = x, a.w = w, a.y = y;
    a.N = N, a.C = C, a.H = H, a.W = W, a.stride = stride, a.cpg = C / groups;
    a.Ho = (H - 1) / stride + 1, a.Wo = (W - 1) / stride + 1;
    a.x_img_stride = x_img_stride;
    a.tw_shift = a.Wo <= 4 ? 2 : a.Wo <= 8 ? 3 : 4;
    const int TW = 1 << a.tw_shift, TH = GC_PIX >> a.tw_shift;
    const int per = TH * 3 * ((TW - 1) * stride + 3);
    a.in_stride = per + ((16 - per % 32) + 32) % 32;
    if (a.in_stride > GC_IN_STRIDE_MAX) return IVLN_E_UNSUPPORTED;  // (cannot happen with the three tile shapes above)
    a.tiles_x = (a.Wo + TW - 1) / TW;
    const int64_t tiles = ((int64_t)N * a.Ho + TH - 1) / TH * a.tiles_x;
    if (tiles > 0x7fffffffLL) return IVLN_E_UNSUPPORTED;
    a.multi = 0, a.cpg_shift = 0;
    if (a.cpg % GC_IC == 0) {
        if (C / GC_OC > 65535) return IVLN_E_UNSUPPORTED;
        hipLaunchKernelGGL(k_gconv3x3_mfma, dim3((unsigned)tiles, C / GC_OC), dim3(GC_THREADS), 0, (hipStream_t)stream, a);
        return LAUNCH_OK();
    }
    int blocks_y;
    if (GC_OC % a.cpg == 0) {
        a.multi = 1;
        while ((1 << a.cpg_shift) < a.cpg) ++a.cpg_shift;
        blocks_y = (C + GC_OC - 1) / GC_OC;
    } else {
        blocks_y = groups * ((a.cpg + GC_OC - 1) / GC_OC);
    }
    if (blocks_y > 65535) return IVLN_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_gconv3x3_valu, dim3((unsigned)tiles, blocks_y), dim3(GC_THREADS), 0, (hipStream_t)stream, a);
    return LAUNCH_OK();
}

int ivln_se_gate_f32(const float* x, const float* gamma, const float* beta, int N, int C, int HW, int groups, float eps,
                     int64_t x_img_stride, int64_t x_chan_stride, int splits, int64_t slab_stride, const float* w1,
                     const float* b1, const float* w2, const float* b2, int Cr, float* gate, void* stream) {
    if (!x || !gamma || !beta || !w1 || !b1 || !w2 || !b2 || !gate) return IVLN_E_UNSUPPORTED;
    if (N <= 0 || C <= 0 || HW <= 0 || groups <= 0 || Cr <= 0 || C % groups) return IVLN_E_UNSUPPORTED;
    if (C > SE_MAX_C || Cr > SE_MAX_CR) return IVLN_E_UNSUPPORTED;
    if (x_chan_stride <= 0) x_chan_stride = HW;
    if (x_img_stride <= 0) x_img_stride = (int64_t)C * HW;
    if (splits < 1) splits = 1;
    // the float4 form: whole float4s per channel, at most four per lane of 64, every access on a 16-byte boundary
    int lpc_shift = -1;
    const int64_t strides = x_img_stride | x_chan_stride | (splits > 1 ? slab_stride : 0);
    if ((HW & 3) == 0 && HW <= 1024 && ((uintptr_t)x & 15) == 0 && (strides & 3) == 0) {
        lpc_shift = 0;
        while ((1 << lpc_shift) < (HW >> 2) && lpc_shift < 6) ++lpc_shift;
    }
    hipLaunchKernelGGL(k_se_gate, dim3(N), dim3(SE_GATE_THREADS), 0, (hipStream_t)stream, x, gamma, beta, C, HW, groups, eps,
                       x_img_stride, x_chan_stride, splits, slab_stride, w1, b1, w2, b2, Cr, gate, lpc_shift);
    return LAUNCH_OK();
}

int ivln_se_apply_f32(const float* x, const float* gamma, const float* beta, const float* gate, const float* residual,
                      float* y, int N, int C, int HW, int groups, float eps, int64_t x_img_stride, int64_t x_chan_stride,
                      int splits, int64_t slab_stride, int64_t y_img_stride, int64_t r_img_stride, const float* x2,
                      const float* gamma2, const float* beta2, int64_t x2_img_stride, int64_t x2_chan_stride, int splits2,
                      int64_t slab_stride2, void* stream) {
    if (!x || !gamma || !beta || !gate || !y) return IVLN_E_UNSUPPORTED;
    if ((residual != nullptr) == (x2 != nullptr)) return IVLN_E_UNSUPPORTED;
    if (x2 && (!gamma2 || !beta2)) return IVLN_E_UNSUPPORTED;
    if (N <= 0 || C <= 0 || HW <= 0 || groups <= 0 || C % groups) return IVLN_E_UNSUPPORTED;
    if ((int64_t)N * groups > 0x7fffffffLL || (int64_t)(C / groups) * HW > 0x7fffffffLL) return IVLN_E_UNSUPPORTED;
    if (x_chan_stride <= 0) x_chan_stride = HW;
    if (x_img_stride <= 0) x_img_stride = (int64_t)C * HW;
    if (y_img_stride <= 0) y_img_stride = (int64_t)C * HW;
    if (r_img_stride <= 0) r_img_stride = (int64_t)C * HW;
    if (x2_chan_stride <= 0) x2_chan_stride = HW;
    if (x2_img_stride <= 0) x2_img_stride = (int64_t)C * HW;
    if (splits < 1) splits = 1;
    if (splits2 < 1) splits2 = 1;
    hipLaunchKernelGGL(k_se_apply, dim3(N * groups), dim3(SE_APPLY_THREADS), 0, (hipStream_t)stream, x, gamma, beta, gate,
                       residual, y, C, HW, groups, eps, x_img_stride, x_chan_stride, splits, slab_stride, y_img_stride,
                       r_img_stride, x2, gamma2, beta2, x2_img_stride, x2_chan_stride, splits2, slab_stride2);
    return LAUNCH_OK();
}

}  // extern "C"
