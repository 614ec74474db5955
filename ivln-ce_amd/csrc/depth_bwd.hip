// Backward kernels of the DD-PPO depth ResNet (MODEL.DEPTH_ENCODER.trainable, resnet_encoders.py:31-43,95) for gfx950,
// all fp32 NCHW: GroupNorm backward (with the ReLU mask of the block's output and the masked gradient as an optional
// output), MaxPool2d(3, 2, 1) backward in gather form, and the (O, I, k, k) -> (I, O, k, k) weight transposition the
// transposed-conv input gradients read.  The conv gradients themselves are GEMMs (gemm_conv.hip).  No float atomics:
// every sum runs in a fixed order, two runs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/ivln_hip.h"
#include "../../include/ivln_depth_bwd.h"

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

constexpr int GB_THREADS = 512;
constexpr int GB_WAVES = GB_THREADS / 64;
constexpr int GB_MAX_CPG = 1024;  // channels per group whose sums fit the LDS arrays

// ------------------------------------------------------------------------------------------
// GroupNorm backward: one 512-thread workgroup per (image, group), as k_groupnorm.
//   dz = dy * (out > 0) (or dy), xh = (x - mean) * rstd
//   s1[c] = sum_hw dz, s2[c] = sum_hw dz * xh            (per channel of the group)
//   A = sum_c gamma[c] s1[c], B = sum_c gamma[c] s2[c]   (per group)
//   dx = rstd * (gamma[c] * dz - A / n - xh * B / n)
// The per-channel sums: a channel belongs to `wpc` waves (8 / channels when the group has fewer than 8), each wave sums a
// strided subset of the plane and the wave partials meet in LDS in wave order.  s1 / s2 of this image go to `part`
// ((N, C) each); k_gn_bwd_params sums them over the images in ascending order.
// VEC: HW % 4 == 0 and every pointer 16-byte aligned (the launcher's decision) - a float4 never crosses a channel.
// ------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(GB_THREADS) void k_gn_bwd(const float* __restrict__ dy, const float* __restrict__ x,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ gamma, const float* __restrict__ out,
                                                       int C, int HW, int groups, float* __restrict__ dx,
                                                       float* __restrict__ dz_out, float* __restrict__ part_dgamma,
                                                       float* __restrict__ part_dbeta) {
    __shared__ float s1[GB_MAX_CPG], s2[GB_MAX_CPG];
    __shared__ float pw1[GB_WAVES], pw2[GB_WAVES];
    __shared__ float ab[2];
    const int img = blockIdx.x / groups, g = blockIdx.x % groups;
    const int cpg = C / groups;
    const int64_t base = ((int64_t)img * C + (int64_t)g * cpg) * HW;
    const float m = mean[blockIdx.x], r = rstd[blockIdx.x];
    const float* dyp = dy + base;
    const float* xp = x + base;
    const float* op = out ? out + base : nullptr;
    float* dzp = dz_out ? dz_out + base : nullptr;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int wpc = cpg >= GB_WAVES ? 1 : GB_WAVES / cpg;  // waves per channel
    const int cpr = GB_WAVES / wpc;                        // channels per round
    const int slot = w / wpc, sub = w - slot * wpc;

    for (int c0 = 0; c0 < cpg; c0 += cpr) {
        const int cl = c0 + slot;
        float a1 = 0.f, a2 = 0.f;
        if (slot < cpr && cl < cpg) {
            const int64_t o = (int64_t)cl * HW;
            if (VEC) {
                for (int i = (sub * 64 + lane) * 4; i < HW; i += wpc * 256) {
                    float4 d = *reinterpret_cast<const float4*>(dyp + o + i);
                    const float4 v = *reinterpret_cast<const float4*>(xp + o + i);
                    if (op) {
                        const float4 y = *reinterpret_cast<const float4*>(op + o + i);
                        d.x = y.x > 0.f ? d.x : 0.f; d.y = y.y > 0.f ? d.y : 0.f;
                        d.z = y.z > 0.f ? d.z : 0.f; d.w = y.w > 0.f ? d.w : 0.f;
                    }
                    if (dzp) *reinterpret_cast<float4*>(dzp + o + i) = d;
                    a1 += (d.x + d.y) + (d.z + d.w);
                    a2 += (d.x * ((v.x - m) * r) + d.y * ((v.y - m) * r)) + (d.z * ((v.z - m) * r) + d.w * ((v.w - m) * r));
                }
            } else {
                for (int i = sub * 64 + lane; i < HW; i += wpc * 64) {
                    float d = dyp[o + i];
                    if (op) d = op[o + i] > 0.f ? d : 0.f;
                    if (dzp) dzp[o + i] = d;
                    a1 += d;
                    a2 += d * ((xp[o + i] - m) * r);
                }
            }
        }
        a1 = wave_sum(a1);
        a2 = wave_sum(a2);
        if (lane == 0) {
            pw1[w] = a1;
            pw2[w] = a2;
        }
        __syncthreads();
        if (tid < cpr && c0 + tid < cpg) {
            float t1 = 0.f, t2 = 0.f;
            for (int k = 0; k < wpc; ++k) {
                t1 += pw1[tid * wpc + k];
                t2 += pw2[tid * wpc + k];
            }
            s1[c0 + tid] = t1;
            s2[c0 + tid] = t2;
        }
        __syncthreads();
    }
    // group sums (one wave, fixed order) and this image's partials of dgamma / dbeta
    if (w == 0) {
        float A = 0.f, B = 0.f;
        for (int c = lane; c < cpg; c += 64) {
            const float ga = gamma[g * cpg + c];
            A += ga * s1[c];
            B += ga * s2[c];
        }
        A = wave_sum(A);
        B = wave_sum(B);
        if (lane == 0) {
            ab[0] = A;
            ab[1] = B;
        }
    }
    for (int c = tid; c < cpg; c += GB_THREADS) {
        part_dbeta[(int64_t)img * C + g * cpg + c] = s1[c];
        part_dgamma[(int64_t)img * C + g * cpg + c] = s2[c];
    }
    __syncthreads();
    const int n = cpg * HW;
    const float inv_n = 1.f / (float)n;
    const float mA = ab[0] * inv_n, mB = ab[1] * inv_n;
    float* dxp = dx + base;
    if (VEC) {
        for (int i = tid * 4; i < n; i += GB_THREADS * 4) {
            const float ga = gamma[g * cpg + i / HW];
            float4 d = *reinterpret_cast<const float4*>(dyp + i);
            const float4 v = *reinterpret_cast<const float4*>(xp + i);
            if (op) {
                const float4 y = *reinterpret_cast<const float4*>(op + i);
                d.x = y.x > 0.f ? d.x : 0.f; d.y = y.y > 0.f ? d.y : 0.f;
                d.z = y.z > 0.f ? d.z : 0.f; d.w = y.w > 0.f ? d.w : 0.f;
            }
            float4 q;
            q.x = r * (ga * d.x - mA - ((v.x - m) * r) * mB);
            q.y = r * (ga * d.y - mA - ((v.y - m) * r) * mB);
            q.z = r * (ga * d.z - mA - ((v.z - m) * r) * mB);
            q.w = r * (ga * d.w - mA - ((v.w - m) * r) * mB);
            *reinterpret_cast<float4*>(dxp + i) = q;
        }
    } else {
        for (int i = tid; i < n; i += GB_THREADS) {
            const float ga = gamma[g * cpg + i / HW];
            float d = dyp[i];
            if (op) d = op[i] > 0.f ? d : 0.f;
            dxp[i] = r * (ga * d - mA - ((xp[i] - m) * r) * mB);
        }
    }
}

// dgamma[c] = sum_img part_dgamma[img][c], dbeta likewise: ascending image order
__global__ __launch_bounds__(256) void k_gn_bwd_params(const float* __restrict__ part_dgamma,
                                                       const float* __restrict__ part_dbeta, int N, int C,
                                                       float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float sg = 0.f, sb = 0.f;
    for (int i = 0; i < N; ++i) {
        sg += part_dgamma[(int64_t)i * C + c];
        sb += part_dbeta[(int64_t)i * C + c];
    }
    dgamma[c] = sg;
    dbeta[c] = sb;
}

// ------------------------------------------------------------------------------------------
// MaxPool2d(3, 2, 1) backward, gather form: an input pixel sums the gradients of the (at most 4) windows in which it is
// the FIRST maximum in row-major window order (torch's rule: a later value replaces the maximum only when it is greater,
// or NaN), the maximum recomputed from the saved input plane.  Windows are visited in ascending (oh, ow).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_maxpool3s2_bwd(const float* __restrict__ dy, const float* __restrict__ x,
                                                        int64_t total, int H, int W, int Ho, int Wo,
                                                        float* __restrict__ dx) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int wq = (int)(idx % W);
    const int hq = (int)((idx / W) % H);
    const int64_t plane = idx / ((int64_t)W * H);
    const float* xp = x + plane * H * W;
    const float* dp = dy + plane * Ho * Wo;
    const int oh0 = max(0, hq / 2), oh1 = min(Ho - 1, (hq + 1) / 2);  // windows with 2*oh - 1 <= hq <= 2*oh + 1
    const int ow0 = max(0, wq / 2), ow1 = min(Wo - 1, (wq + 1) / 2);
    float acc = 0.f;
    for (int oh = oh0; oh <= oh1; ++oh) {
        for (int ow = ow0; ow <= ow1; ++ow) {
            const int h0 = max(0, 2 * oh - 1), h1 = min(H - 1, 2 * oh + 1);
            const int w0 = max(0, 2 * ow - 1), w1 = min(W - 1, 2 * ow + 1);
            float best = -INFINITY;
            int bh = h0, bw = w0;
            for (int h = h0; h <= h1; ++h) {
                for (int w = w0; w <= w1; ++w) {
                    const float v = xp[h * W + w];
                    if (v > best || v != v) {
                        best = v;
                        bh = h;
                        bw = w;
                    }
                }
            }
            if (bh == hq && bw == wq) acc += dp[oh * Wo + ow];
        }
    }
    dx[idx] = acc;
}

// W (O, I, KK) -> (I, O, KK), taps in place (no flip): the weight layout ops.conv_transpose2d reads
__global__ __launch_bounds__(256) void k_weight_oi_transpose(const float* __restrict__ w, float* __restrict__ wt, int O,
                                                             int I, int KK) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)O * I * KK) return;
    const int k = (int)(idx % KK);
    const int o = (int)((idx / KK) % O);
    const int i = (int)(idx / ((int64_t)KK * O));
    wt[idx] = w[((int64_t)o * I + i) * KK + k];
}

}  // namespace

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP)

extern "C" {

int ivln_groupnorm_bwd_f32(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                           const float* out, int N, int C, int HW, int groups, float* dx, float* dz_out, float* dgamma,
                           float* dbeta, float* ws, int64_t ws_floats, void* stream) {
    if (!dy || !x || !mean || !rstd || !gamma || !dx || !dgamma || !dbeta || !ws) return IVLN_E_INVALID;
    if (N <= 0 || C <= 0 || HW <= 0 || groups <= 0 || C % groups) return IVLN_E_INVALID;
    if (ws_floats < (int64_t)2 * N * C) return IVLN_E_INVALID;
    if (C / groups > GB_MAX_CPG || (int64_t)(C / groups) * HW > INT32_MAX || (int64_t)N * groups > INT32_MAX)
        return IVLN_E_UNSUPPORTED;
    const uintptr_t ptrs = (uintptr_t)dy | (uintptr_t)x | (uintptr_t)out | (uintptr_t)dx | (uintptr_t)dz_out;
    const bool vec = (HW & 3) == 0 && (ptrs & 15) == 0;
    float* pg = ws;
    float* pb = ws + (int64_t)N * C;
    if (vec)
        hipLaunchKernelGGL(k_gn_bwd<true>, dim3(N * groups), dim3(GB_THREADS), 0, (hipStream_t)stream, dy, x, mean, rstd,
                           gamma, out, C, HW, groups, dx, dz_out, pg, pb);
    else
        hipLaunchKernelGGL(k_gn_bwd<false>, dim3(N * groups), dim3(GB_THREADS), 0, (hipStream_t)stream, dy, x, mean, rstd,
                           gamma, out, C, HW, groups, dx, dz_out, pg, pb);
    hipLaunchKernelGGL(k_gn_bwd_params, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, pg, pb, N, C, dgamma,
                       dbeta);
    return LAUNCH_OK();
}

int ivln_maxpool3s2_bwd_f32(const float* dy, const float* x, int planes, int H, int W, float* dx, void* stream) {
    if (!dy || !x || !dx || planes <= 0 || H <= 0 || W <= 0) return IVLN_E_INVALID;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int64_t total = (int64_t)planes * H * W;
    if ((int64_t)H * W > INT32_MAX || (total + 255) / 256 > INT32_MAX) return IVLN_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_maxpool3s2_bwd, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, x,
                       total, H, W, Ho, Wo, dx);
    return LAUNCH_OK();
}

int ivln_weight_oi_transpose_f32(const float* w, float* wt, int O, int I, int KK, void* stream) {
    if (!w || !wt || O <= 0 || I <= 0 || KK <= 0) return IVLN_E_INVALID;
    const int64_t total = (int64_t)O * I * KK;
    if ((total + 255) / 256 > INT32_MAX) return IVLN_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_weight_oi_transpose, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w,
                       wt, O, I, KK);
    return LAUNCH_OK();
}

}  // extern "C"
