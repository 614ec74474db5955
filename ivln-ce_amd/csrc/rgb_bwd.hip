// Kernels of the trainable torchvision ResNet-50 RGB encoder (MODEL.RGB_ENCODER.trainable, resnet_encoders.py:141-143,194)
// for gfx950, all fp32 NCHW: the train-mode BatchNorm epilogue (scale / shift, the bottleneck tail with one or two
// normalised operands, ReLU), BatchNorm backward (with the ReLU mask of the activated output and the masked gradient as an
// optional output) and the backward of the adaptive average pool.  The conv gradients are GEMMs (gemm_conv.hip), the
// max-pool backward is depth_bwd.hip's.  No float atomics: every sum runs in a fixed order, two runs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/ivln_hip.h"
#include "../../include/ivln_rgb_bwd.h"

namespace {

constexpr int BT = 256;  // threads per workgroup, every kernel of this file

// The elementwise kernels walk the tensor flat, BT * V consecutive floats per workgroup (V = 4: one float4 per thread,
// HW % 4 == 0 so that it never crosses a plane).  The plane of the workgroup's first element is one 64-bit division on
// uniform values; a thread is at most BT * V floats further: a 32-bit division.
template <int V>
__device__ __forceinline__ bool flat_pos(int64_t total, int C, int HW, int64_t& idx, int& c) {
    const int64_t base = (int64_t)blockIdx.x * (BT * V);
    const int64_t p0 = base / HW;
    const int off = (int)(base - p0 * HW) + (int)threadIdx.x * V;
    idx = base + (int64_t)threadIdx.x * V;
    c = (int)((p0 + off / HW) % C);
    return idx < total;
}

// ------------------------------------------------------------------------------------------
// (a) y = [relu](x * scale[c] + shift[c] [+ r] [+ r2 * scale2[c] + shift2[c]])
// ------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(BT) void k_bn_apply(const float* __restrict__ x, const float* __restrict__ scale,
                                                 const float* __restrict__ shift, const float* __restrict__ r,
                                                 const float* __restrict__ r2, const float* __restrict__ scale2,
                                                 const float* __restrict__ shift2, int64_t total, int C, int HW, int relu,
                                                 float* __restrict__ y) {
    int64_t idx;
    int c;
    if (!flat_pos<(VEC ? 4 : 1)>(total, C, HW, idx, c)) return;
    const float sc = scale[c], sh = shift[c];
    const float sc2 = r2 ? scale2[c] : 0.f, sh2 = r2 ? shift2[c] : 0.f;
    if (VEC) {
        const float4 v = *reinterpret_cast<const float4*>(x + idx);
        float o[4] = {fmaf(v.x, sc, sh), fmaf(v.y, sc, sh), fmaf(v.z, sc, sh), fmaf(v.w, sc, sh)};
        if (r) {
            const float4 a = *reinterpret_cast<const float4*>(r + idx);
            o[0] += a.x, o[1] += a.y, o[2] += a.z, o[3] += a.w;
        }
        if (r2) {
            const float4 a = *reinterpret_cast<const float4*>(r2 + idx);
            o[0] += fmaf(a.x, sc2, sh2), o[1] += fmaf(a.y, sc2, sh2), o[2] += fmaf(a.z, sc2, sh2), o[3] += fmaf(a.w, sc2, sh2);
        }
        if (relu) {
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = fmaxf(o[k], 0.f);
        }
        *reinterpret_cast<float4*>(y + idx) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
        float o = fmaf(x[idx], sc, sh);
        if (r) o += r[idx];
        if (r2) o += fmaf(r2[idx], sc2, sh2);
        y[idx] = relu ? fmaxf(o, 0.f) : o;
    }
}

// ------------------------------------------------------------------------------------------
// (b) BatchNorm backward.  dz = dy * (out > 0) (or dy), xh = (x - mean[c]) * rstd[c]
//   S1[c] = sum dz (= dbeta), S2[c] = sum dz * xh (= dgamma)
//   train: dx = gamma * rstd * (dz - S1 / M - xh * S2 / M);  eval: dx = gamma * rstd * dz
// A channel's values are N planes of HW floats, C * HW apart.  k_bn_bwd_stats: a workgroup serves 256 / lpc neighbouring
// channels - one contiguous run of memory per image - with lpc lanes per channel (lpc = 256: the 112 x 112 planes of the
// stem, one channel per workgroup; lpc = 16: the 7 x 7 planes of layer 4, 16 channels per workgroup) and one slice of the
// images (grid.y: few channels with large planes spread over more workgroups).  The sums are doubles (k_cbra_bwd_stats
// says why): per lane in image / plane order, then across the lanes of a channel by a fixed butterfly, the slices by
// k_bn_bwd_final in ascending order.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float bn_rstd(const float* rv, int c, int train, float eps) {
    return train ? rv[c] : 1.f / sqrtf(rv[c] + eps);  // (eval: the running variance, as k_bn_fold turns it into a scale)
}

template <bool VEC>
__global__ __launch_bounds__(BT) void k_bn_bwd_stats(const float* __restrict__ dy, const float* __restrict__ x,
                                                     const float* __restrict__ mean, const float* __restrict__ rv,
                                                     const float* __restrict__ out, int N, int C, int HW, int train,
                                                     float eps, int lpc, int imgs_per_split, double* __restrict__ partial) {
    __shared__ double red[2][BT / 64];
    const int tid = threadIdx.x, l = tid & (lpc - 1);
    const int c = blockIdx.x * (BT / lpc) + tid / lpc;
    const int sp = blockIdx.y, S = gridDim.y;
    const int i0 = sp * imgs_per_split, i1 = min(N, i0 + imgs_per_split);
    const bool live = c < C;
    const float mu = live ? mean[c] : 0.f, rs = live ? bn_rstd(rv, c, train, eps) : 0.f;
    double s1 = 0.0, s2 = 0.0;
    if (live) {
        for (int img = i0; img < i1; ++img) {
            const int64_t o = ((int64_t)img * C + c) * HW;
            if (VEC) {
                for (int i = l * 4; i < HW; i += lpc * 4) {
                    float4 d = *reinterpret_cast<const float4*>(dy + o + i);
                    const float4 v = *reinterpret_cast<const float4*>(x + o + i);
                    if (out) {
                        const float4 y = *reinterpret_cast<const float4*>(out + o + i);
                        d.x = y.x > 0.f ? d.x : 0.f, d.y = y.y > 0.f ? d.y : 0.f;
                        d.z = y.z > 0.f ? d.z : 0.f, d.w = y.w > 0.f ? d.w : 0.f;
                    }
                    s1 += ((double)d.x + (double)d.y) + ((double)d.z + (double)d.w);
                    s2 += ((double)(d.x * ((v.x - mu) * rs)) + (double)(d.y * ((v.y - mu) * rs))) +
                          ((double)(d.z * ((v.z - mu) * rs)) + (double)(d.w * ((v.w - mu) * rs)));
                }
            } else {
                for (int i = l; i < HW; i += lpc) {
                    float d = dy[o + i];
                    if (out) d = out[o + i] > 0.f ? d : 0.f;
                    s1 += (double)d;
                    s2 += (double)(d * ((x[o + i] - mu) * rs));
                }
            }
        }
    }
    // the lanes of a channel: lpc <= 64 inside one wave; lpc = 256 the four waves through LDS, in wave order
    for (int w = min(lpc, 64) >> 1; w > 0; w >>= 1) {
        s1 += __shfl_xor(s1, w);
        s2 += __shfl_xor(s2, w);
    }
    if (lpc > 64) {
        if ((tid & 63) == 0) red[0][tid >> 6] = s1, red[1][tid >> 6] = s2;
        __syncthreads();
        if (tid == 0) {
            s1 = s2 = 0.0;
            for (int w = 0; w < BT / 64; ++w) s1 += red[0][w], s2 += red[1][w];
        }
    }
    if (l == 0 && live) {
        partial[((int64_t)c * S + sp) * 2] = s1;
        partial[((int64_t)c * S + sp) * 2 + 1] = s2;
    }
}

// one thread per channel: the S slices of both sums in ascending order -> dbeta, dgamma
__global__ __launch_bounds__(64) void k_bn_bwd_final(const double* __restrict__ partial, int S, int C,
                                                     float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    double a = 0.0, b = 0.0;
    for (int sp = 0; sp < S; ++sp) {
        a += partial[((int64_t)c * S + sp) * 2];
        b += partial[((int64_t)c * S + sp) * 2 + 1];
    }
    dbeta[c] = (float)a;
    dgamma[c] = (float)b;
}

// dx may be `out`, dz_out may be `dy`: each thread reads its elements of all operands before it writes them (no __restrict__)
template <bool VEC>
__global__ __launch_bounds__(BT) void k_bn_bwd_apply(const float* dy, const float* x, const float* __restrict__ mean,
                                                     const float* __restrict__ rv, const float* __restrict__ gamma,
                                                     const float* out, const float* __restrict__ dgamma,
                                                     const float* __restrict__ dbeta, int64_t total, int C, int HW,
                                                     float M, int train, float eps, float* dx, float* dz_out) {
    int64_t idx;
    int c;
    if (!flat_pos<(VEC ? 4 : 1)>(total, C, HW, idx, c)) return;
    const float mu = mean[c], rs = bn_rstd(rv, c, train, eps);
    const float sc = gamma[c] * rs;
    const float b_m = train ? dbeta[c] / M : 0.f, g_m = train ? dgamma[c] / M : 0.f;
    if (VEC) {
        const float4 dv = *reinterpret_cast<const float4*>(dy + idx);
        const float4 xv = *reinterpret_cast<const float4*>(x + idx);
        float d[4] = {dv.x, dv.y, dv.z, dv.w};
        const float xx[4] = {xv.x, xv.y, xv.z, xv.w};
        if (out) {
            const float4 yv = *reinterpret_cast<const float4*>(out + idx);
            d[0] = yv.x > 0.f ? d[0] : 0.f, d[1] = yv.y > 0.f ? d[1] : 0.f;
            d[2] = yv.z > 0.f ? d[2] : 0.f, d[3] = yv.w > 0.f ? d[3] : 0.f;
        }
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = train ? sc * (d[k] - b_m - ((xx[k] - mu) * rs) * g_m) : sc * d[k];
        if (dz_out) *reinterpret_cast<float4*>(dz_out + idx) = make_float4(d[0], d[1], d[2], d[3]);
        *reinterpret_cast<float4*>(dx + idx) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
        float d = dy[idx];
        const float xx = x[idx];
        if (out) d = out[idx] > 0.f ? d : 0.f;
        if (dz_out) dz_out[idx] = d;
        dx[idx] = train ? sc * (d - b_m - ((xx - mu) * rs) * g_m) : sc * d;
    }
}

// ------------------------------------------------------------------------------------------
// (c) adaptive average pool backward, gather form: window o of an axis is [floor(o * H / OH), ceil((o + 1) * H / OH)) -
// overlapping for 7 -> 4 and 3 -> 4, replicating for 2 -> 4 - and an input pixel sums dy / (window size) of every window
// that covers it, in ascending (oh, ow).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BT) void k_adaptive_avgpool2d_bwd(const float* __restrict__ dy, int64_t total, int C, int H,
                                                               int W, int OH, int OW, int64_t dy_img_stride,
                                                               float* __restrict__ dx) {
    const int64_t idx = (int64_t)blockIdx.x * BT + threadIdx.x;
    if (idx >= total) return;
    const int w = (int)(idx % W), h = (int)((idx / W) % H);
    const int64_t nc = idx / ((int64_t)W * H);
    const int n = (int)(nc / C), c = (int)(nc % C);
    const float* dp = dy + (int64_t)n * dy_img_stride + (int64_t)c * OH * OW;
    float acc = 0.f;
    for (int oh = 0; oh < OH; ++oh) {
        const int h0 = (oh * H) / OH, h1 = ((oh + 1) * H + OH - 1) / OH;
        if (h < h0 || h >= h1) continue;
        for (int ow = 0; ow < OW; ++ow) {
            const int w0 = (ow * W) / OW, w1 = ((ow + 1) * W + OW - 1) / OW;
            if (w < w0 || w >= w1) continue;
            acc += dp[oh * OW + ow] / (float)((h1 - h0) * (w1 - w0));
        }
    }
    dx[idx] = acc;
}

inline bool grid_fits(int64_t total, int per_block) { return (total + per_block - 1) / per_block <= INT32_MAX; }

}  // namespace

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP)

extern "C" {

int ivln_bn_apply_f32(const float* x, const float* scale, const float* shift, const float* r, const float* r2,
                      const float* scale2, const float* shift2, int N, int C, int HW, int relu, float* y, void* stream) {
    if (!x || !scale || !shift || !y || N <= 0 || C <= 0 || HW <= 0) return IVLN_E_INVALID;
    if ((r2 != nullptr) != (scale2 != nullptr) || (r2 != nullptr) != (shift2 != nullptr)) return IVLN_E_INVALID;
    const int64_t total = (int64_t)N * C * HW;
    const uintptr_t ptrs = (uintptr_t)x | (uintptr_t)r | (uintptr_t)r2 | (uintptr_t)y;
    const bool vec = (HW & 3) == 0 && (ptrs & 15) == 0;
    const int per = vec ? BT * 4 : BT;
    if (!grid_fits(total, per) || (int64_t)N * C > INT32_MAX) return IVLN_E_UNSUPPORTED;
    const dim3 grid((unsigned)((total + per - 1) / per));
    if (vec)
        hipLaunchKernelGGL(k_bn_apply<true>, grid, dim3(BT), 0, (hipStream_t)stream, x, scale, shift, r, r2, scale2, shift2,
                           total, C, HW, relu, y);
    else
        hipLaunchKernelGGL(k_bn_apply<false>, grid, dim3(BT), 0, (hipStream_t)stream, x, scale, shift, r, r2, scale2, shift2,
                           total, C, HW, relu, y);
    return LAUNCH_OK();
}

int ivln_bn_bwd_f32(const float* dy, const float* x, const float* mean, const float* rstd_or_var, const float* gamma,
                    const float* out, int N, int C, int HW, int train, float eps, float* dx, float* dz_out, float* dgamma,
                    float* dbeta, float* ws, int64_t ws_floats, void* stream) {
    if (!dy || !x || !mean || !rstd_or_var || !gamma || !dx || !dgamma || !dbeta || !ws) return IVLN_E_INVALID;
    if (N <= 0 || C <= 0 || HW <= 0 || ws_floats < (int64_t)4 * C + 2 || ((uintptr_t)ws & 3)) return IVLN_E_INVALID;
    const int64_t total = (int64_t)N * C * HW;
    const uintptr_t ptrs = (uintptr_t)dy | (uintptr_t)x | (uintptr_t)out | (uintptr_t)dx | (uintptr_t)dz_out;
    const bool vec = (HW & 3) == 0 && (ptrs & 15) == 0;
    const int per = vec ? BT * 4 : BT;
    if (!grid_fits(total, per) || (int64_t)N * C > INT32_MAX) return IVLN_E_UNSUPPORTED;
    double* wsd = reinterpret_cast<double*>(((uintptr_t)ws + 7) & ~(uintptr_t)7);  // partials are doubles

    // lanes per channel: about four accesses per lane and plane; beyond one wave the whole workgroup
    const int units = vec ? HW / 4 : HW;
    int lpc = 1;
    while (lpc < BT && lpc * 4 < units) lpc *= 2;
    if (lpc > 64) lpc = BT;
    const int cg = BT / lpc, groups = (C + cg - 1) / cg;
    // slices of the images: towards 2048 workgroups (8 per CU), at least 8192 elements each, at most 64
    const int64_t min_imgs = (8192 + (int64_t)cg * HW - 1) / ((int64_t)cg * HW);
    int64_t S = 2048 / groups;
    if (S > N / min_imgs) S = N / min_imgs;
    if (S > 64) S = 64;
    if (S > (ws_floats - 2) / ((int64_t)4 * C)) S = (ws_floats - 2) / ((int64_t)4 * C);
    if (S < 1) S = 1;
    const int ips = (int)((N + S - 1) / S);
    S = (N + ips - 1) / ips;

    const dim3 sgrid(groups, (unsigned)S);
    if (vec)
        hipLaunchKernelGGL(k_bn_bwd_stats<true>, sgrid, dim3(BT), 0, (hipStream_t)stream, dy, x, mean, rstd_or_var, out, N, C,
                           HW, train, eps, lpc, ips, wsd);
    else
        hipLaunchKernelGGL(k_bn_bwd_stats<false>, sgrid, dim3(BT), 0, (hipStream_t)stream, dy, x, mean, rstd_or_var, out, N, C,
                           HW, train, eps, lpc, ips, wsd);
    hipLaunchKernelGGL(k_bn_bwd_final, dim3((C + 63) / 64), dim3(64), 0, (hipStream_t)stream, wsd, (int)S, C, dgamma, dbeta);
    const dim3 agrid((unsigned)((total + per - 1) / per));
    const float M = (float)N * (float)HW;
    if (vec)
        hipLaunchKernelGGL(k_bn_bwd_apply<true>, agrid, dim3(BT), 0, (hipStream_t)stream, dy, x, mean, rstd_or_var, gamma, out,
                           dgamma, dbeta, total, C, HW, M, train, eps, dx, dz_out);
    else
        hipLaunchKernelGGL(k_bn_bwd_apply<false>, agrid, dim3(BT), 0, (hipStream_t)stream, dy, x, mean, rstd_or_var, gamma, out,
                           dgamma, dbeta, total, C, HW, M, train, eps, dx, dz_out);
    return LAUNCH_OK();
}

int ivln_adaptive_avgpool2d_bwd_f32(const float* dy, int N, int C, int H, int W, int OH, int OW, int64_t dy_img_stride,
                                    float* dx, void* stream) {
    if (!dy || !dx || N <= 0 || C <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return IVLN_E_INVALID;
    if (dy_img_stride <= 0) dy_img_stride = (int64_t)C * OH * OW;
    if (dy_img_stride < (int64_t)C * OH * OW) return IVLN_E_INVALID;
    const int64_t total = (int64_t)N * C * H * W;
    if (!grid_fits(total, BT) || (int64_t)H * OH > INT32_MAX || (int64_t)W * OW > INT32_MAX || (int64_t)OH * OW > INT32_MAX)
        return IVLN_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_adaptive_avgpool2d_bwd, dim3((unsigned)((total + BT - 1) / BT)), dim3(BT), 0, (hipStream_t)stream, dy,
                       total, C, H, W, OH, OW, dy_img_stride, dx);
    return LAUNCH_OK();
}

}  // extern "C"
