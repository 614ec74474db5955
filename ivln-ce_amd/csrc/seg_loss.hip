// Segmentation loss and metrics for fine-tuning RedNet on gfx950 (include/ivln_seg_train.h): pixel cross-entropy over NCHW
// scores against nearest-neighbour down-sampled u8 labels (loss + gradient), and confusion counts.  The per-pixel
// arithmetic and every sum are double, in a fixed order: no float atomics, two runs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/ivln_hip.h"
#include "../../include/ivln_seg_train.h"

namespace {

constexpr int BT = 256;        // threads per workgroup, every kernel of this file
constexpr int MAX_BLOCKS = 1024;  // partial sums per call: ws holds 2 * MAX_BLOCKS + 2 doubles (+ alignment slack)

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP)

// One lane's V pixels: unit u = V consecutive pixels of one image plane (V = 4 needs hw % 4 == 0, so a unit never
// crosses a plane).  base = the class-0 score of the first pixel, t[k] = the target or -1 (ignored / refused).
template <int V>
struct Unit {
    const float* base;
    int64_t off;  // offset of `base` in the scores tensor (the gradient is written at the same place)
    int t[V];
};

template <int V>
__device__ __forceinline__ Unit<V> load_unit(const float* scores, const uint8_t* labels, int64_t u, int C, int h, int w, int s,
                                             int ignore, int* err) {
    Unit<V> r;
    const int hw = h * w, upp = hw / V;  // units per plane
    const int64_t n = u / upp;
    const int q = (int)(u - n * upp) * V;
    r.off = n * C * hw + q;
    r.base = scores + r.off;
    const int64_t W = (int64_t)w * s, img = n * ((int64_t)h * s) * W;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const int pix = q + k, i = pix / w, j = pix - i * w;
        int t = labels[img + (int64_t)i * s * W + (int64_t)j * s];
        if (t == ignore) t = -1;
        else if (t >= C) {
            atomicOr(err, 1);
            t = -1;
        }
        r.t[k] = t;
    }
    return r;
}

// max and sum of exp(x - max) over the classes, per pixel of the unit
template <int V>
__device__ __forceinline__ void unit_lse(const float* base, int C, int hw, float (&m)[V], double (&se)[V]) {
#pragma unroll
    for (int k = 0; k < V; ++k) m[k] = -INFINITY, se[k] = 0.0;
    for (int c = 0; c < C; ++c) {
        float v[V];
        if constexpr (V == 4) {
            const float4 f = *reinterpret_cast<const float4*>(base + (int64_t)c * hw);
            v[0] = f.x, v[1 % V] = f.y, v[2 % V] = f.z, v[3 % V] = f.w;
        } else {
            v[0] = base[(int64_t)c * hw];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) m[k] = fmaxf(m[k], v[k]);
    }
    for (int c = 0; c < C; ++c) {
        float v[V];
        if constexpr (V == 4) {
            const float4 f = *reinterpret_cast<const float4*>(base + (int64_t)c * hw);
            v[0] = f.x, v[1 % V] = f.y, v[2 % V] = f.z, v[3 % V] = f.w;
        } else {
            v[0] = base[(int64_t)c * hw];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) se[k] += exp((double)v[k] - (double)m[k]);
    }
}

// fixed tree over the workgroup's lanes
__device__ __forceinline__ void block_sum2(double& a, double& b, double (*red)[BT]) {
    const int tid = threadIdx.x;
    red[0][tid] = a, red[1][tid] = b;
    __syncthreads();
    for (int st = BT / 2; st > 0; st >>= 1) {
        if (tid < st) red[0][tid] += red[0][tid + st], red[1][tid] += red[1][tid + st];
        __syncthreads();
    }
    a = red[0][0], b = red[1][0];
}

// (a) partial[2 b] = sum wt[t] * nll, partial[2 b + 1] = sum wt[t] over workgroup b's pixels
template <int V>
__global__ __launch_bounds__(BT) void k_seg_ce_partial(const float* __restrict__ scores, const uint8_t* __restrict__ labels,
                                                       const float* __restrict__ class_w, int64_t units, int C, int h, int w,
                                                       int s, int ignore, double* __restrict__ partial, int* err) {
    __shared__ double red[2][BT];
    const int hw = h * w;
    double num = 0.0, den = 0.0;
    for (int64_t u = (int64_t)blockIdx.x * BT + threadIdx.x; u < units; u += (int64_t)gridDim.x * BT) {
        const Unit<V> un = load_unit<V>(scores, labels, u, C, h, w, s, ignore, err);
        bool any = false;
#pragma unroll
        for (int k = 0; k < V; ++k) any = any || un.t[k] >= 0;
        if (!any) continue;
        float m[V];
        double se[V];
        unit_lse<V>(un.base, C, hw, m, se);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (un.t[k] < 0) continue;
            const double wt = class_w ? (double)class_w[un.t[k]] : 1.0;
            const double xt = (double)un.base[(int64_t)un.t[k] * hw + k];
            num += wt * (log(se[k]) + ((double)m[k] - xt));
            den += wt;
        }
    }
    block_sum2(num, den, red);
    if (threadIdx.x == 0) partial[2 * blockIdx.x] = num, partial[2 * blockIdx.x + 1] = den;
}

// (b) the partials in ascending order -> ws[0] = num, ws[1] = den, loss = num / den (0 when den == 0)
__global__ __launch_bounds__(BT) void k_seg_ce_final(const double* __restrict__ partial, int blocks, double* __restrict__ totals,
                                                     float* __restrict__ loss, const int* __restrict__ err) {
    __shared__ double red[2][BT];
    double num = 0.0, den = 0.0;
    for (int b = threadIdx.x; b < blocks; b += BT) num += partial[2 * b], den += partial[2 * b + 1];
    block_sum2(num, den, red);
    if (threadIdx.x == 0) {
        totals[0] = num, totals[1] = den;
        if (*err == 0) *loss = den > 0.0 ? (float)(num / den) : 0.f;
    }
}

// (c) dscores = scale * wt[t] / den * (softmax - onehot(t)), zero at ignored pixels and when den == 0
template <int V>
__global__ __launch_bounds__(BT) void k_seg_ce_grad(const float* __restrict__ scores, const uint8_t* __restrict__ labels,
                                                    const float* __restrict__ class_w, int64_t units, int C, int h, int w, int s,
                                                    int ignore, double scale, const double* __restrict__ totals,
                                                    float* __restrict__ dscores, int* err) {
    if (*err != 0) return;  // (set by pass (a), which saw every label this pass would see)
    const int hw = h * w;
    const double den = totals[1];
    const double g = den > 0.0 ? scale / den : 0.0;
    for (int64_t u = (int64_t)blockIdx.x * BT + threadIdx.x; u < units; u += (int64_t)gridDim.x * BT) {
        const Unit<V> un = load_unit<V>(scores, labels, u, C, h, w, s, ignore, err);
        float m[V];
        double se[V], coef[V];
        unit_lse<V>(un.base, C, hw, m, se);
#pragma unroll
        for (int k = 0; k < V; ++k) coef[k] = un.t[k] >= 0 ? g * (class_w ? (double)class_w[un.t[k]] : 1.0) : 0.0;
        float* dst = dscores + un.off;
        for (int c = 0; c < C; ++c) {
            float v[V], o[V];
            if constexpr (V == 4) {
                const float4 f = *reinterpret_cast<const float4*>(un.base + (int64_t)c * hw);
                v[0] = f.x, v[1 % V] = f.y, v[2 % V] = f.z, v[3 % V] = f.w;
            } else {
                v[0] = un.base[(int64_t)c * hw];
            }
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const double p = exp((double)v[k] - (double)m[k]) / se[k];
                o[k] = coef[k] != 0.0 ? (float)(coef[k] * (p - (c == un.t[k] ? 1.0 : 0.0))) : 0.f;
            }
            if constexpr (V == 4)
                *reinterpret_cast<float4*>(dst + (int64_t)c * hw) = make_float4(o[0], o[1 % V], o[2 % V], o[3 % V]);
            else
                dst[(int64_t)c * hw] = o[0];
        }
    }
}

// confusion counts: a C x C histogram per workgroup in LDS (integer atomics), its non-zero cells added to the global one
__global__ __launch_bounds__(BT) void k_seg_confusion(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ truth,
                                                      int64_t n, int C, int ignore, unsigned long long* __restrict__ counts,
                                                      int* err) {
    __shared__ unsigned int hist[64 * 64];
    const int cells = C * C;
    for (int i = threadIdx.x; i < cells; i += BT) hist[i] = 0u;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * BT + threadIdx.x; i < n; i += (int64_t)gridDim.x * BT) {
        const int t = truth[i], p = pred[i];
        if (t == ignore) continue;
        if (t >= C || p >= C) {
            atomicOr(err, 1);
            continue;
        }
        atomicAdd(&hist[t * C + p], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += BT)
        if (hist[i]) atomicAdd(&counts[i], (unsigned long long)hist[i]);
}

}  // namespace

extern "C" {

int ivln_seg_ce_f32(const float* scores, const uint8_t* labels, const float* class_w, int N, int C, int h, int w, int s,
                    int ignore_label, double scale, float* loss, float* dscores, double* ws, int64_t ws_doubles, int* err,
                    void* stream) {
    if (!scores || !labels || !loss || !ws || !err) return IVLN_E_INVALID;
    if (N <= 0 || C < 2 || C > 64 || h <= 0 || w <= 0 || s <= 0 || ignore_label < -1 || ignore_label > 255) return IVLN_E_INVALID;
    if (ws_doubles < IVLN_SEG_CE_WS_DOUBLES || ((uintptr_t)ws & 7)) return IVLN_E_INVALID;
    if ((int64_t)h * w > INT32_MAX / 64 || (int64_t)h * s > INT32_MAX || (int64_t)w * s > INT32_MAX) return IVLN_E_UNSUPPORTED;
    const int hw = h * w;
    const bool vec = (hw & 3) == 0 && (((uintptr_t)scores | (uintptr_t)dscores) & 15) == 0;
    const int64_t units = (int64_t)N * (vec ? hw / 4 : hw);
    int64_t blocks = (units + BT - 1) / BT;
    if (blocks > MAX_BLOCKS) blocks = MAX_BLOCKS;
    double* partial = ws + 2;
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(k_seg_ce_partial<4>, dim3((unsigned)blocks), dim3(BT), 0, st, scores, labels, class_w, units, C, h, w,
                           s, ignore_label, partial, err);
    else
        hipLaunchKernelGGL(k_seg_ce_partial<1>, dim3((unsigned)blocks), dim3(BT), 0, st, scores, labels, class_w, units, C, h, w,
                           s, ignore_label, partial, err);
    hipLaunchKernelGGL(k_seg_ce_final, dim3(1), dim3(BT), 0, st, partial, (int)blocks, ws, loss, err);
    if (dscores) {
        if (vec)
            hipLaunchKernelGGL(k_seg_ce_grad<4>, dim3((unsigned)blocks), dim3(BT), 0, st, scores, labels, class_w, units, C, h,
                               w, s, ignore_label, scale, ws, dscores, err);
        else
            hipLaunchKernelGGL(k_seg_ce_grad<1>, dim3((unsigned)blocks), dim3(BT), 0, st, scores, labels, class_w, units, C, h,
                               w, s, ignore_label, scale, ws, dscores, err);
    }
    return LAUNCH_OK();
}

int ivln_seg_confusion_u8(const uint8_t* pred, const uint8_t* truth, int64_t n, int C, int ignore_label, int64_t* counts,
                          int* err, void* stream) {
    if (!pred || !truth || !counts || !err || n <= 0 || C < 1 || C > 64 || ignore_label < -1 || ignore_label > 255)
        return IVLN_E_INVALID;
    int64_t blocks = (n + (int64_t)BT * 16 - 1) / ((int64_t)BT * 16);  // ~16 pixels per lane: the histogram flush amortised
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_seg_confusion, dim3((unsigned)blocks), dim3(BT), 0, (hipStream_t)stream, pred, truth, n, C,
                       ignore_label, reinterpret_cast<unsigned long long*>(counts), err);
    return LAUNCH_OK();
}

}  // extern "C"
