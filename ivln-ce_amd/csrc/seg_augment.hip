// Training-time augmentation and class statistics for fine-tuning RedNet on gfx950 (include/ivln_seg_augment.h):
// scale + crop / pad + flip of (rgb, depth, labels) with one integer geometry, saturation / value jitter and the input
// normalisation as ONE launch, and the per-class pixel counts behind median-frequency weights.  Built with
// -ffp-contract=off (build.py): every float operation rounds where it is written, as the tests' float32 restatement does.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/ivln_hip.h"
#include "../../include/ivln_seg_augment.h"

namespace {

constexpr int BT = 256;  // threads per workgroup, every kernel of this file
constexpr int MAXB = IVLN_SEG_AUGMENT_MAX_B;
constexpr int ONE = IVLN_SEG_AUGMENT_ONE;

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP)

// The validated records of one call, passed by value: they live in the kernel-argument segment, and blockIdx.y (the image)
// indexes them uniformly per workgroup.
struct AugRecords {
    int32_t geom[MAXB][4];  // q, oy, ox, flip
    float photo[MAXB][4];   // ks, kv, dv, 0
};

__device__ __forceinline__ int scaled(int n, int q) { return (int)(((unsigned)n * (unsigned)q + ONE / 2) / ONE); }

// nearest source index of scaled coordinate t (0 <= t < scaled(n, q)): integer division on non-negative values
__device__ __forceinline__ int nearest(int t, int q, int n) {
    const unsigned s = ((unsigned)(2 * t + 1) * ONE) / (2u * (unsigned)q);
    return (int)(s < (unsigned)(n - 1) ? s : (unsigned)(n - 1));
}

// bilinear taps of scaled coordinate t in an rgb axis of n_rgb pixels under an output axis of n pixels
struct Tap {
    int i0, i1;
    float l;
};
__device__ __forceinline__ Tap tap(int t, float r, float s, int n_rgb) {
    const float f = (float)(2 * t + 1) * r - 0.5f;
    float g = (f + 0.5f) * s - 0.5f;
    g = fminf(fmaxf(g, 0.f), (float)(n_rgb - 1));
    Tap o;
    o.i0 = (int)g;
    o.i1 = o.i0 + (o.i0 < n_rgb - 1 ? 1 : 0);
    o.l = g - (float)o.i0;
    return o;
}

// One lane: V consecutive pixels of output row y of image blockIdx.y; all five planes from one coordinate computation.
template <int V>
__global__ __launch_bounds__(BT) void k_seg_augment(const uint8_t* __restrict__ rgb, const float* __restrict__ depth,
                                                    const uint8_t* __restrict__ labels, int h, int w, int H, int W,
                                                    const AugRecords rec, int ignore, float* __restrict__ rgb_n,
                                                    float* __restrict__ depth_n, uint8_t* __restrict__ labels_a) {
    const int upr = W / V;  // units per row
    const int u = blockIdx.x * BT + threadIdx.x;
    if (u >= H * upr) return;
    const int b = blockIdx.y;
    const int y = u / upr, x0 = (u - y * upr) * V;
    const int q = rec.geom[b][0], oy = rec.geom[b][1], ox = rec.geom[b][2], flip = rec.geom[b][3];
    const float ks = rec.photo[b][0], kv = rec.photo[b][1], dv = rec.photo[b][2];
    const int Hs = scaled(H, q), Ws = scaled(W, q);
    const float r = 2048.0f / (float)q, sy = (float)h / (float)H, sx = (float)w / (float)W;
    const float mean[3] = {0.485f, 0.456f, 0.406f};
    const float stdv[3] = {0.229f, 0.224f, 0.225f};
    const float dfill = (0.f - 0.213f) / 0.285f;
    const int64_t HW = (int64_t)H * W;
    const uint8_t* img = rgb + (int64_t)b * h * w * 3;
    const float* dep = depth + b * HW;
    const uint8_t* lab = labels + b * HW;

    const int ty = y + oy;
    const bool in_y = ty >= 0 && ty < Hs;
    int ys = 0;
    Tap ay = {0, 0, 0.f};
    if (in_y) {
        ys = nearest(ty, q, H);
        ay = tap(ty, r, sy, h);
    }
    float o[3][V], od[V];
    uint8_t ol[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const int x = x0 + k;
        const int tx = (flip ? W - 1 - x : x) + ox;
        if (!(in_y && tx >= 0 && tx < Ws)) {
            o[0][k] = o[1][k] = o[2][k] = 0.f;
            od[k] = dfill;
            ol[k] = (uint8_t)ignore;
            continue;
        }
        const int xs = nearest(tx, q, W);
        od[k] = (dep[(int64_t)ys * W + xs] - 0.213f) / 0.285f;
        ol[k] = lab[(int64_t)ys * W + xs];
        const Tap ax = tap(tx, r, sx, w);
        const uint8_t* p00 = img + ((int64_t)ay.i0 * w + ax.i0) * 3;
        const uint8_t* p01 = img + ((int64_t)ay.i0 * w + ax.i1) * 3;
        const uint8_t* p10 = img + ((int64_t)ay.i1 * w + ax.i0) * 3;
        const uint8_t* p11 = img + ((int64_t)ay.i1 * w + ax.i1) * 3;
        float c[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            c[ch] = (1.f - ay.l) * ((1.f - ax.l) * (float)p00[ch] + ax.l * (float)p01[ch]) +
                    ay.l * ((1.f - ax.l) * (float)p10[ch] + ax.l * (float)p11[ch]);
        const float v = fmaxf(c[0], fmaxf(c[1], c[2]));
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float j = fminf(fmaxf(kv * fmaxf(v - ks * (v - c[ch]), 0.f) + dv, 0.f), 255.f);
            o[ch][k] = (j / 255.0f - mean[ch]) / stdv[ch];
        }
    }
    const int64_t at = (int64_t)y * W + x0;
    float* rn = rgb_n + (int64_t)b * 3 * HW + at;
    if constexpr (V == 4) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            *reinterpret_cast<float4*>(rn + ch * HW) = make_float4(o[ch][0], o[ch][1 % V], o[ch][2 % V], o[ch][3 % V]);
        *reinterpret_cast<float4*>(depth_n + b * HW + at) = make_float4(od[0], od[1 % V], od[2 % V], od[3 % V]);
        *reinterpret_cast<uint32_t*>(labels_a + b * HW + at) =
            (uint32_t)ol[0] | ((uint32_t)ol[1 % V] << 8) | ((uint32_t)ol[2 % V] << 16) | ((uint32_t)ol[3 % V] << 24);
    } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) rn[ch * HW] = o[ch][0];
        depth_n[b * HW + at] = od[0];
        labels_a[b * HW + at] = ol[0];
    }
}

// class counts, launch 1: every label looked at once; one that is neither a class nor the ignore label sets the error word
__global__ __launch_bounds__(BT) void k_seg_labels_check(const uint8_t* __restrict__ labels, int64_t n, int C, int ignore,
                                                         int* err) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * BT + threadIdx.x; i < n; i += (int64_t)gridDim.x * BT) {
        const int t = labels[i];
        bad = bad || (t != ignore && t >= C);
    }
    if (bad) atomicOr(err, 1);
}

// class counts, launch 2: workgroup b = image b; a 64-bin histogram in LDS (integer atomics), then lane c adds class c's
// count to pixels[c] and, where the class occurs, the image's counted pixels to present[c].  Nothing while the word is set.
__global__ __launch_bounds__(BT) void k_seg_class_counts(const uint8_t* __restrict__ labels, int64_t hw, int C, int ignore,
                                                         unsigned long long* __restrict__ pixels,
                                                         unsigned long long* __restrict__ present, const int* __restrict__ err) {
    __shared__ unsigned int hist[64];
    if (*err != 0) return;  // (uniform: launch 1 saw every label this launch sees)
    if (threadIdx.x < 64) hist[threadIdx.x] = 0u;
    __syncthreads();
    const uint8_t* lab = labels + (int64_t)blockIdx.x * hw;
    for (int64_t i = threadIdx.x; i < hw; i += BT) {
        const int t = lab[i];
        if (t != ignore && t < C) atomicAdd(&hist[t], 1u);
    }
    __syncthreads();
    if ((int)threadIdx.x < C && hist[threadIdx.x]) {
        unsigned long long total = 0;
        for (int c = 0; c < C; ++c) total += hist[c];
        atomicAdd(&pixels[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
        atomicAdd(&present[threadIdx.x], total);
    }
}

bool record_ok(const int32_t* g, const float* p, int H, int W, int ignore_label) {
    const int q = g[0], oy = g[1], ox = g[2], flip = g[3];
    if (q < ONE / 2 || q > 2 * ONE || (flip != 0 && flip != 1)) return false;
    for (int i = 0; i < 4; ++i)
        if (!std::isfinite(p[i])) return false;
    if (p[0] < 0.f || p[1] < 0.f) return false;
    const int dy = (int)(((int64_t)H * q + ONE / 2) / ONE) - H, dx = (int)(((int64_t)W * q + ONE / 2) / ONE) - W;
    if ((dy < 0 || dx < 0) && ignore_label < 0) return false;  // an outside pixel has no label to take
    if (dy >= 0 ? (oy < 0 || oy > dy) : (oy < dy || oy > 0)) return false;
    if (dx >= 0 ? (ox < 0 || ox > dx) : (ox < dx || ox > 0)) return false;
    return true;
}

}  // namespace

extern "C" {

int ivln_seg_augment_f32(const uint8_t* rgb, const float* depth, const uint8_t* labels, int B, int h, int w, int H, int W,
                         const int32_t* geom, const float* photo, int ignore_label, float* rgb_n, float* depth_n,
                         uint8_t* labels_a, void* stream) {
    if (!rgb || !depth || !labels || !geom || !photo || !rgb_n || !depth_n || !labels_a) return IVLN_E_INVALID;
    const int D = IVLN_SEG_AUGMENT_MAX_DIM;
    if (B < 1 || B > MAXB || h < 1 || w < 1 || H < 1 || W < 1 || h > D || w > D || H > D || W > D || ignore_label < -1 ||
        ignore_label > 255)
        return IVLN_E_INVALID;
    AugRecords rec = {};
    for (int b = 0; b < B; ++b) {
        if (!record_ok(geom + 4 * b, photo + 4 * b, H, W, ignore_label)) return IVLN_E_INVALID;
        for (int i = 0; i < 4; ++i) rec.geom[b][i] = geom[4 * b + i], rec.photo[b][i] = photo[4 * b + i];
    }
    const bool vec = (W & 3) == 0 && (((uintptr_t)rgb_n | (uintptr_t)depth_n) & 15) == 0 && ((uintptr_t)labels_a & 3) == 0;
    const int64_t units = (int64_t)H * (vec ? W / 4 : W);  // <= 2^30
    const dim3 grid((unsigned)((units + BT - 1) / BT), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(k_seg_augment<4>, grid, dim3(BT), 0, st, rgb, depth, labels, h, w, H, W, rec, ignore_label, rgb_n,
                           depth_n, labels_a);
    else
        hipLaunchKernelGGL(k_seg_augment<1>, grid, dim3(BT), 0, st, rgb, depth, labels, h, w, H, W, rec, ignore_label, rgb_n,
                           depth_n, labels_a);
    return LAUNCH_OK();
}

int ivln_seg_class_counts_u8(const uint8_t* labels, int B, int64_t hw, int C, int ignore_label, int64_t* pixels,
                             int64_t* present, int* err, void* stream) {
    if (!labels || !pixels || !present || !err || B < 1 || B > 65535 || hw < 1 || hw > INT32_MAX || C < 1 || C > 64 ||
        ignore_label < -1 || ignore_label > 255)
        return IVLN_E_INVALID;
    const int64_t n = (int64_t)B * hw;
    int64_t blocks = (n + (int64_t)BT * 16 - 1) / ((int64_t)BT * 16);
    if (blocks > 2048) blocks = 2048;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_seg_labels_check, dim3((unsigned)blocks), dim3(BT), 0, st, labels, n, C, ignore_label, err);
    hipLaunchKernelGGL(k_seg_class_counts, dim3((unsigned)B), dim3(BT), 0, st, labels, hw, C, ignore_label,
                       reinterpret_cast<unsigned long long*>(pixels), reinterpret_cast<unsigned long long*>(present), err);
    return LAUNCH_OK();
}

}  // extern "C"
