// Box-world renderer (include/ivln_boxworld.h): depth, labels and colour of a room with axis-aligned boxes, ray-cast from
// the pose by the inverse of the mapper's un-projection.  Every float step is an explicit round-to-nearest operation (and
// the file is built with -ffp-contract=off): `boxworld.render_reference` restates them in numpy float32 and gives the
// same bits.  Min / max are written as compare + select so that both sides pick the same operand among equals.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>

#include "../../include/ivln_boxworld.h"

namespace {

constexpr int kThreads = 256;

struct BwBox {  // 32 bytes
    float lo[3];
    float hi[3];
    int label;
    int pad;
};
struct BwScene {  // 32 + 32 * 32 bytes
    float lo[3];
    float hi[3];
    int n;
    int present;
    BwBox box[IVLN_BW_MAX_BOXES];
};

// rows 0..12: the label colours; row 13: the second colour of the label-0 checker
__constant__ uint8_t kPalette[14][3] = {
    {200, 200, 200}, {230, 25, 75},  {60, 180, 75},  {255, 225, 25}, {0, 130, 200},  {245, 130, 48}, {145, 30, 180},
    {70, 240, 240},  {240, 50, 230}, {210, 245, 60}, {250, 190, 190}, {0, 128, 128}, {170, 110, 40}, {120, 120, 120},
};
// faces -x, +x, -y, +y, -z, +z
__constant__ int kShade[6] = {200, 232, 120, 255, 168, 216};

struct Hit {
    float t;
    int label;
    int face;
};

// The scene pointer and everything read through it are wave-uniform (blockIdx.y picks the row): scalar loads.
__device__ __forceinline__ Hit cast(const BwScene* __restrict__ sc, const float (&o)[3], const float (&d)[3]) {
    Hit h;
    h.t = INFINITY;
    h.label = 0;
    h.face = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (d[a] != 0.0f) {
            const bool pos = d[a] > 0.0f;
            const float t = __fdiv_rn(__fsub_rn(pos ? sc->hi[a] : sc->lo[a], o[a]), d[a]);
            if (t < h.t) {
                h.t = t;
                h.face = 2 * a + (pos ? 1 : 0);
            }
        }
    }
    const int n = sc->n;
    for (int k = 0; k < n; ++k) {
        const BwBox& bx = sc->box[k];
        float tn = -INFINITY, tf = INFINITY;
        int face = 0;
        bool miss = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (d[a] == 0.0f) {
                if (o[a] < bx.lo[a] || o[a] > bx.hi[a]) miss = true;
            } else {
                const float t1 = __fdiv_rn(__fsub_rn(bx.lo[a], o[a]), d[a]);
                const float t2 = __fdiv_rn(__fsub_rn(bx.hi[a], o[a]), d[a]);
                const float ta = t1 < t2 ? t1 : t2;
                const float tb = t1 < t2 ? t2 : t1;
                if (ta > tn) {
                    tn = ta;
                    face = 2 * a + (d[a] < 0.0f ? 1 : 0);
                }
                if (tb < tf) tf = tb;
            }
        }
        if (!miss && tn > 0.0f && tn <= tf && tn < h.t) {
            h.t = tn;
            h.label = bx.label;
            h.face = face;
        }
    }
    return h;
}

__device__ __forceinline__ int palette_row(const Hit& h, const float (&o)[3], const float (&d)[3]) {
    if (h.label != 0) return h.label;
    const int a = h.face >> 1;
    const float p0 = __fadd_rn(o[0], __fmul_rn(h.t, d[0]));
    const float p1 = __fadd_rn(o[1], __fmul_rn(h.t, d[1]));
    const float p2 = __fadd_rn(o[2], __fmul_rn(h.t, d[2]));
    const float pi = a == 0 ? p1 : p0, pj = a == 2 ? p1 : p2;  // the two in-plane axes i < j
    const float s = __fadd_rn(floorf(__fdiv_rn(pi, 0.5f)), floorf(__fdiv_rn(pj, 0.5f)));
    const float odd = __fsub_rn(s, __fmul_rn(2.0f, floorf(__fmul_rn(s, 0.5f))));
    return odd != 0.0f ? 13 : 0;
}

// One lane: four horizontally adjacent pixels of row blockIdx.y's frame.  RGB false: depth + labels; true: colour.
template <bool RGB>
__global__ __launch_bounds__(kThreads) void k_bw_render(const BwScene* __restrict__ table, int n_scenes,
                                                        const int32_t* __restrict__ scene_index,
                                                        const float* __restrict__ cam_pos, const float* __restrict__ sincos,
                                                        int H, int W, float cx, float cy, float fx, float fy, float dmin,
                                                        float drange, float* __restrict__ depth, uint8_t* __restrict__ labels,
                                                        uint8_t* __restrict__ rgb, int* __restrict__ status) {
    const int b = blockIdx.y;
    const int Wq = (W + 3) >> 2;
    const int q = blockIdx.x * kThreads + threadIdx.x;
    const int idx = scene_index[b];
    const bool ok = idx >= 0 && idx < n_scenes && table[idx < 0 || idx >= n_scenes ? 0 : idx].present != 0;
    if (!ok && blockIdx.x == 0 && threadIdx.x == 0) *status = IVLN_E_INVALID;
    if (q >= H * Wq) return;
    const int v = q / Wq, u0 = (q - v * Wq) << 2;
    const int nu = min(4, W - u0);
    const size_t off = ((size_t)b * H + v) * (size_t)W + u0;
    float dep[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    uint8_t lab[4] = {0, 0, 0, 0};
    uint8_t col[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (ok) {
        const BwScene* __restrict__ sc = table + idx;
        const float o[3] = {cam_pos[3 * b + 0], cam_pos[3 * b + 1], cam_pos[3 * b + 2]};
        const float s = sincos[2 * b + 0], c = sincos[2 * b + 1];
        const float ys = __fdiv_rn(__fsub_rn(__fadd_rn((float)v, 0.5f), cy), fy);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < nu) {
                const float xs = __fdiv_rn(__fsub_rn(__fadd_rn((float)(u0 + i), 0.5f), cx), fx);
                const float d[3] = {__fsub_rn(__fmul_rn(xs, c), s), -ys, __fsub_rn(-__fmul_rn(xs, s), c)};
                const Hit h = cast(sc, o, d);
                if constexpr (RGB) {
                    const int row = palette_row(h, o, d);
                    const int sh = kShade[h.face];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) col[3 * i + ch] = (uint8_t)(((int)kPalette[row][ch] * sh) >> 8);
                } else {
                    float z = __fdiv_rn(__fsub_rn(h.t, dmin), drange);
                    z = z > 0.0f ? z : 0.0f;
                    z = z < 1.0f ? z : 1.0f;
                    dep[i] = z;
                    lab[i] = (uint8_t)h.label;
                }
            }
        }
    }
    if constexpr (RGB) {
        uint8_t* p = rgb + 3 * off;
        if (nu == 4 && ((uintptr_t)p & 3) == 0) {
            uint32_t w[3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
                w[k] = (uint32_t)col[4 * k] | ((uint32_t)col[4 * k + 1] << 8) | ((uint32_t)col[4 * k + 2] << 16) |
                       ((uint32_t)col[4 * k + 3] << 24);
            uint32_t* p32 = reinterpret_cast<uint32_t*>(p);
            p32[0] = w[0];
            p32[1] = w[1];
            p32[2] = w[2];
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k)
                if (k < 3 * nu) p[k] = col[k];
        }
    } else {
        float* pd = depth + off;
        uint8_t* pl = labels + off;
        if (nu == 4 && ((uintptr_t)pd & 15) == 0) {
            *reinterpret_cast<float4*>(pd) = make_float4(dep[0], dep[1], dep[2], dep[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nu) pd[k] = dep[k];
        }
        if (nu == 4 && ((uintptr_t)pl & 3) == 0) {
            *reinterpret_cast<uint32_t*>(pl) =
                (uint32_t)lab[0] | ((uint32_t)lab[1] << 8) | ((uint32_t)lab[2] << 16) | ((uint32_t)lab[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nu) pl[k] = lab[k];
        }
    }
}

}  // namespace

struct ivln_boxworld {
    BwScene* table;
    int* status;
    uint8_t* present;  // host-side bookkeeping
    int max_scenes;
    int n_added;
};

extern "C" {

int ivln_boxworld_create(int max_scenes, ivln_boxworld** out) {
    if (!out || max_scenes < 1 || max_scenes > (1 << 16)) return IVLN_E_INVALID;
    ivln_boxworld* bw = new (std::nothrow) ivln_boxworld();
    if (!bw) return IVLN_E_INVALID;
    bw->table = nullptr;
    bw->status = nullptr;
    bw->max_scenes = max_scenes;
    bw->n_added = 0;
    bw->present = new (std::nothrow) uint8_t[max_scenes]();
    bool ok = bw->present != nullptr && hipMalloc(&bw->table, sizeof(BwScene) * (size_t)max_scenes) == hipSuccess &&
              hipMalloc(&bw->status, sizeof(int)) == hipSuccess;
    if (ok)
        ok = hipMemset(bw->table, 0, sizeof(BwScene) * (size_t)max_scenes) == hipSuccess &&
             hipMemset(bw->status, 0, sizeof(int)) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        ivln_boxworld_destroy(bw);
        return IVLN_E_HIP;
    }
    *out = bw;
    return IVLN_OK;
}

int ivln_boxworld_destroy(ivln_boxworld* bw) {
    if (!bw) return IVLN_E_INVALID;
    if (bw->table) (void)hipFree(bw->table);
    if (bw->status) (void)hipFree(bw->status);
    delete[] bw->present;
    delete bw;
    return IVLN_OK;
}

int ivln_boxworld_add_scene(ivln_boxworld* bw, int scene, const float* room, int n, const float* boxes,
                            const uint8_t* labels, void* stream) {
    if (!bw || !room || scene < 0 || scene >= bw->max_scenes || bw->present[scene]) return IVLN_E_INVALID;
    if (n < 0 || n > IVLN_BW_MAX_BOXES || (n > 0 && (!boxes || !labels))) return IVLN_E_INVALID;
    BwScene rec = {};
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(room[a]) || !std::isfinite(room[3 + a]) || !(room[a] < room[3 + a])) return IVLN_E_INVALID;
        rec.lo[a] = room[a];
        rec.hi[a] = room[3 + a];
    }
    for (int k = 0; k < n; ++k) {
        for (int a = 0; a < 3; ++a) {
            const float lo = boxes[6 * k + a], hi = boxes[6 * k + 3 + a];
            if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) return IVLN_E_INVALID;
            rec.box[k].lo[a] = lo;
            rec.box[k].hi[a] = hi;
        }
        if (labels[k] < 1 || labels[k] > 12) return IVLN_E_INVALID;
        rec.box[k].label = labels[k];
    }
    rec.n = n;
    rec.present = 1;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(bw->table + scene, &rec, sizeof(BwScene), hipMemcpyHostToDevice, s) != hipSuccess) return IVLN_E_HIP;
    if (hipStreamSynchronize(s) != hipSuccess) return IVLN_E_HIP;  // (`rec` lives on this stack frame)
    bw->present[scene] = 1;
    bw->n_added += 1;
    return IVLN_OK;
}

int ivln_boxworld_size(ivln_boxworld* bw) { return bw ? bw->n_added : IVLN_E_INVALID; }

int ivln_boxworld_render(ivln_boxworld* bw, const int32_t* scene_index, const float* cam_pos, const float* sincos, int B,
                         int H, int W, float fx, float fy, float dmin, float dmax, float* depth, uint8_t* labels, int Hr,
                         int Wr, float fxr, float fyr, uint8_t* rgb, void* stream) {
    if (!bw || !scene_index || !cam_pos || !sincos || !depth || !labels) return IVLN_E_INVALID;
    if (B < 1 || B > 65535 || H < 1 || W < 1 || H > IVLN_BW_MAX_DIM || W > IVLN_BW_MAX_DIM) return IVLN_E_INVALID;
    if (Hr < 0 || Wr < 0 || Hr > IVLN_BW_MAX_DIM || Wr > IVLN_BW_MAX_DIM || ((Hr == 0) != (Wr == 0))) return IVLN_E_INVALID;
    if (Hr > 0 && !rgb) return IVLN_E_INVALID;
    if (!(fx > 0.0f) || !(fy > 0.0f) || !(dmax > dmin)) return IVLN_E_INVALID;
    if (Hr > 0 && (!(fxr > 0.0f) || !(fyr > 0.0f))) return IVLN_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const float drange = dmax - dmin;
    {
        const int quads = H * ((W + 3) >> 2);
        hipLaunchKernelGGL(k_bw_render<false>, dim3((quads + kThreads - 1) / kThreads, B), dim3(kThreads), 0, s, bw->table,
                           bw->max_scenes, scene_index, cam_pos, sincos, H, W, (float)(W / 2.0), (float)(H / 2.0), fx, fy,
                           dmin, drange, depth, labels, (uint8_t*)nullptr, bw->status);
    }
    if (Hr > 0) {
        const int quads = Hr * ((Wr + 3) >> 2);
        hipLaunchKernelGGL(k_bw_render<true>, dim3((quads + kThreads - 1) / kThreads, B), dim3(kThreads), 0, s, bw->table,
                           bw->max_scenes, scene_index, cam_pos, sincos, Hr, Wr, (float)(Wr / 2.0), (float)(Hr / 2.0), fxr,
                           fyr, dmin, drange, (float*)nullptr, (uint8_t*)nullptr, rgb, bw->status);
    }
    return hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP;
}

int ivln_boxworld_status(ivln_boxworld* bw, int clear, void* stream) {
    if (!bw) return IVLN_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    int code = 0;
    if (hipMemcpyAsync(&code, bw->status, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess) return IVLN_E_HIP;
    if (hipStreamSynchronize(s) != hipSuccess) return IVLN_E_HIP;
    if (clear && code != 0) {
        if (hipMemsetAsync(bw->status, 0, sizeof(int), s) != hipSuccess) return IVLN_E_HIP;
    }
    return code;
}

}  // extern "C"
