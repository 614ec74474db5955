// Egocentric semantic mapper for gfx950 - bit-exact with the reference's MappingModule
// (ivlnce_baselines/common/mapping_module/mapper.py:904-944) on identical depth/label inputs.
//
// The reference runs ~150 tiny torch ops per step, two torch_scatter.scatter_max calls, sorts the
// cloud by a (colliding) cell hash and relies on last-writer-wins index_put_.  Here one step is 6
// launches and the cloud is an UNORDERED bag: every decision the reference takes by position in its
// sorted cloud is taken by a `rank` carried with each point (= its key in the last keep-highest), so
// append order does not matter and no sort is needed:
//   keep-highest arg-max  -> ONE 64-bit atomicMax of (orderable height, ~index | ~rank) in a dense per-key
//                            table: highest point, and among equal heights the first in cloud order
//   last-writer-wins map  -> atomicMax of (rank<<8 | label) per 10 cm map cell
// HBM traffic (the thing to minimise - this is byte work): the local-cloud kernels re-derive
// a pixel's point from its 4-byte depth instead of passing 16-byte records between them; the world cloud is
// read twice (keep-highest, select) and written once per step, its two buffers swap by a device-side index
// (no copy-back), and the bounding box of the surviving OLD cloud comes from per-env boxes the previous
// select left behind (no third pass).  Round 1's 7-launch version moved 54 MB per 4-env step; see
// profiles/r02_rollout_pmc_traffic.json for this one.
// Float recipe (verified against goldens through oracle/mapper_ref.c): camera->world is an fmaf
// chain over k=0..3, the ego rotation is un-fused (a*x + b*y) + c*z, divisions are IEEE, rounding is
// half-to-even.  Compile with -ffp-contract=off; every op below is an explicit __f*_rn.
//
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <stdlib.h>
#include <new>
#include "../../include/ivln_hip.h"
#include "../../include/ivln_known_lib.h"
#include "../../include/ivln_map_build.h"
#include "../../include/ivln_map_seed.h"
#include "../../include/ivln_mapper_debug.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPPT = 4;                       // pixels per thread in the local-cloud kernels
constexpr uint32_t kLocalRankBit = 1u << 31;  // rank of a point that entered the cloud this step = bit | local key
constexpr int kFrameEnvs = 64;                // envs a workgroup derives camera transforms for (B_max <= 64)

struct Scalars {       // device-side scalars of one mapper
    int mmL[4];        // local cloud: rmin, cmin, rmax, cmax   (published by k_local_argmax)
    int mmW[4];        // world cloud                           (published by k_world_max)
    int mmWold[4];     // surviving OLD world points            (published by k_local_argmax from the per-env boxes)
    unsigned cnt[2];   // points in world buffer 0 / 1
    unsigned cnt_old;  // snapshot of cnt[cur] before this step's appends
    int cur;           // index of the source buffer (the other one receives this step's survivors)
    int n_bbox;        // blocks of per-env bounding-box partials written by the last k_world_select (0: none)
    int n_bbox_envs;   // envs per block in those partials (the batch size of that step)
    int err;           // sticky IVLN_E_*
};

struct Pt {  // 16-byte world point
    float x, y, z;
    uint32_t meta;  // batch << 8 | label
};

__device__ __forceinline__ uint32_t ord_f32(float h) {
    h = __fadd_rn(h, 0.0f);  // -0 -> +0 so that -0 == +0 ties like the reference's `>` compare
    uint32_t u = __float_as_uint(h);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ int cell_index(float v, float half_res) {
    return (int)rintf(__fdiv_rn(v, half_res));  // mapper.py:464 (v / (res/2)).round().long()
}

// {rmin,cmin,rmax,cmax} of a block's threads -> dst4 (wave shuffles + LDS; no atomics: the first version issued 4
// same-address atomics per wave, ~16k serialised L2 atomics = 100-146 us for what is a ~5 us kernel)
__device__ __forceinline__ void block_minmax_store(int rmin, int cmin, int rmax, int cmax, int* __restrict__ dst4) {
    __shared__ int sh[4][4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        rmin = min(rmin, __shfl_xor(rmin, o));
        cmin = min(cmin, __shfl_xor(cmin, o));
        rmax = max(rmax, __shfl_xor(rmax, o));
        cmax = max(cmax, __shfl_xor(cmax, o));
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh[w][0] = rmin; sh[w][1] = cmin; sh[w][2] = rmax; sh[w][3] = cmax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        dst4[0] = min(min(sh[0][0], sh[1][0]), min(sh[2][0], sh[3][0]));
        dst4[1] = min(min(sh[0][1], sh[1][1]), min(sh[2][1], sh[3][1]));
        dst4[2] = max(max(sh[0][2], sh[1][2]), max(sh[2][2], sh[3][2]));
        dst4[3] = max(max(sh[0][3], sh[1][3]), max(sh[2][3], sh[3][3]));
    }
    __syncthreads();
}

// Fold n partial boxes (and an optional extra box) into mm4 (LDS of the calling block); block 0 also publishes.
__device__ __forceinline__ void block_minmax_fold(const int* __restrict__ partials, int n, const int* extra4, int* mm4,
                                                  int* __restrict__ publish) {
    __shared__ int sh[4][4];
    int rmin = INT32_MAX, cmin = INT32_MAX, rmax = INT32_MIN, cmax = INT32_MIN;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const int4 v = *reinterpret_cast<const int4*>(partials + 4 * i);
        rmin = min(rmin, v.x); cmin = min(cmin, v.y); rmax = max(rmax, v.z); cmax = max(cmax, v.w);
    }
    if (extra4 && threadIdx.x == 0) {
        rmin = min(rmin, extra4[0]); cmin = min(cmin, extra4[1]); rmax = max(rmax, extra4[2]); cmax = max(cmax, extra4[3]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        rmin = min(rmin, __shfl_xor(rmin, o));
        cmin = min(cmin, __shfl_xor(cmin, o));
        rmax = max(rmax, __shfl_xor(rmax, o));
        cmax = max(cmax, __shfl_xor(cmax, o));
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh[w][0] = rmin; sh[w][1] = cmin; sh[w][2] = rmax; sh[w][3] = cmax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        mm4[0] = min(min(sh[0][0], sh[1][0]), min(sh[2][0], sh[3][0]));
        mm4[1] = min(min(sh[0][1], sh[1][1]), min(sh[2][1], sh[3][1]));
        mm4[2] = max(max(sh[0][2], sh[1][2]), max(sh[2][2], sh[3][2]));
        mm4[3] = max(max(sh[0][3], sh[1][3]), max(sh[2][3], sh[3][3]));
        if (publish && blockIdx.x == 0) {
            publish[0] = mm4[0]; publish[1] = mm4[1]; publish[2] = mm4[2]; publish[3] = mm4[3];
        }
    }
    __syncthreads();
}

// Block-aggregated append: ONE atomicAdd per block call (wave ballots + a 4-entry LDS prefix);
// returns the slot for threads with pred, 0xFFFFFFFF otherwise / when full.  Every thread of the block
// must call it.  (Per-wave atomics on the single counter serialised ~4k same-address atomics: 59 us.)
__device__ __forceinline__ unsigned wave_append(bool pred, unsigned* counter, unsigned capacity, int* err) {
    __shared__ unsigned wcnt[4];
    __shared__ unsigned bbase;
    const unsigned long long mask = __ballot(pred);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wcnt[w] = (unsigned)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned total = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        bbase = total ? atomicAdd(counter, total) : 0u;
    }
    __syncthreads();
    unsigned off = bbase;
    for (int i = 0; i < w; ++i) off += wcnt[i];
    const unsigned slot = off + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
    __syncthreads();  // wcnt / bbase are reused by the next call
    if (!pred) return 0xFFFFFFFFu;
    if (slot >= capacity) {
        *err = IVLN_E_CAPACITY;
        return 0xFFFFFFFFu;
    }
    return slot;
}

__device__ __forceinline__ int64_t make_key(int b, int r, int c, const int* mm) {
    int64_t R = (int64_t)mm[2] - mm[0], C = (int64_t)mm[3] - mm[1];
    return (int64_t)b * (R * C) + (int64_t)(r - mm[0]) * C + (int64_t)(c - mm[1]);  // mapper.py:469
}

// Slot of a key in the dense arg-max table.  The KEY (above) is the reference's flattened cell number - with its
// multipliers rows.max() / cols.max() (not max + 1: cell (r, C) and cell (r + 1, 0) share a key, quirk Q2) - and it is
// the rank that orders the cloud and breaks ties: it stays what it was.  The table SLOT only has to be a bijection of
// the key, and slot = key makes every probe of a point whose neighbours in the cloud differ in r a separate 64-byte
// line (consecutive points come from consecutive pixels: a wall runs along r as often as along c).  Slots therefore
// tile the key plane (q = key / C, kc = key % C) 4 x 4 = 16 slots = 128 bytes, so that neighbours in either direction
// share lines (counted HBM bytes of the mapper: profiles/README.md, round 3).  -1: outside the table
// (IVLN_E_KEYSPACE; keys are ranks as well and must fit the same 31 bits).
__device__ __forceinline__ int64_t table_slot(int b, int r, int c, const int* mm, int64_t table_cells) {
    const int64_t key = make_key(b, r, c, mm);
    if (key < 0 || key >= table_cells) return -1;
    const int64_t C = (int64_t)mm[3] - mm[1];
    if (C <= 0) return key;  // (one column of cells: every key is a row number already)
    const uint32_t q = (uint32_t)key / (uint32_t)C, kc = (uint32_t)key - q * (uint32_t)C;
    const int64_t Ct = (C + 3) >> 2;
    const int64_t slot = ((((int64_t)(q >> 2)) * Ct + (kc >> 2)) << 4) | ((q & 3) << 2) | (kc & 3);
    return slot < table_cells ? slot : -1;
}

// Unproject + filter one pixel (GenerateSemanticPointCloud.forward, mapper.py:387-425; core.py:137-171).  The three
// local-cloud kernels each RE-DERIVE the point from the depth value (a dozen flops) instead of passing a float4
// record per pixel between them: 4 bytes read per pixel and kernel instead of 16 written + 2 x 16 read.
struct Cam {
    const float* depth; const float* T; const float* pose; const float* xs; const float* ys;
    int B, H, W;
    float half_res;
};
__device__ __forceinline__ bool unproject(const Cam& cm, int64_t pix, float (&w)[3], int& b, int& r, int& c) {
    const int u = (int)(pix % cm.W);
    const int v = (int)((pix / cm.W) % cm.H);
    b = (int)(pix / ((int64_t)cm.W * cm.H));
    const float d = cm.depth[pix];
    if (!(d > 0.01f && d < 0.99f)) return false;  // mapper.py:416-418
    const float z = __fmul_rn(d, 10.0f);          // mapper.py:381-384
    const float x = __fmul_rn(z, cm.xs[u]);       // core.py:137-139
    const float y = __fmul_rn(z, cm.ys[v]);
    const float* t = cm.T + 16 * b;
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // core.py:171 bmm == fma chain over k
        float acc = __fmul_rn(t[4 * k + 0], x);
        acc = __fmaf_rn(t[4 * k + 1], y, acc);
        acc = __fmaf_rn(t[4 * k + 2], z, acc);
        acc = __fmaf_rn(t[4 * k + 3], 1.0f, acc);
        w[k] = __fsub_rn(acc, 0.0f);  // world_shift_origin == 0 (core.py:214)
    }
    const float h = cm.pose[3 * b + 1];
    if (!(w[1] > __fsub_rn(h, 1.0f) && w[1] < __fadd_rn(h, 0.5f))) return false;  // mapper.py:420-424
    r = cell_index(w[2], cm.half_res);
    c = cell_index(w[0], cm.half_res);
    return true;
}

// Camera-to-world transform of env b (core.py:20-36 with elevation + pi, mapper.py:135): fp64 sin / cos, rounded to fp32.
__device__ __forceinline__ void frame_T(const float* __restrict__ pose, const double* __restrict__ orient, int b, float* t) {
    const double elev = orient[2 * b + 0] + 3.141592653589793;
    const double head = orient[2 * b + 1];
    const double cx = cos(elev), sx = sin(elev), cy = cos(head), sy = sin(head);
    t[0] = (float)cy;    t[1] = (float)(sx * sy); t[2] = (float)(cx * sy);  t[3] = pose[3 * b + 0];
    t[4] = 0.f;          t[5] = (float)cx;        t[6] = (float)(-sx);      t[7] = pose[3 * b + 1];
    t[8] = (float)(-sy); t[9] = (float)(cy * sx); t[10] = (float)(cy * cx); t[11] = pose[3 * b + 2];
    t[12] = 0.f; t[13] = 0.f; t[14] = 0.f; t[15] = 1.f;
}
// mapper.py:266 rotate_around_y(-origin.heading)
__device__ __forceinline__ void frame_rot(const double* __restrict__ orient, int b, float* r) {
    const double a = -orient[2 * b + 1];
    r[0] = (float)cos(a);    r[1] = 0.f; r[2] = (float)sin(a);
    r[3] = 0.f;              r[4] = 1.f; r[5] = 0.f;
    r[6] = (float)(-sin(a)); r[7] = 0.f; r[8] = (float)cos(a);
}

// ---- A: local min/max of the cell indices; zero the occupancy output.  FRAMES: the step was given (pose,
// orientation) instead of ready transforms - every workgroup derives the B camera transforms it unprojects with into
// LDS (B <= 64 threads, a few fp64 sin / cos each) and workgroup 0 also leaves T and rot in global memory for the
// kernels behind it: the former k_frames launch in front of the step is gone. ----
template <bool FRAMES>
__global__ __launch_bounds__(kThreads) void k_local_minmax(Cam cm, uint8_t* __restrict__ occ, int map_cells,
                                                           int* __restrict__ bmmL, const double* __restrict__ orient,
                                                           float* __restrict__ T_out, float* __restrict__ rot_out) {
    if constexpr (FRAMES) {
        __shared__ float Ts[kFrameEnvs * 16];
        if ((int)threadIdx.x < cm.B) {
            frame_T(cm.pose, orient, threadIdx.x, Ts + 16 * threadIdx.x);
            if (blockIdx.x == 0) {
#pragma unroll
                for (int k = 0; k < 16; ++k) T_out[16 * threadIdx.x + k] = Ts[16 * threadIdx.x + k];
                frame_rot(orient, threadIdx.x, rot_out + 9 * threadIdx.x);
            }
        }
        __syncthreads();
        cm.T = Ts;
    }
    const int64_t total = (int64_t)cm.B * cm.H * cm.W;
    int rmin = INT32_MAX, cmin = INT32_MAX, rmax = INT32_MIN, cmax = INT32_MIN;
    const int64_t nchunks = (total + kThreads * kPPT - 1) / (kThreads * kPPT);
    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {  // (a narrow grid walks several chunks)
#pragma unroll
        for (int i = 0; i < kPPT; ++i) {
            const int64_t pix = (chunk * kPPT + i) * kThreads + threadIdx.x;
            float w[3];
            int b, r, c;
            if (pix < total && unproject(cm, pix, w, b, r, c)) {
                rmin = min(rmin, r); cmin = min(cmin, c); rmax = max(rmax, r); cmax = max(cmax, c);
            }
        }
    }
    block_minmax_store(rmin, cmin, rmax, cmax, bmmL + 4 * blockIdx.x);
    // zero the occupancy output (DenseMap.update_map fill_(0), mapper.py:570)
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < map_cells; i += (int64_t)gridDim.x * kThreads) occ[i] = 0;
}

// ---- B: local arg-max of height per key (scatter_max, mapper.py:471-472).  Block 0 also derives the box of the
// surviving OLD world points from the per-env boxes the last k_world_select left (clear_completed_episode_data,
// mapper.py:310-326: envs with not_done == 0 and rows >= B drop out) - no pass over the old cloud. ----
__global__ __launch_bounds__(kThreads) void k_local_argmax(const Cam cm, Scalars* sc, unsigned long long* __restrict__ tab64,
                                                           int64_t table_cells, const int* __restrict__ bmmL, int n_partials,
                                                           const int* __restrict__ bbox, int bbox_B,
                                                           const uint8_t* __restrict__ not_done) {
    __shared__ int mm[4];
    block_minmax_fold(bmmL, n_partials, nullptr, mm, sc->mmL);
    if (blockIdx.x == 0) {
        const int nb = sc->n_bbox, ne = min(sc->n_bbox_envs, cm.B);  // envs >= B are paused: their points drop out
        int rmin = INT32_MAX, cmin = INT32_MAX, rmax = INT32_MIN, cmax = INT32_MIN;
        for (int i = threadIdx.x; i < nb * ne; i += kThreads) {
            const int blk = i / ne, b = i - blk * ne;
            if (not_done[b] != 0) {
                const int4 v = *reinterpret_cast<const int4*>(bbox + 4 * ((int64_t)blk * bbox_B + b));
                rmin = min(rmin, v.x); cmin = min(cmin, v.y); rmax = max(rmax, v.z); cmax = max(cmax, v.w);
            }
        }
        block_minmax_store(rmin, cmin, rmax, cmax, sc->mmWold);
        if (threadIdx.x == 0) {
            sc->cnt_old = sc->cnt[sc->cur];
            sc->cnt[sc->cur ^ 1] = 0;
        }
    }
    const int64_t total = (int64_t)cm.B * cm.H * cm.W;
    const int64_t nchunks = (total + kThreads * kPPT - 1) / (kThreads * kPPT);
    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
#pragma unroll
        for (int i = 0; i < kPPT; ++i) {
            const int64_t pix = (chunk * kPPT + i) * kThreads + threadIdx.x;
            float w[3];
            int b, r, c;
            if (pix < total && unproject(cm, pix, w, b, r, c)) {
                const int64_t slot = table_slot(b, r, c, mm, table_cells);
                if (slot < 0) {
                    sc->err = IVLN_E_KEYSPACE;
                    continue;
                }
                const unsigned long long packed =
                    ((unsigned long long)ord_f32(w[1]) << 32) | (0xFFFFFFFFull - (unsigned long long)pix);
                atomicMax(&tab64[slot], packed);
            }
        }
    }
}

// ---- C: local survivors -> appended to the world source buffer (mapper.py:444, 844) ----
__global__ __launch_bounds__(kThreads) void k_local_select(const Cam cm, const uint8_t* __restrict__ labels, Scalars* sc,
                                                           unsigned long long* __restrict__ tab64, int64_t table_cells,
                                                           Pt* __restrict__ w0, Pt* __restrict__ w1,
                                                           int64_t* __restrict__ r0, int64_t* __restrict__ r1,
                                                           unsigned capacity, int* __restrict__ bmmA) {
    const int cur = sc->cur;
    Pt* wsrc = cur ? w1 : w0;
    int64_t* rsrc = cur ? r1 : r0;
    const int64_t total = (int64_t)cm.B * cm.H * cm.W;
    int rmin = INT32_MAX, cmin = INT32_MAX, rmax = INT32_MIN, cmax = INT32_MIN;
    const int64_t nchunks = (total + kThreads * kPPT - 1) / (kThreads * kPPT);
    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x)
    for (int i = 0; i < kPPT; ++i) {
        const int64_t pix = (chunk * kPPT + i) * kThreads + threadIdx.x;
        float w[3] = {0.f, 0.f, 0.f};
        int b = 0, r = 0, c = 0;
        int64_t key = 0, tslot = -1;
        bool win = false;
        if (pix < total && unproject(cm, pix, w, b, r, c)) {
            key = make_key(b, r, c, sc->mmL);
            tslot = table_slot(b, r, c, sc->mmL, table_cells);
            if (tslot >= 0) {
                const unsigned long long packed =
                    ((unsigned long long)ord_f32(w[1]) << 32) | (0xFFFFFFFFull - (unsigned long long)pix);
                win = (tab64[tslot] == packed);
            }
        }
        const unsigned slot = wave_append(win, &sc->cnt[cur], capacity, &sc->err);
        if (win) tab64[tslot] = 0ull;  // leave the table clean for the world phase
        if (win && slot != 0xFFFFFFFFu) {
            Pt q;
            q.x = w[0]; q.y = w[1]; q.z = w[2];
            q.meta = ((uint32_t)b << 8) | labels[pix];
            wsrc[slot] = q;
            rsrc[slot] = (int64_t)(kLocalRankBit | (uint32_t)key);
            rmin = min(rmin, r); cmin = min(cmin, c); rmax = max(rmax, r); cmax = max(cmax, c);
        }
    }
    block_minmax_store(rmin, cmin, rmax, cmax, bmmA + 4 * blockIdx.x);
}

// workgroups of a world-cloud kernel that take part: enough for `wpt` points per thread, at most the grid
__device__ __forceinline__ unsigned working_blocks(unsigned n, int wpt) {
    const unsigned per = (unsigned)kThreads * (unsigned)(wpt > 0 ? wpt : 1);
    const unsigned need = (n + per - 1) / per;
    return need < 1u ? 1u : (need < gridDim.x ? need : gridDim.x);
}

__device__ __forceinline__ bool world_alive(const Pt& p, unsigned i, unsigned cnt_old, int B, const uint8_t* not_done) {
    const int b = (int)(p.meta >> 8);
    if (i >= cnt_old) return true;  // appended this step
    return b < B && not_done[b] != 0;
}

// ---- D: world keep-highest in ONE pass: per key the max of (orderable height, ~rank) - highest point, and among
// equal heights the lowest rank = the first in the reference's cloud order (torch_scatter.scatter_max on the CPU keeps
// the first maximum; old world points, ordered by their previous key, precede this step's local ones).  Ranks fit 32
// bits (key < table_cells <= 2^31, bit 31 = entered this step), so one 64-bit atomicMax replaces the former
// max-height pass + first-rank pass. ----
__global__ __launch_bounds__(kThreads) void k_world_max(const Pt* __restrict__ w0, const Pt* __restrict__ w1,
                                                        const int64_t* __restrict__ r0, const int64_t* __restrict__ r1,
                                                        int B, const uint8_t* __restrict__ not_done, float half_res,
                                                        Scalars* sc, unsigned long long* __restrict__ tab64,
                                                        int64_t table_cells, unsigned capacity,
                                                        const int* __restrict__ bmmA, int n_partials, int wpt) {
    __shared__ int mm[4];
    block_minmax_fold(bmmA, n_partials, sc->mmWold, mm, sc->mmW);
    const int cur = sc->cur;
    const Pt* wsrc = cur ? w1 : w0;
    const int64_t* rsrc = cur ? r1 : r0;
    const unsigned n = min(sc->cnt[cur], capacity);
    const unsigned cnt_old = sc->cnt_old;
    const unsigned nbw = working_blocks(n, wpt);  // (a narrow launch grows with the cloud: wpt points per thread)
    if (blockIdx.x >= nbw) return;
    for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < n; i += nbw * kThreads) {
        const Pt p = wsrc[i];
        if (!world_alive(p, i, cnt_old, B, not_done)) continue;
        const int64_t slot = table_slot((int)(p.meta >> 8), cell_index(p.z, half_res), cell_index(p.x, half_res), mm, table_cells);
        if (slot < 0) {
            sc->err = IVLN_E_KEYSPACE;
            continue;
        }
        const unsigned long long packed = ((unsigned long long)ord_f32(p.y) << 32) | (unsigned long long)(~(uint32_t)rsrc[i]);
        atomicMax(&tab64[slot], packed);
    }
}

// Raster one world point into the egocentric maps (mapper.py:884-901, 255-266, 513-531, 569-571).
__device__ __forceinline__ void raster_point(const Pt& p, uint64_t rank, const float* __restrict__ pose,
                                             const float* __restrict__ rot, int rows, int cols, float res,
                                             float half_h, float half_w, uint8_t* __restrict__ occ,
                                             unsigned long long* __restrict__ cell) {
    int b = (int)(p.meta >> 8);
    float h = pose[3 * b + 1];
    if (!(p.y > __fsub_rn(h, 1.25f) && p.y < __fadd_rn(h, 0.75f))) return;
    float x = __fadd_rn(p.x, -pose[3 * b + 0]);
    float y = __fadd_rn(p.y, -pose[3 * b + 1]);
    float z = __fadd_rn(p.z, -pose[3 * b + 2]);
    const float* r = rot + 9 * b;
    float xr = __fadd_rn(__fadd_rn(__fmul_rn(r[0], x), __fmul_rn(r[1], y)), __fmul_rn(r[2], z));
    float zr = __fadd_rn(__fadd_rn(__fmul_rn(r[6], x), __fmul_rn(r[7], y)), __fmul_rn(r[8], z));
    float fr = rintf(__fdiv_rn(__fadd_rn(zr, half_h), res));
    float fc = rintf(__fdiv_rn(__fadd_rn(xr, half_w), res));
    if (!(fr >= 0.f && fr < (float)rows && fc >= 0.f && fc < (float)cols)) return;
    int o = (b * rows + (int)fr) * cols + (int)fc;
    occ[o] = 1;
    uint32_t label = p.meta & 0xFFu;
    if (label != 0) {
        const unsigned long long v = ((unsigned long long)(rank + 1) << 8) | label;
        if (v > __hip_atomic_load(&cell[o], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&cell[o], v);
    }
}

__device__ __forceinline__ void finalize_scalars(Scalars* sc, int swap, unsigned capacity, int n_bbox, int n_bbox_envs) {
    if (swap) {
        const int cur = sc->cur;
        sc->cnt[cur ^ 1] = min(sc->cnt[cur ^ 1], capacity);
        sc->cnt[cur] = 0;
        sc->cur = cur ^ 1;
        sc->n_bbox = n_bbox;
        sc->n_bbox_envs = n_bbox_envs;
    }
    sc->mmL[0] = sc->mmL[1] = sc->mmW[0] = sc->mmW[1] = sc->mmWold[0] = sc->mmWold[1] = INT32_MAX;
    sc->mmL[2] = sc->mmL[3] = sc->mmW[2] = sc->mmW[3] = sc->mmWold[2] = sc->mmWold[3] = INT32_MIN;
    sc->cnt_old = 0;
}

// ---- E: world survivors -> the other buffer + raster + per-env bounding boxes for the next step.
// (Folding F into this kernel - the last workgroup to finish converts the cells - was built and measured in round 3:
//  the release fence every one of the 1024 workgroups then needs in front of its ticket, an L2 write-back each, took
//  the kernel from 48 us to 123 us (69 us on an empty cloud); a launch of its own costs F 4.8 us.  profiles/README.md) ----
constexpr int kBoxEnvs = 64;  // envs whose box a block tracks in LDS (B_max <= 64)
__global__ __launch_bounds__(kThreads) void k_world_select(
    Pt* w0, Pt* w1, int64_t* r0, int64_t* r1, int B, const uint8_t* __restrict__ not_done, float half_res, Scalars* sc, unsigned long long* __restrict__ tab64,
    int64_t table_cells, unsigned capacity, const float* __restrict__ pose, const float* __restrict__ rot, int rows,
    int cols, float res, float half_h, float half_w, uint8_t* __restrict__ occ, unsigned long long* __restrict__ cell,
    int* __restrict__ bbox, int bbox_B, int wpt) {
    __shared__ int box[kBoxEnvs][4];
    for (int i = threadIdx.x; i < B * 4; i += kThreads) box[i >> 2][i & 3] = (i & 2) ? INT32_MIN : INT32_MAX;
    __syncthreads();
    const int cur = sc->cur;
    const Pt* wsrc = cur ? w1 : w0;
    const int64_t* rsrc = cur ? r1 : r0;
    Pt* wdst = cur ? w0 : w1;  // the OTHER buffer
    int64_t* rdst = cur ? r0 : r1;
    const unsigned n = min(sc->cnt[cur], capacity);
    const unsigned cnt_old = sc->cnt_old;
    const unsigned nbw = working_blocks(n, wpt);
    const unsigned iters = blockIdx.x < nbw ? (n + nbw * kThreads - 1) / (nbw * kThreads) : 0;  // (idle blocks leave empty boxes)
    for (unsigned it = 0; it < iters; ++it) {
        const unsigned i = (it * nbw + blockIdx.x) * kThreads + threadIdx.x;
        bool win = false;
        Pt p;
        p.x = p.y = p.z = 0.f;
        p.meta = 0;
        int64_t key = 0, tslot = -1;
        int r = 0, c = 0;
        if (i < n) {
            p = wsrc[i];
            if (world_alive(p, i, cnt_old, B, not_done)) {
                r = cell_index(p.z, half_res);
                c = cell_index(p.x, half_res);
                key = make_key((int)(p.meta >> 8), r, c, sc->mmW);
                tslot = table_slot((int)(p.meta >> 8), r, c, sc->mmW, table_cells);
                if (tslot >= 0) {
                    const unsigned long long packed =
                        ((unsigned long long)ord_f32(p.y) << 32) | (unsigned long long)(~(uint32_t)rsrc[i]);
                    win = (tab64[tslot] == packed);
                }
            }
        }
        const unsigned slot = wave_append(win, &sc->cnt[cur ^ 1], capacity, &sc->err);
        if (win) {
            tab64[tslot] = 0ull;
            if (slot != 0xFFFFFFFFu) {
                wdst[slot] = p;
                rdst[slot] = key;
                const int b = (int)(p.meta >> 8);
                if (b < B) {  // filtered LDS atomics: a box is touched a handful of times per block
                    if (r < box[b][0]) atomicMin(&box[b][0], r);
                    if (c < box[b][1]) atomicMin(&box[b][1], c);
                    if (r > box[b][2]) atomicMax(&box[b][2], r);
                    if (c > box[b][3]) atomicMax(&box[b][3], c);
                }
            }
            raster_point(p, (uint64_t)key, pose, rot, rows, cols, res, half_h, half_w, occ, cell);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < B * 4; i += kThreads) bbox[(int64_t)blockIdx.x * bbox_B * 4 + i] = box[i >> 2][i & 3];
}

// ---- F: semantic map from the per-cell winners; swap the buffers (a device-side index: the launch sequence has
// fixed pointers and can be captured in a hipGraph; the former copy of the survivors back into the source buffer -
// 2 x 24 bytes per world point and step - is gone); reset the scalars ----
__global__ __launch_bounds__(kThreads) void k_finalize(unsigned long long* __restrict__ cell, uint8_t* __restrict__ sem,
                                                       int map_cells, Scalars* sc, int swap, unsigned capacity,
                                                       int n_bbox, int n_bbox_envs) {
    int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < map_cells) {
        unsigned long long v = cell[i];
        sem[i] = (uint8_t)(v & 0xFFull);
        cell[i] = 0ull;
    }
    if (i == 0) finalize_scalars(sc, swap, capacity, n_bbox, n_bbox_envs);
}

// ---- known-map mode ----
__global__ __launch_bounds__(kThreads) void k_known_clear(Pt* w0, Pt* w1, int64_t* r0, int64_t* r1, int B,
                                                          const uint8_t* __restrict__ not_done, Scalars* sc,
                                                          unsigned capacity) {
    const int cur = sc->cur;
    const Pt* wsrc = cur ? w1 : w0;
    const int64_t* rsrc = cur ? r1 : r0;
    Pt* wdst = cur ? w0 : w1;
    int64_t* rdst = cur ? r0 : r1;
    unsigned n = min(sc->cnt[cur], capacity);
    unsigned iters = (n + gridDim.x * kThreads - 1) / (gridDim.x * kThreads);
    for (unsigned it = 0; it < iters; ++it) {
        unsigned i = (it * gridDim.x + blockIdx.x) * kThreads + threadIdx.x;
        bool keep = false;
        Pt p;
        p.x = p.y = p.z = 0.f;
        p.meta = 0;
        if (i < n) {
            p = wsrc[i];
            int b = (int)(p.meta >> 8);
            keep = b < B && not_done[b] != 0;
        }
        unsigned slot = wave_append(keep, &sc->cnt[cur ^ 1], capacity, &sc->err);
        if (keep && slot != 0xFFFFFFFFu) {
            wdst[slot] = p;
            rdst[slot] = rsrc[i];
        }
    }
}

__global__ void k_swap_counts(Scalars* sc, unsigned capacity) {
    const int cur = sc->cur;
    sc->cnt[cur ^ 1] = min(sc->cnt[cur ^ 1], capacity);
    sc->cnt[cur] = 0;
    sc->cur = cur ^ 1;
}

__global__ __launch_bounds__(kThreads) void k_known_load(const float* __restrict__ xyz,
                                                         const uint8_t* __restrict__ semv, int64_t n, int b,
                                                         int64_t rank_base, Scalars* sc, Pt* w0, Pt* w1, int64_t* r0,
                                                         int64_t* r1, unsigned capacity) {
    // sequential ranks keep the file order (mapper.py:283-294: order of the npz arrays)
    const int cur = sc->cur;
    Pt* wsrc = cur ? w1 : w0;
    int64_t* rsrc = cur ? r1 : r0;
    unsigned start = sc->cnt[cur];  // same value for every block: counts are bumped by k_known_commit
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        uint64_t slot = (uint64_t)start + (uint64_t)i;
        if (slot >= capacity) {
            sc->err = IVLN_E_CAPACITY;
            continue;
        }
        Pt q;
        q.x = xyz[3 * i]; q.y = xyz[3 * i + 1]; q.z = xyz[3 * i + 2];
        q.meta = ((uint32_t)b << 8) | semv[i];
        wsrc[slot] = q;
        rsrc[slot] = rank_base + i;
    }
}

__global__ void k_known_commit(Scalars* sc, int64_t n, unsigned capacity) {
    uint64_t v = (uint64_t)sc->cnt[sc->cur] + (uint64_t)n;
    sc->cnt[sc->cur] = (unsigned)(v > capacity ? capacity : v);
}

__global__ __launch_bounds__(kThreads) void k_known_raster(const Pt* w0, const Pt* w1, const int64_t* r0, const int64_t* r1,
                                                           Scalars* sc, const float* __restrict__ pose,
                                                           const float* __restrict__ rot, int B, int rows,
                                                           int cols, float res, float half_h, float half_w,
                                                           uint8_t* __restrict__ occ,
                                                           unsigned long long* __restrict__ cell) {
    const int cur = sc->cur;
    const Pt* wsrc = cur ? w1 : w0;
    const int64_t* rsrc = cur ? r1 : r0;
    unsigned n = sc->cnt[cur];  // clamped by k_known_commit / k_swap_counts
    for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        Pt p = wsrc[i];
        if ((int)(p.meta >> 8) >= B) continue;
        raster_point(p, (uint64_t)rsrc[i], pose, rot, rows, cols, res, half_h, half_w, occ, cell);
    }
}

__global__ void k_zero_u8(uint8_t* p, int n) {
    int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) p[i] = 0;
}

__global__ void k_frames(const float* __restrict__ pose, const double* __restrict__ orient, int B,
                         float* __restrict__ T, float* __restrict__ rot) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    frame_T(pose, orient, b, T + 16 * b);
    frame_rot(orient, b, rot + 9 * b);
}

// ---- known-map mode over a scene library (include/ivln_known_lib.h): the cloud of a row is always one whole file, so
// the device holds every scene once and a row holds the INDEX of its scene; nothing is copied per step or per reset and
// no launch takes a host-side count ----
struct KScene {  // 16-byte table entry, written by k_known_pack
    const Pt* rec;  // records (x, y, z, label) in file order
    int n;
    int present;
};
constexpr int kKnownBlocks = 256;  // workgroups per row of the library raster (grid-stride over the scene)

__global__ __launch_bounds__(kThreads) void k_known_pack(const float* __restrict__ xyz, const uint8_t* __restrict__ semv,
                                                         int n, Pt* __restrict__ rec, KScene* entry) {
    for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < (unsigned)n; i += gridDim.x * kThreads) {
        Pt q;
        q.x = xyz[3 * (size_t)i]; q.y = xyz[3 * (size_t)i + 1]; q.z = xyz[3 * (size_t)i + 2];
        q.meta = semv[i];
        rec[i] = q;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // (read by launches BEHIND this one on the stream)
        entry->rec = rec;
        entry->n = n;
        entry->present = 1;
    }
}

__device__ __forceinline__ bool known_scene_ok(int c, const KScene* __restrict__ table, int n_scenes) {
    return c >= 0 && c < n_scenes && table[c].present != 0;
}

// latch + rotation (workgroup 0, one thread per row of the handle) and the zeroing of the occupancy output (all)
__global__ __launch_bounds__(kThreads) void k_known_latch(const int32_t* __restrict__ scene_id,
                                                          const uint8_t* __restrict__ not_done,
                                                          const double* __restrict__ orient, int B, int B_max,
                                                          int* __restrict__ cur, float* __restrict__ rot,
                                                          const KScene* __restrict__ table, int n_scenes, Scalars* sc,
                                                          uint8_t* __restrict__ occ, int map_cells) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < map_cells) occ[i] = 0;
    if (blockIdx.x == 0 && (int)threadIdx.x < B_max) {
        const int b = threadIdx.x;
        int c = -1;  // a row at or above the batch size is cleared (mapper.py:315-318)
        if (b < B) {
            c = not_done[b] == 0 ? scene_id[b] : cur[b];  // cleared and reloaded in the same step (mapper.py:851-881)
            frame_rot(orient, b, rot + 9 * b);
        }
        cur[b] = c;
        if (c != -1 && !known_scene_ok(c, table, n_scenes)) sc->err = IVLN_E_INVALID;
    }
}

__global__ __launch_bounds__(kThreads) void k_known_lib_raster(const int* __restrict__ cur, const KScene* __restrict__ table,
                                                               int n_scenes, const float* __restrict__ pose,
                                                               const float* __restrict__ rot, int rows, int cols, float res,
                                                               float half_h, float half_w, uint8_t* __restrict__ occ,
                                                               unsigned long long* __restrict__ cell) {
    const int b = blockIdx.y;  // wave-uniform: the row's latch, table entry, pose and rotation are scalar loads
    const int c = cur[b];
    if (!known_scene_ok(c, table, n_scenes)) return;  // -1: never reset; anything else was reported by k_known_latch
    // (16-byte aligned: ivln_known_lib_add.  A pointer read from memory is generic to the compiler; the records are global
    //  memory, and saying so makes the load a global one instead of a flat one)
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) u32x4* GlobalRec;
    const GlobalRec rec = (GlobalRec)(uintptr_t)table[c].rec;
    const unsigned n = (unsigned)table[c].n;  // < 2^31: i + stride cannot wrap
    for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const u32x4 v = rec[i];  // one 16-byte load per point
        Pt p;
        p.x = __uint_as_float(v.x); p.y = __uint_as_float(v.y); p.z = __uint_as_float(v.z);
        p.meta = ((uint32_t)b << 8) | (v.w & 0xFFu);
        raster_point(p, (uint64_t)i, pose, rot, rows, cols, res, half_h, half_w, occ, cell);
    }
}

__global__ void k_known_count(const int* __restrict__ cur, const KScene* __restrict__ table, int n_scenes, int B,
                              long long* __restrict__ out) {
    long long s = 0;
    for (int b = 0; b < B; ++b) {
        const int c = cur[b];
        if (known_scene_ok(c, table, n_scenes)) s += table[c].n;
    }
    *out = s;
}

// ---- known-map builder (include/ivln_map_build.h): env b's points in ascending rank, compacted on the device.
// Between complete steps rank == key of the last keep-highest: unique, < table_cells, and tab64 is all zero.  So env b's
// points mark slot (key - lowest key of b) of tab64 with (index in the cloud + 1), an exclusive scan of "slot is marked"
// over the window [lowest, highest] is each point's place in the output, and the scatter clears the marks it consumes.
// The scan is hierarchical over tiles of kThreads entries with one LAUNCH per level and direction (count up, scan the top
// tile, scan down, scatter): a workgroup only ever reads what an earlier launch wrote and never waits on another one.
// Everything is bounds-checked against the cloud size, the window and max_n, whatever the table holds. ----
constexpr int kStatBlocks = 128;  // workgroups (and host-summed partials per env) of k_env_stats

// per block and env: {count, lowest rank, highest rank} -> part[(block * B_max + b) * 3]; the host folds the blocks
__global__ __launch_bounds__(kThreads) void k_env_stats(const Pt* __restrict__ w0, const Pt* __restrict__ w1,
                                                        const int64_t* __restrict__ r0, const int64_t* __restrict__ r1,
                                                        const Scalars* __restrict__ sc, unsigned capacity, int B_max,
                                                        unsigned* __restrict__ part) {
    __shared__ unsigned st[kBoxEnvs][3];
    for (int i = threadIdx.x; i < B_max; i += kThreads) {
        st[i][0] = 0u; st[i][1] = 0xFFFFFFFFu; st[i][2] = 0u;
    }
    __syncthreads();
    const int cur = sc->cur & 1;
    const Pt* wsrc = cur ? w1 : w0;
    const int64_t* rsrc = cur ? r1 : r0;
    const unsigned n = min(sc->cnt[cur], capacity);
    for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const unsigned b = wsrc[i].meta >> 8;
        if (b >= (unsigned)B_max) continue;
        const int64_t r = rsrc[i];
        const unsigned k = (r < 0 || r > 0xFFFFFFFFll) ? 0xFFFFFFFFu : (unsigned)r;  // (not a key: the host refuses it)
        atomicAdd(&st[b][0], 1u);  // LDS integer atomics: the result does not depend on their order
        if (k < st[b][1]) atomicMin(&st[b][1], k);
        if (k > st[b][2]) atomicMax(&st[b][2], k);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < B_max * 3; i += kThreads) part[(size_t)blockIdx.x * B_max * 3 + i] = st[i / 3][i % 3];
}

__global__ __launch_bounds__(kThreads) void k_env_mark(const Pt* __restrict__ w0, const Pt* __restrict__ w1,
                                                       const int64_t* __restrict__ r0, const int64_t* __restrict__ r1,
                                                       const Scalars* __restrict__ sc, unsigned capacity, unsigned b,
                                                       unsigned kmin, unsigned window,
                                                       unsigned long long* __restrict__ tab64) {
    const int cur = sc->cur & 1;
    const Pt* wsrc = cur ? w1 : w0;
    const int64_t* rsrc = cur ? r1 : r0;
    const unsigned n = min(sc->cnt[cur], capacity);
    for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        if ((wsrc[i].meta >> 8) != b) continue;
        const int64_t off = rsrc[i] - (int64_t)kmin;
        if (off < 0 || off >= (int64_t)window) continue;
        tab64[off] = (unsigned long long)i + 1ull;  // unique keys: one writer per slot
    }
}

// Exclusive scan of v over the block's threads (wave shuffles + 4 wave sums in LDS); *total = the block's sum.
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned* total) {
    __shared__ unsigned wsum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    unsigned base = 0;
    for (int i = 0; i < w; ++i) base += wsum[i];
    if (total) *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();  // wsum is reused by the next call
    return base + inc - v;
}

// up: dst[j] = sum of tile j (kThreads entries) of the level below - marks of the table (MARKS) or partial sums
template <bool MARKS>
__global__ __launch_bounds__(kThreads) void k_scan_up(const unsigned long long* __restrict__ marks,
                                                      const unsigned* __restrict__ src, unsigned n,
                                                      unsigned* __restrict__ dst) {
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;
    unsigned v = 0;
    if (i < n) v = MARKS ? (marks[i] != 0ull ? 1u : 0u) : src[i];
    unsigned total;
    (void)block_excl_scan(v, &total);
    if (threadIdx.x == 0) dst[blockIdx.x] = total;
}

// top: one workgroup, n <= kThreads entries, exclusive scan in place
__global__ __launch_bounds__(kThreads) void k_scan_top(unsigned* __restrict__ p, unsigned n) {
    const unsigned v = threadIdx.x < n ? p[threadIdx.x] : 0u;
    const unsigned e = block_excl_scan(v, nullptr);
    if (threadIdx.x < n) p[threadIdx.x] = e;
}

// down: tile j of p becomes its exclusive scan + parent[j] (parent: the scanned level above), in place
__global__ __launch_bounds__(kThreads) void k_scan_down(unsigned* __restrict__ p, unsigned n,
                                                        const unsigned* __restrict__ parent) {
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;
    const unsigned v = i < n ? p[i] : 0u;
    const unsigned e = block_excl_scan(v, nullptr) + parent[blockIdx.x];
    if (i < n) p[i] = e;
}

// scatter: marked slot i of the window -> output row base[tile] + (marked slots in front of it in the tile); the mark is
// cleared.  REC: 16-byte library records (x, y, z, label), else xyz f32 (n, 3) + sem u8 (n).
template <bool REC>
__global__ __launch_bounds__(kThreads) void k_env_scatter(unsigned long long* __restrict__ tab64, unsigned window,
                                                          const unsigned* __restrict__ base, const Pt* __restrict__ w0,
                                                          const Pt* __restrict__ w1, const Scalars* __restrict__ sc,
                                                          unsigned capacity, float* __restrict__ xyz,
                                                          uint8_t* __restrict__ sem, Pt* __restrict__ rec, int64_t max_n) {
    const int cur = sc->cur & 1;
    const Pt* wsrc = cur ? w1 : w0;
    const unsigned n = min(sc->cnt[cur], capacity);
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;
    unsigned long long v = 0ull;
    if (i < window) {
        v = tab64[i];
        if (v != 0ull) tab64[i] = 0ull;  // the table is the step kernels' again: all zero
    }
    const unsigned dst = block_excl_scan(v != 0ull ? 1u : 0u, nullptr) + base[blockIdx.x];
    if (v == 0ull || v - 1ull >= (unsigned long long)n || (int64_t)dst >= max_n) return;
    const Pt p = wsrc[v - 1ull];
    if (REC) {
        Pt q = p;
        q.meta = p.meta & 0xFFu;
        rec[dst] = q;
    } else {
        xyz[3 * (size_t)dst] = p.x; xyz[3 * (size_t)dst + 1] = p.y; xyz[3 * (size_t)dst + 2] = p.z;
        sem[dst] = (uint8_t)(p.meta & 0xFFu);
    }
}

__global__ void k_known_entry(KScene* entry, const Pt* rec, int n) {  // (read by launches BEHIND this one on the stream)
    entry->rec = rec;
    entry->n = n;
    entry->present = 1;
}

// ---- seeding an iterative mapper (include/ivln_map_seed.h): rows dropped and pre-built points appended between steps.
// The cloud is a bag ordered by rank, so "behind the cloud, in front of the next step's local points" is a rank band:
// residents carry keys < table_cells, a step's local points carry bit 31, appended points take table_cells + a counter
// of the handle.  What a step reads besides the cloud are the per-env box partials of k_world_select (k_local_argmax folds
// them into mmWold, the box whose extent gives make_key its multipliers): they stay EXACT - emptied for a dropped row, the
// exact cell box of the appended points folded into their row's, nothing else touched. ----
constexpr int kSeedBoxBlocks = 16;  // blocks of box partials a handle gets that has none (never stepped / just reset)

__device__ __forceinline__ void box_store_empty(int* dst4) {
    *reinterpret_cast<int4*>(dst4) = make_int4(INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN);
}

// rows_clear, behind k_known_clear: the partials of every dropped row (keep == 0, or at / beyond B) become empty; the
// buffers swap as in k_swap_counts (thread 0 writes cnt / cur, which no thread of this launch reads)
__global__ __launch_bounds__(kThreads) void k_rows_boxes(const uint8_t* __restrict__ keep, int B, Scalars* sc,
                                                         unsigned capacity, int* __restrict__ bbox, int bbox_B,
                                                         int bbox_blocks) {
    const int nb = min(sc->n_bbox, bbox_blocks), ne = min(sc->n_bbox_envs, bbox_B);
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < nb * ne; i += gridDim.x * kThreads) {
        const int blk = i / ne, e = i - blk * ne;
        if (e >= B || keep[e] == 0) box_store_empty(bbox + 4 * ((int64_t)blk * bbox_B + e));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int cur = sc->cur & 1;
        sc->cnt[cur ^ 1] = min(sc->cnt[cur ^ 1], capacity);
        sc->cnt[cur] = 0;
        sc->cur = cur ^ 1;
    }
}

// append, in front of k_env_append: the partials cover row b.  ONE workgroup (at most 1024 x 64 boxes, usually none): it
// reads the two scalars, fills, and only then rewrites them - the append kernel behind it reads the new ones.
//   no partials (n_bbox == 0):  kSeedBoxBlocks blocks x (b + 1) envs, all empty
//   n_bbox_envs <= b:           columns [n_bbox_envs, b] of every block empty (the row stride is B_max: nothing moves)
__global__ __launch_bounds__(kThreads) void k_seed_boxes(Scalars* sc, int b, int* __restrict__ bbox, int bbox_B,
                                                         int bbox_blocks) {
    int nb = min(sc->n_bbox, bbox_blocks), ne_old = min(sc->n_bbox_envs, bbox_B);
    if (nb <= 0) {
        nb = min(kSeedBoxBlocks, bbox_blocks);
        ne_old = 0;
    }
    const int ne = max(ne_old, b + 1), add = ne - ne_old;
    __syncthreads();  // every thread holds the old scalars
    for (int i = threadIdx.x; i < nb * add; i += kThreads) {
        const int blk = i / add, e = ne_old + (i - blk * add);
        box_store_empty(bbox + 4 * ((int64_t)blk * bbox_B + e));
    }
    if (threadIdx.x == 0) {
        sc->n_bbox = nb;
        sc->n_bbox_envs = ne;
    }
}

// n points -> row b of the source buffer, rank = rank_base + index in the given order.  REC: the library's 16-byte records
// (one global_load_dwordx4 per point), else xyz f32 (n, 3) + sem u8 (n).  One point per thread and pass, one slot claim per
// workgroup and pass (wave_append), the workgroup's cell box in LDS behind filtered integer atomics and folded into ONE
// of row b's partials with four integer atomics at the end: any order of them gives the same box.  (The host checked the
// capacity and the rank band; wave_append's own check still keeps every store inside the buffer.)
template <bool REC>
__global__ __launch_bounds__(kThreads) void k_env_append(const float* __restrict__ xyz, const uint8_t* __restrict__ semv,
                                                         const KScene* __restrict__ entry, int64_t n, int b,
                                                         int64_t rank_base, float half_res, Scalars* sc, Pt* w0, Pt* w1,
                                                         int64_t* r0, int64_t* r1, unsigned capacity,
                                                         int* __restrict__ bbox, int bbox_B, int bbox_blocks) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) u32x4* GlobalRec;
    __shared__ int box[4];
    if (threadIdx.x < 4) box[threadIdx.x] = (threadIdx.x & 2) ? INT32_MIN : INT32_MAX;
    __syncthreads();
    const int cur = sc->cur & 1;
    Pt* wsrc = cur ? w1 : w0;
    int64_t* rsrc = cur ? r1 : r0;
    GlobalRec rec = nullptr;
    if (REC) {
        rec = (GlobalRec)(uintptr_t)entry->rec;
        n = min(n, (int64_t)entry->n);  // (the host's count of the scene; never past the records)
    }
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    const int64_t iters = (n + stride - 1) / stride;
    for (int64_t it = 0; it < iters; ++it) {
        const int64_t i = it * stride + (int64_t)blockIdx.x * kThreads + threadIdx.x;
        const bool in = i < n;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (in) {
            if (REC) {
                v = rec[i];
                v.w &= 0xFFu;
            } else {
                v.x = __float_as_uint(xyz[3 * i]); v.y = __float_as_uint(xyz[3 * i + 1]); v.z = __float_as_uint(xyz[3 * i + 2]);
                v.w = semv[i];
            }
            v.w |= (uint32_t)b << 8;
        }
        const unsigned slot = wave_append(in, &sc->cnt[cur], capacity, &sc->err);
        if (in && slot != 0xFFFFFFFFu) {
            *reinterpret_cast<u32x4*>(wsrc + slot) = v;  // one 16-byte store
            rsrc[slot] = rank_base + i;
            const int r = cell_index(__uint_as_float(v.z), half_res), c = cell_index(__uint_as_float(v.x), half_res);
            if (r < box[0]) atomicMin(&box[0], r);
            if (c < box[1]) atomicMin(&box[1], c);
            if (r > box[2]) atomicMax(&box[2], r);
            if (c > box[3]) atomicMax(&box[3], c);
        }
    }
    __syncthreads();
    const int nb = min(sc->n_bbox, bbox_blocks);  // > 0 and b < n_bbox_envs: k_seed_boxes
    if (threadIdx.x == 0 && nb > 0 && box[0] <= box[2]) {
        int* dst = bbox + 4 * ((int64_t)(blockIdx.x % (unsigned)nb) * bbox_B + b);
        atomicMin(dst + 0, box[0]);
        atomicMin(dst + 1, box[1]);
        atomicMax(dst + 2, box[2]);
        atomicMax(dst + 3, box[3]);
    }
}

// ---- the arg-max table's invariant, observed (include/ivln_mapper_debug.h): non-zero words of a buffer.  Plain loads, a
// wave reduction, one atomicAdd per wave that found any. ----
__global__ __launch_bounds__(kThreads) void k_debug_nonzero(const unsigned long long* __restrict__ p, int64_t n,
                                                            unsigned long long* __restrict__ count) {
    unsigned long long c = 0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) c += p[i] != 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

}  // namespace

struct ivln_known_lib {
    int max_scenes, n_added;
    KScene* table;  // device, fixed for the life of the library
    uint8_t* added;  // host: scene indices that have an entry
    int64_t* count;  // host: points of each such scene (ivln_mapper_env_append_from_lib sizes its launch by it)
};

struct ivln_mapper {
    int B_max, H, W, rows, cols;
    float res, half_h, half_w, half_res;
    int64_t capacity, table_cells;
    float *xs, *ys;
    Pt* wbuf[2];
    int64_t* rbuf[2];
    unsigned long long* tab64;  // dense per-key arg-max table, left zeroed by the winners
    unsigned long long* cell;   // per map cell: (rank + 1) << 8 | label of the last writer
    Scalars* sc;
    int* bmmL;   // per-block min/max partials of the local cloud (k_local_minmax)
    int* bmmA;   // per-block partials of the points appended this step (k_local_select)
    int* bbox;   // per-block, per-env boxes of the surviving world (k_world_select), read by the NEXT step
    int n_blocks_local;
    int local_blocks, world_blocks;  // launch width of the local- / world-cloud kernels (0: full width)
    int64_t known_rank;
    int64_t seed_rank;  // appended points so far (include/ivln_map_seed.h): the next one's rank is table_cells + this
    // library-mode known steps (include/ivln_known_lib.h); allocated by ivln_mapper_known_attach
    const ivln_known_lib* klib;
    int* kcur;          // latched scene index per row (-1: none)
    float* krot;        // ego rotation per row, derived by the step's first launch
    long long* kcount;  // result word of ivln_mapper_known_count
    // known-map builder (include/ivln_map_build.h); allocated by its first call
    unsigned* env_part;       // device: per-block, per-env {count, lowest rank, highest rank} of k_env_stats
    unsigned* env_part_host;  // host copy the blocks are folded from
    unsigned* scan_buf;       // device: the scan's levels above the marks, level 1 first
    // host-side: an ivln_mapper_step_begin whose _finish has not been issued - its arg-max entries sit in tab64 and every call
    // that reads the table or the cloud is refused (include/ivln_hip.h).  Set by calls, not by launches: a captured replay
    // does not move it.
    bool open;
};

#define HIPCHK(x)                          \
    do {                                   \
        if ((x) != hipSuccess) return IVLN_E_HIP; \
    } while (0)

extern "C" {

const char* ivln_strerror(int code) {
    switch (code) {
        case IVLN_OK: return "ok";
        case IVLN_E_INVALID: return "invalid argument";
        case IVLN_E_HIP: return "HIP runtime error";
        case IVLN_E_KEYSPACE: return "mapper keep-highest key exceeds dense table capacity";
        case IVLN_E_CAPACITY: return "mapper world cloud capacity exceeded";
        case IVLN_E_UNSUPPORTED: return "unsupported configuration";
        default: return "unknown error";
    }
}

int ivln_version(void) { return 1; }

static int init_scalars(ivln_mapper* m, hipStream_t s) {
    Scalars h;
    h.mmL[0] = h.mmL[1] = h.mmW[0] = h.mmW[1] = h.mmWold[0] = h.mmWold[1] = INT32_MAX;
    h.mmL[2] = h.mmL[3] = h.mmW[2] = h.mmW[3] = h.mmWold[2] = h.mmWold[3] = INT32_MIN;
    h.cnt[0] = h.cnt[1] = h.cnt_old = 0;
    h.cur = 0;
    h.n_bbox = 0;
    h.n_bbox_envs = 0;
    h.err = 0;
    HIPCHK(hipMemcpyAsync(m->sc, &h, sizeof(h), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return IVLN_OK;
}

constexpr int kWorldBlocks = 1024;  // grid of the world-cloud kernels (grid-stride over the cloud; one point per thread up to 262 k points)

int ivln_mapper_create(int B_max, int H, int W, double vfov_rad, double height_m, double width_m, double res_m,
                       int64_t world_capacity, int64_t table_cells, ivln_mapper** out) {
    if (!out || B_max <= 0 || B_max > kBoxEnvs || H <= 0 || W <= 0 || res_m <= 0) return IVLN_E_INVALID;
    ivln_mapper* m = new (std::nothrow) ivln_mapper();
    if (!m) return IVLN_E_INVALID;
    m->B_max = B_max; m->H = H; m->W = W;
    m->rows = (int)ceil(height_m / res_m);  // mapper.py:97-99
    m->cols = (int)ceil(width_m / res_m);
    m->res = (float)res_m;
    m->half_h = (float)(height_m / 2);
    m->half_w = (float)(width_m / 2);
    m->half_res = (float)(res_m / 2);
    m->capacity = world_capacity > 0 ? world_capacity : (int64_t)B_max * (1 << 20);
    if (m->capacity > 0xFFFFFF00ll) m->capacity = 0xFFFFFF00ll;
    m->table_cells = table_cells > 0 ? table_cells : (int64_t)(16 << 20);
    if (m->table_cells > (1ll << 31)) m->table_cells = 1ll << 31;  // ranks = keys must fit 31 bits (k_world_max)
    m->known_rank = 0;
    m->seed_rank = 0;
    m->open = false;
    m->klib = nullptr; m->kcur = nullptr; m->krot = nullptr; m->kcount = nullptr;
    m->env_part = nullptr; m->env_part_host = nullptr; m->scan_buf = nullptr;
    m->local_blocks = m->world_blocks = 0;
    // core.py:70-115: intrinsics in python doubles -> fp32; (u + 0.5 - cx) / fx in fp32
    double hfov = (double)W / (double)H * vfov_rad;
    float fx = (float)((double)W / (2.0 * tan(hfov / 2.0)));
    float fy = (float)((double)H / (2.0 * tan(vfov_rad / 2.0)));
    float cx = (float)(W / 2.0), cy = (float)(H / 2.0);
    float* hx = new float[W];
    float* hy = new float[H];
    for (int u = 0; u < W; ++u) {
        volatile float t = (float)u + 0.5f;
        t = t - cx;
        hx[u] = t / fx;
    }
    for (int v = 0; v < H; ++v) {
        volatile float t = (float)v + 0.5f;
        t = t - cy;
        hy[v] = t / fy;
    }
    int cells = B_max * m->rows * m->cols;
    m->n_blocks_local = (int)(((int64_t)B_max * H * W + kThreads * kPPT - 1) / (kThreads * kPPT));
    bool ok = hipMalloc(&m->xs, sizeof(float) * W) == hipSuccess && hipMalloc(&m->ys, sizeof(float) * H) == hipSuccess &&
              hipMalloc(&m->wbuf[0], sizeof(Pt) * (size_t)m->capacity) == hipSuccess &&
              hipMalloc(&m->wbuf[1], sizeof(Pt) * (size_t)m->capacity) == hipSuccess &&
              hipMalloc(&m->rbuf[0], sizeof(int64_t) * (size_t)m->capacity) == hipSuccess &&
              hipMalloc(&m->rbuf[1], sizeof(int64_t) * (size_t)m->capacity) == hipSuccess &&
              hipMalloc(&m->tab64, sizeof(unsigned long long) * (size_t)m->table_cells) == hipSuccess &&
              hipMalloc(&m->cell, sizeof(unsigned long long) * (size_t)cells) == hipSuccess &&
              hipMalloc(&m->sc, sizeof(Scalars)) == hipSuccess &&
              hipMalloc(&m->bmmL, sizeof(int) * 4 * (size_t)(m->n_blocks_local + 1)) == hipSuccess &&
              hipMalloc(&m->bmmA, sizeof(int) * 4 * (size_t)(m->n_blocks_local + 1)) == hipSuccess &&
              hipMalloc(&m->bbox, sizeof(int) * 4 * (size_t)kWorldBlocks * B_max) == hipSuccess;
    if (ok) {
        ok = hipMemcpy(m->xs, hx, sizeof(float) * W, hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(m->ys, hy, sizeof(float) * H, hipMemcpyHostToDevice) == hipSuccess &&
             hipMemset(m->tab64, 0, sizeof(unsigned long long) * (size_t)m->table_cells) == hipSuccess &&
             hipMemset(m->cell, 0, sizeof(unsigned long long) * (size_t)cells) == hipSuccess &&
             init_scalars(m, nullptr) == IVLN_OK;
    }
    delete[] hx;
    delete[] hy;
    if (!ok) {
        ivln_mapper_destroy(m);
        return IVLN_E_HIP;
    }
    *out = m;
    return IVLN_OK;
}

int ivln_mapper_destroy(ivln_mapper* m) {
    if (!m) return IVLN_OK;
    (void)hipFree(m->xs); (void)hipFree(m->ys);
    (void)hipFree(m->wbuf[0]); (void)hipFree(m->wbuf[1]); (void)hipFree(m->rbuf[0]); (void)hipFree(m->rbuf[1]);
    (void)hipFree(m->tab64); (void)hipFree(m->cell); (void)hipFree(m->sc); (void)hipFree(m->bmmL); (void)hipFree(m->bmmA);
    (void)hipFree(m->bbox);
    if (m->kcur) (void)hipFree(m->kcur);
    if (m->krot) (void)hipFree(m->krot);
    if (m->kcount) (void)hipFree(m->kcount);
    if (m->env_part) (void)hipFree(m->env_part);
    if (m->scan_buf) (void)hipFree(m->scan_buf);
    free(m->env_part_host);
    delete m;
    return IVLN_OK;
}

int ivln_mapper_reset(ivln_mapper* m, void* stream) {
    if (!m) return IVLN_E_INVALID;
    m->known_rank = 0;
    m->seed_rank = 0;
    // whatever an unfinished ivln_mapper_step_begin (or a step that raised IVLN_E_*) left in the arg-max table goes with the
    // cloud: the next step's winners must find their own entries there, not a forgotten frame's
    HIPCHK(hipMemsetAsync(m->tab64, 0, sizeof(unsigned long long) * (size_t)m->table_cells, (hipStream_t)stream));
    m->open = false;
    if (m->kcur) HIPCHK(hipMemsetAsync(m->kcur, 0xFF, sizeof(int) * (size_t)m->B_max, (hipStream_t)stream));  // -1: no scene
    return init_scalars(m, (hipStream_t)stream);
}

int ivln_mapper_frames(const float* pose, const double* orientation, int B, float* T, float* rot, void* stream) {
    if (B <= 0) return IVLN_E_INVALID;
    hipLaunchKernelGGL(k_frames, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, pose, orientation, B, T, rot);
    return hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP;
}

// The label-free half of a step: camera transforms (posed entry), local min / max, the keep-highest arg-max of the local
// cloud (csrc header: kernels 1-2).  Reads depth and the sensor pose only - with predicted semantics it can run beside the
// network that produces the labels (ivln_mapper_step_begin).
static int mapper_begin(ivln_mapper* m, const float* depth, const float* T, const float* pose, const float* rot,
                        const double* orientation, float* T_out, float* rot_out, const uint8_t* not_done, int B,
                        uint8_t* occ_out, void* stream) {
    if (!m || B <= 0 || B > m->B_max) return IVLN_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int64_t npix = (int64_t)B * m->H * m->W;
    int lb = (int)((npix + kThreads * kPPT - 1) / (kThreads * kPPT));  // local-cloud chunks: 4 pixels / thread
    if (m->local_blocks > 0 && m->local_blocks < lb) lb = m->local_blocks;  // narrow launch: a block walks several chunks
    const int map_cells = B * m->rows * m->cols;
    if (orientation) {  // posed entry: transforms derived inside the first kernel
        const Cam c0{depth, nullptr, pose, m->xs, m->ys, B, m->H, m->W, m->half_res};
        hipLaunchKernelGGL(k_local_minmax<true>, dim3(lb), dim3(kThreads), 0, s, c0, occ_out, map_cells, m->bmmL,
                           orientation, T_out, rot_out);
        T = T_out;
        rot = rot_out;
    }
    const Cam cm{depth, T, pose, m->xs, m->ys, B, m->H, m->W, m->half_res};
    if (!orientation)
        hipLaunchKernelGGL(k_local_minmax<false>, dim3(lb), dim3(kThreads), 0, s, cm, occ_out, map_cells, m->bmmL,
                           (const double*)nullptr, (float*)nullptr, (float*)nullptr);
    hipLaunchKernelGGL(k_local_argmax, dim3(lb), dim3(kThreads), 0, s, cm, m->sc, m->tab64, m->table_cells, m->bmmL, lb,
                       m->bbox, m->B_max, not_done);
    return hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP;
}

// The rest of the step begun by mapper_begin (same batch, same T / pose / rot, same launch width): label the surviving local
// points, merge them into the world cloud, raster.  No host-side state links the two halves - a captured step records each
// half once and replays them many times -, the kernels' own state (arg-max table, block partials) does.  (The handle's
// `open` flag links nothing: it only refuses the calls that must not meet an unfinished arg-max in the table.)
static int mapper_finish(ivln_mapper* m, const float* depth, const uint8_t* labels, const float* T, const float* pose,
                         const float* rot, const uint8_t* not_done, int B, uint8_t* occ_out, uint8_t* sem_out, void* stream) {
    if (!m || B <= 0 || B > m->B_max) return IVLN_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int64_t npix = (int64_t)B * m->H * m->W;
    int lb = (int)((npix + kThreads * kPPT - 1) / (kThreads * kPPT));
    if (m->local_blocks > 0 && m->local_blocks < lb) lb = m->local_blocks;  // (as in mapper_begin)
    const int map_cells = B * m->rows * m->cols;
    const unsigned cap = (unsigned)m->capacity;
    const Cam cm{depth, T, pose, m->xs, m->ys, B, m->H, m->W, m->half_res};
    hipLaunchKernelGGL(k_local_select, dim3(lb), dim3(kThreads), 0, s, cm, labels, m->sc, m->tab64, m->table_cells,
                       m->wbuf[0], m->wbuf[1], m->rbuf[0], m->rbuf[1], cap, m->bmmA);
    // world-cloud kernels: full width = up to 1024 workgroups, one point per thread; a narrow launch (set_launch_width) =
    // at most world_blocks workgroups that take 16 points per thread, so few CUs while the cloud is small
    const int wb = (m->world_blocks > 0 && m->world_blocks < kWorldBlocks) ? m->world_blocks : kWorldBlocks;
    const int wpt = m->world_blocks > 0 ? 16 : 1;
    hipLaunchKernelGGL(k_world_max, dim3(wb), dim3(kThreads), 0, s, m->wbuf[0], m->wbuf[1], m->rbuf[0],
                       m->rbuf[1], B, not_done, m->half_res, m->sc, m->tab64, m->table_cells, cap, m->bmmA, lb, wpt);
    hipLaunchKernelGGL(k_world_select, dim3(wb), dim3(kThreads), 0, s, m->wbuf[0], m->wbuf[1], m->rbuf[0],
                       m->rbuf[1], B, not_done, m->half_res, m->sc, m->tab64, m->table_cells, cap, pose, rot, m->rows,
                       m->cols, m->res, m->half_h, m->half_w, occ_out, m->cell, m->bbox, m->B_max, wpt);
    const int fin_blocks = (map_cells + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(k_finalize, dim3(fin_blocks), dim3(kThreads), 0, s, m->cell, sem_out, map_cells, m->sc, 1, cap,
                       wb, B);
    return hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP;
}

static int mapper_step(ivln_mapper* m, const float* depth, const uint8_t* labels, const float* T, const float* pose,
                       const float* rot, const double* orientation, float* T_out, float* rot_out,
                       const uint8_t* not_done, int B, uint8_t* occ_out, uint8_t* sem_out, void* stream) {
    const int rc = mapper_begin(m, depth, T, pose, rot, orientation, T_out, rot_out, not_done, B, occ_out, stream);
    if (rc != IVLN_OK) return rc;
    return mapper_finish(m, depth, labels, orientation ? T_out : T, pose, orientation ? rot_out : rot, not_done, B, occ_out, sem_out, stream);
}

int ivln_mapper_step_begin(ivln_mapper* m, const float* depth, const float* pose, const double* orientation,
                           const uint8_t* not_done, int B, uint8_t* occ_out, float* T_out, float* rot_out, void* stream) {
    if (!depth || !pose || !orientation || !T_out || !rot_out || !not_done || !occ_out) return IVLN_E_INVALID;
    if (m && m->open) return IVLN_E_INVALID;  // (a second arg-max on top of the first one's entries)
    const int rc = mapper_begin(m, depth, nullptr, pose, nullptr, orientation, T_out, rot_out, not_done, B, occ_out, stream);
    if (rc == IVLN_OK) m->open = true;
    return rc;
}

int ivln_mapper_step_finish(ivln_mapper* m, const float* depth, const uint8_t* labels, const float* T, const float* pose,
                            const float* rot, const uint8_t* not_done, int B, uint8_t* occ_out, uint8_t* sem_out, void* stream) {
    if (!depth || !labels || !T || !pose || !rot || !not_done || !occ_out || !sem_out) return IVLN_E_INVALID;
    // (accepted on a closed mapper as well: a split capture records _finish once per phase behind a single _begin)
    const int rc = mapper_finish(m, depth, labels, T, pose, rot, not_done, B, occ_out, sem_out, stream);
    if (rc == IVLN_OK) m->open = false;
    return rc;
}

int ivln_mapper_step(ivln_mapper* m, const float* depth, const uint8_t* labels, const float* T, const float* pose,
                     const float* rot, const uint8_t* not_done, int B, uint8_t* occ_out, uint8_t* sem_out,
                     void* stream) {
    if (!T || !rot || (m && m->open)) return IVLN_E_INVALID;
    return mapper_step(m, depth, labels, T, pose, rot, nullptr, nullptr, nullptr, not_done, B, occ_out, sem_out, stream);
}

int ivln_mapper_step_posed(ivln_mapper* m, const float* depth, const uint8_t* labels, const float* pose,
                           const double* orientation, const uint8_t* not_done, int B, uint8_t* occ_out,
                           uint8_t* sem_out, float* T_out, float* rot_out, void* stream) {
    if (!orientation || !T_out || !rot_out || (m && m->open)) return IVLN_E_INVALID;
    return mapper_step(m, depth, labels, nullptr, pose, nullptr, orientation, T_out, rot_out, not_done, B, occ_out, sem_out,
                       stream);
}

int ivln_mapper_set_launch_width(ivln_mapper* m, int local_blocks, int world_blocks) {
    if (!m || local_blocks < 0 || world_blocks < 0) return IVLN_E_INVALID;
    m->local_blocks = local_blocks;
    m->world_blocks = world_blocks;
    return IVLN_OK;
}

int ivln_mapper_known_begin(ivln_mapper* m, const uint8_t* not_done, int B, void* stream) {
    if (!m || B <= 0 || B > m->B_max) return IVLN_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_known_clear, dim3(256), dim3(kThreads), 0, s, m->wbuf[0], m->wbuf[1], m->rbuf[0], m->rbuf[1], B,
                       not_done, m->sc, (unsigned)m->capacity);
    hipLaunchKernelGGL(k_swap_counts, dim3(1), dim3(1), 0, s, m->sc, (unsigned)m->capacity);
    return hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP;
}

int ivln_mapper_load_known(ivln_mapper* m, int b, const float* xyz, const uint8_t* sem, int64_t n, void* stream) {
    if (!m || b < 0 || b >= m->B_max || n < 0) return IVLN_E_INVALID;
    if (n == 0) return IVLN_OK;
    hipStream_t s = (hipStream_t)stream;
    int blocks = (int)((n + kThreads - 1) / kThreads);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_known_load, dim3(blocks), dim3(kThreads), 0, s, xyz, sem, n, b, m->known_rank, m->sc,
                       m->wbuf[0], m->wbuf[1], m->rbuf[0], m->rbuf[1], (unsigned)m->capacity);
    hipLaunchKernelGGL(k_known_commit, dim3(1), dim3(1), 0, s, m->sc, n, (unsigned)m->capacity);
    m->known_rank += n;
    return hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP;
}

int ivln_mapper_known_raster(ivln_mapper* m, const float* pose, const float* rot, int B, uint8_t* occ_out,
                             uint8_t* sem_out, void* stream) {
    if (!m || B <= 0 || B > m->B_max) return IVLN_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int map_cells = B * m->rows * m->cols;
    hipLaunchKernelGGL(k_zero_u8, dim3((map_cells + kThreads - 1) / kThreads), dim3(kThreads), 0, s, occ_out, map_cells);
    hipLaunchKernelGGL(k_known_raster, dim3(256), dim3(kThreads), 0, s, m->wbuf[0], m->wbuf[1], m->rbuf[0], m->rbuf[1],
                       m->sc, pose, rot, B, m->rows, m->cols, m->res, m->half_h, m->half_w, occ_out, m->cell);
    hipLaunchKernelGGL(k_finalize, dim3((map_cells + kThreads - 1) / kThreads), dim3(kThreads), 0, s, m->cell,
                       sem_out, map_cells, m->sc, 0, (unsigned)m->capacity, 0, 0);
    return hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP;
}

// ---- known-map mode over a scene library (include/ivln_known_lib.h) ----
int ivln_known_lib_create(int max_scenes, ivln_known_lib** out) {
    if (!out || max_scenes <= 0 || max_scenes > (1 << 20)) return IVLN_E_INVALID;
    ivln_known_lib* lib = new (std::nothrow) ivln_known_lib();
    if (!lib) return IVLN_E_INVALID;
    lib->max_scenes = max_scenes;
    lib->n_added = 0;
    lib->table = nullptr;
    lib->added = (uint8_t*)calloc((size_t)max_scenes, 1);
    lib->count = (int64_t*)calloc((size_t)max_scenes, sizeof(int64_t));
    if (!lib->added || !lib->count || hipMalloc(&lib->table, sizeof(KScene) * (size_t)max_scenes) != hipSuccess ||
        hipMemset(lib->table, 0, sizeof(KScene) * (size_t)max_scenes) != hipSuccess) {
        ivln_known_lib_destroy(lib);
        return IVLN_E_HIP;
    }
    *out = lib;
    return IVLN_OK;
}

int ivln_known_lib_destroy(ivln_known_lib* lib) {
    if (!lib) return IVLN_OK;
    if (lib->table) (void)hipFree(lib->table);
    free(lib->added);
    free(lib->count);
    delete lib;
    return IVLN_OK;
}

int ivln_known_lib_add(ivln_known_lib* lib, int scene, const float* xyz, const uint8_t* sem, int64_t n, void* records,
                       void* stream) {
    if (!lib || scene < 0 || scene >= lib->max_scenes || lib->added[scene] || n < 0 || n >= (1ll << 31)) return IVLN_E_INVALID;
    if (n > 0 && (!xyz || !sem || !records || ((uintptr_t)records & 15u))) return IVLN_E_INVALID;
    int blocks = (int)((n + kThreads - 1) / kThreads);
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;  // (an empty scene still gets its entry)
    hipLaunchKernelGGL(k_known_pack, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, xyz, sem, (int)n, (Pt*)records,
                       lib->table + scene);
    if (hipGetLastError() != hipSuccess) return IVLN_E_HIP;
    lib->added[scene] = 1;
    lib->count[scene] = n;
    lib->n_added += 1;
    return IVLN_OK;
}

int ivln_known_lib_size(ivln_known_lib* lib) { return lib ? lib->n_added : IVLN_E_INVALID; }

int ivln_mapper_known_attach(ivln_mapper* m, ivln_known_lib* lib) {
    if (!m || !lib) return IVLN_E_INVALID;
    if (!m->kcur) {
        int* cur = nullptr;
        float* rot = nullptr;
        long long* cnt = nullptr;
        const bool ok = hipMalloc(&cur, sizeof(int) * (size_t)m->B_max) == hipSuccess &&
                        hipMalloc(&rot, sizeof(float) * 9 * (size_t)m->B_max) == hipSuccess &&
                        hipMalloc(&cnt, sizeof(long long)) == hipSuccess &&
                        hipMemset(cur, 0xFF, sizeof(int) * (size_t)m->B_max) == hipSuccess &&
                        hipMemset(rot, 0, sizeof(float) * 9 * (size_t)m->B_max) == hipSuccess;
        if (!ok) {
            (void)hipFree(cur); (void)hipFree(rot); (void)hipFree(cnt);
            return IVLN_E_HIP;
        }
        m->kcur = cur; m->krot = rot; m->kcount = cnt;
    }
    m->klib = lib;
    return IVLN_OK;
}

int ivln_mapper_known_step(ivln_mapper* m, const int32_t* scene_id, const float* pose, const double* orientation,
                           const uint8_t* not_done, int B, uint8_t* occ_out, uint8_t* sem_out, void* stream) {
    if (!m || !m->klib || !scene_id || !pose || !orientation || !not_done || !occ_out || !sem_out || B <= 0 || B > m->B_max)
        return IVLN_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int map_cells = B * m->rows * m->cols;
    const int cell_blocks = (map_cells + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(k_known_latch, dim3(cell_blocks), dim3(kThreads), 0, s, scene_id, not_done, orientation, B, m->B_max,
                       m->kcur, m->krot, m->klib->table, m->klib->max_scenes, m->sc, occ_out, map_cells);
    hipLaunchKernelGGL(k_known_lib_raster, dim3(kKnownBlocks, B), dim3(kThreads), 0, s, m->kcur, m->klib->table,
                       m->klib->max_scenes, pose, m->krot, m->rows, m->cols, m->res, m->half_h, m->half_w, occ_out, m->cell);
    hipLaunchKernelGGL(k_finalize, dim3(cell_blocks), dim3(kThreads), 0, s, m->cell, sem_out, map_cells, m->sc, 0,
                       (unsigned)m->capacity, 0, 0);
    return hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP;
}

int ivln_mapper_known_count(ivln_mapper* m, int B, int64_t* n, void* stream) {
    if (!m || !m->klib || !n || B <= 0 || B > m->B_max) return IVLN_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_known_count, dim3(1), dim3(1), 0, s, m->kcur, m->klib->table, m->klib->max_scenes, B, m->kcount);
    long long h = 0;
    HIPCHK(hipMemcpyAsync(&h, m->kcount, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *n = (int64_t)h;
    return IVLN_OK;
}

int ivln_mapper_status(ivln_mapper* m, int64_t* world_n, void* stream) {
    if (!m) return IVLN_E_INVALID;
    Scalars h;
    HIPCHK(hipMemcpyAsync(&h, m->sc, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    if (world_n) *world_n = (int64_t)h.cnt[h.cur & 1];
    return h.err;
}

int ivln_mapper_world_export(ivln_mapper* m, float* xyz, uint32_t* meta, int64_t* rank, int64_t max_n,
                             int64_t* n_out, void* stream) {
    if (!m || !n_out) return IVLN_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    Scalars h;
    HIPCHK(hipMemcpyAsync(&h, m->sc, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const int cur = h.cur & 1;
    int64_t n = (int64_t)h.cnt[cur];
    *n_out = n;
    if (n > max_n) n = max_n;
    if (n > 0) {
        // strided device->device copies out of the 16-byte point records
        HIPCHK(hipMemcpy2DAsync(xyz, 12, m->wbuf[cur], sizeof(Pt), 12, (size_t)n, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpy2DAsync(meta, 4, (const char*)m->wbuf[cur] + 12, sizeof(Pt), 4, (size_t)n,
                                hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(rank, m->rbuf[cur], sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return IVLN_OK;
}

// ---- known-map builder (include/ivln_map_build.h) ----
struct EnvStat {
    int64_t n;
    uint32_t kmin, kmax;
};

static int builder_scratch(ivln_mapper* m) {
    if (m->env_part) return IVLN_OK;
    const size_t part = (size_t)kStatBlocks * m->B_max * 3;
    size_t levels = 0;  // entries of every scan level above a window of table_cells marks
    for (int64_t n = m->table_cells;;) {
        n = (n + kThreads - 1) / kThreads;
        levels += (size_t)n;
        if (n <= kThreads) break;
    }
    unsigned *dp = nullptr, *ds = nullptr;
    unsigned* hp = (unsigned*)malloc(sizeof(unsigned) * part);
    if (!hp || hipMalloc(&dp, sizeof(unsigned) * part) != hipSuccess || hipMalloc(&ds, sizeof(unsigned) * levels) != hipSuccess) {
        free(hp);
        (void)hipFree(dp);
        (void)hipFree(ds);
        return IVLN_E_HIP;
    }
    m->env_part = dp; m->env_part_host = hp; m->scan_buf = ds;
    return IVLN_OK;
}

// One launch + one read-back (synchronises): st[b] for every b < B_max, *total = points of the cloud.
static int env_stats(ivln_mapper* m, EnvStat* st, int64_t* total, hipStream_t s) {
    const int rc = builder_scratch(m);
    if (rc != IVLN_OK) return rc;
    hipLaunchKernelGGL(k_env_stats, dim3(kStatBlocks), dim3(kThreads), 0, s, m->wbuf[0], m->wbuf[1], m->rbuf[0], m->rbuf[1],
                       m->sc, (unsigned)m->capacity, m->B_max, m->env_part);
    if (hipGetLastError() != hipSuccess) return IVLN_E_HIP;
    const size_t part = (size_t)kStatBlocks * m->B_max * 3;
    HIPCHK(hipMemcpyAsync(m->env_part_host, m->env_part, sizeof(unsigned) * part, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *total = 0;
    for (int b = 0; b < m->B_max; ++b) {
        EnvStat e{0, 0xFFFFFFFFu, 0u};
        for (int k = 0; k < kStatBlocks; ++k) {
            const unsigned* p = m->env_part_host + ((size_t)k * m->B_max + b) * 3;
            e.n += p[0];
            if (p[1] < e.kmin) e.kmin = p[1];
            if (p[2] > e.kmax) e.kmax = p[2];
        }
        st[b] = e;
        *total += e.n;
    }
    return IVLN_OK;
}

// mark / scan / scatter of env b (e.n <= max_n was checked); xyz + sem, or rec
static int env_compact(ivln_mapper* m, int b, const EnvStat& e, int64_t total, float* xyz, uint8_t* sem, Pt* rec,
                       int64_t max_n, hipStream_t s) {
    if (e.n == 0) return IVLN_OK;
    if (e.kmin > e.kmax || (int64_t)e.kmax >= m->table_cells) return IVLN_E_UNSUPPORTED;  // ranks that are not keys
    const unsigned window = e.kmax - e.kmin + 1u;  // <= table_cells <= 2^31
    const unsigned cap = (unsigned)m->capacity;
    int mb = (int)((total + kThreads - 1) / kThreads);
    if (mb > kWorldBlocks) mb = kWorldBlocks;
    hipLaunchKernelGGL(k_env_mark, dim3(mb), dim3(kThreads), 0, s, m->wbuf[0], m->wbuf[1], m->rbuf[0], m->rbuf[1], m->sc, cap,
                       (unsigned)b, e.kmin, window, m->tab64);
    // levels of the scan: cnt[0] marks, cnt[k + 1] = tiles of level k, until one tile holds the top level
    unsigned cnt[8];
    unsigned* lvl[8];
    int top = 0;
    cnt[0] = window;
    lvl[0] = nullptr;
    unsigned* next = m->scan_buf;
    do {
        cnt[top + 1] = (cnt[top] + kThreads - 1) / kThreads;
        lvl[top + 1] = next;
        next += cnt[top + 1];
        ++top;
    } while (cnt[top] > (unsigned)kThreads);
    hipLaunchKernelGGL(k_scan_up<true>, dim3(cnt[1]), dim3(kThreads), 0, s, m->tab64, (const unsigned*)nullptr, window, lvl[1]);
    for (int k = 1; k < top; ++k)
        hipLaunchKernelGGL(k_scan_up<false>, dim3(cnt[k + 1]), dim3(kThreads), 0, s, (const unsigned long long*)nullptr, lvl[k],
                           cnt[k], lvl[k + 1]);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(kThreads), 0, s, lvl[top], cnt[top]);
    for (int k = top - 1; k >= 1; --k)
        hipLaunchKernelGGL(k_scan_down, dim3(cnt[k + 1]), dim3(kThreads), 0, s, lvl[k], cnt[k], lvl[k + 1]);
    if (rec)
        hipLaunchKernelGGL(k_env_scatter<true>, dim3(cnt[1]), dim3(kThreads), 0, s, m->tab64, window, lvl[1], m->wbuf[0],
                           m->wbuf[1], m->sc, cap, (float*)nullptr, (uint8_t*)nullptr, rec, max_n);
    else
        hipLaunchKernelGGL(k_env_scatter<false>, dim3(cnt[1]), dim3(kThreads), 0, s, m->tab64, window, lvl[1], m->wbuf[0],
                           m->wbuf[1], m->sc, cap, xyz, sem, (Pt*)nullptr, max_n);
    return hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP;
}

int ivln_mapper_env_counts(ivln_mapper* m, int B, int64_t* counts_host, void* stream) {
    if (!m || !counts_host || B <= 0 || B > m->B_max) return IVLN_E_INVALID;
    EnvStat st[kBoxEnvs];
    int64_t total = 0;
    const int rc = env_stats(m, st, &total, (hipStream_t)stream);
    if (rc != IVLN_OK) return rc;
    for (int b = 0; b < B; ++b) counts_host[b] = st[b].n;
    return IVLN_OK;
}

int ivln_mapper_env_export(ivln_mapper* m, int b, float* xyz, uint8_t* sem, int64_t max_n, int64_t* n_out, void* stream) {
    if (!m || !n_out || b < 0 || b >= m->B_max || max_n < 0 || (max_n > 0 && (!xyz || !sem))) return IVLN_E_INVALID;
    if (m->open) return IVLN_E_INVALID;  // (the marks would share the table with an unfinished arg-max)
    if (m->known_rank != 0) return IVLN_E_UNSUPPORTED;
    EnvStat st[kBoxEnvs];
    int64_t total = 0;
    const int rc = env_stats(m, st, &total, (hipStream_t)stream);
    if (rc != IVLN_OK) return rc;
    *n_out = st[b].n;
    if (st[b].n > max_n) return IVLN_E_CAPACITY;
    return env_compact(m, b, st[b], total, xyz, sem, nullptr, max_n, (hipStream_t)stream);
}

int ivln_known_lib_add_from_mapper(ivln_known_lib* lib, int scene, ivln_mapper* m, int b, void* records, int64_t max_n,
                                   void* stream) {
    if (!lib || !m || scene < 0 || scene >= lib->max_scenes || lib->added[scene] || b < 0 || b >= m->B_max || max_n < 0)
        return IVLN_E_INVALID;
    if (max_n > 0 && (!records || ((uintptr_t)records & 15u))) return IVLN_E_INVALID;
    if (m->open) return IVLN_E_INVALID;
    if (m->known_rank != 0) return IVLN_E_UNSUPPORTED;
    EnvStat st[kBoxEnvs];
    int64_t total = 0;
    int rc = env_stats(m, st, &total, (hipStream_t)stream);
    if (rc != IVLN_OK) return rc;
    if (st[b].n > max_n) return IVLN_E_CAPACITY;
    if (st[b].n >= (1ll << 31)) return IVLN_E_INVALID;  // (a library scene holds < 2^31 points: ivln_known_lib_add)
    rc = env_compact(m, b, st[b], total, nullptr, nullptr, (Pt*)records, max_n, (hipStream_t)stream);
    if (rc != IVLN_OK) return rc;
    hipLaunchKernelGGL(k_known_entry, dim3(1), dim3(1), 0, (hipStream_t)stream, lib->table + scene, (const Pt*)records,
                       (int)st[b].n);
    if (hipGetLastError() != hipSuccess) return IVLN_E_HIP;
    lib->added[scene] = 1;
    lib->count[scene] = st[b].n;
    lib->n_added += 1;
    return IVLN_OK;
}

// ---- seeding an iterative mapper (include/ivln_map_seed.h) ----
static int seed_refused(const ivln_mapper* m) {
    if (m->open) return IVLN_E_INVALID;  // (between an ivln_mapper_step_begin and its _finish the cloud is not to be touched)
    return (m->klib || m->known_rank != 0) ? IVLN_E_UNSUPPORTED : IVLN_OK;
}

int ivln_mapper_rows_clear(ivln_mapper* m, const uint8_t* keep, int B, void* stream) {
    if (!m || !keep || B <= 0 || B > m->B_max) return IVLN_E_INVALID;
    const int rc = seed_refused(m);
    if (rc != IVLN_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const unsigned cap = (unsigned)m->capacity;
    hipLaunchKernelGGL(k_known_clear, dim3(256), dim3(kThreads), 0, s, m->wbuf[0], m->wbuf[1], m->rbuf[0], m->rbuf[1], B,
                       keep, m->sc, cap);
    hipLaunchKernelGGL(k_rows_boxes, dim3(kSeedBoxBlocks), dim3(kThreads), 0, s, keep, B, m->sc, cap, m->bbox, m->B_max,
                       kWorldBlocks);
    return hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP;
}

// the checks that need the device (arguments were checked by the caller), then the two launches
static int env_append(ivln_mapper* m, int b, const float* xyz, const uint8_t* sem, const KScene* entry, int64_t n,
                      hipStream_t s) {
    const int64_t rank_base = m->table_cells + m->seed_rank;
    if (n > (1ll << 31) - rank_base) return IVLN_E_KEYSPACE;
    if (n == 0) return IVLN_OK;
    Scalars h;
    HIPCHK(hipMemcpyAsync(&h, m->sc, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if ((int64_t)h.cnt[h.cur & 1] + n > m->capacity) return IVLN_E_CAPACITY;
    hipLaunchKernelGGL(k_seed_boxes, dim3(1), dim3(kThreads), 0, s, m->sc, b, m->bbox, m->B_max, kWorldBlocks);
    int blocks = (int)((n + kThreads - 1) / kThreads);
    if (blocks > kWorldBlocks) blocks = kWorldBlocks;
    const unsigned cap = (unsigned)m->capacity;
    if (entry)
        hipLaunchKernelGGL(k_env_append<true>, dim3(blocks), dim3(kThreads), 0, s, (const float*)nullptr,
                           (const uint8_t*)nullptr, entry, n, b, rank_base, m->half_res, m->sc, m->wbuf[0], m->wbuf[1],
                           m->rbuf[0], m->rbuf[1], cap, m->bbox, m->B_max, kWorldBlocks);
    else
        hipLaunchKernelGGL(k_env_append<false>, dim3(blocks), dim3(kThreads), 0, s, xyz, sem, (const KScene*)nullptr, n, b,
                           rank_base, m->half_res, m->sc, m->wbuf[0], m->wbuf[1], m->rbuf[0], m->rbuf[1], cap, m->bbox,
                           m->B_max, kWorldBlocks);
    if (hipGetLastError() != hipSuccess) return IVLN_E_HIP;
    m->seed_rank += n;
    return IVLN_OK;
}

int ivln_mapper_env_append(ivln_mapper* m, int b, const float* xyz, const uint8_t* sem, int64_t n, void* stream) {
    if (!m || b < 0 || b >= m->B_max || n < 0 || (n > 0 && (!xyz || !sem))) return IVLN_E_INVALID;
    const int rc = seed_refused(m);
    if (rc != IVLN_OK) return rc;
    return env_append(m, b, xyz, sem, nullptr, n, (hipStream_t)stream);
}

int ivln_mapper_env_append_from_lib(ivln_mapper* m, int b, const ivln_known_lib* lib, int scene, void* stream) {
    if (!m || b < 0 || b >= m->B_max || !lib || scene < 0 || scene >= lib->max_scenes || !lib->added[scene])
        return IVLN_E_INVALID;
    const int rc = seed_refused(m);
    if (rc != IVLN_OK) return rc;
    return env_append(m, b, nullptr, nullptr, lib->table + scene, lib->count[scene], (hipStream_t)stream);
}

// ---- the table's invariant, observed (include/ivln_mapper_debug.h) ----
int ivln_mapper_debug_nonzero(ivln_mapper* m, int64_t out[2], void* stream) {
    if (!m || !out) return IVLN_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* d = nullptr;
    unsigned long long h[2] = {0ull, 0ull};
    HIPCHK(hipMalloc(&d, sizeof(h)));
    const int64_t n[2] = {m->table_cells, (int64_t)m->B_max * m->rows * m->cols};
    const unsigned long long* p[2] = {m->tab64, m->cell};
    bool ok = hipMemsetAsync(d, 0, sizeof(h), s) == hipSuccess;
    for (int k = 0; ok && k < 2; ++k) {
        int64_t blocks = (n[k] + kThreads - 1) / kThreads;
        if (blocks > kWorldBlocks) blocks = kWorldBlocks;
        hipLaunchKernelGGL(k_debug_nonzero, dim3((unsigned)blocks), dim3(kThreads), 0, s, p[k], n[k], d + k);
        ok = hipGetLastError() == hipSuccess;
    }
    ok = ok && hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = hipStreamSynchronize(s) == hipSuccess && ok;
    (void)hipFree(d);
    if (!ok) return IVLN_E_HIP;
    out[0] = (int64_t)h[0];
    out[1] = (int64_t)h[1];
    return IVLN_OK;
}
}  // extern "C"
