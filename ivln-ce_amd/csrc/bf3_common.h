// Device- and host-side pieces of the split-bf16 convolutions of conv_bf3.hip, each written ONCE: the piece arithmetic, the
// layout of a staged pixel, the product ladder, the record store, the quad epilogue, the partial tiles' way through LDS and
// the launchers' LDS limit ("Split-bf16 convs: what is shared").  Every formula keeps the association and the
// issue order it always had: the kernels are held to the same bytes, not to a tolerance.
//
//   x = x1 + x2 + x3: x1 = bf16(x) (round to nearest even), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2); the remainders are
//   exact in fp32, |x2| <= 2^-8 |x|, |x3| <= 2^-16 |x|, and what the three pieces miss is below 2^-25 |x| - an fp32
//   significand is 24 bits, bf16 has fp32's exponent range (below 2^-110 the last piece runs out of exponent; infinities
//   and NaNs travel in x1 alone: a non-finite input never gives a finite output, but an infinity can come out as NaN).
//   a * b = (a1 + a2 + a3)(b1 + b2 + b3): of the nine piece products the kernels issue the six of relative size >= 2^-16 -
//   a1b1, a1b2, a2b1, a1b3, a2b2, a3b1 - each exact in the MFMA (8 x 8 significand bits) and accumulated in fp32 like
//   the fp32 MFMA accumulates its products; the three they drop (a2b3, a3b2 <= 2^-24 |a b| each, a3b3) sum to less than
//   2^-23 |a b| - the size of fp32's own rounding of the product.  Measured against float64 the result is as close as the
//   fp32 MFMA kernel's (tests/test_gpu_kernels.py: both within the same bar, error tables in DESIGN.md section 3).
//   Six bf16 MFMAs of K = 16 replace eight fp32 MFMAs of K = 2: 192 instead of 512 pipe cycles per 16 channels x 1 tap.
#pragma once
#include "gemm_common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v2i __attribute__((ext_vector_type(2)));

constexpr int PIXB = 112;   // bytes per staged pixel: 3 pieces x 16 channels x 2 bytes + 16 of padding
constexpr int CB = 16;      // input channels per chunk = K of one MFMA

__host__ __device__ constexpr int bf3_taps_padded(int KS) { return KS == 7 ? 54 : (KS == 3 ? 9 : (KS == 2 ? 4 : 1)); }  // multiple of every prefetch depth used (3, 6 | 3, 9 | 2, 4)
// KS == 2: the 2 x 2 window of the stacked output-parity classes of a stride-2 3x3 transposed conv (IVLN_B_CONV_K2 ->
// IVLN_D_NCHW_UP2X4, rednet.py:152-181: taps at input offsets 0..1, pad 0, the row / column past the edge reads as zero; rows
// m = 4 * channel + class, a row's pixel (ho, wo) is output pixel (2 ho + a, 2 wo + b) of channel m / 4).
// Patch geometry of a (PTH x PTW) tile: rows ho0 - pad .. + PTH + KS - 2; columns on a grid of aligned 16-byte groups that
// starts bf3_gx0(KS) pixels left of the tile (odd kernels need the left halo's group, the 2 x 2 window does not).
__host__ __device__ constexpr int bf3_gx0(int KS) { return KS == 2 ? 0 : 4; }
__host__ __device__ constexpr int bf3_xoff(int KS) { return KS == 2 ? 0 : 4 - KS / 2; }  // patch column x = pixel x + XOFF of the group grid
__host__ __device__ constexpr int bf3_stage_chunks(int KS) { return KS == 1 ? 4 : 1; }  // 16-channel chunks staged per barrier pair (1x1: one tap per chunk)

// x -> the upper 16 bits of its three pieces (see the header): round-to-nearest-even at each step, remainders exact.
__device__ __forceinline__ uint32_t bf16_rne_bits(float v, bool& fin) {
    const uint32_t u = __float_as_uint(v);
    fin = (u & 0x7F800000u) != 0x7F800000u;
    uint32_t hb = (u + 0x7FFFu + ((u >> 16) & 1u)) & 0xFFFF0000u;
    if (fin && (hb & 0x7F800000u) == 0x7F800000u) hb = u & 0xFFFF0000u;  // (next to FLT_MAX: do not round a finite value to infinity)
    if (!fin) hb = (u & 0xFFFF0000u) | ((u & 0x007FFFFFu) ? 0x00400000u : 0u);  // infinity as it is; a NaN stays a NaN
    return hb;
}
__device__ __forceinline__ void split3(float x, uint32_t& h, uint32_t& m, uint32_t& l) {
    bool fin, f2;
    const uint32_t hb = bf16_rne_bits(x, fin);
    const float r = fin ? __fsub_rn(x, __uint_as_float(hb)) : 0.f;  // (infinities and NaNs travel in the first piece alone)
    const uint32_t mb = bf16_rne_bits(r, f2);
    const float r2 = __fsub_rn(r, __uint_as_float(mb));
    const uint32_t lb = bf16_rne_bits(r2, f2);
    h = hb >> 16;
    m = mb >> 16;
    l = lb >> 16;
}

// Two values at once, on v_cvt_pk_bf16_f32 (round to nearest even, two floats -> one packed word: first value in the low half):
// 11 VALU operations per pair and piece set instead of ~40.  What the staging passes use; non-finite values: the first piece
// carries them, the remainders turn NaN (the header's "an infinity can come out as NaN"), and a finite value within 2^-9 of
// FLT_MAX rounds its first piece to infinity.
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t cvt_pk_bf16(float a, float b) {
    const f32x2_t v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}
__device__ __forceinline__ void split3_pair(float v0, float v1, uint32_t& H, uint32_t& M, uint32_t& L) {
    H = cvt_pk_bf16(v0, v1);
    const float r0 = __fsub_rn(v0, __uint_as_float(H << 16)), r1 = __fsub_rn(v1, __uint_as_float(H & 0xFFFF0000u));
    M = cvt_pk_bf16(r0, r1);
    const float q0 = __fsub_rn(r0, __uint_as_float(M << 16)), q1 = __fsub_rn(r1, __uint_as_float(M & 0xFFFF0000u));
    L = cvt_pk_bf16(q0, q1);
}

#ifdef BF3_TIMING  // tools/conv_bf3_phases.py: per-workgroup phase sums (100 MHz wall clock): prologue, staging, MFMA, epilogue
#define BF3_T() (threadIdx.x == 0 ? wall_clock64() : 0ull)
#else
#define BF3_T() 0ull
#endif

// Behind a 16-byte buffer store issued straight from computed registers: four wait states, pinned in place, before anything
// may write the store's data registers again.  The store unit reads its data a few cycles after issue, 16 lanes at a time;
// the compiler pads for that only in the cases its hazard table lists, and on this part a VALU write right behind such a
// store (scalar channel offset in soffset) was seen to land first in lanes 48-63 - one register of one store stale, once in
// a few thousand workgroups, run-to-run different (tools/dbg_fuse.py: the fused bottleneck tail against the two launches).
#ifdef BF3_NO_STORE_GUARD  // (tools/check_store_hazard.py's self-test: the checker has to find these sites unguarded)
#define BF3_STORE_GUARD() do {} while (0)
#else
#define BF3_STORE_GUARD()                       \
    do {                                        \
        __builtin_amdgcn_sched_barrier(0);      \
        asm volatile("s_nop 3" ::: "memory");   \
        __builtin_amdgcn_sched_barrier(0);      \
    } while (0)
#endif

__device__ __forceinline__ __amdgpu_buffer_rsrc_t bf3_rsrc(const void* p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, 0x00020000);
}

// ---- the product ladder.  acc[tm][tn] += a[tm] * b[tn] over their pieces, smallest products first; PRODUCT-major, tile-minor:
// a product goes to every accumulator before the next product is issued, so consecutive MFMAs hit different accumulators
// and the dependent chains of one accumulator stand TM * TN issues apart.  Operands: bf16x8, or the v4i a load left. ----
enum Bf3Products {
    BF3_SIX = 0,    // a1b3 a2b2 a3b1 a1b2 a2b1 a1b1
    BF3_THREE = 1,  // b is exact in bf16 (one-hot features, u8 maps): its lower pieces are zero - a3b1 a2b1 a1b1, the same bits
    BF3_ONE = 2,    // a1b1 alone (BF3_PROBE_NO_MFMA of tools/conv_bf3_ks_phases.py: wrong results)
};
template <int PA, int PB, int TM, int TN, typename A, typename B>
__device__ __forceinline__ void bf3_product(f32x16 (&acc)[TM][TN], const A (&a)[TM][3], const B (&b)[TN][3]) {
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[tm][PA]), __builtin_bit_cast(bf16x8, b[tn][PB]),
                                                                  acc[tm][tn], 0, 0, 0);
}
template <int MODE = BF3_SIX, int TM, int TN, typename A, typename B>
__device__ __forceinline__ void bf3_products(f32x16 (&acc)[TM][TN], const A (&a)[TM][3], const B (&b)[TN][3]) {
    if constexpr (MODE == BF3_SIX) {
        bf3_product<0, 2>(acc, a, b);
        bf3_product<1, 1>(acc, a, b);
    }
    if constexpr (MODE != BF3_ONE) bf3_product<2, 0>(acc, a, b);
    if constexpr (MODE == BF3_SIX) bf3_product<0, 1>(acc, a, b);
    if constexpr (MODE != BF3_ONE) bf3_product<1, 0>(acc, a, b);
    bf3_product<0, 0>(acc, a, b);
}
// (one channel tile per wave: acc[TN], a[3])
template <int MODE = BF3_SIX, int TN, typename A, typename B>
__device__ __forceinline__ void bf3_products(f32x16 (&acc)[TN], const A (&a)[3], const B (&b)[TN][3]) {
    // (T[N] seen as T[1][N]: the same elements at the same addresses)
    static_assert(sizeof(f32x16[1][TN]) == sizeof(f32x16[TN]) && sizeof(A[1][3]) == sizeof(A[3]), "one row of the two-dimensional form");
    bf3_products<MODE>(reinterpret_cast<f32x16(&)[1][TN]>(acc), reinterpret_cast<const A(&)[1][3]>(a), b);
}

// (... with its three weight pieces BY VALUE: k_conv1x1_bf3_ks copies them under a branch, and an array assigned under a
//  branch and read through a reference is kept as one 48-byte value - 4 VGPRs and 24 instructions more in that kernel)
template <int MODE = BF3_SIX, int TN, typename A, typename B>
__device__ __forceinline__ void bf3_products(f32x16 (&acc)[TN], const A a0, const A a1, const A a2, const B (&b)[TN][3]) {
    const A a[1][3] = {{a0, a1, a2}};
    static_assert(sizeof(f32x16[1][TN]) == sizeof(f32x16[TN]), "one row of the two-dimensional form");
    bf3_products<MODE>(reinterpret_cast<f32x16(&)[1][TN]>(acc), a, b);
}

// ---- a channel pair's pieces into the staged pixel's record: [piece][16 channels] x 2 bytes, d = record + 4 * pair ----
__device__ __forceinline__ void bf3_store_pieces(unsigned char* d, uint32_t H, uint32_t M, uint32_t L) {
    *reinterpret_cast<uint32_t*>(d) = H;
    *reinterpret_cast<uint32_t*>(d + 32) = M;
    *reinterpret_cast<uint32_t*>(d + 64) = L;
}

// ---- the aligned-group patch stager of the 2x2 / 3x3 / 7x7 kernels.  NTH threads (a workgroup, or a wave that stages its own
// patch) share the ITEMS of a 16-channel chunk; an ITEM = one aligned 16-byte group of four pixels of a patch row x one
// channel pair - two buffer_load_b128 (one per channel) through an SGPR descriptor with the chunk's channel base in the
// scalar offset.  W is a multiple of 4 and the groups start at multiples of 4 pixels of the image row, so a group lies wholly
// inside the row or wholly outside: what is outside (halo past the image, images past the batch, channels past Cin) gets an
// out-of-range offset and the hardware returns zeros - no selects, no per-element validity.  Item -> thread: the pair index
// fastest, then the group (the LDS writes of 32 lanes then hit 16 banks twice: free; a wave's loads touch whole 128-byte
// lines).  The loads are unconditional, so the compiler knows how many are in flight at every tap.
// Patch of IMGS images x PH x PWR pixels (bf3_xoff / bf3_gx0 place it on the group grid).  S2: the stride-2 3x3 conv's FOUR PHASE
// PLANES of PH x PWR = (PTH + 1) x (PTW + 1) pixels per image, staged from 2 PTH + 1 input rows.  RAGGED: Cin % 16 != 0 may occur. ----
template <int KS, int PH, int PWR, int IMGS, int NTH, bool S2 = false, bool RAGGED = true>
struct Bf3GroupStager {
    static constexpr int XOFF = bf3_xoff(KS), PLANE = PH * PWR;
    static constexpr int PROWS = S2 ? 2 * PH - 1 : PH;                                  // INPUT rows staged per image
    static constexpr int NG = S2 ? (2 * PWR + 1) / 4 + 1 : (XOFF + PWR + 3) / 4;        // 16-byte groups per input row
    static constexpr int ITEMS = IMGS * PROWS * NG * (CB / 2), NI = (ITEMS + NTH - 1) / NTH;
    static constexpr unsigned OOB = 0x80000000u;  // (>= num_records of the descriptor: the load returns zeros)
    static_assert(NTH % 8 == 0, "a thread keeps its channel pair over its items");
    unsigned ivo[NI];
    int idst[NI], imask[NI];
    int idst1[S2 ? NI : 1];  // (stride 2: the odd-column plane's base; idst is the even-column plane's)
    int qpair;
    v4i rv[NI][2];

    // tid: index among the NTH threads; the tile's first image, output row and column; pad: rows above the tile's first
    __device__ __forceinline__ void setup(const ivln_gemm_desc& p, int tid, int img0, int nimg, int ho0, int wo0, int pad) {
        const int HW = p.Hin * p.Win;
        qpair = tid & 7;
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int idx = tid + j * NTH, rest = idx >> 3;
            const int g = rest % NG, yy = rest / NG, il = IMGS == 1 ? 0 : yy / PROWS, y = yy - il * PROWS;
            // stride 2: group g of input row y = pixels wi = 2 wo0 - 4 + 4 g + e of input row 2 ho0 - 1 + y
            const int hi = S2 ? 2 * ho0 - 1 + y : ho0 - pad + y, wi = S2 ? 2 * wo0 - 4 + 4 * g : wo0 - bf3_gx0(KS) + 4 * g, img = img0 + il;
            const bool ok = idx < ITEMS && img < nimg && (unsigned)hi < (unsigned)p.Hin && wi >= 0 && wi + 3 < p.Win;
            ivo[j] = ok ? (unsigned)(((int64_t)img * p.in_img_stride + (int64_t)(2 * qpair) * HW + hi * p.Win + wi) * 4) : OOB;
            int m = 0;
            if constexpr (S2) {
                // e = 0, 2 are even columns 2 (wo0 + c): plane column c = 2 g - 2 + e / 2 (needed for c < PTW); e = 1, 3 are odd columns
                // 2 (wo0 + c) - 1: c = 2 g - 1 + e / 2 (c <= PTW).  y even = an odd row (plane row y / 2 <= PTH), y odd = an even row
                // (plane row (y - 1) / 2).
                constexpr int PTW = PWR - 1;
                const int rp = (y & 1) ^ 1, prow = y >> 1;
                const int pbase = (il * 4 + rp * 2) * PLANE + prow * PWR;
                idst[j] = (pbase + 2 * g - 2) * PIXB + qpair * 4;           // even columns: e = 0 here, e = 2 one pixel on
                idst1[j] = (pbase + PLANE + 2 * g - 1) * PIXB + qpair * 4;  // odd columns:  e = 1 here, e = 3 one pixel on
                if (idx < ITEMS) {
                    m |= ((unsigned)(2 * g - 2) < (unsigned)PTW) ? 1 : 0;
                    m |= ((unsigned)(2 * g - 1) <= (unsigned)PTW) ? 2 : 0;
                    m |= ((unsigned)(2 * g - 1) < (unsigned)PTW) ? 4 : 0;
                    m |= ((unsigned)(2 * g) <= (unsigned)PTW) ? 8 : 0;
                }
            } else {
                idst[j] = ((il * PH + y) * PWR + 4 * g - XOFF) * PIXB + qpair * 4;  // pixel e of the group: + e * PIXB
#pragma unroll
                for (int e = 0; e < 4; ++e) m |= (idx < ITEMS && (unsigned)(4 * g + e - XOFF) < (unsigned)PWR) ? (1 << e) : 0;
            }
            imask[j] = m;  // (pixels of the group outside the patch - or items past the last - are not staged)
        }
    }
    // chunk c's values into registers (a ragged last chunk reads its missing channels as zero)
    __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t rB, int c, int HW, int Cin) {
        const int so = c * CB * HW * 4;
        const unsigned hw4 = (unsigned)HW * 4u;
        const int left = Cin - c * CB;
        const bool ok0 = !RAGGED || 2 * qpair < left, ok1 = !RAGGED || 2 * qpair + 1 < left;
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            rv[j][0] = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)(ok0 ? ivo[j] : OOB), so, 0);
            rv[j][1] = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)(ok1 && !(ivo[j] & OOB) ? ivo[j] + hw4 : OOB), so, 0);
        }
    }
    // ... split and written to the patch at `base`; returns the OR of the lower pieces written (0: the values were bf16-exact)
    __device__ __forceinline__ uint32_t stage(unsigned char* base) const {
        uint32_t nz = 0;
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                uint32_t H, M, L;
                split3_pair(__int_as_float(rv[j][0][e]), __int_as_float(rv[j][1][e]), H, M, L);
                if ((imask[j] >> e) & 1) {
                    nz |= M | L;
                    bf3_store_pieces(S2 ? base + ((e & 1) ? idst1[j] : idst[j]) + (e >> 1) * PIXB : base + idst[j] + e * PIXB, H, M, L);
                }
            }
        return nz;
    }
};

// ---- the plain epilogue of four consecutive outputs of channel ch at D + addr: scale / shift or shift, residual, D +=, ReLU,
// one 16-byte store.  v comes back as stored (the tiled kernel's Welford partials read it). ----
__device__ __forceinline__ void bf3_quad_store(const ivln_gemm_desc& p, float4& v, int64_t addr, int ch) {
    if (p.scale) {
        const float sc = p.scale[ch], sh = p.shift[ch];
        v.x = fmaf(v.x, sc, sh), v.y = fmaf(v.y, sc, sh), v.z = fmaf(v.z, sc, sh), v.w = fmaf(v.w, sc, sh);
    } else if (p.shift) {
        const float sh = p.shift[ch];
        v.x += sh, v.y += sh, v.z += sh, v.w += sh;
    }
    if (p.residual) {
        const float4 rr = *reinterpret_cast<const float4*>(p.residual + addr);
        v.x += rr.x, v.y += rr.y, v.z += rr.z, v.w += rr.w;
    }
    if (p.accumulate) {
        const float4 rr = *reinterpret_cast<const float4*>(p.D + addr);
        v.x += rr.x, v.y += rr.y, v.z += rr.z, v.w += rr.w;
    }
    if (p.relu) v.x = fmaxf(v.x, 0.f), v.y = fmaxf(v.y, 0.f), v.z = fmaxf(v.z, 0.f), v.w = fmaxf(v.w, 0.f);
    *reinterpret_cast<float4*>(p.D + addr) = v;
}

// ---- K split over the waves of a workgroup: the waves' partial tiles meet in LDS as red[wave][32 channels][32 TN pixels (+4)]
// (LDT floats per channel row) and are summed over the NW waves in a FIXED order - the sum does not depend on the run.
// acc[tn][r] -> channel (r & 3) + 8 (r >> 2) + 4 half, pixel 32 tn + l31. ----
template <int LDT, int TN>
__device__ __forceinline__ void bf3_red_put(float* red, int wave, int half, int l31, const f32x16 (&acc)[TN]) {
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[(wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * LDT + tn * 32 + l31] = acc[tn][r];
}
// q = wave 0's copy of the values; V = float4 | float2: pixels of one channel row STEP floats apart (1: one LDS read of
// sizeof(V) bytes; 32: the same column of consecutive pixel tiles)
template <int NW, int LDT, typename V, int STEP = 1>
__device__ __forceinline__ V bf3_red_sum(const float* q) {
    constexpr bool QUAD = sizeof(V) == 16;
    V v;
    v.x = 0.f, v.y = 0.f;
    if constexpr (QUAD) v.z = 0.f, v.w = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const float* const qw = q + w * 32 * LDT;
        V u;
        if constexpr (STEP == 1) {
            u = *reinterpret_cast<const V*>(qw);
        } else {
            u.x = qw[0], u.y = qw[STEP];
            if constexpr (QUAD) u.z = qw[2 * STEP], u.w = qw[3 * STEP];
        }
        v.x += u.x, v.y += u.y;
        if constexpr (QUAD) v.z += u.z, v.w += u.w;
    }
    return v;
}

// ---- host: a kernel's dynamic LDS limit, raised once per kernel (idempotent; a race only repeats the call) ----
template <auto KERN>
int bf3_set_lds(size_t bytes) {
    static bool attr_done = false;
    if (!attr_done) {
        if (hipFuncSetAttribute((const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return IVLN_E_HIP;
        attr_done = true;
    }
    return IVLN_OK;
}

}  // namespace
