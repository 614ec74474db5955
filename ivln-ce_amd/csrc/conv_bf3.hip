// Direct stride-1 3x3 / 7x7 convolution with fp32 operands carried as THREE bf16 pieces each, on the bf16 MFMA pipe
// (gfx950: v_mfma_f32_32x32x16_bf16 issues 16x the FLOPs of v_mfma_f32_32x32x2_f32 per cycle).  The arithmetic and the pieces
// every kernel here shares - product ladder, record store, quad epilogue, partial tiles through LDS - are in bf3_common.h.
//
// Users: the map CNN's four 7x7 convs and their input gradients (map_encoder.py:8-97 under base_il_trainer.py:173-219),
// RedNet's 3x3 convs (rednet.py:190-358).  Data flow per workgroup (512 threads = 8 waves, 2 per SIMD):
//   * tile = BM output channels x BN output pixels (IMGS images x PTH x PTW), waves WM x WN, wave tile (32 TM) x 64;
//   * the input patch of 16 channels is staged ONCE per chunk in LDS, already split, channel-last: a pixel is a 112-byte
//     record [piece][16 channels] (28 words: the 16 lanes of a ds_read_b128 phase hit 16 distinct bank quads), so an
//     operand fetch for tap (kh, kw) is `ds_read_b128 v, base offset:imm` with a per-lane base that never changes;
//   * the weights arrive split and in the MFMA's per-lane order from ivln_conv_split_weights_f32 and stream global ->
//     registers, DA taps ahead, through a buffer resource (loads through a plain pointer are sunk to their first use);
//   * the next chunk's patch values fly under the MFMA phase (registers), are split and written after the barrier;
//   * epilogue through LDS in slabs of 32 channels: 16-byte stores along the pixel index with the fused scale / shift /
//     residual / ReLU of ivln_gemm_f32 and the per-(128-pixel segment, channel) Welford partials of stat_partials.
#include <stdlib.h>

#include <type_traits>

#include "bf3_common.h"
#include "residency.h"
#include "../../include/ivln_conv_ks_waves.h"

namespace {

#ifdef BF3_TIMING  // tools/conv_bf3_phases.py: per-workgroup phase sums (BF3_T of bf3_common.h)
__device__ unsigned long long g_bf3_stamp[8192 * 8];  // records of 8 words
#endif

// ST = 2 (round 6): the stride-2 3x3 convs of RedNet's layer 2-4 entry blocks (rednet.py:84-110, pad 1, Hin = 2 Hout).  Output
// (ho, wo) reads input rows 2 ho - 1 .. 2 ho + 1: the patch is staged as FOUR PHASE PLANES - (row parity, column parity) of the
// input pixel, each (PTH + 1) x (PTW + 1) pixels per image - so that tap (kh, kw) is plane (kh != 1, kw != 1) at offset
// ((kh == 2), (kw == 2)): a compile-time LDS offset per tap, and a lane's base address depends on its output pixel only,
// exactly as in the stride-1 kernel.  Odd input rows 2 i - 1 are plane row i (i = 0 .. PTH), even rows 2 i plane row i.
template <int KS, int TM, int WM, int WN, int PTH, int PTW, int IMGS, int DA, bool FUSE = false, int ST = 1>
__global__ __launch_bounds__(64 * WM * WN, 2) void k_conv_bf3(const ivln_gemm_desc p, const unsigned char* a_split, long long a_grp_bytes,
                                                           int tiles_w, int tiles_h, int nimg, int chunks_per_split) {
#ifdef BF3_TIMING
    const unsigned long long t_entry = threadIdx.x == 0 ? wall_clock64() : 0ull;
#endif
    constexpr int NTB = 64 * WM * WN, TN = 2;
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    static_assert(IMGS * PTH * PTW == BN && PTW % 4 == 0, "pixel tile");
    constexpr int KK = KS * KS, KKP = bf3_taps_padded(KS), CS = bf3_stage_chunks(KS);
    constexpr int RP = KKP * CS;  // taps (padded) between two barriers: a STAGE = CS chunks of 16 channels
    static_assert(RP % DA == 0 && KKP >= KK && (CS == 1 || KK == 1), "prefetch rotation closes over a stage");
    static_assert(ST == 1 || (ST == 2 && KS == 3 && !FUSE), "stride 2: the 3x3 kernel only");
    constexpr bool S2 = ST == 2;
    // stride 1: PH x PWR patch pixels per image.  stride 2: four planes of PH x PWR = (PTH + 1) x (PTW + 1) each
    constexpr int PH = S2 ? PTH + 1 : PTH + KS - 1, PWR = S2 ? PTW + 1 : PTW + KS - 1;
    constexpr int PLANE = PH * PWR, NPIX = IMGS * (S2 ? 4 : 1) * PLANE;
    constexpr int ITEMS = NPIX * (CB / 2) * CS;
    constexpr int LDT = BN + 4;
    constexpr bool HAS_LITE = KS == 7 && TM == 1;  // (a second copy of the unrolled tap loop: only where one-hot inputs occur)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);  // (uniform: the weight stream's buffer resource lives in SGPRs)
    const int half = lane >> 5, l31 = lane & 31;
    const int wm = wave / WN, wn = wave % WN;
    const BlockId bid = xcd_block_id(p.no_xcd_remap);
    const int bx = bid.x;
    const int tw = bx % tiles_w, th = (bx / tiles_w) % tiles_h, ig = bx / (tiles_w * tiles_h);
    const int img0 = ig * IMGS, ho0 = th * PTH, wo0 = tw * PTW;
    const int m0 = bid.y * BM;
    const int nch = (p.Cin + CB - 1) / CB;
    const int HW = p.Hin * p.Win;
    const int grp = p.grp_imgs > 0 ? img0 / p.grp_imgs : 0;

    // Staging work of a thread.
    // 3x3 / 7x7 / 2x2: its items of the aligned-group scheme (Bf3GroupStager; stride 2: into the four phase planes).  The loads
    // being unconditional, the compiler knows how many are in flight at every tap: the first version's
    // `if (c + 1 < c_end) load_patch` made it wait for the NEXT chunk's patch (an HBM round trip) at the first tap of every
    // chunk (s_waitcnt vmcnt(13) with 50 loads in flight).
    // 1x1 (CS chunks per stage, no halo): the flat (pixel, pair) enumeration with offsets re-derived per stage.
    constexpr bool UP = KS == 2;                     // rows = 4 * channel + parity class, stores into the (2 H x 2 W) output
    constexpr unsigned OOB = 0x80000000u;            // (>= num_records of the descriptor: the load returns zeros)
    Bf3GroupStager<KS, PH, PWR, IMGS, NTB, S2, !S2> gs;  // (1x1: unused; stride 2: the launcher insists on whole 16-channel chunks)
    if constexpr (KS != 1) gs.setup(p, t, img0, nimg, ho0, wo0, p.pad);
    const __amdgpu_buffer_rsrc_t rB = bf3_rsrc(p.B);
    // 1x1: the patch is the output tile itself (no halo, maybe strided); NTB / NPIX thread groups share a pixel set and take
    // every (NTB / NPIX)-th chunk of the stage, all 8 channel pairs of each
    constexpr int NPI = KS == 1 ? ITEMS / NTB : 1;
    constexpr int G1 = KS == 1 ? NTB / NPIX : 1;
    static_assert(KS != 1 || (NTB % NPIX == 0 && CS % G1 == 0), "1x1: whole thread groups per pixel set");
    int src1 = -1, dst1 = 0, g1 = 0;
    if constexpr (KS == 1) {
        const int pix = t % NPIX;
        g1 = t / NPIX;
        const int il = pix / (PH * PWR), rem = pix - il * (PH * PWR);
        const int y = rem / PWR, x = rem - y * PWR;
        const int hi = (ho0 + y) * p.stride, wi = (wo0 + x) * p.stride, img = img0 + il;
        const bool ok = img < nimg && (unsigned)hi < (unsigned)p.Hin && (unsigned)wi < (unsigned)p.Win;
        src1 = ok ? (int)((int64_t)img * p.in_img_stride + hi * p.Win + wi) : -1;
        dst1 = pix * PIXB;
    }
    float r0[NPI], r1[NPI];
    auto load_patch = [&](int c) {
        if constexpr (KS == 1) {
            const int cbase = c * (CB * CS) * HW;
            const int left = p.Cin - c * (CB * CS);  // channels this stage still has (ragged last chunk: the rest reads as zero)
#pragma unroll
            for (int jj = 0; jj < CS / G1; ++jj)
#pragma unroll
                for (int q = 0; q < CB / 2; ++q) {
                    const int ch = (g1 + jj * G1) * CB + 2 * q;  // channel of the pair inside the stage
                    const bool ok0 = src1 >= 0 && ch < left, ok1 = src1 >= 0 && ch + 1 < left;
                    const int o = src1 + cbase + ch * HW;
                    r0[jj * (CB / 2) + q] = p.B[ok0 ? o : 0];
                    r1[jj * (CB / 2) + q] = p.B[ok1 ? o + HW : 0];
                }
        } else {
            gs.load(rB, c, HW, p.Cin);
        }
    };
    auto stage = [&](int c) -> uint32_t {  // returns the OR of the lower pieces this thread wrote (0: its values were bf16-exact)
        if constexpr (KS == 1) {
            uint32_t nz = 0;
            const int left = p.Cin - c * (CB * CS);
#pragma unroll
            for (int jj = 0; jj < CS / G1; ++jj)
#pragma unroll
                for (int q = 0; q < CB / 2; ++q) {
                    const int ch = (g1 + jj * G1) * CB + 2 * q;
                    const float v0 = (src1 >= 0 && ch < left) ? r0[jj * (CB / 2) + q] : 0.f;
                    const float v1 = (src1 >= 0 && ch + 1 < left) ? r1[jj * (CB / 2) + q] : 0.f;
                    uint32_t H, M, L;
                    split3_pair(v0, v1, H, M, L);
                    nz |= M | L;
                    bf3_store_pieces(smem + (g1 + jj * G1) * (NPIX * PIXB) + dst1 + q * 4, H, M, L);
                }
            return nz;
        } else {
            return gs.stage(smem);
        }
    };

    // per-lane operand bases
    int bbase[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int nl = (wn * TN + tn) * 32 + l31;
        const int il = nl / (PTH * PTW), ph = (nl / PTW) % PTH, pw = nl % PTW;
        bbase[tn] = ((il * (S2 ? 4 : 1) * PH + ph) * PWR + pw) * PIXB + half * 16;  // (stride 2: plane (0, 0) of the image; the tap adds its plane)
    }
    // weights: [32-channel tile][chunk][tap (padded)][piece][lane] x 16 bytes
    __amdgpu_buffer_rsrc_t rA[TM];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
        const int mt = min(m0 / 32 + wm * TM + tm, (p.M + 31) / 32 - 1);  // (a channel tile past M reads the last one's weights; its rows are never stored)
        rA[tm] = bf3_rsrc(a_split + (int64_t)grp * a_grp_bytes + (int64_t)mt * nch * KKP * (3 * 1024));
    }
    const int nst = (nch + CS - 1) / CS;  // stages
    const int c_beg = bid.z * chunks_per_split, c_end = min(nst, c_beg + chunks_per_split);  // (split K: stages over blockIdx.z)
    const int steps = nch * KKP;
    auto load_a = [&](int tm, int s, int pl) -> v4i {
        const int sc = s < steps ? s : steps - 1;
        return __builtin_amdgcn_raw_buffer_load_b128(rA[tm], (sc * 3 + pl) * 1024 + lane * 16, 0, 0);
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[tm][tn][i] = 0.f;

    v4i abuf[DA][TM][3];
#pragma unroll
    for (int d = 0; d < DA; ++d)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) abuf[d][tm][pl] = load_a(tm, c_beg * RP + d, pl);

    unsigned long long tk0 = BF3_T(), t_stage = 0, t_mma = 0;
    (void)tk0, (void)t_stage, (void)t_mma;
#ifdef BF3_TIMING
    const unsigned long long cyc0 = clock64();
#endif
    load_patch(c_beg);
    for (int c = c_beg; c < c_end; ++c) {
        const unsigned long long ta = BF3_T();
        const uint32_t nz = stage(c);
        // A chunk whose staged values are all bf16-exact (one-hot map features: the map CNN's first layer) has zero second and
        // third pieces: the three products against them are exact zeros and are not issued - same bits, half the MFMAs and a
        // third of the operand reads.  The block-wide OR rides in the barrier the staging needs anyway.
        const bool lite = HAS_LITE ? __syncthreads_or((int)(nz != 0)) == 0 : (__syncthreads(), false);
        const unsigned long long tb = BF3_T();
        t_stage += tb - ta;
        // The next chunk's patch flies under the MFMA phase.  Unconditional (the last chunk re-loads itself, six loads nobody
        // reads): with a branch around it the compiler cannot count the loads in flight and waits for ALL of them at the first
        // tap.  3x3 / 7x7: issued PATCH_TAP taps into the phase, ~3 us of MFMA work before the staging pass that reads them -
        // the weight loads of the taps in between (waited for in order, a tap after tap) then never queue behind an HBM miss.
        constexpr int PATCH_TAP = KS == 1 ? -1 : (KK - (TM == 2 ? 4 : 8) > 0 ? KK - (TM == 2 ? 4 : 8) : 0);
        if constexpr (KS == 1) load_patch(c + 1 < c_end ? c + 1 : c);
        const int s0 = c * RP;
        auto taps = [&](auto lite_tag) {
            constexpr bool LITE = decltype(lite_tag)::value;
            constexpr int NPL = LITE ? 1 : 3;
            auto read_b = [&](int r, bf16x8 (&b)[TN][3]) {  // the tap's B fragments: one ds_read_b128 per (pixel tile, piece)
                const int kh = r / KS, kw = r - kh * KS;
                const int toff = KS == 1 ? r * (NPIX * PIXB)  // (1x1: tap r = chunk r of the stage)
                                 : (S2 ? ((((kh != 1) * 2 + (kw != 1)) * PLANE + (kh == 2) * PWR + (kw == 2)) * PIXB) : (kh * PWR + kw) * PIXB);
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                    for (int pl = 0; pl < NPL; ++pl)
                        b[tn][pl] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const v4i*>(smem + bbase[tn] + toff + pl * 32));
            };
            bf16x8 bq[2][TN][3];  // this tap's fragments and the next tap's, read while this tap's MFMAs issue
            read_b(0, bq[0]);
#pragma unroll
            for (int r = 0; r < RP; ++r) {
                const int slot = r % DA;
                if (r < KK * CS && (KS != 1 || c * CS + r < nch)) {  // (padding taps, and 1x1: chunks past the last one, issue nothing)
                    if (r + 1 < KK * CS) read_b(r + 1, bq[(r + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);  // (the reads stay AHEAD of this tap's MFMAs: left alone they sink to their use)
                    bf3_products<LITE ? BF3_THREE : BF3_SIX>(acc, abuf[slot], bq[r & 1]);
                }
                __builtin_amdgcn_sched_barrier(0);
                // the slot just used receives the weights of DA taps ahead (the rotation closes over the stage: RP % DA == 0)
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) abuf[slot][tm][pl] = load_a(tm, s0 + r + DA, pl);
                if (r == PATCH_TAP) load_patch(min(c + 1, c_end - 1));  // (behind this tap's weight loads: every wait of this chunk is for loads older than these)
                __builtin_amdgcn_sched_barrier(0);  // (... and so do the weight loads: DA taps of flight time, not one)
            }
        };
        if constexpr (HAS_LITE) {
            if (lite) taps(std::true_type{});
            else taps(std::false_type{});
        } else {
            taps(std::false_type{});
        }
        __syncthreads();
        t_mma += BF3_T() - tb;
    }
    const unsigned long long tk1 = BF3_T();
    (void)tk1;

    // ---- FUSE: the bottleneck's 1x1 expansion behind this 3x3 conv, in the same launch (ivln_gemm_desc.fuse_*).  The workgroup
    // holds ALL of the conv's channels (M == BM) for its 128 pixels:
    //   1. y = ReLU(scale * acc + shift) goes to LDS as fp32 [channel][pixel of the tile] - over the patch, which is dead;
    //   2. every wave then runs the wave-tile 1x1 kernel's loop (k_conv1x1_bf3_ks<true>) on it for the 32-channel tiles
    //      wave, wave + 4, ... of the fuse_M outputs: a lane reads four consecutive pixels of a channel (one ds_read_b128 where
    //      that kernel issues a buffer load), builds the B fragments in registers, streams the 1x1 weights global -> registers;
    //   3. and stores its tile straight from the accumulators (register r of the four tiles = a float4 along the pixel index)
    //      with the folded bn3, the residual and the ReLU.
    // Same arithmetic, same order per accumulator as the two separate launches; the planes-channel tensor never leaves the CU
    // (written + read once per block before: 2 x 4 B x planes x pixels), one launch and one prologue / epilogue less. ----
    if constexpr (FUSE) {
        static_assert(KS == 3 && IMGS == 1 && PTW == 32 && (BN == 128 || BN == 64) && NTB == 256, "the fused tail is built for the 4 x 32 and 2 x 32 pixel tiles");
        constexpr int Q = BN / 32;  // consecutive pixels of a lane in the second stage = pixel tiles of its B fragments (4 | 2)
        constexpr int LDY = BN + 4;
        float* const Y = reinterpret_cast<float*>(smem);
        {
            const __amdgpu_buffer_rsrc_t rS = bf3_rsrc(p.scale), rH = bf3_rsrc(p.shift);
            const int me0 = grp * p.M + m0 + 4 * half;
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int cl = 32 * (wm * TM + tm) + (r & 3) + 8 * (r >> 2);  // (+ 4 half: in me0 / below)
                    const float sc = p.scale ? __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rS, me0 * 4, cl * 4, 0)) : 1.f;
                    const float sh = p.shift ? __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rH, me0 * 4, cl * 4, 0)) : 0.f;
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn) {
                        float v = acc[tm][tn][r];
                        v = p.scale ? fmaf(v, sc, sh) : v + sh;
                        if (p.relu) v = fmaxf(v, 0.f);
                        Y[(cl + 4 * half) * LDY + (wn * TN + tn) * 32 + l31] = v;
                    }
                }
        }
        __syncthreads();
        constexpr int NCH2 = BM / CB, DA2 = 2;
        const int ntile2 = p.fuse_M / 32;
        // this lane's pixels: tile-linear Q l31 .. + Q - 1 = row Q l31 / 32 of the tile, columns (Q l31) % 32 ..
        const int ph = (Q * l31) >> 5, pw = (Q * l31) & 31;
        const int ho = ho0 + ph, wo = wo0 + pw;
        const bool pix_ok = img0 < nimg && ho < p.Hout && wo < p.Wout;
        const unsigned char* const a2 = reinterpret_cast<const unsigned char*>(p.fuse_A_split) + (int64_t)grp * p.fuse_a_grp_stride * 4;
        const __amdgpu_buffer_rsrc_t rR = bf3_rsrc(p.residual), rS3 = bf3_rsrc(p.fuse_scale), rH3 = bf3_rsrc(p.fuse_shift), rD = bf3_rsrc(p.D);
        const bool has_res = p.residual != nullptr, has_sc = p.fuse_scale != nullptr, has_sh = p.fuse_shift != nullptr;
        const float* const yl = Y + (8 * half) * LDY + Q * l31;
        for (int mt = wave; mt < ntile2; mt += NTB / 64) {
            const __amdgpu_buffer_rsrc_t rA2 = bf3_rsrc(a2 + (int64_t)mt * NCH2 * 3072);
            auto load_a2 = [&](int c, v4i (&ab)[3]) {
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) ab[pl] = __builtin_amdgcn_raw_buffer_load_b128(rA2, (min(c, NCH2 - 1) * 3 + pl) * 1024 + lane * 16, 0, 0);
            };
            v4i ab[DA2][3];
#pragma unroll
            for (int d = 0; d < DA2; ++d) load_a2(d, ab[d]);
            // the tile's epilogue operands, requested before its K loop
            const int mch = mt * 32 + 4 * half;
            const int me3 = grp * p.fuse_M + mch;
            const unsigned off0 = (unsigned)((((int64_t)img0 * p.Ctot + mch) * p.HoWo + ho * p.Wout + wo) * 4);
            float rres[16][Q];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ro = pix_ok && has_res ? (int)off0 : (int)OOB, so = ((r & 3) + 8 * (r >> 2)) * p.HoWo * 4;
                if constexpr (Q == 4) {
                    const v4i t4 = __builtin_amdgcn_raw_buffer_load_b128(rR, ro, so, 0);
#pragma unroll
                    for (int e = 0; e < Q; ++e) rres[r][e] = __int_as_float(t4[e]);
                } else {
                    const v2i t2 = __builtin_amdgcn_raw_buffer_load_b64(rR, ro, so, 0);
#pragma unroll
                    for (int e = 0; e < Q; ++e) rres[r][e] = __int_as_float(t2[e]);
                }
            }
            f32x16 acc2[Q];
#pragma unroll
            for (int e = 0; e < Q; ++e)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc2[e][i] = 0.f;
#pragma unroll
            for (int c = 0; c < NCH2; ++c) {
                v4i bq[Q][3];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float x0[Q], x1[Q];
                    if constexpr (Q == 4) {
                        const v4i t0 = *reinterpret_cast<const v4i*>(yl + (c * CB + 2 * i) * LDY), t1 = *reinterpret_cast<const v4i*>(yl + (c * CB + 2 * i + 1) * LDY);
#pragma unroll
                        for (int e = 0; e < Q; ++e) x0[e] = __int_as_float(t0[e]), x1[e] = __int_as_float(t1[e]);
                    } else {
                        const v2i t0 = *reinterpret_cast<const v2i*>(yl + (c * CB + 2 * i) * LDY), t1 = *reinterpret_cast<const v2i*>(yl + (c * CB + 2 * i + 1) * LDY);
#pragma unroll
                        for (int e = 0; e < Q; ++e) x0[e] = __int_as_float(t0[e]), x1[e] = __int_as_float(t1[e]);
                    }
#pragma unroll
                    for (int e = 0; e < Q; ++e) {
                        uint32_t H, M, L;
                        split3_pair(x0[e], x1[e], H, M, L);
                        bq[e][0][i] = (int)H, bq[e][1][i] = (int)M, bq[e][2][i] = (int)L;
                    }
                }
                bf16x8 a[3];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) a[pl] = __builtin_bit_cast(bf16x8, ab[c % DA2][pl]);
                __builtin_amdgcn_sched_barrier(0);
                load_a2(c + DA2, ab[c % DA2]);
                __builtin_amdgcn_sched_barrier(0);
                bf3_products(acc2, a, bq);
            }
            // (the folded bn3 of the tile's channels: 8 x 16 bytes per lane, L2-resident after the first workgroups - asked for
            //  here, not before the K loop, because 32 more live registers there spill)
            v4i esc4[4], esh4[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                esc4[g] = __builtin_amdgcn_raw_buffer_load_b128(rS3, has_sc ? me3 * 4 : (int)OOB, g * 32, 0);
                esh4[g] = __builtin_amdgcn_raw_buffer_load_b128(rH3, has_sh ? me3 * 4 : (int)OOB, g * 32, 0);
            }
            // (not bf3_quad_store: operands in registers before the K loop, straight-line code between scalar-offset buffer stores)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int cs = (r & 3) + 8 * (r >> 2);
                float v[Q];
#pragma unroll
                for (int e = 0; e < Q; ++e) v[e] = acc2[e][r];
                // STRAIGHT-LINE code between the stores (absent scale = 1, absent shift / residual = the zeros the out-of-range
                // loads returned): a 16-byte buffer store with a scalar offset reads its data registers a few cycles after
                // it issues, the compiler's hazard recognizer pads for that inside a basic block, and with uniform branches
                // here it let a VALU write follow the store across a block boundary - lanes 48-63 of one register of one store
                // stale, once in a few thousand workgroups (found by tools/dbg_fuse.py against the two-launch path).
                const float sc = has_sc ? __int_as_float(esc4[r >> 2][r & 3]) : 1.f, sh = __int_as_float(esh4[r >> 2][r & 3]);
#pragma unroll
                for (int e = 0; e < Q; ++e) v[e] = fmaxf(fmaf(v[e], sc, sh) + rres[r][e], 0.f);  // (bn3, residual, the block's closing ReLU)
                if constexpr (Q == 4) {
                    v4i o;
#pragma unroll
                    for (int e = 0; e < Q; ++e) o[e] = __float_as_int(v[e]);
                    __builtin_amdgcn_raw_buffer_store_b128(o, rD, pix_ok ? (int)off0 : (int)OOB, cs * p.HoWo * 4, 0);
                } else {
                    v2i o;
#pragma unroll
                    for (int e = 0; e < Q; ++e) o[e] = __float_as_int(v[e]);
                    __builtin_amdgcn_raw_buffer_store_b64(o, rD, pix_ok ? (int)off0 : (int)OOB, cs * p.HoWo * 4, 0);
                }
                BF3_STORE_GUARD();
            }
        }
        return;
    }

    // ---- epilogue: slabs of 32 channels through LDS.  acc[r] -> channel (r&3) + 8*(r>>2) + 4*half, pixel l31 ----
    float* T = reinterpret_cast<float*>(smem);
    for (int slab = 0; slab < TM * WM; ++slab) {
        const int sw = slab / TM, stm = slab - sw * TM;
        if (wm == sw) {
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
                if (tm == stm)
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            T[((r & 3) + 8 * (r >> 2) + 4 * half) * LDT + (wn * TN + tn) * 32 + l31] = acc[tm][tn][r];
        }
        __syncthreads();
        const int mbase = m0 + slab * 32;
        if constexpr (UP) {
            // the slab's 32 rows = 8 channels x 4 parity classes; rows 4 c + 2 a (b = 0) and + 1 (b = 1) x two horizontally
            // adjacent pixels of the tile = four consecutive floats of output row 2 ho + a: one 16-byte store per
            // (channel, a, pixel pair), whole 64-byte segments of the (2 H x 2 W) tensor (gemm_common.h: up2x4_wide_store)
            for (int idx = t; idx < 16 * (BN / 2); idx += NTB) {
                const int r = idx / (BN / 2), j = idx - r * (BN / 2);  // r = 2 * (channel of the slab) + a
                const int ml = 2 * r, nl = 2 * j;
                const int il = nl / (PTH * PTW), ph = (nl / PTW) % PTH, pw = nl % PTW;
                const int img = img0 + il, ho = ho0 + ph, wo = wo0 + pw;
                if (mbase + ml >= p.M || img >= nimg || ho >= p.Hout || wo >= p.Wout) continue;  // (M % 4 == 0, Wout % 4 == 0: in or out whole)
                const int co = (mbase + ml) >> 2, a = r & 1;
                const int64_t addr = (((int64_t)img * p.Ctot + co) * (2 * p.Hout) + 2 * ho + a) * (2 * p.Wout) + 2 * wo;
                const float2 t0 = *reinterpret_cast<const float2*>(T + ml * LDT + nl);
                const float2 t1 = *reinterpret_cast<const float2*>(T + (ml + 1) * LDT + nl);
                float4 v = make_float4(t0.x, t1.x, t0.y, t1.y);
                bf3_quad_store(p, v, addr, co);
            }
            __syncthreads();
            continue;
        }
        for (int idx = t; idx < 32 * (BN / 4); idx += NTB) {
            const int ml = idx / (BN / 4), c4 = idx - ml * (BN / 4);
            const int m = mbase + ml;
            const int nl = 4 * c4;
            const int il = nl / (PTH * PTW), ph = (nl / PTW) % PTH, pw = nl % PTW;
            const int img = img0 + il, ho = ho0 + ph, wo = wo0 + pw;
            const bool ok = m < p.M && img < nimg && ho < p.Hout && wo < p.Wout;  // (Wout % 4 == 0: a quad is in or out whole)
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok && p.splits > 1) {  // (uniform) raw partial sums of this channel range: slab [split][M][N], reduced by k_splitk_epilogue
                v = *reinterpret_cast<const float4*>(T + ml * LDT + nl);
                *reinterpret_cast<float4*>(p.ws + ((int64_t)bid.z * p.M + m) * p.N + (int64_t)img * p.HoWo + ho * p.Wout + wo) = v;
            } else if (ok) {
                v = *reinterpret_cast<const float4*>(T + ml * LDT + nl);
                const int64_t addr = ((int64_t)img * p.Ctot + m) * p.HoWo + ho * p.Wout + wo;
                bf3_quad_store(p, v, addr, p.grp_imgs > 0 ? (img / p.grp_imgs) * p.M + m : m);
            }
            if (p.stat_partials) {  // (uniform) {count, mean, M2} of the 128 pixels a half-wave just stored
                float cnt = ok ? 4.f : 0.f, sum = ok ? (v.x + v.y) + (v.z + v.w) : 0.f;
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o), sum += __shfl_xor(sum, o);
                const float mean = cnt > 0.f ? sum / cnt : 0.f;
                const float d0 = v.x - mean, d1 = v.y - mean, d2 = v.z - mean, d3 = v.w - mean;
                float q = ok ? (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3) : 0.f;
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) q += __shfl_xor(q, o);
                if ((t & 31) == 0 && m < p.M) {
                    float* st = p.stat_partials + ((int64_t)(bx * (BN / 128) + c4 / 32) * p.M + m) * 3;
                    st[0] = cnt, st[1] = mean, st[2] = q;
                }
            }
        }
        __syncthreads();
    }
#ifdef BF3_TIMING
    if (threadIdx.x == 0) {
        const int b = (blockIdx.y * gridDim.x + blockIdx.x) & 8191;
        g_bf3_stamp[b * 8 + 0] = tk1 - tk0;
        g_bf3_stamp[b * 8 + 1] = t_stage;
        g_bf3_stamp[b * 8 + 2] = t_mma;
        g_bf3_stamp[b * 8 + 3] = clock64() - cyc0;  // shader cycles over the whole kernel: with [0] + epilogue wall time, the clock it ran at
        g_bf3_stamp[b * 8 + 4] = t_entry;
        g_bf3_stamp[b * 8 + 5] = tk0;
        __builtin_amdgcn_s_waitcnt(0);
        g_bf3_stamp[b * 8 + 6] = wall_clock64();
    }
#endif
}

// ------------------------------------------------------------------------------------------------------------------
// The same arithmetic for the PIXEL-STARVED deep 3x3 convs (RedNet's layers 3-4 and the decoder's first stages,
// rednet.py:190-263: 128-512 channels on 8x8 ... 32x32 maps, N = 512 ... 8192 pixels, K = 1152 ... 4608): round 5.
// The tiled kernel above fills the chip there only by splitting K over blockIdx.z - two or three 16-channel chunks per
// workgroup between a prologue and a slab epilogue, then a reduction launch: 30 us + 6.5 us for 2.4 GFLOP.  Here K is split
// over the WAVES of a workgroup instead:
//   * a workgroup (8 waves) owns 32 output channels x 64 output pixels (a whole 8x8 image, 4 rows of a 16-wide or 2 rows of
//     a 32-wide one) over the WHOLE K; wave w takes the contiguous range [w, w + 1) * ceil(nch / 8) of the 16-channel chunks;
//   * everything a wave needs is wave-private: its chunk's input patch is loaded (aligned 16-byte buffer loads, zeros from
//     out-of-range offsets - the scheme of the tiled kernel), split into the three bf16 pieces and written to ITS region of
//     LDS, its weight stream comes global -> registers three taps ahead.  No workgroup barrier inside the K loop: LDS
//     accesses of one wave execute in program order, so the waves run free of each other and hide one another's latencies;
//   * at the end the eight partial tiles meet in LDS (a barrier, 8 x 8 KB, aliasing the patch regions), every thread sums
//     four outputs over the waves in a fixed order and applies the fused epilogue of ivln_gemm_f32: no slabs, no reduction
//     launch, the same bits on every run.
// L2 -> CU traffic is the price: every workgroup streams its 32 channels' weights for the whole K (885 KB at K = 4608).
// ------------------------------------------------------------------------------------------------------------------
// KS = 2: the same kernel for the stacked parity classes of a stride-2 3x3 transposed conv over few pixels (the decoder's first
// upsampling stages, rednet.py:152-181 at 8 x 8 and 16 x 16): rows = 4 * channel + class, a 2 x 2 window, and an epilogue that
// stores 2 x 2 output blocks (IVLN_D_NCHW_UP2X4).
// NW = 4 (two workgroups of four waves on a CU instead of two rounds of one eight-wave workgroup: DESIGN.md section 3,
// "co-resident K-split workgroups"): the same K over four waves, twice the chunks per wave, half the LDS - for the grids
// with more workgroups than CUs and at most twice as many, where every workgroup then starts at once and a CU pays the
// prologue, the reduction barrier and the epilogue once.  The K loop is the same code; the sum over K is four partial
// tiles in a fixed order (not bit-equal to NW = 8).
template <int PTH, int PTW, int TN = 2, int KS = 3, int NW = 8>
__global__ __launch_bounds__(64 * NW, 2) void k_conv_bf3_ks(const ivln_gemm_desc p, const unsigned char* a_split, long long a_grp_bytes,
                                                        int tiles_w, int tiles_h, int nimg) {
    // DA: weight taps in flight.  A tap is only 12 MFMAs here (384 pipe cycles, 768 with the SIMD's other wave): three taps
    // ahead were ~1 us of cover against an L2 round trip of 1-2 us under load - every tap waited (first version: 28 us for
    // 512 x 512 x 4608 with 13 us of MFMA issue).  A whole chunk ahead (9 taps, 108 registers) covers it.
    // TN = 1 (32 pixels per workgroup): the launches that fill less than half the chip with 64-pixel tiles (512 x 512 x 4608:
    // 128 workgroups) - twice the workgroups, half the MFMAs per wave, 20 % more halo per output.
    constexpr int KK = KS * KS, DA = KK, BS = 64 * NW;
    constexpr bool UP = KS == 2;
    static_assert(PTH * PTW == 32 * TN && (KS == 3 || KS == 2) && (NW == 8 || NW == 4), "32 TN pixels per workgroup, 8 or 4 waves");
    constexpr int PH = PTH + KS - 1, PWR = PTW + KS - 1, NPIX = PH * PWR;
    constexpr int WREG = (NPIX * PIXB + 15) & ~15;  // bytes of a wave's patch region
    constexpr int LDT = 32 * TN + 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const BlockId bid = xcd_block_id(p.no_xcd_remap);
    const int bx = bid.x;
    const int tw = bx % tiles_w, th = (bx / tiles_w) % tiles_h, img0 = bx / (tiles_w * tiles_h);
    const int ho0 = th * PTH, wo0 = tw * PTW;
    const int m0 = bid.y * 32;
    const int nch = p.Cin / CB;
    const int HW = p.Hin * p.Win;
    const int grp = p.grp_imgs > 0 ? img0 / p.grp_imgs : 0;
    const int cpw = (nch + NW - 1) / NW;
    const int c0 = min(nch, wave * cpw), c1 = min(nch, c0 + cpw);
    unsigned char* const wsm = smem + wave * WREG;

    // the wave stages its own patch: the items of a LANE (pad 1 | the 2 x 2 window starts at the pixel itself)
    Bf3GroupStager<KS, PH, PWR, 1, 64, false, false> gs;
    gs.setup(p, lane, img0, nimg, ho0, wo0, KS == 3 ? 1 : 0);
    const __amdgpu_buffer_rsrc_t rB = bf3_rsrc(p.B);
    int bbase[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int nl = tn * 32 + l31, ph = nl / PTW, pw = nl % PTW;
        bbase[tn] = (ph * PWR + pw) * PIXB + half * 16;
    }
    const int mt = min(m0 / 32, (p.M + 31) / 32 - 1);
    const __amdgpu_buffer_rsrc_t rA = bf3_rsrc(a_split + (int64_t)grp * a_grp_bytes + (int64_t)mt * nch * KK * (3 * 1024));
    const int s_last = max(c1 * KK - 1, 0);
    auto load_a = [&](int s_, int pl) -> v4i {
        return __builtin_amdgcn_raw_buffer_load_b128(rA, (min(s_, s_last) * 3 + pl) * 1024 + lane * 16, 0, 0);
    };
    f32x16 acc[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[tn][i] = 0.f;

#ifdef BF3_TIMING
    const unsigned long long ts0 = lane == 0 ? wall_clock64() : 0ull;
    unsigned long long ts1 = ts0, t_stage = 0;
#endif
    if (c0 < c1) {
        v4i abuf[DA][3];
#pragma unroll
        for (int d = 0; d < DA; ++d)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) abuf[d][pl] = load_a(c0 * KK + d, pl);
        gs.load(rB, c0, HW, p.Cin);
#ifdef BF3_TIMING
        __builtin_amdgcn_s_waitcnt(0);  // (timing build only: the prologue's round trip as a phase of its own)
        ts1 = lane == 0 ? wall_clock64() : 0ull;
#endif
        for (int c = c0; c < c1; ++c) {
#ifdef BF3_TIMING
            const unsigned long long tsa = lane == 0 ? wall_clock64() : 0ull;
#endif
            gs.stage(wsm);
#ifdef BF3_TIMING
            __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
            t_stage += (lane == 0 ? wall_clock64() : 0ull) - tsa;
#endif
            const int s0 = c * KK;
            auto read_b = [&](int r, bf16x8 (&b)[TN][3]) {
                const int kh = r / KS, kw = r - kh * KS, toff = (kh * PWR + kw) * PIXB;
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl)
                        b[tn][pl] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const v4i*>(wsm + bbase[tn] + toff + pl * 32));
            };
            bf16x8 bq[2][TN][3];
            read_b(0, bq[0]);
#pragma unroll
            for (int r = 0; r < KK; ++r) {
                const int slot = r % DA;
                if (r + 1 < KK) read_b(r + 1, bq[(r + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
                bf3_products(acc, abuf[slot], bq[r & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) abuf[slot][pl] = load_a(s0 + r + DA, pl);
                if (r == (KK > 4 ? 1 : 0)) gs.load(rB, min(c + 1, c1 - 1), HW, p.Cin);  // (next chunk's patch: 7 | 3 taps of MFMA work before the staging pass reads it)
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    // ---- the NW partial tiles meet in LDS: red[wave][32 channels][64 pixels (+4)] over the patch regions (a wave with an empty
    // slice brings zeros); the items below go over the workgroup's 64 NW threads in passes ----
#ifdef BF3_TIMING
    const unsigned long long ts2 = lane == 0 ? wall_clock64() : 0ull;
#endif
    __syncthreads();  // every wave is done reading its patch
    float* const red = reinterpret_cast<float*>(smem);
    bf3_red_put<LDT>(red, wave, half, l31, acc);
    __syncthreads();
    if constexpr (UP) {
        // 8 channels x 2 rows of the 2 x 2 blocks x 16 TN pixel pairs: GEMM rows 4 c + 2 a (b = 0) and + 1 (b = 1) at two
        // horizontally adjacent pixels = four consecutive floats of output row 2 ho + a
#pragma unroll
        for (int it = 0; it < (16 * 16 * TN + BS - 1) / BS; ++it) {
            const int item = t + it * BS;
            if (item >= 16 * 16 * TN) break;
            const int r = item / (16 * TN), j = item % (16 * TN);
            const int ml = 2 * r, nl = 2 * j;
            const int ph = nl / PTW, pw = nl % PTW;
            const int ho = ho0 + ph, wo = wo0 + pw;
            const float2 u0 = bf3_red_sum<NW, LDT, float2>(red + ml * LDT + nl), u1 = bf3_red_sum<NW, LDT, float2>(red + (ml + 1) * LDT + nl);
            float4 v = make_float4(u0.x, u1.x, u0.y, u1.y);
            if (m0 + ml < p.M && img0 < nimg && ho < p.Hout && wo < p.Wout) {
                const int co = (m0 + ml) >> 2, a = r & 1;
                const int64_t addr = (((int64_t)img0 * p.Ctot + co) * (2 * p.Hout) + 2 * ho + a) * (2 * p.Wout) + 2 * wo;
                bf3_quad_store(p, v, addr, co);
            }
        }
    } else {
#pragma unroll
        for (int it = 0; it < (32 * 8 * TN + BS - 1) / BS; ++it) {
            const int item = t + it * BS;
            if (item >= 32 * 8 * TN) break;
            const int ml = item / (8 * TN), c4 = item % (8 * TN);  // 32 channels x 8 TN pixel quads
            const int m = m0 + ml, nl = 4 * c4;
            const int ph = nl / PTW, pw = nl % PTW;
            const int ho = ho0 + ph, wo = wo0 + pw;
            float4 v = bf3_red_sum<NW, LDT, float4>(red + ml * LDT + nl);
            if (m < p.M && img0 < nimg && ho < p.Hout && wo < p.Wout) {
                const int64_t addr = ((int64_t)img0 * p.Ctot + m) * p.HoWo + ho * p.Wout + wo;
                bf3_quad_store(p, v, addr, p.grp_imgs > 0 ? (img0 / p.grp_imgs) * p.M + m : m);
            }
        }
    }
#ifdef BF3_TIMING
    if (lane == 0) {  // one record per wave: prologue round trip, K loop (of which staging: [3] low half), reduction + epilogue, start
        __builtin_amdgcn_s_waitcnt(0);
        const unsigned long long ts3 = wall_clock64();
        const int b = ((blockIdx.y * gridDim.x + blockIdx.x) * NW + wave) & 8191;
        g_bf3_stamp[b * 8 + 0] = ts1 - ts0;
        g_bf3_stamp[b * 8 + 1] = ts2 - ts1;
        g_bf3_stamp[b * 8 + 2] = ts3 - ts2;
        g_bf3_stamp[b * 8 + 3] = ts0;
        g_bf3_stamp[b * 8 + 4] = t_stage;
    }
#endif
}

// launches of the two K-split kernels by wave count since the last reset (ivln_conv_ks_waves): [0] k_conv_bf3_ks with 8 waves,
// [1] with 4, [2] k_conv1x1_bf3_ks' K-split form with 8 waves, [3] with 4.  Host-side tally, not thread-safe.
static long long g_bf3_ks_waves[4] = {0, 0, 0, 0};

template <int PTH, int PTW, int TN = 2, int KS = 3, int NW = 8>
int launch_bf3_ks_tile(const ivln_gemm_desc& d, hipStream_t s, const unsigned char* a_split, int64_t grp_bytes, int nimg) {
    constexpr int NPIX = (PTH + KS - 1) * (PTW + KS - 1), WREG = (NPIX * PIXB + 15) & ~15, RED = NW * 32 * (32 * TN + 4) * 4;
    constexpr size_t lds = (size_t)(NW * WREG > RED ? NW * WREG : RED);
    static_assert(lds <= 160 * 1024, "patch regions do not fit");
    static_assert(NW == 8 || lds <= 80 * 1024, "two four-wave workgroups share a CU's LDS");
    constexpr auto kern = k_conv_bf3_ks<PTH, PTW, TN, KS, NW>;
    if (bf3_set_lds<kern>(lds) != IVLN_OK) return IVLN_E_HIP;
    const int tiles_w = d.Wout / PTW, tiles_h = d.Hout / PTH;
    dim3 grid(tiles_w * tiles_h * nimg, (d.M + 31) / 32, 1);
    IVLN_LAUNCH_FAMILY_NAMED("k_conv_bf3_ks", kern, grid, dim3(64 * NW), lds, s, d, a_split, (long long)grp_bytes, tiles_w, tiles_h, nimg);
    ++g_bf3_ks_waves[NW == 8 ? 0 : 1];
    return IVLN_OK;
}
// (the 64-pixel tile of an 8- | 16- | 32-wide map with 8 or 4 waves)
template <int KS>
int launch_bf3_ks_px64(const ivln_gemm_desc& d, hipStream_t s, const unsigned char* a, int64_t gb, int nimg, bool nw4) {
    if (d.Wout == 8) return nw4 ? launch_bf3_ks_tile<8, 8, 2, KS, 4>(d, s, a, gb, nimg) : launch_bf3_ks_tile<8, 8, 2, KS>(d, s, a, gb, nimg);
    if (d.Wout == 16) return nw4 ? launch_bf3_ks_tile<4, 16, 2, KS, 4>(d, s, a, gb, nimg) : launch_bf3_ks_tile<4, 16, 2, KS>(d, s, a, gb, nimg);
    return nw4 ? launch_bf3_ks_tile<2, 32, 2, KS, 4>(d, s, a, gb, nimg) : launch_bf3_ks_tile<2, 32, 2, KS>(d, s, a, gb, nimg);
}

// Four waves instead of eight (two co-resident workgroups per CU): where the eight-wave grid would run as two rounds - more
// workgroups than CUs, at most twice as many - and every wave still gets two chunks.  nw_pin = 8 | 4 pins one (tile_override
// 16 | 17 here, 18 | 19 for the 1x1 K-split form).  Kept per shape where it won: profiles/coresident_ks_sweep.txt.
static bool bf3_ks_four_waves(int64_t wgs, int nch, int nw_pin) {
    if (nw_pin) return nw_pin == 4;
    const int64_t cus = ivln_cu_count();
    return wgs > cus && wgs <= 2 * cus && nch >= 2 * 4;
}

// Eligibility of the K-split-over-waves kernel: deep 3x3 convs over few pixels.  mode: 0 = heuristic, 1 = insist (tests, tuning)
int bf3_ks_launch(ivln_gemm_desc& d, hipStream_t s, int nimg, int mode, int tn_pin = 0, int nw_pin = 0) {
    if (d.Cin % CB != 0 || d.Cin < 8 * CB || d.stat_partials || d.splits > 1) return IVLN_E_UNSUPPORTED;
    if (d.bmode == BMODE_CONV_K2) {  // the stacked transposed-conv classes: 64-pixel tiles, no image groups
        if (d.grp_imgs > 0 || (d.Wout != 8 && d.Wout != 16 && d.Wout != 32) || d.Hout % (64 / d.Wout) != 0 || (d.in_img_stride & 3) ||
            (((uintptr_t)d.B) & 15) || (int64_t)nimg * d.in_img_stride * 4 >= (int64_t)1 << 31)
            return IVLN_E_UNSUPPORTED;
        const int64_t wgs2 = (int64_t)(d.N / 64) * ((d.M + 31) / 32);
        if (mode == 0 && (wgs2 > 2 * (int64_t)ivln_cu_count() || wgs2 < ivln_cu_count() / 4)) return IVLN_E_UNSUPPORTED;
        d.splits = 1;
        const unsigned char* a2 = (const unsigned char*)d.A_split;
        const int64_t gb2 = d.a_split_grp_stride * 4;
        return launch_bf3_ks_px64<2>(d, s, a2, gb2, nimg, bf3_ks_four_waves(wgs2, d.Cin / CB, nw_pin));
    }
    if (d.Wout != 8 && d.Wout != 16 && d.Wout != 32) return IVLN_E_UNSUPPORTED;
    const int64_t wgs = (int64_t)(d.N / 64) * ((d.M + 31) / 32);
    // 32-pixel tiles where 64-pixel ones leave half of the CUs without a workgroup; tn_pin = 1 | 2 pins one (tile_override 14 | 15)
    const bool small = tn_pin ? tn_pin == 1 : 2 * wgs <= ivln_cu_count();
    const int pth = (small ? 32 : 64) / d.Wout;
    if (d.Hout % pth != 0 || (d.in_img_stride & 3) || (((uintptr_t)d.B) & 15)) return IVLN_E_UNSUPPORTED;
    if ((int64_t)nimg * d.in_img_stride * 4 >= (int64_t)1 << 31) return IVLN_E_UNSUPPORTED;  // byte offsets of the buffer loads
    if (d.grp_imgs > 0 && nimg % d.grp_imgs != 0) return IVLN_E_UNSUPPORTED;
    if (mode == 0 && (wgs > 2 * (int64_t)ivln_cu_count() || wgs < ivln_cu_count() / 4)) return IVLN_E_UNSUPPORTED;  // (more pixels: the tiled kernel fills the chip by itself)
    const int64_t gb = d.a_split_grp_stride * 4;
    d.splits = 1;
    const unsigned char* a = (const unsigned char*)d.A_split;
    if (small) {
        if (d.Wout == 8) return launch_bf3_ks_tile<4, 8, 1>(d, s, a, gb, nimg);
        if (d.Wout == 16) return launch_bf3_ks_tile<2, 16, 1>(d, s, a, gb, nimg);
        return launch_bf3_ks_tile<1, 32, 1>(d, s, a, gb, nimg);
    }
    return launch_bf3_ks_px64<3>(d, s, a, gb, nimg, bf3_ks_four_waves(wgs, d.Cin / CB, nw_pin));
}

// ------------------------------------------------------------------------------------------------------------------
// The map CNN's blocks at rollout batch (map_encoder.py:8-20: Conv 7x7 same -> BatchNorm (eval) -> ReLU -> AvgPool(2), 14 -> 32
// -> 64 -> 128 -> 256 channels on 64x64 ... 8x8 maps of 1-16 images) as ONE launch each (ivln_gemm_desc.pool2).  The fp32 kernels
// filled the chip there by splitting K over blockIdx.z: raw slabs to HBM, a reduction + pooling launch behind (16-64 slabs per
// output in the tail layers).  Here, the scheme of k_conv_bf3_ks with a 7x7 window:
//   * a workgroup of NW waves owns 32 output channels x a 4 x 8 pixel tile (whole 2x2 pooling windows: even origin, even
//     extent) over the WHOLE K; wave w takes the 16-channel chunks w, w + NW, ... (NW = the chunk count, 1 ... 8: one chunk,
//     49 taps, per wave at the CNN's shapes - 1024 waves per layer at 8 images);
//   * wave-private patch (10 x 14 pixels x 112 bytes = 15.7 KB, 125 KB at NW = 8), wave-private weight stream a kernel row
//     (7 taps) ahead, no barrier inside the K loop;
//   * the partial tiles meet in LDS; a thread sums the four pixels of a pooling window over the waves in a fixed order,
//     applies the folded scale / shift and the ReLU to each and stores (((a + b) + c) + d) * 0.25f - the order of
//     k_scale_shift_relu_avgpool2 - into the pooled NCHW tensor.  No slabs, no second launch.
//   * U8 (layer 1): the patch is built from the u8 occupancy and label maps themselves - channel 0 = the occupancy value,
//     channel 1 + k = (label == k), labels >= 13 match nothing: what k_map_features4 writes - as ONE bf16 piece (every value
//     is exact in bf16: the products against the lower pieces are exact zeros and are not issued), so the one-hot fp32
//     tensor and its launch are gone.
// ------------------------------------------------------------------------------------------------------------------
template <int NW, bool U8>
__global__ __launch_bounds__(64 * NW, 2) void k_conv7_pool_bf3(const ivln_gemm_desc p, const unsigned char* a_split, int tiles_w, int tiles_h, int nimg) {
    constexpr int KS = 7, KK = KS * KS, KKP = bf3_taps_padded(KS), DA = KS, PTH = 4, PTW = 8, NTB = 64 * NW;
    constexpr int PH = PTH + KS - 1, PWR = PTW + KS - 1, NPIX = PH * PWR;
    constexpr int NPJ = (NPIX + 63) / 64;  // (U8: patch pixels per lane)
    constexpr int WREG = (NPIX * PIXB + 15) & ~15;
    constexpr int LDT = 32 + 4;
    constexpr int NPL = U8 ? 1 : 3;  // pieces of the activations
    static_assert(KK % DA == 0, "the weight rotation closes over a chunk");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const BlockId bid = xcd_block_id(p.no_xcd_remap);
    const int bx = bid.x;
    const int tw = bx % tiles_w, th = (bx / tiles_w) % tiles_h, img0 = bx / (tiles_w * tiles_h);
    const int ho0 = th * PTH, wo0 = tw * PTW;
    const int m0 = bid.y * 32;
    const int nch = (p.Cin + CB - 1) / CB;
    const int HW = p.Hin * p.Win;
    const int niter = wave < nch ? (nch - wave + NW - 1) / NW : 0;  // chunks wave, wave + NW, ...
    unsigned char* const wsm = smem + wave * WREG;

    // f32 input: the wave stages its own patch, as in k_conv_bf3_ks (a ragged last chunk - 14 channels - reads the rest as zero)
    Bf3GroupStager<KS, PH, PWR, 1, 64> gs;
    if constexpr (!U8) gs.setup(p, lane, img0, nimg, ho0, wo0, KS / 2);
    const __amdgpu_buffer_rsrc_t rB = bf3_rsrc(p.B);
    auto load_patch = [&](int c) {
        if constexpr (!U8) gs.load(rB, c, HW, p.Cin);
    };
    auto stage = [&]() {
        if constexpr (!U8) {
            gs.stage(wsm);
        } else {
            // a patch pixel per lane and round: its two bytes -> the 16-channel record of the first piece (32 bytes: word q =
            // channels 2 q, 2 q + 1).  Outside the image (the conv's zero padding): zeros, no label matches.
            const uint8_t* const occ = reinterpret_cast<const uint8_t*>(p.B);
            const uint8_t* const sem = p.map_sem_u8;
            int ov[NPJ], sv[NPJ];
#pragma unroll
            for (int j = 0; j < NPJ; ++j) {
                const int pix = lane + j * 64, y = pix / PWR, x = pix - y * PWR;
                const int hi = ho0 - KS / 2 + y, wi = wo0 - KS / 2 + x;
                const bool ok = pix < NPIX && img0 < nimg && (unsigned)hi < (unsigned)p.Hin && (unsigned)wi < (unsigned)p.Win;
                const int64_t o = (int64_t)img0 * HW + hi * p.Win + wi;
                ov[j] = ok ? (int)occ[o] : 0;
                sv[j] = ok ? (int)sem[o] : -1;
            }
#pragma unroll
            for (int j = 0; j < NPJ; ++j) {
                const int pix = lane + j * 64;
                constexpr uint32_t ONE = 0x3F80u;  // bf16 1.0
                v4i w0, w1;
                w0[0] = (int)((__float_as_uint((float)ov[j]) >> 16) | (sv[j] == 0 ? ONE << 16 : 0u));  // (0 ... 255: exact in bf16's 8 bits)
#pragma unroll
                for (int q = 1; q < 4; ++q) w0[q] = (int)((sv[j] == 2 * q - 1 ? ONE : 0u) | (sv[j] == 2 * q ? ONE << 16 : 0u));
#pragma unroll
                for (int q = 4; q < 7; ++q) w1[q - 4] = (int)((sv[j] == 2 * q - 1 ? ONE : 0u) | (sv[j] == 2 * q ? ONE << 16 : 0u));
                w1[3] = 0;  // channels 14, 15: past Cin
                if (pix < NPIX) {
                    *reinterpret_cast<v4i*>(wsm + pix * PIXB) = w0;
                    *reinterpret_cast<v4i*>(wsm + pix * PIXB + 16) = w1;
                }
            }
        }
    };
    const int bbase = ((l31 / PTW) * PWR + (l31 % PTW)) * PIXB + half * 16;
    const int mt = min(m0 / 32, (p.M + 31) / 32 - 1);
    const __amdgpu_buffer_rsrc_t rA = bf3_rsrc(a_split + (int64_t)mt * nch * KKP * (3 * 1024));
    const int q_last = max(niter * KK - 1, 0);
    auto load_a = [&](int q, int pl) -> v4i {  // q: tap index in THIS wave's sequence (iteration i = q / 49 is chunk wave + i NW)
        const int qc = min(q, q_last), i = qc / KK, r = qc - i * KK;
        return __builtin_amdgcn_raw_buffer_load_b128(rA, (((wave + i * NW) * KKP + r) * 3 + pl) * 1024 + lane * 16, 0, 0);
    };
    f32x16 acc[1];  // (one 32-pixel tile)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[0][i] = 0.f;

    if (niter > 0) {
        v4i abuf[DA][3];
#pragma unroll
        for (int d = 0; d < DA; ++d)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) abuf[d][pl] = load_a(d, pl);
        load_patch(wave);
        for (int i = 0; i < niter; ++i) {
            stage();
            const int s0 = i * KK;
            auto read_b = [&](int r, bf16x8 (&b)[1][3]) {
                const int kh = r / KS, kw = r - kh * KS, toff = (kh * PWR + kw) * PIXB;
#pragma unroll
                for (int pl = 0; pl < NPL; ++pl) b[0][pl] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const v4i*>(wsm + bbase + toff + pl * 32));
            };
            bf16x8 bq[2][1][3];
            read_b(0, bq[0]);
#pragma unroll
            for (int r = 0; r < KK; ++r) {
                const int slot = r % DA;
                if (r + 1 < KK) read_b(r + 1, bq[(r + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
                bf3_products<U8 ? BF3_THREE : BF3_SIX>(acc, abuf[slot], bq[r & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) abuf[slot][pl] = load_a(s0 + r + DA, pl);
                if (r == 1) load_patch(wave + min(i + 1, niter - 1) * NW);  // (the next chunk's patch: 47 taps of MFMA work before the staging pass reads it)
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    // ---- the partial tiles meet in LDS: red[wave][32 channels][32 pixels (+4)] over the patch regions; then the CBRA tail ----
    __syncthreads();
    float* const red = reinterpret_cast<float*>(smem);
    bf3_red_put<LDT>(red, wave, half, l31, acc);
    __syncthreads();
    const int Hp = p.Hout >> 1, Wp = p.Wout >> 1;
    for (int idx = t; idx < 32 * (PTH / 2) * (PTW / 2); idx += NTB) {
        const int ml = idx >> 3, pp = idx & 7, py = pp >> 2, px = pp & 3;  // (PTH / 2) x (PTW / 2) = 2 x 4 windows per channel
        const int m = m0 + ml;
        const float* const rp = red + ml * LDT + (2 * py) * PTW + 2 * px;  // the window's upper row; the lower one PTW on
        const float2 tt = bf3_red_sum<NW, LDT, float2>(rp), uu = bf3_red_sum<NW, LDT, float2>(rp + PTW);
        if (m < p.M && img0 < nimg) {  // (not bf3_quad_store: four outputs become ONE pooled value, in k_scale_shift_relu_avgpool2's order)
            const float sc = p.scale[m], sh = p.shift[m];
            const float a = fmaxf(fmaf(tt.x, sc, sh), 0.f), b = fmaxf(fmaf(tt.y, sc, sh), 0.f);
            const float c2 = fmaxf(fmaf(uu.x, sc, sh), 0.f), d = fmaxf(fmaf(uu.y, sc, sh), 0.f);
            p.D[(((int64_t)img0 * p.Ctot + m) * Hp + (ho0 >> 1) + py) * Wp + (wo0 >> 1) + px] = (((a + b) + c2) + d) * 0.25f;
        }
    }
}

template <int NW, bool U8>
int launch_conv7_pool(const ivln_gemm_desc& d, hipStream_t s, int nimg) {
    constexpr int WREG = ((4 + 6) * (8 + 6) * PIXB + 15) & ~15, RED = 32 * 36 * 4;
    constexpr size_t lds = (size_t)NW * (WREG > RED ? WREG : RED);
    static_assert(lds <= 160 * 1024, "patch regions do not fit");
    constexpr auto kern = k_conv7_pool_bf3<NW, U8>;
    if (bf3_set_lds<kern>(lds) != IVLN_OK) return IVLN_E_HIP;
    const int tiles_w = d.Wout / 8, tiles_h = d.Hout / 4;
    dim3 grid(tiles_w * tiles_h * nimg, (d.M + 31) / 32, 1);
    IVLN_LAUNCH_FAMILY_NAMED("k_conv7_pool_bf3", kern, grid, dim3(64 * NW), lds, s, d, (const unsigned char*)d.A_split, tiles_w, tiles_h, nimg);
    return IVLN_OK;
}

// ivln_gemm_desc.pool2: eligibility of the fused map-CNN block.  Anything else is IVLN_E_UNSUPPORTED - the caller issues conv + tail.
int bf3_conv7_pool_launch(ivln_gemm_desc& d, hipStream_t s) {
    if (d.bmode != BMODE_CONV_K7 || d.amode != AMODE_MK || d.dmode != DMODE_NCHW || d.dil != 1 || d.stride != 1 || d.pad != 3 ||
        d.Hout != d.Hin || d.Wout != d.Win || d.K != d.Cin * 49 || d.HoWo != d.Hout * d.Wout || d.N % d.HoWo != 0)
        return IVLN_E_UNSUPPORTED;
    if ((d.Hout & 3) || (d.Wout & 7) || !d.scale || !d.shift || !d.relu || d.residual || d.accumulate || d.residual_after_relu || d.defer_epilogue ||
        d.splits > 1 || d.stat_partials || d.img_run_flags || d.fuse_A_split || d.grp_imgs > 0 || d.Cin > 8 * CB)
        return IVLN_E_UNSUPPORTED;
    const int nimg = d.N / d.HoWo;
    const int64_t tiles = (int64_t)nimg * (d.Hout / 4) * (d.Wout / 8);
    if (tiles >= (int64_t)1 << 30) return IVLN_E_UNSUPPORTED;
    d.splits = 1;
    if (d.map_sem_u8) {  // B = the u8 occupancy map, map_sem_u8 = the u8 labels: 1 + 13 channels built while staging
        if (d.Cin != 14 || (int64_t)nimg * d.HoWo >= (int64_t)1 << 31) return IVLN_E_UNSUPPORTED;
        return launch_conv7_pool<1, true>(d, s, nimg);
    }
    if ((d.in_img_stride & 3) || (((uintptr_t)d.B) & 15) || (int64_t)nimg * d.in_img_stride * 4 >= (int64_t)1 << 31) return IVLN_E_UNSUPPORTED;
    const int nch = (d.Cin + CB - 1) / CB;
    if (nch == 1) return launch_conv7_pool<1, false>(d, s, nimg);
    if (nch == 2) return launch_conv7_pool<2, false>(d, s, nimg);
    if (nch <= 4) return launch_conv7_pool<4, false>(d, s, nimg);
    return launch_conv7_pool<8, false>(d, s, nimg);
}

// ------------------------------------------------------------------------------------------------------------------
// 1x1 convs with a deep K (RedNet's bottleneck reductions 1024 -> 256, 2048 -> 512, its 2048-channel expansions and skip
// convs: rednet.py:20-65, 244-248) on the same arithmetic, K split over the waves of a workgroup, NO LDS in the K loop:
//   * a workgroup (8 waves) owns 32 output channels x 128 consecutive pixels over the whole K, wave w the chunks
//     [w, w + 1) * ceil(nch / 8);
//   * a 1x1 conv needs no patch: the B fragment of v_mfma_f32_32x32x16_bf16 - column n, 8 consecutive k per lane - is
//     built IN REGISTERS.  Lane (l31, half) loads, for its 8 channels (8 half ..) of the chunk, the four consecutive pixels
//     4 l31 .. 4 l31 + 3 (one buffer_load_b128 per channel, 512 contiguous bytes per half-wave), splits channel pairs
//     into the three bf16 pieces (v_cvt_pk_bf16_f32 packs a pair into the word the fragment wants) and has the B fragments
//     of FOUR pixel tiles - tile e holds pixel 4 l31 + e in column l31 - without a single LDS access or barrier;
//   * weights: the split image of ivln_conv_split_weights_f32 (KS = 1), global -> registers four chunks ahead;
//   * the eight partial tiles meet in LDS at the end, summed in a fixed order, fused epilogue, 16-byte stores.
// An activation element is split once per 32-channel tile that reads it (176 VALU operations per lane and chunk beside 24
// MFMAs): the VALU work rides under the other wave's MFMAs.
// ------------------------------------------------------------------------------------------------------------------
// WT (wave tiles, short K: 64 ... 256 input channels - the bottleneck expansions 64 -> 256 ... 256 -> 1024 with their residual):
// no K split at all - each of the workgroup's 4 waves owns its own 32 x 128 tile over the whole K and finishes it alone
// (wave-private LDS for the transposing epilogue, no barrier anywhere); these launches are bound by their activation bytes.
// K-split form with NW = 4: two co-resident workgroups per CU for the grids that would run as two rounds (see k_conv_bf3_ks).
template <bool WT, int NW = WT ? 4 : 8>
__global__ __launch_bounds__(64 * NW, 2) void k_conv1x1_bf3_ks(const ivln_gemm_desc p, const unsigned char* a_split, long long a_grp_bytes) {
    constexpr int TN = 4, DA = 4, BN = 128, BS = 64 * NW;
    static_assert(WT ? NW == 4 : (NW == 8 || NW == 4), "wave tiles: 4 waves; K split: 8 or 4");
    constexpr int LDT = BN + 4;
    constexpr unsigned OOB = 0x80000000u;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const BlockId bid = xcd_block_id(p.no_xcd_remap);
    // grid = (channel tiles, pixel tiles): consecutive workgroup ids - one XCD's contiguous range after the remap - share their
    // PIXELS.  A 1x1 conv's activation tile (128 pixels x Cin x 4 bytes: 512 KB at 1024 channels) outweighs a channel tile's
    // weights (196 KB), and with the pixel tile as the fast index every XCD fetched every activation: 8 x the input bytes
    // over the fabric, which is what bounded the first version (256 x 4096 x 1024: 134 MB in 23 us).
    // (WT: the workgroup's four waves own four pixel tiles of ONE channel tile - they stream the same weights; four channel tiles of
    //  one pixel tile, i.e. shared activations, measured 38 us per RedNet step slower: profiles/r06_predsem_ab_wtshare.txt)
    const int n0 = WT ? (bid.y * NW + wave) * BN : bid.y * BN, m0 = bid.x * 32;
    const int nch = p.Cin / CB;
    const int HW = p.HoWo;
    const int cpw = WT ? nch : (nch + NW - 1) / NW;
    const int c0 = WT ? 0 : min(nch, wave * cpw), c1 = WT ? nch : min(nch, c0 + cpw);
    const int n_img0 = min(n0, p.N - 1) / HW;
    const int grp = p.grp_imgs > 0 ? n_img0 / p.grp_imgs : 0;

    const int nq = n0 + 4 * l31;  // this lane's four pixels (one image: HW is a multiple of 4)
    const int qimg = nq / HW, qpp = nq - qimg * HW;
    const unsigned hw4 = (unsigned)HW * 4u;
    const unsigned xvo = nq < p.N ? (unsigned)(((int64_t)qimg * p.in_img_stride + qpp + (int64_t)(8 * half) * HW) * 4) : OOB;
    const __amdgpu_buffer_rsrc_t rB = bf3_rsrc(p.B);
    auto load_x = [&](int c, v4i (&xb)[8]) {  // (the channel steps ride in the SCALAR offset, which the range check ignores: no VALU per load)
        const int so = c * CB * HW * 4;
#pragma unroll
        for (int j = 0; j < 8; ++j) xb[j] = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)xvo, so + j * (int)hw4, 0);
    };
    const int mt = min(m0 / 32, (p.M + 31) / 32 - 1);
    const __amdgpu_buffer_rsrc_t rA = bf3_rsrc(a_split + (int64_t)grp * a_grp_bytes + (int64_t)mt * nch * (3 * 1024));
    const int c_last = max(c1 - 1, 0);
    auto load_a = [&](int c, v4i (&ab)[3]) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) ab[pl] = __builtin_amdgcn_raw_buffer_load_b128(rA, (min(c, c_last) * 3 + pl) * 1024 + lane * 16, 0, 0);
    };
    f32x16 acc[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[tn][i] = 0.f;

#ifdef BF3_TIMING
    const unsigned long long ts0 = lane == 0 ? wall_clock64() : 0ull;
    unsigned long long ts1 = ts0, tc_split = 0, tc_load = 0, tc_mfma = 0;  // (shader cycles inside the K loop: waits + split | load issue | MFMA issue)
#endif
    if (c0 < c1 && (!WT || n0 < p.N)) {
        v4i xb[2][8], ab[DA][3];
#pragma unroll
        for (int d = 0; d < DA; ++d) load_a(c0 + d, ab[d]);
        load_x(c0, xb[0]);
        load_x(min(c0 + 1, c_last), xb[1]);
#ifdef BF3_TIMING
        __builtin_amdgcn_s_waitcnt(0);  // (timing build only: the prologue's round trip as a phase of its own)
        ts1 = lane == 0 ? wall_clock64() : 0ull;
#endif
        for (int cc = c0; cc < c1; cc += DA) {
#pragma unroll
            for (int k = 0; k < DA; ++k) {
                const int c = cc + k;
                v4i bq[TN][3];
                bf16x8 a[3];
#ifdef BF3_TIMING
                const unsigned long long tl0 = __builtin_readcyclecounter();
#endif
                // (loads stay outside the branch: the compiler then knows how many are in flight at every wait)
                if (c < c1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            uint32_t H, M, L;
#ifdef BF3_PROBE_NO_SPLIT  // (tools/conv_bf3_ks_phases.py: what the K loop costs without its VALU work - wrong results)
                            H = xb[k & 1][2 * i][e], M = xb[k & 1][2 * i + 1][e], L = H ^ M;
#else
                            split3_pair(__int_as_float(xb[k & 1][2 * i][e]), __int_as_float(xb[k & 1][2 * i + 1][e]), H, M, L);
#endif
                            bq[e][0][i] = (int)H, bq[e][1][i] = (int)M, bq[e][2][i] = (int)L;
                        }
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) a[pl] = __builtin_bit_cast(bf16x8, ab[k][pl]);
                }
                __builtin_amdgcn_sched_barrier(0);
#ifdef BF3_TIMING
                const unsigned long long tl1 = __builtin_readcyclecounter();
                __builtin_amdgcn_sched_barrier(0);
#endif
                load_x(min(c + 2, c_last), xb[k & 1]);  // two chunks ahead
                load_a(c + DA, ab[k]);                   // DA chunks ahead
                __builtin_amdgcn_sched_barrier(0);
#ifdef BF3_TIMING
                const unsigned long long tl2 = __builtin_readcyclecounter();
                __builtin_amdgcn_sched_barrier(0);
#endif
                if (c < c1) {
#ifdef BF3_PROBE_NO_MFMA  // (... and without its matrix work: one product of the six)
                    bf3_products<BF3_ONE>(acc, a[0], a[1], a[2], bq);
#else
                    bf3_products(acc, a[0], a[1], a[2], bq);
#endif
                }
#ifdef BF3_TIMING
                __builtin_amdgcn_sched_barrier(0);
                const unsigned long long tl3 = __builtin_readcyclecounter();
                tc_split += tl1 - tl0, tc_load += tl2 - tl1, tc_mfma += tl3 - tl2;
#endif
            }
        }
    }
    // ---- epilogue.
    // WT: straight from the accumulators.  Tile e holds pixel 4 l31 + e in column l31, so register r of the four tiles IS the
    // float4 of channel (r & 3) + 8 (r >> 2) + 4 half at pixels 4 l31 .. + 3: one 16-byte store per register, 512 contiguous
    // bytes per half-wave, no LDS, no transposition.  The channel step of register r rides in the scalar offset of the
    // buffer accesses (the range check ignores it).  The operands (residual quads, scale / shift) are requested FIRST, all of
    // them: with one wave per SIMD every dependent round trip would otherwise sit exposed at the end of a 20 us kernel.
    // KS: the eight waves' partial tiles meet in LDS - red[wave][32 channels][4 tiles x 32 columns (+4)] -, summed in a fixed order. ----
#ifdef BF3_TIMING
    const unsigned long long ts2 = lane == 0 ? wall_clock64() : 0ull;
#endif
    // IVLN_D_NCHW_UP2X4 (the 2 x 2 stride-2 upsampling branches and the final deconv, rednet.py:239-245, 217-218: one tap per
    // parity class): rows 4 c + 2 a (b = 0) and + 1 (b = 1) are registers r and r + 1 of one lane, its four pixels of a class-grid
    // row are eight consecutive floats of output row 2 ho + a - two 16-byte stores per register pair, plain stores (no
    // scalar-offset buffer stores here: nothing for the store guard to do).
    const bool up = p.dmode == DMODE_NCHW_UP2X4;  // (uniform)
    if (WT && up) {
        const int n = n0 + 4 * l31;
        if (n < p.N) {
            const int img = n / HW, pp = n - img * HW;
            const int ho = pp / p.Wout, wo = pp - ho * p.Wout;
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const int m = m0 + 4 * half + (r & 3) + 8 * (r >> 2);  // row of b = 0; + 1 is b = 1 (M % 4 == 0: in or out together)
                if (m >= p.M) continue;
                const int co = m >> 2, a = (m >> 1) & 1;
                const int64_t addr = (((int64_t)img * p.Ctot + co) * (2 * p.Hout) + 2 * ho + a) * (2 * p.Wout) + 2 * wo;
                float v[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[2 * e] = acc[e][r], v[2 * e + 1] = acc[e][r + 1];
                const float sc = p.scale ? p.scale[co] : 1.f, sh = p.shift ? p.shift[co] : 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = p.scale ? fmaf(v[e], sc, sh) : v[e] + sh;
                if (p.residual) {
                    const float4 r0 = *reinterpret_cast<const float4*>(p.residual + addr), r1 = *reinterpret_cast<const float4*>(p.residual + addr + 4);
                    v[0] += r0.x, v[1] += r0.y, v[2] += r0.z, v[3] += r0.w, v[4] += r1.x, v[5] += r1.y, v[6] += r1.z, v[7] += r1.w;
                }
                if (p.relu) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
                }
                *reinterpret_cast<float4*>(p.D + addr) = make_float4(v[0], v[1], v[2], v[3]);
                *reinterpret_cast<float4*>(p.D + addr + 4) = make_float4(v[4], v[5], v[6], v[7]);
            }
        }
    } else
    if constexpr (WT) {
        const int n = n0 + 4 * l31;
        const int img = min(n, p.N - 1) / HW, pp = n - img * HW;
        const int mrem = n < p.N ? p.M - m0 - 4 * half : 0;  // register r is inside the tensor iff its channel step is below this
        const int me0 = (p.grp_imgs > 0 ? (img / p.grp_imgs) * p.M : 0) + m0 + 4 * half;
        const unsigned off0 = (unsigned)(((img * p.Ctot + m0 + 4 * half) * HW + pp) * 4);
        const __amdgpu_buffer_rsrc_t rR = bf3_rsrc(p.residual), rS = bf3_rsrc(p.scale), rH = bf3_rsrc(p.shift), rD = bf3_rsrc(p.D);
        const bool has_res = p.residual != nullptr, has_sc = p.scale != nullptr, has_sh = p.shift != nullptr;
        const float relu_lo = p.relu ? 0.f : -__builtin_huge_valf();
        const bool res_post = p.residual_after_relu != 0;
        // (not bf3_quad_store: straight-line code between scalar-offset buffer stores, BF3_STORE_GUARD behind each)
        v4i rres[16];
        float esc[16], esh[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int cs = (r & 3) + 8 * (r >> 2);  // channel step of the register
            const bool ok = cs < mrem;
            esc[r] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rS, ok && has_sc ? me0 * 4 : (int)OOB, cs * 4, 0));
            esh[r] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rH, ok && has_sh ? me0 * 4 : (int)OOB, cs * 4, 0));
            rres[r] = __builtin_amdgcn_raw_buffer_load_b128(rR, ok && has_res ? (int)off0 : (int)OOB, cs * HW * 4, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int cs = (r & 3) + 8 * (r >> 2);
            float4 v = make_float4(acc[0][r], acc[1][r], acc[2][r], acc[3][r]);
            // STRAIGHT-LINE code between the stores (absent scale = 1, absent shift / residual = the zeros the out-of-range loads
            // returned; `accumulate` is declined by the launcher): see the fused tail of k_conv_bf3 for what a uniform branch
            // behind a 16-byte buffer store with a scalar offset does to the store's data registers.
            const float sc = has_sc ? esc[r] : 1.f, sh = esh[r];
            v.x = fmaf(v.x, sc, sh), v.y = fmaf(v.y, sc, sh), v.z = fmaf(v.z, sc, sh), v.w = fmaf(v.w, sc, sh);
            // the residual in front of the ReLU (a bottleneck's identity) or behind it (ivln_gemm_desc.residual_after_relu: the
            // decoder's skip adds) - selects, no branch
            const float r0 = __int_as_float(rres[r][0]), r1 = __int_as_float(rres[r][1]), r2 = __int_as_float(rres[r][2]), r3 = __int_as_float(rres[r][3]);
            v.x += res_post ? 0.f : r0, v.y += res_post ? 0.f : r1, v.z += res_post ? 0.f : r2, v.w += res_post ? 0.f : r3;
            const float lo = relu_lo;  // 0 with ReLU, -inf without: fmaxf(x, -inf) == x
            v.x = fmaxf(v.x, lo), v.y = fmaxf(v.y, lo), v.z = fmaxf(v.z, lo), v.w = fmaxf(v.w, lo);
            v.x += res_post ? r0 : 0.f, v.y += res_post ? r1 : 0.f, v.z += res_post ? r2 : 0.f, v.w += res_post ? r3 : 0.f;
            v4i o;
            o[0] = __float_as_int(v.x), o[1] = __float_as_int(v.y), o[2] = __float_as_int(v.z), o[3] = __float_as_int(v.w);
            __builtin_amdgcn_raw_buffer_store_b128(o, rD, cs < mrem ? (int)off0 : (int)OOB, cs * HW * 4, 0);
            BF3_STORE_GUARD();
        }
    } else if (up) {
        // the eight waves' partial tiles meet in LDS as below; an item = (channel of the tile, a, pixel pair): rows 4 c + 2 a and + 1
        // at two horizontally adjacent class-grid pixels = four consecutive floats of output row 2 ho + a
        float* const red = reinterpret_cast<float*>(smem);
        bf3_red_put<LDT>(red, wave, half, l31, acc);
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 16 * 64 / BS; ++it) {
            const int item = t + it * BS, r = item >> 6, j = item & 63;  // 16 (channel, a) x 64 pixel pairs
            const int ml = 2 * r, nl = 2 * j, n = n0 + nl;
            const int e0 = nl & 3, q = nl >> 2;  // tile e, column q holds pixel 4 q + e
            const float* const r0 = red + ml * LDT + q + e0 * 32;  // rows ml and ml + 1, tiles e0 and e0 + 1
            const float2 u0 = bf3_red_sum<NW, LDT, float2, 32>(r0), u1 = bf3_red_sum<NW, LDT, float2, 32>(r0 + LDT);
            float4 v = make_float4(u0.x, u1.x, u0.y, u1.y);
            if (m0 + ml < p.M && n < p.N) {
                const int img = n / HW, pp = n - img * HW;
                const int ho = pp / p.Wout, wo = pp - ho * p.Wout;
                const int co = (m0 + ml) >> 2, a = r & 1;
                const int64_t addr = (((int64_t)img * p.Ctot + co) * (2 * p.Hout) + 2 * ho + a) * (2 * p.Wout) + 2 * wo;
                bf3_quad_store(p, v, addr, co);  // (`accumulate` never set here: the launcher declines it)
            }
        }
    } else {
    // (not bf3_quad_store: the operands are requested BEFORE the barrier, and the absent residual stays a branch - see the -0 remark)
    constexpr int ITEMS = 32 * 32 / BS;  // 32 channels x 32 pixel quads = 1024 items over the workgroup's 512 | 256 threads
    v4i rres[ITEMS];
    float esc[ITEMS], esh[ITEMS];
    int eoff[ITEMS];  // element offset of the item's quad in D / residual (< 2^29: checked by the launcher), -1 = outside
    const __amdgpu_buffer_rsrc_t rR = bf3_rsrc(p.residual), rS = bf3_rsrc(p.scale), rH = bf3_rsrc(p.shift);
    const bool has_res = p.residual != nullptr, has_sc = p.scale != nullptr, has_sh = p.shift != nullptr;
    auto request = [&](int it) {
        const int item = t + it * BS, ml = item >> 5, q = item & 31;
        const int m = m0 + ml, n = n0 + 4 * q;
        const bool ok = m < p.M && n < p.N;
        const int img = n / HW, pp = n - img * HW;
        const int off = (img * p.Ctot + m) * HW + pp;
        const int me = p.grp_imgs > 0 ? (img / p.grp_imgs) * p.M + m : m;
        eoff[it] = ok ? off : -1;
        esc[it] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rS, ok && has_sc ? me * 4 : (int)OOB, 0, 0));
        esh[it] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rH, ok && has_sh ? me * 4 : (int)OOB, 0, 0));
        rres[it] = __builtin_amdgcn_raw_buffer_load_b128(rR, ok && has_res ? off * 4 : (int)OOB, 0, 0);
    };
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) request(it);
    float* const red = reinterpret_cast<float*>(smem);
    bf3_red_put<LDT>(red, wave, half, l31, acc);
    __syncthreads();
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const int item = t + it * BS, ml = item >> 5, q = item & 31;
        float4 v = bf3_red_sum<NW, LDT, float4, 32>(red + ml * LDT + q);  // tile e, column q = pixel 4 q + e
        if (eoff[it] >= 0) {
            const int64_t addr = eoff[it];
            const float sc = esc[it], sh = esh[it];
            if (p.scale) v.x = fmaf(v.x, sc, sh), v.y = fmaf(v.y, sc, sh), v.z = fmaf(v.z, sc, sh), v.w = fmaf(v.w, sc, sh);
            else if (p.shift) v.x += sh, v.y += sh, v.z += sh, v.w += sh;
            // (absent residual: the out-of-range loads returned zeros, but adding them would turn a -0 into +0: the branch stays)
            const bool res_pre = p.residual && !p.residual_after_relu, res_post = p.residual && p.residual_after_relu;
            if (res_pre)
                v.x += __int_as_float(rres[it][0]), v.y += __int_as_float(rres[it][1]), v.z += __int_as_float(rres[it][2]),
                    v.w += __int_as_float(rres[it][3]);
            if (p.accumulate) {
                const float4 ra = *reinterpret_cast<const float4*>(p.D + addr);
                v.x += ra.x, v.y += ra.y, v.z += ra.z, v.w += ra.w;
            }
            if (p.relu) v.x = fmaxf(v.x, 0.f), v.y = fmaxf(v.y, 0.f), v.z = fmaxf(v.z, 0.f), v.w = fmaxf(v.w, 0.f);
            if (res_post)  // (ivln_gemm_desc.residual_after_relu: the decoder's skip adds)
                v.x += __int_as_float(rres[it][0]), v.y += __int_as_float(rres[it][1]), v.z += __int_as_float(rres[it][2]),
                    v.w += __int_as_float(rres[it][3]);
            *reinterpret_cast<float4*>(p.D + addr) = v;
        }
    }
    }
#ifdef BF3_TIMING
    if (lane == 0) {  // one record per wave: prologue round trip, K loop, epilogue (100 MHz wall clock), start offset of the wave
        __builtin_amdgcn_s_waitcnt(0);
        const unsigned long long ts3 = wall_clock64();
        const int b = ((blockIdx.y * gridDim.x + blockIdx.x) * NW + wave) & 8191;
        g_bf3_stamp[b * 8 + 0] = ts1 - ts0;
        g_bf3_stamp[b * 8 + 1] = ts2 - ts1;
        g_bf3_stamp[b * 8 + 2] = ts3 - ts2;
        g_bf3_stamp[b * 8 + 3] = ts0;
        g_bf3_stamp[b * 8 + 4] = tc_split;
        g_bf3_stamp[b * 8 + 5] = tc_load;
        g_bf3_stamp[b * 8 + 6] = tc_mfma;
    }
#endif
}

// Eligibility of the 1x1 kernels in their two forms.  mode: 0 = heuristic, 1 = insist; *kind: the form launched, as
// ivln_conv_split_kinds counts it (2 = K split over the waves, 3 = wave tiles)
int bf3_1x1_ks_launch(ivln_gemm_desc& d, hipStream_t s, int mode, int form_pin, int* kind, int nw_pin = 0) {
    if (d.stride != 1 || d.pad != 0 || d.Cin % CB != 0 || d.Cin < 4 * CB || d.stat_partials || d.splits > 1) return IVLN_E_UNSUPPORTED;
    if ((d.HoWo & 3) || (d.in_img_stride & 3) || ((((uintptr_t)d.B) | ((uintptr_t)d.D) | ((uintptr_t)d.residual)) & 15)) return IVLN_E_UNSUPPORTED;
    const int64_t nimg = d.N / d.HoWo;
    if (nimg * d.in_img_stride * 4 >= (int64_t)1 << 31 || nimg * d.Ctot * d.HoWo * 4 >= (int64_t)1 << 31) return IVLN_E_UNSUPPORTED;  // byte offsets of the buffer loads
    if (d.grp_imgs > 0 && ((int64_t)d.grp_imgs * d.HoWo) % 128 != 0) return IVLN_E_UNSUPPORTED;  // a tile's pixels share one weight set
    const int nch = d.Cin / CB;
    // wave tiles (no K split) up to 16 chunks, K split over the 8 waves from 32 (in between - 272 ... 496 channels - the K-split
    // form with short slices); form_pin = 0 | 1 pins one (tile_override 12 | 13)
    bool wt = nch <= 16;
    // (32 chunks over MANY pixels - 256 x 16384 x 512, layer 3's first reduction at 8 + 8 images - would be four rounds of one
    //  K-split workgroup per CU: the wave tiles take it, 43.6 against 51.5 us on the tiled 1x1 form and 52.1 K-split, tools/conv_cfg_sweep.py)
    if (nch == 32 && (int64_t)((d.N + 127) / 128) * ((d.M + 31) / 32) > 2 * (int64_t)ivln_cu_count()) wt = true;
    // (24 and 48 chunks over MANY pixels - 512 x 16384 x 384 and 1024 x 4096 x 768, the stride-2 entry blocks' expansion with the
    //  downsample branch in its K at 8 + 8 images (rednet.py: MERGE_ENTRY_CONV3) - are the same case.  Both forms pinned, image-
    //  grouped, shift + ReLU, back to back in one call: 47.6 us as wave tiles against 76.6 K-split (2048 workgroups) for the
    //  first, 47.0 against 69.3 (1024 workgroups) for the second; the downsample conv + conv3-with-residual pairs they replace
    //  took 61.4 and 52.8.  2048 x 1024 x 1536 - 96 chunks, beyond the wave-tile form, whose 128 workgroups would leave half
    //  of the CUs empty anyway - is 512 K-split workgroups, which the rule below already takes: 52.2 us against the pair's 65.1.)
    if ((nch == 24 || nch == 48) && (int64_t)((d.N + 127) / 128) * ((d.M + 31) / 32) > 2 * (int64_t)ivln_cu_count()) wt = true;
    if (form_pin >= 0) wt = form_pin == 1;
    if (wt && nch > 64) wt = false;
    if (wt && d.accumulate) return IVLN_E_UNSUPPORTED;  // (the wave-tile epilogue is straight-line code: no D += form)
    const int64_t mtiles = (d.M + 31) / 32;
    const int64_t wgs = wt ? (int64_t)((d.N + 511) / 512) * mtiles : (int64_t)((d.N + 127) / 128) * mtiles;
    if ((d.N + 127) / 128 > 65535) return IVLN_E_UNSUPPORTED;
    if (mode == 0) {
        // (measured inside RedNet: wins at 128 ... 512 workgroups - 256 x 4096 x 1024 35.7 -> 28 us, 256 x 2048 x 1024 28.4 -> 21.6 -,
        //  loses at 64 - 512 x 512 x 2048 - and at 1024 - 256 x 16384 x 512, four rounds of one workgroup per CU)
        if (!wt && (d.Cin < 32 * CB || wgs > 2 * (int64_t)ivln_cu_count() || wgs < ivln_cu_count() / 2)) return IVLN_E_UNSUPPORTED;
        if (wt && wgs < ivln_cu_count()) return IVLN_E_UNSUPPORTED;  // (too few wave tiles to fill the chip: the tiled GEMMs split K)
    }
    d.splits = 1;
    *kind = wt ? 3 : 2;
    const unsigned char* a = (const unsigned char*)d.A_split;
    const long long gb = (long long)(d.a_split_grp_stride * 4);
    if (wt) {
        constexpr size_t lds = 0;  // (the wave-tile form keeps everything in registers)
        dim3 grid((unsigned)mtiles, (unsigned)((d.N + 511) / 512), 1);
        IVLN_LAUNCH_FAMILY(k_conv1x1_bf3_ks<true>, grid, dim3(256), lds, s, d, a, gb);
    } else if (bf3_ks_four_waves(wgs, nch, nw_pin)) {  // two co-resident four-wave workgroups per CU
        constexpr size_t lds = (size_t)4 * 32 * (128 + 4) * 4;
        static_assert(lds <= 80 * 1024, "two four-wave workgroups share a CU's LDS");
        constexpr auto kern = k_conv1x1_bf3_ks<false, 4>;
        if (bf3_set_lds<kern>(lds) != IVLN_OK) return IVLN_E_HIP;
        dim3 grid((unsigned)mtiles, (unsigned)((d.N + 127) / 128), 1);
        IVLN_LAUNCH_FAMILY_NAMED("k_conv1x1_bf3_ks<false>", kern, grid, dim3(256), lds, s, d, a, gb);
        ++g_bf3_ks_waves[3];
    } else {
        constexpr size_t lds = (size_t)8 * 32 * (128 + 4) * 4;
        if (bf3_set_lds<k_conv1x1_bf3_ks<false>>(lds) != IVLN_OK) return IVLN_E_HIP;
        dim3 grid((unsigned)mtiles, (unsigned)((d.N + 127) / 128), 1);
        IVLN_LAUNCH_FAMILY(k_conv1x1_bf3_ks<false>, grid, dim3(512), lds, s, d, a, gb);
        ++g_bf3_ks_waves[2];
    }
    return IVLN_OK;
}

// OIHW fp32 weights -> [32-channel tile][16-channel chunk][tap, padded][piece][lane] x 8 bf16: lane (l31, half) of tile mt
// holds W[32 mt + l31][16 c + 8 half .. + 7][tap] - the A operand of v_mfma_f32_32x32x16_bf16 as one 16-byte load.
__global__ __launch_bounds__(256) void k_conv_bf3_pack(const float* __restrict__ W, int M, int Cin, int KS, uint16_t* __restrict__ out,
                                                       int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int KK = KS * KS, KKP = bf3_taps_padded(KS), nch = (Cin + CB - 1) / CB;
    const int e = (int)(idx & 7), lane = (int)((idx >> 3) & 63);
    int64_t q = idx >> 9;
    const int pl = (int)(q % 3);
    q /= 3;
    const int r = (int)(q % KKP);
    q /= KKP;
    const int c = (int)(q % nch);
    const int mt = (int)(q / nch);
    const int m = mt * 32 + (lane & 31), ci = c * CB + (lane >> 5) * 8 + e;
    const float v = (m < M && ci < Cin && r < KK) ? W[((int64_t)m * Cin + ci) * KK + r] : 0.f;
    uint32_t h, mm, l;
    split3(v, h, mm, l);
    out[idx] = (uint16_t)(pl == 0 ? h : (pl == 1 ? mm : l));
}

template <int KS, int TM, int WM, int WN, int PTH, int PTW, int IMGS, int DA, int ST = 1>
int launch_bf3(const ivln_gemm_desc& d, hipStream_t s, const unsigned char* a_split, int64_t grp_bytes, int nimg, int cps) {
    constexpr int NTB = 64 * WM * WN, BM = 32 * TM * WM, BN = 64 * WN;
    constexpr int PH = ST == 2 ? PTH + 1 : PTH + KS - 1, PWR = ST == 2 ? PTW + 1 : PTW + KS - 1;
    constexpr int NPIX = IMGS * (ST == 2 ? 4 : 1) * PH * PWR * bf3_stage_chunks(KS);  // (stride 2: four phase planes)
    constexpr size_t lds = (size_t)(NPIX * PIXB > 32 * (BN + 4) * 4 ? NPIX * PIXB : 32 * (BN + 4) * 4);
    if constexpr (lds > 160 * 1024) {
        return IVLN_E_UNSUPPORTED;  // (a stride-2 tile whose planes do not fit: the dispatcher picks another)
    } else {
    constexpr auto kern = k_conv_bf3<KS, TM, WM, WN, PTH, PTW, IMGS, DA, false, ST>;
    if (bf3_set_lds<kern>(lds) != IVLN_OK) return IVLN_E_HIP;
    const int tiles_w = (d.Wout + PTW - 1) / PTW, tiles_h = (d.Hout + PTH - 1) / PTH;
    const int groups = (nimg + IMGS - 1) / IMGS;
    dim3 grid(tiles_w * tiles_h * groups, (d.M + BM - 1) / BM, d.splits);
    IVLN_LAUNCH_FAMILY_NAMED("k_conv_bf3", kern, grid, dim3(NTB), lds, s, d, a_split, (long long)grp_bytes, tiles_w, tiles_h, nimg, cps);
    return IVLN_OK;
    }
}

// The fused bottleneck tail (ivln_gemm_desc.fuse_*): the 64 x 128 / 128 x 128 tiles of the 3x3 kernel with the 1x1 expansion behind.
template <int TM, int WM, int WN, int DA>
int launch_bf3_fused(const ivln_gemm_desc& d, hipStream_t s, const unsigned char* a_split, int64_t grp_bytes, int nimg) {
    constexpr int KS = 3, PTW = 32, NTB = 64 * WM * WN, BM = 32 * TM * WM, BN = 64 * WN, PTH = BN / PTW;
    static_assert(NTB == 256, "four waves");
    constexpr int NPIX = (PTH + 2) * (PTW + 2);
    constexpr size_t ybytes = (size_t)BM * (BN + 4) * 4, lds = (size_t)NPIX * PIXB > ybytes ? (size_t)NPIX * PIXB : ybytes;
    constexpr auto kern = k_conv_bf3<KS, TM, WM, WN, PTH, PTW, 1, DA, true>;
    if (bf3_set_lds<kern>(lds) != IVLN_OK) return IVLN_E_HIP;
    const int tiles_w = d.Wout / PTW, tiles_h = d.Hout / PTH;
    dim3 grid(tiles_w * tiles_h * nimg, 1, 1);
    const int nch = d.Cin / CB;
    IVLN_LAUNCH_FAMILY_NAMED("k_conv_bf3", kern, grid, dim3(NTB), lds, s, d, a_split, (long long)grp_bytes, tiles_w, tiles_h, nimg, nch);
    return IVLN_OK;
}

// pixel tile of a block for its pixel count BN and the output width: rows x columns x images
struct Bf3Px { int pth, ptw, imgs; };
inline Bf3Px bf3_px(int BN, int Wout) {
    const int ptw = Wout > 16 ? 32 : (Wout > 8 ? 16 : 8);
    const int pth = ptw == 32 ? BN / 32 : (ptw == 16 ? (BN >= 256 ? 16 : 8) : 8);
    return {pth, ptw, BN / (ptw * pth)};
}

template <int KS, int TM, int WM, int WN, int DA, int ST = 1>
int launch_bf3_px(const ivln_gemm_desc& d, hipStream_t s, const unsigned char* a, int64_t gb, int nimg, int cps) {
    constexpr int BN = 64 * WN;
    if constexpr (ST == 2) {  // stride-2 3x3: the 128- and 256-pixel tiles
        static_assert(KS == 3 && (BN == 128 || BN == 256), "stride-2 tiles");
        if constexpr (BN == 256) {
            if (d.Wout > 16) return launch_bf3<KS, TM, WM, WN, 8, 32, 1, DA, 2>(d, s, a, gb, nimg, cps);
            if (d.Wout > 8) return launch_bf3<KS, TM, WM, WN, 16, 16, 1, DA, 2>(d, s, a, gb, nimg, cps);
            return launch_bf3<KS, TM, WM, WN, 8, 8, 4, DA, 2>(d, s, a, gb, nimg, cps);
        } else {
            if (d.Wout > 16) return launch_bf3<KS, TM, WM, WN, 4, 32, 1, DA, 2>(d, s, a, gb, nimg, cps);
            if (d.Wout > 8) return launch_bf3<KS, TM, WM, WN, 8, 16, 1, DA, 2>(d, s, a, gb, nimg, cps);
            return launch_bf3<KS, TM, WM, WN, 8, 8, 2, DA, 2>(d, s, a, gb, nimg, cps);
        }
    } else
    if constexpr (BN == 512 && KS == 1) {
        return IVLN_E_UNSUPPORTED;  // (four staged chunks of 512 pixels do not fit the LDS)
    } else if constexpr (BN == 512) {
        if (d.Wout > 16) return launch_bf3<KS, TM, WM, WN, 16, 32, 1, DA>(d, s, a, gb, nimg, cps);
        if (d.Wout > 8) return launch_bf3<KS, TM, WM, WN, 16, 16, 2, DA>(d, s, a, gb, nimg, cps);
        if constexpr (KS == 3) return launch_bf3<KS, TM, WM, WN, 8, 8, 8, DA>(d, s, a, gb, nimg, cps);
        return IVLN_E_UNSUPPORTED;
    } else if constexpr (BN == 256) {
        if (d.Wout > 16) return launch_bf3<KS, TM, WM, WN, 8, 32, 1, DA>(d, s, a, gb, nimg, cps);
        if (d.Wout > 8) return launch_bf3<KS, TM, WM, WN, 16, 16, 1, DA>(d, s, a, gb, nimg, cps);
        return launch_bf3<KS, TM, WM, WN, 8, 8, 4, DA>(d, s, a, gb, nimg, cps);
    } else {
        if (d.Wout > 16) return launch_bf3<KS, TM, WM, WN, 4, 32, 1, DA>(d, s, a, gb, nimg, cps);
        if (d.Wout > 8) return launch_bf3<KS, TM, WM, WN, 8, 16, 1, DA>(d, s, a, gb, nimg, cps);
        return launch_bf3<KS, TM, WM, WN, 8, 8, 2, DA>(d, s, a, gb, nimg, cps);
    }
}

// block tiles: {channels, pixels, waves}
constexpr int kBf3Cfgs = 7;
constexpr int kBf3BM[kBf3Cfgs] = {32, 64, 64, 128, 64, 128, 32};
constexpr int kBf3BN[kBf3Cfgs] = {512, 512, 256, 256, 128, 128, 256};

template <int KS>
int launch_bf3_ks(const ivln_gemm_desc& d, hipStream_t s, const unsigned char* a, int64_t gb, int nimg, int cfg, int cps) {
    // weight taps in flight: a tap is 24 MFMAs = 768 pipe cycles per wave (12 = 384 with one channel tile per wave), an L2 /
    // MALL round trip ~2000
    constexpr int DA2 = KS == 1 || KS == 2 ? 2 : 3, DA1 = KS == 1 || KS == 2 ? 4 : (KS == 7 ? 2 : 3);  // (6 / 9 taps ahead measured the same as 3 and cost 36-72 registers)
    if constexpr (KS == 2) {  // (the transposed-conv classes: 4 M rows per output channel - only the tiles their shapes take)
        switch (cfg) {
            case 2: return launch_bf3_px<KS, 1, 2, 4, DA1>(d, s, a, gb, nimg, cps);   // 64 x 256
            case 3: return launch_bf3_px<KS, 2, 2, 4, DA2>(d, s, a, gb, nimg, cps);   // 128 x 256
            case 4: return launch_bf3_px<KS, 1, 2, 2, DA1>(d, s, a, gb, nimg, cps);   // 64 x 128
            case 5: return launch_bf3_px<KS, 2, 2, 2, DA2>(d, s, a, gb, nimg, cps);   // 128 x 128
            default: return IVLN_E_UNSUPPORTED;
        }
    }
    switch (cfg) {
        case 0: return launch_bf3_px<KS, 1, 1, 8, DA1>(d, s, a, gb, nimg, cps);   // 32 x 512, 8 waves
        case 1: return launch_bf3_px<KS, 2, 1, 8, DA2>(d, s, a, gb, nimg, cps);   // 64 x 512
        case 2: return launch_bf3_px<KS, 1, 2, 4, DA1>(d, s, a, gb, nimg, cps);   // 64 x 256
        case 3: return launch_bf3_px<KS, 2, 2, 4, DA2>(d, s, a, gb, nimg, cps);   // 128 x 256
        case 4: return launch_bf3_px<KS, 1, 2, 2, DA1>(d, s, a, gb, nimg, cps);   // 64 x 128, 4 waves: several workgroups per CU
        case 5: return launch_bf3_px<KS, 2, 2, 2, DA2>(d, s, a, gb, nimg, cps);   // 128 x 128, 4 waves
        default: return launch_bf3_px<KS, 1, 1, 4, DA1>(d, s, a, gb, nimg, cps);  // 32 x 256, 4 waves: two workgroups per CU
    }
}


// stride-2 3x3 (k_conv_bf3<..., ST = 2>): the tiles whose four phase planes fit the LDS
int launch_bf3_s2(const ivln_gemm_desc& d, hipStream_t s, const unsigned char* a, int64_t gb, int nimg, int cfg, int cps) {
    // (k_conv_bf3<..., ST = 2> stages without the ragged-chunk test - Bf3GroupStager<..., RAGGED = false>: a last chunk of fewer
    //  than 16 channels would read the next image's)
    if (d.Cin % CB != 0) return IVLN_E_UNSUPPORTED;
    switch (cfg) {
        case 2: return launch_bf3_px<3, 1, 2, 4, 3, 2>(d, s, a, gb, nimg, cps);   // 64 x 256
        case 3: return launch_bf3_px<3, 2, 2, 4, 3, 2>(d, s, a, gb, nimg, cps);   // 128 x 256
        case 4: return launch_bf3_px<3, 1, 2, 2, 3, 2>(d, s, a, gb, nimg, cps);   // 64 x 128
        case 5: return launch_bf3_px<3, 2, 2, 2, 3, 2>(d, s, a, gb, nimg, cps);   // 128 x 128
        case 6: return launch_bf3_px<3, 1, 1, 4, 3, 2>(d, s, a, gb, nimg, cps);   // 32 x 256
        default: return IVLN_E_UNSUPPORTED;
    }
}


// ------------------------------------------------------------------------------------------------------------------
// Weight gradient of a 7x7 same-size conv on the same arithmetic (map CNN, base_il_trainer.py:173-219):
//   dW[co][(ci,kh,kw)] = sum over pixels p of dy[co][p] * x[ci][p + (kh,kw) - pad]      M = Cout, N = Cin * 49, K = pixels.
// K of an MFMA = 16 consecutive pixels of an output row (W = 8: two rows of 8), a lane's 8 k-values = 8 consecutive pixels.
//   * A = dy: a STRIP of 128 pixels (2 / 4 / 8 rows of one image, or two 8x8 images) per (channel, piece) as a row of 256 + 16
//     bytes in LDS: one ds_read_b128 per fragment, 16 lanes on 16 distinct bank quads;
//   * B = x: the column's (kh, kw) moves the fragment by kw PIXELS = 2 kw bytes in a bf16 row, which ds_read_b128 cannot
//     address.  The patch of the strip ((rows + 6) x (W + 6) pixels of the <= 7 / 12 input channels the column tile touches)
//     is kept as TWO copies per piece, pixel pairs (2j, 2j+1) and (2j+1, 2j+2): every kw is 4-byte aligned in one of them and
//     a fragment is four ds_read_b32 from a per-lane base ((ci, kh, kw) of the lane's column) + an immediate (the k-step);
//   * strips are split over blockIdx.z (M x N is tiny, K is millions of pixels): raw slabs, reduced in fixed order by the
//     family's k_splitk_epilogue like the fp32 weight-gradient kernel's;
//   * the next strip's dy pairs and x triples fly under the MFMA phase in registers, are split and written after the barrier.
// ------------------------------------------------------------------------------------------------------------------
// XE (ivln_gemm_desc.split_ok == 2: the caller's promise that every x value is exact in bf16 - the first layer's one-hot map
// features): x is staged as ONE piece (its upper 16 bits; a value with lower bits set poisons the result with NaNs), the three
// products against its lower pieces do not exist, the x region is a third (43 KB of LDS with dy for a 32 x 256 tile: three
// workgroups per CU hide each other's strip loads and barriers) and the kernel fits three waves per SIMD.
template <int TM, int WM, int WN, int W, bool XE = false>
__global__ __launch_bounds__(64 * WM * WN, XE ? 3 : 1) void k_wgrad_bf3(const ivln_gemm_desc p, int nimg, int strips_total, int strips_per_split) {
    constexpr int NTB = 64 * WM * WN, TN = 2, KS = 7, KK = 49;
    constexpr int NPX = XE ? 1 : 3;                                // pieces of x in LDS
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr int IMS = W == 8 ? 2 : 1, ROWS = 128 / (W * IMS);   // a strip: IMS images x ROWS rows x W columns = 128 pixels
    constexpr int PR = ROWS + KS - 1, PRT = IMS * PR, PWP = W + KS - 1;
    constexpr int XW = PWP / 2 + 1;                                // pixel-pair words a patch row needs in either copy
    constexpr int XP = (XW | 1);                                   // row pitch in words (odd)
    constexpr int NCIB = (BN + KK - 1) / KK + 1;                   // input channels a column tile can touch
    constexpr int DP = 272;                                        // bytes per (channel, piece) row of dy: 128 bf16 + 16
    constexpr int CHB = PRT * XP * 4, PLB = NCIB * CHB, CPYB = NPX * PLB;
    constexpr int DYB = 3 * BM * DP;                               // dy region in front of the x region
    constexpr int ND = BM * 64, NDI = (ND + NTB - 1) / NTB, NX = NCIB * PRT * XW, NXI = (NX + NTB - 1) / NTB;
    constexpr bool HAS_LITE = TM == 1 && !XE;  // (the 32-channel layer: the one whose x is the one-hot map features)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const xS = smem + DYB;

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int wm = wave / WN, wn = wave % WN;
    const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM;
    const int ci_lo = n0 / KK;
    const int spi = p.Hout / ROWS;  // strips per image (W = 8: one strip = two whole images)
    const int HWo = p.HoWo, HWi = p.Hin * p.Win;
    const float* __restrict__ dy = p.A;
    const float* __restrict__ x = p.B;

    // per-lane operand bases
    int abase[TM], bbase[TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) abase[tm] = ((wm * TM + tm) * 32 + l31) * DP + half * 16;
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int n = min(n0 + (wn * TN + tn) * 32 + l31, p.N - 1);  // (columns past N compute a duplicate; never stored)
        const int ci = n / KK, rem = n - ci * KK, kh = rem / KS, kw = rem - kh * KS, sft = kw & 1;
        bbase[tn] = sft * CPYB + (ci - ci_lo) * CHB + kh * (XP * 4) + ((kw - sft) >> 1) * 4 + (W >= 16 ? half * 16 : half * (XP * 4));
    }

    float2 dyv[NDI];
    float xv[NXI][3];
    // x items of this thread, derived once: offset of patch column 2j relative to the strip's (image 0, row 0) origin, the
    // LDS word, and what does not depend on the strip - channel and column validity (bits 0-2), image of the pair (bit 3),
    // patch row (bits 4..) - so that a strip costs an add and a row test per item, not three divisions
    int xrel[NXI], xdst[NXI], xinf[NXI];
#pragma unroll
    for (int i = 0; i < NXI; ++i) {
        const int idx = t + i * NTB;
        const int cl = idx / (PRT * XW), rem = idx - cl * (PRT * XW);
        const int prow = rem / XW, j = rem - prow * XW;
        const int il = prow / PR, pr = prow - il * PR;
        const bool cok = idx < NX && ci_lo + cl < p.Cin;
        int m = 0;
#pragma unroll
        for (int e = 0; e < 3; ++e) m |= (cok && (unsigned)(2 * j + e - p.pad) < (unsigned)p.Win) ? (1 << e) : 0;
        xinf[i] = m | (il << 3) | (pr << 4);
        xrel[i] = (int)((int64_t)il * p.in_img_stride + (int64_t)(ci_lo + cl) * HWi + (pr - p.pad) * p.Win + 2 * j - p.pad);
        xdst[i] = idx < NX ? cl * CHB + prow * (XP * 4) + j * 4 : -1;
    }
    auto strip_origin = [&](int st, int& img0, int& row0) {
        img0 = (st / spi) * IMS;
        row0 = (st - (st / spi) * spi) * ROWS;
    };
    auto load_strip = [&](int st) {
        int img0, row0;
        strip_origin(st, img0, row0);
        int tt = t;
        asm volatile("" : "+v"(tt));
#pragma unroll
        for (int i = 0; i < NDI; ++i) {  // dy: (channel, pixel pair)
            const int idx = tt + i * NTB;
            const int co = idx >> 6, px = (idx & 63) * 2;
            const int il = px / (ROWS * W), q = px - il * (ROWS * W);
            const int img = img0 + il;
            const bool ok = idx < ND && m0 + co < p.M && img < nimg;
            dyv[i] = ok ? *reinterpret_cast<const float2*>(dy + ((int64_t)img * p.M + m0 + co) * HWo + row0 * W + q) : make_float2(0.f, 0.f);
        }
        const float* const xo = x + (int64_t)img0 * p.in_img_stride + row0 * p.Win;
#pragma unroll
        for (int i = 0; i < NXI; ++i) {  // x: (channel, patch row, pixel-pair word): columns 2j, 2j+1, 2j+2 of the patch
            const int inf = xinf[i];
            const int hi = row0 + (inf >> 4) - p.pad;
            const bool rok = img0 + ((inf >> 3) & 1) < nimg && (unsigned)hi < (unsigned)p.Hin;
#pragma unroll
            for (int e = 0; e < 3; ++e) xv[i][e] = (rok && ((inf >> e) & 1)) ? xo[xrel[i] + e] : 0.f;
        }
    };
    auto stage_strip = [&]() -> uint32_t {  // returns the OR of the x values' lower pieces (0: the strip's patch is bf16-exact)
        uint32_t nzx = 0;
        int tt = t;
        asm volatile("" : "+v"(tt));
#pragma unroll
        for (int i = 0; i < NDI; ++i) {
            const int idx = tt + i * NTB;
            const int co = idx >> 6, pr = idx & 63;
            uint32_t H, M, L;
            split3_pair(dyv[i].x, dyv[i].y, H, M, L);
            unsigned char* d = smem + co * DP + pr * 4;
            if (ND % NTB == 0 || idx < ND) {
                *reinterpret_cast<uint32_t*>(d) = H;
                *reinterpret_cast<uint32_t*>(d + BM * DP) = M;
                *reinterpret_cast<uint32_t*>(d + 2 * BM * DP) = L;
            }
        }
        if constexpr (XE) {
#pragma unroll
            for (int i = 0; i < NXI; ++i) {  // exact values: the upper halves ARE the first pieces, the lower halves must be zero
                const uint32_t u0 = __float_as_uint(xv[i][0]), u1 = __float_as_uint(xv[i][1]), u2 = __float_as_uint(xv[i][2]);
                nzx |= (u0 | u1 | u2) & 0xFFFFu;
                unsigned char* d = xS + xdst[i];
                if (xdst[i] >= 0) {
                    *reinterpret_cast<uint32_t*>(d) = (u0 >> 16) | (u1 & 0xFFFF0000u);         // pair (2j, 2j+1)
                    *reinterpret_cast<uint32_t*>(d + CPYB) = (u1 >> 16) | (u2 & 0xFFFF0000u);  // pair (2j+1, 2j+2)
                }
            }
            return nzx;
        }
#pragma unroll
        for (int i = 0; i < NXI; ++i) {
            uint32_t pa0, pa1, pa2, pb0, pb1, pb2;
            split3_pair(xv[i][0], xv[i][1], pa0, pa1, pa2);  // pairs (2j, 2j+1)
            split3_pair(xv[i][1], xv[i][2], pb0, pb1, pb2);  // pairs (2j+1, 2j+2)
            nzx |= pa1 | pa2 | pb1 | pb2;
            unsigned char* d = xS + xdst[i];
            if (xdst[i] >= 0) {
                *reinterpret_cast<uint32_t*>(d) = pa0;
                *reinterpret_cast<uint32_t*>(d + PLB) = pa1;
                *reinterpret_cast<uint32_t*>(d + 2 * PLB) = pa2;
                *reinterpret_cast<uint32_t*>(d + CPYB) = pb0;
                *reinterpret_cast<uint32_t*>(d + CPYB + PLB) = pb1;
                *reinterpret_cast<uint32_t*>(d + CPYB + 2 * PLB) = pb2;
            }
        }
        return nzx;
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[tm][tn][i] = 0.f;

    const int s_beg = blockIdx.z * strips_per_split, s_end = min(strips_total, s_beg + strips_per_split);
    unsigned long long tk0 = BF3_T(), t_stage = 0, t_mma = 0;
    (void)tk0, (void)t_stage, (void)t_mma;
#ifdef BF3_TIMING
    const unsigned long long cyc0 = clock64();
#endif
    uint32_t inexact = 0;  // (XE: lower bits seen in x)
    if (s_beg < s_end) load_strip(s_beg);
    for (int st = s_beg; st < s_end; ++st) {
        const unsigned long long ta = BF3_T();
        const uint32_t nzx = stage_strip();
        if constexpr (XE) inexact |= nzx;
        // (a strip whose x patch is bf16-exact - the first layer's one-hot map features - has zero lower pieces: the products
        //  against them are not issued and their fragments not read: a third of the 4-byte LDS reads that bound this kernel)
        const bool lite = HAS_LITE ? __syncthreads_or((int)(nzx != 0)) == 0 : (__syncthreads(), false);
        const unsigned long long tb = BF3_T();
        t_stage += tb - ta;
        if (st + 1 < s_end) load_strip(st + 1);  // in flight under the MFMA phase
        auto ksteps = [&](auto lite_tag) {
            constexpr bool LITE = decltype(lite_tag)::value;
            constexpr int NPL = LITE ? 1 : 3;
            auto read_ab = [&](int ks, bf16x8 (&a)[TM][3], bf16x8 (&b)[TN][3]) {
                // the k-step's 16 pixels: W >= 16 a run of a row (the lane halves take its two octets), W = 8 two rows of an image
                const int aoff = ks * 32;
                const int boff = W >= 16 ? ((ks * 16) / W) * (XP * 4) + (((ks * 16) % W) >> 1) * 4
                                         : ((ks / 4) * PR + (ks % 4) * 2) * (XP * 4);
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl)
                        a[tm][pl] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const v4i*>(smem + pl * (BM * DP) + abase[tm] + aoff));
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                    for (int pl = 0; pl < NPL; ++pl) {
                        const uint32_t* q = reinterpret_cast<const uint32_t*>(xS + bbase[tn] + pl * PLB + boff);
                        v4i v;
                        v.x = (int)q[0], v.y = (int)q[1], v.z = (int)q[2], v.w = (int)q[3];
                        b[tn][pl] = __builtin_bit_cast(bf16x8, v);
                    }
            };
            bf16x8 aq[2][TM][3], bq[2][TN][3];
            read_ab(0, aq[0], bq[0]);
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                if (ks + 1 < 8) read_ab(ks + 1, aq[(ks + 1) & 1], bq[(ks + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
                bf3_products<LITE ? BF3_THREE : BF3_SIX>(acc, aq[ks & 1], bq[ks & 1]);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        if constexpr (XE) {
            ksteps(std::true_type{});
        } else if constexpr (HAS_LITE) {
            if (lite) ksteps(std::true_type{});
            else ksteps(std::false_type{});
        } else {
            ksteps(std::false_type{});
        }
        __syncthreads();
        t_mma += BF3_T() - tb;
    }
    // XE: a broken promise must not pass for a gradient - every output of a workgroup that saw an inexact x value becomes a NaN
    const bool poison = XE ? __syncthreads_or((int)(inexact != 0)) != 0 : false;
#ifdef BF3_TIMING
    if (threadIdx.x == 0) {
        const int b = ((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) & 8191;
        g_bf3_stamp[b * 8 + 0] = wall_clock64() - tk0;
        g_bf3_stamp[b * 8 + 1] = t_stage;
        g_bf3_stamp[b * 8 + 2] = t_mma;
        g_bf3_stamp[b * 8 + 3] = clock64() - cyc0;
    }
#endif

    // acc[r] -> channel (r&3) + 8*(r>>2) + 4*half, column l31 of the sub-tile: 32 consecutive columns per store instruction
    // always a raw slab, even a single one (the reduction launch applies the epilogue): ivln_gemm_f32's epilogue_store inlined
    // 64 times made the nest too large to unroll, and the accumulators, then indexed dynamically, lived in scratch
    float* const slab = p.ws + (int64_t)blockIdx.z * p.M * p.N;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + (wn * TN + tn) * 32 + l31;
                const int m = m0 + (wm * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (m < p.M && n < p.N) slab[(int64_t)m * p.N + n] = poison ? __builtin_nanf("") : acc[tm][tn][r];
            }
}

template <int TM, int WM, int WN, int W, bool XE = false>
int launch_wgrad_bf3(const ivln_gemm_desc& d, hipStream_t s, int nimg, int strips, int sps) {
    constexpr int BM = 32 * TM * WM, BN = 64 * WN, IMS = W == 8 ? 2 : 1, ROWS = 128 / (W * IMS);
    constexpr int PRT = IMS * (ROWS + 6), XP = ((W + 6) / 2 + 1) | 1, NCIB = (BN + 48) / 49 + 1;
    constexpr size_t lds = (size_t)3 * BM * 272 + (size_t)(XE ? 2 : 6) * NCIB * PRT * XP * 4;
    static_assert(lds <= 160 * 1024, "strip does not fit");
    constexpr auto kern = k_wgrad_bf3<TM, WM, WN, W, XE>;
    if (bf3_set_lds<kern>(lds) != IVLN_OK) return IVLN_E_HIP;
    dim3 grid((d.N + BN - 1) / BN, (d.M + BM - 1) / BM, d.splits);
    IVLN_LAUNCH_FAMILY_NAMED("k_wgrad_bf3", kern, grid, dim3(64 * WM * WN), lds, s, d, nimg, strips, sps);
    return IVLN_OK;
}

template <int TM, int WM, int WN>
int launch_wgrad_bf3_w(const ivln_gemm_desc& d, hipStream_t s, int nimg, int strips, int sps) {
    switch (d.Wout) {
        case 64: return launch_wgrad_bf3<TM, WM, WN, 64>(d, s, nimg, strips, sps);
        case 32: return launch_wgrad_bf3<TM, WM, WN, 32>(d, s, nimg, strips, sps);
        case 16: return launch_wgrad_bf3<TM, WM, WN, 16>(d, s, nimg, strips, sps);
        default: return launch_wgrad_bf3<TM, WM, WN, 8>(d, s, nimg, strips, sps);
    }
}

}  // namespace

extern "C" int64_t ivln_conv_split_words(int M, int Cin, int KS) {
    if ((KS != 1 && KS != 2 && KS != 3 && KS != 7) || M <= 0 || Cin <= 0) return 0;
    return (int64_t)((M + 31) / 32) * ((Cin + CB - 1) / CB) * bf3_taps_padded(KS) * (3 * 1024 / 4);
}

extern "C" int ivln_conv_split_weights_f32(const float* W, int M, int Cin, int KS, void* out, void* stream) {
    const int64_t words = ivln_conv_split_words(M, Cin, KS);
    if (!W || !out || words <= 0) return IVLN_E_INVALID;
    const int64_t total = words * 2;
    hipLaunchKernelGGL(k_conv_bf3_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, W, M, Cin, KS,
                       (uint16_t*)out, total);
    return hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP;
}

namespace {
// ------------------------------------------------------------------------------------------------------------------
// RedNet's stems (rednet.py:201-210, 190-199: conv1 3 -> 64 and conv1_d 1 -> 64; 7x7, stride 2, pad 3) on the same arithmetic.
// Three or one input channels leave the 16-channel chunks of the kernels above 81 / 94 % empty, so K is laid out the other
// way round: a K step of 16 = TWO kernel rows (channel c, row kh) x 8 columns (kw = 0 .. 6 and a zero) - 11 steps for the 21
// rows of the RGB stem, 4 for the 7 of the depth stem (one zero row each).  NO LDS and no barrier anywhere:
//   * a wave owns 32 output channels x 128 consecutive pixels of ONE output row; as in the 1x1 kernels tile e holds pixel
//     4 l31 + e in column l31, so register r of the four accumulators is a float4 of the output row;
//   * lane (l31, half) needs, for its kernel row of the step, input columns 2 (4 l31 + e) - 3 + kw: the 14 consecutive floats
//     8 l31 - 3 .. 8 l31 + 10 of input row 2 ho - 3 + kh, read as FOUR aligned 16-byte loads (8 l31 - 4 ..); rows and column
//     groups outside the image are out-of-range buffer offsets, i.e. zeros - the padding costs nothing;
//   * element pairs (2 t + 1, 2 t + 2), t = 0 .. 6, are split into the three bf16 pieces once (v_cvt_pk_bf16_f32 leaves the
//     word the fragment wants); tile e's B fragment is pairs e .. e + 3 - every register index static;
//   * weights: the image of ivln_conv_stem_split_weights_f32 - [32-channel tile][step][piece][lane] x 8 bf16, lane (l31, half)
//     holding W[32 mt + l31][row 2 s + half][kw 0 .. 6], 0 - global -> registers two steps ahead;
//   * epilogue: the 1x1 wave-tile kernel's (scale / shift, residual in front of or BEHIND the ReLU - the depth stem's output
//     added to the RGB stem's, rednet.py:196 -, 16-byte stores).
// ------------------------------------------------------------------------------------------------------------------
template <int CIN>
__global__ __launch_bounds__(256, 2) void k_conv7s2_bf3(const ivln_gemm_desc p, const unsigned char* a_split, int segs, int items) {
    constexpr int Q = CIN * 7, S = (Q + 1) / 2, TN = 4;
    constexpr unsigned OOB = 0x80000000u;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const BlockId bid = xcd_block_id(p.no_xcd_remap);
    const int item = bid.x * 4 + wave;  // (channel tile, row segment, output row, image), channel tile fastest: a workgroup shares its input rows
    if (item >= items) return;
    const int mtiles = (p.M + 31) / 32;
    const int mt = item % mtiles;
    int rest = item / mtiles;
    const int seg = rest % segs;
    rest /= segs;
    const int ho = rest % p.Hout, img = rest / p.Hout;
    const int m0 = mt * 32;
    const int H = p.Hin, W = p.Win, HW = p.HoWo;
    const int b = 256 * seg + 8 * l31;  // input column of the lane's first pixel (2 * (128 seg + 4 l31))
    const bool in0 = b >= 4, in3 = b + 8 < W;
    const __amdgpu_buffer_rsrc_t rB = bf3_rsrc(p.B);
    const __amdgpu_buffer_rsrc_t rA = bf3_rsrc(a_split + (int64_t)mt * S * 3072);
    const int64_t img_off = (int64_t)img * p.in_img_stride + b - 4;
    auto load_x = [&](int s, v4i (&xb)[4]) {
        const int q = 2 * s + half;  // this half's kernel row (channel c, row kh) of step s
        const int c = q / 7, kh = q - 7 * c;
        const int hi = 2 * ho - 3 + kh;
        const bool ok = q < Q && (unsigned)hi < (unsigned)H;
        const unsigned off = (unsigned)((img_off + ((int64_t)c * H + hi) * W) * 4);
        const unsigned o12 = ok ? off : OOB, o0 = ok && in0 ? off : OOB, o3 = ok && in3 ? off : OOB;
        xb[0] = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)o0, 0, 0);
        xb[1] = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)(o12 + 16u), 0, 0);
        xb[2] = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)(o12 + 32u), 0, 0);
        xb[3] = __builtin_amdgcn_raw_buffer_load_b128(rB, (int)(o3 + 48u), 0, 0);
    };
    auto load_a = [&](int s, v4i (&ab)[3]) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) ab[pl] = __builtin_amdgcn_raw_buffer_load_b128(rA, (s * 3 + pl) * 1024 + lane * 16, 0, 0);
    };
    f32x16 acc[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[tn][i] = 0.f;
    {
        v4i xb[3][4], ab[3][3];
        load_a(0, ab[0]);
        load_x(0, xb[0]);
        if (S > 1) load_a(1, ab[1]), load_x(1, xb[1]);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (s + 2 < S) load_a(s + 2, ab[(s + 2) % 3]), load_x(s + 2, xb[(s + 2) % 3]);  // two steps ahead
            uint32_t Hh[7], Mm[7], Ll[7];
#pragma unroll
            for (int u = 0; u < 7; ++u) {
                const int i0 = 2 * u + 1, i1 = 2 * u + 2;
                split3_pair(__int_as_float(xb[s % 3][i0 >> 2][i0 & 3]), __int_as_float(xb[s % 3][i1 >> 2][i1 & 3]), Hh[u], Mm[u], Ll[u]);
            }
            v4i bq[TN][3];
#pragma unroll
            for (int e = 0; e < TN; ++e)
#pragma unroll
                for (int i = 0; i < 4; ++i) bq[e][0][i] = (int)Hh[e + i], bq[e][1][i] = (int)Mm[e + i], bq[e][2][i] = (int)Ll[e + i];
            bf3_products(acc, ab[s % 3], bq);
        }
    }
    // ---- epilogue (the wave-tile 1x1 kernel's): register r of the four tiles = channel (r & 3) + 8 (r >> 2) + 4 half at pixels
    // 4 l31 .. + 3; operands requested first, straight-line code between the stores (BF3_STORE_GUARD) ----
    const int pp = ho * p.Wout + 128 * seg + 4 * l31;
    const int mrem = p.M - m0 - 4 * half;
    const int me0 = m0 + 4 * half;
    const unsigned off0 = (unsigned)(((img * p.Ctot + m0 + 4 * half) * HW + pp) * 4);
    const __amdgpu_buffer_rsrc_t rR = bf3_rsrc(p.residual), rS = bf3_rsrc(p.scale), rH = bf3_rsrc(p.shift), rD = bf3_rsrc(p.D);
    const bool has_res = p.residual != nullptr, has_sc = p.scale != nullptr, has_sh = p.shift != nullptr;
    const float relu_lo = p.relu ? 0.f : -__builtin_huge_valf();
    const bool res_post = p.residual_after_relu != 0;
    v4i rres[16];
    float esc[16], esh[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int cs = (r & 3) + 8 * (r >> 2);
        const bool ok = cs < mrem;
        esc[r] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rS, ok && has_sc ? me0 * 4 : (int)OOB, cs * 4, 0));
        esh[r] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rH, ok && has_sh ? me0 * 4 : (int)OOB, cs * 4, 0));
        rres[r] = __builtin_amdgcn_raw_buffer_load_b128(rR, ok && has_res ? (int)off0 : (int)OOB, cs * HW * 4, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int cs = (r & 3) + 8 * (r >> 2);
        float4 v = make_float4(acc[0][r], acc[1][r], acc[2][r], acc[3][r]);
        const float sc = has_sc ? esc[r] : 1.f, sh = esh[r];
        v.x = fmaf(v.x, sc, sh), v.y = fmaf(v.y, sc, sh), v.z = fmaf(v.z, sc, sh), v.w = fmaf(v.w, sc, sh);
        const float r0 = __int_as_float(rres[r][0]), r1 = __int_as_float(rres[r][1]), r2 = __int_as_float(rres[r][2]), r3 = __int_as_float(rres[r][3]);
        v.x += res_post ? 0.f : r0, v.y += res_post ? 0.f : r1, v.z += res_post ? 0.f : r2, v.w += res_post ? 0.f : r3;
        const float lo = relu_lo;
        v.x = fmaxf(v.x, lo), v.y = fmaxf(v.y, lo), v.z = fmaxf(v.z, lo), v.w = fmaxf(v.w, lo);
        v.x += res_post ? r0 : 0.f, v.y += res_post ? r1 : 0.f, v.z += res_post ? r2 : 0.f, v.w += res_post ? r3 : 0.f;
        v4i o;
        o[0] = __float_as_int(v.x), o[1] = __float_as_int(v.y), o[2] = __float_as_int(v.z), o[3] = __float_as_int(v.w);
        __builtin_amdgcn_raw_buffer_store_b128(o, rD, cs < mrem ? (int)off0 : (int)OOB, cs * HW * 4, 0);
        BF3_STORE_GUARD();
    }
}

// [32-channel tile][step][piece][lane] x 8 bf16 of the stem kernel above: lane (l31, half), element j = W[32 mt + l31][c][kh][j] with
// (c, kh) = kernel row 2 step + half, zero for j = 7 and rows past the last
__global__ __launch_bounds__(256) void k_conv7s2_pack(const float* __restrict__ W, int M, int Cin, uint16_t* __restrict__ out, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int S = (Cin * 7 + 1) / 2;
    const int j = (int)(idx & 7), lane = (int)((idx >> 3) & 63);
    int64_t q = idx >> 9;
    const int pl = (int)(q % 3);
    q /= 3;
    const int st = (int)(q % S);
    const int mt = (int)(q / S);
    const int m = mt * 32 + (lane & 31), row = 2 * st + (lane >> 5);
    const float v = (m < M && row < Cin * 7 && j < 7) ? W[((int64_t)m * Cin * 7 + row) * 7 + j] : 0.f;
    uint32_t h, mm, l;
    split3(v, h, mm, l);
    out[idx] = (uint16_t)(pl == 0 ? h : (pl == 1 ? mm : l));
}

}  // namespace

extern "C" int64_t ivln_conv_stem_split_words(int M, int Cin) {
    if (M <= 0 || (Cin != 1 && Cin != 3)) return 0;
    return (int64_t)((M + 31) / 32) * ((Cin * 7 + 1) / 2) * (3 * 1024 / 4);
}

extern "C" int ivln_conv_stem_split_weights_f32(const float* W, int M, int Cin, void* out, void* stream) {
    const int64_t words = ivln_conv_stem_split_words(M, Cin);
    if (!W || !out || words <= 0) return IVLN_E_INVALID;
    const int64_t total = words * 2;
    hipLaunchKernelGGL(k_conv7s2_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, W, M, Cin, (uint16_t*)out, total);
    return hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP;
}

namespace {
// The stems' launcher: 7x7, stride 2, pad 3, one or three input channels, output rows of whole 128-pixel segments
int bf3_stem_launch(ivln_gemm_desc& d, hipStream_t s) {
    if ((d.Cin != 1 && d.Cin != 3) || d.pad != 3 || d.dil != 1 || d.Hin != 2 * d.Hout || d.Win != 2 * d.Wout || d.Wout % 128 != 0 ||
        d.K != d.Cin * 49 || d.HoWo != d.Hout * d.Wout || d.N % d.HoWo != 0 || d.dmode != DMODE_NCHW || d.amode != AMODE_MK)
        return IVLN_E_UNSUPPORTED;
    if (d.grp_imgs > 0 || d.accumulate || d.defer_epilogue || d.splits > 1 || d.stat_partials || d.img_run_flags || d.fuse_A_split)
        return IVLN_E_UNSUPPORTED;
    if ((d.in_img_stride & 3) || ((((uintptr_t)d.B) | ((uintptr_t)d.D) | ((uintptr_t)d.residual)) & 15)) return IVLN_E_UNSUPPORTED;
    const int64_t nimg = d.N / d.HoWo;
    if (nimg * d.in_img_stride * 4 >= (int64_t)1 << 31 || nimg * d.Ctot * d.HoWo * 4 >= (int64_t)1 << 31) return IVLN_E_UNSUPPORTED;  // byte offsets of the buffer accesses
    const int segs = d.Wout / 128;
    const int64_t items = nimg * d.Hout * segs * ((d.M + 31) / 32);
    if (items >= (int64_t)1 << 30) return IVLN_E_UNSUPPORTED;
    d.splits = 1;
    const dim3 grid((unsigned)((items + 3) / 4));
    const unsigned char* a = (const unsigned char*)d.A_split;
    if (d.Cin == 3) IVLN_LAUNCH_FAMILY(k_conv7s2_bf3<3>, grid, dim3(256), 0, s, d, a, segs, (int)items);
    else IVLN_LAUNCH_FAMILY(k_conv7s2_bf3<1>, grid, dim3(256), 0, s, d, a, segs, (int)items);
    return IVLN_OK;
}
}  // namespace

// Eligibility + tile choice.  IVLN_E_UNSUPPORTED sends the caller to the fp32 MFMA kernels.
// What went through this kernel since the last reset: algorithmic FLOPs (2 M N K of the convs it took) and launches -
// bench.py prices them against the bf16 peak / 6 instead of the fp32 MFMA peak.  Host-side tally, not thread-safe.
static double g_bf3_flops = 0.0;
static long long g_bf3_launches = 0;
static long long g_bf3_kind[4] = {0, 0, 0, 0};  // launches by form: tiled | 3x3 K-split over waves | 1x1 K-split over waves | 1x1 wave tiles
extern "C" int ivln_conv_split_counters(double* flops, long long* launches, int reset) {
    if (flops) *flops = g_bf3_flops;
    if (launches) *launches = g_bf3_launches;
    if (reset) g_bf3_flops = 0.0, g_bf3_launches = 0;
    return IVLN_OK;
}
/* launches of the split-bf16 conv kernels by form since the last reset: [0] tiled (k_conv_bf3), [1] 3x3 with K split over the
 * waves (k_conv_bf3_ks), [2] 1x1 with K split over the waves, [3] 1x1 wave tiles (k_conv1x1_bf3_ks) */
extern "C" int ivln_conv_split_kinds(long long* out4, int reset) {
    if (out4) for (int i = 0; i < 4; ++i) out4[i] = g_bf3_kind[i];
    if (reset) for (int i = 0; i < 4; ++i) g_bf3_kind[i] = 0;
    return IVLN_OK;
}
/* launches of the K-split kernels by wave count since the last reset: [0] k_conv_bf3_ks with 8 waves, [1] with 4,
 * [2] k_conv1x1_bf3_ks' K-split form with 8 waves, [3] with 4 ([0] + [1] and [2] are launches ivln_conv_split_kinds counts
 * under [1] and [2]; the pooled map-CNN kernel, also under its [1], is not counted here) */
extern "C" int ivln_conv_ks_waves(long long* out4, int reset) {
    if (out4) for (int i = 0; i < 4; ++i) out4[i] = g_bf3_ks_waves[i];
    if (reset) for (int i = 0; i < 4; ++i) g_bf3_ks_waves[i] = 0;
    return IVLN_OK;
}

#ifdef BF3_TIMING
extern "C" int ivln_conv_bf3_stamps(unsigned long long* host, int n) {
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_bf3_stamp), sizeof(unsigned long long) * n) != hipSuccess) return -1;
    void* dp = nullptr;  // (cleared for the next launch: a smaller grid leaves no stale entries behind)
    if (hipGetSymbolAddress(&dp, HIP_SYMBOL(g_bf3_stamp)) != hipSuccess) return -1;
    return hipMemset(dp, 0, sizeof(g_bf3_stamp)) == hipSuccess ? 0 : -1;
}
#endif

int ivln_conv_bf3_launch(ivln_gemm_desc& d, hipStream_t s, bool force) {
    if (!d.A_split) return IVLN_E_UNSUPPORTED;
    // every launch below returns through here: the tally of ivln_conv_split_counters / _kinds, and the caller's stat_tiles
    // (st < 0: the path does not know stat_partials' caller and leaves the word alone)
    auto done = [&](int rc, double flops, int kind, int st) {
        if (rc == IVLN_OK) {
            g_bf3_flops += flops, ++g_bf3_launches, ++g_bf3_kind[kind];
            if (st >= 0 && d.stat_tiles) *d.stat_tiles = st;
        }
        return rc;
    };
    const double flops = 2.0 * d.M * (double)d.N * d.K;  // algorithmic FLOPs of the conv
    if (d.pool2) {  // a map-CNN block as one launch (k_conv7_pool_bf3): K split over the waves, the CBRA tail in the epilogue
        return done(bf3_conv7_pool_launch(d, s), flops, 1, -1);
    }
    const int KS = d.bmode == BMODE_CONV1X1 ? 1 : conv_ks(d.bmode);
    if ((KS != 1 && KS != 2 && KS != 3 && KS != 7) || d.amode != AMODE_MK || d.dil != 1) return IVLN_E_UNSUPPORTED;
    // RedNet's stems: A_split is the image of ivln_conv_stem_split_weights_f32 (the caller's contract)
    if (KS == 7 && d.stride == 2) return done(bf3_stem_launch(d, s), flops, 0, 0);
    // (the 2 x 2 window only as the stacked transposed-conv classes; a 1x1 conv may store them too: the 2 x 2 stride-2 upsampling convs)
    const bool up1 = KS == 1 && d.dmode == DMODE_NCHW_UP2X4;
    if (!up1 && d.dmode != (KS == 2 ? DMODE_NCHW_UP2X4 : DMODE_NCHW)) return IVLN_E_UNSUPPORTED;
    if (up1) {  // stacked one-tap classes: the register-built stride-1 1x1 kernels with their 2 x 2-block epilogue, or nothing
        static const bool convt_off1 = getenv("IVLN_BF3_CONVT") && getenv("IVLN_BF3_CONVT")[0] == '0';
        if ((convt_off1 && !force) || (d.M & 3) || d.Ctot * 4 != d.M || d.grp_imgs > 0 || d.accumulate || d.residual_after_relu || d.defer_epilogue ||
            d.splits > 1 || d.stat_partials || d.img_run_flags || d.fuse_A_split || (d.Wout & 3) || d.stride != 1 || d.pad != 0 || d.Hout != d.Hin ||
            d.Wout != d.Win || d.K != d.Cin || d.HoWo != d.Hout * d.Wout || d.N % d.HoWo != 0)
            return IVLN_E_UNSUPPORTED;
        const int ovu = d.tile_override;
        int kind1 = 2;  // (the form the launcher took: a pinned form or 24 / 32 / 48 chunks over many pixels is not the chunk count's)
        const int nwu = ovu == 18 ? 8 : (ovu == 19 ? 4 : 0);  // (18 | 19: the K-split form with 8 | 4 waves)
        const int rc = bf3_1x1_ks_launch(d, s, (force || ovu == 11 || ovu == 12 || ovu == 13 || nwu) ? 1 : 0, (ovu == 12 || nwu) ? 0 : (ovu == 13 ? 1 : -1), &kind1, nwu);
        return done(rc, flops, kind1, -1);
    }
    if (KS == 2) {
        // (the stacked classes multiply their common window's zero padding too: ivln_gemm_desc.real_taps)
        const double flops2 = flops * (d.real_taps > 0 ? d.real_taps / 16.0 : 1.0);
        if (d.stride != 1 || d.pad != 0 || d.Hout != d.Hin || d.Wout != d.Win || (d.M & 3) || d.grp_imgs > 0 || d.stat_partials || d.defer_epilogue ||
            d.splits > 1 || d.fuse_A_split || d.residual_after_relu || d.img_run_flags || d.K != d.Cin * 4 || d.HoWo != d.Hout * d.Wout ||
            d.N % d.HoWo != 0 || (d.Wout & 3) || d.Wout < 8 || (((uintptr_t)d.D | (uintptr_t)d.residual) & 15) || d.Ctot * 4 != d.M)
            return IVLN_E_UNSUPPORTED;
        const int nimg2 = d.N / d.HoWo;
        if ((int64_t)nimg2 * d.in_img_stride >= (int64_t)1 << 31) return IVLN_E_UNSUPPORTED;
        static const bool convt_off = getenv("IVLN_BF3_CONVT") && getenv("IVLN_BF3_CONVT")[0] == '0';  // A/B switch
        if (convt_off && !force) return IVLN_E_UNSUPPORTED;
        const int ov2 = d.tile_override;
        if (ov2 < 20) {  // few pixels: K split over the waves
            const int nw2 = ov2 == 16 ? 8 : (ov2 == 17 ? 4 : 0);  // (16 | 17: 8 | 4 waves)
            const bool ins2 = ov2 == 10 || ov2 == 15 || nw2;
            const int rc = bf3_ks_launch(d, s, nimg2, ins2 ? 1 : 0, 0, nw2);
            if (rc != IVLN_E_UNSUPPORTED || ins2) return done(rc, flops2, 1, -1);
        }
        const int CUS2 = ivln_cu_count();
        auto blocks2 = [&](int cfg) {
            const Bf3Px t = bf3_px(kBf3BN[cfg], d.Wout);
            return (int64_t)((d.Wout + t.ptw - 1) / t.ptw) * ((d.Hout + t.pth - 1) / t.pth) * ((nimg2 + t.imgs - 1) / t.imgs) *
                   ((d.M + kBf3BM[cfg] - 1) / kBf3BM[cfg]);
        };
        // the widest of the four tiles that gives every CU a workgroup (the classes cannot split K: no slabs in this store form)
        int cfg2 = blocks2(3) >= CUS2 ? 3 : (blocks2(2) >= CUS2 ? 2 : (blocks2(5) >= CUS2 ? 5 : 4));
        if (ov2 >= 20 && ov2 < 20 + kBf3Cfgs) cfg2 = ov2 - 20;
        if (!force && blocks2(cfg2) < CUS2 / 2) return IVLN_E_UNSUPPORTED;
        d.splits = 1;
        return done(launch_bf3_ks<2>(d, s, (const unsigned char*)d.A_split, d.a_split_grp_stride * 4, nimg2, cfg2, (d.Cin + CB - 1) / CB), flops2, 0, -1);
    }
    // deep-K 1x1 convs: K split over the waves of a workgroup, fragments built in registers (k_conv1x1_bf3_ks);
    // IVLN_BF3_1X1_KS=0 | 1 = never | wherever eligible, tile_override 11 insists
    static const int ks1_env = getenv("IVLN_BF3_1X1_KS") ? atoi(getenv("IVLN_BF3_1X1_KS")) : -1;
    // (tuning, tools/conv_cfg_sweep.py: tile_override 12 / 13 insist on the K-split / wave-tile form, 14 / 15 on 32- / 64-pixel tiles
    //  of the 3x3 K-split kernel, 16 / 17 on its 64-pixel tiles with 8 / 4 waves - the stacked 2 x 2 form too -, 18 / 19 on the 1x1
    //  K-split form with 8 / 4 waves, 20 + c on tile c of the tiled kernel; without a pin the wave count is bf3_ks_four_waves')
    const int ov = d.tile_override;
    const bool post = d.residual_after_relu != 0;  // (only the stride-1 1x1 kernels below know this epilogue form: they are insisted on)
    const int nw3 = ov == 16 ? 8 : (ov == 17 ? 4 : 0), nw1 = ov == 18 ? 8 : (ov == 19 ? 4 : 0);
    const bool ins1 = ov == 11 || ov == 12 || ov == 13 || nw1 || post, ins3 = ov == 10 || ov == 14 || ov == 15 || nw3;
    if (KS == 1 && ov < 20 && (ks1_env != 0 || ins1) && d.splits <= 1 && !d.defer_epilogue && d.HoWo == d.Hout * d.Wout &&
        d.K == d.Cin && d.N % d.HoWo == 0 && d.Hout == d.Hin && d.Wout == d.Win) {
        int kind1 = 2;
        const int rc = bf3_1x1_ks_launch(d, s, (ks1_env == 1 || ins1) ? 1 : 0, (ov == 12 || nw1) ? 0 : (ov == 13 ? 1 : -1), &kind1, nw1);
        if (rc != IVLN_E_UNSUPPORTED || ins1) return done(rc, flops, kind1, 0);
    }
    if (ins1 || (ins3 && KS != 3)) return IVLN_E_UNSUPPORTED;
    if (KS == 1) {  // 1x1, stride 1 or 2, no padding
        if ((d.stride != 1 && d.stride != 2) || d.pad != 0 || d.Hout != (d.Hin - 1) / d.stride + 1 || d.Wout != (d.Win - 1) / d.stride + 1 || d.M < 64)
            return IVLN_E_UNSUPPORTED;
    } else if (KS == 3 && d.stride == 2) {  // stride-2 3x3 (pad 1, even input): the tiled kernel's phase-plane staging
        static const bool s2_off = getenv("IVLN_BF3_S2") && getenv("IVLN_BF3_S2")[0] == '0';  // A/B switch
        // (Cin % CB: the stride-2 instantiations have no ragged-chunk test; launch_bf3_s2 checks it again)
        if ((s2_off && !force) || d.pad != 1 || d.Hin != 2 * d.Hout || d.Win != 2 * d.Wout || d.Cin % CB != 0 || d.fuse_A_split || d.stat_partials ||
            d.img_run_flags)
            return IVLN_E_UNSUPPORTED;
    } else if (d.stride != 1 || d.pad != KS / 2 || d.Hout != d.Hin || d.Wout != d.Win) {
        return IVLN_E_UNSUPPORTED;
    }
    const bool s2 = KS == 3 && d.stride == 2;
    if (d.K != d.Cin * KS * KS || d.HoWo != d.Hout * d.Wout || d.N % d.HoWo != 0) return IVLN_E_UNSUPPORTED;
    if (d.defer_epilogue || d.splits > 1 || (d.Wout & 3) || d.Wout < 8 || (((uintptr_t)d.D | (uintptr_t)d.residual | (uintptr_t)d.ws) & 15))
        return IVLN_E_UNSUPPORTED;
    const int nimg = d.N / d.HoWo;
    if ((int64_t)nimg * d.in_img_stride >= (int64_t)1 << 31) return IVLN_E_UNSUPPORTED;  // 32-bit patch offsets
    if (d.fuse_A_split) {  // the bottleneck tail: this 3x3 conv + the 1x1 expansion behind it in one launch (k_conv_bf3<..., FUSE>)
        static const bool fuse_off = getenv("IVLN_BF3_FUSE") && getenv("IVLN_BF3_FUSE")[0] == '0';  // A/B switch
        if (fuse_off || KS != 3 || (d.M != 64 && d.M != 128) || d.Cin % CB != 0 || d.Wout % 32 != 0 || d.Hout % 4 != 0 || d.fuse_M <= 0 ||
            d.fuse_M % 32 != 0 || d.stat_partials || d.accumulate || !d.relu || d.img_run_flags)
            return IVLN_E_UNSUPPORTED;
        if ((int64_t)nimg * d.Ctot * d.HoWo * 4 >= (int64_t)1 << 31 || (d.grp_imgs > 0 && nimg % d.grp_imgs != 0)) return IVLN_E_UNSUPPORTED;
        d.splits = 1;
        const unsigned char* a = (const unsigned char*)d.A_split;
        const int64_t gb = d.a_split_grp_stride * 4;
        // tiles: 64 or 128 channels x 128 pixels (4 x 32); 128 channels x 64 pixels (2 x 32, four waves of 32 channels) where the
        // 128-pixel grid would leave CUs without a workgroup (layer 2 at 8 + 8 images: 128 workgroups)
        const int64_t wg128 = (int64_t)nimg * (d.Wout / 32) * (d.Hout / 4);
        const bool px64 = d.M == 128 && d.Hout % 2 == 0 && wg128 < ivln_cu_count();
        const int rc = d.M == 64 ? launch_bf3_fused<1, 2, 2, 3>(d, s, a, gb, nimg)
                       : (px64 ? launch_bf3_fused<1, 4, 1, 3>(d, s, a, gb, nimg) : launch_bf3_fused<2, 2, 2, 3>(d, s, a, gb, nimg));
        return done(rc, flops + 2.0 * d.fuse_M * (double)d.N * d.M, 0, 0);
    }
    // pixel-starved deep 3x3 convs: K split over the waves of a workgroup, no slabs (k_conv_bf3_ks); IVLN_BF3_KS=0 | 1 = never | wherever eligible
    static const int ks_env = getenv("IVLN_BF3_KS") ? atoi(getenv("IVLN_BF3_KS")) : -1;
    if (KS == 3 && !s2 && ov < 20 && (ks_env != 0 || ins3) && d.splits <= 1) {
        const int rc = bf3_ks_launch(d, s, nimg, (ks_env == 1 || ins3) ? 1 : 0, ov == 14 ? 1 : ((ov == 15 || nw3) ? 2 : 0), nw3);
        if (rc != IVLN_E_UNSUPPORTED || ins3) return done(rc, flops, 1, 0);
    }
    const int nch = ((d.Cin + CB - 1) / CB + bf3_stage_chunks(KS) - 1) / bf3_stage_chunks(KS);  // stages: what blockIdx.z can split
    auto tiles_of = [&](int cfg) {
        const Bf3Px t = bf3_px(kBf3BN[cfg], d.Wout);
        return (int64_t)((d.Wout + t.ptw - 1) / t.ptw) * ((d.Hout + t.pth - 1) / t.pth) * ((nimg + t.imgs - 1) / t.imgs);
    };
    auto blocks_of = [&](int cfg) { return tiles_of(cfg) * ((d.M + kBf3BM[cfg] - 1) / kBf3BM[cfg]); };
    // fills the chip: at most a quarter of the last round of 256 x slots workgroups empty
    const int CUS = ivln_cu_count();  // (256 on MI355X; a partition mode or another part gets its own count)
    auto fills = [&](int64_t nb, int slots) {
        const int64_t round = (int64_t)CUS * slots, rounds = (nb + round - 1) / round;
        return nb * 4 >= rounds * round * 3;
    };
    // the widest tile that fills the chip on its own; else the 4-wave tiles (two or three workgroups per CU) with the channel
    // chunks split over blockIdx.z (raw slabs reduced by k_splitk_epilogue, like the fp32 kernels)
    int cfg = -1, splits = 1;
    const bool big_ok = !(KS == 7 && d.Wout <= 8) && !s2;  // (7x7 on 8x8 maps: eight images of 14 x 14 patch pixels do not fit; stride 2: 128- / 256-pixel tiles only)
    // (4-wave tiles, measured on RedNet's 3x3 shapes at 8 + 8 stacked images against the fp32 kernels: 128 x 128 wins from
    //  2 M outputs - 57 vs 64 us on 128 x 16384, 50 vs 67 on 256 x 4096 and 512 x 1024 -, 64 x 128 below - 41 vs 46 on
    //  128 x 8192, 37.5 vs 44 on 256 x 2048 and 512 x 512; 64-channel convs that need them lose - 42 vs 38 us on 64 x 32768)
    //  (the 64 x 128 tile that gives every CU a workgroup stays unsplit)
    if (d.M <= 32) cfg = 6;
    else if (d.M <= 64)
        cfg = (big_ok && KS != 1 && fills(blocks_of(1), 1)) ? 1
              : (fills(blocks_of(2), 1) ? 2 : ((force || blocks_of(4) >= CUS) ? 4 : -1));
    // (64 x 32768, the decoder's 64-channel convs at 64 x 64: the 64 x 128 tile UNSPLIT - one workgroup per CU - 24.9 us against the
    //  fp32 kernel's 37.2 and 35.8 with its channel chunks split three ways + the reduction launch: tools/conv_cfg_sweep.py)
    // (round 5, aligned-group staging: the 64 x 128 tile now beats 128 x 128 wherever the latter leaves CUs without a workgroup -
    //  128 x 16384: 42.7 vs 50.9 us, 256 x 4096: 43.2 vs 45.3)
    else cfg = fills(blocks_of(3), 1) ? 3 : (fills(blocks_of(2), 1) ? 2 : (((int64_t)d.M * d.N >= (1 << 21) && blocks_of(5) >= CUS) ? 5 : 4));
    if (cfg < 0) return IVLN_E_UNSUPPORTED;
    if (d.tile_override >= 20 && d.tile_override < 20 + kBf3Cfgs) cfg = d.tile_override - 20;  // (tuning: tools/conv_cfg_sweep.py pins a tile)
    if ((cfg == 0 && !big_ok) || (KS == 1 && (cfg <= 1 || cfg == 6))) return IVLN_E_UNSUPPORTED;
    const int64_t nb = blocks_of(cfg);
    // a pixel tile is rows x columns of ONE image (or whole small images): a Conv1d-shaped input (H = 1: the policy's k / v
    // projections, 384 x 8192 x 192 in an update) would fill 1 row of 16 - 427 us for 1.2 GFLOP, found in round 5 after the
    // 1x1 eligibility had been widened.  Tilings that use less than 15 % of their pixels go back to the fp32 GEMMs (at 21 % -
    // 256 x 40960 x 256 as rows of 80 - this kernel still wins: 66.7 against 80.3 us).
    if (!force && (double)d.N < 0.15 * (double)tiles_of(cfg) * kBf3BN[cfg]) return IVLN_E_UNSUPPORTED;
    if (cfg >= 4) {
        const int slots = cfg == 4 ? 3 : 2;
        const bool may_split = d.splits == 0 && d.ws && nch >= 2 && !d.stat_partials;
        if (may_split && nb < (int64_t)CUS * slots && !(cfg == 4 && nb >= CUS)) {  // (128 x 16384: 45.0 unsplit, 53.0 split two ways)
            const int64_t want = (int64_t)CUS * slots;
            splits = (int)((want + nb - 1) / nb);
            if (splits > nch) splits = nch;
            if (splits > 16) splits = 16;
            const int64_t cap = d.ws_floats / ((int64_t)d.M * d.N);
            if (splits > cap) splits = (int)cap;
            if (splits < 1) splits = 1;
        }
        if (!force && nb * splits < CUS * 3 / 4) return IVLN_E_UNSUPPORTED;  // pixel- and channel-starved: the implicit GEMM splits K deeper
    } else if (!force && !fills(nb, cfg == 6 ? 2 : 1)) {
        return IVLN_E_UNSUPPORTED;
    }
    const int cps = (nch + splits - 1) / splits;
    splits = (nch + cps - 1) / cps;
    const Bf3Px t = bf3_px(kBf3BN[cfg], d.Wout);
    if (d.grp_imgs > 0 && (d.grp_imgs % t.imgs != 0 || nimg % d.grp_imgs != 0)) return IVLN_E_UNSUPPORTED;  // a tile's images share one weight set
    d.splits = splits;
    if (splits > 1) d.stat_partials = nullptr;
    const int64_t tiles = tiles_of(cfg);
    const int BN = kBf3BN[cfg];
    const int64_t gb = d.a_split_grp_stride * 4;
    const int rc = KS == 7   ? launch_bf3_ks<7>(d, s, (const unsigned char*)d.A_split, gb, nimg, cfg, cps)
                   : s2      ? launch_bf3_s2(d, s, (const unsigned char*)d.A_split, gb, nimg, cfg, cps)
                   : KS == 3 ? launch_bf3_ks<3>(d, s, (const unsigned char*)d.A_split, gb, nimg, cfg, cps)
                             : launch_bf3_ks<1>(d, s, (const unsigned char*)d.A_split, gb, nimg, cfg, cps);
    return done(rc, flops, 0, d.stat_partials ? (int)(tiles * (BN / 128)) : 0);
}

// The 7x7 weight gradient on the split-bf16 arithmetic (k_wgrad_bf3).  IVLN_E_UNSUPPORTED -> the fp32 MFMA weight-gradient kernel.
int ivln_wgrad_bf3_launch(ivln_gemm_desc& d, hipStream_t s, bool force) {
    if (!d.split_ok && !force) return IVLN_E_UNSUPPORTED;
    if (d.amode != AMODE_NCHW_P || d.bmode != BMODE_IM2COL_T || d.dmode != DMODE_DENSE || d.stride != 1 || d.dil != 1 || d.Cin <= 0 ||
        d.N != d.Cin * 49 || d.defer_epilogue || d.pad != 3)
        return IVLN_E_UNSUPPORTED;
    if (d.HoWo != d.Hout * d.Wout || d.K % d.HoWo != 0 || d.Hout != d.Hin || d.Wout != d.Win) return IVLN_E_UNSUPPORTED;
    if (d.Wout != 64 && d.Wout != 32 && d.Wout != 16 && d.Wout != 8) return IVLN_E_UNSUPPORTED;
    const int ims = d.Wout == 8 ? 2 : 1, rows = 128 / (d.Wout * ims);
    if (d.Hout % rows != 0 || (d.Wout == 8 && d.Hout != 8) || (((uintptr_t)d.A) & 7)) return IVLN_E_UNSUPPORTED;
    const int nimg = d.K / d.HoWo;
    if ((int64_t)nimg * d.in_img_stride >= (int64_t)1 << 31 || (int64_t)nimg * d.M * d.HoWo >= (int64_t)1 << 31) return IVLN_E_UNSUPPORTED;
    const int strips = ((nimg + ims - 1) / ims) * (d.Hout / rows);
    // tile: 32 x 512, 64 x 512 or 128 x 256 (channels x columns); strips over blockIdx.z until a workgroup per CU
    // (32-channel outputs: 14 x 49 = 686 columns are two tiles of 384 - six waves - with 11 % of the columns idle; two tiles of
    //  512 left 33 % idle)
    const bool six = d.M <= 32 && (d.N + 383) / 384 * 384 < (d.N + 511) / 512 * 512;
    // x promised exact in bf16 (split_ok = 2): the one-piece form, as 32 x 256 tiles of four waves - 43 KB of LDS, 3 workgroups per CU
    // (9.09 against 9.02 ms per update with 32 x 384 tiles of six waves, two per CU; 9.44 with the three-piece form)
    const bool xe = d.split_ok == 2 && d.M <= 32 && d.Wout == 64;
    const int BM = d.M <= 32 ? 32 : (d.M <= 64 ? 64 : 128), BN = xe ? 256 : (d.M <= 32 ? (six ? 384 : 512) : (d.M <= 64 ? 512 : 256));
    const int64_t blocks = (int64_t)((d.N + BN - 1) / BN) * ((d.M + BM - 1) / BM);
    if (!d.ws || d.ws_floats < (int64_t)d.M * d.N) return IVLN_E_UNSUPPORTED;  // (the kernel always leaves raw slabs)
    int splits = 1;
    if (d.splits == 0) {
        if (d.ws) {
            // one workgroup per CU (LDS): as many splits as keep the grid inside whole rounds of 256 (13 column tiles x 20
            // splits = 260 workgroups ran a second round for four of them)
            const int64_t want = (xe ? 3 : 1) * (int64_t)ivln_cu_count();
            splits = (int)(want / blocks);
            if (splits < 1) splits = 1;
            if (splits > strips) splits = strips;
            const int64_t cap = d.ws_floats / ((int64_t)d.M * d.N);
            if (splits > cap) splits = (int)cap;
            if (splits < 1) splits = 1;
        }
    } else {
        splits = d.splits > strips ? strips : d.splits;
        if (splits > 1 && (!d.ws || d.ws_floats < (int64_t)splits * d.M * d.N)) return IVLN_E_INVALID;
    }
    if (!force && blocks * splits < ivln_cu_count() / 2) return IVLN_E_UNSUPPORTED;  // (a rollout-sized batch: nothing to win)
    const int sps = (strips + splits - 1) / splits;
    splits = (strips + sps - 1) / sps;
    d.splits = splits;
    int rc;
    if (xe) rc = launch_wgrad_bf3<1, 1, 4, 64, true>(d, s, nimg, strips, sps);
    else if (d.M <= 32 && six) rc = launch_wgrad_bf3_w<1, 1, 6>(d, s, nimg, strips, sps);
    else if (d.M <= 32) rc = launch_wgrad_bf3_w<1, 1, 8>(d, s, nimg, strips, sps);
    else if (d.M <= 64) rc = launch_wgrad_bf3_w<2, 1, 8>(d, s, nimg, strips, sps);
    else rc = launch_wgrad_bf3_w<2, 2, 4>(d, s, nimg, strips, sps);
    if (rc == IVLN_OK) g_bf3_flops += 2.0 * d.M * (double)d.N * d.K, ++g_bf3_launches;
    return rc;
}
