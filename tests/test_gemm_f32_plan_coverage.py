"""CPU: the fp32 part of ivln_gemm_f32's dispatch - what every conv runs on when it has no A_split - restated in plain Python,
and the case tables of tests/test_gpu_gemm_f32_kernels.py (which imports them, and `plan`, from here and holds the real
launchers to the plans: kernel name, splits_used, *stat_tiles, accepted versus refused with the return code).

Restated (files of ivln-ce_amd/csrc):
  ivln_gemm_f32 below the A_split branches   gemm_conv.hip 534-558, 609-718   the img_run_flags normalisation, the route order
                                             direct -> stream -> vec / scalar, the tile heuristic, the grp_imgs tile fix-up,
                                             the split heuristic (min_tiles, want, below, max_splits, the workspace cap), the
                                             drop of empty trailing splits
  launch_splitk_epilogue                     gemm_conv.hip 387-408   flat4 | k_splitk_epilogue4 | k_splitk_epilogue
  launch_tile                                gemm_conv.hip 410-433   the block tiles and the operand pairs k_gemm is built for
  epilogue_tile's vec4 predicate             gemm_common.h 99-104    dense destinations only: every conv case here is scalar
  ivln_gemm_vec_eligible / _launch           gemm_vec.hip 308-351    tiles 3 and 4 are unreachable for k_gemm_vec through the
                                             dispatcher (gemm_conv.hip 652 sends them to 0); stride-2 conv1x1 (BS2) keeps the
                                             one-accumulator tiles (gemm_vec.hip 289-294, 341)
  WIDE_FITS of k_gemm_vec                    gemm_vec.hip 31-38      from BKV, LDK = BKV + 4, LDC = BN + 4: holds with no word
                                             to spare for the 64 x 64 conv1x1 tile, fails for LAY_R x LAY_R
  ivln_conv_direct_launch, launch_ks / _wm   conv_direct.hip 260-285, 491-550   refusals, the pixel-tile ladder, WM by M, chunk
                                             splits, the wide predicate, stat_tiles
  ivln_conv1x1_stream_launch, launch_k       conv1x1_stream.hip 127-164
  ivln_conv_packed_floats, the packed index  conv_direct.hip 608-614, conv1x1_stream.hip 38-49
Nothing in this part of the dispatch reads the CU count: `cus` is accepted by plan() for symmetry with the split-bf16 file and
ignored, so every plan here holds on every device.  Environment switches and the constexpr A/B switches are taken as they
stand in the sources (off).

Read from the sources by regex and compared with what this file states (test_constants_are_the_sources): BK, BKV,
conv_direct_ci, the PTW / PTH / IMGS ladder (launcher and launch_ks), min_n and the 192-block floor of the stream kernel, the
block tiles of launch_tile / launch_vec, kFamilyKernels.

The defect this file records.  k_conv1x1_stream<64, MT = 2> read its PACKED weights at tile (m_base >> 5) + mt, and
ivln_conv_packed_floats(M, 64, 1) holds ceil(M / 32) tiles: whenever that count is odd the last wave's second row tile read
32 * 64 floats past the pack (rows masked at the store: values right, nothing noticed).  packed_index_parent keeps that rule
with the M it overruns; packed_index is the kernel's rule now (the tile index clamped to the last tile, as the unpacked path
clamps its row).  A second one, in the dispatcher: tile_override 8 with splits > 1 skipped the stream launcher and ran k_gemm -
an insisting override that did not insist; it is refused now (IVLN_E_UNSUPPORTED, the launcher's own answer to splits > 1).

Instantiation keys (plan.keys):
  ("k_gemm", tile 0 ... 4, "A_MK", bmode)                 30; the five dense / weight-gradient pairs are DENSE_PAIRS below
  ("k_gemm_vec", tile 0 | 1 | 2, "LAY_K", "LAY_R", BS2)   what the dispatcher produces for A_MK x B_CONV1X1
  ("k_conv_direct", KS, S, PTW, WM, PACKED)               80
  ("k_conv1x1_stream", K, WAVES_M, PACKED)                18
  ("k_splitk_epilogue", "nchw" | "up2" | "up2x4"), ("k_splitk_epilogue4", "nchw", grouped)
test_cases_cover_every_instantiation_the_plans_can_produce enumerates the accepted domain over a grid of descriptors wider than
the cases and requires the union of the cases' keys to equal what the grid reaches."""
import itertools
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ivln-ce_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def cdiv(a, b):
    return -(-a // b)


_GEMM, _VEC, _DIRECT, _STREAM, _COMMON = (_src(n) for n in ("gemm_conv.hip", "gemm_vec.hip", "conv_direct.hip",
                                                              "conv1x1_stream.hip", "gemm_common.h"))

# ---- what this file states (test_constants_are_the_sources holds it to the sources) ----
BK, BKV = 16, 32                         # K tile of k_gemm / k_gemm_vec
CI = {7: 2, 2: 16, 3: 8}                 # conv_direct_ci: input channels per chunk of the direct kernel
LADDER = ((16, 32, 4, 1), (8, 16, 8, 1), (4, 8, 8, 2), (0, 4, 4, 8))   # Wout > w: (PTW, PTH, IMGS)
STREAM_MIN_N, STREAM_FLOOR = 4096, 192
TILES = ((64, 64, 1, 1), (32, 128, 1, 1), (128, 32, 1, 1), (128, 128, 2, 2), (64, 128, 1, 2))   # tile -> BM, BN, TM, TN
FAMILY = ("k_gemm", "k_gemm_vec", "k_conv_direct", "k_conv1x1_stream")
BMODES = {"conv": 0, "1x1": 1, "convt": 5, "k3": 6, "k7": 7, "k2": 8}
KS_OF = {"k3": 3, "k7": 7, "k2": 2}
DMODES = {"nchw": 0, "up2": 2, "up2x4": 3}
FORMS = ("plain", "full")   # every instantiation: no epilogue operand | scale + shift + residual + ReLU into a channel slice
C0, WIDER = 4, 8            # the slice's first channel and the extra channels of the `full` form's destination


def ladder(Wout):
    for w, ptw, pth, imgs in LADDER:
        if Wout > w:
            return ptw, pth, imgs


# ------------------------------------------------------------------------------------------------------------------
# a case -> the descriptor's integers
# ------------------------------------------------------------------------------------------------------------------
def desc(c, form="plain"):
    """The ivln_gemm_desc of a case as integers and presence flags.  Case keys: bmode (conv | 1x1 | convt | k3 | k7 | k2), KH, KW
    (conv / convt), stride, pad, dil, opad (convt), imgs, Cin, Hin, Win, M, ov (tile_override), dmode (nchw | up2 | up2x4), cls
    (up2: the parity class (a, b)), splits (forced; 0 = heuristic), ws_slabs (workspace size in slabs), defer, grp, acc, nwe,
    noxcd, packed, stats, flags (img_run_flags), misA / misB / misD (four bytes off a 16-byte boundary), lda_pad, img_pad
    (floats added to the image stride), no_ws.  form: plain | full | shift (shift without scale)."""
    d = types.SimpleNamespace()
    bm = c["bmode"]
    KS = KS_OF.get(bm, 1 if bm == "1x1" else 0)
    d.bmode, d.KS = bm, KS_OF.get(bm, 0)
    d.KH, d.KW = (KS, KS) if KS else (c["KH"], c["KW"])
    d.stride, d.pad, d.dil, d.opad = c.get("stride", 1), c.get("pad", 0), c.get("dil", 1), c.get("opad", 0)
    d.nimg, d.Cin, d.Hin, d.Win, d.M = c["imgs"], c["Cin"], c["Hin"], c["Win"], c["M"]
    if bm == "convt":
        d.Hout, d.Wout = ((n - 1) * d.stride - 2 * d.pad + k + d.opad for n, k in ((d.Hin, d.KH), (d.Win, d.KW)))
    elif bm == "k2":   # the stacked parity classes: same-size output, the row / column past the edge reads as zero
        d.Hout, d.Wout = d.Hin, d.Win
    else:
        d.Hout, d.Wout = ((n + 2 * d.pad - d.dil * (k - 1) - 1) // d.stride + 1 for n, k in ((d.Hin, d.KH), (d.Win, d.KW)))
    d.HoWo = d.Hout * d.Wout
    d.N, d.K = d.nimg * d.HoWo, d.Cin * d.KH * d.KW
    d.dmode, d.cls = c.get("dmode", "nchw"), c.get("cls", (0, 0))
    d.ov, d.splits, d.defer = c.get("ov", 0), c.get("splits", 1), bool(c.get("defer"))
    d.grp, d.acc, d.nwe, d.noxcd = c.get("grp", 0), bool(c.get("acc")), bool(c.get("nwe")), bool(c.get("noxcd"))
    d.packed, d.stats, d.flags = bool(c.get("packed")), bool(c.get("stats")), c.get("flags")
    d.A_al, d.B_al, d.D_al, d.res_al = not c.get("misA"), not c.get("misB"), not c.get("misD"), True
    full = form == "full"
    d.has_scale, d.has_shift, d.has_res, d.relu = full, full or form == "shift", full, full
    d.C = d.M // 4 if d.dmode == "up2x4" else d.M                  # channels of the destination the launch writes
    d.Ctot = d.C + (WIDER if full else 0)
    d.lda = d.K + c.get("lda_pad", 0)
    d.in_img_stride = d.Cin * d.Hin * d.Win + c.get("img_pad", 8 if full else 0)
    d.ws = (d.splits != 1 or d.defer) and not c.get("no_ws")
    d.ws_floats = (c.get("ws_slabs") or max(d.splits, 1)) * d.M * d.N if d.ws else 0
    return d


def _no(code, why):
    return types.SimpleNamespace(ok=False, code=code, why=why, keys=set())


def _yes(d, kernel, key, grid, splits, k_step, reduce=None, stat_tiles=0, wide=False, tile=None, runs=None):
    p = types.SimpleNamespace(ok=True, code=None, why=None, kernel=kernel, key=key, grid=grid, nwg=grid[0] * grid[1] * grid[2],
                              splits=splits, k_step=k_step, reduce=reduce, stat_tiles=stat_tiles, wide=wide, tile=tile, runs=runs)
    p.keys = {key} | ({reduce} if reduce else set())
    p.slabs = splits if (splits > 1 or d.defer) else 0   # slabs the launch leaves in the workspace
    return p


# ------------------------------------------------------------------------------------------------------------------
# the launchers, restated
# ------------------------------------------------------------------------------------------------------------------
def splitk_epilogue(d, splits):
    """launch_splitk_epilogue for the NCHW-family destinations (dense ones: tests/test_gpu_train_gemms.py)"""
    if splits <= 1 or d.defer:
        return None
    lay = d.dmode == "nchw" and d.HoWo % 4 == 0
    vec4 = lay and d.N % 4 == 0 and not d.nwe and d.D_al and d.res_al
    return ("k_splitk_epilogue4", "nchw", d.grp > 0) if vec4 else ("k_splitk_epilogue", d.dmode)


def epilogue_tile_vec4(dense, sDm, sDn, M, aligned, to_ws):
    """epilogue_tile's 16-byte form: dense destinations with unit ROW stride only"""
    return (not to_ws) and dense and sDm == 1 and sDn % 4 == 0 and M % 4 == 0 and aligned


def vec_eligible(d):
    """ivln_gemm_vec_eligible for A_MK x the conv modes -> (eligible, the clause that refused)"""
    if not d.A_al:
        return False, "A"
    if not d.B_al:
        return False, "B"
    if d.K & 3:
        return False, "K%4"
    if d.lda & 3:
        return False, "lda%4"
    if d.bmode == "1x1" and d.stride == 2:
        if d.pad != 0:
            return False, "s2 pad"
        if d.Win != 2 * d.Wout or d.Hin < 2 * d.Hout - 1 or d.Wout & 1 or d.Win & 3 or (d.Hin * d.Win) & 3:
            return False, "s2 geometry"
        if d.in_img_stride & 3:
            return False, "s2 image stride"
    elif d.bmode == "1x1":
        if d.stride != 1:
            return False, "stride"
        if d.pad != 0 or d.Hin * d.Win != d.HoWo:
            return False, "pad"
        if d.HoWo & 3:
            return False, "HoWo%4"
        if d.in_img_stride & 3:
            return False, "image stride"
    else:
        return False, "bmode"
    return True, None


def vec_wide_fits(BM, BN, alay_k=True, blay_k=False):
    """WIDE_FITS of k_gemm_vec: the output tile [BM][BN + 4] must fit the operand tiles' LDS block"""
    LDK, LDC = BKV + 4, BN + 4
    a_words = BM * LDK if alay_k else BKV * BM
    b_words = BN * LDK if blay_k else BKV * BN
    return BM * LDC <= a_words + b_words, a_words + b_words - BM * LDC


def conv_direct_launch(d, ov, splits_req):
    KS = d.KS
    if KS == 0 or d.dil != 1:
        return _no("unsupported", "not a 2x2 / 3x3 / 7x7 mode, or dilated")
    if d.stride != 1 and not (d.stride == 2 and KS != 2):
        return _no("unsupported", "stride")
    ci = CI[KS]
    if d.Cin % ci != 0 and not (KS == 7 and d.stride == 2):
        return _no("unsupported", "Cin % CI off the stems")
    ptw, pth, imgs = ladder(d.Wout)
    if d.grp > 0 and (d.grp % imgs != 0 or d.nimg % d.grp != 0):
        return _no("unsupported", "grp_imgs % IMGS")
    tiles = cdiv(d.Wout, ptw) * cdiv(d.Hout, pth) * cdiv(d.nimg, imgs)
    BM = 32 if d.M <= 32 else 64
    blocks, nch = tiles * cdiv(d.M, BM), cdiv(d.Cin, ci)
    if ov == 0 and (blocks < 16 if KS == 7 else blocks * min(nch, 16) < 128):
        return _no("unsupported", "pixel-starved: the implicit GEMM splits deeper")
    if d.defer and (not d.ws or d.ws_floats < d.M * d.N):
        return _no("invalid", "deferred without a slab")
    splits = 1
    if splits_req == 0:
        want = 256 if d.defer else 512
        if d.ws and blocks < 256 and nch >= 2:
            splits = max(1, min(cdiv(want, blocks), nch, 16, d.ws_floats // (d.M * d.N)))
    else:
        splits = min(splits_req, nch)
        if splits > 1 and (not d.ws or d.ws_floats < splits * d.M * d.N):
            return _no("invalid", "workspace")
    cps = cdiv(nch, splits)
    splits = cdiv(nch, cps)
    wide = d.dmode == "nchw" and splits == 1 and not d.defer and d.Wout % 4 == 0 and d.D_al and d.res_al and not d.nwe
    wide_up = KS == 2 and d.dmode == "up2x4" and splits == 1 and not d.defer and d.Wout % 2 == 0 and d.D_al and d.res_al and not d.nwe
    key = ("k_conv_direct", KS, d.stride, ptw, 1 if d.M <= 32 else 2, d.packed)
    return _yes(d, "k_conv_direct", key, (tiles, cdiv(d.M, BM), splits), splits, cps * ci * KS * KS, splitk_epilogue(d, splits),
                stat_tiles=tiles if (d.stats and wide) else 0, wide=wide or wide_up)


def stream_waves(M, K):
    rows = 64 if K == 64 else 32
    return rows, (1 if M <= rows else (2 if M <= 2 * rows else 4))


def conv1x1_stream_launch(d, force, splits_req):
    if d.bmode != "1x1" or d.dmode != "nchw":
        return _no("unsupported", "not a 1x1 conv into NCHW")
    if d.K not in (128, 256) and not (d.K == 64 and force):
        return _no("unsupported", "K")
    if d.stride != 1 or d.pad != 0 or d.Hin * d.Win != d.HoWo or d.defer or splits_req > 1 or d.stats:
        return _no("unsupported", "stride / pad / deferred / splits / statistics")
    if d.HoWo & 127 or (d.N < STREAM_MIN_N and not force) or d.lda & 3 or d.in_img_stride & 3:
        return _no("unsupported", "HoWo % 128, N, lda, image stride")
    if not (d.A_al and d.B_al and d.D_al and d.res_al) or (d.grp > 0 and (d.M * d.lda) & 3):
        return _no("unsupported", "alignment")
    rows, wavesm = stream_waves(d.M, d.K)
    grid = (cdiv(d.N // 128, 4 // wavesm), cdiv(d.M, rows * wavesm), 1)
    if grid[0] * grid[1] < STREAM_FLOOR and not force:
        return _no("unsupported", "too few blocks")
    return _yes(d, "k_conv1x1_stream", ("k_conv1x1_stream", d.K, wavesm, d.packed), grid, 1, d.K, wide=True)


def tiles_run(d, BN):
    """per column tile of the output: does any image it touches carry a non-zero flag (ivln_tile_skipped)"""
    runs = []
    for n0 in range(0, d.N, BN):
        last = min(d.N, n0 + BN) - 1
        runs.append(any(d.flags[i] for i in range(n0 // d.HoWo, last // d.HoWo + 1)))
    return runs


def plan_desc(d):
    ov, splits_req = d.ov, d.splits
    if d.dmode == "up2x4" and d.M & 3:
        return _no("invalid", "UP2X4 with M % 4")
    if d.grp > 0 and (d.dmode != "nchw" or d.N % (d.grp * d.HoWo) != 0):
        return _no("invalid", "grp_imgs")
    if d.flags is not None:
        if d.dmode != "nchw" or d.defer or ov in (6, 8, 9):
            return _no("invalid", "img_run_flags with a kernel that does not honour them")
        splits_req = 1
        if ov == 0:
            ov = 7 if vec_eligible(d)[0] else 1
    if ov >= 9:
        return _no("unsupported", "the split-bf16 kernels need A_split")
    if ov in (0, 6):
        p = conv_direct_launch(d, ov, splits_req)
        if p.ok or p.code != "unsupported" or ov == 6:
            return p
    if ov == 8 or (ov == 0 and splits_req <= 1):
        p = conv1x1_stream_launch(d, ov == 8, splits_req)
        if p.ok or p.code != "unsupported" or ov == 8:
            return p
    nblocks = lambda bm, bn: cdiv(d.M, bm) * cdiv(d.N, bn)   # noqa: E731
    tile = 1 if d.M <= 32 else (2 if d.N <= 32 else (4 if nblocks(64, 128) >= 512 else 0))
    if 1 <= ov <= 5:
        tile = ov - 1
    elig, clause = vec_eligible(d)
    vec = ov in (0, 7) and elig
    if ov == 7 and not vec:
        return _no("unsupported", "vec: " + clause)
    bk = BKV if vec else BK
    if vec and tile not in (1, 2):
        tile = 0
    if d.grp > 0:
        gp = d.grp * d.HoWo
        if gp % TILES[tile][1] != 0:
            if gp % 64 == 0:
                tile = 0
            elif gp % 32 == 0:
                tile = 2
            else:
                return _no("unsupported", "an output tile would straddle two weight groups")
    BM, BN = TILES[tile][:2]
    blocks, nk = cdiv(d.M, BM) * cdiv(d.N, BN), cdiv(d.K, bk)
    if d.defer and (not d.ws or d.ws_floats < d.M * d.N):
        return _no("invalid", "deferred without a slab")
    splits = 1
    if splits_req == 0:
        min_tiles, want = (2, 256) if d.defer else (4, 512)
        if d.ws and blocks < 256 and nk >= 2 * min_tiles:
            splits = min(cdiv(want, blocks), nk // min_tiles)
            max_splits = (64 if blocks <= 8 else (32 if blocks <= 32 else 16)) if d.defer else (256 if nk >= 4096 else (64 if nk >= 512 else 16))
            splits = max(1, min(splits, max_splits, d.ws_floats // (d.M * d.N)))
    else:
        splits = splits_req
        if splits > 1 and (not d.ws or d.ws_floats < splits * d.M * d.N):
            return _no("invalid", "workspace")
    tps = cdiv(nk, splits)
    splits = cdiv(nk, tps)   # empty trailing splits dropped
    grid = (cdiv(d.N, BN), cdiv(d.M, BM), splits)
    runs = tiles_run(d, BN) if d.flags is not None else None
    if vec:
        bs2 = d.stride == 2
        fits = vec_wide_fits(BM, BN)[0]
        wide = fits and splits == 1 and not d.defer and d.D_al and d.res_al and not d.nwe and (
            (d.dmode == "nchw" and d.HoWo % 4 == 0) or (d.dmode == "up2x4" and d.Wout % 2 == 0))
        key = ("k_gemm_vec", tile, "LAY_K", "LAY_R", bs2)
        p = _yes(d, "k_gemm_vec", key, grid, splits, tps * bk, splitk_epilogue(d, splits), wide=wide, tile=tile, runs=runs)
    else:
        p = _yes(d, "k_gemm", ("k_gemm", tile, "A_MK", d.bmode), grid, splits, tps * bk, splitk_epilogue(d, splits), tile=tile, runs=runs)
    p.nk, p.tps, p.last_tiles = nk, tps, nk - (splits - 1) * tps
    return p


def plan(c, cus=256, form="plain"):
    """(`cus` is not read: see the docstring)"""
    return plan_desc(desc(c, form))


# ------------------------------------------------------------------------------------------------------------------
# the packed weights of k_conv1x1_stream
# ------------------------------------------------------------------------------------------------------------------
def conv_packed_floats(M, Cin, KS):
    """ivln_conv_packed_floats"""
    if KS == 1:
        return cdiv(M, 32) * 32 * Cin if (M > 0 and Cin in (64, 128, 256)) else 0
    if KS not in (2, 3, 7) or M <= 0 or (Cin % CI[KS] and KS != 7):
        return 0
    BM = 32 if M <= 32 else 64
    return cdiv(M, BM) * cdiv(Cin, CI[KS]) * (CI[KS] * KS * KS) * (BM + 4)


def _stream_waves_of(M, K):
    """(m_base, MT) of every wave that passes the kernel's `m_base < M` test"""
    MT = 2 if K == 64 else 1
    rows, wavesm = stream_waves(M, K)
    for by in range(cdiv(M, rows * wavesm)):
        for wm in range(wavesm):
            m_base = (by * wavesm + wm) * 32 * MT
            if m_base < M:
                yield m_base, MT


def packed_index_parent(M, K):
    """the largest index of A_packed the kernel read before the fix: (m_base >> 5) * NQ * 64 + (mt * NQ + q) * 64 + lane"""
    NQ = K // 2
    return max((m_base >> 5) * NQ * 64 + (mt * NQ + q) * 64 + lane
               for m_base, MT in _stream_waves_of(M, K) for mt in range(MT) for q in (0, NQ - 1) for lane in (0, 63))


def packed_index(M, K):
    """... and now: the row tile clamped to the pack's last one"""
    NQ, last = K // 2, cdiv(M, 32) - 1
    return max((min((m_base >> 5) + mt, last) * NQ + q) * 64 + lane
               for m_base, MT in _stream_waves_of(M, K) for mt in range(MT) for q in (0, NQ - 1) for lane in (0, 63))


PARENT_OVERRUNS = [M for M in range(1, 201) if cdiv(M, 32) % 2 == 1]   # K = 64: an odd number of 32-row tiles


def test_packed_index_stays_inside_the_pack_and_the_parents_did_not():
    for K in (64, 128, 256):
        for M in range(1, 201):
            size = conv_packed_floats(M, K, 1)
            assert packed_index(M, K) < size, (M, K)
            over = packed_index_parent(M, K) >= size
            assert over == (K == 64 and M in PARENT_OVERRUNS), (M, K)
            if over:   # exactly one tile of 32 rows x 64 channels past the end
                assert packed_index_parent(M, K) == size + 32 * 64 - 1
    with pytest.raises(AssertionError):
        for M in range(1, 201):
            assert packed_index_parent(M, 64) < conv_packed_floats(M, 64, 1)
    # the kernel source carries the clamp
    assert re.search(r"min\(\(m_base >> 5\) \+ mt, last_tile\)", _STREAM) and "(p.M + 31) / 32 - 1" in _STREAM


# ------------------------------------------------------------------------------------------------------------------
# the case tables
# ------------------------------------------------------------------------------------------------------------------
def _c(tag, bmode, ov, imgs, Cin, Hin, Win, M, edges=(), **kw):
    return dict(tag=tag, bmode=bmode, ov=ov, imgs=imgs, Cin=Cin, Hin=Hin, Win=Win, M=M, edges=tuple(edges), **kw)


# N = imgs x (H x W) one short of, equal to and one past 32 / 64 / 128 (1x1 convs: any N is reachable)
N_SHAPE = {31: (1, 1, 31), 32: (2, 4, 4), 33: (3, 1, 11), 63: (3, 3, 7), 64: (2, 4, 8), 65: (5, 1, 13), 127: (1, 1, 127),
           128: (2, 8, 8), 129: (3, 1, 43)}


def _ragged_cases():
    """k_gemm, every block tile: M and N one short of, equal to and one past the tile (B_CONV1X1, K = 20: a ragged second K tile)"""
    out = []
    for t, (BM, BN, _, _) in enumerate(TILES):
        for dm, dn in ((-1, 1), (0, 0), (1, -1)):
            imgs, H, W = N_SHAPE[BN + dn]
            out.append(_c("g-t%d-m%d-n%d" % (t, BM + dm, BN + dn), "1x1", t + 1, imgs, 20, H, W, BM + dm,
                          edges=("ragged_k", "m%+d" % dm, "n%+d" % dn)))
    return out


def _geometry_cases():
    """k_gemm, every (tile, conv operand mode): one geometry edge each"""
    geo = {
        "conv": [dict(KH=3, KW=3, dil=2, pad=2, edges=("dil2",)), dict(KH=2, KW=3, pad=1, edges=("kh_ne_kw",)),
                 dict(KH=3, KW=3, stride=2, pad=1, edges=("s2_odd",)), dict(KH=3, KW=3, pad=2, edges=("pad_ks-1",)),
                 dict(KH=3, KW=3, pad=0, edges=("pad0",))],
        "k3": [dict(pad=0, edges=("pad0",)), dict(pad=1, Cin=3, edges=("k27", "ragged_k")), dict(pad=2, edges=("pad_ks-1",)),
               dict(stride=2, pad=1, edges=("s2_odd",)), dict(pad=1, edges=("pad1",))],
        "k7": [dict(pad=3, Cin=2), dict(pad=6, Cin=2, edges=("pad_ks-1",)), dict(pad=0, Cin=2, edges=("pad0",)),
               dict(stride=2, pad=3, Cin=1, edges=("s2_odd",)), dict(stride=2, pad=3, Cin=3, edges=("s2_odd", "ragged_k"))],
        "k2": [dict(edges=("zero_edge",)), dict(edges=("zero_edge",)), dict(dmode="up2x4", edges=("zero_edge",)),
               dict(dmode="up2x4", edges=("zero_edge",)), dict(dmode="up2x4", edges=("zero_edge",))],
        "convt": [dict(KH=3, KW=3, stride=2, pad=1, opad=1, edges=("convt_opad",)), dict(KH=3, KW=3, stride=2, pad=1, edges=("convt_s2",)),
                  dict(KH=2, KW=2, stride=2, edges=("convt_s2",)), dict(KH=3, KW=3, pad=1), dict(KH=4, KW=4, stride=2, pad=1, edges=("convt_s2",))],
    }
    out = []
    for bm, rows in geo.items():
        for t, g in enumerate(rows):
            g = dict(g)
            edges = g.pop("edges", ())
            cin = g.pop("Cin", 5)
            out.append(_c("g-t%d-%s" % (t, bm), bm, t + 1, 2, cin, 9, 7, 40 if t != 1 else 20, edges=edges, **g))
    return out


GEMM_CASES = _ragged_cases() + _geometry_cases() + [
    # the K pipeline: 1, 2, 3, 4 K tiles per split
    *[_c("g-k%d" % n, "1x1", 1, 2, 16 * n, 4, 8, 40, edges=("ktiles%d" % n,)) for n in (1, 2, 3, 4)],
    _c("g-split-short", "1x1", 1, 2, 80, 4, 8, 40, splits=2, edges=("short_last_split",)),
    _c("g-split-empty", "1x1", 1, 2, 80, 4, 8, 40, splits=4, edges=("empty_splits",)),
    # the heuristic's tiles 1 and 2 (no override): a dilated conv is nobody else's
    _c("g-auto-m20", "conv", 0, 2, 5, 9, 7, 20, KH=3, KW=3, dil=2, pad=2, edges=("auto_tile1",)),
    _c("g-auto-n25", "conv", 0, 1, 5, 5, 5, 40, KH=3, KW=3, dil=2, pad=2, edges=("auto_tile2",)),
    _c("g-s2-1x1", "1x1", 1, 2, 20, 9, 7, 40, stride=2, edges=("s2_odd",)),
    _c("g-xcd", "1x1", 1, 17, 20, 8, 8, 40, edges=("xcd",)),
]

VEC_CASES = [
    # ragged M / N on the three tiles the dispatcher gives the vec kernel (tile by M <= 32, N <= 32)
    _c("v-t0-m63-n68", "1x1", 7, 1, 36, 4, 17, 63, edges=("ragged_k", "m-1")),
    _c("v-t0-m64-n64", "1x1", 7, 2, 36, 4, 8, 64, edges=("m+0", "n+0")),
    _c("v-t0-m65-n60", "1x1", 7, 3, 36, 4, 5, 65, edges=("m+1",)),
    _c("v-t1-m31-n132", "1x1", 7, 3, 36, 4, 11, 31, edges=("m-1",)),
    _c("v-t1-m32-n128", "1x1", 7, 2, 36, 8, 8, 32, edges=("m+0", "n+0")),
    _c("v-t1-m20-n124", "1x1", 7, 1, 36, 4, 31, 20),
    _c("v-t2-m127-n16", "1x1", 7, 1, 36, 4, 4, 127, edges=("m-1", "one_4x4_image")),
    _c("v-t2-m128-n32", "1x1", 7, 2, 36, 4, 4, 128, edges=("m+0", "n+0")),
    _c("v-t2-m129-n28", "1x1", 7, 1, 36, 4, 7, 129, edges=("m+1",)),
    *[_c("v-k%d" % n, "1x1", 7, 2, 32 * n, 4, 8, 40, edges=("ktiles%d" % n,)) for n in (1, 2, 3, 4)],
    *[_c("v-K%d" % k, "1x1", 7, 2, k, 4, 8, 40, edges=("ragged_k",)) for k in (36, 68, 100)],
    _c("v-split-short", "1x1", 7, 2, 160, 4, 8, 40, splits=2, edges=("short_last_split",)),
    _c("v-split-empty", "1x1", 7, 2, 160, 4, 8, 40, splits=4, edges=("empty_splits",)),
    # BS2: stride-2 conv1x1, two columns per load, on the three tiles; HoWo = 6: the scalar epilogue
    _c("v-s2-t0", "1x1", 7, 2, 36, 9, 16, 40, stride=2, edges=("bs2",)),
    _c("v-s2-t1", "1x1", 7, 3, 36, 10, 12, 20, stride=2, edges=("bs2",)),
    _c("v-s2-t2", "1x1", 7, 1, 36, 5, 12, 40, stride=2, edges=("bs2",)),
    _c("v-s2-howo6", "1x1", 7, 3, 36, 5, 4, 40, stride=2, edges=("bs2", "scalar_epilogue")),
    _c("v-up2x4", "1x1", 7, 2, 36, 4, 8, 40, dmode="up2x4", edges=("wide_up",)),
    _c("v-misD", "1x1", 7, 2, 36, 4, 8, 40, misD=True, edges=("scalar_epilogue",)),
    _c("v-auto", "1x1", 0, 2, 36, 4, 8, 40),
    _c("v-xcd", "1x1", 7, 17, 36, 8, 8, 40, edges=("xcd",)),
]


def _direct_cases():
    """k_conv_direct: every (KS, S) x pixel tile x WM, ragged rows / columns / images; packed twins come from packed_twin()"""
    out = []
    forms = (("k3", 1, 1, 24), ("k3", 2, 1, 24), ("k7", 1, 3, 6), ("k7", 2, 3, None), ("k2", 1, 0, 48))
    # Wout, Hout, images: 9 on the 4x4 tile, 3 on the 8x8 tile; Hout is no multiple of PTH and tall enough that the LAST staged row
    # of the patch lies inside the image under the first tile row (7x7: 7 | 11 rows - at 5 | 9 that row is always padding)
    shapes = ((3, 5, 9), (5, 9, 3), (9, 9, 2), (17, 5, 2))
    for bm, S, pad, cin in forms:
        for (Wo, Ho, imgs), M in itertools.product(shapes, (20, 40)):
            Ho += 2 if bm == "k7" else 0
            Hin, Win = (Ho, Wo) if S == 1 else (2 * Ho - 1, 2 * Wo - 1)
            if bm == "k7" and S == 2:
                cin_ = 1 if M == 20 else 3
            else:
                cin_ = cin
            kw = dict(dmode="up2x4") if bm == "k2" else {}
            edges = ["ragged_tile", "last_patch_row", "wm%d" % (1 if M == 20 else 2)] + (["s2_odd"] if S == 2 else []) + (["stem_tail"] if cin is None else [])
            out.append(_c("d-%s-s%d-w%d-m%d" % (bm, S, Wo, M), bm, 6, imgs, cin_, Hin, Win, M, stride=S, pad=pad, edges=edges, **kw))
    # one width per ladder step with Wout % 4 == 0: the wide epilogues (NCHW for 3x3, the 2 x 2 blocks for 2x2)
    for Wo, Ho in ((4, 5), (8, 9), (16, 9), (20, 5)):
        out.append(_c("d-k3-wide-w%d" % Wo, "k3", 6, 2, 8, Ho, Wo, 40, pad=1, edges=("wide",)))
        out.append(_c("d-k2-wide-w%d" % Wo, "k2", 6, 2, 16, Ho, Wo, 40, dmode="up2x4", edges=("wide",)))
    # two column tiles (Wout > 32), the second ragged: the only shapes whose patch starts at a column other than -pad
    for bm, S, pad, cin in forms:
        Ho = 7 if bm == "k7" else 5
        Hin, Win = (Ho, 33) if S == 1 else (2 * Ho - 1, 65)
        out.append(_c("d-%s-s%d-w33" % (bm, S), bm, 6, 1, cin or 3, Hin, Win, 40, stride=S, pad=pad, edges=("two_column_tiles", "last_patch_row"),
                      **(dict(dmode="up2x4") if bm == "k2" else {})))
    out += [
        _c("d-k2-odd-w5", "k2", 6, 2, 16, 5, 5, 40, dmode="up2x4", edges=("scalar_epilogue",)),
        _c("d-k2-nchw-w8", "k2", 6, 2, 16, 5, 8, 40, edges=("wide",)),
        _c("d-split2", "k3", 6, 2, 24, 5, 8, 40, pad=1, splits=2, edges=("short_last_split",)),
        _c("d-split16", "k3", 6, 2, 24, 5, 8, 40, pad=1, splits=16, edges=("splits_clamped",)),
        _c("d-auto", "k7", 0, 32, 2, 8, 8, 40, pad=3),   # no override: 16 blocks, just past the 7x7 pixel-starved gate
        _c("d-xcd", "k3", 6, 34, 8, 5, 5, 40, pad=1, edges=("xcd",)),
    ]
    return out


DIRECT_CASES = _direct_cases()

STREAM_CASES = [_c("s-k%d-m%d" % (K, M), "1x1", 8, 3, K, 8, 16, M, edges=("strips_change_image",) + (("ragged_strips",) if stream_waves(M, K)[1] < 4 else ()))
                for K in (64, 128, 256) for M in (20, 52, 96, 130)]


def packed_twin(c):
    return dict(c, tag=c["tag"] + "-pk", packed=True)


PACKED_CASES = [packed_twin(c) for c in DIRECT_CASES if c["ov"] == 6 and not c.get("splits")] + [packed_twin(c) for c in STREAM_CASES]

_R = dict(bmode="k3", ov=1, imgs=2, Cin=5, pad=1, M=40, splits=2)
REDUCE_CASES = [
    dict(_R, tag="r-nchw-howo25", Hin=5, Win=5, edges=("reduce_scalar",)),
    dict(_R, tag="r-nchw-howo64", Hin=8, Win=8, edges=("reduce4",)),
    dict(_R, tag="r-nchw-howo64-nwe", Hin=8, Win=8, nwe=True, edges=("reduce_scalar",)),
    dict(_R, tag="r-nchw-howo64-grp", Hin=8, Win=8, grp=1, edges=("reduce4",)),
    dict(_R, tag="r-up2", Hin=5, Win=6, dmode="up2", cls=(1, 0), edges=("reduce_scalar",)),
    dict(_R, tag="r-up2x4", bmode="k2", pad=0, Hin=5, Win=6, dmode="up2x4", edges=("reduce_scalar",)),
    dict(_R, tag="r-vec4", bmode="1x1", ov=7, Cin=160, pad=0, Hin=8, Win=8, edges=("reduce4",)),
]
UP2_CASES = [
    _c("u-k3-cls10", "k3", 1, 2, 5, 5, 6, 40, pad=1, dmode="up2", cls=(1, 0)),
    _c("u-1x1-cls01", "1x1", 1, 2, 20, 5, 6, 40, dmode="up2", cls=(0, 1)),
    _c("u-k2-cls11", "k2", 2, 2, 5, 5, 6, 20, dmode="up2", cls=(1, 1)),
]
# forms on the cases that name them: `kind` says what the GPU file does with the case
FORM_CASES = [
    dict(_c("f-shift-gemm", "k3", 1, 2, 5, 5, 6, 40, pad=1), kind="shift"),
    dict(_c("f-shift-vec", "1x1", 7, 2, 36, 4, 8, 40), kind="shift"),
    dict(_c("f-shift-direct", "k3", 6, 2, 8, 5, 8, 40, pad=1), kind="shift"),
    dict(_c("f-shift-stream", "1x1", 8, 3, 64, 8, 16, 52), kind="shift"),
    dict(_c("f-acc-gemm", "k3", 1, 2, 5, 5, 6, 40, pad=1, acc=True), kind="acc"),
    dict(_c("f-acc-gemm-3slabs", "k3", 1, 2, 5, 5, 6, 40, pad=1, acc=True, splits=3), kind="acc"),
    dict(_c("f-acc-vec", "1x1", 7, 2, 36, 4, 8, 40, acc=True), kind="acc"),
    dict(_c("f-acc-vec-2slabs", "1x1", 7, 2, 160, 4, 8, 40, acc=True, splits=2), kind="acc"),
    dict(_c("f-acc-direct", "k3", 6, 2, 24, 5, 8, 40, pad=1, acc=True), kind="acc"),
    dict(_c("f-acc-direct-3slabs", "k3", 6, 2, 24, 5, 5, 40, pad=1, acc=True, splits=3), kind="acc"),
    dict(_c("f-acc-stream", "1x1", 8, 3, 128, 8, 16, 52, acc=True), kind="acc"),
    dict(_c("f-defer-gemm", "k3", 1, 2, 5, 5, 6, 40, pad=1, defer=True, splits=3), kind="defer"),
    dict(_c("f-defer-gemm-1slab", "k3", 1, 2, 5, 5, 6, 40, pad=1, defer=True), kind="defer"),
    dict(_c("f-defer-vec", "1x1", 7, 2, 160, 4, 8, 40, defer=True, splits=2), kind="defer"),
    dict(_c("f-defer-direct", "k3", 6, 2, 24, 5, 8, 40, pad=1, defer=True, splits=3), kind="defer"),
    dict(_c("f-grp-gemm", "k3", 1, 4, 5, 8, 8, 40, pad=1, grp=2), kind="grp"),
    dict(_c("f-grp-gemm-fixup", "k3", 2, 4, 5, 8, 8, 20, pad=1, grp=1, edges=("grp_fixup",)), kind="grp"),
    dict(_c("f-grp-vec", "1x1", 7, 4, 36, 8, 8, 40, grp=2), kind="grp"),
    dict(_c("f-grp-direct", "k3", 6, 4, 8, 9, 9, 40, pad=1, grp=2), kind="grp"),
    dict(_c("f-grp-direct-wide", "k3", 6, 4, 8, 5, 8, 40, pad=1, grp=2), kind="grp"),
    dict(_c("f-grp-stream", "1x1", 8, 4, 128, 8, 16, 52, grp=2), kind="grp"),
    dict(REDUCE_CASES[3], kind="grp"),
    dict(_c("f-nwe-vec", "1x1", 7, 2, 36, 4, 8, 40), kind="nwe"),
    dict(_c("f-nwe-vec-up2x4", "1x1", 7, 2, 36, 4, 8, 40, dmode="up2x4"), kind="nwe"),
    dict(_c("f-nwe-direct", "k3", 6, 2, 8, 5, 8, 40, pad=1), kind="nwe"),
    dict(_c("f-nwe-direct-up2x4", "k2", 6, 2, 16, 5, 8, 40, dmode="up2x4"), kind="nwe"),
    dict(REDUCE_CASES[1], kind="nwe"),
    dict(GEMM_CASES[-1], kind="noxcd"), dict(VEC_CASES[-1], kind="noxcd"), dict(DIRECT_CASES[-1], kind="noxcd"),
]
_F = dict(imgs=4, Cin=36, Hin=4, Win=8, M=40, bmode="1x1")
FLAG_CASES = [dict(_F, tag="fl-%s-%s" % (name, "".join(map(str, fl))), ov=ov, flags=fl, edges=())
              for name, ov in (("gemm", 1), ("vec", 7), ("auto", 0)) for fl in ((1, 0, 0, 0), (0, 0, 1, 1), (0, 0, 0, 0), (0, 1, 1, 0))]
FLAG_CASES += [dict(_F, tag="fl-auto-k3", bmode="k3", Cin=5, pad=1, ov=0, flags=(0, 0, 1, 0), edges=())]
STAT_CASES = [
    _c("st-k3-w8", "k3", 6, 3, 8, 5, 8, 20, pad=1, stats=True),
    _c("st-k7-w16-m40", "k7", 6, 2, 2, 9, 16, 40, pad=3, stats=True),
    _c("st-k3-s2-w4", "k3", 6, 9, 8, 9, 7, 40, stride=2, pad=1, stats=True),
    _c("st-k3-w5-scalar", "k3", 6, 2, 8, 5, 5, 20, pad=1, stats=True, edges=("scalar_epilogue",)),
    _c("st-k3-w8-split", "k3", 6, 2, 24, 5, 8, 20, pad=1, stats=True, splits=3, edges=("scalar_epilogue",)),
]

_D = dict(bmode="k3", ov=6, imgs=2, Cin=8, Hin=5, Win=8, M=40, pad=1)
_V = dict(bmode="1x1", ov=7, imgs=2, Cin=36, Hin=4, Win=8, M=40)
_S = dict(bmode="1x1", ov=8, imgs=3, Cin=128, Hin=8, Win=16, M=52)
REFUSALS = [   # (case, return code)
    (dict(_D, tag="no-d-dil", bmode="conv", KH=3, KW=3, dil=2, pad=2), "unsupported"),
    (dict(_D, tag="no-d-dil-k3", dil=2, pad=2), "unsupported"),
    (dict(_D, tag="no-d-k2-s2", bmode="k2", Cin=16, stride=2, pad=0), "unsupported"),
    (dict(_D, tag="no-d-cin", Cin=12), "unsupported"),
    (dict(_D, tag="no-d-cin-k7-s1", bmode="k7", Cin=3, pad=3), "unsupported"),
    (dict(_D, tag="no-d-grp", imgs=4, Hin=5, Win=5, grp=1), "unsupported"),
    (dict(_V, tag="no-v-A", misA=True), "unsupported"),
    (dict(_V, tag="no-v-B", misB=True), "unsupported"),
    (dict(_V, tag="no-v-K", Cin=38), "unsupported"),
    (dict(_V, tag="no-v-lda", lda_pad=2), "unsupported"),
    (dict(_V, tag="no-v-s2-pad", stride=2, pad=1, Hin=8, Win=8), "unsupported"),
    (dict(_V, tag="no-v-s2-geometry", stride=2, Hin=9, Win=7), "unsupported"),
    (dict(_V, tag="no-v-s2-wout-odd", stride=2, Hin=8, Win=6), "unsupported"),
    (dict(_V, tag="no-v-s2-imgstride", stride=2, Hin=8, Win=8, img_pad=2), "unsupported"),
    (dict(_V, tag="no-v-stride3", stride=3, Hin=8, Win=8), "unsupported"),
    (dict(_V, tag="no-v-pad", pad=1), "unsupported"),
    (dict(_V, tag="no-v-howo", Hin=3, Win=5), "unsupported"),
    (dict(_V, tag="no-v-imgstride", img_pad=2), "unsupported"),
    (dict(_V, tag="no-v-bmode", bmode="k3", Cin=8, pad=1), "unsupported"),
    (dict(_S, tag="no-s-k96", Cin=96), "unsupported"),
    (dict(_S, tag="no-s-howo", Hin=8, Win=12), "unsupported"),
    (dict(_S, tag="no-s-misD", misD=True), "unsupported"),
    (dict(_S, tag="no-s-splits", splits=2), "unsupported"),
    (dict(_S, tag="no-s-stats", stats=True), "unsupported"),
    (dict(_D, tag="no-flags-6", flags=(1, 0)), "invalid"),
    (dict(_S, tag="no-flags-8", flags=(1, 0, 1)), "invalid"),
    (dict(_V, tag="no-flags-9", ov=9, flags=(1, 0)), "invalid"),
    (dict(_V, tag="no-flags-defer", defer=True, flags=(1, 0)), "invalid"),
    (dict(_D, tag="no-up2x4-m", bmode="k2", Cin=16, pad=0, ov=1, M=42, dmode="up2x4"), "invalid"),
    (dict(_V, tag="no-9-without-split", ov=9), "unsupported"),
]
for _case, _ in REFUSALS:
    _case.setdefault("edges", ())

LAUNCH_CASES = GEMM_CASES + VEC_CASES + DIRECT_CASES + STREAM_CASES + PACKED_CASES + REDUCE_CASES + UP2_CASES + \
    [c for c in FORM_CASES if c["tag"].startswith("f-")] + FLAG_CASES + STAT_CASES

# the operand pairs k_gemm is also built for: dense / weight-gradient descriptors, held by tests that exist
DENSE_PAIRS = {
    ("A_KM", "B_NK"): ("test_gpu_train_gemms.py", "test_linear_bwd_input"),
    ("A_KM", "B_KN"): ("test_gpu_train_gemms.py", "test_linear_bwd_weight"),
    ("A_NCHW_P", "B_IM2COL_T"): ("test_gpu_train_gemms.py", "test_conv2d_bwd_weight_gemm_geometries"),
    ("A_MK", "B_NK"): ("test_gpu_kernels.py", "test_vector_load_gemm_all_operand_layouts"),
    ("A_MK", "B_KN"): None,   # built, and no descriptor of ops.py asks for it
}
REDUCE_COVERED = {"k_splitk_epilogue_flat4": ("test_gpu_train_gemms.py", "test_linear_bwd_weight")}


def by_tag():
    out = {}
    for c in LAUNCH_CASES + [c for c, _ in REFUSALS]:
        assert out.setdefault(c["tag"], c) is c or out[c["tag"]] == c, "two cases named " + c["tag"]
    return out


# ------------------------------------------------------------------------------------------------------------------
# the tests
# ------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_sources():
    const = lambda src, name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))   # noqa: E731
    assert (const(_COMMON, "BK"), const(_VEC, "BKV"), const(_STREAM, "min_n")) == (BK, BKV, STREAM_MIN_N)
    assert int(re.search(r"blocks < (\d+) && !force", _STREAM).group(1)) == STREAM_FLOOR
    m = re.search(r"conv_direct_ci\(int KS\) \{ return KS == 7 \? (\d+) : \(KS == 2 \? (\d+) : (\d+)\); \}", _COMMON)
    assert {7: int(m.group(1)), 2: int(m.group(2)), 3: int(m.group(3))} == CI
    # the pixel-tile ladder, in the launcher and in launch_ks
    m = re.search(r"PTW = d\.Wout > (\d+) \? (\d+) : \(d\.Wout > (\d+) \? (\d+) : \(d\.Wout > (\d+) \? (\d+) : (\d+)\)\);", _DIRECT)
    w = [int(v) for v in m.groups()]
    assert [(w[0], w[1]), (w[2], w[3]), (w[4], w[5]), (0, w[6])] == [(a, b) for a, b, _, _ in LADDER]
    assert "PTH = PTW == 32 ? 4 : (PTW == 4 ? 4 : 8);" in _DIRECT and "IMGS = 128 / (PTW * PTH);" in _DIRECT
    ks = re.findall(r"(?:if|else if|else) ?\(?(?:d\.Wout > (\d+)\))? ?launch_wm<KS, (\d+), (\d+), (\d+), S>", _DIRECT)
    assert [(int(a or 0), int(b), int(c), int(e)) for a, b, c, e in ks] == list(LADDER)
    for w_, ptw, pth, imgs in LADDER:
        assert ptw * pth * imgs == 128 and pth == (4 if ptw in (32, 4) else 8)
    # the block tiles: `case t:` of ivln_gemm_f32's switch and of ivln_gemm_vec_launch
    for src, fn, order in ((_GEMM, "launch_tile", (1, 2, 3, 4, 0)), (_VEC, "launch_vec", (1, 2, 3, 4, 0))):
        got = re.findall(r"(?:case \d|default): (?:rc = )?%s<(\d), (\d), (\d), (\d)>\(d, s" % fn, src)
        assert len(got) == 5
        for t, (wm, wn, tm, tn) in zip(order, got):
            assert (32 * int(wm) * int(tm), 32 * int(wn) * int(tn), int(tm), int(tn)) == TILES[t], (fn, t)
    fam = re.findall(r'"(\w+)"', re.search(r"kFamilyKernels\[\] = \{([^}]*)\}", _GEMM).group(1))
    assert set(FAMILY) <= set(fam)
    # the operand pairs k_gemm is built for: the six conv modes of this file + DENSE_PAIRS
    pairs = re.findall(r"IVLN_CASE\(AMODE_(\w+), BMODE_(\w+)\)", _GEMM)
    conv = {("MK", m) for m in ("CONV", "CONV1X1", "CONV_K3", "CONV_K7", "CONV_K2", "CONVT")}
    assert set(pairs) == conv | {(a[2:], b[2:]) for a, b in DENSE_PAIRS}
    # enum values the GPU file hands to the descriptor
    enum = dict(re.findall(r"BMODE_(\w+) = (\d+)", _COMMON))
    assert {k: int(enum[n]) for k, n in (("conv", "CONV"), ("1x1", "CONV1X1"), ("convt", "CONVT"), ("k3", "CONV_K3"), ("k7", "CONV_K7"), ("k2", "CONV_K2"))} == BMODES
    assert re.search(r"DMODE_NCHW = 0, DMODE_DENSE = 1, DMODE_NCHW_UP2 = 2, DMODE_NCHW_UP2X4 = 3", _COMMON)


def test_wide_fits_per_vec_instantiation():
    """64 x 64 (LAY_K, LAY_R) fits with no word to spare; LAY_R x LAY_R does not; the two other tiles have room"""
    assert vec_wide_fits(64, 64) == (True, 0)
    assert vec_wide_fits(32, 128) == (True, 1024) and vec_wide_fits(128, 32) == (True, 1024)
    assert vec_wide_fits(64, 64, alay_k=False)[0] is False
    assert vec_wide_fits(64, 64, blay_k=True)[0] and vec_wide_fits(64, 64, alay_k=False, blay_k=True)[0]
    # the register-tiled tiles, which the dispatcher never hands the vec kernel
    assert vec_wide_fits(128, 128)[0] is False and vec_wide_fits(64, 128)[0] is False
    assert "LDK = BKV + 4" in _VEC and "LDC = BN + 4" in _VEC and "WIDE_FITS = BM * LDC <= A_WORDS + B_WORDS" in _VEC
    assert "if (vec && tile != 1 && tile != 2) tile = vec_tile_env >= 0 ? vec_tile_env : 0;" in _GEMM
    assert "constexpr int vec_tile_env = -1;" in _GEMM


def test_epilogue_tile_vec4_is_for_dense_destinations_only():
    assert "const bool vec4 = !to_ws && p.dmode == DMODE_DENSE && p.sDm == 1 && (p.sDn & 3) == 0 && (p.M & 3) == 0 &&" in _COMMON
    assert epilogue_tile_vec4(True, 1, 512, 40, True, False)
    assert not epilogue_tile_vec4(False, 1, 512, 40, True, False) and not epilogue_tile_vec4(True, 1, 512, 40, True, True)
    assert not epilogue_tile_vec4(True, 1, 510, 40, True, False) and not epilogue_tile_vec4(True, 1, 512, 42, True, False)


def test_dense_pairs_and_the_flat_reduction_are_held_by_tests_that_exist():
    for where in list(DENSE_PAIRS.values()) + list(REDUCE_COVERED.values()):
        if where is not None:
            assert re.search(r"^def %s\(" % where[1], open(os.path.join(ROOT, "tests", where[0])).read(), re.M), where
    ops_src = open(os.path.join(ROOT, "ivln-ce_amd", "ops.py")).read()
    assert not re.search(r"A_MK, B_KN\b", ops_src)


def _edge(c, name):
    d, p = desc(c), plan(c)
    BM, BN = TILES[p.tile][:2] if p.tile is not None else (None, None)
    bk = BKV if p.kernel == "k_gemm_vec" else BK
    if name.startswith("ktiles"):
        return p.splits == 1 and cdiv(d.K, bk) == int(name[6:])
    if name[0] in "mn" and name[1] in "+-":
        v, b = (d.M, BM) if name[0] == "m" else (d.N, BN)
        return (v - int(name[1:])) % b == 0
    if name == "one_4x4_image":
        return d.N == 16 and d.nimg == 1
    return {
        "ragged_k": lambda: d.K % bk != 0,
        "short_last_split": lambda: p.splits == d.splits and (
            0 < p.last_tiles < p.tps if p.kernel != "k_conv_direct" else cdiv(d.Cin, CI[d.KS]) % p.splits != 0),
        "empty_splits": lambda: 1 < p.splits < d.splits,
        "splits_clamped": lambda: p.splits == cdiv(d.Cin, CI[d.KS]) < d.splits,
        "auto_tile1": lambda: d.ov == 0 and p.tile == 1, "auto_tile2": lambda: d.ov == 0 and p.tile == 2,
        "s2_odd": lambda: d.stride == 2 and (d.Hin % 2 == 1 or d.Win % 2 == 1),
        "dil2": lambda: d.dil == 2, "kh_ne_kw": lambda: d.KH != d.KW, "k27": lambda: d.K == 27,
        "pad0": lambda: d.pad == 0 and d.KH > 1, "pad1": lambda: d.pad == 1, "pad_ks-1": lambda: d.pad == d.KH - 1 and d.KH > 2,
        "zero_edge": lambda: d.bmode == "k2" and d.Hout == d.Hin,
        "convt_opad": lambda: d.bmode == "convt" and d.stride == 2 and d.opad == 1,
        "convt_s2": lambda: d.bmode == "convt" and d.stride == 2 and d.opad == 0,
        "xcd": lambda: p.nwg >= 16 and p.nwg % 8 != 0,
        "bs2": lambda: p.key[-1] is True,
        "wide": lambda: p.wide, "wide_up": lambda: p.wide and d.dmode == "up2x4",
        "scalar_epilogue": lambda: not p.wide and plan(dict(c, misD=False, nwe=False, stats=False)).kernel == p.kernel,
        "ragged_tile": lambda: d.Wout % p.key[3] != 0 and d.Hout % ladder(d.Wout)[1] != 0 and d.nimg % ladder(d.Wout)[2] in (1, 0)
        and (ladder(d.Wout)[2] == 1 or d.nimg % ladder(d.Wout)[2] == 1),
        "last_patch_row": lambda: (ladder(d.Wout)[1] - 1) * d.stride + d.KS - 1 - d.pad < d.Hin and d.Hout > ladder(d.Wout)[1],
        "two_column_tiles": lambda: cdiv(d.Wout, p.key[3]) == 2 and d.Wout % p.key[3] != 0,
        "wm1": lambda: p.key[4] == 1 and d.M == 20, "wm2": lambda: p.key[4] == 2 and d.M == 40,
        "stem_tail": lambda: d.KS == 7 and d.stride == 2 and d.Cin in (1, 3),
        "strips_change_image": lambda: d.HoWo == 128 and d.nimg > 1,
        "ragged_strips": lambda: (d.N // 128) % (4 // p.key[2]) != 0,
        "reduce_scalar": lambda: p.reduce[0] == "k_splitk_epilogue", "reduce4": lambda: p.reduce[0] == "k_splitk_epilogue4",
        "grp_fixup": lambda: d.ov - 1 != p.tile,
    }[name]()


def test_every_case_reaches_the_edges_its_tag_names():
    for c in LAUNCH_CASES:
        for form in FORMS:
            p = plan(c, form=form)
            assert p.ok, (c["tag"], form, p.why)
        for name in c["edges"]:
            assert _edge(c, name), (c["tag"], name)
    tags = by_tag()
    # what the tags themselves promise
    for K in (64, 128, 256):
        assert {plan(tags["s-k%d-m%d" % (K, M)]).key[2] for M in (20, 52, 96, 130)} == {1, 2, 4}
    for c in PACKED_CASES:
        assert plan(c).key[-1] is True and plan(dict(c, packed=False)).key[:-1] == plan(c).key[:-1]
    assert {M for M in (20, 52, 96, 130) if M in PARENT_OVERRUNS} == {20, 96, 130}   # the K = 64 packed cases the parent overran
    for c in FLAG_CASES:
        p = plan(c)
        assert p.splits == 1 and p.kernel == ("k_gemm" if c["ov"] == 1 or c["bmode"] == "k3" else "k_gemm_vec")
        assert p.runs == [any(c["flags"][2 * i:2 * i + 2]) for i in range(2)]   # 64-pixel tiles over 32-pixel images
    assert plan(tags["fl-gemm-0110"]).runs == [True, True] and plan(tags["fl-vec-0000"]).runs == [False, False]
    for c in STAT_CASES:
        p = plan(c)
        assert (p.stat_tiles > 0) == ("scalar_epilogue" not in c["edges"]) and (p.stat_tiles == 0 or p.stat_tiles == p.grid[0])
    assert plan(tags["st-k3-s2-w4"]).stat_tiles == 2 * cdiv(9, 8) and plan(tags["st-k3-w8"]).stat_tiles == cdiv(3, 2)   # rows x image groups
    for c in FORM_CASES:
        p = plan(c)
        assert p.ok
        if c["kind"] == "defer":
            assert p.slabs == p.splits and p.reduce is None
        if c["kind"] == "nwe":
            assert (p.wide or p.reduce[0] == "k_splitk_epilogue4") and not plan(dict(c, nwe=True)).wide
            assert plan(dict(c, nwe=True)).key == p.key
        if c["kind"] == "grp":
            assert c["grp"] > 0
    assert plan(tags["f-acc-gemm-3slabs"]).splits == 3 and plan(tags["f-acc-direct-3slabs"]).splits == 3
    assert plan(tags["d-split2"]).splits == 2 and plan(tags["d-split16"]).splits == 3
    assert plan(tags["g-split-short"]).splits == 2 and plan(tags["g-split-empty"]).splits == 3
    assert plan(tags["d-auto"]).kernel == "k_conv_direct" and plan(tags["v-auto"]).kernel == "k_gemm_vec"


def test_refusal_shapes_are_refused_by_the_clause_they_name():
    seen = set()
    for c, code in REFUSALS:
        for form in FORMS:
            p = plan(c, form=form)
            assert not p.ok and p.code == code, (c["tag"], form, p.why)
        seen.add(plan(c).why)
    # every clause of ivln_gemm_vec_eligible an A_MK x conv descriptor can fail, once each
    vec = {plan(c).why for c, _ in REFUSALS if c["tag"].startswith("no-v-")}
    assert vec == {"vec: " + w for w in ("A", "B", "K%4", "lda%4", "s2 pad", "s2 geometry", "s2 image stride", "stride", "pad",
                                          "HoWo%4", "image stride", "bmode")} , vec
    # the base shapes the refusals are cut from are accepted
    for base in (_D, _V, _S):
        assert plan(dict(base, tag="base", edges=())).ok


def _grid():
    """descriptors wider than the cases: every override x mode x a spread of sizes, with and without splits / packs"""
    sizes = [(1, 4, 4), (2, 5, 5), (2, 8, 8), (3, 9, 7), (9, 5, 3), (2, 5, 9), (2, 5, 17), (2, 8, 16), (3, 8, 16), (2, 12, 20), (40, 8, 16), (2, 9, 33)]
    for bm in BMODES:
        for ov in range(0, 9):
            for imgs, H, W in sizes:
                for M in (20, 32, 40, 64, 96, 130, 260):
                    for cin in ((1, 3, 8, 16, 24, 36, 48, 64, 128, 256) if ov in (0, 6, 7, 8) else (5,)):
                        for extra in ({}, dict(stride=2), dict(splits=2), dict(packed=True), dict(stride=2, packed=True), dict(dmode="up2x4"), dict(dmode="up2", splits=2),
                                      dict(splits=2, nwe=True), dict(splits=2, grp=1), dict(dmode="up2x4", splits=2)):
                            c = dict(tag="grid", bmode=bm, ov=ov, imgs=imgs, Cin=cin, Hin=H, Win=W, M=M, edges=(), **extra)
                            if bm in ("conv", "convt"):
                                c.update(KH=3, KW=3)
                            c["pad"] = {"k3": 1, "k7": 3, "conv": 1, "convt": 1}.get(bm, 0)
                            if extra.get("packed") and conv_packed_floats(M, cin, {"1x1": 1}.get(bm, KS_OF.get(bm, 0))) == 0:
                                continue
                            if bm == "convt" and extra.get("stride") and H < 2:
                                continue
                            yield c


def reachable_keys():
    keys = set()
    for c in _grid():
        p = plan(c)
        if p.ok:
            keys |= p.keys
    return keys


def test_cases_cover_every_instantiation_the_plans_can_produce():
    have = set()
    for c in LAUNCH_CASES:
        have |= plan(c).keys
    reach = reachable_keys()
    assert reach - have == set(), sorted(reach - have, key=str)
    assert have - reach == set(), sorted(have - reach, key=str)   # (the grid is wider than the cases)
    of = lambda name: {k for k in have if k[0] == name}   # noqa: E731
    assert of("k_gemm") == {("k_gemm", t, "A_MK", bm) for t in range(5) for bm in BMODES}
    assert of("k_gemm_vec") == {("k_gemm_vec", t, "LAY_K", "LAY_R", s2) for t in (0, 1, 2) for s2 in (False, True)}
    assert of("k_conv_direct") == {("k_conv_direct", KS, S, ptw, wm, pk) for KS, S in ((3, 1), (3, 2), (7, 1), (7, 2), (2, 1))
                                   for ptw in (4, 8, 16, 32) for wm in (1, 2) for pk in (False, True)}
    assert of("k_conv1x1_stream") == {("k_conv1x1_stream", K, w, pk) for K in (64, 128, 256) for w in (1, 2, 4) for pk in (False, True)}
    assert of("k_splitk_epilogue") == {("k_splitk_epilogue", m) for m in DMODES}
    assert of("k_splitk_epilogue4") == {("k_splitk_epilogue4", "nchw", g) for g in (False, True)}
