"""CPU: the dispatch of the split-bf16 conv kernels (csrc/conv_bf3.hip behind ivln_gemm_f32) restated in plain Python, the
case tables of tests/test_gpu_conv_bf3_kernels.py (which imports them, and `plan`, from here and holds the real launchers to
the plans: kernel name, splits_used, the ivln_conv_split_kinds tally, stat_tiles, accepted versus refused), and the kernels'
arithmetic - split3 and the six-of-nine piece products - restated in numpy / float64.

Restated (line ranges of ivln-ce_amd/csrc/conv_bf3.hip unless another file is named):
  ivln_gemm_f32's A_split branches   gemm_conv.hip 532-606   residual_after_relu, pool2, fuse_A_split, tile_override 0 | >= 9
  ivln_conv_bf3_launch               1883-2067   refusals, the override ladder (9 | 10 14 15 | 11 12 13 | 20 + c), the tile
                                                 heuristic, slabs over blockIdx.z, stat_tiles, the tally's form index
  bf3_px / launch_bf3_px             1295-1334   pixel tile (rows x columns x images) of a block tile for the output width
  launch_bf3 / launch_bf3_fused      1260-1293   LDS bytes (a tile whose patch exceeds 160 KB is refused), the grid
  launch_bf3_ks<KS> / launch_bf3_s2  1336-1380   block tiles per kernel size; stride 2: whole 16-channel chunks, tiles 2 ... 6
  bf3_ks_launch                      645-694     3x3 / stacked 2x2 with K split over the waves: 32- or 64-pixel tiles
  bf3_1x1_ks_launch                  1189-1236   the 1x1 kernels: K-split form or wave tiles
  bf3_conv7_pool_launch              844-879     the map CNN block: NW = 1, 2, 4, 8 waves by chunk count, the u8 map form
  bf3_stem_launch                    1833-1851   7x7 stride 2 of 1 | 3 channels: four items per workgroup
  ivln_wgrad_bf3_launch              2070-2121   the five tile forms, strips over blockIdx.z
ivln_cu_count() is the parameter `cus` (256 here, the device's count in the GPU file).  Environment switches (IVLN_BF3_*) are
taken as unset.  Not restated: img_run_flags (ivln_gemm_f32 clears A_split for it: these kernels never see it) and
defer_epilogue (refused by every launcher here).

The tables read from the sources - kBf3BM, kBf3BN, CB, PIXB, bf3_taps_padded, kFamilyKernels - are compared with the tiles
this file states (test_tile_tables_are_the_sources): a changed tile table is noticed here before a GPU sees it.

Cases.  Every case pins its form with tile_override (20 + c, 10, 14, 15, 12, 13, 9), so its plan is the same at every CU
count; the exceptions say so (`cus` in the case: the fused tail's 64-pixel tile needs wg128 < CUs, the slab cases' split
count is the chunk count at every CU count >= 4).  test_every_case_reaches_the_edges_its_tag_names asserts it of the plan.  The coverage pin
(test_cases_cover_every_instantiation_the_plans_can_produce) enumerates the launchers' accepted domain over a grid of
descriptors wider than the cases and requires the union of the cases' instantiation keys to equal what the grid reaches.

Arithmetic.  split3_np is bf3_common.h's split3 (round to nearest even at each step, remainders exact in fp32); piece_product_conv
is the conv as the kernels compute it: the six piece products a1b3 a2b2 a3b1 a1b2 a2b1 a1b1, each conv exact (float64), the
accumulator rounded to fp32 after each.  On the `single_tap` inputs (one non-zero weight per output channel: every output is
ONE product) every five-product form is over the bar of tests/kernel_bar.py - a lost cross term in any instantiation fails
the GPU test.  `dense` inputs do not show that: with K = 1176 terms of random sign a dropped low product moves a sum by about
1.1e-5 relative to its largest term's scale, which the bar's 4 * e32 (the fp32 reference's own error over 1176 terms) does
not exclude; with one term per output e32 is one rounding and the bar is about 8 * 2^-24 of the product.

The defect this file records: the index ivln_conv_split_kinds counts a 1x1 launch under was worked out beside the launcher
from the chunk count (<= 16 chunks: wave tiles), not from the form bf3_1x1_ks_launch chose - a pinned form into the 2 x 2-block
stores (x1-12-up) and, in production, 24 / 32 / 48 chunks over more than 2 CUs' worth of tiles (256 x 16384 x 512 runs as wave
tiles) were counted as the other form.  kind_parent keeps that rule; no kernel, grid or split count of any plan changed.

Scope.  The GPU file runs the tiled kernel (k_conv_bf3: stride 1 for KS 1 / 2 / 3 / 7, stride 2 for 1x1 and 3x3, slabs over
blockIdx.z, the fused tail), k_conv_bf3_ks, k_conv1x1_bf3_ks, k_conv7_pool_bf3, k_conv7s2_bf3 and k_wgrad_bf3; the tables
below list every case."""
import itertools
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ivln-ce_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _int_table(src, name):
    m = re.search(r"constexpr int %s\[\w+\] = \{([^}]*)\};" % name, src)
    return [int(v) for v in m.group(1).split(",")]


def _const(src, name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


_BF3, _COMMON, _GEMM = _src("conv_bf3.hip"), _src("bf3_common.h"), _src("gemm_conv.hip")
BM_T, BN_T = _int_table(_BF3, "kBf3BM"), _int_table(_BF3, "kBf3BN")   # channels, pixels of block tile c
CB, PIXB = _const(_COMMON, "CB"), _const(_COMMON, "PIXB")
LDS_MAX = 160 * 1024
# (TM, WM, WN) of block tile c as launch_bf3_ks<KS> instantiates it: BM = 32 TM WM, BN = 64 WN
TILE = [(1, 1, 8), (2, 1, 8), (1, 2, 4), (2, 2, 4), (1, 2, 2), (2, 2, 2), (1, 1, 4)]
# (plan.kind: the counter of ivln_conv_split_kinds a launch lands in - 0 tiled, 1 3x3 K-split, 2 1x1 K-split, 3 1x1 wave tiles)


def family_kernels():
    m = re.search(r"kFamilyKernels\[\] = \{([^}]*)\}", _GEMM)
    return re.findall(r'"(\w+)"', m.group(1))


def taps_padded(KS):
    return {7: 54, 3: 9, 2: 4, 1: 1}[KS]


def stage_chunks(KS):
    return 4 if KS == 1 else 1


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------
# a case -> the descriptor's integers
# ------------------------------------------------------------------------------------------------------------------
FORMS = ("plain", "full")   # epilogue forms every instantiation runs: nothing | scale + shift + residual + ReLU into a channel slice


def desc(c, form="plain"):
    """The ivln_gemm_desc of a case as integers and presence flags (pointers: True / False; *_al: 16-byte aligned).
    Case keys: kind (conv | pool | stem | wgrad | fused), KS, stride, imgs, Cin, H, W (the OUTPUT map), M, ov (tile_override),
    up (IVLN_D_NCHW_UP2X4; KS 2 always), ws (a workspace and splits = 0: the launcher may split), splits (forced),
    ws_splits (workspace size in slabs), stats, grp (grp_imgs), acc, post (residual_after_relu), nwe (no_wide_epilogue),
    misB (B four bytes off a 16-byte boundary), fuse_M, u8, split_ok, and for refusal shapes only: Hin / Win overrides."""
    kind, KS, st = c.get("kind", "conv"), c.get("KS", 7), c.get("stride", 1)
    d = types.SimpleNamespace()
    d.kind, d.KS, d.stride, d.M, d.Cin, d.Hout, d.Wout = kind, KS, st, c["M"], c["Cin"], c["H"], c["W"]
    d.Hin, d.Win = c["H"] * st, c["W"] * st
    d.nimg = c["imgs"]
    d.HoWo = d.Hout * d.Wout
    d.pad = 0 if KS in (1, 2) else KS // 2
    d.up = bool(c.get("up")) or KS == 2
    d.ov = c.get("ov", 0)
    d.A_split = True
    d.grp_imgs, d.accumulate, d.post = c.get("grp", 0), bool(c.get("acc")), bool(c.get("post"))
    d.stats, d.nwe = bool(c.get("stats")), bool(c.get("nwe"))
    d.fuse_M, d.pool2, d.u8, d.split_ok = c.get("fuse_M", 0), kind == "pool", bool(c.get("u8")), c.get("split_ok", 1)
    full = form == "full"
    d.has_scale = d.has_shift = full or kind in ("pool", "fused")
    d.relu = full or kind in ("pool", "fused")
    d.has_res = (full and kind != "pool") or d.post or kind == "fused"
    if kind == "wgrad":   # A = dy (NCHW_P), B = x (IM2COL_T), dense dW: M = Cout, N = Cin * 49, K = pixels
        d.N, d.K = d.Cin * 49, d.nimg * d.HoWo
        d.has_scale = d.has_shift = d.has_res = d.relu = False
        d.Ctot = 0
    else:
        d.N, d.K = d.nimg * d.HoWo, d.Cin * KS * KS
        # the slice form: a destination 8 channels wider than the launch writes (not where Ctot is bound to M: the 2 x 2-block stores)
        d.Ctot = d.M // 4 if d.up else (d.fuse_M if kind == "fused" else d.M) + (8 if full and not d.up else 0)
    d.in_img_stride = d.Cin * d.Hin * d.Win + (8 if full and not d.u8 else 0)   # padded image stride in the full form
    d.B_al, d.D_al, d.res_al, d.ws_al, d.A_al8 = not c.get("misB"), True, True, True, True
    d.ws = bool(c.get("ws")) or kind == "wgrad" and not c.get("no_ws")
    d.splits = c.get("splits", 0 if d.ws else 1)
    slabs = c.get("ws_splits", 16)
    d.ws_floats = slabs * d.M * d.N if d.ws else 0
    for k in ("Hin", "Win"):
        if k in c:
            setattr(d, k, c[k])
    return d


def _no(code, why):
    return types.SimpleNamespace(ok=False, code=code, why=why)


def _yes(kernel, key, grid, splits, kind, stat_tiles=0, lds=0):
    return types.SimpleNamespace(ok=True, kernel=kernel, key=(kernel,) + tuple(key), grid=tuple(grid), splits=splits, kind=kind,
                                 stat_tiles=stat_tiles, lds=lds)


# ------------------------------------------------------------------------------------------------------------------
# the tiled kernel's launchers
# ------------------------------------------------------------------------------------------------------------------
def bf3_px(BN, Wout):
    """pixel tile of a block for its pixel count and the output width: rows, columns, images"""
    ptw = 32 if Wout > 16 else (16 if Wout > 8 else 8)
    pth = BN // 32 if ptw == 32 else ((16 if BN >= 256 else 8) if ptw == 16 else 8)
    return pth, ptw, BN // (ptw * pth)


# launch_bf3_px's own table, written out as the C has it (the dispatcher counts blocks with bf3_px: the two must agree)
PX_TABLE = {512: ((16, 32, 1), (16, 16, 2), (8, 8, 8)), 256: ((8, 32, 1), (16, 16, 1), (8, 8, 4)), 128: ((4, 32, 1), (8, 16, 1), (8, 8, 2))}


def launch_bf3(d, KS, cfg, px, ST, cps):
    TM, WM, WN = TILE[cfg]
    BM, BN = 32 * TM * WM, 64 * WN
    pth, ptw, imgs = px
    PH, PWR = (pth + 1, ptw + 1) if ST == 2 else (pth + KS - 1, ptw + KS - 1)
    npix = imgs * (4 if ST == 2 else 1) * PH * PWR * stage_chunks(KS)
    lds = max(npix * PIXB, 32 * (BN + 4) * 4)
    if lds > LDS_MAX:
        return _no("unsupported", "patch exceeds the LDS")
    tiles_w, tiles_h, groups = cdiv(d.Wout, ptw), cdiv(d.Hout, pth), cdiv(d.nimg, imgs)
    form = "tile-strided" if (KS == 1 and d.stride == 2) else "tile"   # (1x1 at stride 2: the same instantiation, another patch address)
    return _yes("k_conv_bf3", (KS, cfg, pth, ptw, imgs, ST, form), (tiles_w * tiles_h * groups, cdiv(d.M, BM), d.splits), d.splits, 0, lds=lds)


def launch_bf3_px(d, KS, cfg, ST, cps):
    BN = 64 * TILE[cfg][2]
    cls = 0 if d.Wout > 16 else (1 if d.Wout > 8 else 2)
    if ST == 2:
        assert KS == 3 and BN in (128, 256)
        return launch_bf3(d, KS, cfg, PX_TABLE[BN][cls], 2, cps)
    if BN == 512 and KS == 1:
        return _no("unsupported", "four staged chunks of 512 pixels")
    if BN == 512 and cls == 2 and KS != 3:
        return _no("unsupported", "512-pixel tile on an 8-wide map")
    return launch_bf3(d, KS, cfg, PX_TABLE[BN][cls], 1, cps)


def launch_bf3_ks(d, KS, cfg, cps):
    if KS == 2 and cfg not in (2, 3, 4, 5):
        return _no("unsupported", "2x2 window: tiles 2 ... 5")
    return launch_bf3_px(d, KS, min(cfg, 6), 1, cps)


def launch_bf3_s2(d, cfg, cps):
    if d.Cin % CB:
        return _no("unsupported", "Cin % 16")
    if cfg not in (2, 3, 4, 5, 6):
        return _no("unsupported", "stride 2: tiles 2 ... 6")
    return launch_bf3_px(d, 3, cfg, 2, cps)


def launch_bf3_fused(d, cfg_form):
    TM, WM, WN = {"m64": (1, 2, 2), "m128px64": (1, 4, 1), "m128": (2, 2, 2)}[cfg_form]
    BN = 64 * WN
    pth = BN // 32
    grid = ((d.Wout // 32) * (d.Hout // pth) * d.nimg, 1, 1)
    return _yes("k_conv_bf3", (3, cfg_form, pth, 32, 1, 1, "fused"), grid, 1, 0)


# ------------------------------------------------------------------------------------------------------------------
# K split over the waves: 3x3 / stacked 2x2, 1x1, the map CNN block; the stems
# ------------------------------------------------------------------------------------------------------------------
def bf3_ks_launch(d, cus, mode, tn_pin=0):
    if d.Cin % CB or d.Cin < 8 * CB or d.stats or d.splits > 1:
        return _no("unsupported", "Cin % 16, Cin < 128, statistics or slabs")
    wgs = (d.N // 64) * cdiv(d.M, 32)
    if d.KS == 2:
        if d.grp_imgs > 0 or d.Wout not in (8, 16, 32) or d.Hout % (64 // d.Wout) or d.in_img_stride & 3 or not d.B_al:
            return _no("unsupported", "K-split 2x2: width, rows, alignment")
        if mode == 0 and (wgs > 2 * cus or wgs < cus // 4):
            return _no("unsupported", "grid size")
        pth = 64 // d.Wout
        return _yes("k_conv_bf3_ks", (2, pth, d.Wout, 2), ((d.Hout // pth) * d.nimg, cdiv(d.M, 32), 1), 1, 1)
    if d.Wout not in (8, 16, 32):
        return _no("unsupported", "K-split 3x3: width")
    small = (tn_pin == 1) if tn_pin else 2 * wgs <= cus
    pth = (32 if small else 64) // d.Wout
    if d.Hout % pth or d.in_img_stride & 3 or not d.B_al:
        return _no("unsupported", "K-split 3x3: rows, alignment")
    if d.grp_imgs > 0 and d.nimg % d.grp_imgs:
        return _no("unsupported", "grp_imgs")
    if mode == 0 and (wgs > 2 * cus or wgs < cus // 4):
        return _no("unsupported", "grid size")
    return _yes("k_conv_bf3_ks", (3, pth, d.Wout, 1 if small else 2), ((d.Hout // pth) * d.nimg, cdiv(d.M, 32), 1), 1, 1)


def bf3_1x1_ks_launch(d, cus, mode, form_pin=-1):
    if d.stride != 1 or d.pad != 0 or d.Cin % CB or d.Cin < 4 * CB or d.stats or d.splits > 1:
        return _no("unsupported", "1x1: stride, Cin % 16, Cin < 64, statistics or slabs")
    if d.HoWo & 3 or d.in_img_stride & 3 or not (d.B_al and d.D_al and d.res_al):
        return _no("unsupported", "1x1: HoWo % 4, alignment")
    if d.grp_imgs > 0 and (d.grp_imgs * d.HoWo) % 128:
        return _no("unsupported", "grp_imgs splits a tile")
    nch = d.Cin // CB
    mtiles = cdiv(d.M, 32)
    wt = nch <= 16
    if nch in (24, 32, 48) and cdiv(d.N, 128) * mtiles > 2 * cus:
        wt = True
    if form_pin >= 0:
        wt = form_pin == 1
    if wt and nch > 64:
        wt = False
    if wt and d.accumulate:
        return _no("unsupported", "wave tiles with accumulate")
    wgs = cdiv(d.N, 512) * mtiles if wt else cdiv(d.N, 128) * mtiles
    if mode == 0:
        if not wt and (d.Cin < 32 * CB or wgs > 2 * cus or wgs < cus // 2):
            return _no("unsupported", "grid size")
        if wt and wgs < cus:
            return _no("unsupported", "grid size")
    store = "up2x4" if d.up else ("post" if d.post else "nchw")
    grid = (mtiles, cdiv(d.N, 512 if wt else 128), 1)
    return _yes("k_conv1x1_bf3_ks", ("wt" if wt else "ks", store), grid, 1, 3 if wt else 2)


def bf3_conv7_pool_launch(d):
    if d.KS != 7 or d.up or d.stride != 1 or d.pad != 3 or d.Hout != d.Hin or d.Wout != d.Win:
        return _no("unsupported", "pool2: a same-size 7x7 conv")
    if (d.Hout & 3 or d.Wout & 7 or not (d.has_scale and d.has_shift and d.relu) or d.has_res or d.accumulate or d.post or d.splits > 1 or
            d.stats or d.fuse_M or d.grp_imgs > 0 or d.Cin > 8 * CB):
        return _no("unsupported", "pool2: Hout % 4, Wout % 8, Cin > 128 or an epilogue it has not")
    grid = ((d.Wout // 8) * (d.Hout // 4) * d.nimg, cdiv(d.M, 32), 1)
    if d.u8:
        if d.Cin != 14:
            return _no("unsupported", "pool2: the u8 map form has 14 channels")
        return _yes("k_conv7_pool_bf3", (1, "u8"), grid, 1, 1)
    if d.in_img_stride & 3 or not d.B_al:
        return _no("unsupported", "pool2: alignment")
    nch = cdiv(d.Cin, CB)
    nw = 1 if nch == 1 else (2 if nch == 2 else (4 if nch <= 4 else 8))
    return _yes("k_conv7_pool_bf3", (nw, "f32"), grid, 1, 1)


def bf3_stem_launch(d):
    if d.Cin not in (1, 3) or d.pad != 3 or d.Hin != 2 * d.Hout or d.Win != 2 * d.Wout or d.Wout % 128 or d.up:
        return _no("unsupported", "stem: 1 | 3 channels, Wout % 128")
    if d.grp_imgs > 0 or d.accumulate or d.splits > 1 or d.stats or d.fuse_M:
        return _no("unsupported", "stem: an epilogue it has not")
    if d.in_img_stride & 3 or not (d.B_al and d.D_al and d.res_al):
        return _no("unsupported", "stem: alignment")
    segs = d.Wout // 128
    items = d.nimg * d.Hout * segs * cdiv(d.M, 32)
    p = _yes("k_conv7s2_bf3", (d.Cin, "post" if d.post else "pre"), (cdiv(items, 4), 1, 1), 1, 0)
    p.items = items
    return p


# ------------------------------------------------------------------------------------------------------------------
# ivln_conv_bf3_launch / ivln_wgrad_bf3_launch / ivln_gemm_f32
# ------------------------------------------------------------------------------------------------------------------
def conv_bf3_launch(d, cus, force):
    if not d.A_split:
        return _no("unsupported", "no split weights")
    if d.pool2:
        return bf3_conv7_pool_launch(d)
    KS = d.KS
    if KS not in (1, 2, 3, 7):
        return _no("unsupported", "kernel size")
    if KS == 7 and d.stride == 2:
        return bf3_stem_launch(d)
    up1 = KS == 1 and d.up
    if not up1 and d.up != (KS == 2):
        return _no("unsupported", "destination form")
    ov = d.ov
    if up1:
        if (d.M & 3 or d.Ctot * 4 != d.M or d.grp_imgs > 0 or d.accumulate or d.post or d.splits > 1 or d.stats or d.fuse_M or d.Wout & 3 or
                d.stride != 1 or d.Hout != d.Hin or d.Wout != d.Win):
            return _no("unsupported", "1x1 into 2 x 2 blocks: arguments")
        return bf3_1x1_ks_launch(d, cus, 1 if (force or ov in (11, 12, 13)) else 0, 0 if ov == 12 else (1 if ov == 13 else -1))
    if KS == 2:
        if (d.stride != 1 or d.Hout != d.Hin or d.Wout != d.Win or d.M & 3 or d.grp_imgs > 0 or d.stats or d.splits > 1 or d.fuse_M or d.post or
                d.Wout & 3 or d.Wout < 8 or not (d.D_al and d.res_al) or d.Ctot * 4 != d.M):
            return _no("unsupported", "2x2 window: arguments")
        if ov < 20:
            p = bf3_ks_launch(d, cus, 1 if ov in (10, 15) else 0)
            if p.ok or ov in (10, 15):
                return p

        def blocks2(cfg):
            pth, ptw, imgs = bf3_px(BN_T[cfg], d.Wout)
            return cdiv(d.Wout, ptw) * cdiv(d.Hout, pth) * cdiv(d.nimg, imgs) * cdiv(d.M, BM_T[cfg])

        cfg2 = 3 if blocks2(3) >= cus else (2 if blocks2(2) >= cus else (5 if blocks2(5) >= cus else 4))
        if 20 <= ov < 20 + len(BM_T):
            cfg2 = ov - 20
        if not force and blocks2(cfg2) < cus // 2:
            return _no("unsupported", "grid size")
        d.splits = 1
        return launch_bf3_ks(d, 2, cfg2, cdiv(d.Cin, CB))
    post = d.post
    ins1, ins3 = ov in (11, 12, 13) or post, ov in (10, 14, 15)
    if KS == 1 and ov < 20 and d.splits <= 1 and d.Hout == d.Hin and d.Wout == d.Win:
        p = bf3_1x1_ks_launch(d, cus, 1 if ins1 else 0, 0 if ov == 12 else (1 if ov == 13 else -1))
        if p.ok or ins1:
            return p
    if ins1 or (ins3 and KS != 3):
        return _no("unsupported", "the pinned form does not take this conv")
    if KS == 1:
        if d.stride not in (1, 2) or d.Hout != (d.Hin - 1) // d.stride + 1 or d.Wout != (d.Win - 1) // d.stride + 1 or d.M < 64:
            return _no("unsupported", "tiled 1x1: M < 64")
    elif KS == 3 and d.stride == 2:
        if d.Hin != 2 * d.Hout or d.Win != 2 * d.Wout or d.Cin % CB or d.fuse_M or d.stats:
            return _no("unsupported", "stride-2 3x3: Cin % 16")
    elif d.stride != 1 or d.Hout != d.Hin or d.Wout != d.Win:
        return _no("unsupported", "same-size convs only")
    s2 = KS == 3 and d.stride == 2
    if d.splits > 1 or d.Wout & 3 or d.Wout < 8 or not (d.D_al and d.res_al and d.ws_al):
        return _no("unsupported", "Wout % 4, Wout < 8 or alignment")
    nimg = d.nimg
    if d.fuse_M or d.kind == "fused":
        if (KS != 3 or d.M not in (64, 128) or d.Cin % CB or d.Wout % 32 or d.Hout % 4 or d.fuse_M <= 0 or d.fuse_M % 32 or d.stats or
                d.accumulate or not d.relu):
            return _no("unsupported", "fused tail: arguments")
        if d.grp_imgs > 0 and nimg % d.grp_imgs:
            return _no("unsupported", "grp_imgs")
        wg128 = nimg * (d.Wout // 32) * (d.Hout // 4)
        px64 = d.M == 128 and d.Hout % 2 == 0 and wg128 < cus
        return launch_bf3_fused(d, "m64" if d.M == 64 else ("m128px64" if px64 else "m128"))
    if KS == 3 and not s2 and ov < 20 and d.splits <= 1:
        p = bf3_ks_launch(d, cus, 1 if ins3 else 0, 1 if ov == 14 else (2 if ov == 15 else 0))
        if p.ok or ins3:
            return p
    nch = cdiv(cdiv(d.Cin, CB), stage_chunks(KS))

    def tiles_of(cfg):
        pth, ptw, imgs = bf3_px(BN_T[cfg], d.Wout)
        return cdiv(d.Wout, ptw) * cdiv(d.Hout, pth) * cdiv(nimg, imgs)

    def blocks_of(cfg):
        return tiles_of(cfg) * cdiv(d.M, BM_T[cfg])

    def fills(nb, slots):
        rnd = cus * slots
        return nb * 4 >= cdiv(nb, rnd) * rnd * 3

    big_ok = not (KS == 7 and d.Wout <= 8) and not s2
    if d.M <= 32:
        cfg = 6
    elif d.M <= 64:
        cfg = 1 if (big_ok and KS != 1 and fills(blocks_of(1), 1)) else (2 if fills(blocks_of(2), 1) else (4 if (force or blocks_of(4) >= cus) else -1))
    else:
        cfg = 3 if fills(blocks_of(3), 1) else (2 if fills(blocks_of(2), 1) else (5 if (d.M * d.N >= (1 << 21) and blocks_of(5) >= cus) else 4))
    if cfg < 0:
        return _no("unsupported", "grid size")
    if 20 <= ov < 20 + len(BM_T):
        cfg = ov - 20
    if (cfg == 0 and not big_ok) or (KS == 1 and (cfg <= 1 or cfg == 6)):
        return _no("unsupported", "the tile does not take this kernel size")
    nb = blocks_of(cfg)
    if not force and d.N < 0.15 * tiles_of(cfg) * BN_T[cfg]:
        return _no("unsupported", "tiling uses too few of its pixels")
    splits = 1
    if cfg >= 4:
        slots = 3 if cfg == 4 else 2
        may_split = d.splits == 0 and d.ws and nch >= 2 and not d.stats
        if may_split and nb < cus * slots and not (cfg == 4 and nb >= cus):
            splits = min(cdiv(cus * slots, nb), nch, 16, d.ws_floats // (d.M * d.N))
            splits = max(splits, 1)
        if not force and nb * splits < cus * 3 // 4:
            return _no("unsupported", "grid size")
    elif not force and not fills(nb, 2 if cfg == 6 else 1):
        return _no("unsupported", "grid size")
    cps = cdiv(nch, splits)
    splits = cdiv(nch, cps)
    imgs = bf3_px(BN_T[cfg], d.Wout)[2]
    if d.grp_imgs > 0 and (d.grp_imgs % imgs or nimg % d.grp_imgs):
        return _no("unsupported", "grp_imgs splits a tile")
    d.splits = splits
    stats = d.stats and splits == 1
    p = launch_bf3_ks(d, 7, cfg, cps) if KS == 7 else (launch_bf3_s2(d, cfg, cps) if s2 else launch_bf3_ks(d, KS, cfg, cps))
    if p.ok:
        p.stat_tiles = tiles_of(cfg) * (BN_T[cfg] // 128) if stats else 0
        p.cps = cps
    return p


def kind_parent(d, plan_):
    """THE PARENT'S tally index of a 1x1 launch (ivln_conv_split_kinds), kept as the record of the defect and used by no plan:
    it was worked out beside the launcher from the chunk count (and, NCHW stores only, from tile_override 12 / 13), so a form
    the launcher chose otherwise - wave tiles for 24 / 32 / 48 chunks over more than 2 CUs' worth of tiles, the K-split form
    pinned into the 2 x 2-block stores - was counted as the other one.  Now the launcher reports the form it launched."""
    if plan_.kernel != "k_conv1x1_bf3_ks":
        return plan_.kind
    by_chunks = 3 if d.Cin // CB <= 16 else 2
    if d.up:
        return by_chunks
    return 3 if d.ov == 13 else (2 if d.ov == 12 else by_chunks)


WGRAD_TILE = {"xe": (1, 1, 4), "six": (1, 1, 6), "eight": (1, 1, 8), "64x512": (2, 1, 8), "128x256": (2, 2, 4)}


def wgrad_bf3_launch(d, cus, force):
    if not d.split_ok and not force:
        return _no("unsupported", "not asked for")
    if d.Wout not in (64, 32, 16, 8):
        return _no("unsupported", "wgrad: width")
    ims = 2 if d.Wout == 8 else 1
    rows = 128 // (d.Wout * ims)
    if d.Hout % rows or (d.Wout == 8 and d.Hout != 8) or not d.A_al8:
        return _no("unsupported", "wgrad: rows")
    strips = cdiv(d.nimg, ims) * (d.Hout // rows)
    six = d.M <= 32 and cdiv(d.N, 384) * 384 < cdiv(d.N, 512) * 512
    xe = d.split_ok == 2 and d.M <= 32 and d.Wout == 64
    BM = 32 if d.M <= 32 else (64 if d.M <= 64 else 128)
    BN = 256 if xe else ((384 if six else 512) if d.M <= 32 else (512 if d.M <= 64 else 256))
    blocks = cdiv(d.N, BN) * cdiv(d.M, BM)
    if not d.ws or d.ws_floats < d.M * d.N:
        return _no("unsupported", "wgrad: no workspace")
    if d.splits == 0:
        splits = max(min(max(((3 if xe else 1) * cus) // blocks, 1), strips, d.ws_floats // (d.M * d.N)), 1)
    else:
        splits = min(d.splits, strips)
        if splits > 1 and d.ws_floats < splits * d.M * d.N:
            return _no("invalid", "wgrad: workspace below the forced splits")
    if not force and blocks * splits < cus // 2:
        return _no("unsupported", "grid size")
    sps = cdiv(strips, splits)
    splits = cdiv(strips, sps)
    form = "xe" if xe else (("six" if six else "eight") if d.M <= 32 else ("64x512" if d.M <= 64 else "128x256"))
    TM, WM, WN = WGRAD_TILE[form]
    assert (32 * TM * WM, 64 * WN) == (BM, BN)
    p = _yes("k_wgrad_bf3", (form, d.Wout), (cdiv(d.N, BN), cdiv(d.M, BM), splits), splits, None)
    p.strips, p.sps = strips, sps
    return p


def plan(c, cus=256, form="plain"):
    """ivln_gemm_f32 on a case: a refusal (code, why) or the plan (kernel, key, grid, splits, kind, stat_tiles)"""
    d = desc(c, form)
    if d.M <= 0 or d.N <= 0 or d.K <= 0:
        return _no("invalid", "arguments")
    if d.up and d.M & 3:
        return _no("invalid", "2 x 2 blocks: M % 4")
    if d.grp_imgs > 0 and (d.up or d.kind == "wgrad" or d.nimg % d.grp_imgs):
        return _no("invalid", "grp_imgs")
    if d.post:
        if not d.has_res or d.up or d.fuse_M or d.accumulate:
            return _no("unsupported", "residual_after_relu: arguments")
        return conv_bf3_launch(d, cus, True)
    if d.pool2:
        if d.up or d.fuse_M or d.ov:
            return _no("unsupported", "pool2: arguments")
        return conv_bf3_launch(d, cus, True)
    if d.kind == "fused":
        if d.up:
            return _no("unsupported", "fused tail: arguments")
        return conv_bf3_launch(d, cus, True)
    if d.kind == "wgrad":
        if d.ov not in (0, 9):
            return _no("unsupported", "the pinned form does not take this conv")
        p = wgrad_bf3_launch(d, cus, d.ov == 9)
        return p if (p.ok or p.code != "unsupported" or d.ov == 9) else _no("fp32", "the fp32 kernels")
    if d.ov == 0 or d.ov >= 9:
        p = conv_bf3_launch(d, cus, d.ov >= 9)
        return p if (p.ok or p.code != "unsupported" or d.ov >= 9) else _no("fp32", "the fp32 kernels")
    return _no("fp32", "the fp32 kernels")


# ------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------
def _tiled(KS, cfg, W, stride=1, **kw):
    """the smallest shape with every edge of tile `cfg` at width class W: one tile row + 4 rows (two tile rows, the second
    overhanging), IMGS + 1 images (a ragged image group), BM + 8 channels (a second, masked channel tile)"""
    pth, ptw, imgs = bf3_px(BN_T[cfg], W)
    Cin = {1: 80, 2: 24, 3: 24, 7: 24}[KS] if stride == 1 or KS == 1 else 32
    M = BM_T[cfg] + 8
    tag = "k%d%s-c%d-w%d" % (KS, "s2" if stride == 2 else "", cfg, W)
    c = dict(tag=tag, KS=KS, stride=stride, imgs=imgs + 1, Cin=Cin, H=pth + 4, W=W, M=max(M, 64) if KS == 1 else M, ov=20 + cfg)
    c.update(kw)
    return c


WIDTHS = (8, 12, 36)
TILED_CASES = (
    [_tiled(3, cfg, W) for cfg in range(7) for W in WIDTHS] +
    [_tiled(7, cfg, W) for cfg in range(7) for W in WIDTHS if not (cfg in (0, 1) and W == 8)] +
    [_tiled(1, cfg, W) for cfg in (2, 3, 4, 5) for W in WIDTHS] +
    [_tiled(1, cfg, W, stride=2) for cfg in (2, 3, 4, 5) for W in WIDTHS] +
    [_tiled(2, cfg, W) for cfg in (2, 3, 4, 5) for W in WIDTHS] +
    [_tiled(3, cfg, W, stride=2) for cfg in (2, 3, 4, 5, 6) for W in WIDTHS]
)
# slabs over blockIdx.z: three 16-channel chunks (the last one of 8 channels) = three slabs of one chunk each, reduced by
# k_splitk_epilogue4, or with no_wide_epilogue by k_splitk_epilogue
SLAB_CASES = [dict(_tiled(3, cfg, 12, ws=True), tag="slab-c%d%s" % (cfg, "-nwe" if nwe else ""), Cin=40, nwe=nwe)
              for cfg in (4, 5, 6) for nwe in (False, True)]
# per-tile statistics (stride-1 3x3 / 7x7, one slab), image-grouped weights, D +=
EXTRA_TILED = [
    dict(_tiled(3, 2, 12), tag="stats-k3-c2-w12", stats=True),
    dict(_tiled(3, 0, 36), tag="stats-k3-c0-w36", stats=True),
    dict(_tiled(7, 4, 8), tag="stats-k7-c4-w8", stats=True),
    dict(_tiled(3, 2, 8), tag="grp-k3-c2-w8", imgs=8, grp=4),
    dict(_tiled(1, 4, 12), tag="grp-k1-c4-w12", imgs=4, grp=2),
    dict(_tiled(3, 4, 12), tag="acc-k3-c4-w12", acc=True),
    dict(_tiled(3, 5, 12, ws=True), tag="acc-slab-c5", Cin=40, acc=True),
]
# the fused bottleneck tail: M = 64; M = 128 on 64-pixel tiles (wg128 < CUs: 4 x 16 x 128 x 64 is 256 workgroups of 128 pixels -
# the case is sized from the CU count, `cus`, below) and on 128-pixel tiles
def fused_cases(cus):
    big = max(1, cdiv(cus, 64))   # images of a 128 x 64 map (64 workgroups of 128 pixels each): wg128 >= cus
    return [
        dict(tag="fuse-m64", kind="fused", KS=3, imgs=2, Cin=16, H=8, W=32, M=64, fuse_M=96),
        dict(tag="fuse-m64-grp", kind="fused", KS=3, imgs=2, Cin=32, H=4, W=64, M=64, fuse_M=96, grp=1),
        dict(tag="fuse-m128-px64", kind="fused", KS=3, imgs=2, Cin=16, H=8, W=32, M=128, fuse_M=96),
        dict(tag="fuse-m128-px64-grp", kind="fused", KS=3, imgs=2, Cin=32, H=4, W=32, M=128, fuse_M=96, grp=1),
        dict(tag="fuse-m128", kind="fused", KS=3, imgs=big, Cin=16, H=128, W=64, M=128, fuse_M=96, cus=cus),
    ]


# k_conv_bf3_ks: the six stride-1 tiles (14 / 15 x three widths), Cin = 128 and 144 (8 and 9 chunks over 8 waves), M = 40
KS_CASES = (
    [dict(tag="ks%d-w%d" % (ov, W), KS=3, imgs=3, Cin=128 if ov == 14 else 144, H=2 * ((32 if ov == 14 else 64) // W), W=W, M=40, ov=ov)
     for ov in (14, 15) for W in (8, 16, 32)] +
    [dict(tag="ks15-w16-c128", KS=3, imgs=2, Cin=128, H=8, W=16, M=40, ov=15),
     dict(tag="ks14-w16-c144", KS=3, imgs=2, Cin=144, H=4, W=16, M=40, ov=14),
     dict(tag="ks14-w8-grp", KS=3, imgs=4, Cin=128, H=8, W=8, M=40, ov=14, grp=2),
     dict(tag="ks15-w8-acc", KS=3, imgs=4, Cin=128, H=8, W=8, M=40, ov=15, acc=True)] +
    [dict(tag="ks2-w%d" % W, KS=2, imgs=3, Cin=128 if W != 16 else 144, H=2 * (64 // W), W=W, M=40, ov=10) for W in (8, 16, 32)]
)
# k_conv1x1_bf3_ks: both forms x the store forms; nch = 4, 9, 17; N = 540 or 300 pixels (no multiple of 128 or 512), M = 40
X1_CASES = (
    [dict(tag="x1-%d-nch%d" % (ov, nch), KS=1, imgs=9, Cin=16 * nch, H=6, W=10, M=40, ov=ov) for ov in (12, 13) for nch in (4, 9, 17)] +
    [dict(tag="x1-%d-post" % ov, KS=1, imgs=9, Cin=144, H=6, W=10, M=40, ov=ov, post=True) for ov in (12, 13)] +
    [dict(tag="x1-%d-up" % ov, KS=1, imgs=9, Cin=80, H=6, W=12, M=40, ov=ov, up=True) for ov in (12, 13)] +
    [dict(tag="x1-12-acc", KS=1, imgs=9, Cin=272, H=6, W=10, M=40, ov=12, acc=True),
     dict(tag="x1-12-grp", KS=1, imgs=8, Cin=64, H=8, W=16, M=40, ov=12, grp=4),
     dict(tag="x1-13-grp", KS=1, imgs=8, Cin=64, H=8, W=16, M=40, ov=13, grp=4)]
)
# k_conv7_pool_bf3: NW = 1, 2, 4, 8 by chunk count, the u8 map form; 4 x 8 (one tile) and 12 x 16 (six) maps, M = 40
POOL_CASES = (
    [dict(tag="pool-nw%d-%dx%d" % (nw, H, W), kind="pool", KS=7, imgs=2, Cin=cin, H=H, W=W, M=40)
     for nw, cin in ((1, 14), (2, 24), (4, 40), (8, 72)) for H, W in ((4, 8), (12, 16))] +
    [dict(tag="pool-u8-%dx%d" % (H, W), kind="pool", KS=7, imgs=2, Cin=14, H=H, W=W, M=40, u8=True) for H, W in ((4, 8), (12, 16))]
)
# k_conv7s2_bf3: 1 x 3 rows x 1 segment x 2 channel tiles = 6 items, four per workgroup: the last holds two
STEM_CASES = [dict(tag="stem-c%d%s" % (cin, "-post" if post else ""), KS=7, stride=2, imgs=1, Cin=cin, H=3, W=128, M=40, post=post, ov=0 if post else 9)
              for cin in (1, 3) for post in (False, True)]
# k_wgrad_bf3: the five launch forms x the widths; width 8: 3 images (a ragged image pair); forced splits 1 and 3
def _wgrad_cases():
    out = []
    for fi, (form, M, Cin) in enumerate((("six", 20, 14), ("eight", 20, 8), ("64x512", 48, 14), ("128x256", 72, 8))):
        for wi, W in enumerate((64, 32, 16, 8)):
            rows = 128 // (W * (2 if W == 8 else 1))
            if W == 8:     # 8 x 8 maps, two per strip: 3 images (the second pair holds one), or 9 in five strips over three slabs
                imgs, H, splits = (9, 8, 3) if fi == 0 else (3, 8, 1)
            elif (fi + wi) % 2 == 0:   # five strips forced over three slabs: two, two and one
                imgs, H, splits = 1, 5 * rows, 3
            else:
                imgs, H, splits = 2, 2 * rows, 1
            out.append(dict(tag="wg-%s-w%d" % (form, W), kind="wgrad", imgs=imgs, Cin=Cin, H=H, W=W, M=M, ov=9, splits=splits))
    out.append(dict(tag="wg-xe-w64", kind="wgrad", imgs=1, Cin=14, H=10, W=64, M=20, ov=9, splits=3, split_ok=2))
    return out


WGRAD_CASES = _wgrad_cases()


def launch_cases(cus=256):
    """every case the GPU file launches and checks against float64 (the fused tail's big case sized for `cus`)"""
    return TILED_CASES + SLAB_CASES + EXTRA_TILED + fused_cases(cus) + KS_CASES + X1_CASES + POOL_CASES + STEM_CASES + WGRAD_CASES


# One shape just inside (why None) and one just outside each refusal reason; `why` as the restatement words it.
_K3 = dict(KS=3, imgs=2, Cin=24, H=12, W=12, M=40, ov=24)
_KS3 = dict(KS=3, imgs=2, Cin=128, H=8, W=8, M=40, ov=15)
_X1 = dict(KS=1, imgs=2, Cin=64, H=8, W=8, M=40, ov=12)
_POOL = dict(kind="pool", KS=7, imgs=1, Cin=24, H=4, W=8, M=40)
_STEM = dict(KS=7, stride=2, imgs=1, Cin=3, H=2, W=128, M=40, ov=9)
_WG = dict(kind="wgrad", imgs=2, Cin=8, H=8, W=16, M=20, ov=9, splits=1)
REFUSALS = [
    dict(_K3, tag="wout4-in", why=None),
    dict(_K3, tag="wout4-out", W=10, why="Wout % 4, Wout < 8 or alignment"),
    dict(_K3, tag="wout8-in", W=8, why=None),
    dict(_K3, tag="wout8-out", W=4, why="Wout % 4, Wout < 8 or alignment"),
    dict(_KS3, tag="misB-in", why=None),
    dict(_KS3, tag="misB-out", misB=True, why="K-split 3x3: rows, alignment"),
    dict(_K3, tag="s2-cin-in", stride=2, Cin=32, why=None),
    dict(_K3, tag="s2-cin-out", stride=2, Cin=24, why="stride-2 3x3: Cin % 16"),
    dict(_KS3, tag="ks-cin-in", Cin=144, why=None),
    dict(_KS3, tag="ks-cin-out", Cin=136, why="Cin % 16, Cin < 128, statistics or slabs"),
    dict(_X1, tag="x1-cin-in", why=None),
    dict(_X1, tag="x1-cin-out", Cin=72, why="1x1: stride, Cin % 16, Cin < 64, statistics or slabs"),
    dict(_K3, tag="m64-in", KS=1, Cin=80, M=64, why=None),
    dict(_K3, tag="m64-out", KS=1, Cin=80, M=63, why="tiled 1x1: M < 64"),
    dict(_K3, tag="grp-in", W=8, imgs=4, ov=24, grp=2, why=None),       # 64 x 128 on 8-wide maps: two images per tile
    dict(_K3, tag="grp-out", W=8, imgs=3, ov=24, grp=1, why="grp_imgs splits a tile"),
    dict(_X1, tag="wt-acc-in", ov=12, acc=True, why=None),
    dict(_X1, tag="wt-acc-out", ov=13, acc=True, why="wave tiles with accumulate"),
    dict(_POOL, tag="pool-h4-in", why=None),
    dict(_POOL, tag="pool-h4-out", H=6, why="pool2: Hout % 4, Wout % 8, Cin > 128 or an epilogue it has not"),
    dict(_POOL, tag="pool-w8-out", W=12, why="pool2: Hout % 4, Wout % 8, Cin > 128 or an epilogue it has not"),
    dict(_POOL, tag="pool-cin-in", Cin=128, why=None),
    dict(_POOL, tag="pool-cin-out", Cin=129, why="pool2: Hout % 4, Wout % 8, Cin > 128 or an epilogue it has not"),
    dict(_STEM, tag="stem-w-in", why=None),
    dict(_STEM, tag="stem-w-out", W=64, why="stem: 1 | 3 channels, Wout % 128"),
    dict(_WG, tag="wg-w-in", why=None),
    dict(_WG, tag="wg-w-out", W=24, H=16, why="wgrad: width"),
    dict(_WG, tag="wg-ws-out", no_ws=True, why="wgrad: no workspace"),
]


# ------------------------------------------------------------------------------------------------------------------
# what each tag claims
# ------------------------------------------------------------------------------------------------------------------
def tile_edges(c, p):
    """the ragged edges of a tiled plan, from the case and its instantiation key"""
    _, KS, cfg, pth, ptw, imgs, ST, _ = p.key
    chunks = cdiv(c["Cin"], CB)
    return dict(
        tiles_h=cdiv(c["H"], pth), over_h=c["H"] % pth != 0, tiles_w=cdiv(c["W"], ptw), over_w=c["W"] % ptw != 0,
        groups=cdiv(c["imgs"], imgs), ragged_group=c["imgs"] % imgs != 0, m_tiles=p.grid[1], masked_m=c["M"] % BM_T[cfg] != 0,
        ragged_chunk=c["Cin"] % CB != 0, chunks=chunks, ragged_stage=chunks % stage_chunks(KS) != 0, stages=cdiv(chunks, stage_chunks(KS)))


def _find(tag, cus=256):
    return next(c for c in launch_cases(cus) if c["tag"] == tag)


def test_tile_tables_are_the_sources():
    """kBf3BM / kBf3BN / CB / PIXB / bf3_taps_padded as the sources have them; launch_bf3_px's pixel tiles = bf3_px's"""
    assert BM_T == [32 * tm * wm for tm, wm, _ in TILE] and BN_T == [64 * wn for _, _, wn in TILE]
    assert BM_T == [32, 64, 64, 128, 64, 128, 32] and BN_T == [512, 512, 256, 256, 128, 128, 256]
    assert (CB, PIXB) == (16, 112)
    m = re.search(r"bf3_taps_padded\(int KS\) \{ return KS == 7 \? (\d+) : \(KS == 3 \? (\d+) : \(KS == 2 \? (\d+) : (\d+)\)\); \}", _COMMON)
    assert [int(v) for v in m.groups()] == [taps_padded(k) for k in (7, 3, 2, 1)]
    for BN, rows in PX_TABLE.items():
        for W, px in zip((36, 12, 8), rows):
            assert bf3_px(BN, W) == px and px[0] * px[1] * px[2] == BN
    # the launch table in the source: `case c: return launch_bf3_px<KS, TM, WM, WN, ...>` of launch_bf3_ks
    body = _BF3[_BF3.index("int launch_bf3_ks("):_BF3.index("int launch_bf3_s2(")]
    body = body[body.index("switch (cfg) {", body.index("default: return IVLN_E_UNSUPPORTED")):]
    got = [tuple(int(v) for v in m) for m in re.findall(r"launch_bf3_px<KS, (\d), (\d), (\d), DA\d>", body)]
    assert got == TILE


def test_every_case_reaches_the_edges_its_tag_names():
    cases = launch_cases()
    assert len({c["tag"] for c in cases}) == len(cases)
    for c in TILED_CASES:
        for form in FORMS:
            p = plan(c, 256, form)
            assert p.ok, (c["tag"], p.why)
        e = tile_edges(c, p)
        KS, cfg, W = c["KS"], p.key[2], c["W"]
        assert p.kernel == "k_conv_bf3" and p.key[2] == c["ov"] - 20 and p.splits == 1 and p.kind == 0
        # two tile rows, the second overhanging; a second, ragged image group (8-wide maps aside: one image per 32-wide tile);
        # a second channel tile, masked; width 12 and 36 overhang their 16- / 32-pixel columns, 36 in a second tile column
        # (4-row tiles - 128 pixels on maps wider than 16 - end on the map's last row: one tile row + 4 is two whole ones)
        assert e["tiles_h"] == 2 and e["over_h"] == (p.key[3] != 4) and e["groups"] == 2 and e["m_tiles"] == 2 and e["masked_m"], (c["tag"], e)
        assert e["ragged_group"] == (p.key[5] > 1)
        assert (e["tiles_w"], e["over_w"]) == {8: (1, False), 12: (1, True), 36: (2, True)}[W]
        if KS == 1:   # five chunks: a full stage of four and a stage with one
            assert e["chunks"] == 5 and e["stages"] == 2 and e["ragged_stage"] and c["M"] >= 64
        elif c.get("stride", 1) == 2:
            assert not e["ragged_chunk"] and e["chunks"] == 2 and p.lds <= LDS_MAX
        else:         # 24 channels: a full chunk and a short one
            assert e["ragged_chunk"] and e["chunks"] == 2
    for c in SLAB_CASES:
        for cus in (64, 256, 304):
            p = plan(c, cus)
            assert p.ok and p.splits == 3 and p.grid[2] == 3 and p.cps == 1 and tile_edges(c, p)["ragged_chunk"], (c["tag"], vars(p))
    for c in EXTRA_TILED:
        p = plan(c)
        assert p.ok and (p.stat_tiles > 0) == bool(c.get("stats")), c["tag"]
        if c.get("stats"):
            _, KS, cfg, pth, ptw, imgs, ST, _ = p.key
            assert p.stat_tiles == p.grid[0] * (BN_T[cfg] // 128) and p.grid[0] >= 4
    assert plan(_find("acc-slab-c5")).splits == 3
    for cus in (64, 256, 304):
        f = {c["tag"]: plan(c, cus) for c in fused_cases(cus)}
        assert [f[t].key[2] for t in ("fuse-m64", "fuse-m64-grp", "fuse-m128-px64", "fuse-m128-px64-grp", "fuse-m128")] == \
            ["m64", "m64", "m128px64", "m128px64", "m128"], cus
    assert _find("fuse-m128")["imgs"] == 4   # 4 x 16 x 128 x 64 at 256 CUs: 256 workgroups of 128 pixels
    for c in KS_CASES:
        p = plan(c)
        assert p.ok and p.kernel == "k_conv_bf3_ks" and p.kind == 1 and p.grid[1] == 2 and c["M"] % 32, c["tag"]
        assert p.grid[0] >= 4 and c["Cin"] in (128, 144)
    for c in X1_CASES:
        p = plan(c)
        assert p.ok and p.kernel == "k_conv1x1_bf3_ks" and p.key[1] == ("ks" if c["ov"] == 12 else "wt"), c["tag"]
        n = c["imgs"] * c["H"] * c["W"]
        assert p.grid[1] >= 2 and p.grid[0] == 2 and (n % 128 and n % 512 or c.get("grp")) and (c["H"] * c["W"]) % 4 == 0
        assert p.kind == (2 if c["ov"] == 12 else 3)
    assert {c["Cin"] // CB for c in X1_CASES} >= {4, 9, 17}
    for c in POOL_CASES:
        p = plan(c)
        assert p.ok and p.key[1] == (1 if c.get("u8") else {14: 1, 24: 2, 40: 4, 72: 8}[c["Cin"]]) and p.grid[0] in (2, 12) and p.grid[1] == 2
    for c in STEM_CASES:
        p = plan(c)
        assert p.ok and p.items == 6 and p.grid[0] == 2 and p.items % 4 == 2 and p.key[2] == ("post" if c["post"] else "pre")
    for c in WGRAD_CASES:
        p = plan(c)
        assert p.ok and p.key[1] == c["tag"].split("-")[1] and p.key[2] == c["W"] and p.splits == c["splits"], (c["tag"], vars(p))
        if c["splits"] == 3:   # a ragged last slab of strips
            assert p.strips == 5 and p.sps == 2 and p.grid[2] == 3
        if c["W"] == 8:        # a ragged image pair
            assert c["imgs"] % 2 == 1 and p.strips == (c["imgs"] + 1) // 2
    assert {c["W"] for c in WGRAD_CASES} == {64, 32, 16, 8}


def test_1x1_tally_names_the_form_launched_and_the_parents_did_not():
    """the defect x1-12-up exposed, and its reach: the kernel, grid and splits of every plan are what they were - only the
    counter a 1x1 launch lands in moved, for the shapes below"""
    moved = []
    for c in launch_cases():
        p = plan(c)
        if kind_parent(desc(c), p) != p.kind:
            moved.append(c["tag"])
    assert moved == ["x1-12-up"]   # five chunks pinned to the K-split form: counted as wave tiles
    # production (heuristic dispatch, 256 CUs): RedNet layer 3's first reduction at 8 + 8 images, 256 x 16384 x 512 - 32 chunks
    # over 1024 tiles - runs as wave tiles and was counted as K-split; 256 x 4096 x 1024 (64 chunks) is K-split under both rules
    big = dict(KS=1, imgs=16, Cin=512, H=32, W=32, M=256)
    p = plan(big)
    assert p.ok and p.key[1] == "wt" and p.kind == 3 and kind_parent(desc(big), p) == 2
    deep = dict(KS=1, imgs=16, Cin=1024, H=16, W=16, M=256)
    p = plan(deep)
    assert p.ok and p.key[1] == "ks" and p.kind == 2 and kind_parent(desc(deep), p) == 2


def test_refusal_shapes_sit_on_either_side_of_each_reason():
    whys = set()
    for c in REFUSALS:
        for form in (("plain",) if c.get("kind") in ("pool", "wgrad") else FORMS):
            p = plan(c, 256, form)
            assert p.ok == (c["why"] is None), (c["tag"], form, vars(p))
            if not p.ok:
                assert p.code == "unsupported" and p.why == c["why"], (c["tag"], p.why)
                whys.add(p.why)
    assert len(whys) >= 11


# ------------------------------------------------------------------------------------------------------------------
# the coverage pin
# ------------------------------------------------------------------------------------------------------------------
def reachable_keys(cus=256):
    """every instantiation key the restated launchers produce over their accepted domain: a grid of descriptors over kernel
    size, stride, every tile_override, the three width classes, channel counts on both sides of every threshold and every
    epilogue switch that selects a kernel"""
    keys = set()
    for KS, stride, ov, W, up, post in itertools.product((1, 2, 3, 7), (1, 2), (0, 9, 10, 11, 12, 13, 14, 15) + tuple(range(20, 27)), (8, 12, 16, 32, 36, 128),
                                                          (False, True), (False, True)):
        for Cin, M in ((1, 40), (3, 40), (24, 40), (32, 40), (80, 72), (144, 40), (144, 136), (1040, 40)):
            c = dict(KS=KS, stride=stride, imgs=3, Cin=Cin, H=16, W=W, M=M, ov=ov, up=up, post=post)
            p = plan(c, cus)
            if p.ok:
                keys.add(p.key)
    for M, px in ((64, 1), (128, 1), (128, 64)):
        p = plan(dict(kind="fused", KS=3, imgs=px, Cin=16, H=64, W=32, M=M, fuse_M=96), cus)
        keys.add(p.key)
    for Cin, u8 in ((14, False), (24, False), (40, False), (72, False), (14, True)):
        keys.add(plan(dict(kind="pool", KS=7, imgs=1, Cin=Cin, H=4, W=8, M=40, u8=u8), cus).key)
    for M, Cin, W, ok in itertools.product((20, 48, 72), (8, 14), (64, 32, 16, 8), (1, 2)):
        keys.add(plan(dict(kind="wgrad", imgs=2, Cin=Cin, H=8, W=W, M=M, ov=9, splits=1, split_ok=ok), cus).key)
    return keys


def case_keys(cases):
    out = set()
    for c in cases:
        p = plan(c, c.get("cus", 256))
        assert p.ok, c["tag"]
        out.add(p.key)
    return out


def test_cases_cover_every_instantiation_the_plans_can_produce():
    want, got = reachable_keys(), case_keys(launch_cases())
    assert got == want, (sorted(want - got, key=str), sorted(got - want, key=str))
    # every kernel of the family that conv_bf3.hip defines has a case
    defined = set(re.findall(r"__global__ __launch_bounds__\([^)]*\)\s*void (\w+)\(", _BF3))
    here = [k for k in family_kernels() if k in defined]
    assert sorted(here) == ["k_conv1x1_bf3_ks", "k_conv7_pool_bf3", "k_conv7s2_bf3", "k_conv_bf3", "k_conv_bf3_ks", "k_wgrad_bf3"]
    assert {k[0] for k in got} == set(here)
    # ... and the pin notices a removed case: any single tiled case gone leaves its instantiation without one
    for drop in ("k3-c0-w8", "k7-c6-w36", "k1s2-c3-w12", "k2-c5-w8", "k3s2-c6-w12"):
        fewer = [c for c in launch_cases() if c["tag"] != drop]
        assert len(fewer) == len(launch_cases()) - 1 and case_keys(fewer) != want, drop
    assert len([k for k in want if k[0] == "k_conv_bf3" and k[-1].startswith("tile")]) == 21 + 19 + 24 + 12 + 15


# ------------------------------------------------------------------------------------------------------------------
# what ran before this file: the shapes of tests/test_gpu_kernels.py under the restated dispatch
# ------------------------------------------------------------------------------------------------------------------
def prior_keys(cus=256):
    """The instantiation keys the split-bf16 shapes of tests/test_gpu_kernels.py reach (its parametrize lists, transcribed, with
    the tile_override each test sets and ops.conv2d's 2^18-output gate for the default dispatch; both with and without a
    workspace where the test does both).  Where 20 + c is not pinned there the tile is the heuristic's: the count depends on
    the CU count."""
    keys = set()

    def add(**c):
        for ws in c.pop("wss", (False, True)):
            cc = dict(c, ws=ws)
            if cc.get("kind") == "wgrad":
                cc.pop("ws")
            p = plan(cc, cus, "plain")
            if p.ok:
                keys.add(p.key)

    def gate(ov, outs):
        return ov >= 9 or outs >= (1 << 18)

    # test_conv2d_split_bf16_kernel (override 9), accuracy / one-hot / specials / grouped + stats
    for N, Cin, H, W, M, k in [(6,14,64,64,32,7),(4,32,32,32,64,7),(5,64,16,16,128,7),(9,128,8,8,128,7),(3,64,32,32,32,7),(2,64,128,128,64,3),
                               (3,48,40,24,70,3),(16,256,8,8,40,3),(2,16,16,48,256,3),(4,64,32,32,64,3),(16,16,32,32,32,3),(8,64,64,64,64,3),(4,64,64,64,64,3)]:
        add(KS=k, imgs=N, Cin=Cin, H=H, W=W, M=M, ov=9)
    add(KS=3, imgs=8, Cin=64, H=64, W=64, M=64, ov=9, grp=4, wss=(False,))
    add(KS=3, imgs=8, Cin=64, H=64, W=64, M=64, ov=9, stats=True, wss=(True,))
    # stems (override 0), residual in front of and behind the ReLU
    for N, Cin, H, W, M in [(8,3,256,256,64),(8,1,256,256,64),(2,3,12,512,48),(3,1,6,256,72),(1,3,2,256,32)]:
        for post in (False, True):
            add(KS=7, stride=2, imgs=N, Cin=Cin, H=H//2, W=W//2, M=M, ov=0, post=post)
    # stride-2 3x3: override 9, 22 ... 26, default at N == 16
    for N, Cin, H, W, M, G in [(16,128,64,64,128,2),(16,256,32,32,256,2),(16,512,16,16,512,2),(3,48,24,40,40,0),(2,32,16,16,24,0)]:
        g = dict(grp=N // G) if G else {}
        add(KS=3, stride=2, imgs=N, Cin=Cin, H=H//2, W=W//2, M=M, ov=9, **g)
        for ov in (22,23,24,25,26):
            if (ov in (23,25) and M < 128) or (G and N // G * (H//2) * (W//2) % (256 if ov in (22,23,26) else 128)):
                continue
            add(KS=3, stride=2, imgs=N, Cin=Cin, H=H//2, W=W//2, M=M, ov=ov, wss=(False,), **g)
        if N == 16:
            add(KS=3, stride=2, imgs=N, Cin=Cin, H=H//2, W=W//2, M=M, ov=0, **g)
    # residual behind the ReLU (default dispatch insists), then the pinned form
    for N, Cin, M, H, W, form in [(2,64,64,32,32,13),(2,256,64,16,16,13),(2,512,128,8,16,12),(1,1024,256,8,8,12),(3,80,40,4,8,13)]:
        add(KS=1, imgs=N, Cin=Cin, H=H, W=W, M=M, ov=0, post=True, wss=(False,))
        add(KS=1, imgs=N, Cin=Cin, H=H, W=W, M=M, ov=form)
    # fused tail + the two-launch path it is compared with (default dispatch)
    for N, Cin, Cmid, M, H, W, G in [(2,64,64,256,32,32,0),(2,128,128,512,8,32,0),(4,64,64,256,16,64,2),(3,48,64,96,4,32,0),(2,128,128,512,32,32,2),(32,128,128,256,32,32,2)]:
        g = dict(grp=N // G) if G else {}
        add(kind="fused", KS=3, imgs=N, Cin=Cin, H=H, W=W, M=Cmid, fuse_M=M, wss=(False,), **g)
        if gate(0, N*H*W*Cmid): add(KS=3, imgs=N, Cin=Cin, H=H, W=W, M=Cmid, ov=0, **g)
        if gate(0, N*H*W*M): add(KS=1, imgs=N, Cin=Cmid, H=H, W=W, M=M, ov=0, **g)
    # k_conv_bf3_ks (override 10)
    for N, Cin, H, M, G in [(8,512,8,512,0),(8,256,16,256,0),(4,128,32,128,0),(16,256,16,256,2),(3,144,8,96,0),(2,128,16,40,0),(1,128,32,64,0),(32,128,8,256,0)]:
        g = dict(grp=N // G) if G else {}
        add(KS=3, imgs=N, Cin=Cin, H=H, W=H, M=M, ov=10, **g)
    # k_conv1x1_bf3_ks (override 11)
    for N, Cin, H, M, G in [(8,1024,16,256,0),(16,2048,8,512,2),(3,528,8,40,0),(5,512,4,96,0),(2,512,32,128,0),(4,64,64,256,0),(8,128,32,512,2),(4,256,16,1024,0),(3,80,8,40,0),(2,64,16,64,0)]:
        g = dict(grp=N // G) if G else {}
        add(KS=1, imgs=N, Cin=Cin, H=H, W=H, M=M, ov=11, **g)
    # the tiled 1x1 form (override 9)
    for N, Cin, H, M, s in [(16,256,16,1024,1),(8,200,32,128,1),(4,128,64,512,2),(16,2048,8,64,1)]:
        add(KS=1, stride=s, imgs=N, Cin=Cin, H=H//s, W=H//s, M=M, ov=9)
    # stride-2 1x1 through the gather (a stride-1 1x1 at half size) and strided, default dispatch
    for N, Cin, H, M, G in [(16,256,64,512,2),(16,512,32,1024,2),(16,1024,16,2048,2),(3,64,16,96,0)]:
        g = dict(grp=N // G) if G else {}
        if gate(0, N*(H//2)**2*M):
            add(KS=1, imgs=N, Cin=Cin, H=H//2, W=H//2, M=M, ov=0, **g)
            add(KS=1, stride=2, imgs=N, Cin=Cin, H=H//2, W=H//2, M=M, ov=0, **g)
    # weight gradient (override 9, the launcher's own split count), the one-piece form
    for N, Cin, H, M in [(6,14,64,32),(8,32,32,64),(16,64,16,128),(33,128,8,128),(5,20,16,70)]:
        add(kind="wgrad", imgs=N, Cin=Cin, H=H, W=H, M=M, ov=9, splits=0)
    for N, Cin, M in [(6,14,32),(64,14,32),(5,9,20)]:
        for ok, ov in ((2, 9), (1, 9), (2, 0)):
            add(kind="wgrad", imgs=N, Cin=Cin, H=64, W=64, M=M, ov=ov, splits=0, split_ok=ok)
    # stacked transposed-conv classes: 2x2 window (10 | 9, 24, default at N == 8), one tap (12 | 13)
    for N, Cin, H, C, form in [(8,512,8,256,"ks"),(8,256,16,128,"ks"),(8,128,32,64,"tiled"),(8,64,64,64,"tiled"),(3,128,16,24,"ks"),(2,48,32,40,"tiled")]:
        add(KS=2, imgs=N, Cin=Cin, H=H, W=H, M=4*C, ov=10 if form == "ks" else 9)
        if form == "tiled": add(KS=2, imgs=N, Cin=Cin, H=H, W=H, M=4*C, ov=24)
        if N == 8: add(KS=2, imgs=N, Cin=Cin, H=H, W=H, M=4*C, ov=0)
    for N, Cin, H, C, form in [(8,512,8,256,12),(8,256,16,128,13),(8,128,32,64,13),(8,64,64,64,13),(8,64,128,13,13),(3,96,8,20,13),(2,512,16,24,12)]:
        add(KS=1, imgs=N, Cin=Cin, H=H, W=H, M=4*C, ov=form, up=True)
        add(KS=1, imgs=N, Cin=Cin, H=H, W=H, M=4*C, ov=0, up=True)
    return keys


def test_most_instantiations_had_no_case_before():
    """at 256 CUs the workload-shaped tests reach 58 of the 135 instantiation keys: 77 had no case (60 of the tiled kernel's 94,
    1 of k_conv_bf3_ks' 9, 11 of k_wgrad_bf3's 17; k_conv7_pool_bf3's 5 run in tests/test_gpu_map_cnn_infer.py only)"""
    want, before = reachable_keys(256), prior_keys(256)
    assert before <= want
    by = {k: (len([x for x in before if x[0] == k]), len([x for x in want if x[0] == k])) for k in {x[0] for x in want}}
    assert by == {"k_conv_bf3": (34, 94), "k_conv_bf3_ks": (8, 9), "k_conv1x1_bf3_ks": (6, 6), "k_conv7_pool_bf3": (0, 5),
                  "k_conv7s2_bf3": (4, 4), "k_wgrad_bf3": (6, 17)}
    assert len(want) - len(before) == 77


# ------------------------------------------------------------------------------------------------------------------
# the arithmetic
# ------------------------------------------------------------------------------------------------------------------
def _bf16_rne(x):
    """fp32 array -> the fp32 value of its nearest bf16 (ties to even); finite inputs"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    hb = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return hb.view(np.float32)


def split3_np(x):
    """bf3_common.h's split3: x = h + m + l, each a bf16 value (as fp32), remainders computed in fp32 (exact)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    h = _bf16_rne(x)
    r = (x - h).astype(np.float32)
    m = _bf16_rne(r)
    r2 = (r - m).astype(np.float32)
    return h, m, _bf16_rne(r2)


SIX = ((0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0))   # (weight piece, input piece) in the ladder's issue order


def piece_product_conv(x, w, products=SIX, **conv):
    """the conv as the kernels compute it: per piece product the exact conv (float64), the accumulator rounded to fp32 after each"""
    xs = [torch.from_numpy(p).double() for p in split3_np(x.numpy())]
    ws = [torch.from_numpy(p).double() for p in split3_np(w.numpy())]
    acc = None
    for a, b in products:
        t = F.conv2d(xs[b], ws[a], **conv)
        acc = t.float() if acc is None else (acc.double() + t).float()
    return acc


def inputs(name, imgs, Cin, H, W, M, KS, seed):
    """the two input sets of every case: `dense`, and `single_tap` (one non-zero weight per output channel, its channel and
    tap varying with the output channel; the input dense, not bf16-exact)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(imgs, Cin, H, W, generator=g)
    w = torch.randn(M, Cin, KS, KS, generator=g)
    if name == "dense":
        return x, w / (Cin * KS * KS) ** 0.5
    assert name == "single_tap"
    keep = torch.zeros_like(w)
    m = torch.arange(M)
    ci, tap = (m * 5 + 3) % Cin, (m * 7 + 1) % (KS * KS)
    keep[m, ci, tap // KS, tap % KS] = 1.0
    return x, w * keep + keep * 0.5 * torch.sign(w)   # (|w| >= 0.5: no product vanishes)


def bar_of(ref64, ref32):
    e32 = float((ref32.double() - ref64).abs().max())
    return 4 * e32 + 4 * 2.0 ** -24 * float(ref64.abs().max())


ARITH_SHAPES = [(3, 24, 12, 8, 40, 3), (2, 24, 20, 12, 72, 7), (2, 80, 8, 8, 72, 1)]   # imgs Cin H W M KS


@pytest.mark.parametrize("imgs,Cin,H,W,M,KS", ARITH_SHAPES)
def test_six_products_stay_inside_the_bar_and_no_five_do(imgs, Cin, H, W, M, KS):
    conv = dict(padding=KS // 2)
    for name in ("dense", "single_tap"):
        x, w = inputs(name, imgs, Cin, H, W, M, KS, 11 * KS + M)
        ref64, ref32 = F.conv2d(x.double(), w.double(), **conv), F.conv2d(x, w, **conv)
        bar = bar_of(ref64, ref32)
        err6 = float((piece_product_conv(x, w, SIX, **conv).double() - ref64).abs().max())
        assert err6 <= bar, (name, err6, bar)
        assert err6 <= 0.5 * bar   # (measured: 4.9e-7 ... 7.0e-7 against 2.0e-6 ... 2.2e-6 on `dense`)
        if name == "single_tap":
            for drop in range(6):
                five = SIX[:drop] + SIX[drop + 1:]
                err5 = float((piece_product_conv(x, w, five, **conv).double() - ref64).abs().max())
                assert err5 > 4 * bar, (drop, err5, bar)   # (measured: the least-wrong form is 8.6 ... 10.6 bars)


def test_split3_pieces_are_bf16_and_sum_exactly():
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(4096, generator=g) * torch.exp(4 * torch.randn(4096, generator=g))).numpy()
    h, m, l = split3_np(x)
    for p in (h, m, l):
        assert not (p.view(np.uint32) & np.uint32(0xFFFF)).any()
    assert (h.astype(np.float64) + m + l == x.astype(np.float64)).all()
    assert (np.abs(m) <= 2.0 ** -8 * np.abs(x)).all() and (np.abs(l) <= 2.0 ** -16 * np.abs(x)).all()
    # ties go to even: 1 + 2^-8 is halfway between the bf16 neighbours 1 and 1 + 2^-7
    t = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], dtype=np.float32)
    assert list(_bf16_rne(t)) == [1.0, 1 + 2.0 ** -6]
