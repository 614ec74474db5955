"""Per-wrapper GPU parity of the update path's GEMM-shaped gradients: the ivln_gemm_f32 descriptors that ops.linear_bwd_input,
ops.linear_bwd_weight and ops.conv2d_bwd_weight build (ivln-ce_amd/ops.py, "GEMM-shaped gradients"), and the conv input
gradient as train.py composes it (ops.conv2d over ops.weight_flip_transpose), each alone, against the same operation in
plain torch float64 on the CPU (F.linear / F.conv2d) differentiated by autograd.  Nothing here imports ivln_ce_amd.train or
oracle/.  Written like tests/test_gpu_train_kernels.py, whose helpers it imports.

Inputs are drawn in fp32 from a seeded generator and widened for the reference, so both sides see the same numbers.

Error bar: _Bar.check's,  4 * e32 + 4 * 2^-24 * max|float64|,  where e32 is the LARGER of two fp32 reference errors against
float64: torch-CPU fp32 autograd, and the same product in torch-CPU fp32 with K cut into `splits_used` contiguous chunks (the
kernel's chunk length where the route has a K tile), one fp32 matmul per chunk, the chunk results added in chunk order
(torch's blocked sum can be tighter than any split-K order at deep K).  Both are reference arithmetic, never the kernel's
output.  Every comparison writes one line to train_kernels.log: hip, e32, their ratio, the bar, and in the name column the
kernel that ran (family timing sink), ivln_gemm_desc.splits_used and `accumulate`.

Every result: the launch runs twice on the same inputs and must give identical bytes (split-K sums are in fixed order);
a strided destination's sentinel columns outside the slice are unchanged to the bit.

Which split-K epilogue a case is built for (launch_splitk_epilogue, csrc/gemm_conv.hip - the reduction kernels are not family
launches, so the selection is by construction, not observed):
  k_splitk_epilogue_flat4  contiguous dense output, M*N % 4 == 0: linear_bwd_weight (40, 12, 7) forced to split, (512, 96, 64),
                           the deep-K cases, every conv weight gradient with M*N % 4 == 0 that splits
  k_splitk_epilogue        everything else dense: linear_bwd_input whenever it splits (sDm = 1), linear_bwd_weight (40, 5, 13),
                           conv2d_bwd_weight Cout = 5, Cin = 3 (M*N = 135)
  k_splitk_epilogue4       dense outputs of these wrappers never reach it (a contiguous (M, N) with N % 4 == 0 is taken by
                           flat4 first); the NCHW form does: the 7x7 conv input gradient under tile_override 1
                           (M = 14, N = 768, K = 1568: 12 blocks of 64 x 64, 98 K tiles -> 16 splits, HoWo = 256)

GEMM_COVERED (bottom of the file) names the test of every wrapper; tests/test_train_kernel_coverage.py (CPU) pins it to
ops.py."""
import ctypes as C
import functools
import os
import re

import pytest
import torch
import torch.nn.functional as F

from test_gpu_train_kernels import DEV, E_INVALID, E_UNSUPPORTED, EPS, ROOT, _Bar, _leaf, _refused, _same_bytes, _strided, _twice

pytestmark = pytest.mark.gpu
SENTINEL = 7.0  # _strided's fill


def _const(path, name):
    """`constexpr int <name> = <value>;` of a kernel source"""
    src = open(os.path.join(ROOT, "ivln-ce_amd", "csrc", path)).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


BK = _const("gemm_common.h", "BK")    # K tile of k_gemm
BKV = _const("gemm_vec.hip", "BKV")   # K tile of k_gemm_vec
K_TILE = {"k_gemm": BK, "k_gemm_vec": BKV}  # (the direct weight-gradient kernels split over pixel tiles: equal chunks)


# ------------------------------------------------------------------------------------------------------------------
# observation: which family kernel ran, how many splits
# ------------------------------------------------------------------------------------------------------------------
def _observed(fn, max_launches=16):
    """fn() between ivln_family_timing_begin / _end -> (fn's result, {kernel name: launches})"""
    from ivln_ce_amd._lib import check, lib

    L = lib()
    L.ivln_family_timing_begin.argtypes = [C.c_int]
    L.ivln_family_timing_end.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.ivln_family_timing_report.argtypes = [C.c_char_p, C.c_int]
    check(L.ivln_family_timing_begin(max_launches), "ivln_family_timing_begin")
    ms, n, dropped = C.c_double(0), C.c_int(0), C.c_int(0)
    try:
        out = fn()
    finally:
        rc = L.ivln_family_timing_end(C.byref(ms), C.byref(n), C.byref(dropped))
    check(rc, "ivln_family_timing_end")
    assert dropped.value == 0
    ran = {}
    if n.value:
        buf = C.create_string_buffer(4096)
        assert L.ivln_family_timing_report(buf, 4096) == 0
        for line in buf.value.decode().splitlines():
            name, count, _ = line.split()
            ran[name] = int(count)
    return out, ran


def _one_kernel(ran, launches=2):
    assert len(ran) == 1 and list(ran.values()) == [launches], ran
    return next(iter(ran))


def _dropped(nk, splits):
    """the split count ivln_gemm_f32 uses for a forced one: empty trailing splits dropped"""
    tps = -(-nk // splits)
    return -(-nk // tps)


def _chunked(K, kernel, splits, part):
    """sum in chunk order of part(k0, k1) (an fp32 matmul over k0 <= k < k1) over `splits` contiguous chunks of K, cut where
    the kernel cuts them"""
    bk = K_TILE.get(kernel, 1)
    nk = -(-K // bk)
    step = -(-nk // splits) * bk
    acc = None
    for k0 in range(0, K, step):
        p = part(k0, min(K, k0 + step))
        acc = p if acc is None else acc + p
    return acc


def _worse(ref64, *refs32):
    """the fp32 reference that is further from float64: _Bar.check's e32 is then the larger of the reference errors"""
    return max(refs32, key=lambda r: float((r.double() - ref64).abs().max()))


def _al16(t):
    return t.data_ptr() % 16 == 0


def _with_override(override, fn):
    from ivln_ce_amd import ops

    saved = ops.TILE_OVERRIDE
    try:
        ops.TILE_OVERRIDE = override
        return fn()
    finally:
        ops.TILE_OVERRIDE = saved


# ------------------------------------------------------------------------------------------------------------------
# linear gradients
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lin_case(rows, O, I, seed=0):
    """inputs and the float64 / fp32 autograd gradients of F.linear, computed once per shape and left unchanged"""
    g = torch.Generator().manual_seed(rows * 7919 + O * 131 + I + seed)
    x = torch.randn(rows, I, generator=g)
    w = torch.randn(O, I, generator=g) / O ** 0.5
    dy = torch.randn(rows, O, generator=g)
    dx0 = torch.randn(rows, I, generator=g)   # non-zero destinations of the accumulating calls
    dw0 = torch.randn(O, I, generator=g)
    c = dict(x=x, w=w, dy=dy, dx0=dx0, dw0=dw0)
    for dt, tag in ((torch.float64, "64"), (torch.float32, "32")):
        xl, wl = _leaf(x, dt), _leaf(w, dt)
        F.linear(xl, wl).backward(dy.to(dt))
        c["dx" + tag], c["dw" + tag] = xl.grad, wl.grad
    return c


def _lin_refs(c, which, kernel, splits, accumulate):
    """(float64 reference, the worse of the two fp32 references) of dX or dW, `out0 + ...` when accumulating"""
    dy, w, x = c["dy"], c["w"], c["x"]
    if which == "dx":
        r64, r32, init = c["dx64"], c["dx32"], c["dx0"]
        ch = _chunked(dy.shape[1], kernel, splits, lambda a, b: dy[:, a:b] @ w[a:b, :])
    else:
        r64, r32, init = c["dw64"], c["dw32"], c["dw0"]
        ch = _chunked(dy.shape[0], kernel, splits, lambda a, b: dy[a:b, :].t() @ x[a:b, :])
    if accumulate:
        r64, r32, ch = init.double() + r64, init + r32, init + ch
    return r64, _worse(r64, r32, ch)


def _vec_ok(which, dy, other):
    """ivln_gemm_vec_eligible for the two linear descriptors: 16-byte bases, M, lda, K or N, ldb multiples of four"""
    rows, O = dy.shape
    I = other.shape[1]
    if which == "dx":  # A = w [k = o][m = i] (lda = I), B = dy [n = row][k = o]
        return _al16(other) and _al16(dy) and I % 4 == 0 and O % 4 == 0 and dy.stride(0) % 4 == 0
    return _al16(dy) and _al16(other) and O % 4 == 0 and dy.stride(0) % 4 == 0 and I % 4 == 0 and other.stride(0) % 4 == 0


def _run_lin(which, dy, other, override=0, accumulate=False, splits=None, init=None, strided_out=False):
    """one wrapper call, twice, under the timing sink -> (result, kernel, splits_used); `init`: the destination's contents
    (accumulate); strided_out: the destination is a column slice of a sentinel-filled wider matrix, checked afterwards"""
    from ivln_ce_amd import ops

    fn = ops.linear_bwd_input if which == "dx" else ops.linear_bwd_weight
    info, wides = {}, []

    def once():
        out = None
        if init is not None:
            if strided_out:
                out, wide = _strided(init)
                wides.append(wide)
            else:
                out = init.to(DEV).clone()
        return (fn(dy, other, out=out, accumulate=accumulate, splits=splits, info=info),)

    (got,), ran = _with_override(override, lambda: _observed(lambda: _twice(once)))
    for wide in wides:
        cols = got.shape[1]
        assert bool((wide[:, :4] == SENTINEL).all()) and bool((wide[:, 4 + cols:] == SENTINEL).all()), "sentinel columns changed"
    return got, _one_kernel(ran), info["splits_used"]


def _sweep_lin(which, c, label, dy=None, other=None, expect=None, overrides=None, accumulate=False, init=None,
               strided_out=False, splits=None, want_split=None):
    """default dispatch, then tile_override 1..5 and 7 where eligible: each against float64, all routes within the bar of
    the default one"""
    dy = c["dy"].to(DEV) if dy is None else dy
    other = (c["w"] if which == "dx" else c["x"]).to(DEV) if other is None else other
    vec = _vec_ok(which, dy, other)
    if expect is not None:
        assert ("k_gemm_vec" if vec else "k_gemm") == expect, "the case is not built for the route it names"
    bar = _Bar(f"linear_bwd_{'input' if which == 'dx' else 'weight'} {label}")
    base = None
    for ov in (overrides if overrides is not None else [0, 1, 2, 3, 4, 5] + ([7] if vec else [])):
        got, kernel, used = _run_lin(which, dy, other, ov, accumulate, splits, init, strided_out)
        assert kernel == ("k_gemm_vec" if (vec and ov in (0, 7)) else "k_gemm"), (ov, kernel)
        assert want_split is None or (used > 1) == want_split, (ov, used)
        r64, r32 = _lin_refs(c, which, kernel, used, accumulate)
        _, b = bar.check(f"ov{ov} {kernel} s{used} acc{int(accumulate)}", got, r64, r32)
        if base is None:
            base = (got, b)
        else:
            bar.within(f"ov{ov}/ov0", got, base[0], base[1])
    return bar, base[0]


DX_SHAPES = [
    (24, 384, 416),     # rows <= 32: 128 x 32 tiles, 12 / 24 K tiles -> split by the heuristic
    (100, 64, 96),      # ragged rows
    (1, 1536, 128),     # one row, deep K
    (333, 36, 260),     # K barely over one 32-deep tile, several blocks
    (5, 3, 512),        # K below one K tile (and K % 4 != 0: the scalar-gather kernel)
    (7, 50, 13),        # M and K both no multiples of four
    (64, 128, 1184),    # the state-compress input width
]


@pytest.mark.parametrize("rows,O,I", DX_SHAPES)
def test_linear_bwd_input(rows, O, I):
    """dX = dY W against float64 autograd of F.linear on every route.  (7, 50, 13): k_gemm runs, tile_override 7 is refused."""
    from ivln_ce_amd import ops

    c = _lin_case(rows, O, I)
    aligned = I % 4 == 0 and O % 4 == 0
    bar, _ = _sweep_lin("dx", c, f"{rows}x{O}x{I}", expect="k_gemm_vec" if aligned else "k_gemm")
    if not aligned:
        _with_override(7, lambda: _refused(E_UNSUPPORTED, ops.linear_bwd_input, c["dy"].to(DEV), c["w"].to(DEV)))
    bar.done()


def test_linear_bwd_input_strided_operands_and_accumulate():
    """dy as a column slice of a wider matrix at offset 4 (16-byte aligned: the vector-load kernel still runs) and at offset 3
    (base not 16-byte aligned: k_gemm, the same gradient); out as a column slice with accumulate into non-zero contents,
    split (the reduction kernel's add) and not (the main kernel's add)."""
    c = _lin_case(100, 64, 96)
    dy4, _ = _strided(c["dy"])
    dy3, _ = _strided(c["dy"], pad_l=3, pad_r=5)
    assert dy4.stride(0) == dy3.stride(0) == 72 and _al16(dy4) and not _al16(dy3)
    b4, g4 = _sweep_lin("dx", c, "dy[:,4:68]", dy=dy4, expect="k_gemm_vec")
    b3, g3 = _sweep_lin("dx", c, "dy[:,3:67]", dy=dy3, expect="k_gemm")
    b3.within("off3/off4", g3, g4, 4 * float((c["dx32"].double() - c["dx64"]).abs().max()) + 4 * EPS * float(c["dx64"].abs().max()))
    ba, _ = _sweep_lin("dx", c, "out slice, acc", accumulate=True, init=c["dx0"], strided_out=True, want_split=False)
    # (24, 384, 416) splits by the heuristic: the accumulate is the split-K reduction's; forced to one slab: the main kernel's
    c2 = _lin_case(24, 384, 416)
    bs, _ = _sweep_lin("dx", c2, "out slice, acc, split", accumulate=True, init=c2["dx0"], strided_out=True,
                       want_split=True)
    b1, _ = _sweep_lin("dx", c2, "out slice, acc, s=1", accumulate=True, init=c2["dx0"], strided_out=True, splits=1,
                       want_split=False)
    bn, _ = _sweep_lin("dx", c2, "out slice", init=c2["dx0"], strided_out=True)  # (not accumulating: the contents are overwritten)
    for b in (b4, b3, ba, bs, b1, bn):
        b.done()


def test_linear_bwd_input_forced_splits_and_workspace():
    """K = 384 forced to 1, 2, 3, 7 and nk + 5 splits on both kernels: splits_used is the count after the empty trailing splits
    are dropped, every result within the bar of float64.  A forced split with one float too little workspace is refused
    (IVLN_E_INVALID) before anything is launched."""
    from ivln_ce_amd import ops

    rows, O, I = 24, 384, 416
    c = _lin_case(rows, O, I)
    dy, w = c["dy"].to(DEV), c["w"].to(DEV)
    bar = _Bar(f"linear_bwd_input {rows}x{O}x{I} forced")
    for ov, kernel_want in ((0, "k_gemm_vec"), (1, "k_gemm")):
        nk = -(-O // K_TILE[kernel_want])
        for s in (1, 2, 3, 7, nk + 5):
            got, kernel, used = _run_lin("dx", dy, w, ov, splits=s)
            assert kernel == kernel_want and used == _dropped(nk, s), (ov, s, kernel, used)
            r64, r32 = _lin_refs(c, "dx", kernel, used, False)
            bar.check(f"ov{ov} {kernel} s{used}<-{s} acc0", got, r64, r32)
    assert _dropped(12, 7) == 6 and _dropped(12, 17) == 12 and _dropped(24, 7) == 6 and _dropped(24, 29) == 24

    def raw(splits, ws_floats):
        out = torch.full((rows, I), SENTINEL, device=DEV)
        ws = torch.zeros(splits * I * rows, device=DEV)
        d = ops.GemmDesc()
        d.A, d.B, d.D = w.data_ptr(), dy.data_ptr(), out.data_ptr()
        d.M, d.N, d.K = I, rows, O
        d.amode, d.bmode, d.dmode = ops.A_KM, ops.B_NK, ops.D_DENSE
        d.lda, d.ldb, d.sDm, d.sDn, d.HoWo = I, O, 1, I, 1
        d.splits, d.ws, d.ws_floats = splits, ws.data_ptr(), ws_floats
        rc, ran = _observed(lambda: ops._L().ivln_gemm_f32(C.byref(d), ops.stream_ptr()))
        torch.cuda.synchronize()
        return rc, ran, out

    rc, ran, out = raw(3, 3 * I * rows - 1)
    assert rc == E_INVALID and ran == {} and bool((out == SENTINEL).all())
    rc, ran, out = raw(3, 3 * I * rows)
    assert rc == 0 and ran == {"k_gemm_vec": 1}
    r64, r32 = _lin_refs(c, "dx", "k_gemm_vec", 3, False)
    bar.check("exact ws k_gemm_vec s3 acc0", out, r64, r32)
    bar.done()


DW_SHAPES = [
    (512, 96, 64),     # 16 / 32 K tiles under two blocks: split by the heuristic -> flat4 reduction
    (40, 12, 7),       # M*N % 4 == 0 and N % 4 != 0: the flat4 reduction once split
    (40, 5, 13),       # M*N odd: the scalar reduction
    (33, 128, 416),    # K just over one 32-deep tile
    (3, 8, 12),        # K below every tile
]


@pytest.mark.parametrize("rows,O,I", DW_SHAPES)
def test_linear_bwd_weight(rows, O, I):
    """dW = dY^T X against float64 autograd of F.linear on every route, by the heuristic and forced to 2 and 3 splits (the
    small shapes do not split on their own: K is a few tiles)."""
    c = _lin_case(rows, O, I)
    aligned = I % 4 == 0 and O % 4 == 0
    bar, _ = _sweep_lin("dw", c, f"{rows}x{O}x{I}", expect="k_gemm_vec" if aligned else "k_gemm")
    dy, x = c["dy"].to(DEV), c["x"].to(DEV)
    for ov in (0, 1):
        for s in (2, 3):
            got, kernel, used = _run_lin("dw", dy, x, ov, splits=s)
            assert used == _dropped(-(-rows // K_TILE[kernel]), s)
            r64, r32 = _lin_refs(c, "dw", kernel, used, False)
            bar.check(f"ov{ov} {kernel} s{used}<-{s} acc0", got, r64, r32)
            assert (used > 1) == (rows > K_TILE[kernel])  # (40 rows are two 32-deep / three 16-deep tiles: the reduction ran)
    bar.done()


@pytest.mark.parametrize("tier,more_than", [(512, 16), (4096, 64)])
def test_linear_bwd_weight_deep_k_split_tiers(tier, more_than):
    """A tiny M x N = 8 x 12 under `tier` K tiles of the route taken (rows = tier * the larger K tile, so that both kernels
    cross it): the split heuristic's 64- and 256-split tiers."""
    rows, O, I = tier * max(BK, BKV), 8, 12
    c = _lin_case(rows, O, I)
    dy, x = c["dy"].to(DEV), c["x"].to(DEV)
    bar = _Bar(f"linear_bwd_weight {rows}x{O}x{I} deep K")
    for ov, kernel_want in ((0, "k_gemm_vec"), (1, "k_gemm")):
        assert -(-rows // K_TILE[kernel_want]) >= tier
        got, kernel, used = _run_lin("dw", dy, x, ov)
        assert kernel == kernel_want and used > more_than, (kernel, used)
        r64, r32 = _lin_refs(c, "dw", kernel, used, False)
        bar.check(f"ov{ov} {kernel} s{used} acc0", got, r64, r32)
    bar.done()


def test_linear_bwd_weight_accumulate_and_strided_operands():
    """accumulate with LINEAR_BWD_SPLIT on (the split-K reduction adds into out) and off (one slab, the main kernel adds);
    dy and x as column slices of wider matrices, 16-byte aligned (vector loads) and not (k_gemm)."""
    from ivln_ce_amd import ops

    c = _lin_case(512, 96, 64)
    bars = []
    saved = ops.LINEAR_BWD_SPLIT
    try:
        for flag in (True, False):
            ops.LINEAR_BWD_SPLIT = flag
            dy, x = c["dy"].to(DEV), c["x"].to(DEV)
            for ov in (0, 1):
                _, _, used = _run_lin("dw", dy, x, ov, accumulate=True, init=c["dw0"])
                assert (used > 1) == flag, (flag, ov, used)
            bars.append(_sweep_lin("dw", c, f"acc, LINEAR_BWD_SPLIT={flag}", accumulate=True, init=c["dw0"])[0])
    finally:
        ops.LINEAR_BWD_SPLIT = saved
    dy4, x4 = _strided(c["dy"])[0], _strided(c["x"])[0]
    dy3, x3 = _strided(c["dy"], pad_l=3, pad_r=5)[0], _strided(c["x"], pad_l=3, pad_r=5)[0]
    assert _al16(dy4) and _al16(x4) and not _al16(dy3) and not _al16(x3)
    b4, g4 = _sweep_lin("dw", c, "dy, x slices +4", dy=dy4, other=x4, expect="k_gemm_vec")
    b3, g3 = _sweep_lin("dw", c, "dy, x slices +3", dy=dy3, other=x3, expect="k_gemm")
    bd, _ = _sweep_lin("dw", c, "dy slice +3", dy=dy3, expect="k_gemm", overrides=[0])
    bx, _ = _sweep_lin("dw", c, "x slice +3", other=x3, expect="k_gemm", overrides=[0])
    b3.within("off3/off4", g3, g4, 4 * float((c["dw32"].double() - c["dw64"]).abs().max()) + 4 * EPS * float(c["dw64"].abs().max()))
    for b in bars + [b4, b3, bd, bx]:
        b.done()


# ------------------------------------------------------------------------------------------------------------------
# conv weight gradient
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv_case(N, Cin, H, W, Cout, KH, KW, stride, pad, one_hot=False):
    g = torch.Generator().manual_seed(N * 1009 + Cin * 101 + H * 31 + W * 7 + Cout + KH * 3 + KW + stride + pad)
    x = (torch.rand(N, Cin, H, W, generator=g) < 0.3).float() if one_hot else torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, KH, KW, generator=g) / (Cin * KH * KW) ** 0.5
    c = dict(x=x, w=w)
    for dt, tag in ((torch.float64, "64"), (torch.float32, "32")):
        xl, wl = _leaf(x, dt), _leaf(w, dt)
        y = F.conv2d(xl, wl, None, stride, pad)
        if "dy" not in c:
            c["dy"] = torch.randn(y.shape, generator=g)
        y.backward(c["dy"].to(dt))
        c["dx" + tag], c["dw" + tag] = xl.grad, wl.grad
    # the weight gradient as the GEMM the kernels run: dy [Cout][k = image, pixel]  x  im2col(x) [k][(ci, kh, kw)]
    L = c["dy"].shape[2] * c["dy"].shape[3]
    c["A"] = c["dy"].reshape(N, Cout, L).permute(1, 0, 2).reshape(Cout, N * L).contiguous()
    c["B"] = F.unfold(x, (KH, KW), padding=pad, stride=stride).permute(0, 2, 1).reshape(N * L, Cin * KH * KW).contiguous()
    return c


def _wgrad_refs(c, kernel, splits):
    A, B = c["A"], c["B"]
    ch = _chunked(A.shape[1], kernel, splits, lambda a, b: A[:, a:b] @ B[a:b, :]).view_as(c["dw64"])
    return c["dw64"], _worse(c["dw64"], c["dw32"], ch)


def _run_wgrad(c, KH, KW, stride, pad, override=0, x_exact_bf16=False, splits=None):
    from ivln_ce_amd import ops

    info = {}
    dy, x = c["dy"].to(DEV), c["x"].to(DEV)
    once = lambda: (ops.conv2d_bwd_weight(dy, x, KH, KW, stride, pad, x_exact_bf16=x_exact_bf16, splits=splits, info=info),)  # noqa: E731
    (got,), ran = _with_override(override, lambda: _observed(lambda: _twice(once)))
    return got, _one_kernel(ran), info["splits_used"]


def _sweep_wgrad(geom, extra=(), x_exact_bf16=False, one_hot=False, need_split=()):
    """default dispatch and tile_override 1..5 (k_gemm), plus `extra` overrides (6: k_wgrad_direct, 9: k_wgrad_bf3), the route
    asserted: by default k_wgrad_direct takes the stride-1 3x3 / 7x7 geometries and k_gemm (A_NCHW_P x B_IM2COL_T) the rest
    (at these sizes k_wgrad_bf3 declines unless insisted on: fewer workgroups than half the chip)."""
    N, Cin, H, W, Cout, KH, KW, stride, pad = geom
    c = _conv_case(*geom, one_hot=one_hot)
    direct = stride == 1 and KH == KW and KH in (3, 7)
    bar = _Bar(f"conv2d_bwd_weight {'x'.join(map(str, geom[:5]))} k{KH}x{KW} s{stride} p{pad}{' xe' if x_exact_bf16 else ''}")
    base = None
    for ov in [0, 1, 2, 3, 4, 5] + list(extra):
        want = "k_wgrad_bf3" if ov == 9 else ("k_wgrad_direct" if (direct and ov in (0, 6)) else "k_gemm")
        got, kernel, used = _run_wgrad(c, KH, KW, stride, pad, ov, x_exact_bf16)
        assert kernel == want, (ov, kernel, want)
        if ov in need_split:
            assert used > 1, (ov, used)
        r64, r32 = _wgrad_refs(c, kernel, used)
        _, b = bar.check(f"ov{ov} {kernel} s{used} acc0", got, r64, r32)
        if base is None:
            base = (got, b)
        else:
            bar.within(f"ov{ov}/ov0", got, base[0], base[1])
    return bar


WGRAD_GEOMETRIES = [  # (N, Cin, H, W, Cout, KH, KW, stride, pad)
    (6, 48, 1, 16, 96, 1, 1, 1, 0),    # Conv1d k = 1, the kv projections (H = 1)
    (5, 13, 1, 7, 10, 1, 1, 1, 0),     # ragged
    (3, 16, 9, 10, 8, 1, 1, 2, 0),     # 1x1 stride 2
    (2, 8, 11, 12, 24, 3, 3, 2, 1),    # 3x3 stride 2
    (2, 6, 9, 9, 8, 5, 5, 1, 2),       # 5x5
    (2, 6, 9, 10, 8, 1, 3, 1, 1),      # 1x3 (the single pad pads both axes: 11 x 10 outputs)
    (2, 6, 9, 10, 8, 1, 3, 1, 0),
    (2, 6, 9, 10, 8, 3, 1, 1, 1),      # 3x1
    (2, 6, 9, 10, 8, 3, 1, 1, 0),
]


@pytest.mark.parametrize("geom", WGRAD_GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
def test_conv2d_bwd_weight_gemm_geometries(geom):
    """B_IM2COL_T on k_gemm beyond stride-1 3x3 / 7x7: k = 1 (the live Conv1d form), stride 2, k = 5, KH != KW - every one
    against float64 autograd of F.conv2d.  None of them is refused: the gather takes any kernel size, stride and pad."""
    _sweep_wgrad(geom).done()


def test_conv2d_bwd_weight_scalar_split_reduction():
    """3x3, Cout = 5, Cin = 3: M*N = 135 is odd, so the slabs of a split launch are reduced by the scalar k_splitk_epilogue;
    four 8 x 8 images are two pixel tiles of k_wgrad_direct and sixteen K tiles of k_gemm: both split."""
    _sweep_wgrad((4, 3, 8, 8, 5, 3, 3, 1, 1), extra=[6], need_split=(0, 1, 6)).done()


def test_conv2d_bwd_weight_direct_and_split_bf16_routes():
    """stride-1 3x3 and 7x7 pad 3 on every route that takes them - k_wgrad_direct (default and insisted on), k_gemm, and for
    the 7x7 k_wgrad_bf3 (tile_override 9; widths 16 and 8, more than 32 channels too), with x_exact_bf16 on one-hot input
    and without - all with this file's bar.  What a kernel is not built for it refuses before any launch."""
    from ivln_ce_amd import ops

    bars = [_sweep_wgrad((3, 8, 10, 16, 24, 3, 3, 1, 1), extra=[6]),
            _sweep_wgrad((4, 6, 16, 16, 8, 7, 7, 1, 3), extra=[6, 9]),
            _sweep_wgrad((4, 5, 8, 8, 40, 7, 7, 1, 3), extra=[6, 9]),
            _sweep_wgrad((4, 6, 16, 16, 8, 7, 7, 1, 3), extra=[6, 9], x_exact_bf16=True, one_hot=True),
            _sweep_wgrad((4, 6, 16, 16, 8, 7, 7, 1, 3), extra=[6, 9], one_hot=True)]
    c = _conv_case(3, 8, 10, 16, 24, 3, 3, 1, 1)
    _with_override(9, lambda: _refused(E_UNSUPPORTED, ops.conv2d_bwd_weight, c["dy"].to(DEV), c["x"].to(DEV), 3, 3, 1, 1))
    c = _conv_case(2, 8, 11, 12, 24, 3, 3, 2, 1)
    _with_override(6, lambda: _refused(E_UNSUPPORTED, ops.conv2d_bwd_weight, c["dy"].to(DEV), c["x"].to(DEV), 3, 3, 2, 1))
    for b in bars:
        b.done()


# ------------------------------------------------------------------------------------------------------------------
# conv input gradient, as train.py composes it
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Cin,H,W,Cout,k,p", [(3, 14, 16, 16, 32, 7, 3), (2, 8, 9, 11, 6, 3, 1)])
def test_conv2d_bwd_input_composed(N, Cin, H, W, Cout, k, p):
    """dX = conv2d(dY, weight_flip_transpose(W), pad = k - 1 - p) against float64 autograd's x.grad, by default dispatch and
    on the implicit GEMM (tile_override 1; the 7x7 case splits there and leaves through the NCHW four-column reduction)."""
    from ivln_ce_amd import ops

    c = _conv_case(N, Cin, H, W, Cout, k, k, 1, p)
    dy, w = c["dy"].to(DEV), c["w"].to(DEV)
    wt = ops.weight_flip_transpose(w)
    assert _same_bytes(wt.cpu(), c["w"].flip(2, 3).transpose(0, 1).contiguous())  # (pure data movement)
    # the same product in fp32 as a GEMM over K = (co, kh, kw) in `splits` chunks: the split count of ops.conv2d is not
    # exposed, so the chunked reference takes the deepest the dispatcher can choose (16) and the shallowest (1 = autograd's)
    A = c["w"].flip(2, 3).transpose(0, 1).reshape(Cin, Cout * k * k)
    B = F.unfold(c["dy"], (k, k), padding=k - 1 - p)  # (N, Cout*k*k, H*W)
    ch = _chunked(A.shape[1], "k_gemm", 16, lambda a, b: torch.einsum("ck,nkl->ncl", A[:, a:b], B[:, a:b, :])).reshape(N, Cin, H, W)
    r64, r32 = c["dx64"], _worse(c["dx64"], c["dx32"], ch)
    bar = _Bar(f"conv2d_bwd_input {N}x{Cin}x{H}x{W}x{Cout} k{k} p{p}")
    base = None
    for ov in (0, 1):
        once = lambda: (ops.conv2d(dy, wt, pad=k - 1 - p, weight_is_temp=True),)  # noqa: E731
        (got,), ran = _with_override(ov, lambda: _observed(lambda: _twice(once)))
        kernel = _one_kernel(ran)
        assert ov == 0 or kernel == "k_gemm"
        _, b = bar.check(f"ov{ov} {kernel} acc0", got, r64, r32)
        if base is None:
            base = (got, b)
        else:
            bar.within("ov1/ov0", got, base[0], base[1])
    bar.done()


GEMM_COVERED = {
    "linear_bwd_input": "test_linear_bwd_input",
    "linear_bwd_weight": "test_linear_bwd_weight",
    "conv2d_bwd_weight": "test_conv2d_bwd_weight_gemm_geometries",
    "conv2d_bwd_input(composed)": "test_conv2d_bwd_input_composed",
}
