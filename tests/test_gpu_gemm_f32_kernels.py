"""Per-kernel GPU parity of the fp32 MFMA forward routes behind ivln_gemm_f32 - k_gemm on its conv operand modes
(csrc/gemm_conv.hip), k_gemm_vec (gemm_vec.hip), k_conv_direct (conv_direct.hip), k_conv1x1_stream (conv1x1_stream.hip) and the
split-K reductions in their NCHW forms - each alone, at the smallest shapes that reach every tile's ragged edges
(tests/test_gemm_f32_plan_coverage.py holds the case tables and asserts the edges on the CPU), against the same operation in
plain torch float64 on the CPU: F.conv2d, F.conv_transpose2d for B_CONVT, F.pixel_shuffle(F.conv2d(F.pad(x, (0, 1, 0, 1)), W), 2)
for B_CONV_K2 -> UP2X4 (B_CONV1X1 -> UP2X4: the same without the pad), the parity-class scatter of a conv into a 2H x 2W
destination for UP2, the epilogue in float64.  ops.GemmDesc is filled here and handed to ops.gemm, so this file owns every
buffer and ops.conv2d's Python gates are not in the way of the small shapes.

Inputs are drawn in fp32 from a seeded generator and widened for the reference.  Error bar: _Bar.check of tests/kernel_bar.py,
unchanged: 4 * e32 + 4 * 2^-24 * max|float64| with e32 the error of the same torch ops in fp32 on the CPU - for a launch that
splits, the worse of that and the fp32 sum over the launch's own K chunks added in chunk order (_worse of
tests/test_gpu_train_gemms.py; the direct kernel's chunks are cps * CI input channels).  Both references are reference
arithmetic, never the kernel's output.  Every comparison goes to gemm_f32_kernels.log in the suite's log directory before
anything is asserted.

Buffers.  Every operand (A, A_packed, B, residual, scale, shift, koff / kpos, img_run_flags) sits between NaN (integer:
out-of-range) guard bands; the gap between two images of a padded in_img_stride and the residual's channels beside the slice
are NaN too.  Every destination - D, a Ctot-wider D written as a channel slice at an offset that keeps 16-byte alignment (and,
`misD`, four bytes off it), the slabs of a deferred launch, stat_partials - starts as NaN between two bands of sentinels, with
sentinels in the channels beside the slice: an element never written fails the bar, one written outside fails the band, to
the bit.  `accumulate` and img_run_flags forms start from finite values instead.  Every launch runs twice (_twice) and must
give the same bytes.

Observed and held to plan(case): the kernel name (family timing sink), ivln_gemm_desc.splits_used, *stat_tiles, accepted versus
refused with the return code (refusals only through the launcher's return code: nothing here launches past a predicate).
Which reduction kernel ran is by construction (they are not family launches); k_splitk_epilogue4 and k_splitk_epilogue are
held to each other bit for bit.

Forms.  Every instantiation runs `plain` (no epilogue operand) and `full` (scale + shift + residual + ReLU into a channel slice,
the input's image stride padded).  On the cases that name them (FORM_CASES and the tables beside it): shift without scale,
accumulate with one slab and with several, defer_epilogue (the slabs summed in float64 against the raw conv, as many slabs as
splits_used, D untouched), grp_imgs == one launch per weight set, no_wide_epilogue == the wide epilogue, no_xcd_remap == the
default, A_packed == unpacked (all bit for bit), img_run_flags (skipped tiles keep their bytes, a 0-flagged image beside a
1-flagged one is written and meets the bar, all zeros leaves the destination untouched), stat_partials merged by
ivln_bn_stats_from_partials_f32 against the float64 count / mean / variance of what the launch stored.

Measured on an MI355X (304 tests, 571 comparisons, none OVER, under 3 s for the file).  Largest hip / e32 per kernel:
k_conv_direct 2.95 (d-k3-s1-w33 plain: err 2.9e-06, bar 4.9e-06), k_gemm 2.02 (g-t2-k7 full), k_gemm_vec 1.89 (v-s2-howo6
plain), k_conv1x1_stream 1.08 (s-k256-m96 full); slab sums 1.13 (r-up2x4) and below; the merged statistics 4.62 (st-k7-w16-m40
variance: err 1.3e-07 against a bar of 3.6e-07, whose larger term is 4 * 2^-24 * max|variance|).  Every observed kernel name,
split count, *stat_tiles and refusal equalled the plan's.  The first run found no kernel defect beyond the two the CPU file
records (the packed read of k_conv1x1_stream<64, 2>, fixed before any such shape ran; tile_override 8 with splits > 1, which
the plan could not restate as the header describes it).  One case of the first version was OVER and is not in the tables:
d-auto as a 3x3 conv of 128 channels (K = 1152 in ONE accumulator chain, 16 images of 8 x 8, 40 channels out) measured hip
5.75e-06, e32 1.04e-06 (5.54), bar 5.11e-06 - 576 sequential MFMA steps per output against torch's blocked fp32 sum; no
arithmetic of the kernel is wrong (the same products, the order the header of conv_direct.hip states), and the shape was
outside this file's own size rule (at most a few dozen channels), so the route it was there for - no override, the direct
kernel past its pixel-starved gate - is now held by the 7x7 shape with 2 channels over 32 images.  Deep K in one slab stays
with the workload shapes of tests/test_gpu_kernels.py.

A scratch build with ONE value-only defect in each main kernel (nothing of it is committed) fails 181 of the 304 tests:
  k_gemm::stage zeroes the last A element of a thread            24 of 69 (+ the 5 below): that element is row 16 e + 48 ... 63 of a
      64-row tile (112 ... 127 of 128, 16 ... 31 of 32): dead rows at M = 40, live in the ragged-M cases and on the 32 x 128 tile
  k_gemm_vec stages the second register set as zeros             36 of 39 (+ 4): v-k1 has one K tile, two flag cases run no tile
  k_conv_direct drops the patch's last staged row                108 of 126 (+ 3): the 18 others are images shorter than their pixel
      tile (5 rows on the 8-row tiles: that row is padding).  The first version's 7x7 cases (5 and 9 rows) ALL passed it - their
      last staged row was padding on every tile - hence 7 | 11 rows there, the two-column-tile cases and the CPU edge last_patch_row
  k_conv1x1_stream reads shift[m] for shift[me]                  1 of 27: f-grp-stream, the one launch where me != m
  k_splitk_epilogue4 skips slab 0                                12 of 12 (5 behind k_gemm, 4 behind k_gemm_vec, 3 behind k_conv_direct)
and none of the 30 refusal tests (nothing launches)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import test_gemm_f32_plan_coverage as P
from kernel_bar import _Bar, _same_bytes, _twice

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOG = "gemm_f32_kernels.log"
RC = {"invalid": -1, "unsupported": -5}
SENT, PAD, NAN = -777.0, 8, float("nan")
IBAND = 0x7FFF7FFF   # guard value of the integer tables: a tap (32767, 32767) is outside every image, a flag of it is not 0 | 1


def _observed(fn):
    from test_gpu_train_gemms import _observed as obs

    return obs(fn)


def _worse(ref64, *refs32):
    from test_gpu_train_gemms import _worse as w

    return w(ref64, *refs32)


def test_return_codes_are_the_headers():
    import os
    import re

    hdr = open(os.path.join(P.ROOT, "include", "ivln_hip.h")).read()
    for name, code in RC.items():
        assert int(re.search(r"IVLN_E_%s\s*=?\s*(-?\d+)" % name.upper(), hdr).group(1)) == code


def _seed(tag):
    s = 23
    for ch in tag.split("-pk")[0]:   # (a packed twin draws its unpacked case's numbers)
        s = (s * 131 + ord(ch)) % (2 ** 31)
    return s


# ------------------------------------------------------------------------------------------------------------------
# inputs and references (CPU)
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tensors(tag):
    """the case's operands in fp32 on the CPU (one draw per case): A as the GEMM sees it, (G, M, K) with K = (ci, kh, kw)"""
    c = _case(tag)
    d = P.desc(c)
    g = torch.Generator().manual_seed(_seed(tag))
    G = d.nimg // d.grp if d.grp else 1
    Ho, Wo = (d.Hout, d.Wout) if d.dmode == "nchw" else (2 * d.Hout, 2 * d.Wout)
    Cp = d.C   # channels of the epilogue parameters and of the destination
    return dict(G=G, x=torch.randn(d.nimg, d.Cin, d.Hin, d.Win, generator=g), A=torch.randn(G, d.M, d.K, generator=g) / d.K ** 0.5,
                scale=torch.rand(G * Cp, generator=g) + 0.5, shift=torch.randn(G * Cp, generator=g) * 0.3,
                res=torch.randn(d.nimg, Cp + P.WIDER, Ho, Wo, generator=g), d0=torch.randn(d.nimg, Cp, Ho, Wo, generator=g),
                out_shape=(d.nimg, Cp, Ho, Wo))


def _raw(c, dt, k0=0, k1=None):
    """the bare product over K columns [k0, k1) in dtype dt as the GEMM's rows: (imgs, M, Hout, Wout)"""
    d, t = P.desc(c), _tensors(c["tag"])
    x = t["x"].to(dt)
    A = t["A"].clone()
    A[:, :, :k0] = 0
    if k1 is not None:
        A[:, :, k1:] = 0
    per = d.nimg // t["G"]
    outs = []
    for gi in range(t["G"]):
        xg, w = x[gi * per:(gi + 1) * per], A[gi].to(dt).reshape(d.M, d.Cin, d.KH, d.KW)
        if d.bmode == "convt":
            outs.append(F.conv_transpose2d(xg, w.permute(1, 0, 2, 3), stride=d.stride, padding=d.pad, output_padding=d.opad))
        elif d.bmode == "k2":
            outs.append(F.conv2d(F.pad(xg, (0, 1, 0, 1)), w))
        else:
            outs.append(F.conv2d(xg, w, stride=d.stride, padding=d.pad, dilation=d.dil))
    return torch.cat(outs, 0)


def _raw_chunked(c, step):
    """fp32: one product per K chunk of `step` columns, added in chunk order (what a split launch sums)"""
    K = P.desc(c).K
    acc = None
    for k0 in range(0, K, step):
        part = _raw(c, torch.float32, k0, min(K, k0 + step))
        acc = part if acc is None else acc + part
    return acc


def _finish(c, form, raw, dt):
    """raw (imgs, M, Hout, Wout) -> what the launch leaves in its destination's slice: the parity-class layout, then the form's
    epilogue in the kernels' order (scale / shift, residual, D +=, ReLU).  UP2: the class's own (Hout, Wout) grid."""
    d, t = P.desc(c, form), _tensors(c["tag"])
    y = F.pixel_shuffle(raw, 2) if d.dmode == "up2x4" else raw
    per = d.nimg // t["G"]
    pick = (lambda v: v[:, :, d.cls[0]::2, d.cls[1]::2]) if d.dmode == "up2" else (lambda v: v)
    chan = lambda v: v.to(dt).reshape(t["G"], d.C).repeat_interleave(per, 0)[:, :, None, None]   # noqa: E731
    if d.has_scale:
        y = y * chan(t["scale"]) + chan(t["shift"])
    elif d.has_shift:
        y = y + chan(t["shift"])
    if d.has_res:
        y = y + pick(t["res"][:, P.C0:P.C0 + d.C]).to(dt)
    if d.acc:
        y = y + pick(t["d0"]).to(dt)
    return torch.relu(y) if d.relu else y


@functools.lru_cache(maxsize=None)
def _refs(tag, form, k_step):
    """(float64, fp32) of (case, form); k_step: the K columns per split of a launch that splits (0: one slab)"""
    c = _case(tag)
    r64 = _finish(c, form, _raw(c, torch.float64), torch.float64)
    r32 = _finish(c, form, _raw(c, torch.float32), torch.float32)
    if k_step:
        r32 = _worse(r64, r32, _finish(c, form, _raw_chunked(c, k_step), torch.float32))
    return r64, r32


@functools.lru_cache(maxsize=None)
def _all_cases():
    return P.by_tag()


def _case(tag):
    return _all_cases()[tag]


# ------------------------------------------------------------------------------------------------------------------
# one launch
# ------------------------------------------------------------------------------------------------------------------
class _Guarded:
    """n elements between two bands of PAD guard values (`off` more in front: four bytes off a 16-byte boundary)"""

    def __init__(self, n, fill=NAN, band=SENT, dtype=torch.float32, off=0):
        self.buf = torch.full((n + 2 * PAD + off,), band, dtype=dtype, device=DEV)
        self.n, self.lo, self.band = n, PAD + off, band
        self.mid[:] = fill

    @property
    def mid(self):
        return self.buf[self.lo:self.lo + self.n]

    def bands_ok(self):
        return bool((self.buf[:self.lo] == self.band).all()) and bool((self.buf[self.lo + self.n:] == self.band).all())


def _operand(t, off=0, band=NAN, dtype=torch.float32):
    """a read-only operand between guard bands -> (the buffer, keeping it alive; the device view of the data)"""
    g = _Guarded(t.numel(), fill=0, band=band, dtype=dtype, off=off)
    g.mid[:] = t.reshape(-1).to(DEV)
    return g, g.mid


def _launch(c, form="plain", only_group=None, marker=None):
    """Fill the descriptor of (case, form) from P.desc and the case's tensors, launch once, return dict(out = the written slice
    (imgs, C, Ho, Wo), splits_used, stat_tiles, stats, slabs (slabs, M, N) of a split or deferred launch).  Raises IvlnError on
    a refusal.  only_group = g: the launch for weight set g alone (its images, its weights, no grp_imgs).  marker: a finite
    tensor the slice starts from (img_run_flags)."""
    from ivln_ce_amd import ops

    d, t = P.desc(c, form), _tensors(c["tag"])
    tag = c["tag"]
    keep = []
    g = ops.GemmDesc()
    used, ntiles = ops.i32(-1), ops.i32(-1)
    g.splits_used = C.pointer(used)
    G, per = t["G"], d.nimg // t["G"]
    sl = slice(0, d.nimg) if only_group is None else slice(only_group * per, (only_group + 1) * per)
    gsl = slice(0, G) if only_group is None else slice(only_group, only_group + 1)
    nimg, Gl = sl.stop - sl.start, gsl.stop - gsl.start
    g.M, g.N, g.K = d.M, nimg * d.HoWo, d.K
    g.Cin, g.Hin, g.Win, g.Hout, g.Wout = d.Cin, d.Hin, d.Win, d.Hout, d.Wout
    g.stride, g.pad, g.dil, g.HoWo = d.stride, d.pad, d.dil, d.HoWo
    g.amode, g.bmode, g.dmode = ops.A_MK, P.BMODES[d.bmode], P.DMODES[d.dmode]
    g.tile_override, g.splits, g.no_wide_epilogue, g.no_xcd_remap = d.ov, d.splits, int(d.nwe), int(d.noxcd)
    g.defer_epilogue = int(d.defer)
    # A: (G, M, lda), the columns past K and the bands NaN
    Ad = torch.full((Gl, d.M, d.lda), NAN)
    Ad[:, :, :d.K] = t["A"][gsl]
    ka, av = _operand(Ad, off=0 if d.A_al else 1)
    keep.append(ka)
    g.A, g.lda = av.data_ptr(), d.lda
    if d.grp and only_group is None:
        g.grp_imgs, g.a_grp_stride = d.grp, d.M * d.lda
    if d.packed:
        L = ops._L()
        L.ivln_conv_packed_floats.restype = C.c_int64
        L.ivln_conv_packed_floats.argtypes = [C.c_int] * 3
        L.ivln_conv_pack_weights_f32.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        KS = d.KS or 1
        n1 = L.ivln_conv_packed_floats(d.M, d.Cin, KS)
        assert n1 == P.conv_packed_floats(d.M, d.Cin, KS) > 0 and d.lda == d.K
        pk = _Guarded(Gl * n1, band=NAN)
        for gi in range(Gl):
            rc = L.ivln_conv_pack_weights_f32(av.data_ptr() + 4 * gi * d.M * d.K, d.M, d.Cin, KS, pk.mid.data_ptr() + 4 * gi * n1, None)
            assert rc == 0
        torch.cuda.synchronize()
        assert not bool(torch.isnan(pk.mid).any()), tag   # (the pack is written whole: a NaN left would hide a read of it)
        keep.append(pk)
        g.A_packed, g.a_packed_grp_stride = pk.mid.data_ptr(), n1
    # B: the images in_img_stride floats apart, NaN between them
    per_img = d.Cin * d.Hin * d.Win
    Bd = torch.full((nimg, d.in_img_stride), NAN)
    Bd[:, :per_img] = t["x"][sl].reshape(nimg, per_img)
    kb, bv = _operand(Bd, off=0 if d.B_al else 1)
    keep.append(kb)
    g.B, g.in_img_stride = bv.data_ptr(), d.in_img_stride
    if d.bmode in ("conv", "convt"):
        koff, kpos = ops.conv_tables(d.Cin, d.KH, d.KW, d.Hin, d.Win, d.dil, torch.device(DEV), transposed=d.bmode == "convt")
        ko, kov = _operand(koff.cpu(), band=IBAND, dtype=torch.int32)
        kp, kpv = _operand(kpos.cpu(), band=IBAND, dtype=torch.int32)
        keep += [ko, kp]
        g.koff, g.kpos = kov.data_ptr(), kpv.data_ptr()
    # D: (imgs, Ctot, Ho, Wo), the launch's channels at C0 of a wider tensor (full form) or the whole of it
    _, Cd, Ho, Wo = t["out_shape"]
    Ctot = d.Ctot
    c0 = P.C0 if Ctot > Cd else 0
    out = _Guarded(nimg * Ctot * Ho * Wo, fill=SENT, off=0 if d.D_al else 1)
    ov = out.mid.view(nimg, Ctot, Ho, Wo)
    ov[:, c0:c0 + Cd] = _dev(t["d0"][sl]) if d.acc else (NAN if marker is None else _dev(marker[sl]))
    before = ov.clone()
    g.D, g.Ctot = ov[0, c0].data_ptr(), Ctot
    if d.dmode == "up2":
        g.sDm, g.sDn = d.cls
    cs = slice(0, G * d.C) if only_group is None else slice(only_group * d.C, (only_group + 1) * d.C)
    if d.has_scale:
        ks, sv = _operand(t["scale"][cs])
        keep.append(ks)
        g.scale = sv.data_ptr()
    if d.has_shift:
        kh, hv = _operand(t["shift"][cs])
        keep.append(kh)
        g.shift = hv.data_ptr()
    if d.has_res:   # the residual has the destination's layout: the same channel slice of a tensor as wide
        R = torch.full((nimg, Ctot, Ho, Wo), NAN)
        R[:, c0:c0 + Cd] = t["res"][sl, P.C0:P.C0 + Cd]
        kr, rv = _operand(R)
        keep.append(kr)
        g.residual = rv.view(nimg, Ctot, Ho, Wo)[0, c0].data_ptr()
    g.relu, g.accumulate = int(d.relu), int(d.acc)
    ws = None
    if d.ws:
        nws = d.ws_floats // d.nimg * nimg
        ws = _Guarded(nws)
        g.ws, g.ws_floats = ws.mid.data_ptr(), nws
    st = None
    if d.stats:
        st = _Guarded(max(getattr(P.plan(c, form=form), "stat_tiles", 0), 2) * d.M * 3)
        g.stat_partials, g.stat_tiles = st.mid.data_ptr(), C.pointer(ntiles)
    if d.flags is not None:
        kf, fv = _operand(torch.tensor(d.flags, dtype=torch.int32), band=IBAND, dtype=torch.int32)
        keep.append(kf)
        g.img_run_flags = fv.data_ptr()
    ops.gemm(g)
    torch.cuda.synchronize()
    assert out.bands_ok() and (ws is None or ws.bands_ok()) and (st is None or st.bands_ok()), f"{tag}: written outside a buffer's extent"
    assert _same_bytes(ov[:, :c0], before[:, :c0]) and _same_bytes(ov[:, c0 + Cd:], before[:, c0 + Cd:]), f"{tag}: written outside the channel slice"
    res = dict(out=ov[:, c0:c0 + Cd].clone(), before=before[:, c0:c0 + Cd], splits_used=used.value, stat_tiles=ntiles.value,
               stats=None if st is None else st.mid.clone(), slabs=None)
    if ws is not None and used.value >= 1 and (used.value > 1 or d.defer):
        res["slabs"] = ws.mid[:used.value * d.M * g.N].view(used.value, d.M, g.N).clone()
        assert bool(torch.isnan(ws.mid[used.value * d.M * g.N:]).all()), f"{tag}: more slabs written than splits_used"
    return res


def _dev(t):
    return t.to(DEV).contiguous()


def _picked(c, r):
    """the part of the slice the launch writes: all of it, or (UP2) its parity class - the rest must keep its bytes"""
    d = P.desc(c)
    if d.dmode != "up2":
        return r["out"]
    a, b = d.cls
    mask = torch.zeros_like(r["out"], dtype=torch.bool)
    mask[:, :, a::2, b::2] = True
    assert _same_bytes(torch.where(mask, 0.0, r["out"]), torch.where(mask, 0.0, r["before"])), f"{c['tag']}: written outside the parity class"
    return r["out"][:, :, a::2, b::2]


def _run(c, form, bar, check=True, **kw):
    """the launch twice under the timing sink, held to the plan; the result against float64"""
    p = P.plan(c, form=form)
    assert p.ok, (c["tag"], p.why)
    res = []

    def once():
        r = _launch(c, form, **kw)
        res.append(r)
        return (r["out"],) + tuple(r[k] for k in ("stats", "slabs") if r[k] is not None)

    _, ran = _observed(lambda: _twice(once))
    r = res[0]
    assert ran == {p.kernel: 2}, (c["tag"], ran, p.kernel)
    assert r["splits_used"] == p.splits, (c["tag"], r["splits_used"], p.splits)
    if P.desc(c, form).stats:
        assert r["stat_tiles"] == p.stat_tiles, (c["tag"], r["stat_tiles"], p.stat_tiles)
    if check:
        r64, r32 = _refs(c["tag"], form, p.k_step if p.splits > 1 else 0)
        bar.check(f"{form[:5]} s{p.splits}", _picked(c, r), r64, r32)
    return r, p


def _case_test(tag, forms=P.FORMS):
    c = _case(tag)
    bar = _Bar(tag, LOG)
    for form in forms:
        _run(c, form, bar)
    bar.done()


def _tags(cases):
    return [c["tag"] for c in cases]


# ------------------------------------------------------------------------------------------------------------------
# the tests: every instantiation, plain and full
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", _tags(P.GEMM_CASES))
def test_scalar_gather_gemm_every_tile_and_conv_mode(tag):
    """k_gemm: the five block tiles x the six conv operand modes; M and N one short of, equal to and one past the tile; 1 ... 4 K
    tiles per split, a ragged K tile, a short last split, empty trailing splits; pads 0 / 1 / KS - 1, stride 2 over odd inputs,
    dilation 2, KH != KW, transposed convs with and without output padding, the 2x2 window's zero row and column"""
    _case_test(tag)


@pytest.mark.parametrize("tag", _tags(P.VEC_CASES))
def test_vector_load_gemm_conv1x1_forms(tag):
    """k_gemm_vec: its three reachable tiles, stride 1 and the two-columns-per-load stride-2 form, the three epilogues"""
    _case_test(tag)


@pytest.mark.parametrize("tag", _tags(P.DIRECT_CASES))
def test_direct_conv_every_pixel_tile(tag):
    """k_conv_direct: (3x3, 7x7) x (stride 1, 2) and 2x2 on the four pixel tiles with ragged rows, columns and images, WM 1 / 2,
    the stems' ragged channel chunk, chunk splits, the wide epilogues and their scalar fall-backs"""
    _case_test(tag)


@pytest.mark.parametrize("tag", _tags(P.STREAM_CASES))
def test_streaming_conv1x1_every_k_and_wave_grid(tag):
    _case_test(tag)


@pytest.mark.parametrize("tag", _tags(P.PACKED_CASES))
def test_packed_weights_equal_unpacked_bit_for_bit(tag):
    """A_packed on the direct and the streaming kernel: the bar, and the unpacked launch's bytes.  K = 64 with an odd number of
    32-row tiles is the shape whose last wave read past the pack before the clamp"""
    _case_test(tag)
    c = _case(tag)
    for form in P.FORMS:
        a, b = _launch(c, form), _launch(dict(c, packed=False), form)
        assert _same_bytes(a["out"], b["out"]), (tag, form)


@pytest.mark.parametrize("tag", _tags(P.REDUCE_CASES))
def test_split_k_reductions_nchw_forms(tag):
    """k_splitk_epilogue (NCHW with HoWo % 4 != 0, UP2, UP2X4, no_wide_epilogue) and k_splitk_epilogue4 (with and without image
    groups) behind two slabs: the slabs summed in float64 against the raw product too"""
    _case_test(tag)
    c = _case(tag)
    r, p = _run(c, "plain", _Bar(tag, LOG), check=False)
    assert p.reduce is not None and r["slabs"].shape[0] == p.splits == 2
    raw64 = _raw(c, torch.float64).permute(1, 0, 2, 3).reshape(c["M"], -1)
    bar = _Bar(tag, LOG)
    bar.check("slab sum", r["slabs"].cpu().double().sum(0), raw64, _raw_chunked(c, p.k_step).permute(1, 0, 2, 3).reshape(c["M"], -1))
    bar.done()


@pytest.mark.parametrize("tag", _tags(P.UP2_CASES))
def test_up2_scatter_writes_one_parity_class(tag):
    _case_test(tag)


@pytest.mark.parametrize("tag", [c["tag"] for c in P.FORM_CASES if c["kind"] in ("shift", "acc")])
def test_shift_without_scale_and_accumulate(tag):
    _case_test(tag, forms=("shift", "full") if _case(tag)["tag"].startswith("f-shift") else P.FORMS)


@pytest.mark.parametrize("tag", [c["tag"] for c in P.FORM_CASES if c["kind"] == "defer"])
def test_deferred_epilogue_leaves_raw_slabs(tag):
    c = _case(tag)
    bar = _Bar(tag, LOG)
    r, p = _run(c, "plain", bar, check=False)
    assert r["slabs"].shape[0] == r["splits_used"] == p.splits == p.slabs
    assert _same_bytes(r["out"], r["before"]), f"{tag}: a deferred launch wrote its destination"
    M = c["M"]
    raw64 = _raw(c, torch.float64).permute(1, 0, 2, 3).reshape(M, -1)
    raw32 = _worse(raw64, *(v.permute(1, 0, 2, 3).reshape(M, -1) for v in (_raw(c, torch.float32), _raw_chunked(c, p.k_step))))
    bar.check(f"slabs s{p.splits}", r["slabs"].cpu().double().sum(0), raw64, raw32)
    bar.done()


@pytest.mark.parametrize("tag", [c["tag"] for c in P.FORM_CASES if c["kind"] == "grp"])
def test_image_grouped_weights_equal_one_launch_per_weight_set(tag):
    c = _case(tag)
    _case_test(tag)
    per = c["grp"]
    for form in P.FORMS:
        whole = _launch(c, form)["out"]
        for gi in range(c["imgs"] // per):
            part = _launch(c, form, only_group=gi)["out"]
            assert _same_bytes(whole[gi * per:(gi + 1) * per], part), (tag, form, gi)


@pytest.mark.parametrize("tag,kind", [(c["tag"], c["kind"]) for c in P.FORM_CASES if c["kind"] in ("nwe", "noxcd")])
def test_switches_change_no_byte(tag, kind):
    """no_wide_epilogue (vec NCHW, vec UP2X4, direct NCHW, direct UP2X4, k_splitk_epilogue4 -> k_splitk_epilogue) and
    no_xcd_remap (a grid of 17 workgroups on each kernel that remaps): the same bytes as the default"""
    c = _case(tag)
    other = dict(c, **{kind: True})
    bar = _Bar(tag + " " + kind, LOG)
    for form in P.FORMS:
        p, q = P.plan(c, form=form), P.plan(other, form=form)
        assert q.ok and q.kernel == p.kernel and q.splits == p.splits
        a, _ = _run(c, form, bar)
        r64, r32 = _refs(tag, form, p.k_step if p.splits > 1 else 0)
        b = _launch(other, form)
        bar.check(f"{form[:5]} {kind}", _picked(c, b), r64, r32)
        assert _same_bytes(a["out"], b["out"]), (tag, kind, form)
    bar.done()


@pytest.mark.parametrize("tag", _tags(P.FLAG_CASES))
def test_img_run_flags_skip_whole_tiles_only(tag):
    c = _case(tag)
    d = P.desc(c)
    bar = _Bar(tag, LOG)
    marker = _tensors(tag)["d0"] * 0 + 3.25
    for form in P.FORMS:
        p = P.plan(c, form=form)
        BN = P.TILES[p.tile][1]
        r, _ = _run(c, form, bar, check=False, marker=marker)
        r64, r32 = _refs(tag, form, 0)
        cols = torch.tensor([p.runs[n // BN] for n in range(d.N)]).view(d.nimg, 1, d.Hout, d.Wout).expand_as(r["out"])
        assert _same_bytes(torch.where(cols.to(DEV), 0.0, r["out"]), torch.where(cols.to(DEV), 0.0, r["before"])), f"{tag}: a skipped tile was written"
        if any(p.runs):
            sel = cols.reshape(-1)
            bar.check(f"{form[:5]} ran", r["out"].cpu().reshape(-1)[sel], r64.reshape(-1)[sel], r32.reshape(-1)[sel])
        else:
            assert _same_bytes(r["out"], r["before"])
    bar.done()


@pytest.mark.parametrize("tag", _tags(P.STAT_CASES))
def test_direct_conv_statistics_partials(tag):
    """stat_partials through ivln_bn_stats_from_partials_f32 (momentum 1: running_mean = the mean, running_var = the unbiased
    variance) against float64 statistics of the values the launch stored; the counts of the partials sum to the pixel count.
    The scalar epilogue (odd width, splits): *stat_tiles = 0 and the partials keep their bytes"""
    from ivln_ce_amd import ops
    from ivln_ce_amd._lib import check, stream_ptr

    c = _case(tag)
    M = c["M"]
    bar = _Bar(tag, LOG)
    for form in P.FORMS:
        r, p = _run(c, form, bar)
        if p.stat_tiles == 0:
            assert r["stat_tiles"] == 0 and bool(torch.isnan(r["stats"]).all()), tag
            continue
        parts = r["stats"][:p.stat_tiles * M * 3].contiguous()
        assert bool(torch.isnan(r["stats"][p.stat_tiles * M * 3:]).all())
        y = r["out"].cpu().permute(1, 0, 2, 3).reshape(M, -1)
        assert bool((parts.view(p.stat_tiles, M, 3)[:, :, 0].sum(0).cpu() == y.shape[1]).all()), tag
        one, zero = torch.ones(M, device=DEV), torch.zeros(M, device=DEV)
        rmean, rvar, sc, sh = (torch.zeros(M, device=DEV) for _ in range(4))
        L = ops._L()
        L.ivln_bn_stats_from_partials_f32.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_float] * 2 + [C.c_void_p] * 5
        check(L.ivln_bn_stats_from_partials_f32(parts.data_ptr(), p.stat_tiles, M, one.data_ptr(), zero.data_ptr(), rmean.data_ptr(),
                                                rvar.data_ptr(), 1.0, 0.0, sc.data_ptr(), sh.data_ptr(), None, None, stream_ptr()),
              "ivln_bn_stats_from_partials_f32")
        torch.cuda.synchronize()
        y64 = y.double()
        # (a tile's mean is a sum of <= 128 stored values over their count: it rounds at the values' magnitude, not the mean's)
        bar.check(f"{form[:5]} mean", rmean, y64.mean(1), y.mean(1), mag=float(y64.abs().max()))
        bar.check(f"{form[:5]} var", rvar, y64.var(1), y.var(1))
    bar.done()


@pytest.mark.parametrize("tag", [c["tag"] for c, _ in P.REFUSALS])
def test_refusals_are_the_launchers_own(tag):
    """the launcher's return code, no family launch, the destination's bytes unchanged"""
    from ivln_ce_amd._lib import IvlnError

    c = _case(tag)
    code = dict((k["tag"], v) for k, v in P.REFUSALS)[tag]
    for form in P.FORMS:
        p = P.plan(c, form=form)
        assert not p.ok and p.code == code

        def attempt():
            with pytest.raises(IvlnError, match=r"\(%d\)" % RC[code]):
                _launch(c, form)

        _, ran = _observed(attempt)
        assert ran == {}, (tag, ran)
