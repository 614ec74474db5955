"""Per-kernel GPU parity of csrc/conv_bf3.hip - k_conv_bf3 (tiled: stride 1 and 2, slabs over blockIdx.z, the fused
bottleneck tail), k_conv_bf3_ks, k_conv1x1_bf3_ks, k_conv7_pool_bf3, k_conv7s2_bf3, k_wgrad_bf3 - each alone behind
ivln_gemm_f32, at the smallest shapes that reach every tile's ragged edges (tests/test_conv_bf3_plan_coverage.py holds the case
tables and asserts the edges on the CPU), against the same operation in plain torch float64 on the CPU: F.conv2d,
F.conv_transpose2d for the 2 x 2-block stores, F.avg_pool2d(F.relu(...)) for the pooled block, autograd of F.conv2d for the
weight gradient, the two-conv composition for the fused tail.  ops.GemmDesc is filled here and handed to ops.gemm, so this
file owns every buffer; ops.conv2d's Python gates (Cin >= 128, 2^18 outputs, ...) are not in the way of the small shapes.

Inputs are drawn in fp32 from a seeded generator and widened for the reference.  Two input sets per case: `dense`, and
`single_tap` (one non-zero weight per output channel - every output is ONE product, so a lost piece product is 8 ... 10 bars
off: the CPU file shows it on the emulation).  Error bar: _Bar.check of tests/kernel_bar.py, unchanged:
4 * e32 + 4 * 2^-24 * max|float64| with e32 the error of the same torch ops in fp32 on the CPU.  Every comparison goes to
conv_bf3_kernels.log in the suite's log directory before anything is asserted.

Every destination (D, a Ctot-wider D written as a channel slice, stat_partials, the dense dW) starts as NaN between two bands
of sentinels (and sentinels in the channels beside the slice): an element never written fails the bar, one written outside
fails the band.  Every launch runs twice (_twice) and must give the same bytes.  Observed and held to the restated plan for
the device's CU count: the kernel name (family timing sink), ivln_gemm_desc.splits_used, the delta of ivln_conv_split_kinds
(the weight-gradient launcher does not tally), *stat_tiles, accepted versus refused (refusals only through the launcher's
return code: nothing here launches past a predicate).

Epilogue forms: every instantiation runs `plain` (no epilogue operand) and `full` (scale + shift + residual + ReLU into a
channel slice of a wider destination, the input's image stride padded); accumulate, image-grouped weights (== one launch per
weight set, bit for bit) and no_wide_epilogue (== the wide epilogue, bit for bit) on the cases that name them.

Measured on an MI355X (256 CUs; 201 tests, 700 comparisons, none OVER, 6 s for the file): the largest hip / e32 ratios are
all on `single_tap`, where e32 is one fp32 rounding of one product - k_conv_bf3 2.67 (k3-c2-w36 plain: err 7.3e-07, bar
3.5e-06), k_wgrad_bf3 2.49 (wg-six-w16, three slabs), k_conv7_pool_bf3 2.30 (pool-nw4-12x16), k_conv_bf3_ks 2.28 (ks14-w16),
k_conv1x1_bf3_ks 2.16 (x1-12-up), k_conv7s2_bf3 1.96 (stem-c1); the merged statistics partials 1.17 (stats-k7-c4-w8 mean).
On `dense` the largest is 2.19 (k7-c2-w12 full: err 7.1e-06, bar 1.5e-05).  The first run found one defect, in the launcher, not in a kernel: x1-12-up (five chunks
pinned to the K-split form, 2 x 2-block stores) was tallied by ivln_conv_split_kinds as wave tiles - the tally was worked out
from the chunk count beside the launcher; bf3_1x1_ks_launch now reports the form it launched (the CPU file's kind_parent keeps
the old rule and shows which production shape it miscounted).  A second one showed in the whole suite: see
test_timing_sink_keeps_each_armings_own_launch_limit.  A scratch build with ONE piece product dropped (a1b3 out of
bf3_products) fails 176 of the 201 tests: every one that compares a launch with float64 except the three whose kernels never
issue that product (the u8 map form and the one-piece weight gradient: x is exact in bf16, its third piece is zero).  The
first version of the weight gradient's `single_tap` set left dy all zero for more than one image; that run showed it (five
cases passed the mutation), hence the non-zero count asserted in _tensors."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import test_conv_bf3_plan_coverage as P
from kernel_bar import _Bar, _same_bytes, _twice

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOG = "conv_bf3_kernels.log"
E_UNSUPPORTED = -5
SENT, PAD, NAN = -777.0, 8, float("nan")
SETS = ("dense", "single_tap")
C0 = 4   # first channel of the slice in the `full` form's wider destination (Ctot = M + 8)


def _observed(fn):
    from test_gpu_train_gemms import _observed as obs

    return obs(fn)


@functools.lru_cache(maxsize=None)
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _seed(c, which):
    s = 17 if which == "dense" else 29
    for ch in c["tag"]:
        s = (s * 131 + ord(ch)) % (2 ** 31)
    return s


# ------------------------------------------------------------------------------------------------------------------
# inputs and references (CPU)
# ------------------------------------------------------------------------------------------------------------------
def _single_tap(w, g):
    """one non-zero weight per output channel (of each weight set), |w| >= 0.5, channel and tap varying with the channel"""
    M, Cin, KH, KW = w.shape[-4:]
    keep = torch.zeros_like(w)
    m = torch.arange(M)
    ci, tap = (m * 5 + 3) % Cin, (m * 7 + 1) % (KH * KW)
    keep[..., m, ci, tap // KW, tap % KW] = 1.0
    return w * keep + keep * 0.5 * torch.sign(w)


def _tensors(c, which):
    """the case's operands in fp32 on the CPU (one draw per case and input set)"""
    g = torch.Generator().manual_seed(_seed(c, which))
    d = P.desc(c)
    kind, KS, imgs, M, Cin = d.kind, d.KS, d.nimg, d.M, d.Cin
    G = imgs // d.grp_imgs if d.grp_imgs else 1
    t = dict(G=G)
    if kind == "wgrad":
        x = torch.randn(imgs, Cin, d.Hin, d.Win, generator=g)
        if d.split_ok == 2:
            x = x.bfloat16().float()   # the caller's promise: exact in bf16
        dy = torch.randn(imgs, M, d.Hout, d.Wout, generator=g)
        if which == "single_tap":   # one non-zero pixel of dy per channel: every dW element is one product (or zero)
            keep = torch.zeros(M, imgs * d.HoWo)
            m = torch.arange(M)
            keep[m, (m * 37 + 5) % (imgs * d.HoWo)] = 1.0
            keep = keep.reshape(M, imgs, d.Hout, d.Wout).permute(1, 0, 2, 3)
            dy = dy * keep + keep * 0.5 * torch.sign(dy)
            assert int((dy != 0).sum()) == M
        else:
            dy = dy / (imgs * d.HoWo) ** 0.5
        t.update(x=x, dy=dy)
        return t
    if d.u8:
        t["occ"] = torch.randint(0, 256, (imgs, d.Hin, d.Win), generator=g, dtype=torch.uint8)
        t["sem"] = torch.randint(0, 16, (imgs, d.Hin, d.Win), generator=g, dtype=torch.uint8)   # (13 ... 15: no class)
        x = torch.cat([t["occ"].float()[:, None]] + [(t["sem"] == k).float()[:, None] for k in range(13)], 1)
    else:
        x = torch.randn(imgs, Cin, d.Hin, d.Win, generator=g)
    w = torch.randn(G, M, Cin, KS, KS, generator=g)
    w = _single_tap(w, g) if which == "single_tap" else w / (Cin * KS * KS) ** 0.5
    C_ep = M // 4 if d.up else M   # channels of the epilogue's scale / shift
    t.update(x=x, w=w, scale=torch.rand(G * C_ep, generator=g) + 0.5, shift=torch.randn(G * C_ep, generator=g) * 0.3)
    Cd = d.fuse_M if kind == "fused" else C_ep
    Ho, Wo = (2 * d.Hout, 2 * d.Wout) if d.up else ((d.Hout // 2, d.Wout // 2) if kind == "pool" else (d.Hout, d.Wout))
    t["out_shape"] = (imgs, Cd, Ho, Wo)
    t["res"] = torch.randn(imgs, Cd + 8, Ho, Wo, generator=g)   # as wide as the widest destination: the slice's channels are used
    t["d0"] = torch.randn(imgs, Cd, Ho, Wo, generator=g)        # the destination's contents for `accumulate`
    if kind == "fused":
        w3 = torch.randn(G, d.fuse_M, M, 1, 1, generator=g)
        t["w3"] = _single_tap(w3, g) if which == "single_tap" else w3 / M ** 0.5
        t["scale3"], t["shift3"] = torch.rand(G * d.fuse_M, generator=g) + 0.5, torch.randn(G * d.fuse_M, generator=g) * 0.3
    return t


def _up_weight(w, KS):
    """the stacked classes (4 C, Cin, KS, KS), rows 4 c + 2 a + b, as the transposed conv they are: KS 1 -> (Cin, C, 2, 2),
    stride 2; KS 2 -> (Cin, C, 4, 4), stride 2, padding 2 over the input with one zero row / column behind it (output row
    2 h + a takes input row h + kh through tap a - 2 kh + 2)"""
    M, Cin = w.shape[:2]
    ws = w.reshape(M // 4, 2, 2, Cin, KS, KS)   # c a b ci kh kw
    if KS == 1:
        return ws[..., 0, 0].permute(3, 0, 1, 2).contiguous()
    wt = torch.zeros(Cin, M // 4, 4, 4, dtype=w.dtype)
    for a in (0, 1):
        for b in (0, 1):
            for kh in (0, 1):
                for kw in (0, 1):
                    wt[:, :, a - 2 * kh + 2, b - 2 * kw + 2] = ws[:, a, b, :, kh, kw].t()
    return wt


def _conv(c, t, dt):
    """the bare operation in dtype dt: (imgs, C, Ho, Wo)"""
    d = P.desc(c)
    x, w = t["x"].to(dt), t["w"].to(dt)
    per = d.nimg // t["G"]
    outs = []
    for g in range(t["G"]):
        xg, wg = x[g * per:(g + 1) * per], w[g]
        if d.up:
            if d.KS == 2:
                xg = F.pad(xg, (0, 1, 0, 1))
            outs.append(F.conv_transpose2d(xg, _up_weight(wg, d.KS), stride=2, padding=2 if d.KS == 2 else 0))
        else:
            outs.append(F.conv2d(xg, wg, stride=d.stride, padding=d.pad))
    return torch.cat(outs, 0)


def _per_image(v, c, t, Cc):
    """scale / shift (G * Cc) -> (imgs, Cc, 1, 1): image i uses weight set i / grp_imgs"""
    d = P.desc(c)
    per = d.nimg // t["G"]
    return v.reshape(t["G"], Cc).repeat_interleave(per, 0)[:, :, None, None]


def _reference(c, which, form, dt):
    """the launch's result in dtype dt: conv, then the form's epilogue in the kernels' order of operations
    (scale / shift, residual, D +=, ReLU; residual_after_relu: behind the ReLU)"""
    d, t = P.desc(c, form), _tensors(c, which)
    if d.kind == "wgrad":
        x = t["x"].to(dt)
        w0 = torch.zeros(d.M, d.Cin, 7, 7, dtype=dt, requires_grad=True)
        F.conv2d(x, w0, padding=3).backward(t["dy"].to(dt))
        return w0.grad.reshape(d.M, d.Cin * 49)
    y = _conv(c, t, dt)
    Cc = y.shape[1]
    if d.kind == "fused":   # relu(bn2(conv3x3)) -> conv1x1 -> bn3 -> + residual -> relu
        y = torch.relu(y * _per_image(t["scale"].to(dt), c, t, Cc) + _per_image(t["shift"].to(dt), c, t, Cc))
        per = d.nimg // t["G"]
        y = torch.cat([F.conv2d(y[g * per:(g + 1) * per], t["w3"][g].to(dt)) for g in range(t["G"])], 0)
        y = y * _per_image(t["scale3"].to(dt), c, t, d.fuse_M) + _per_image(t["shift3"].to(dt), c, t, d.fuse_M)
        return torch.relu(y + t["res"][:, C0:C0 + d.fuse_M].to(dt))
    if d.has_scale:
        y = y * _per_image(t["scale"].to(dt), c, t, Cc) + _per_image(t["shift"].to(dt), c, t, Cc)
    res = t["res"][:, C0:C0 + Cc].to(dt) if d.has_res else None
    if d.kind == "pool":
        return F.avg_pool2d(torch.relu(y), 2)
    if res is not None and not d.post:
        y = y + res
    if d.accumulate:
        y = y + t["d0"].to(dt)
    if d.relu:
        y = torch.relu(y)
    if res is not None and d.post:
        y = y + res
    return y


@functools.lru_cache(maxsize=None)
def _refs(tag, which, form):
    c = _case(tag)
    return _reference(c, which, form, torch.float64), _reference(c, which, form, torch.float32)


@functools.lru_cache(maxsize=None)
def _all_cases():
    return {c["tag"]: c for c in P.launch_cases(_cus()) + P.REFUSALS}


def _case(tag):
    return _all_cases()[tag]


# ------------------------------------------------------------------------------------------------------------------
# one launch
# ------------------------------------------------------------------------------------------------------------------
class _Guarded:
    """n floats between two bands of PAD sentinels; the n start as `fill` (NaN unless the launch accumulates)"""

    def __init__(self, n, fill=NAN):
        self.buf = torch.full((n + 2 * PAD,), SENT, dtype=torch.float32, device=DEV)
        self.n = n
        self.mid[:] = fill

    @property
    def mid(self):
        return self.buf[PAD:PAD + self.n]

    def bands_ok(self):
        return bool((self.buf[:PAD] == SENT).all()) and bool((self.buf[PAD + self.n:] == SENT).all())


def _dev(t):
    return t.to(DEV).contiguous()


def _launch(c, which, form, only_group=None, nwe=None):
    """Fill the descriptor of (case, input set, form) from P.desc and the case's tensors, launch once, return
    dict(out=the written region as (imgs, C, Ho, Wo) | (M, N), splits_used, stat_tiles, stats, rc-free) - raises IvlnError on a
    refusal.  only_group = g: the launch for weight set g alone (its images, its weights, no grp_imgs)."""
    from ivln_ce_amd import ops

    d, t = P.desc(c, form), _tensors(c, which)
    keep = []   # device tensors the descriptor points into
    g = ops.GemmDesc()
    used, ntiles = ops.i32(-1), ops.i32(-1)
    g.splits_used = C.pointer(used)
    g.M, g.N, g.K = d.M, d.N, d.K
    g.Cin, g.Hin, g.Win, g.Hout, g.Wout = d.Cin, d.Hin, d.Win, d.Hout, d.Wout
    g.stride, g.pad, g.dil, g.HoWo = d.stride, d.pad, 1, d.HoWo
    g.tile_override, g.splits, g.no_wide_epilogue = d.ov, d.splits, int(d.nwe if nwe is None else nwe)
    if d.kind == "wgrad":
        x, dy = _dev(t["x"]), _dev(t["dy"])
        out = _Guarded(d.M * d.N)
        ws = _Guarded(d.ws_floats) if d.ws else None
        koff, kpos = ops.conv_tables(d.Cin, 7, 7, d.Hin, d.Win, 1, torch.device(DEV))
        keep += [x, dy, koff, kpos]
        g.A, g.B, g.D = dy.data_ptr(), x.data_ptr(), out.mid.data_ptr()
        g.amode, g.bmode, g.dmode = ops.A_NCHW_P, ops.B_IM2COL_T, ops.D_DENSE
        g.sDm, g.sDn, g.koff, g.kpos, g.split_ok = d.N, 1, koff.data_ptr(), kpos.data_ptr(), d.split_ok
        if ws is not None:
            g.ws, g.ws_floats = ws.mid.data_ptr(), d.ws_floats
        ops.gemm(g)
        torch.cuda.synchronize()
        assert out.bands_ok() and (ws is None or ws.bands_ok()), f"{c['tag']}: written outside dW or the workspace"
        return dict(out=out.mid.reshape(d.M, d.N).clone(), splits_used=used.value)
    G = t["G"]
    per = d.nimg // G
    sl = slice(0, d.nimg) if only_group is None else slice(only_group * per, (only_group + 1) * per)
    nimg = sl.stop - sl.start
    w = t["w"] if only_group is None else t["w"][only_group:only_group + 1]
    Gl = w.shape[0]
    g.N = nimg * d.HoWo
    # B: the images `in_img_stride` floats apart (padded in the `full` form), optionally four bytes off a 16-byte boundary
    if d.u8:
        occ, sem = _dev(t["occ"][sl]), _dev(t["sem"][sl])
        keep += [occ, sem]
        g.B, g.map_sem_u8 = occ.data_ptr(), sem.data_ptr()
    else:
        per_img = d.Cin * d.Hin * d.Win
        xb = torch.full((nimg * d.in_img_stride + 4,), SENT, dtype=torch.float32, device=DEV)
        off = 1 if not d.B_al else 0
        xv = xb[off:off + nimg * d.in_img_stride].view(nimg, d.in_img_stride)
        xv[:, :per_img] = _dev(t["x"][sl]).reshape(nimg, per_img)
        keep.append(xb)
        g.B, g.in_img_stride = xv.data_ptr(), d.in_img_stride
    wd = _dev(w if Gl > 1 else w[0])
    stem = d.KS == 7 and d.stride == 2
    sp = ops.packed_conv_weights(wd, cache=False, split="stem" if stem else True)
    assert sp is not None
    keep += [wd, sp]
    g.A, g.lda, g.A_split, g.a_split_grp_stride = wd.data_ptr(), d.K, sp.data_ptr(), sp.numel() // Gl
    g.amode = ops.A_MK
    g.bmode = {1: ops.B_CONV1X1, 2: ops.B_CONV_K2, 3: ops.B_CONV_K3, 7: ops.B_CONV_K7}[d.KS]
    g.dmode = ops.D_NCHW_UP2X4 if d.up else ops.D_NCHW
    if d.grp_imgs and only_group is None:
        g.grp_imgs, g.a_grp_stride = d.grp_imgs, d.M * d.K
    # D: (imgs, Ctot, Ho, Wo) with the launch's channels at C0 (full form: Ctot = C + 8) or at 0
    _, Cd, Ho, Wo = t["out_shape"]
    Ctot = d.Ctot
    c0 = C0 if Ctot > Cd else 0
    out = _Guarded(nimg * Ctot * Ho * Wo, fill=SENT)
    ov = out.mid.view(nimg, Ctot, Ho, Wo)
    ov[:, c0:c0 + Cd] = _dev(t["d0"][sl]) if d.accumulate else NAN
    g.D, g.Ctot = ov[0, c0].data_ptr(), Ctot
    Cs = d.M // 4 if d.up else d.M
    gs = slice(0, G * Cs) if only_group is None else slice(only_group * Cs, (only_group + 1) * Cs)
    if d.has_scale:
        sc, sh = _dev(t["scale"][gs]), _dev(t["shift"][gs])
        keep += [sc, sh]
        g.scale, g.shift = sc.data_ptr(), sh.data_ptr()
    if d.has_res:   # the residual has the destination's layout: the same channel slice of a tensor as wide
        rw = _dev(t["res"][sl, C0 - c0:C0 - c0 + Ctot])
        keep.append(rw)
        g.residual = rw[0, c0].data_ptr()
    g.relu, g.accumulate, g.residual_after_relu = int(d.relu), int(d.accumulate), int(d.post)
    ws = None
    if d.ws:
        ws = _Guarded(d.ws_floats)
        g.ws, g.ws_floats = ws.mid.data_ptr(), d.ws_floats
    st = None
    if d.stats:
        p = P.plan(c, _cus(), form)
        st = _Guarded(max(p.stat_tiles, 1) * d.M * 3)
        g.stat_partials, g.stat_tiles = st.mid.data_ptr(), C.pointer(ntiles)
    if d.pool2:
        g.pool2 = 1
    if d.kind == "fused":
        gf = slice(0, G * d.fuse_M) if only_group is None else slice(only_group * d.fuse_M, (only_group + 1) * d.fuse_M)
        w3 = t["w3"] if only_group is None else t["w3"][only_group:only_group + 1]
        w3d = _dev(w3 if Gl > 1 else w3[0])
        sp3 = ops.packed_conv_weights(w3d, cache=False, split=True)
        s3, h3 = _dev(t["scale3"][gf]), _dev(t["shift3"][gf])
        keep += [w3d, sp3, s3, h3]
        g.fuse_A_split, g.fuse_a_grp_stride, g.fuse_M = sp3.data_ptr(), sp3.numel() // Gl, d.fuse_M
        g.fuse_scale, g.fuse_shift = s3.data_ptr(), h3.data_ptr()
    ops.gemm(g)
    torch.cuda.synchronize()
    tag = c["tag"]
    assert out.bands_ok() and (ws is None or ws.bands_ok()) and (st is None or st.bands_ok()), f"{tag}: written outside a buffer's extent"
    assert bool((ov[:, :c0] == SENT).all()) and bool((ov[:, c0 + Cd:] == SENT).all()), f"{tag}: written outside the channel slice"
    return dict(out=ov[:, c0:c0 + Cd].clone(), splits_used=used.value, stat_tiles=ntiles.value,
                stats=None if st is None else st.mid.clone())


def _kinds():
    from ivln_ce_amd import ops

    L = ops._L()
    L.ivln_conv_split_kinds.argtypes = [C.POINTER(C.c_longlong), C.c_int]
    out = (C.c_longlong * 4)()
    assert L.ivln_conv_split_kinds(out, 0) == 0
    return list(out)


def _run(c, which, form, bar, **kw):
    """the launch twice under the timing sink, held to the plan; the result against float64"""
    p = P.plan(c, _cus(), form)
    assert p.ok, (c["tag"], p.why)
    res = []
    before = _kinds()

    def once():
        r = _launch(c, which, form, **kw)
        res.append(r)
        return (r["out"],) + ((r["stats"],) if r.get("stats") is not None else ())

    outs, ran = _observed(lambda: _twice(once))
    assert ran == {p.kernel: 2}, (c["tag"], ran, p.kernel)
    delta = [a - b for a, b in zip(_kinds(), before)]
    assert delta == [2 if i == p.kind else 0 for i in range(4)], (c["tag"], delta, p.kind)
    assert res[0]["splits_used"] == p.splits, (c["tag"], res[0]["splits_used"], p.splits)
    if "stat_tiles" in res[0] and P.desc(c, form).stats:
        assert res[0]["stat_tiles"] == p.stat_tiles, (c["tag"], res[0]["stat_tiles"], p.stat_tiles)
    if kw.get("only_group") is None:
        r64, r32 = _refs(c["tag"], which, form)
        bar.check(f"{which[:5]} {form[:5]} s{p.splits}", outs[0], r64, r32)
    return res[0], p


def _case_test(tag, forms=P.FORMS):
    c = _case(tag)
    bar = _Bar(tag, LOG)
    for which in SETS:
        for form in forms:
            _run(c, which, form, bar)
    bar.done()


def _tags(cases):
    return [c["tag"] for c in cases]


# ------------------------------------------------------------------------------------------------------------------
# the tests
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", _tags(P.TILED_CASES))
def test_tiled_kernel_every_tile_and_width_class(tag):
    """k_conv_bf3 at every (kernel size, block tile, width class, stride) the launcher accepts: two tile rows, a ragged image
    group, a masked channel tile, a ragged last chunk (1x1: a last stage of one chunk), both input sets, both epilogue forms"""
    _case_test(tag)


@pytest.mark.parametrize("tag", _tags(P.SLAB_CASES))
def test_tiled_kernel_slabs_over_blockidx_z(tag):
    """three slabs of one 16-channel chunk each (the last of 8 channels), reduced by k_splitk_epilogue4 or - no_wide_epilogue -
    by k_splitk_epilogue: the two reductions give the same bytes"""
    _case_test(tag)
    c = _case(tag)
    if not c["nwe"]:
        for form in P.FORMS:
            a, b = _launch(c, "dense", form, nwe=False), _launch(c, "dense", form, nwe=True)
            assert a["splits_used"] == b["splits_used"] == 3 and _same_bytes(a["out"], b["out"]), (tag, form)


def _chan_merge(parts):
    """(tiles, M, 3) partials {count, mean, M2} merged in float64 (Chan et al.) -> count, mean, M2 per channel"""
    n = torch.zeros(parts.shape[1], dtype=torch.float64)
    mean, m2 = n.clone(), n.clone()
    for part in parts.double().unbind(0):
        cnt, mu, q = part.unbind(1)
        tot = n + cnt
        delta = mu - mean
        f = torch.where(tot > 0, cnt / tot.clamp(min=1), torch.zeros_like(tot))
        mean = mean + delta * f
        m2 = m2 + q + delta * delta * n * f
        n = tot
    return n, mean, m2


@pytest.mark.parametrize("tag", [c["tag"] for c in P.EXTRA_TILED if c.get("stats")])
def test_tiled_kernel_statistics_partials(tag):
    """stat_partials: {count, mean, M2} per (128-pixel segment, channel) of what the launch stored; counts sum to the pixel count,
    the float64 merge matches the statistics of the kernel's own output"""
    c = _case(tag)
    bar = _Bar(tag, LOG)
    for which in SETS:
        for form in P.FORMS:
            r, p = _run(c, which, form, bar)
            M = c["M"]
            parts = r["stats"].cpu().reshape(p.stat_tiles, M, 3)
            n, mean, m2 = _chan_merge(parts)
            y = r["out"].cpu().permute(1, 0, 2, 3).reshape(M, -1)
            assert bool((n == y.shape[1]).all()), (tag, n)
            y64 = y.double()
            mean64, m264 = y64.mean(1), ((y64 - y64.mean(1, keepdim=True)) ** 2).sum(1)
            mean32, m232 = y.mean(1), ((y - y.mean(1, keepdim=True)) ** 2).sum(1)
            # (a segment's mean is a sum of 128 stored values over their count: it rounds at the values' magnitude, not the mean's)
            bar.check(f"{which[:5]} {form[:5]} mean", mean, mean64, mean32, mag=float(y64.abs().max()))
            bar.check(f"{which[:5]} {form[:5]} M2", m2, m264, m232)
    bar.done()


@pytest.mark.parametrize("tag", [c["tag"] for c in P.EXTRA_TILED + P.KS_CASES + P.X1_CASES + P.fused_cases(256) if c.get("grp")])
def test_image_grouped_weights_equal_one_launch_per_weight_set(tag):
    c = _case(tag)
    _case_test(tag)
    for form in P.FORMS:
        whole = _launch(c, "dense", form)["out"]
        per = c["grp"]
        for gi in range(c["imgs"] // per):
            part = _launch(c, "dense", form, only_group=gi)["out"]
            assert _same_bytes(whole[gi * per:(gi + 1) * per], part), (tag, form, gi)


@pytest.mark.parametrize("tag", [c["tag"] for c in P.EXTRA_TILED + P.KS_CASES + P.X1_CASES if c.get("acc")])
def test_accumulate_into_the_destination(tag):
    _case_test(tag)


@pytest.mark.parametrize("tag", [c["tag"] for c in P.fused_cases(256) if not c.get("grp")])
def test_fused_bottleneck_tail(tag):
    """k_conv_bf3<..., FUSE>: M = 64, M = 128 on 64-pixel tiles, M = 128 on 128-pixel tiles (the case sized from the CU count)"""
    _case_test(tag)


@pytest.mark.parametrize("tag", [c["tag"] for c in P.KS_CASES if not (c.get("grp") or c.get("acc"))])
def test_k_split_3x3_and_2x2_kernel(tag):
    """k_conv_bf3_ks: 32- and 64-pixel tiles at the three widths, 8 and 9 chunks over the 8 waves, a masked channel tile; the
    stacked 2 x 2 classes into 2 x 2 output blocks"""
    _case_test(tag)


@pytest.mark.parametrize("tag", [c["tag"] for c in P.X1_CASES if not (c.get("grp") or c.get("acc"))])
def test_1x1_kernels_both_forms(tag):
    """k_conv1x1_bf3_ks: the K-split form and the wave tiles; plain NCHW, residual behind the ReLU, 2 x 2-block stores; 4, 9 and
    17 chunks; a ragged last pixel tile, a masked channel tile"""
    _case_test(tag)


@pytest.mark.parametrize("tag", _tags(P.POOL_CASES))
def test_conv7_pool_kernel(tag):
    _case_test(tag)


@pytest.mark.parametrize("tag", _tags(P.STEM_CASES))
def test_stem_kernel_ragged_last_workgroup(tag):
    _case_test(tag)


@pytest.mark.parametrize("tag", _tags(P.WGRAD_CASES))
def test_weight_gradient_kernel(tag):
    """k_wgrad_bf3 against float64 autograd of F.conv2d: the five tile forms x four widths, ragged image pairs and strip slabs"""
    _case_test(tag, forms=("plain",))


@pytest.mark.parametrize("tag", _tags(P.REFUSALS))
def test_refusals_are_the_launchers_own(tag):
    """one shape inside and one outside each refusal reason: the launcher's return code, no launch, nothing written"""
    from ivln_ce_amd._lib import IvlnError

    c = _case(tag)
    forms = ("plain",) if c.get("kind") in ("pool", "wgrad") else P.FORMS
    if c["why"] is None:
        _case_test(tag, forms=forms)
        return
    for form in forms:
        p = P.plan(c, _cus(), form)
        assert not p.ok and p.code == "unsupported"
        before = _kinds()
        with pytest.raises(IvlnError, match=r"\(%d\)" % E_UNSUPPORTED):
            _observed(lambda: _launch(c, "dense", form))
        assert _kinds() == before


def test_timing_sink_keeps_each_armings_own_launch_limit():
    """What running this file in front of tests/test_gpu_kernels.py exposed: the sink's event pool keeps the largest arming's
    events, and ivln_family_timing_next counted against the pool - after an arming for 16 launches one for 2 timed a third.
    The limit is the arming's own now."""
    from ivln_ce_amd import ops
    from ivln_ce_amd._lib import check

    c = _case("k3-c4-w12")
    _observed(lambda: _launch(c, "dense", "plain"))   # (arms for 16 launches)
    L = ops._L()
    L.ivln_family_timing_begin.argtypes = [C.c_int]
    L.ivln_family_timing_end.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    check(L.ivln_family_timing_begin(2), "ivln_family_timing_begin")
    ms, n, dropped = C.c_double(0), C.c_int(0), C.c_int(0)
    try:
        outs = [_launch(c, "dense", "plain")["out"] for _ in range(3)]
    finally:
        rc = L.ivln_family_timing_end(C.byref(ms), C.byref(n), C.byref(dropped))
    check(rc, "ivln_family_timing_end")
    assert (n.value, dropped.value) == (2, 1)
    assert _same_bytes(outs[0], outs[1]) and _same_bytes(outs[0], outs[2])   # (timed or not: the same launch)


# ------------------------------------------------------------------------------------------------------------------
# the weight images
# ------------------------------------------------------------------------------------------------------------------
def _pieces_np(w):
    import numpy as np

    return [torch.from_numpy(np.ascontiguousarray(p)) for p in P.split3_np(w.numpy())]


@pytest.mark.parametrize("M,Cin,KS", [(40, 80, 1), (40, 24, 3), (40, 24, 7), (72, 17, 2)])
def test_split_weight_image(M, Cin, KS):
    """ivln_conv_split_weights_f32: [32-channel tile][16-channel chunk][tap, padded][piece][lane] x 8 bf16 (k_conv_bf3_pack) -
    every piece the numpy split3's, h + m + l == w exactly, padding taps / channels / rows zero"""
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(M * 100 + Cin * 10 + KS)
    w = torch.randn(M, Cin, KS, KS, generator=g) * torch.exp(2 * torch.randn(M, Cin, KS, KS, generator=g))
    sp = ops.packed_conv_weights(_dev(w), cache=False, split=True)
    torch.cuda.synchronize()
    KK, KKP, nch, mt = KS * KS, P.taps_padded(KS), P.cdiv(Cin, P.CB), P.cdiv(M, 32)
    assert sp.numel() == mt * nch * KKP * 3 * 1024 // 4
    img = sp.cpu().view(torch.int16).view(mt, nch, KKP, 3, 2, 32, 8)   # tile, chunk, tap, piece, half, l31, element
    vals = (img.to(torch.int32) << 16).view(torch.float32)                # a bf16 as the fp32 with the same upper bits
    # -> [piece][m][ci][tap], padded
    full = vals.permute(3, 0, 5, 1, 4, 6, 2).reshape(3, mt * 32, nch * 16, KKP)
    want = torch.zeros(3, mt * 32, nch * 16, KKP)
    for i, p in enumerate(_pieces_np(w.reshape(M, Cin, KK))):
        want[i, :M, :Cin, :KK] = p
    assert _same_bytes(full, want)
    assert bool((full.double().sum(0)[:M, :Cin, :KK] == w.reshape(M, Cin, KK).double()).all())


@pytest.mark.parametrize("M,Cin", [(40, 1), (40, 3)])
def test_stem_split_weight_image(M, Cin):
    """ivln_conv_stem_split_weights_f32: [32-channel tile][step][piece][lane] x 8 bf16, lane (l31, half) element j =
    W[32 mt + l31][kernel row 2 step + half][j], zero for j = 7 and rows past the last (k_conv7s2_pack)"""
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(M + Cin)
    w = torch.randn(M, Cin, 7, 7, generator=g) * torch.exp(2 * torch.randn(M, Cin, 7, 7, generator=g))
    sp = ops.packed_conv_weights(_dev(w), cache=False, split="stem")
    torch.cuda.synchronize()
    S, mt = (Cin * 7 + 1) // 2, P.cdiv(M, 32)
    assert sp.numel() == mt * S * 3 * 1024 // 4
    img = sp.cpu().view(torch.int16).view(mt, S, 3, 2, 32, 8)   # tile, step, piece, half, l31, element
    vals = (img.to(torch.int32) << 16).view(torch.float32)
    full = vals.permute(2, 0, 4, 1, 3, 5).reshape(3, mt * 32, 2 * S, 8)   # piece, m, kernel row, column
    want = torch.zeros(3, mt * 32, 2 * S, 8)
    for i, p in enumerate(_pieces_np(w.reshape(M, Cin * 7, 7))):
        want[i, :M, :Cin * 7, :7] = p
    assert _same_bytes(full, want)
    assert bool((full.double().sum(0)[:M, :Cin * 7, :7] == w.reshape(M, Cin * 7, 7).double()).all())
