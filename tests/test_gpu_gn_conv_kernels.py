"""Per-kernel GPU parity of csrc/gn_conv.hip - k_gn_conv behind ivln_gn_conv_f32 and k_nconv behind ivln_nconv_f32 - each
alone, at the smallest shapes that reach each edge of the launchers' plans (tile counts that are no power of two, streamed
weights, ragged channel slices, dropped `part` scratch, DPP-row and looped statistics merges, ...), against the same
operation written in plain torch in float64 on the CPU.  Nothing here imports oracle/, ivln_ce_amd.encoders or depth_net;
the descriptors are filled through ctypes so that this file owns every output buffer.

Inputs are drawn in fp32 from a seeded generator and widened for the reference.  Error bar (tests/kernel_bar.py):
e32 = max|fp32 torch-CPU - float64| of the same torch ops on the case's inputs; a kernel must stay within
4 * e32 + 4 * 2^-24 * max|float64|.  Every output (act_out, ya, yb, stats_a, stats_b) lies in a sentinel band and starts as
NaN, so an element the kernel never writes fails the bar and one written outside fails the band; every case runs twice and
must give the same bytes.  ivln_gn_conv_f32's partial slabs are compared ONE BY ONE (slab g = the conv over group g's
channels only) before their sum is; ivln_nconv_f32's emitted (count, mean, M2) partials are compared per (strip, image,
group) with the float64 statistics of the kernel's own output over that strip, then merged (Chan) and compared with the
two-pass statistics of the whole output.  Every comparison goes to gn_conv_kernels.log in the suite's log directory.

tests/test_gn_conv_plan_coverage.py (CPU) restates the launchers' plans in Python, asserts that every case below reaches
the edge its tag names, and lends this file gn_plan / nconv_plan: launcher and restatement must agree on accepted versus
refused for every case and refusal shape, and for ivln_nconv_f32 on the number of strips (the written extent of stats_a).

Measured on an MI355X (46 tests, 361 comparisons, none OVER, under 3 s): the largest hip / e32 ratios are the emitted
variances - n-plain st_b 26.1 (err 5.7e-06, bar 7.9e-06), n-x2-res st_a 20.9, n-t5 st_a 20.0, n-g32 st_a 17.5, g32-in st_a
13.8 (torch's two-pass fp32 variance is the e32 there, the kernel's is one pass) -; the conv outputs stay at or below 3.1
(n-halved ya), the slabs of ivln_gn_conv_f32 at or below 2.8 (lds-in ya[9])."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from kernel_bar import _Bar, _log, _same_bytes, _twice

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOG = "gn_conv_kernels.log"
E_UNSUPPORTED = -5
SENT = -777.0   # sentinel of the guard bands
PAD = 8         # guard floats on either side (32 bytes: the view stays 16-byte aligned)
EPS_GN = 1e-5
NAN = float("nan")

# ivln_gn_conv_f32.  a = (Cout, k, stride, pad), b = (Cout, stride), x2 = slabs of the second operand, front = (C0, groups0,
# slabs of x0); `splits` slabs of x: 16 is slab_sum's unrolled path, 5 the first slab plus one group of four, 6 that plus a
# tail, 3 the tail only
GN_CASES = [
    dict(tag="t3", N=1, C=64, H=9, W=9, groups=8, splits=3, a=(32, 3, 1, 1), act_out=True),
    dict(tag="t5", N=1, C=64, H=12, W=12, groups=16, splits=16, a=(32, 1, 1, 0)),
    dict(tag="t7", N=1, C=64, H=14, W=14, groups=16, splits=5, a=(20, 3, 1, 1)),
    dict(tag="b3", N=20, C=128, H=8, W=8, groups=16, splits=1, a=(256, 1, 1, 0), b=(96, 2)),
    dict(tag="stream", N=1, C=128, H=8, W=8, groups=2, splits=3, a=(200, 3, 1, 1), b=(72, 2), act_out=True),
    dict(tag="ragged-S", N=3, C=32, H=6, W=6, groups=16, splits=16, a=(66, 3, 2, 1), x2=5),
    dict(tag="pool", N=2, C=32, H=13, W=11, groups=16, splits=5, pool=True, a=(24, 3, 1, 1), b=(40, 1), act_out=True),
    dict(tag="act-only", N=2, C=48, H=5, W=5, groups=16, splits=3, act_out=True, residual=True),
    dict(tag="front3", N=2, C=256, H=9, W=9, groups=16, front=(32, 16, 5), a=(32, 1, 1, 0), act_out=True),
    dict(tag="front-nopart", N=2, C=512, H=8, W=8, groups=16, front=(256, 16, 16), a=(16, 1, 1, 0), residual=True),
    dict(tag="front-x2", N=2, C=128, H=4, W=4, groups=16, front=(64, 8, 3), x2=16, b=(64, 2), act_out=True),
    # (two branches the plan search found beside the table's: a spare wave handed to the front-stage / the tile loaders,
    #  and `part` dropped without a front stage - 256 channels in one group is also the largest cpg the launcher takes)
    dict(tag="spare-front", N=1, C=16, H=4, W=4, groups=8, front=(32, 16, 1), b=(16, 1), act_out=True),
    dict(tag="spare-tile", N=1, C=16, H=4, W=4, groups=8, front=(32, 16, 1), x2=16, a=(256, 1, 1, 0), act_out=True),
    dict(tag="nofront-nopart", N=1, C=256, H=1, W=32, groups=1, splits=6, x2=1, residual=True, pool=True, a=(8, 1, 1, 0), act_out=True),
]
# ivln_nconv_f32.  a = (Cout, k, groups of the next GroupNorm, stride), b = (Cout, groups, stride); groups / parts: the
# input's GroupNorm and the number of statistics partials it comes with (absent: the input is used as given); x2 = parts2
NCONV_CASES = [
    dict(tag="n-t6", N=2, C=16, H=8, W=8, groups=8, parts=2, a=(96, 3, 16, 1), zero_part=True),
    dict(tag="n-t5", N=2, C=32, H=4, W=8, groups=16, parts=1, a=(160, 1, 16, 1)),
    dict(tag="n-t3", N=1, C=16, H=7, W=12, groups=8, parts=3, a=(24, 3, 2, 1), rows_per_block=7, zero_part=True),
    dict(tag="n-loop17", N=2, C=32, H=20, W=4, groups=16, parts=17, a=(32, 3, 16, 1), zero_part=True),
    dict(tag="n-dpp16", N=2, C=32, H=20, W=4, groups=16, parts=16, a=(32, 3, 16, 1)),
    dict(tag="n-g32", N=2, C=64, H=8, W=8, groups=32, parts=2, a=(64, 1, 32, 1), zero_part=True),
    dict(tag="n-b-odd", N=1, C=16, H=7, W=8, groups=8, parts=1, a=(32, 1, 16, 1), b=(64, 16, 2)),
    dict(tag="n-s2-odd", N=2, C=16, H=9, W=8, groups=8, parts=1, a=(32, 3, 16, 2)),
    dict(tag="n-w64", N=1, C=48, H=8, W=64, groups=8, parts=8, a=(32, 3, 16, 1)),
    dict(tag="n-halved", N=1, C=64, H=16, W=32, groups=16, parts=8, a=(64, 3, 16, 2)),
    dict(tag="n-plain", N=2, C=16, H=8, W=8, a=(32, 3, 16, 1), b=(32, 16, 1), residual=True),
    dict(tag="n-x2-res", N=2, C=32, H=8, W=8, groups=16, parts=4, x2=2, a=(32, 1, 16, 1), residual=True, act_out=True),
]
# one shape just inside (why None: accepted, and checked like a case) and one just outside each refusal reason; `why` is the
# reason as tests/test_gn_conv_plan_coverage.py's restatement words it
GN_REFUSALS = [
    dict(tag="tile-in", N=1, C=32, H=64, W=64, groups=16, splits=1, act_out=True, why=None),
    dict(tag="tile-out", N=1, C=32, H=64, W=66, groups=16, splits=1, act_out=True, why="cpg * H * W > 8192"),
    dict(tag="oddcpg-in", N=2, C=32, H=5, W=5, groups=16, splits=3, a=(8, 1, 1, 0), why=None),
    dict(tag="oddcpg-out", N=2, C=48, H=5, W=5, groups=16, splits=3, a=(8, 1, 1, 0), why="odd channels per group with a conv"),
    dict(tag="lds-in", N=1, C=32, H=8, W=8, groups=16, front=(512, 16, 1), a=(16, 1, 1, 0), why=None),
    dict(tag="lds-out", N=1, C=32, H=8, W=8, groups=16, front=(576, 16, 1), a=(16, 1, 1, 0), why="152 KB of LDS"),
]
_BAD = "k, W % 4, odd C or groups > 32"
NCONV_REFUSALS = [
    dict(tag="w4-in", N=1, C=16, H=8, W=8, groups=8, parts=1, a=(32, 1, 16, 1), why=None),
    dict(tag="w4-out", N=1, C=16, H=8, W=6, groups=8, parts=1, a=(32, 1, 16, 1), why=_BAD),
    dict(tag="oddc-in", N=1, C=14, H=8, W=8, a=(32, 1, 16, 1), why=None),
    dict(tag="oddc-out", N=1, C=15, H=8, W=8, a=(32, 1, 16, 1), why=_BAD),
    dict(tag="g32-in", N=1, C=64, H=8, W=8, groups=32, parts=1, a=(32, 1, 16, 1), why=None),
    dict(tag="g33-out", N=1, C=66, H=8, W=8, groups=33, parts=1, a=(32, 1, 16, 1), why=_BAD),
    dict(tag="wo4-in", N=1, C=16, H=8, W=16, groups=8, parts=1, a=(32, 3, 16, 2), why=None),
    dict(tag="wo4-out", N=1, C=16, H=8, W=12, groups=8, parts=1, a=(32, 3, 16, 2), why="Wo % 4"),
    dict(tag="actout-s1-in", N=1, C=16, H=8, W=8, groups=8, parts=1, a=(32, 3, 16, 1), act_out=True, why=None),
    dict(tag="actout-s2-out", N=1, C=16, H=8, W=8, groups=8, parts=1, a=(32, 3, 16, 2), act_out=True, why="act_out beside a stride-2 conv A"),
    dict(tag="b-s1-in", N=1, C=16, H=8, W=8, groups=8, parts=1, a=(32, 3, 16, 1), b=(32, 16, 1), why=None),
    dict(tag="b-s2-out", N=1, C=16, H=8, W=8, groups=8, parts=1, a=(32, 3, 16, 2), b=(32, 16, 1), why="conv B beside a stride-2 conv A"),
    dict(tag="rpb-in", N=1, C=64, H=6, W=32, groups=16, parts=1, a=(32, 3, 16, 1), rows_per_block=3, why=None),
    dict(tag="rpb-out", N=1, C=64, H=6, W=32, groups=16, parts=1, a=(32, 3, 16, 1), rows_per_block=6, why="rows_per_block does not fit"),
]


def _lib():
    from ivln_ce_amd import ops

    L = ops._L()
    L.ivln_gn_conv_f32.argtypes = [C.POINTER(ops.GnConvDesc), C.c_void_p]
    L.ivln_nconv_f32.argtypes = [C.POINTER(ops.NconvDesc), C.c_void_p]
    return L, ops


def _sp():
    from ivln_ce_amd import ops

    return ops.stream_ptr()


def _gen(c):
    s = 0
    for ch in c["tag"]:
        s = (s * 131 + ord(ch)) % (2 ** 31)
    return torch.Generator().manual_seed(s)


class _Outs:
    """the output buffers of one launch: each `n` NaN floats between two bands of PAD sentinels (+ `spare` more behind)"""

    def __init__(self):
        self.names, self.bufs, self.n = [], [], []

    def add(self, name, n, spare=0):
        buf = torch.full((n + spare + 2 * PAD,), SENT, dtype=torch.float32, device=DEV)
        buf[PAD:PAD + n] = NAN
        self.names.append(name)
        self.bufs.append(buf)
        self.n.append(n)
        return buf[PAD:].data_ptr()

    def get(self, name):
        i = self.names.index(name)
        return self.bufs[i][PAD:PAD + self.n[i]]

    def bands_ok(self, case):
        for name, buf, n in zip(self.names, self.bufs, self.n):
            assert bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + n:] == SENT).all()), f"{case} {name}: written outside its {n} floats"

    def untouched(self, case):
        self.bands_ok(case)
        for name, buf, n in zip(self.names, self.bufs, self.n):
            assert bool(torch.isnan(buf[PAD:PAD + n]).all()), f"{case} {name}: a refused launch wrote to it"


def _params(Cc, g):
    return [torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.3]


# ------------------------------------------------------------------------------------------------------------------
# ivln_gn_conv_f32
# ------------------------------------------------------------------------------------------------------------------
def _gn_tensors(c):
    """the case's inputs in fp32 on the CPU"""
    g = _gen(c)
    N, Cc, H, W = c["N"], c["C"], c["H"], c["W"]

    def slabs(ch, splits, scale, off):
        s = torch.randn(splits, ch, N * H * W, generator=g) * (scale / splits ** 0.5)
        s[0] += off
        return s

    t = {}
    if c.get("front"):
        C0, _, s0 = c["front"]
        t["x0"] = slabs(C0, s0, 1.5, 0.25)
        t["gamma0"], t["beta0"] = _params(C0, g)
        t["w0"] = torch.randn(Cc, C0, 1, 1, generator=g) / C0 ** 0.5
    else:
        t["x"] = slabs(Cc, c["splits"], 1.5, 0.25)
    t["gamma"], t["beta"] = _params(Cc, g)
    if c.get("x2"):
        t["x2"] = slabs(Cc, c["x2"], 1.0, -0.1)
        t["gamma2"], t["beta2"] = _params(Cc, g)
    if c.get("residual"):
        t["residual"] = torch.randn(N, Cc, H, W, generator=g)
    if c.get("a"):
        co, k = c["a"][0], c["a"][1]
        t["wa"] = torch.randn(co, Cc, k, k, generator=g) / (Cc * k * k) ** 0.5
    if c.get("b"):
        t["wb"] = torch.randn(c["b"][0], Cc, 1, 1, generator=g) / Cc ** 0.5
    return t


def _gn_sizes(c):
    H, W = c["H"], c["W"]
    Hc, Wc = ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if c.get("pool") else (H, W)
    oa = ob = None
    if c.get("a"):
        _, k, s, p = c["a"]
        oa = ((Hc + 2 * p - k) // s + 1, (Wc + 2 * p - k) // s + 1)
    if c.get("b"):
        ob = ((Hc - 1) // c["b"][1] + 1, (Wc - 1) // c["b"][1] + 1)
    return (Hc, Wc), oa, ob


def _gn_ref(c, t, dt):
    """act (N, C, Hc, Wc), then per conv (slabs [groups][Cout][N][Ho*Wo], full [Cout][N][Ho*Wo]) in dtype dt"""
    N, Cc, H, W, G = c["N"], c["C"], c["H"], c["W"], c["groups"]

    def img(s, ch):
        return s.to(dt).sum(0).view(ch, N, H, W).permute(1, 0, 2, 3)

    if c.get("front"):
        C0, G0, _ = c["front"]
        x = F.conv2d(F.relu(F.group_norm(img(t["x0"], C0), G0, t["gamma0"].to(dt), t["beta0"].to(dt), EPS_GN)), t["w0"].to(dt))
    else:
        x = img(t["x"], Cc)
    y = F.group_norm(x, G, t["gamma"].to(dt), t["beta"].to(dt), EPS_GN)
    if c.get("x2"):
        y = y + F.group_norm(img(t["x2"], Cc), G, t["gamma2"].to(dt), t["beta2"].to(dt), EPS_GN)
    if c.get("residual"):
        y = y + t["residual"].to(dt)
    if c.get("relu", True):
        y = F.relu(y)
    if c.get("pool"):
        y = F.max_pool2d(y, 3, 2, 1)
    out = {"act": y}
    cpg = Cc // G
    for name, w, stride, pad in (("a", t.get("wa"), c["a"][2] if c.get("a") else 0, c["a"][3] if c.get("a") else 0),
                                 ("b", t.get("wb"), c["b"][1] if c.get("b") else 0, 0)):
        if w is None:
            continue
        co, k = w.shape[0], w.shape[2]
        wg = w.to(dt).view(co, G, cpg, k, k).permute(1, 0, 2, 3, 4).reshape(G * co, cpg, k, k)   # block g: W[:, g*cpg:(g+1)*cpg]
        s = F.conv2d(y, wg, None, stride, pad, 1, G)
        out[name + "_slabs"] = s.reshape(N, G, co, -1).permute(1, 2, 0, 3)
        out[name] = F.conv2d(y, w.to(dt), None, stride, pad).reshape(N, co, -1).permute(1, 0, 2)
    return out


def _gn_launch(c, t, d_t):
    """one launch on fresh output buffers -> (return code, _Outs)"""
    L, ops = _lib()
    N, Cc, H, W, G = c["N"], c["C"], c["H"], c["W"], c["groups"]
    (Hc, Wc), oa, ob = _gn_sizes(c)
    p = lambda k: d_t[k].data_ptr() if k in d_t else None  # noqa: E731
    d = ops.GnConvDesc()
    if c.get("front"):
        C0, G0, s0 = c["front"]
        d.x0, d.splits0, d.slab_stride0, d.C0, d.groups0 = p("x0"), s0, C0 * N * H * W, C0, G0
        d.gamma0, d.beta0, d.w0 = p("gamma0"), p("beta0"), p("w0")
    else:
        d.x, d.splits, d.slab_stride = p("x"), c["splits"], Cc * N * H * W
    d.gamma, d.beta = p("gamma"), p("beta")
    if c.get("x2"):
        d.x2, d.splits2, d.slab_stride2, d.gamma2, d.beta2 = p("x2"), c["x2"], Cc * N * H * W, p("gamma2"), p("beta2")
    d.residual = p("residual")
    d.N, d.C, d.H, d.W, d.groups, d.eps, d.relu, d.pool = N, Cc, H, W, G, EPS_GN, int(c.get("relu", True)), int(bool(c.get("pool")))
    o = _Outs()
    if c.get("act_out"):
        d.act_out = o.add("act", N * Cc * Hc * Wc)
    if c.get("a"):
        co, k, s, pad = c["a"]
        d.wa, d.Cout_a, d.ka, d.stride_a, d.pad_a = p("wa"), co, k, s, pad
        d.ya = o.add("ya", G * co * N * max(oa[0], 0) * max(oa[1], 0))
    if c.get("b"):
        d.wb, d.Cout_b, d.stride_b = p("wb"), c["b"][0], c["b"][1]
        d.yb = o.add("yb", G * c["b"][0] * N * ob[0] * ob[1])
    rc = L.ivln_gn_conv_f32(C.byref(d), _sp())
    torch.cuda.synchronize()
    return rc, o


def _run_gn(c):
    from test_gn_conv_plan_coverage import gn_plan

    case = "gn_conv " + c["tag"]
    plan = gn_plan(c)
    t = _gn_tensors(c)
    d_t = {k: v.contiguous().to(DEV) for k, v in t.items()}
    if not plan.ok:
        rc, o = _gn_launch(c, t, d_t)
        _log(f"{case:44s} refused rc {rc} (plan: {plan.why})", LOG)
        assert plan.code == "unsupported" and rc == E_UNSUPPORTED, f"{case}: launcher {rc}, plan refuses ({plan.why})"
        o.untouched(case)
        return
    keep = []

    def run():
        rc, o = _gn_launch(c, t, d_t)
        assert rc == 0, f"{case}: launcher {rc}, plan accepts"
        keep.append(o)
        return tuple(o.bufs)

    _twice(run)
    o = keep[0]
    o.bands_ok(case)
    r64, r32 = _gn_ref(c, t, torch.float64), _gn_ref(c, t, torch.float32)
    bar = _Bar(case, LOG)
    if c.get("act_out"):
        bar.check("act", o.get("act"), r64["act"], r32["act"])
    G = c["groups"]
    for name in ("a", "b"):
        if not c.get(name):
            continue
        y = o.get("y" + name).cpu().view(G, c[name][0], c["N"], -1)
        for g in range(G):   # slab g alone: a contribution written to the wrong slab does not cancel here
            bar.check(f"y{name}[{g}]", y[g], r64[name + "_slabs"][g], r32[name + "_slabs"][g])
        bar.check(f"y{name} sum", y.double().sum(0), r64[name], r32[name])
    bar.done()


@pytest.mark.parametrize("c", GN_CASES, ids=[c["tag"] for c in GN_CASES])
def test_gn_conv_case(c):
    """k_gn_conv at one plan edge (the tag; tests/test_gn_conv_plan_coverage.py asserts that the shape reaches it): the
    activation, every partial slab of conv A / conv B alone, and their sum, within the bar; twice the same bytes; nothing
    written outside the outputs and nothing left unwritten inside."""
    _run_gn(c)


@pytest.mark.parametrize("c", GN_REFUSALS, ids=[c["tag"] for c in GN_REFUSALS])
def test_gn_conv_refusals(c):
    """Either side of each refusal reason of ivln_gn_conv_f32: the shape just inside is computed (and checked like a case),
    the one just outside returns IVLN_E_UNSUPPORTED with every output buffer still NaN between intact sentinels; the Python
    restatement of the plan agrees on which is which."""
    _run_gn(c)


# ------------------------------------------------------------------------------------------------------------------
# ivln_nconv_f32
# ------------------------------------------------------------------------------------------------------------------
def _cuts(HW, parts):
    """ragged strips of the input's pixels: unequal counts, none empty"""
    return [0] + [(HW * i) // parts + (i & 1) for i in range(1, parts)] + [HW]


def _partials(x, groups, parts, zero_part=False):
    """what a producer leaves: (count, mean, M2) per (part, image, group) of x (N, C, H, W), computed in float64 over ragged
    strips, cast to fp32; zero_part appends the empty partial (0, 0, 0) the kernel itself emits for an empty strip"""
    N, Cc, H, W = x.shape
    xg = x.double().reshape(N, groups, Cc // groups, H * W)
    cuts = _cuts(H * W, parts)
    assert len(set(b - a for a, b in zip(cuts, cuts[1:]))) > 1 or parts == 1
    out = torch.zeros(parts + int(zero_part), N, groups, 3, dtype=torch.float64)
    for i in range(parts):
        blk = xg[..., cuts[i]:cuts[i + 1]].reshape(N, groups, -1)
        out[i, :, :, 0] = blk.shape[2]
        out[i, :, :, 1] = blk.mean(2)
        out[i, :, :, 2] = ((blk - blk.mean(2, keepdim=True)) ** 2).sum(2)
    return out.float()


def _nc_tensors(c):
    g = _gen(c)
    N, Cc, H, W = c["N"], c["C"], c["H"], c["W"]
    t = {"x": torch.randn(N, Cc, H, W, generator=g) * 1.7 + 0.4}
    if c.get("groups"):
        t["gamma"], t["beta"] = _params(Cc, g)
    if c.get("x2"):
        t["x2"] = torch.randn(N, Cc, H, W, generator=g) * 0.8 - 0.3
        t["gamma2"], t["beta2"] = _params(Cc, g)
    if c.get("residual"):
        t["residual"] = torch.randn(N, Cc, H, W, generator=g)
    co, k = c["a"][0], c["a"][1]
    t["wa"] = torch.randn(co, Cc, k, k, generator=g) / (Cc * k * k) ** 0.5
    if c.get("b"):
        t["wb"] = torch.randn(c["b"][0], Cc, 1, 1, generator=g) / Cc ** 0.5
    return t


def _nc_sizes(c):
    H, W, (_, k, _, sa) = c["H"], c["W"], c["a"]
    oa = ((H + 2 * (k // 2) - k) // sa + 1, (W + 2 * (k // 2) - k) // sa + 1)
    ob = ((H - 1) // c["b"][2] + 1, (W - 1) // c["b"][2] + 1) if c.get("b") else None
    return oa, ob


def _nc_ref(c, t, dt):
    """the transformed input (N, C, H, W) and the conv outputs [Cout][N][Ho][Wo] in dtype dt"""
    y = t["x"].to(dt)
    if c.get("groups"):
        G = c["groups"]
        y = F.group_norm(y, G, t["gamma"].to(dt), t["beta"].to(dt), EPS_GN)
        if c.get("x2"):
            y = y + F.group_norm(t["x2"].to(dt), G, t["gamma2"].to(dt), t["beta2"].to(dt), EPS_GN)
    if c.get("residual"):
        y = y + t["residual"].to(dt)
    if c.get("relu", True):
        y = F.relu(y)
    out = {"act": y, "a": F.conv2d(y, t["wa"].to(dt), None, c["a"][3], c["a"][1] // 2).permute(1, 0, 2, 3)}
    if c.get("b"):
        out["b"] = F.conv2d(y, t["wb"].to(dt), None, c["b"][2]).permute(1, 0, 2, 3)
    return out


def _nc_launch(c, d_t, strips, zero_part=False):
    """one launch on fresh output buffers -> (return code, _Outs).  strips: what the plan expects - stats_a / stats_b get
    that many strips of NaN and sentinels up to one strip per output row behind them"""
    L, ops = _lib()
    N, Cc, H, W = c["N"], c["C"], c["H"], c["W"]
    oa, ob = _nc_sizes(c)
    p = lambda k: d_t[k].data_ptr() if k in d_t else None  # noqa: E731
    d = ops.NconvDesc()
    stats = bool(c.get("groups"))
    d.x = p("x_raw") if stats else p("x")
    if stats:
        d.stats, d.parts, d.gamma, d.beta, d.groups = p("stats_z" if zero_part else "stats"), c["parts"] + int(zero_part), p("gamma"), p("beta"), c["groups"]
    if c.get("x2"):
        d.x2, d.stats2, d.parts2, d.gamma2, d.beta2 = p("x2_raw"), p("stats2_z" if zero_part else "stats2"), c["x2"] + int(zero_part), p("gamma2"), p("beta2")
    d.residual = p("residual")
    d.N, d.C, d.H, d.W, d.eps, d.relu = N, Cc, H, W, EPS_GN, int(c.get("relu", True))
    o = _Outs()
    if c.get("act_out"):
        d.act_out = o.add("act", N * Cc * H * W)
    co, k, ga, sa = c["a"]
    rows_a = max(oa[0], 1)
    d.wa, d.Cout_a, d.ka, d.groups_a, d.stride_a = p("wa"), co, k, ga, sa
    d.ya = o.add("ya", co * N * max(oa[0], 0) * max(oa[1], 0))
    d.stats_a = o.add("stats_a", strips * N * ga * 3, (rows_a - strips) * N * ga * 3)
    if c.get("b"):
        cb, gb, sb = c["b"]
        d.wb, d.Cout_b, d.groups_b, d.stride_b = p("wb"), cb, gb, sb
        d.yb = o.add("yb", cb * N * ob[0] * ob[1])
        d.stats_b = o.add("stats_b", strips * N * gb * 3, (rows_a - strips) * N * gb * 3)
    d.rows_per_block = c.get("rows_per_block", 0)
    rc = L.ivln_nconv_f32(C.byref(d), _sp())
    torch.cuda.synchronize()
    return rc, o


def _stats_check(bar, name, st, y, RS, N, ng):
    """the emitted partials st [strips][N][ng][3] against the float64 statistics of the kernel's OWN output y [Cout][N][Ho][Wo]
    (fp32, CPU) per strip of RS rows - the statistics arithmetic alone, without the conv's error - and, merged, against the
    two-pass statistics of the whole output"""
    Co, _, Ho, Wo = y.shape
    cpo = Co // ng
    st = st.cpu().view(-1, N, ng, 3)
    cnt, m64, m32, v64, v32, mag = [], [], [], [], [], []
    for s in range(st.shape[0]):
        blk = y[:, :, s * RS:min(Ho, (s + 1) * RS)].reshape(ng, cpo, N, -1).permute(2, 0, 1, 3).reshape(N, ng, -1)
        b64 = blk.double()
        cnt.append(torch.full((N, ng), float(blk.shape[2])))
        m64.append(b64.mean(2))
        m32.append(blk.mean(2))
        v64.append(b64.var(2, unbiased=False))
        v32.append(blk.var(2, unbiased=False))
        # the kernel's one-pass formula shifts by the group's first value (pilot): sum((v - pilot)^2) / n - ((sum(v - pilot)) / n)^2
        # = var + (pilot - mean)^2 minus (pilot - mean)^2 - both terms are rounded at var + (pilot - mean)^2
        mag.append(v64[-1] + (b64[..., 0] - m64[-1]) ** 2)
    cnt, m64, m32, v64, v32, mag = (torch.stack(v) for v in (cnt, m64, m32, v64, v32, mag))
    ok = torch.equal(st[..., 0], cnt)
    _log(f"{bar.case:44s} {name + ' n':10s} exact  {'ok' if ok else 'OVER'}", LOG)
    if not ok:
        bar.bad.append(f"{name}: counts differ")
        return
    vmag = float(mag.max())
    # the mean comes from the same shifted sums, mean = pilot + sum(v - pilot) / n: each v - pilot is rounded at |v - pilot|
    # (on average at most their root mean square, sqrt(var + (pilot - mean)^2)), the quotient at |mean - pilot| <= that root,
    # and only the last add at |mean| - so it rounds at |mean| + sqrt(var + (pilot - mean)^2), the root of the variance's
    # term, not at |mean| alone (a group mean is near 0 among values of a few units: with max|mean| = 0.387 as the term,
    # n-t5's partial means were 2.326e-07 off against a bar of 1.675e-07, every other case inside)
    mmag = float((m64.abs() + mag.sqrt()).max())
    bar.check(name + " mean", st[..., 1], m64, m32, mag=mmag)
    bar.check(name + " var", st[..., 2] / st[..., 0], v64, v32, mag=vmag)
    # Chan's merge of the partials in float64 == the two-pass statistics of the whole output (which inherit the partials'
    # rounding: the same magnitude term for the variance)
    s64 = st.double()
    n_all = s64[..., 0].sum(0)
    mean = (s64[..., 0] * s64[..., 1]).sum(0) / n_all
    var = (s64[..., 2] + s64[..., 0] * (s64[..., 1] - mean) ** 2).sum(0) / n_all
    whole = y.reshape(ng, cpo, N, -1).permute(2, 0, 1, 3).reshape(N, ng, -1)
    bar.check(name + " Mmean", mean, whole.double().mean(2), whole.mean(2), mag=mmag)
    bar.check(name + " Mvar", var, whole.double().var(2, unbiased=False), whole.var(2, unbiased=False), mag=vmag)


def _run_nconv(c):
    from test_gn_conv_plan_coverage import nconv_plan

    case = "nconv " + c["tag"]
    plan = nconv_plan(c)
    t = _nc_tensors(c)
    d_t = {k: v.contiguous().to(DEV) for k, v in t.items()}
    if c.get("groups"):   # raw conv outputs are channel-major over the batch, with the producer's partials
        for k, parts in (("x", c["parts"]), ("x2", c.get("x2"))):
            if parts:
                d_t[k + "_raw"] = t[k].permute(1, 0, 2, 3).contiguous().to(DEV)
                sk = "stats" if k == "x" else "stats2"
                d_t[sk] = _partials(t[k], c["groups"], parts).to(DEV)
                d_t[sk + "_z"] = _partials(t[k], c["groups"], parts, True).to(DEV)
    if not plan.ok:
        rc, o = _nc_launch(c, d_t, 1)
        _log(f"{case:44s} refused rc {rc} (plan: {plan.why})", LOG)
        assert plan.code == "unsupported" and rc == E_UNSUPPORTED, f"{case}: launcher {rc}, plan refuses ({plan.why})"
        o.untouched(case)
        return
    keep = []

    def run():
        rc, o = _nc_launch(c, d_t, plan.strips)
        assert rc == 0, f"{case}: launcher {rc}, plan accepts"
        keep.append(o)
        return tuple(o.bufs)

    _twice(run)
    o = keep[0]
    o.bands_ok(case)   # (stats_a / stats_b: written up to the plan's number of strips and no further ...)
    r64, r32 = _nc_ref(c, t, torch.float64), _nc_ref(c, t, torch.float32)
    bar = _Bar(case, LOG)
    if c.get("act_out"):
        bar.check("act", o.get("act"), r64["act"], r32["act"])
    for name in ("a", "b"):
        if not c.get(name):
            continue
        y = o.get("y" + name).cpu().view(r64[name].shape)
        bar.check("y" + name, y, r64[name], r32[name])
        st = o.get("stats_" + name)
        assert not bool(torch.isnan(st).any()), f"{case}: the launcher wrote fewer than the plan's {plan.strips} strips of stats_{name}"   # (... and no less)
        _stats_check(bar, "st_" + name, st, y, plan.RS if name == "a" else plan.RSb, c["N"], c[name][2 if name == "a" else 1])
    bar.done()
    if c.get("zero_part"):   # an appended empty partial (count 0, mean 0, M2 0) changes no bit of any output
        rc, oz = _nc_launch(c, d_t, plan.strips, zero_part=True)
        assert rc == 0
        same = all(_same_bytes(x, y) for x, y in zip(o.bufs, oz.bufs))
        _log(f"{case:44s} {'+0 part':10s} exact  {'ok' if same else 'OVER'}", LOG)
        assert same, f"{case}: an empty statistics partial changed the outputs"


@pytest.mark.parametrize("c", NCONV_CASES, ids=[c["tag"] for c in NCONV_CASES])
def test_nconv_case(c):
    """k_nconv at one plan edge: the transformed input (where handed out), conv A / conv B, the emitted statistics partials
    per (strip, image, group) and their merge, within the bar; twice the same bytes; the number of strips the plan says
    (written extent of stats_a / stats_b); where marked, an appended empty input partial changes no byte."""
    _run_nconv(c)


@pytest.mark.parametrize("c", NCONV_REFUSALS, ids=[c["tag"] for c in NCONV_REFUSALS])
def test_nconv_refusals(c):
    """Either side of each refusal reason of ivln_nconv_f32: just inside is computed and checked like a case, just outside
    returns IVLN_E_UNSUPPORTED with every output buffer still NaN between intact sentinels; the plan restatement agrees."""
    _run_nconv(c)
