"""GPU: the kernels of the trainable RGB ResNet-50 alone (csrc/rgb_bwd.hip) against float64 formulas.

Bar: tests/kernel_bar.py's - e32 = the same formula in fp32 torch on the CPU against float64 is the arithmetic's own noise on
the case's inputs, a kernel stays within 4 * e32 + 4 * 2^-24 * max|float64|; selections (dz) are exact.  Every launch runs
twice with identical bytes, every output starts as NaN between sentinel bands that must survive.  The measured values go to
rgb_bwd_kernels.log in the suite's log directory before anything is asserted."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from kernel_bar import _Bar, _log, _same_bytes  # noqa: E402

DEV = torch.device("cuda:0")
LOG = "rgb_bwd_kernels.log"
SENT = -777.0
E_INVALID = -1


def _banded(shape, pad, nan=True):
    """a dense tensor of `shape` inside a sentinel-filled buffer, `pad` floats from its start (pad % 4 != 0: the view is not
    16-byte aligned) -> (view, buffer)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * pad,), SENT, dtype=torch.float32, device=DEV)
    v = buf[pad:pad + n]
    if nan:
        v.fill_(float("nan"))
    return v.view(shape), buf


def _intact(buf, pad, what):
    assert bool((buf[:pad] == SENT).all()) and bool((buf[buf.numel() - pad:] == SENT).all()), f"{what}: written outside"


def _put(t, pad):
    if t is None:
        return None
    v, _ = _banded(tuple(t.shape), pad, nan=False)
    v.copy_(t)
    return v


# ------------------------------------------------------------------------------------------------
# (a) ivln_bn_apply_f32
# ------------------------------------------------------------------------------------------------
def _apply_formula(x, sc, sh, r, x2, sc2, sh2, relu):
    v = lambda t: t.view(1, -1, 1)  # noqa: E731
    y = x * v(sc) + v(sh)
    if r is not None:
        y = y + r
    if x2 is not None:
        y = y + (x2 * v(sc2) + v(sh2))
    return torch.relu(y) if relu else y


# HW = 49, C = 5: the 4-byte path, 7 workgroups whose first element is inside a plane; HW = 16, C = 8: the 16-byte path,
# 3 workgroups; the last: HW % 4 == 0 behind an unaligned pointer takes the 4-byte path
APPLY_SHAPES = [(7, 5, 49, 8), (20, 8, 16, 8), (20, 8, 16, 5)]


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("mode", ["plain", "residual", "two_bn", "both"])
@pytest.mark.parametrize("N,C,HW,pad", APPLY_SHAPES, ids=["scalar_49x5", "vector_16x8", "unaligned_16x8"])
def test_bn_apply_against_the_float64_formula(N, C, HW, pad, mode, relu):
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(N + C + HW + len(mode))
    x = torch.randn(N, C, HW, generator=g) * 1.5 + 0.3
    sc, sh = torch.randn(C, generator=g) * 0.3 + 1.0, torch.randn(C, generator=g)
    r = torch.randn(N, C, HW, generator=g) if mode in ("residual", "both") else None
    x2 = torch.randn(N, C, HW, generator=g) if mode in ("two_bn", "both") else None
    sc2, sh2 = (torch.randn(C, generator=g), torch.randn(C, generator=g)) if x2 is not None else (None, None)
    d = lambda t: None if t is None else t.double()  # noqa: E731
    r64 = _apply_formula(d(x), d(sc), d(sh), d(r), d(x2), d(sc2), d(sh2), relu)
    r32 = _apply_formula(x, sc, sh, r, x2, sc2, sh2, relu)
    dv = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    args = (_put(x, pad), dv(sc), dv(sh))
    kw = dict(relu=relu, residual=_put(r, pad), x2=_put(x2, pad), scale2=dv(sc2), shift2=dv(sh2))

    def once():
        y, buf = _banded((N, C, HW), pad)
        ops.bn_apply(*args, out=y, **kw)
        torch.cuda.synchronize()
        _intact(buf, pad, "y")
        return y

    a, b = once(), once()
    assert _same_bytes(a, b)
    bar = _Bar(f"bn_apply N{N} C{C} HW{HW} pad{pad} {mode} relu{int(relu)}", LOG)
    bar.check("y", a, r64, r32)
    bar.done()


# ------------------------------------------------------------------------------------------------
# (b) ivln_bn_bwd_f32
# ------------------------------------------------------------------------------------------------
def _bn_bwd_formula(dy, x, mean, rv, gamma, out, train, eps):
    """the header's formulas in the dtype of the inputs -> (dx, dgamma, dbeta, dz)"""
    N, C, HW = x.shape
    v = lambda t: t.view(1, C, 1)  # noqa: E731
    dz = dy * (out > 0).to(dy.dtype) if out is not None else dy
    rstd = rv if train else 1.0 / torch.sqrt(rv + eps)
    xh = (x - v(mean)) * v(rstd)
    dbeta, dgamma = dz.sum((0, 2)), (dz * xh).sum((0, 2))
    M = N * HW
    if train:
        dx = v(gamma * rstd) * (dz - v(dbeta) / M - xh * v(dgamma) / M)
    else:
        dx = v(gamma * rstd) * dz
    return dx, dgamma, dbeta, dz


# (N, C, HW, pad): the issue's three; M = 1; 8 slices of the images with one wave per channel; two slices with the whole
# workgroup on one channel; HW % 4 == 0 behind an unaligned pointer (4-byte path)
BWD_SHAPES = [(3, 5, 49, 8), (2, 64, 144, 8), (1, 2048, 4, 8), (1, 3, 1, 8), (16, 4, 1024, 8), (8, 3, 2048, 8),
              (2, 64, 144, 5)]


@pytest.mark.parametrize("with_dz", [False, True], ids=["no_dz_out", "dz_out"])
@pytest.mark.parametrize("with_out", [False, True], ids=["no_mask", "mask"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("N,C,HW,pad", BWD_SHAPES, ids=[f"N{s[0]}_C{s[1]}_HW{s[2]}_pad{s[3]}" for s in BWD_SHAPES])
def test_bn_bwd_against_the_float64_formula(N, C, HW, pad, train, with_out, with_dz):
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(N * 1000 + C + HW + 7 * with_out)
    eps = 1e-5
    x = torch.randn(N, C, HW, generator=g) * 1.5 + 0.3
    dy = torch.randn(N, C, HW, generator=g)
    gamma = torch.randn(C, generator=g) * 0.2 + 1.0
    out = torch.relu(torch.randn(N, C, HW, generator=g)) if with_out else None
    if train:  # the forward's saved statistics: fp32 values, shared by every evaluation
        xc = x.double().permute(1, 0, 2).reshape(C, -1)
        mean = xc.mean(1).float()
        rv = (1.0 / torch.sqrt(xc.var(1, unbiased=False) + eps)).float()
    else:
        mean, rv = torch.randn(C, generator=g) * 0.5, torch.rand(C, generator=g) * 2 + 0.1
    r64 = _bn_bwd_formula(dy.double(), x.double(), mean.double(), rv.double(), gamma.double(),
                          None if out is None else out.double(), train, eps)
    r32 = _bn_bwd_formula(dy, x, mean, rv, gamma, out, train, eps)
    d_dy, d_x, d_out = _put(dy, pad), _put(x, pad), _put(out, pad)
    d_mean, d_rv, d_gamma = mean.to(DEV), rv.to(DEV), gamma.to(DEV)

    def once():
        dx, bx = _banded((N, C, HW), pad)
        dgam, bg = _banded((C,), 8)
        dbet, bb = _banded((C,), 8)
        dz, bz = _banded((N, C, HW), pad) if with_dz else (False, None)
        res = ops.bn_bwd(d_dy, d_x, d_mean, d_rv, d_gamma, train=train, eps=eps, out=d_out, want_dz=dz, dx=dx, dgamma=dgam,
                         dbeta=dbet)
        torch.cuda.synchronize()
        for b, p, w in ((bx, pad, "dx"), (bg, 8, "dgamma"), (bb, 8, "dbeta")) + (((bz, pad, "dz"),) if with_dz else ()):
            _intact(b, p, w)
        assert (res[3] is None) == (not with_dz)
        return res

    a, b = once(), once()
    bar = _Bar(f"bn_bwd N{N} C{C} HW{HW} pad{pad} train{int(train)} mask{int(with_out)} dz{int(with_dz)}", LOG)
    for name, got, again, ref64, ref32 in zip(("dx", "dgamma", "dbeta"), a, b, r64, r32):
        assert _same_bytes(got, again), f"{bar.case} {name}: two runs differ"
        assert not bool(torch.isnan(got).any()), f"{bar.case} {name}: NaN left"
        bar.check(name, got, ref64, ref32)
    if with_dz:
        assert _same_bytes(a[3], b[3])
        assert torch.equal(a[3].cpu(), r32[3]), f"{bar.case}: dz is dy where out > 0, else 0, exactly"
    if train and N * HW == 1:
        assert float(a[0].abs().max()) == 0.0, "M = 1: dz - dbeta / 1 and xh are exact zeros"
    bar.done()


def test_bn_bwd_in_place_gives_the_same_bits_and_a_small_scratch_is_refused():
    """dx over `out` and dz over `dy` (what train.rgb_encoder_backward does) against separate destinations; a scratch below
    4 * C + 2 floats returns IVLN_E_INVALID and writes nothing."""
    from ivln_ce_amd import ops
    from ivln_ce_amd._lib import f32, i32, i64, vp

    N, C, HW = 4, 6, 64
    g = torch.Generator().manual_seed(3)
    x, dy = torch.randn(N, C, HW, generator=g).to(DEV), torch.randn(N, C, HW, generator=g).to(DEV)
    out = torch.relu(torch.randn(N, C, HW, generator=g)).to(DEV)
    mean, rstd = x.mean((0, 2)), 1.0 / torch.sqrt(x.var((0, 2), unbiased=False) + 1e-5)
    gamma = torch.randn(C, generator=g).to(DEV)
    ref = ops.bn_bwd(dy, x, mean, rstd, gamma, out=out, want_dz=True)
    o2, d2 = out.clone(), dy.clone()
    got = ops.bn_bwd(d2, x, mean, rstd, gamma, out=o2, want_dz=d2, dx=o2)
    torch.cuda.synchronize()
    assert got[0].data_ptr() == o2.data_ptr() and got[3].data_ptr() == d2.data_ptr()
    for a, b in zip(ref, got):
        assert _same_bytes(a, b)

    L = ops._T()
    L.ivln_bn_bwd_f32.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp, i64, vp]
    dx, bx = _banded((N, C, HW), 8)
    dg, bg = _banded((C,), 8)
    db, bb = _banded((C,), 8)
    ws = torch.full((4 * C + 16,), SENT, device=DEV)
    p = lambda t: t.data_ptr()  # noqa: E731
    rc = L.ivln_bn_bwd_f32(p(dy), p(x), p(mean), p(rstd), p(gamma), None, N, C, HW, 1, 1e-5, p(dx), None, p(dg), p(db), p(ws),
                           4 * C + 1, None)
    torch.cuda.synchronize()
    assert rc == E_INVALID
    assert all(bool(torch.isnan(t).all()) for t in (dx, dg, db)) and bool((ws == SENT).all())
    rc = L.ivln_bn_bwd_f32(p(dy), p(x), p(mean), p(rstd), p(gamma), None, N, C, HW, 1, 1e-5, p(dx), None, p(dg), p(db), p(ws),
                           4 * C + 2, None)  # the smallest scratch: one slice
    torch.cuda.synchronize()
    assert rc == 0 and _same_bytes(dx, ops.bn_bwd(dy, x, mean, rstd, gamma)[0])
    for b_ in (bx, bg, bb):
        _intact(b_, 8, "smallest scratch")
    assert bool((ws[4 * C + 2:] == SENT).all()), "the scratch was overrun"


# ------------------------------------------------------------------------------------------------
# (c) ivln_adaptive_avgpool2d_bwd_f32
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(7, 7), (3, 3), (2, 2), (4, 4), (7, 3)], ids=lambda v: str(v))
def test_adaptive_avgpool2d_bwd_against_float64_autograd(H, W):
    """overlapping windows (7 -> 4, 3 -> 4), replicating (2 -> 4), identity (4 -> 4); dy is a channel slice that starts at
    channel 1 of a wider buffer, as the policy's feature buffer is."""
    from ivln_ce_amd import ops

    N, C, CT = 3, 5, 9
    g = torch.Generator().manual_seed(H * 10 + W)
    wide = torch.randn(N, CT, 4, 4, generator=g)
    dy = wide[:, 1:1 + C]
    refs = []
    for dt in (torch.float64, torch.float32):
        xr = torch.zeros(N, C, H, W, dtype=dt, requires_grad=True)
        F.adaptive_avg_pool2d(xr, (4, 4)).backward(dy.to(dt))
        refs.append(xr.grad)
    d_wide = torch.full((N, CT, 4, 4), float("nan"), device=DEV)
    d_wide[:, 1:1 + C] = dy.to(DEV)  # (every other channel of the buffer is NaN: reading one would show)
    a = ops.adaptive_avgpool2d_bwd(d_wide[:, 1:1 + C], H, W, out_ctot=CT)
    b = ops.adaptive_avgpool2d_bwd(d_wide[:, 1:1 + C], H, W, out_ctot=CT)
    dense = ops.adaptive_avgpool2d_bwd(dy.contiguous().to(DEV), H, W)
    torch.cuda.synchronize()
    assert _same_bytes(a, b) and _same_bytes(a, dense)
    bar = _Bar(f"adaptive_avgpool2d_bwd {H}x{W} -> 4x4", LOG)
    bar.check("dx", a, refs[0], refs[1])
    bar.done()
    # through the C entry between sentinels
    from ivln_ce_amd._lib import i32, i64, vp

    L = ops._T()
    L.ivln_adaptive_avgpool2d_bwd_f32.argtypes = [vp, i32, i32, i32, i32, i32, i32, i64, vp, vp]
    dx, buf = _banded((N, C, H, W), 5)
    assert L.ivln_adaptive_avgpool2d_bwd_f32(d_wide[:, 1:1 + C].data_ptr(), N, C, H, W, 4, 4, CT * 16, dx.data_ptr(), None) == 0
    torch.cuda.synchronize()
    _intact(buf, 5, "pool dx")
    assert _same_bytes(dx, a)
    _log(f"adaptive_avgpool2d_bwd {H}x{W}: C entry between sentinels ok", LOG)
