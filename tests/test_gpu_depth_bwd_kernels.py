"""GPU: the backward kernels of the depth ResNet alone (csrc/depth_bwd.hip) against float64 formulas, and the conv-gradient
wrappers at the encoder's shapes.

GroupNorm backward: per output the bound is 2 x (the same formula in fp32 torch on the same inputs vs float64) + 1e-6 x
max|float64|; dz is a selection and has to be exact.  Every launch runs twice with identical bytes, every output starts as
NaN between sentinel bands that must survive, a refusal returns its code and launches nothing.  The measured values go to
depth_bwd_kernels.log in the suite's log directory before anything is asserted.
MaxPool2d(3, 2, 1) backward: integer-valued inputs (ties in every window), exact against torch's autograd."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from kernel_bar import _log, _refused, _same_bytes  # noqa: E402

DEV = torch.device("cuda:0")
LOG = "depth_bwd_kernels.log"
SENT = -777.0
E_INVALID, E_UNSUPPORTED = -1, -5


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
    v, _ = _banded(tuple(t.shape), pad, nan=False)
    v.copy_(t)
    return v


def _gn_bwd_formula(dy, x, mean, rstd, gamma, out, groups):
    """the issue's formulas in the dtype of the inputs -> (dx, dgamma, dbeta, dz)"""
    N, C, HW = x.shape
    cpg = C // groups
    dz = dy * (out > 0).to(dy.dtype) if out is not None else dy
    m, r = mean.view(N, groups, 1, 1), rstd.view(N, groups, 1, 1)
    xh = (x.view(N, groups, cpg, HW) - m) * r
    gz = gamma.view(1, groups, cpg, 1) * dz.view(N, groups, cpg, HW)
    dx = r * (gz - gz.mean((2, 3), keepdim=True) - xh * (gz * xh).mean((2, 3), keepdim=True))
    dgamma = (dz.view(N, groups, cpg, HW) * xh).sum((0, 3)).reshape(C)
    return dx.reshape(N, C, HW), dgamma, dz.sum((0, 2)), dz


GN_CASES = [(2, 6, 3, 5), (1, 32, 16, 4096), (3, 128, 1, 16), (2, 1024, 16, 16)]


@pytest.mark.parametrize("pad", [8, 5], ids=["aligned", "unaligned_view"])
@pytest.mark.parametrize("with_dz", [False, True], ids=["no_dz_out", "dz_out"])
@pytest.mark.parametrize("with_out", [False, True], ids=["no_mask", "mask"])
@pytest.mark.parametrize("N,C,groups,HW", GN_CASES)
def test_groupnorm_bwd_against_the_float64_formula(N, C, groups, HW, with_out, with_dz, pad):
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(N * 1000 + C + HW + 7 * with_out)
    x = torch.randn(N, C, HW, generator=g) * 1.5 + 0.3
    dy = torch.randn(N, C, HW, generator=g)
    gamma = torch.randn(C, generator=g) * 0.2 + 1.0
    out = torch.relu(torch.randn(N, C, HW, generator=g)) if with_out else None
    xg = x.double().view(N, groups, -1)
    mean = xg.mean(2).reshape(-1).float()  # the forward's saved statistics: fp32 values, shared by every evaluation
    rstd = (1.0 / torch.sqrt(xg.var(2, unbiased=False) + 1e-5)).reshape(-1).float()
    r64 = _gn_bwd_formula(dy.double(), x.double(), mean.double(), rstd.double(), gamma.double(),
                          None if out is None else out.double(), groups)
    r32 = _gn_bwd_formula(dy, x, mean, rstd, gamma, out, groups)

    d_dy, d_x, d_out = _put(dy, pad), _put(x, pad), (None if out is None else _put(out, pad))
    d_mean, d_rstd, d_gamma = mean.to(DEV), rstd.to(DEV), gamma.to(DEV)

    def once():
        dx, bx = _banded((N, C, HW), pad)
        dgam, bg = _banded((C,), 8)
        dbet, bb = _banded((C,), 8)
        dz, bz = _banded((N, C, HW), pad) if with_dz else (False, None)
        res = ops.groupnorm_bwd(d_dy, d_x, d_mean, d_rstd, d_gamma, groups, out=d_out, want_dz=dz, dx=dx, dgamma=dgam,
                                dbeta=dbet)
        torch.cuda.synchronize()
        for b, p, w in ((bx, pad, "dx"), (bg, 8, "dgamma"), (bb, 8, "dbeta")) + (((bz, pad, "dz"),) if with_dz else ()):
            _intact(b, p, w)
        assert (res[3] is None) == (not with_dz)
        return res

    a, b = once(), once()
    case = f"gn_bwd N{N} C{C} G{groups} HW{HW} mask{int(with_out)} dz{int(with_dz)} pad{pad}"
    bad = []
    for name, got, again, ref64, ref32 in zip(("dx", "dgamma", "dbeta"), a, b, r64, r32):
        assert _same_bytes(got, again), f"{case} {name}: two runs differ"
        got = got.cpu().double()
        assert not bool(torch.isnan(got).any()), f"{case} {name}: NaN left"
        err = float((got - ref64.reshape(got.shape)).abs().max())
        e32 = float((ref32.double() - ref64).abs().max())
        bar = 2 * e32 + 1e-6 * float(ref64.abs().max())
        _log(f"{case:60s} {name:7s} hip {err:.3e} e32 {e32:.3e} max|ref| {float(ref64.abs().max()):.3e} bar {bar:.3e} "
             f"{'ok' if err <= bar else 'OVER'}", LOG)
        if not err <= bar:
            bad.append(f"{name}: {err:.3e} > {bar:.3e}")
    if with_dz:
        assert _same_bytes(a[3], b[3])
        assert torch.equal(a[3].cpu(), r32[3].reshape(a[3].shape)), f"{case}: dz is dy where out > 0, else 0, exactly"
    assert not bad, case + ": " + "; ".join(bad)


def test_groupnorm_bwd_refusals_launch_nothing():
    from ivln_ce_amd import ops
    from ivln_ce_amd._lib import i32, i64, vp

    N, C, G, HW = 2, 8, 2, 4
    mk = lambda *s: torch.randn(*s, device=DEV)  # noqa: E731
    dy, x, out, mean, rstd, gamma = mk(N, C, HW), mk(N, C, HW), mk(N, C, HW), mk(N * G), mk(N * G).abs(), mk(C)
    L = ops._T()
    L.ivln_groupnorm_bwd_f32.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, i64, vp]
    ws = torch.full((2 * N * C + 16,), SENT, device=DEV)

    def raw(drop=None, C_=C, G_=G, ws_floats=2 * N * C):
        dx, bx = _banded((N, C, HW), 8)
        dz, bz = _banded((N, C, HW), 8)
        dg, bg = _banded((C,), 8)
        db, bb = _banded((C,), 8)
        p = dict(dy=dy, x=x, mean=mean, rstd=rstd, gamma=gamma, out=out, dx=dx, dz=dz, dgamma=dg, dbeta=db, ws=ws)
        a = {k: (None if k == drop else v.data_ptr()) for k, v in p.items()}
        rc = L.ivln_groupnorm_bwd_f32(a["dy"], a["x"], a["mean"], a["rstd"], a["gamma"], a["out"], N, C_, HW, G_, a["dx"],
                                      a["dz"], a["dgamma"], a["dbeta"], a["ws"], ws_floats, None)
        torch.cuda.synchronize()
        for t, b in ((dx, bx), (dz, bz), (dg, bg), (db, bb)):
            assert bool(torch.isnan(t).all()), f"drop={drop}: an output was written on a refusal"
            _intact(b, 8, "refusal")
        assert bool((ws == SENT).all()), "the scratch was written on a refusal"
        return rc

    for drop in ("dy", "x", "mean", "rstd", "gamma", "dx", "dgamma", "dbeta", "ws"):
        assert raw(drop) == E_INVALID, drop
    assert raw(C_=7) == E_INVALID           # C % groups != 0
    assert raw(G_=0) == E_INVALID
    assert raw(ws_floats=2 * N * C - 1) == E_INVALID
    # what cannot fit: more than 1024 channels in a group (the per-channel sums live in LDS)
    big = torch.randn(1, 1025, 1, device=DEV)
    _refused(E_UNSUPPORTED, ops.groupnorm_bwd, big, big, torch.zeros(1, device=DEV), torch.ones(1, device=DEV),
             torch.ones(1025, device=DEV), 1)
    # optional operands may be absent: out and dz_out NULL is a plain GroupNorm backward
    ops.groupnorm_bwd(dy, x, mean, rstd, gamma, G)
    torch.cuda.synchronize()


@pytest.mark.parametrize("H,W", [(7, 5), (8, 8), (1, 4)])
def test_maxpool3s2_bwd_is_exact_with_ties(H, W):
    from ivln_ce_amd import ops

    N, C = 2, 3
    g = torch.Generator().manual_seed(H * 10 + W)
    x = torch.randint(0, 3, (N, C, H, W), generator=g).float()  # three values over nine taps: every window has ties
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, 3, 2, 1)
    dy = torch.randint(-4, 5, y.shape, generator=g).float()
    y.backward(dy)
    d_x, d_dy = x.to(DEV), dy.to(DEV)
    a, b = ops.maxpool3s2_bwd(d_dy, d_x), ops.maxpool3s2_bwd(d_dy, d_x)
    torch.cuda.synchronize()
    assert _same_bytes(a, b)
    _log(f"maxpool_bwd {H}x{W}: max|got - torch| {float((a.cpu() - xr.grad).abs().max()):.1e}", LOG)
    assert torch.equal(a.cpu(), xr.grad)
    # between sentinels, through the C entry
    from ivln_ce_amd._lib import i32, vp

    L = ops._T()
    L.ivln_maxpool3s2_bwd_f32.argtypes = [vp, vp, i32, i32, i32, vp, vp]
    dx, buf = _banded((N, C, H, W), 5)
    assert L.ivln_maxpool3s2_bwd_f32(d_dy.data_ptr(), d_x.data_ptr(), N * C, H, W, dx.data_ptr(), None) == 0
    torch.cuda.synchronize()
    _intact(buf, 5, "maxpool dx")
    assert torch.equal(dx.cpu(), xr.grad)
    nan, nbuf = _banded((N, C, H, W), 5)
    assert L.ivln_maxpool3s2_bwd_f32(None, d_x.data_ptr(), N * C, H, W, nan.data_ptr(), None) == E_INVALID
    assert L.ivln_maxpool3s2_bwd_f32(d_dy.data_ptr(), d_x.data_ptr(), N * C, 0, W, nan.data_ptr(), None) == E_INVALID
    torch.cuda.synchronize()
    assert bool(torch.isnan(nan).all())


def test_weight_oi_transpose_is_a_permutation():
    from ivln_ce_amd import ops

    w = torch.randn(6, 5, 3, 3, generator=torch.Generator().manual_seed(1))
    assert torch.equal(ops.weight_oi_transpose(w.to(DEV)).cpu(), w.permute(1, 0, 2, 3).contiguous())
    w1 = torch.randn(7, 3, 1, 1, generator=torch.Generator().manual_seed(2))
    assert torch.equal(ops.weight_oi_transpose(w1.to(DEV)).cpu(), w1.permute(1, 0, 2, 3).contiguous())


# (name, N, Cin, Cout, k, stride, pad, H): the encoder's convs whose gradients take a form no other path of the update uses
CONV_CASES = [
    ("stem 7x7 s2 Cin=1", 2, 1, 32, 7, 2, 3, 128),
    ("layer2 downsample 1x1 s2", 2, 256, 512, 1, 2, 0, 32),
    ("layer2 3x3 s2", 2, 128, 128, 3, 2, 1, 32),
    ("layer4 1x1, K = N * 16", 3, 512, 2048, 1, 1, 0, 4),
    ("layer4 3x3, K = N * 16", 3, 512, 512, 3, 1, 1, 4),
    ("layer4 downsample 1x1 s2", 3, 1024, 2048, 1, 2, 0, 8),
]


@pytest.mark.parametrize("name,N,Cin,Cout,k,s,p,H", CONV_CASES, ids=[c[0].replace(" ", "_") for c in CONV_CASES])
def test_conv_gradients_at_the_encoder_shapes(name, N, Cin, Cout, k, s, p, H):
    """train._conv_backward (conv2d_bwd_weight; conv2d over the flipped weights, or conv_transpose2d with output padding 1
    for stride 2) against float64 autograd at the project's gradient bar: max|err| <= 1e-3 max|ref| + 2e-7, cosine >= 1 - 1e-6
    (tests/test_gpu_train.py).  The stem takes no input gradient."""
    import types

    from depth_twin import compare

    from ivln_ce_amd import train

    g = torch.Generator().manual_seed(Cin + Cout + k)
    x = torch.randn(N, Cin, H, H, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * (2.0 / (Cin * k * k)) ** 0.5
    Ho = (H + 2 * p - k) // s + 1
    dy = torch.randn(N, Cout, Ho, Ho, generator=g)
    res = torch.randn(N, Cin, H, H, generator=g)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    F.conv2d(xr, wr, None, s, p).backward(dy.double())
    conv = types.SimpleNamespace(weight=w.to(DEV), stride=(s, s), padding=(p, p))
    need_dx = Cin > 1
    outs = []
    for _ in range(2):
        G = {}
        dx = train._conv_backward(conv, dy.to(DEV), x.to(DEV), G, need_dx=need_dx, residual=res.to(DEV) if need_dx else None)
        outs.append((G[conv.weight], dx))
    torch.cuda.synchronize()
    assert _same_bytes(outs[0][0], outs[1][0]) and (not need_dx or _same_bytes(outs[0][1], outs[1][1]))
    got, ref = {"dW": outs[0][0]}, {"dW": wr.grad}
    if need_dx:
        got["dX+res"], ref["dX+res"] = outs[0][1], xr.grad + res.double()
    log, bad = compare(got, ref)
    for line in log:
        _log(f"conv_bwd {name}: {line}", LOG)
    assert not bad, name + "\n" + "\n".join(bad)
