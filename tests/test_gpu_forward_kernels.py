"""Per-kernel GPU parity of the non-GEMM forward kernels (csrc/nn_ops.hip, the "Non-GEMM forward kernels" section of
include/ivln_hip.h), each alone, at the sizes where the kernel changes path, against the same operation written in plain
torch in float64 on the CPU.  Nothing here imports oracle/, ivln_ce_amd.policy, rednet or train.

Inputs are drawn in fp32 from a seeded generator and widened for the reference, so both sides see the same numbers.

Error bar (tests/kernel_bar.py, the one of tests/test_gpu_train_kernels.py): e32 = max|fp32 torch-CPU - float64| on the
case's inputs; a kernel must stay within  4 * e32 + 4 * 2^-24 * max|float64|.  Pure data movement and selection (copies,
map features, embedding gather, arg-maxes, previous-action embedding, tour memory, max-pool, subsample) and the single
correctly rounded fp32 add (add, add_multi) are compared for equal values / bytes.  Every kernel runs twice on the same
inputs and must give the same bytes.  Every output written through a stride or a slice, and every workspace with a
documented size, lies inside a larger buffer filled with a sentinel that must survive.  Every comparison goes to
forward_kernels.log in the suite's log directory (hip / e32 ratio, or `exact`).

FWD_COVERED (bottom of the file) names the test of every entry point of the section; tests/test_forward_kernel_coverage.py
(CPU) pins it to the header."""
import ctypes as C
import types

import pytest
import torch
import torch.nn.functional as F

from kernel_bar import _Bar, _log, _refused, _same_bytes, _twice

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOG = "forward_kernels.log"
E_INVALID, E_UNSUPPORTED = -1, -5
SENT = -777.0   # float sentinel of the guard bands
SENT_U8 = 0xA5
PAD = 8         # guard elements on either side (32 bytes of floats: the view stays 16-byte aligned)

vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float


def _lib():
    """the library with the signatures of the entry points this file calls through the C ABI"""
    from ivln_ce_amd import ops

    L = ops._L()
    L.ivln_groupnorm2_f32.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, i32, i64, i64, i32, i64, i64, i64, vp,
                                      vp, vp, vp, vp, i64, i64, i32, i64, vp]
    L.ivln_bn_stats_from_partials_f32.argtypes = [vp, i32, i32, vp, vp, vp, vp, f32, f32, vp, vp, vp, vp, vp]
    L.ivln_attn_fwd_idx_f32.argtypes = [vp, i64, vp, i64, vp, i64, vp, f32, i32, i32, i32, i32, vp, i64, vp, vp, vp, vp]
    L.ivln_attn_small2_f32.argtypes = [vp, i64, f32, i32, i32, vp, i64, vp, i64, i32, i32, vp, i64, vp, i64, vp, i64,
                                       i32, i32, vp, i64, vp]
    L.ivln_kv_linear_f32.argtypes = [vp, i32, i32, i32, vp, vp, i32, vp, vp, vp, i32, i32, vp, i64, vp]
    L.ivln_copy_multi.argtypes = [C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), i32, vp]
    L.ivln_add_multi_f32.argtypes = [C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), i32, vp]
    return L


def _sp():
    from ivln_ce_amd import ops

    return ops.stream_ptr()


def _bar(case):
    return _Bar(case, LOG)


def _exact(case, name, got, want):
    """equal values (and shapes and dtypes), logged like the bar's lines"""
    got, want = got.detach().cpu(), want.detach().cpu()
    ok = got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want)
    _log(f"{case:44s} {name:10s} exact  {'ok' if ok else 'OVER'}", LOG)
    assert ok, f"{case} {name}: not equal to the reference"


def _band(n, dtype=torch.float32, fill=None, pad=PAD):
    """n elements inside a sentinel-filled buffer: (view, buffer)"""
    if fill is None:
        fill = SENT if dtype.is_floating_point else (SENT_U8 if dtype == torch.uint8 else -99)
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=DEV)
    return buf[pad:pad + n], buf


def _band_ok(buf, n, what, pad=PAD):
    fill = buf[0].item()
    assert bool((buf[:pad] == fill).all()) and bool((buf[pad + n:] == fill).all()), f"{what}: written outside its {n} elements"


def _cols(rows, cols, left=4, right=4, dtype=torch.float32):
    """a (rows, cols) column slice of a wider sentinel-filled matrix: (view, matrix)"""
    wide = torch.full((rows, left + cols + right), SENT, dtype=dtype, device=DEV)
    return wide[:, left:left + cols], wide


def _cols_ok(wide, left, cols, what):
    assert bool((wide[:, :left] == SENT).all()) and bool((wide[:, left + cols:] == SENT).all()), f"{what}: written outside its columns"


def _in_cols(t, left=4, right=4):
    """the same 2-D values as a column slice of a wider matrix, on the GPU"""
    v, _ = _cols(t.shape[0], t.shape[1], left, right, t.dtype)
    v.copy_(t)
    return v


def _off_by_one(t):
    """the same contiguous values one element into a larger buffer (4 bytes / 1 byte off a 16-byte boundary)"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
    return v


def _gen(*seed):
    s = 0
    for k in seed:
        s = s * 1009 + int(k)
    return torch.Generator().manual_seed(s % (2 ** 31))


# ------------------------------------------------------------------------------------------------------------------
# GroupNorm (+ second operand) (+ residual) (+ ReLU)
# ------------------------------------------------------------------------------------------------------------------
EPS_GN = 1e-5


def _gn_ref(x, x2, gamma, beta, gamma2, beta2, res, relu, G, dt):
    """x, x2: (N, C, HW) already reduced over their slabs, in dt"""
    y = F.group_norm(x, G, gamma.to(dt), beta.to(dt), EPS_GN)
    if x2 is not None:
        y = y + F.group_norm(x2, G, gamma2.to(dt), beta2.to(dt), EPS_GN)
    if res is not None:
        y = y + res.to(dt)
    if relu:
        y = F.relu(y)
    N = x.shape[0]
    xg = x.reshape(N, G, -1)
    mean = xg.mean(-1)
    rstd = (((xg - mean.unsqueeze(-1)) ** 2).mean(-1) + EPS_GN).rsqrt()
    return y, mean.reshape(-1), rstd.reshape(-1)


def _slabs(N, C, HW, splits, g):
    """split-K slabs [splits][C][N*HW] in fp32 and their sums as (N, C, HW) tensors in float64 / fp32"""
    s = torch.randn(splits, C, N * HW, generator=g)
    as_img = lambda t: t.view(C, N, HW).permute(1, 0, 2).contiguous()
    return s, as_img(s.double().sum(0)), as_img(s.sum(0))


def _gn_run(case, N, C, HW, G, relu, res, x, x2, gamma, beta, gamma2, beta2):
    """x / x2: ("raw", device tensor (N, C, HW)) or ("slabs", device tensor, splits).  Returns y, mean, rstd."""
    L = _lib()

    def operand(o):
        if o is None:
            return None, 0, 0, 1, 0
        if o[0] == "raw":
            return o[1].data_ptr(), 0, 0, 1, 0
        return o[1].data_ptr(), HW, N * HW, o[2], C * N * HW

    xp, x_img, x_chan, splits, slab = operand(x)
    x2p, x2_img, x2_chan, splits2, slab2 = operand(x2)
    ctot = C + 2   # y: a channel slice of a wider NCHW buffer, the residual another
    res_w = None
    if res is not None:
        res_w = torch.full((N, C + 1, HW), 3.0, device=DEV)
        res_w[:, :C] = res.to(DEV)

    def run():
        y_w = torch.full((N, ctot, HW), SENT, device=DEV)
        mean, mean_b = _band(N * G)
        rstd, rstd_b = _band(N * G)
        rc = L.ivln_groupnorm2_f32(xp, gamma.data_ptr(), beta.data_ptr(), None if res_w is None else res_w.data_ptr(),
                                   y_w.data_ptr(), N, C, HW, G, EPS_GN, int(relu), x_img, x_chan, splits, slab, ctot * HW,
                                   (C + 1) * HW, mean.data_ptr(), rstd.data_ptr(), x2p,
                                   None if x2 is None else gamma2.data_ptr(), None if x2 is None else beta2.data_ptr(),
                                   x2_img, x2_chan, splits2, slab2, _sp())
        assert rc == 0, rc
        return y_w, mean_b, rstd_b

    y_w, mean_b, rstd_b = _twice(run)
    assert bool((y_w[:, C:] == SENT).all()), f"{case}: y written outside its channel slice"
    _band_ok(mean_b, N * G, case + " save_mean")
    _band_ok(rstd_b, N * G, case + " save_rstd")
    if x2 is None:   # the entry point without a second operand is the same launch
        y1 = torch.full((N, ctot, HW), SENT, device=DEV)
        rc = L.ivln_groupnorm_f32(xp, gamma.data_ptr(), beta.data_ptr(), None if res_w is None else res_w.data_ptr(),
                                  y1.data_ptr(), N, C, HW, G, EPS_GN, int(relu), x_img, x_chan, splits, slab, ctot * HW,
                                  (C + 1) * HW, None, None, _sp())
        assert rc == 0 and _same_bytes(y1, y_w), f"{case}: ivln_groupnorm_f32 and ivln_groupnorm2_f32 differ"
    return y_w[:, :C], mean_b[PAD:PAD + N * G], rstd_b[PAD:PAD + N * G]


def _gn_params(C, g):
    return [(torch.rand(C, generator=g) + 0.5), torch.randn(C, generator=g) * 0.3, (torch.rand(C, generator=g) + 0.5),
            torch.randn(C, generator=g) * 0.3]


def _gn_check(case, got, x64, x32, x2_64, x2_32, p, res, relu, G):
    r64 = _gn_ref(x64, x2_64, p[0], p[1], p[2], p[3], res, relu, G, torch.float64)
    r32 = _gn_ref(x32, x2_32, p[0], p[1], p[2], p[3], res, relu, G, torch.float32)
    bar = _bar(case)
    for name, a, b, c in zip(("y", "save_mean", "save_rstd"), got, r64, r32):
        bar.check(name, a, b, c)
    bar.done()


@pytest.mark.parametrize("res_relu", [False, True], ids=["plain", "res+relu"])
@pytest.mark.parametrize("N,C,H,W,G,path", [(1, 6, 52, 54, 2, "uncached float4"), (1, 6, 52, 53, 2, "uncached float4"),
                                            (1, 6, 53, 53, 2, "uncached scalar"), (2, 6, 52, 52, 2, "cached")])
def test_groupnorm(N, C, H, W, G, path, res_relu):
    """k_groupnorm on an NCHW tensor on either side of n = (C/G)*HW = 8192 (GN_CACHE): n = 8424 and n = 8268 (HW = 52 * 53
    is still a multiple of 4) re-read the input by float4 for the output pass and by scalar for the variance pass, n = 8427
    (HW = 53 * 53, odd) by scalar for both, n = 8112 stays in LDS.  With and without residual + ReLU; y and the residual are channel slices of wider buffers; the
    first shape also with the second normalised operand (ivln_groupnorm2_f32)."""
    HW = H * W
    n = C // G * HW
    assert (n > 8192) == path.startswith("uncached") and ((HW % 4 == 0) == (path != "uncached scalar"))
    g = _gen(N, C, H, W, res_relu)
    x = torch.randn(N, C, HW, generator=g) * 1.5 + 0.25
    x2 = torch.randn(N, C, HW, generator=g)
    res = torch.randn(N, C, HW, generator=g) if res_relu else None
    p = _gn_params(C, g)
    pd = [t.to(DEV) for t in p]
    x_d, x2_d = x.to(DEV), x2.to(DEV)
    for second in ([False, True] if (H, W) == (52, 54) else [False]):
        case = f"groupnorm {N}x{C}x{H}x{W} g{G} {'res+relu' if res_relu else 'plain'}{' +x2' if second else ''}"
        got = _gn_run(case, N, C, HW, G, res_relu, res, ("raw", x_d), ("raw", x2_d) if second else None, *pd)
        _gn_check(case, got, x.double(), x, x2.double() if second else None, x2 if second else None, p, res, res_relu, G)


GN_SLAB_CASES = ([(16, s, "cooperative") for s in (2, 33, 64)] + [(128, s, "cooperative") for s in (2, 3, 5, 8)]
                 + [(256, 3, "cooperative")] + [(260, s, "by-4 loop") for s in (1, 2, 4, 5, 6)])


@pytest.mark.parametrize("HW,splits,path", GN_SLAB_CASES)
def test_groupnorm_over_split_k_slabs(HW, splits, path):
    """k_groupnorm reading the producing conv's split-K slabs ([splits][C][N*HW], built here by hand), C = 16 in 4 groups,
    N = 2.  Cooperative path (splits > 1, n/4*2 <= 512, 2n <= 8192): n = 64 with nz = min(32, splits, 128) slab slots - 33
    and 64 slabs leave nz = 32 with the odd-tail branch of gn_load4_strided taken (33) or not (64) -, n = 512 with nz =
    min(4, splits): 2, 3 (z0 = 2 has no partner), 4 of 5 and 4 of 8 slabs, n = 1024 is the n/4*2 == 512 boundary (nz = 2
    of 3).  n = 1040 is just outside: gn_load4's by-4 slab loop and its tail at 1, 2, 4, 5, 6 slabs.  Reference: float64
    sum of the slabs, then F.group_norm.  With ReLU and a residual; n = 512 / 5 slabs also with a second operand that
    is itself 3 slabs."""
    N, C, G = 2, 16, 4
    n = C // G * HW
    coop = splits > 1 and n // 4 * 2 <= 512 and 2 * n <= 8192
    assert coop == (path == "cooperative") and HW % 4 == 0
    g = _gen(HW, splits)
    s, x64, x32 = _slabs(N, C, HW, splits, g)
    second = (HW, splits) == (128, 5)
    s2, x2_64, x2_32 = _slabs(N, C, HW, 3, g) if second else (None, None, None)
    res = torch.randn(N, C, HW, generator=g)
    p = _gn_params(C, g)
    pd = [t.to(DEV) for t in p]
    s_d = s.to(DEV)
    case = f"groupnorm slabs n={n} splits={splits}{' +x2(3 slabs)' if second else ''}"
    got = _gn_run(case, N, C, HW, G, True, res, ("slabs", s_d, splits), ("slabs", s2.to(DEV), 3) if second else None, *pd)
    _gn_check(case, got, x64, x32, x2_64, x2_32, p, res, True, G)


def test_groupnorm_refusals_and_views_off_the_vector_boundary():
    """C % groups != 0 is refused.  HW % 4 == 0 alone does not make the float4 path safe: an input one float into a buffer,
    or a slab stride that is no multiple of 4, takes the scalar path (the launcher's check) and gives the same values
    within the bar."""
    L = _lib()
    z = torch.zeros(64, device=DEV)
    assert L.ivln_groupnorm_f32(z.data_ptr(), z.data_ptr(), z.data_ptr(), None, z.data_ptr(), 1, 6, 4, 4, EPS_GN, 0, 0, 0, 1,
                                0, 0, 0, None, None, _sp()) == E_INVALID
    N, C, HW, G = 2, 8, 16, 2
    g = _gen(77)
    x = torch.randn(N, C, HW, generator=g)
    p = _gn_params(C, g)
    pd = [t.to(DEV) for t in p]
    case = "groupnorm 2x8x16 x one float off"
    got = _gn_run(case, N, C, HW, G, False, None, ("raw", _off_by_one(x)), None, *pd)
    _gn_check(case, got, x.double(), x, None, None, p, None, False, G)
    # slabs whose stride is C*N*HW + 1 floats
    splits = 3
    s, x64, x32 = _slabs(N, C, HW, splits, g)
    loose = torch.zeros(splits, C * N * HW + 1, device=DEV)
    loose[:, :C * N * HW] = s.view(splits, -1).to(DEV)
    case = "groupnorm 2x8x16 slab stride % 4 == 1"
    y_w = torch.full((N, C, HW), SENT, device=DEV)
    rc = L.ivln_groupnorm_f32(loose.data_ptr(), pd[0].data_ptr(), pd[1].data_ptr(), None, y_w.data_ptr(), N, C, HW, G, EPS_GN, 0,
                              HW, N * HW, splits, C * N * HW + 1, 0, 0, None, None, _sp())
    assert rc == 0
    bar = _bar(case)
    bar.check("y", y_w, _gn_ref(x64, None, p[0], p[1], None, None, None, False, G, torch.float64)[0],
              _gn_ref(x32, None, p[0], p[1], None, None, None, False, G, torch.float32)[0])
    bar.done()


# ------------------------------------------------------------------------------------------------------------------
# BatchNorm: eval folding, train-mode statistics, statistics from per-tile partials
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "conv_bias"])
@pytest.mark.parametrize("Cc", [1, 64, 65])
def test_bn_fold(Cc, bias):
    """ivln_bn_fold_f32: scale = gamma / sqrt(rv + eps), shift = beta - (rm - conv_bias) * scale; C on either side of the
    64-thread block."""
    from ivln_ce_amd import ops

    g = _gen(Cc, bias)
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g)
    rm, rv = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.1
    cb = torch.randn(Cc, generator=g) if bias else None
    bn = types.SimpleNamespace(weight=gamma.to(DEV), bias=beta.to(DEV), running_mean=rm.to(DEV), running_var=rv.to(DEV),
                               eps=1e-5, num_features=Cc)
    cb_d = cb.to(DEV) if bias else None

    def run():
        sc, sc_b = _band(Cc)
        sh, sh_b = _band(Cc)
        ops.bn_fold(bn, sc, sh, cb_d)
        return sc_b, sh_b

    sc_b, sh_b = _twice(run)
    _band_ok(sc_b, Cc, "scale")
    _band_ok(sh_b, Cc, "shift")

    def ref(dt):
        sc = gamma.to(dt) / (rv.to(dt) + 1e-5).sqrt()
        m = rm.to(dt) - (cb.to(dt) if bias else 0)
        return sc, beta.to(dt) - m * sc

    bar = _bar(f"bn_fold C={Cc} {'conv_bias' if bias else 'nobias'}")
    for name, a, b, c in zip(("scale", "shift"), (sc_b[PAD:PAD + Cc], sh_b[PAD:PAD + Cc]), ref(torch.float64), ref(torch.float32)):
        bar.check(name, a, b, c)
    bar.done()


def _bn_ref(x, gamma, beta, rm, rv, mom, eps, dt):
    """train-mode nn.BatchNorm2d statistics over (N, C, HW) in dt: scale, shift, mean, rstd, running mean / variance"""
    x = x.to(dt)
    cnt = x.shape[0] * x.shape[2]
    mean = x.mean((0, 2))
    var = ((x - mean.view(1, -1, 1)) ** 2).mean((0, 2))
    rstd = (var + eps).rsqrt()
    sc = gamma.to(dt) * rstd
    unbiased = var * cnt / (cnt - 1) if cnt > 1 else var
    return (sc, beta.to(dt) - mean * sc, mean, rstd, (1 - mom) * rm.to(dt) + mom * mean, (1 - mom) * rv.to(dt) + mom * unbiased)


BN_NAMES = ("scale", "shift", "save_mean", "save_rstd", "run_mean", "run_var")


def _bn_finish(case, outs_b, Cc, refs64, refs32, keep=None):
    bar = _bar(case)
    bars = []
    for name, b_, r64, r32 in zip(BN_NAMES, outs_b, refs64, refs32):
        _band_ok(b_, Cc, f"{case} {name}")
        bars.append(bar.check(name, b_[PAD:PAD + Cc], r64, r32)[1])
    if keep is not None:
        for name, b_, other, lim in zip(BN_NAMES, outs_b, keep, bars):
            bar.within(name, b_[PAD:PAD + Cc], other[PAD:PAD + Cc], lim)
    bar.done()


@pytest.mark.parametrize("N,Cc,HW,far", [(5, 3, 4096, False), (3, 3, 90 * 91, False), (1, 2, 16, False), (5, 3, 4096, True)],
                         ids=["3+2 images", "2+1 images scalar", "one block", "mean 100 std 0.1"])
def test_bn_train_stats(N, Cc, HW, far):
    """k_bn_stats_partial + k_bn_stats_final: (5, 3, 4096) is two splits of 3 and 2 images (Chan merge with unequal
    counts), (3, 3, 8190) the non-vector path with splits of 2 and 1 images, (1, 2, 16) a single block; the first again
    with mean 100 and std 0.1 (a one-pass variance would cancel).  A workspace of 3*C floats forces one split, which must
    agree with the default within the bar; both workspaces lie in sentinel bands.  Running mean / variance (unbiased,
    momentum 0.1) and the saved mean / rstd go against float64.  ws_floats < 3*C is refused."""
    L = _lib()
    S = min((N * HW + 16383) // 16384, N, 64)
    ips = -(-N // S)
    assert [min(ips, N - k) for k in range(0, N, ips)] == {5: [3, 2], 3: [2, 1], 1: [1]}[N]
    assert (HW % 4 != 0) == (HW == 8190)
    g = _gen(N, Cc, HW, far)
    x = torch.randn(N, Cc, HW, generator=g)
    x = x * 0.1 + 100.0 if far else x * torch.tensor([1.0, 0.5, 2.0])[:Cc].view(1, -1, 1) + torch.tensor([0.3, -1.0, 2.0])[:Cc].view(1, -1, 1)
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.3
    rm, rv = torch.randn(Cc, generator=g) * 0.1, torch.rand(Cc, generator=g) + 0.5
    mom, eps = 0.1, 1e-5
    x_d, gamma_d, beta_d = x.to(DEV), gamma.to(DEV), beta.to(DEV)

    def launch(ws_floats, full):
        def run():
            outs = [_band(Cc) for _ in range(6)]
            outs[4][0].copy_(rm)
            outs[5][0].copy_(rv)
            ws, ws_b = _band(full)
            rc = L.ivln_bn_train_stats_f32(x_d.data_ptr(), N, Cc, HW, gamma_d.data_ptr(), beta_d.data_ptr(), outs[4][0].data_ptr(),
                                           outs[5][0].data_ptr(), mom, eps, outs[0][0].data_ptr(), outs[1][0].data_ptr(),
                                           outs[2][0].data_ptr(), outs[3][0].data_ptr(), ws.data_ptr(), ws_floats, _sp())
            assert rc == 0, rc
            return tuple(o[1] for o in outs) + (ws_b,)
        got = _twice(run)
        _band_ok(got[6], ws_floats, "bn_train_stats workspace")
        return got[:6]

    refs64 = _bn_ref(x, gamma, beta, rm, rv, mom, eps, torch.float64)
    refs32 = _bn_ref(x, gamma, beta, rm, rv, mom, eps, torch.float32)
    case = f"bn_train_stats {N}x{Cc}x{HW}{' far' if far else ''}"
    default = launch(3 * Cc * 64, 3 * Cc * 64)
    _bn_finish(case, default, Cc, refs64, refs32)
    one = launch(3 * Cc, 3 * Cc * 64)   # the same band, but only 3*C floats of it are the kernel's
    _bn_finish(case + " ws=3C", one, Cc, refs64, refs32, keep=default)
    z = torch.zeros(8, device=DEV)
    assert L.ivln_bn_train_stats_f32(x_d.data_ptr(), N, Cc, HW, gamma_d.data_ptr(), beta_d.data_ptr(), None, None, mom, eps,
                                     z.data_ptr(), z.data_ptr(), None, None, x_d.data_ptr(), 3 * Cc - 1, _sp()) == E_INVALID


@pytest.mark.parametrize("tiles", [1, 2, 1025])
def test_bn_stats_from_partials(tiles):
    """k_bn_stats_from_tiles on hand-made [tiles][C][3] = {count, mean, M2} partials, some tiles with count 0 (whose mean
    and M2 are garbage that must not be read into the result): one tile, two, and 1025 (thread 0 folds two tiles before
    the LDS tree).  Reference: the pooled statistics of the same fp32 partials in float64."""
    L = _lib()
    Cc = 3
    g = _gen(tiles)
    cnt = torch.randint(1, 50, (tiles, Cc), generator=g).float()
    if tiles > 1:
        cnt[torch.rand(tiles, generator=g) < 0.2] = 0.0
        cnt[0], cnt[-1, 1] = 0.0, 0.0
        cnt[1] = torch.tensor([7.0, 1.0, 40.0])
    mean = torch.randn(tiles, Cc, generator=g) * 0.5 + torch.tensor([0.0, 3.0, -1.0])
    m2 = (torch.rand(tiles, Cc, generator=g) + 0.5) * cnt.clamp(min=1.0)
    part = torch.stack((cnt, mean, m2), -1).contiguous()
    part[cnt == 0] = torch.tensor([0.0, 1e30, 1e30])   # never read
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.3
    rm, rv = torch.randn(Cc, generator=g) * 0.1, torch.rand(Cc, generator=g) + 0.5
    mom, eps = 0.1, 1e-5
    part_d, gamma_d, beta_d = part.to(DEV), gamma.to(DEV), beta.to(DEV)

    def run():
        outs = [_band(Cc) for _ in range(6)]
        outs[4][0].copy_(rm)
        outs[5][0].copy_(rv)
        rc = L.ivln_bn_stats_from_partials_f32(part_d.data_ptr(), tiles, Cc, gamma_d.data_ptr(), beta_d.data_ptr(),
                                               outs[4][0].data_ptr(), outs[5][0].data_ptr(), mom, eps, outs[0][0].data_ptr(),
                                               outs[1][0].data_ptr(), outs[2][0].data_ptr(), outs[3][0].data_ptr(), _sp())
        assert rc == 0, rc
        return tuple(o[1] for o in outs)

    def ref(dt):
        live = (cnt > 0).to(dt)
        n_, m_, q_ = cnt.to(dt), mean.to(dt) * live, m2.to(dt) * live
        tot = n_.sum(0)
        mu = (n_ * m_).sum(0) / tot
        M2 = q_.sum(0) + (n_ * (m_ - mu) ** 2 * live).sum(0)
        var = M2 / tot
        rstd = (var + eps).rsqrt()
        sc = gamma.to(dt) * rstd
        unb = torch.where(tot > 1, M2 / (tot - 1).clamp(min=1), var)
        return sc, beta.to(dt) - mu * sc, mu, rstd, (1 - mom) * rm.to(dt) + mom * mu, (1 - mom) * rv.to(dt) + mom * unb

    _bn_finish(f"bn_stats_from_partials tiles={tiles}", _twice(run), Cc, ref(torch.float64), ref(torch.float32))
    assert L.ivln_bn_stats_from_partials_f32(part_d.data_ptr(), 0, Cc, gamma_d.data_ptr(), beta_d.data_ptr(), None, None, mom, eps,
                                             gamma_d.data_ptr(), gamma_d.data_ptr(), None, None, _sp()) == E_INVALID


# ------------------------------------------------------------------------------------------------------------------
# BatchNorm scale / shift -> ReLU -> AvgPool2d(2)
# ------------------------------------------------------------------------------------------------------------------
def lanes_per_output(splits, total):
    """the launcher's choice (ivln_scale_shift_relu_avgpool2_f32)"""
    lpo = 1
    while lpo < 16 and lpo * 2 <= splits and total * lpo < 65536:
        lpo *= 2
    return lpo


def _ssra_ref(x, sc, sh, dt):
    return F.avg_pool2d(F.relu(x * sc.to(dt).view(1, -1, 1, 1) + sh.to(dt).view(1, -1, 1, 1)), 2)


@pytest.mark.parametrize("splits", [1, 2, 3, 7, 16, 33])
def test_scale_shift_relu_avgpool2_over_slabs(splits):
    """k_scale_shift_relu_avgpool2 on hand-made split-K slabs of a (1, 2, 4, 4) map: 8 outputs, lpo = 1, 2, 2, 4, 16, 16
    lanes per output (8 * lpo live lanes of a 256-thread block: the rest stay in the shuffles with idx = 0), each lane
    summing slabs sub, sub + lpo, ... ."""
    L = _lib()
    N, Cc, H, W = 1, 2, 4, 4
    total = N * Cc * (H // 2) * (W // 2)
    assert lanes_per_output(splits, total) == {1: 1, 2: 2, 3: 2, 7: 4, 16: 16, 33: 16}[splits]
    g = _gen(splits, 5)
    s = torch.randn(splits, Cc, N * H * W, generator=g)
    sc, sh = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.3
    as_img = lambda t: t.view(Cc, N, H, W).permute(1, 0, 2, 3).contiguous()
    s_d, sc_d, sh_d = s.to(DEV), sc.to(DEV), sh.to(DEV)

    def run():
        y, y_b = _band(total)
        rc = L.ivln_scale_shift_relu_avgpool2_f32(s_d.data_ptr(), sc_d.data_ptr(), sh_d.data_ptr(), y.data_ptr(), N, Cc, H, W,
                                                  H * W, N * H * W, splits, Cc * N * H * W, _sp())
        assert rc == 0, rc
        return (y_b,)

    (y_b,) = _twice(run)
    _band_ok(y_b, total, "avgpool2 output")
    bar = _bar(f"scale_shift_relu_avgpool2 slabs={splits}")
    bar.check("y", y_b[PAD:PAD + total], _ssra_ref(as_img(s.double().sum(0)), sc, sh, torch.float64),
              _ssra_ref(as_img(s.sum(0)), sc, sh, torch.float32))
    bar.done()


def test_scale_shift_relu_avgpool2_nchw_and_alignment_refusals():
    """The NCHW form at (2, 3, 6, 10) (W % 4 != 0, 45 outputs).  The kernel reads two neighbouring pixels with one 8-byte
    load: an input 4 bytes off an 8-byte boundary and an odd channel / slab stride are refused before anything is
    launched (the odd-size refusal is tested in tests/test_gpu_kernels.py)."""
    from ivln_ce_amd import ops

    L = _lib()
    N, Cc, H, W = 2, 3, 6, 10
    g = _gen(6, 10)
    x = torch.randn(N, Cc, H, W, generator=g)
    sc, sh = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.3
    x_d, sc_d, sh_d = x.to(DEV), sc.to(DEV), sh.to(DEV)
    total = N * Cc * (H // 2) * (W // 2)

    def run():
        y, y_b = _band(total)
        ops.scale_shift_relu_avgpool2(x_d, sc_d, sh_d, out=y.view(N, Cc, H // 2, W // 2))
        return (y_b,)

    (y_b,) = _twice(run)
    _band_ok(y_b, total, "avgpool2 output")
    bar = _bar("scale_shift_relu_avgpool2 2x3x6x10")
    bar.check("y", y_b[PAD:PAD + total], _ssra_ref(x.double(), sc, sh, torch.float64), _ssra_ref(x, sc, sh, torch.float32))
    bar.done()
    y = torch.zeros(total, device=DEV)
    call = lambda xp, img, chan, splits, slab: L.ivln_scale_shift_relu_avgpool2_f32(
        xp, sc_d.data_ptr(), sh_d.data_ptr(), y.data_ptr(), N, Cc, H, W, img, chan, splits, slab, _sp())
    off = _off_by_one(x)
    assert off.data_ptr() % 8 == 4
    assert call(off.data_ptr(), 0, 0, 1, 0) == E_INVALID
    assert call(x_d.data_ptr(), Cc * H * W, H * W + 1, 1, 0) == E_INVALID
    assert call(x_d.data_ptr(), Cc * H * W + 1, H * W, 1, 0) == E_INVALID
    assert call(x_d.data_ptr(), H * W, N * H * W, 2, Cc * N * H * W + 1) == E_INVALID
    assert call(x_d.data_ptr(), 0, 0, 1, 7) == 0   # one slab: its stride is not used


# ------------------------------------------------------------------------------------------------------------------
# pooling, map features, embedding + lengths
# ------------------------------------------------------------------------------------------------------------------
def _pool_run(x_d, k, s, p, mode):
    from ivln_ce_amd import ops

    N, Cc, H, W = x_d.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    n = N * Cc * Ho * Wo

    def run():
        y, y_b = _band(n)
        ops.pool2d(x_d, k, s, p, mode, out=y.view(N, Cc, Ho, Wo))
        return (y_b,)

    (y_b,) = _twice(run)
    _band_ok(y_b, n, "pool2d output")
    return y_b[PAD:PAD + n].view(N, Cc, Ho, Wo)


@pytest.mark.parametrize("shape,path", [((2, 3, 4, 8), "x4"), ((1, 2, 6, 16), "x4"), ((1, 2, 5, 8), "generic: odd H"),
                                        ((1, 2, 4, 12), "generic: W % 8"), ((2, 3, 4, 8), "generic: view one float off")])
def test_pool2d_subsample(shape, path):
    """k = 1, s = 2, p = 0: k_subsample2_x4 (W % 8 == 0, even H, 16-byte aligned) and the generic kernel on the other side of
    each dispatch condition, all equal to x[..., ::2, ::2]."""
    N, Cc, H, W = shape
    fast = W % 8 == 0 and H % 2 == 0 and "off" not in path
    assert fast == (path == "x4")
    x = torch.randn(*shape, generator=_gen(*shape))
    x_d = _off_by_one(x) if "off" in path else x.to(DEV)
    for mode in ("max", "avg"):   # one value per output: the mode is irrelevant
        _exact(f"pool2d subsample {shape} {path}", mode, _pool_run(x_d, 1, 2, 0, mode), x[..., ::2, ::2].contiguous())


def test_pool2d_average_and_max():
    """Average pooling with padding divides by k*k (count_include_pad=True) and clips the window at the border; max pooling
    takes the values it compares unchanged (exact)."""
    g = _gen(57)
    x = torch.randn(1, 2, 5, 7, generator=g)
    bar = _bar("pool2d avg k3 s2 p1 1x2x5x7")
    bar.check("y", _pool_run(x.to(DEV), 3, 2, 1, "avg"), F.avg_pool2d(x.double(), 3, 2, 1, count_include_pad=True),
              F.avg_pool2d(x, 3, 2, 1, count_include_pad=True))
    bar.done()
    x1 = torch.randn(1, 1, 5, 7, generator=g)
    bar = _bar("pool2d avg k2 s2 p0 1x1x5x7")
    bar.check("y", _pool_run(x1.to(DEV), 2, 2, 0, "avg"), F.avg_pool2d(x1.double(), 2, 2, 0), F.avg_pool2d(x1, 2, 2, 0))
    bar.done()
    _exact("pool2d max k2 s2 p0 1x2x5x7", "y", _pool_run(x.to(DEV), 2, 2, 0, "max"), F.max_pool2d(x, 2, 2, 0))
    _exact("pool2d max k3 s2 p1 1x2x5x7", "y", _pool_run(x.to(DEV), 3, 2, 1, "max"), F.max_pool2d(x, 3, 2, 1))


@pytest.mark.parametrize("off", [False, True], ids=["aligned", "one byte off"])
@pytest.mark.parametrize("classes", [13, 5])
@pytest.mark.parametrize("B,rows,cols", [(2, 5, 5), (1, 4, 4)])
def test_map_features(B, rows, cols, classes, off):
    """k_map_features (cells % 4 != 0, or u8 views one byte into a buffer) and k_map_features4: channel 0 is the occupancy
    as a float, channel 1 + c is (label == c).  Labels >= classes (255 among them) give all-zero class planes; the
    reference is written by comparison."""
    from ivln_ce_amd import ops

    cells = rows * cols
    g = _gen(B, rows, cols, classes)
    occ = torch.randint(0, 256, (B, rows, cols), generator=g).to(torch.uint8)
    sem = torch.randint(0, classes + 3, (B, rows, cols), generator=g).to(torch.uint8)
    sem[0, 0, 0], sem[0, 1, 1], sem[-1, -1, -1], sem[0, 2, 2] = 255, classes, classes - 1, 0
    occ_d, sem_d = (_off_by_one(occ), _off_by_one(sem)) if off else (occ.to(DEV), sem.to(DEV))
    n = B * (1 + classes) * cells

    def run():
        y, y_b = _band(n)
        ops.map_features(occ_d, sem_d, classes, out=y.view(B, 1 + classes, rows, cols))
        return (y_b,)

    (y_b,) = _twice(run)
    _band_ok(y_b, n, "map_features output")
    want = torch.zeros(B, 1 + classes, rows, cols)
    want[:, 0] = occ.float()
    for c in range(classes):
        want[:, 1 + c] = (sem == c).float()
    assert float(want[0, 1:, 0, 0].sum()) == 0 and float(want[0, 1:, 1, 1].sum()) == 0
    _exact(f"map_features {B}x{rows}x{cols} classes={classes}{' off' if off else ''}", "y",
           y_b[PAD:PAD + n].view(B, 1 + classes, rows, cols), want)


@pytest.mark.parametrize("Lq,E", [(1, 50), (16, 64), (17, 65), (40, 50), (40, 65)])
def test_embed_lengths(Lq, E):
    """k_embed_lengths, a wave per token and 16 waves per sequence: L up to, at and past the 16 waves, E below, at and past
    the 64 lanes.  Tokens -1 and V read row 0; row 3 of the table is all zero (used in mid-sentence: not counted), row 4
    has its only non-zero entry in the last element (counted: the lane that sees it is lane (E-1) % 64 of the last pass)."""
    L = _lib()
    B, V = 3, 20
    g = _gen(Lq, E)
    table = torch.randn(V, E, generator=g)
    table[3] = 0.0
    table[4] = 0.0
    table[4, E - 1] = 0.5
    tok = torch.randint(1, V, (B, Lq), generator=g)
    tok[0, Lq // 2] = 3
    tok[1, 0] = -1
    tok[1, Lq - 1] = V
    tok[2, Lq // 3] = 4
    tok[2, Lq - 1] = 0 if Lq > 1 else 4
    if Lq >= 16:
        tok[0, 1], tok[0, 15], tok[1, 7] = 4, 3, 3
    tok_d, table_d = tok.to(DEV), table.to(DEV)

    def run():
        emb, emb_b = _band(B * Lq * E)
        ln, ln_b = _band(B, torch.int32)
        rc = L.ivln_embed_lengths(tok_d.data_ptr(), table_d.data_ptr(), B, Lq, E, V, emb.data_ptr(), ln.data_ptr(), _sp())
        assert rc == 0, rc
        return emb_b, ln_b

    emb_b, ln_b = _twice(run)
    _band_ok(emb_b, B * Lq * E, "emb")
    _band_ok(ln_b, B, "lengths")
    row = torch.where((tok < 0) | (tok >= V), torch.zeros_like(tok), tok)
    want = table[row.view(-1)]
    want_len = (want.view(B, Lq, E) != 0).any(-1).sum(-1).to(torch.int32)
    case = f"embed_lengths L={Lq} E={E}"
    _exact(case, "emb", emb_b[PAD:PAD + B * Lq * E].view(B * Lq, E), want)
    _exact(case, "lengths", ln_b[PAD:PAD + B], want_len)


# ------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------
def _attn_ref(q, k, v, valid, idx, scale, dt):
    """MapCMANet._attn in dt: rows attend over image idx[r]; positions >= valid[image] get logits - 1e8"""
    k, v = k.to(dt)[idx], v.to(dt)[idx]
    logits = torch.einsum("rc,rci->ri", q.to(dt), k)
    I = k.shape[2]
    masked = torch.arange(I).view(1, -1) >= valid[idx].view(-1, 1)
    logits = torch.where(masked, logits - 1e8, logits)
    attn = torch.softmax(logits * scale, dim=1)
    return torch.einsum("ri,rci->rc", attn, v), attn


def _attn_run(q, k, v, valid, idx, scale, plain_entry=False):
    """ivln_attn_fwd_idx_f32 (or ivln_attn_fwd_f32) with strided q / out and banded save_attn / logits workspace"""
    L = _lib()
    rows, Ck = q.shape
    Cv, I = v.shape[1], v.shape[2]
    q_d = _in_cols(q)
    kv_d = torch.cat((k, v), 1).to(DEV)   # k / v channel slices of one tensor: image strides (Ck + Cv) * I
    k_d, v_d = kv_d[:, :Ck], kv_d[:, Ck:]
    valid_d = None if valid is None else valid.to(torch.int32).to(DEV)
    idx_d = None if plain_entry else idx.to(torch.int32).to(DEV)

    def run():
        out, out_w = _cols(rows, Cv, 4, 3)
        sa, sa_b = _band(rows * I)
        ws, ws_b = _band(rows * I)
        a = (q_d.data_ptr(), q_d.stride(0), k_d.data_ptr(), kv_d.stride(0), v_d.data_ptr(), kv_d.stride(0),
             None if valid_d is None else valid_d.data_ptr(), scale, rows, Ck, Cv, I, out.data_ptr(), out.stride(0), sa.data_ptr(),
             ws.data_ptr())
        rc = L.ivln_attn_fwd_f32(*a, _sp()) if plain_entry else L.ivln_attn_fwd_idx_f32(*a, idx_d.data_ptr(), _sp())
        assert rc == 0, rc
        return out_w, sa_b, ws_b

    out_w, sa_b, ws_b = _twice(run)
    _cols_ok(out_w, 4, Cv, "attention out")
    _band_ok(sa_b, rows * I, "save_attn")
    _band_ok(ws_b, rows * I, "logits workspace")
    return out_w[:, 4:4 + Cv], sa_b[PAD:PAD + rows * I].view(rows, I)


ATTN_CASES = [(5, 3, 5, 1, 1), (5, 3, 57, 15, 33), (4, 3, 64, 17, 49), (5, 3, 65, 15, 65), (4, 2, 121, 17, 512),
              (3, 2, 1024, 1, 33), (5, 3, 64, 15, 512), (4, 3, 121, 1, 49), (5, 3, 5, 17, 65), (4, 3, 57, 17, 1),
              (3, 2, 1024, 15, 65), (5, 3, 65, 1, 512), (4, 3, 56, 16, 48), (4, 3, 120, 16, 64)]


@pytest.mark.parametrize("rows,imgs,Ck,Cv,I", ATTN_CASES)
def test_attn(rows, imgs, Ck, Cv, I):
    """k_attn_logits + k_attn_out through ivln_attn_fwd_idx_f32.  A channel part tp of k_attn_logits takes the 8-deep
    unrolled pass while c + 56 < Ck: Ck = 57 has it for tp = 0 only, 64 for all parts with no tail, 65 a one-element tail
    for tp = 0, 121 two passes for tp = 0 and one + tail for the rest, 5 leaves parts 5..7 idle, 1024 fills the LDS query;
    56 and 120 are one short of a pass.  k_attn_out has the same shape in i + 48 < I over 16 position parts: I = 49, 65
    (first / second pass for part 0 only), 33, 1 and 512 (ATT_MAX_I, two softmax elements per thread), 48 and 64 one short;
    Cv = 1, 15, 17 (16 channels per block: a second block with one live channel).  valid_len per image: I, 1, mid-range;
    row_index permutes and repeats the images over more rows than images; q and out are column slices; save_attn goes
    against the float64 softmax."""
    g = _gen(rows, imgs, Ck, Cv, I)
    scale = Ck ** -0.5
    q = torch.randn(rows, Ck, generator=g)
    k = torch.randn(imgs, Ck, I, generator=g)
    v = torch.randn(imgs, Cv, I, generator=g)
    valid = torch.tensor([I, 1, max(1, I // 2)])[:imgs]
    idx = torch.tensor([imgs - 1, 0, 1, 0, imgs - 1])[:rows]
    assert rows > imgs and len(set(idx.tolist())) == imgs
    out, attn = _attn_run(q, k, v, valid, idx, scale)
    r64, r32 = _attn_ref(q, k, v, valid, idx, scale, torch.float64), _attn_ref(q, k, v, valid, idx, scale, torch.float32)
    bar = _bar(f"attn rows={rows} Ck={Ck} Cv={Cv} I={I}")
    bar.check("out", out, r64[0], r32[0])
    bar.check("save_attn", attn, r64[1], r32[1])
    bar.done()


def test_attn_plain_entry_unmasked_and_fully_masked_row():
    """ivln_attn_fwd_f32 (no row_index, valid_len NULL) is the same launch.  An image with valid_len = 0: every logit is
    s - 1e8, which fp32 quantises to multiples of 8, so float64 cannot be the bar; the row is checked for finite output and
    for save_attn summing to 1 within the bar of the fp32 formula's own sum."""
    rows, Ck, Cv, I = 3, 65, 17, 33
    g = _gen(rows, Ck, Cv, I, 1)
    scale = Ck ** -0.5
    q, k, v = torch.randn(rows, Ck, generator=g), torch.randn(rows, Ck, I, generator=g), torch.randn(rows, Cv, I, generator=g)
    idx = torch.arange(rows)
    full = torch.full((rows,), I)
    out, attn = _attn_run(q, k, v, None, idx, scale, plain_entry=True)
    r64, r32 = _attn_ref(q, k, v, full, idx, scale, torch.float64), _attn_ref(q, k, v, full, idx, scale, torch.float32)
    bar = _bar("attn plain entry, no mask")
    bar.check("out", out, r64[0], r32[0])
    bar.check("save_attn", attn, r64[1], r32[1])
    out2, attn2 = _attn_run(q, k, v, full, idx, scale)
    assert _same_bytes(out2.contiguous(), out.contiguous()) and _same_bytes(attn2, attn), "valid_len = I is no mask"
    valid = torch.tensor([I, 0, 5])
    out, attn = _attn_run(q, k, v, valid, idx, scale)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(attn).all())
    r64, r32 = _attn_ref(q, k, v, valid, idx, scale, torch.float64), _attn_ref(q, k, v, valid, idx, scale, torch.float32)
    live = torch.tensor([0, 2])
    bar.case = "attn valid_len = (I, 0, 5)"
    bar.check("out", out.cpu()[live], r64[0][live], r32[0][live])
    bar.check("save_attn", attn.cpu()[live], r64[1][live], r32[1][live])
    bar.check("sum(attn)", attn.cpu().double().sum(1), torch.ones(rows, dtype=torch.float64), r32[1].double().sum(1))
    bar.done()


def test_attn_refusals():
    """I > 512 (ATT_MAX_I) and Ck > 1024 (the LDS query) are refused."""
    from ivln_ce_amd import ops

    z = lambda *s: torch.zeros(*s, device=DEV)
    _refused(E_UNSUPPORTED, ops.attn, z(1, 8), z(1, 8, 513), z(1, 4, 513), None, 1.0, z(1, 4))
    _refused(E_UNSUPPORTED, ops.attn, z(1, 1025), z(1, 1025, 4), z(1, 4, 4), None, 1.0, z(1, 4))


def _small_ref(q, k, v, scale, dt):
    attn = torch.softmax(torch.einsum("rc,rci->ri", q[:, :k.shape[1]].to(dt), k.to(dt)) * scale, dim=1)
    return torch.einsum("ri,rci->rc", attn, v.to(dt))


@pytest.mark.parametrize("order", ["narrow second", "narrow first", "one set"])
@pytest.mark.parametrize("I", [1, 16, 31, 32])
def test_attn_small2(I, order):
    """k_attn_small: two key / value sets sharing the query in one launch, (Ck, Cv) = (72, 40) and (200, 17) in either order -
    the grid has ceil(40 / 16) = 3 channel blocks per set and the third block of the 17-wide set leaves at once -, and one
    set alone (k1 = NULL).  I = 1, 16, 31 and 32 positions (half a wave: lanes >= I carry -inf into the wave maximum).  I =
    33 is refused."""
    L = _lib()
    rows = 3
    dims = {"narrow second": [(72, 40), (200, 17)], "narrow first": [(200, 17), (72, 40)], "one set": [(72, 40)]}[order]
    g = _gen(I, len(order))
    scale = 0.11
    q = torch.randn(rows, 200, generator=g)
    ks = [torch.randn(rows, ck, I, generator=g) for ck, _ in dims]
    vs = [torch.randn(rows, cv, I, generator=g) for _, cv in dims]
    q_d = _in_cols(q)
    kv_d = [torch.cat((k_, v_), 1).to(DEV) for k_, v_ in zip(ks, vs)]

    def args(j, out):
        if j >= len(dims):
            return (None, 0, None, 0, 0, 0, None, 0)
        ck, cv = dims[j]
        return (kv_d[j][:, :ck].data_ptr(), kv_d[j].stride(0), kv_d[j][:, ck:].data_ptr(), kv_d[j].stride(0), ck, cv,
                out.data_ptr(), out.stride(0))

    def run():
        outs = [_cols(rows, cv, 4, 5) for _, cv in dims]
        rc = L.ivln_attn_small2_f32(q_d.data_ptr(), q_d.stride(0), scale, rows, I, *args(0, outs[0][0]),
                                    *args(1, outs[1][0] if len(dims) > 1 else None), _sp())
        assert rc == 0, rc
        return tuple(o[1] for o in outs)

    wides = _twice(run)
    bar = _bar(f"attn_small2 I={I} {order}")
    for j, (w, (ck, cv)) in enumerate(zip(wides, dims)):
        _cols_ok(w, 4, cv, f"attn_small2 out{j}")
        bar.check(f"out{j}", w[:, 4:4 + cv], _small_ref(q, ks[j], vs[j], scale, torch.float64),
                  _small_ref(q, ks[j], vs[j], scale, torch.float32))
    bar.done()
    out = torch.zeros(rows, 64, device=DEV)
    a0 = (kv_d[0].data_ptr(), kv_d[0].stride(0), kv_d[0].data_ptr(), kv_d[0].stride(0), 8, 8, out.data_ptr(), 64)
    assert L.ivln_attn_small2_f32(q_d.data_ptr(), q_d.stride(0), scale, rows, 33, *a0, None, 0, None, 0, 0, 0, None, 0,
                                  _sp()) == E_UNSUPPORTED


# ------------------------------------------------------------------------------------------------------------------
# skinny linear, GRU step
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,K,O,relu", [(1, 4, 1, False), (8, 50, 5, True), (9, 1020, 5, False), (16, 1024, 1, True),
                                           (9, 1028, 5, True), (16, 50, 1, False), (1, 1024, 5, False), (8, 1028, 1, False)])
def test_linear_skinny(rows, K, O, relu):
    """k_linear_skinny: rows 8 at a time (1, 8, 9 = a second pass of one row, 16), K on the float4 path (4: one thread;
    1020 / 1024 / 1028: the last thread of the first 1024-wide pass idle / busy / one thread in a second pass) and on the
    scalar path (50), one output block and five; x and y are column slices."""
    from ivln_ce_amd import ops

    g = _gen(rows, K, O)
    x, w, b = torch.randn(rows, K, generator=g), torch.randn(O, K, generator=g) * K ** -0.5, torch.randn(O, generator=g)
    x_d, w_d, b_d = _in_cols(x), w.to(DEV), b.to(DEV)
    assert x_d.stride(0) % 4 == 0 or K % 4

    def run():
        y, y_w = _cols(rows, O, 3, 2)
        ops.linear(x_d, w_d, b_d, relu, out=y)
        return (y_w,)

    (y_w,) = _twice(run)
    _cols_ok(y_w, 3, O, "linear_skinny y")
    ref = lambda dt: (F.relu if relu else (lambda t: t))(F.linear(x.to(dt), w.to(dt), b.to(dt)))
    bar = _bar(f"linear_skinny rows={rows} K={K} O={O}")
    bar.check("y", y_w[:, 3:3 + O], ref(torch.float64), ref(torch.float32))
    if K % 4 == 0:
        # x one float into its row (row stride still a multiple of 4) and W one float into a buffer: the launcher takes the
        # scalar loop instead of 16-byte loads from 4-byte boundaries
        wide = torch.zeros(rows, K + 8, device=DEV)
        wide[:, 1:1 + K] = x.to(DEV)
        assert wide[:, 1:1 + K].data_ptr() % 16 == 4 and wide.stride(0) % 4 == 0
        y1, y2 = torch.empty(rows, O, device=DEV), torch.empty(rows, O, device=DEV)
        ops.linear(wide[:, 1:1 + K], w_d, b_d, relu, out=y1)
        ops.linear(x_d, _off_by_one(w), b_d, relu, out=y2)
        bar.check("y(x off)", y1, ref(torch.float64), ref(torch.float32))
        bar.check("y(W off)", y2, ref(torch.float64), ref(torch.float32))
        assert _same_bytes(y1, y2), "the scalar loop does not depend on which operand was off the boundary"
    bar.done()


def test_linear_skinny_refuses_a_row_stride_off_the_vector_path():
    from ivln_ce_amd import ops

    x = torch.zeros(2, 13, device=DEV)[:, :8]   # K % 4 == 0, ldx = 13
    _refused(E_INVALID, ops.linear, x, torch.zeros(3, 8, device=DEV))


def _gru_ref(x, gi_pre, h_in, mask, w_ih, w_hh, b_ih, b_hh, dt):
    H = w_hh.shape[1]
    h = h_in.to(dt) * (mask.to(dt).view(-1, 1) if mask is not None else 1.0)
    gi = F.linear(x.to(dt), w_ih.to(dt), b_ih.to(dt)) if x is not None else gi_pre.to(dt)
    gh = F.linear(h, w_hh.to(dt), b_hh.to(dt))
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return (1 - z) * n + z * h, r, z, n, gh[:, 2 * H:]


@pytest.mark.parametrize("rows", [4, 5, 9, 33])
@pytest.mark.parametrize("H,I", [(8, 4), (64, 36)])
def test_gru_step(H, I, rows):
    """k_rnn_step<GruCell>: 64 lanes per row up to 4 rows, 32 from 5 (8 rows per pass: 9 and 33 need a second / fifth pass with one live
    row).  H = 8, I = 4: two / one lanes of a row carry data; H = 64, I = 36: I is no multiple of the 32-lane stride.  Mask
    given or NULL, the x path and the gi_pre path; h_in, h_out and h_out2 are column slices; the four saves go against
    float64."""
    from ivln_ce_amd import ops

    g = _gen(H, I, rows)
    x, h_in = torch.randn(rows, I, generator=g), torch.randn(rows, H, generator=g)
    w_ih, w_hh = torch.randn(3 * H, I, generator=g) * I ** -0.5, torch.randn(3 * H, H, generator=g) * H ** -0.5
    b_ih, b_hh = torch.randn(3 * H, generator=g) * 0.1, torch.randn(3 * H, generator=g) * 0.1
    mask = (torch.rand(rows, generator=g) < 0.6).to(torch.uint8)
    mask[0], mask[-1] = 0, 1
    gi_pre = F.linear(x, w_ih, b_ih)
    x_d, h_d, gi_d, m_d = _in_cols(x), _in_cols(h_in, 4, 8), _in_cols(gi_pre), mask.to(DEV)
    wd = [t.to(DEV) for t in (w_ih, w_hh, b_ih, b_hh)]
    for use_x in (True, False):
        for use_mask in (True, False):
            def run():
                o1, o1_w = _cols(rows, H, 4, 4)
                o2, o2_w = _cols(rows, H, 8, 4)
                sv = [_band(rows * H) for _ in range(4)]
                ops.gru_step(x_d if use_x else None, None if use_x else gi_d, h_d, m_d if use_mask else None, *wd, o1, o2,
                             saves=tuple(s[0].view(rows, H) for s in sv))
                return (o1_w, o2_w) + tuple(s[1] for s in sv)

            got = _twice(run)
            _cols_ok(got[0], 4, H, "gru h_out")
            _cols_ok(got[1], 8, H, "gru h_out2")
            a = (x if use_x else None, None if use_x else gi_pre, h_in, mask if use_mask else None, w_ih, w_hh, b_ih, b_hh)
            r64, r32 = _gru_ref(*a, torch.float64), _gru_ref(*a, torch.float32)
            bar = _bar(f"gru_step H={H} I={I} rows={rows} {'x' if use_x else 'gi_pre'} {'mask' if use_mask else 'nomask'}")
            bar.check("h_out", got[0][:, 4:4 + H], r64[0], r32[0])
            assert _same_bytes(got[0][:, 4:4 + H].contiguous(), got[1][:, 8:8 + H].contiguous()), "h_out2 != h_out"
            for name, b_, ref64, ref32 in zip(("save_r", "save_z", "save_n", "save_ghn"), got[2:], r64[1:], r32[1:]):
                _band_ok(b_, rows * H, name)
                bar.check(name, b_[PAD:PAD + rows * H].view(rows, H), ref64, ref32)
            bar.done()


def test_gru_step_refusals():
    """H % 4 != 0 is refused, and so are operands of the 16-byte loads that do not start on a 16-byte boundary (the kernel has
    no scalar form); nothing is launched."""
    from ivln_ce_amd import ops

    z = lambda *s: torch.zeros(*s, device=DEV)
    _refused(E_INVALID, ops.gru_step, z(2, 4), None, z(2, 6), None, z(18, 4), z(18, 6), z(18), z(18), z(2, 6))
    H, I, rows = 8, 4, 2
    ok = dict(x=z(rows, I), h=z(rows, H), w_ih=z(3 * H, I), w_hh=z(3 * H, H))
    call = lambda **kw: ops.gru_step({**ok, **kw}["x"], None, {**ok, **kw}["h"], None, {**ok, **kw}["w_ih"], {**ok, **kw}["w_hh"],
                                     z(3 * H), z(3 * H), z(rows, H))
    call()
    for name in ok:
        _refused(E_INVALID, call, **{name: _off_by_one(ok[name])})
    # with gi_pre the x-side operands are not read and need no alignment
    ops.gru_step(None, z(rows, 3 * H), ok["h"], None, _off_by_one(ok["w_ih"]), ok["w_hh"], z(3 * H), z(3 * H), z(rows, H))


def test_kv_linear_refuses_operands_off_the_vector_boundary():
    """ivln_kv_linear_f32 stages feat and reads w_lin with 16-byte loads: either one float off a 16-byte boundary is refused
    before the launch (the kernel itself is tested in tests/test_gpu_kernels.py)."""
    L = _lib()
    rows, Cc, P, Ckv, O = 2, 4, 4, 8, 3
    z = lambda *s: torch.zeros(*s, device=DEV)
    feat, wkv, kv, wl, lin = z(rows, Cc, P), z(Ckv, Cc), z(rows, Ckv, P), z(O, Cc * P), z(rows, O)
    call = lambda f, w: L.ivln_kv_linear_f32(f.data_ptr(), rows, Cc, P, wkv.data_ptr(), None, Ckv, kv.data_ptr(), w.data_ptr(),
                                             None, O, 1, lin.data_ptr(), O, _sp())
    assert call(feat, wl) == 0
    assert call(_off_by_one(feat), wl) == E_INVALID
    assert call(feat, _off_by_one(wl)) == E_INVALID


# ------------------------------------------------------------------------------------------------------------------
# previous-action embedding, tour memory, arg-maxes
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acts,masks", [([2], [1]), ([0], [0]), ([0, 3, -1, 9, 2], [1, 1, 1, 1, 0]), ([1, 2, 9, -1, 3], [0, 1, 0, 1, 1])])
def test_prev_action_embed(acts, masks):
    """k_prev_action_embed: row ((a + 1) * mask) of the table, clamped to [0, n_emb - 1] (a = 9 with the mask set reads the last
    row, a = -1 and every masked row read row 0), written to both strided destinations."""
    from ivln_ce_amd import ops

    rows, E, n_emb = len(acts), 32, 5
    table = torch.randn(n_emb, E, generator=_gen(rows, acts[0]))
    a, m = torch.tensor(acts, dtype=torch.int64), torch.tensor(masks, dtype=torch.uint8)
    a_d, m_d, t_d = a.to(DEV), m.to(DEV), table.to(DEV)

    def run():
        o1, w1 = _cols(rows, E, 4, 4)
        o2, w2 = _cols(rows, E, 8, 3)
        ops.prev_action_embed(a_d, m_d, t_d, o1, o2)
        return w1, w2

    w1, w2 = _twice(run)
    _cols_ok(w1, 4, E, "out1")
    _cols_ok(w2, 8, E, "out2")
    want = table[((a + 1) * m.long()).clamp(0, n_emb - 1)]
    case = f"prev_action_embed a={acts} m={masks}"
    _exact(case, "out1", w1[:, 4:4 + E], want)
    _exact(case, "out2", w2[:, 8:8 + E], want)


@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("with_h", [True, False], ids=["h", "noh"])
@pytest.mark.parametrize("N,H", [(1, 4), (5, 130), (5, 4), (1, 130)])
def test_tour_memory(N, H, with_h, with_mask):
    """k_tour_memory: mask * max(mem, h) with h and the mask each given or NULL; mem, h, out1 and out2 are column slices of
    wider matrices (N * H = 650 spans three blocks)."""
    from ivln_ce_amd import ops

    g = _gen(N, H)
    mem, h = torch.randn(N, H, generator=g), torch.randn(N, H, generator=g)
    mask = torch.tensor([0, 1, 1, 0, 1][:N] if N > 1 else [1], dtype=torch.uint8)
    mem_d, h_d, mask_d = _in_cols(mem, 3, 2), _in_cols(h, 1, 6), mask.to(DEV)

    def run():
        o1, w1 = _cols(N, H, 4, 1)
        o2, w2 = _cols(N, H, 2, 5)
        ops.tour_memory(mem_d, h_d if with_h else None, mask_d if with_mask else None, o1, o2)
        return w1, w2

    w1, w2 = _twice(run)
    _cols_ok(w1, 4, H, "out1")
    _cols_ok(w2, 2, H, "out2")
    want = torch.maximum(mem, h) if with_h else mem.clone()
    if with_mask:
        want = torch.where(mask.bool().view(-1, 1), want, torch.zeros(()))
    case = f"tour_memory {N}x{H} {'h' if with_h else 'noh'} {'mask' if with_mask else 'nomask'}"
    _exact(case, "out1", w1[:, 4:4 + H], want)
    _exact(case, "out2", w2[:, 2:2 + H], want)
    if N == 1 and with_mask:   # a reset row is zero whatever it held
        ops.tour_memory(mem_d, h_d if with_h else None, torch.zeros(1, dtype=torch.uint8, device=DEV), w1[:, 4:4 + H])
        _exact(case + " reset", "out1", w1[:, 4:4 + H], torch.zeros(N, H))


def _argmax_input(N, Cc, HW, g):
    """(N, C, HW) logits with exact ties, a pixel whose channels are all equal, -inf entries and an all -inf pixel"""
    x = torch.randn(N, Cc, HW, generator=g)
    x[0, :, 0] = 0.25
    if Cc > 2:
        x[1, 1, HW // 2] = x[1, Cc - 1, HW // 2] = 9.0
        x[1, 0, HW - 1] = x[1, Cc // 2, HW - 1] = 7.5
        x[0, 0, HW - 1] = float("-inf")
        x[0, Cc - 1, HW // 3] = float("-inf")
    x[1, :, 0] = float("-inf")
    return x


@pytest.mark.parametrize("HW", [1, 255, 257])
@pytest.mark.parametrize("Cc", [1, 13, 40])
def test_argmax_rows_and_channels(Cc, HW):
    """k_argmax_rows (a thread per row) and k_argmax_channels_u8 (a thread per pixel) on the same values: exact ties and an
    all-equal or all -inf pixel take the first index, like torch.argmax on the same fp32 values; 255 / 257 pixels of 2 images
    end inside the second / third block.  NaN handling is not tested: the kernels' `v > best` never selects a NaN, torch's
    argmax does."""
    from ivln_ce_amd import ops

    N = 2
    x = _argmax_input(N, Cc, HW, _gen(Cc, HW))
    x_d = x.to(DEV)
    rows_d = x.permute(0, 2, 1).reshape(N * HW, Cc).contiguous().to(DEV)
    L = _lib()

    def run():
        lab, lab_b = _band(N * HW, torch.uint8, pad=16)
        rc = L.ivln_argmax_channels_u8(x_d.data_ptr(), N, Cc, HW, lab.data_ptr(), _sp())
        assert rc == 0, rc
        out, out_b = _band(N * HW, torch.int64)
        ops.argmax_rows(rows_d, out=out.view(N * HW, 1))
        return lab_b.to(torch.int32), out_b

    lab_b, out_b = _twice(run)
    _band_ok(lab_b, N * HW, "labels", pad=16)
    _band_ok(out_b, N * HW, "argmax_rows out")
    want = torch.argmax(x, dim=1)
    assert HW == 1 or (int(want[0, 0]) == 0 and int(want[1, 0]) == 0 and (Cc <= 2 or int(want[1, HW // 2]) == 1))
    case = f"argmax C={Cc} HW={HW}"
    _exact(case, "channels", lab_b[16:16 + N * HW].view(N, HW), want.to(torch.int32))
    _exact(case, "rows", out_b[PAD:PAD + N * HW], want.reshape(-1))
    if Cc == 13 and HW == 255:   # the wrapper's (N, 1, H, W) u8 output
        _exact(case, "wrapper", ops.argmax_channels_u8(x_d.view(N, Cc, 15, 17)), want.view(N, 1, 15, 17).to(torch.uint8))


# ------------------------------------------------------------------------------------------------------------------
# image preparation, elementwise, adaptive average pool
# ------------------------------------------------------------------------------------------------------------------
RGB_MEAN = torch.tensor([0.485, 0.456, 0.406])   # fp32, the kernel's constants
RGB_STD = torch.tensor([0.229, 0.224, 0.225])


def test_rgb_to_nchw():
    """k_rgb_to_nchw at an odd size: u8 NHWC -> f32 NCHW / div (one IEEE division per value)."""
    from ivln_ce_amd import ops

    B, H, W = 2, 3, 5
    rgb = torch.randint(0, 256, (B, H, W, 3), generator=_gen(1), dtype=torch.uint8)
    rgb[0, 0, 0] = torch.tensor([0, 255, 1], dtype=torch.uint8)
    rgb_d = rgb.to(DEV)
    bar = _bar("rgb_to_nchw 2x3x5")
    for div in (255.0, 3.0):
        (got,) = _twice(lambda: (ops.rgb_to_nchw(rgb_d, div),))
        ref = lambda dt: rgb.permute(0, 3, 1, 2).to(dt) / torch.tensor(div, dtype=torch.float32).to(dt)
        bar.check(f"/{div:g}", got, ref(torch.float64), ref(torch.float32))
    bar.done()
    L = _lib()
    assert L.ivln_rgb_to_nchw_f32(rgb_d.data_ptr(), B, H, W, 0.0, rgb_d.data_ptr(), _sp()) == E_INVALID


@pytest.mark.parametrize("Hi,Wi,Ho,Wo", [(5, 7, 4, 4), (4, 4, 8, 8), (3, 5, 3, 5)])
def test_rgb_resize_normalize(Hi, Wi, Ho, Wo):
    """k_rgb_resize_normalize: u8 NHWC / 255 -> bilinear resize (align_corners=False; down, up, and the same odd size, which
    the four-pixel kernel does not take) -> (x - mean) / std, against F.interpolate in float64 with the kernel's fp32
    constants."""
    from ivln_ce_amd import ops

    B = 2
    rgb = torch.randint(0, 256, (B, Hi, Wi, 3), generator=_gen(Hi, Wi, Ho), dtype=torch.uint8)
    rgb_d = rgb.to(DEV)
    (got,) = _twice(lambda: (ops.rgb_resize_normalize(rgb_d, Ho, Wo),))

    def ref(dt):
        x = rgb.permute(0, 3, 1, 2).to(dt) / 255.0
        x = F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=False)
        return (x - RGB_MEAN.to(dt).view(1, 3, 1, 1)) / RGB_STD.to(dt).view(1, 3, 1, 1)

    bar = _bar(f"rgb_resize_normalize {Hi}x{Wi}->{Ho}x{Wo}")
    bar.check("y", got, ref(torch.float64), ref(torch.float32))
    bar.done()


@pytest.mark.parametrize("n", [1, 255, 257, 30])
def test_affine_and_add(n):
    """k_affine ((x - sub) / div) against float64; k_add with and without ReLU for equal bytes with the fp32 sum (one correctly
    rounded add); n around the 256-thread block, and 30 = the (2, 3, 5) odd shape."""
    from ivln_ce_amd import ops

    g = _gen(n)
    shape = (2, 3, 5) if n == 30 else (n,)
    a, b = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    a_d, b_d = a.to(DEV), b.to(DEV)
    sub, div = torch.tensor(0.213), torch.tensor(0.285)
    (got,) = _twice(lambda: (ops.affine(a_d, float(sub), float(div)),))
    bar = _bar(f"affine n={n}")
    bar.check("y", got, (a.double() - sub.double()) / div.double(), (a - sub) / div)
    bar.done()
    for relu in (False, True):
        def run():
            y, y_b = _band(n)
            ops.add(a_d, b_d, relu, out=y.view(shape))
            return (y_b,)

        (y_b,) = _twice(run)
        _band_ok(y_b, n, "add output")
        want = F.relu(a + b) if relu else a + b
        assert _same_bytes(y_b[PAD:PAD + n].cpu(), want.reshape(-1)), "add: not the fp32 sum's bytes"
        _exact(f"add n={n} relu={int(relu)}", "y", y_b[PAD:PAD + n], want.reshape(-1))


@pytest.mark.parametrize("broadcast", [False, True], ids=["rows", "broadcast"])
def test_copy2d(broadcast):
    """k_copy2d between column slices at an odd size, and one source row broadcast to every destination row."""
    from ivln_ce_amd import ops

    rows, cols = 3, 5
    src = torch.randn(rows, cols, generator=_gen(3, 5))
    src_d = _in_cols(src, 2, 3)

    def run():
        dst, w = _cols(rows, cols, 3, 4)
        ops.copy2d(src_d[1] if broadcast else src_d, dst, rows, cols, broadcast_rows=broadcast)
        return (w,)

    (w,) = _twice(run)
    _cols_ok(w, 3, cols, "copy2d dst")
    _exact(f"copy2d 3x5 {'broadcast' if broadcast else 'rows'}", "dst", w[:, 3:3 + cols],
           src[1].expand(rows, cols).contiguous() if broadcast else src)


def adaptive_windows(size, out):
    """F.adaptive_avg_pool2d's windows along one axis: [floor(i * size / out), ceil((i + 1) * size / out))"""
    return [((i * size) // out, ((i + 1) * size + out - 1) // out) for i in range(out)]


@pytest.mark.parametrize("H,W", [(8, 8), (7, 5), (3, 3), (1, 1)])
def test_adaptive_avgpool2d(H, W):
    """k_adaptive_avgpool2d to 4 x 4: even windows (8), overlapping windows of unequal size (7, 5), windows that repeat input
    rows (3) and a single pixel; `out` is a channel slice of a wider buffer whose guard channels keep their sentinel."""
    from ivln_ce_amd import ops

    N, Cc, OH, OW = 2, 3, 4, 4
    x = torch.randn(N, Cc, H, W, generator=_gen(H, W))
    x_d = x.to(DEV)

    def run():
        wide = torch.full((N, Cc + 2, OH, OW), SENT, device=DEV)
        ops.adaptive_avgpool2d(x_d, OH, OW, out=wide[:, :Cc], out_ctot=Cc + 2)
        return (wide,)

    (wide,) = _twice(run)
    assert bool((wide[:, Cc:] == SENT).all()), "adaptive_avgpool2d wrote into the guard channels"
    bar = _bar(f"adaptive_avgpool2d {H}x{W}->4x4")
    bar.check("y", wide[:, :Cc], F.adaptive_avg_pool2d(x.double(), (OH, OW)), F.adaptive_avg_pool2d(x, (OH, OW)))
    bar.done()


# ------------------------------------------------------------------------------------------------------------------
# multi-tensor copy / add
# ------------------------------------------------------------------------------------------------------------------
COPY_CHUNK, ADD_CHUNK = 16384, 4096   # bytes / floats per block (csrc/nn_ops.hip)


def block_partition(sizes, chunk):
    """first_block of the launchers: empty jobs are skipped, job j gets ceil(size / chunk) blocks"""
    live = [s for s in sizes if s > 0]
    first = [0]
    for s in live:
        first.append(first[-1] + -(-s // chunk))
    return live, first


@pytest.mark.parametrize("off", [False, True], ids=["aligned", "one byte off"])
def test_copy_multi(off):
    """k_copy_multi: 8 jobs of 1, 15, 16, 17 bytes (scalar tail only / one uint4 / one + tail), 16383, 16384, 16385 (the chunk
    boundary: a second block of one byte) and 3 * 16384 + 5 bytes in one call; the same from u8 views one byte into their
    buffers (the scalar path); a zero-byte job in the middle of a call; 9 pairs through the wrapper (8 + 1); n = 9 through
    the C ABI is refused.  Guard bytes behind every destination."""
    from ivln_ce_amd import ops

    sizes = [1, 15, 16, 17, 16383, 16384, 16385, 3 * 16384 + 5]
    assert block_partition(sizes, COPY_CHUNK)[1] == [0, 1, 2, 3, 4, 5, 6, 8, 12]
    g = _gen(11)
    srcs = [torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8) for n in sizes]
    place = _off_by_one if off else (lambda t: t.to(DEV))
    srcs_d = [place(s) for s in srcs]
    G = 17 if off else 16   # the view starts one byte / sixteen bytes into its guard band

    def fresh(n):
        buf = torch.full((n + G + 16,), SENT_U8, dtype=torch.uint8, device=DEV)
        return buf[G:G + n], buf

    def run():
        dsts = [fresh(n) for n in sizes]
        assert all((d[0].data_ptr() % 16 == 1) == off for d in dsts)
        ops.copy_multi([(s, d[0]) for s, d in zip(srcs_d, dsts)])
        return tuple(d[1].to(torch.int32) for d in dsts)

    bufs = _twice(run)
    case = f"copy_multi 8 jobs{' off' if off else ''}"
    for n, s, b in zip(sizes, srcs, bufs):
        assert bool((b[:G] == SENT_U8).all()) and bool((b[G + n:] == SENT_U8).all()), f"{n} bytes: guard bytes overwritten"
        _exact(case, f"{n}B", b[G:G + n], s.to(torch.int32))
    if off:
        return
    # a zero-byte job in the middle, and 9 pairs through the wrapper
    nine = [100, 0, 50, 16400, 3, 0, 7, 33, 20000]
    assert block_partition(nine[:8], COPY_CHUNK) == ([100, 50, 16400, 3, 7, 33], [0, 1, 2, 4, 5, 6, 7])
    srcs9 = [torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8) for n in nine]
    dsts9 = [fresh(n) for n in nine]
    ops.copy_multi([(s.to(DEV), d[0]) for s, d in zip(srcs9, dsts9)])
    for n, s, (d, b) in zip(nine, srcs9, dsts9):
        assert bool((b[:G] == SENT_U8).all()) and bool((b[G + n:] == SENT_U8).all()), f"{n} bytes: guard bytes overwritten"
        _exact("copy_multi 9 pairs", f"{n}B", d, s)
    L = _lib()
    ptrs, nb = (vp * 9)(*[d[0].data_ptr() or None for d in dsts9]), (i64 * 9)(*nine)
    assert L.ivln_copy_multi(ptrs, ptrs, nb, 9, _sp()) == E_INVALID
    assert L.ivln_copy_multi(ptrs, ptrs, nb, 0, _sp()) == 0


@pytest.mark.parametrize("off", [False, True], ids=["aligned", "one float off"])
def test_add_multi(off):
    """k_add_multi: dst += src for counts 1, 3 (scalar tail only), 4, 5 (one float4, + tail), 4095, 4096, 4097 (the chunk
    boundary: a second block of one float) and 2 * 4096 + 3 in one call; the same from float views one float into their
    buffers (the scalar path).  64 jobs in one launch and 65 through the wrapper (64 + 1).  Result bytes equal d + s in
    fp32; 65 jobs through the C ABI are refused."""
    from ivln_ce_amd import ops

    sizes = [1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 3]
    assert block_partition(sizes, ADD_CHUNK)[1] == [0, 1, 2, 3, 4, 5, 6, 8, 11]
    g = _gen(13)

    def case(sizes, name):
        srcs = [torch.randn(n, generator=g) for n in sizes]
        base = [torch.randn(n, generator=g) for n in sizes]
        place = (lambda t: _off_by_one(t) if t.numel() else t.to(DEV)) if off else (lambda t: t.to(DEV))
        srcs_d = [place(s) for s in srcs]
        G = PAD + 1 if off else PAD

        def run():
            dsts = []
            for n, b0 in zip(sizes, base):
                buf = torch.full((n + G + PAD,), SENT, device=DEV)
                buf[G:G + n] = b0.to(DEV)
                assert (buf[G:].data_ptr() % 16 == 4) == off
                dsts.append((buf[G:G + n], buf))
            ops.add_multi([(s, d[0]) for s, d in zip(srcs_d, dsts)])
            return tuple(d[1] for d in dsts)

        bufs = _twice(run)
        for n, s, b0, b in zip(sizes, srcs, base, bufs):
            assert bool((b[:G] == SENT).all()) and bool((b[G + n:] == SENT).all()), f"{n} floats: guard floats overwritten"
            assert _same_bytes(b[G:G + n].cpu(), b0 + s), f"{name} {n} floats: not the bytes of d + s"
        _log(f"{name + (' off' if off else ''):44s} {'d+s':10s} exact  ok", LOG)

    case(sizes, "add_multi 8 jobs")
    case([k % 7 + 1 for k in range(64)], "add_multi 64 jobs")
    case([k % 5 + 1 for k in range(65)] + [0, 9], "add_multi 67 pairs, one empty")
    L = _lib()
    z = torch.zeros(4, device=DEV)
    ptrs, cnt = (vp * 65)(*[z.data_ptr()] * 65), (i64 * 65)(*[1] * 65)
    assert L.ivln_add_multi_f32(ptrs, ptrs, cnt, 65, _sp()) == E_INVALID


# every entry point of the header's "Non-GEMM forward kernels" section -> the test that runs it alone: a test of this file,
# or "file.py::test_name" where another file of the suite already has one (tests/test_forward_kernel_coverage.py)
FWD_COVERED = {
    "ivln_groupnorm_f32": "test_groupnorm",
    "ivln_groupnorm2_f32": "test_groupnorm_over_split_k_slabs",
    "ivln_bn_fold_f32": "test_bn_fold",
    "ivln_bn_train_stats_f32": "test_bn_train_stats",
    "ivln_bn_stats_from_partials_f32": "test_bn_stats_from_partials",
    "ivln_scale_shift_relu_avgpool2_f32": "test_scale_shift_relu_avgpool2_over_slabs",
    "ivln_pool2d_f32": "test_pool2d_subsample",
    "ivln_map_features_f32": "test_map_features",
    "ivln_embed_lengths": "test_embed_lengths",
    "ivln_embed_gates_dirs_f32": "test_gpu_policy.py::test_instruction_front_end_folded_into_a_table_lookup_is_the_same_encoder",
    "ivln_lstm_dirs_fwd_f32": "test_gpu_instruction_options.py::test_lstm_is_the_same_bytes_through_every_launch_form",
    "ivln_gru_dirs_fwd_f32": "test_gpu_instruction_options.py::test_forward_matches_the_packed_torch_module",
    "ivln_gru_dirs_bwd_f32": "test_gpu_instruction_options.py::test_bptt_matches_float64_autograd",
    "ivln_kv_linear_f32": "test_gpu_kernels.py::test_kv_projection_and_flatten_linear_in_one_launch",
    "ivln_linear_skinny_f32": "test_linear_skinny",
    "ivln_gru_step_f32": "test_gru_step",
    "ivln_cma_seq_fwd_f32": "test_gpu_kernels.py::test_persistent_sequence_gru_matches_per_step_launches_and_torch",
    "ivln_cma_seq_persistent_ok": "test_gpu_kernels.py::test_persistent_sequence_gru_matches_per_step_launches_and_torch",
    "ivln_seq_sync_init": "test_gpu_kernels.py::test_persistent_sequence_gru_matches_per_step_launches_and_torch",
    "ivln_seq_sync_status": "test_gpu_kernels.py::test_persistent_sequence_gru_matches_per_step_launches_and_torch",
    "ivln_attn_fwd_f32": "test_attn_plain_entry_unmasked_and_fully_masked_row",
    "ivln_attn_fwd_idx_f32": "test_attn",
    "ivln_attn_small2_f32": "test_attn_small2",
    "ivln_prev_action_embed_f32": "test_prev_action_embed",
    "ivln_linear_argmax_f32": "test_gpu_kernels.py::test_action_head_linear_argmax_one_launch",
    "ivln_linear_sample_f32": "test_gpu_kernels.py::test_sampled_action_head_inverse_cdf_mixing_and_skip_rule",
    "ivln_tour_memory_f32": "test_tour_memory",
    "ivln_rgb_to_nchw_f32": "test_rgb_to_nchw",
    "ivln_adaptive_avgpool2d_f32": "test_adaptive_avgpool2d",
    "ivln_argmax_rows": "test_argmax_rows_and_channels",
    "ivln_argmax_channels_u8": "test_argmax_rows_and_channels",
    "ivln_rgb_resize_normalize_f32": "test_rgb_resize_normalize",
    "ivln_affine_f32": "test_affine_and_add",
    "ivln_add_f32": "test_affine_and_add",
    "ivln_copy_multi": "test_copy_multi",
    "ivln_add_multi_f32": "test_add_multi",
    "ivln_colsum_multi_f32": "test_gpu_kernels.py::test_colsum_queue_equals_per_matrix_colsums_bit_for_bit",
    "ivln_copy2d_f32": "test_copy2d",
    "ivln_rednet_fwd": "test_gpu_rednet.py::test_rednet_forward_as_one_c_call_equals_the_layer_walk",
}
