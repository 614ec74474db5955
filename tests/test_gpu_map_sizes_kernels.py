"""Kernels behind egocentric maps other than 64 x 64 cells, each alone:

* ivln_attn_pair_f32 (include/ivln_map_sizes.h, csrc/nn_ops.hip k_attn_pair) through the C ABI against float64, with the bar
  of tests/kernel_bar.py (4 * e32 + 4 * 2^-24 * max|float64|, no tuned constant) and two runs giving the same bytes;
* the map CNN's block (ops.conv7_bn_relu_pool: k_conv7_pool_bf3, u8 first layer included) at the planes of a 32 x 48 and a
  96 x 112 map, and the two-launch path it falls back to at 24 x 28 and 12 x 14 (no multiple of its 4 x 8 tile);
* the training forward with conv-epilogue BatchNorm partials and ivln_cbra_bwd_f32 at a non-square plane.

Every comparison goes to map_sizes_kernels.log in the suite's log directory before anything is asserted."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from kernel_bar import _Bar, _log, _same_bytes, _twice

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOG = "map_sizes_kernels.log"
E_UNSUPPORTED = -5


def _gen(*seed):
    s = 0
    for k in seed:
        s = s * 1009 + int(k)
    return torch.Generator().manual_seed(s % (2 ** 31))


def _lib():
    from ivln_ce_amd import ops

    L = ops._L()
    L.ivln_attn_pair_f32.argtypes = ops.ATTN_PAIR_ARGTYPES
    return L, ops.stream_ptr()


def _ref(q, k, v, scale, dt):
    attn = torch.softmax(torch.einsum("rc,rci->ri", q[:, :k.shape[1]].to(dt), k.to(dt)) * scale, dim=1)
    return torch.einsum("ri,rci->rc", attn, v.to(dt))


def _nan_cols(rows, cols, left=4, right=5):
    wide = torch.full((rows, left + cols + right), float("nan"), device=DEV)
    return wide[:, left:left + cols], wide


def _set_args(kv, ck, cv, out):
    """one set's arguments: k, k_img_stride, v, v_img_stride, Ck, Cv, I, out, ldo"""
    if kv is None:
        return (None, 0, None, 0, 0, 0, 0, None, 0)
    return (kv[:, :ck].data_ptr(), kv.stride(0), kv[:, ck:].data_ptr(), kv.stride(0), ck, cv, kv.shape[2], out.data_ptr(),
            out.stride(0))


PAIRS = [(16, 1), (16, 6), (32, 33), (16, 42), (64, 255), (256, 256)]


@pytest.mark.parametrize("rows", [1, 8])
@pytest.mark.parametrize("order", ["narrow second", "narrow first", "one set"])
@pytest.mark.parametrize("I0,I1", PAIRS)
def test_attn_pair(I0, I1, order, rows):
    """Two key / value sets with a key count each sharing the query, (Ck, Cv) = (72, 40) and (200, 17) in either order, and one
    set alone (k1 = NULL: the second count is then the only one, so every count of the list runs alone too).  q is a column
    slice; the outputs are column slices of NaN-filled wider rows whose other columns must stay NaN."""
    L, sp = _lib()
    dims = {"narrow second": [(72, 40), (200, 17)], "narrow first": [(200, 17), (72, 40)], "one set": [(72, 40)]}[order]
    counts = [I0, I1] if len(dims) == 2 else [I1]
    g = _gen(I0, I1, len(order), rows)
    scale = 0.11
    q = torch.randn(rows, 200, generator=g)
    ks = [torch.randn(rows, ck, i, generator=g) for (ck, _), i in zip(dims, counts)]
    vs = [torch.randn(rows, cv, i, generator=g) for (_, cv), i in zip(dims, counts)]
    q_w = torch.full((rows, 4 + 200 + 4), float("nan"), device=DEV)
    q_d = q_w[:, 4:204]
    q_d.copy_(q)
    kv_d = [torch.cat((k_, v_), 1).to(DEV) for k_, v_ in zip(ks, vs)]

    def run():
        outs = [_nan_cols(rows, cv) for _, cv in dims]
        a1 = _set_args(kv_d[1], *dims[1], outs[1][0]) if len(dims) == 2 else _set_args(None, 0, 0, None)
        rc = L.ivln_attn_pair_f32(q_d.data_ptr(), q_d.stride(0), scale, rows, *_set_args(kv_d[0], *dims[0], outs[0][0]), *a1, sp)
        assert rc == 0, rc
        return tuple(o[1] for o in outs)

    wides = _twice(run)
    bar = _Bar(f"attn_pair I=({I0},{I1}) {order} rows={rows}", LOG)
    for j, (w, (ck, cv)) in enumerate(zip(wides, dims)):
        assert bool(torch.isnan(w[:, :4]).all()) and bool(torch.isnan(w[:, 4 + cv:]).all()), f"out{j}: written outside its columns"
        bar.check(f"out{j}", w[:, 4:4 + cv], _ref(q, ks[j], vs[j], scale, torch.float64), _ref(q, ks[j], vs[j], scale, torch.float32))
    bar.done()


def test_attn_pair_refusals():
    """a key count of 257 or 0, Ck = 1025 and rows = 0 are refused with IVLN_E_UNSUPPORTED before a launch, in either set"""
    L, sp = _lib()
    z = lambda *s: torch.zeros(*s, device=DEV)
    q, out = z(2, 1025), z(2, 8)
    ok = _set_args(z(2, 16, 4), 8, 8, out)
    for bad in (_set_args(z(2, 16, 257), 8, 8, out), _set_args(z(2, 1025 + 8, 4), 1025, 8, out)):
        assert L.ivln_attn_pair_f32(q.data_ptr(), 1025, 1.0, 2, *bad, *_set_args(None, 0, 0, None), sp) == E_UNSUPPORTED
        assert L.ivln_attn_pair_f32(q.data_ptr(), 1025, 1.0, 2, *ok, *bad, sp) == E_UNSUPPORTED
    zero_i = ok[:6] + (0,) + ok[7:]
    assert L.ivln_attn_pair_f32(q.data_ptr(), 1025, 1.0, 2, *zero_i, *_set_args(None, 0, 0, None), sp) == E_UNSUPPORTED
    assert L.ivln_attn_pair_f32(q.data_ptr(), 1025, 1.0, 0, *ok, *_set_args(None, 0, 0, None), sp) == E_UNSUPPORTED
    assert L.ivln_attn_pair_f32(q.data_ptr(), 1025, 1.0, 2, *ok, *ok, sp) == 0
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0  # (zero values: the refused calls wrote nothing, the accepted one wrote zeros)


def test_attn_pair_at_equal_counts_stays_with_attn_small2():
    """(16, 16), the head's shapes: the pair kernel's outputs lie within the float64 bar of attn_small2's"""
    from ivln_ce_amd import ops

    rows, Ck, g = 8, 256, _gen(16, 16)
    q = torch.randn(rows, Ck, generator=g)
    kv = [torch.randn(rows, Ck + cv, 16, generator=g) for cv in (128, 256)]
    q_d, kv_d = q.to(DEV), [t.to(DEV) for t in kv]
    bar = _Bar("attn_pair vs attn_small2 (16,16)", LOG)
    outs = {}
    for name, fn in (("pair", ops.attn_pair), ("small2", ops.attn_small2)):
        o = [torch.empty(rows, 128, device=DEV), torch.empty(rows, 256, device=DEV)]
        fn(q_d, kv_d[0][:, :Ck], kv_d[0][:, Ck:], o[0], kv_d[1][:, :Ck], kv_d[1][:, Ck:], o[1], 0.0625)
        outs[name] = o
    for j in range(2):
        r64 = _ref(q, kv[j][:, :Ck], kv[j][:, Ck:], 0.0625, torch.float64)
        r32 = _ref(q, kv[j][:, :Ck], kv[j][:, Ck:], 0.0625, torch.float32)
        _, b = bar.check(f"pair{j}", outs["pair"][j], r64, r32)
        bar.check(f"small2_{j}", outs["small2"][j], r64, r32)
        bar.within(f"apart{j}", outs["pair"][j], outs["small2"][j], b)
    bar.done()


# ------------------------------------------------------------------------------------------------------------------
# the map CNN's block at other planes
# ------------------------------------------------------------------------------------------------------------------
def _spy(ops, taken):
    orig = ops.gemm_soft

    def spy(desc):
        ok = orig(desc)
        taken.append((int(desc.pool2), ok))
        return ok

    return orig, spy


# (plane, the block of the CNN that meets it first: Cin, Cout, one launch?)
PLANES = [((32, 48), 14, 32, True), ((96, 112), 14, 32, True), ((24, 28), 64, 128, False), ((12, 14), 128, 256, False)]


@pytest.mark.parametrize("src", ["u8", "f32"])
@pytest.mark.parametrize("plane,Cin,Cout,fused", PLANES, ids=[f"{p[0]}x{p[1]}" for p, *_ in PLANES])
def test_map_cnn_block_at_other_planes(plane, Cin, Cout, fused, src):
    """A CBRA block (7x7 conv -> folded BatchNorm -> ReLU -> AvgPool(2)) of 2 images as SemanticMapEncoder.forward issues it,
    against float64.  32 x 48 and 96 x 112 are multiples of the kernel's 4 x 8 pixel tile: one launch; 24 x 28 and 12 x 14 (the
    third and fourth planes of a 96 x 112 map) are not: the library declines (asserted with the gemm_soft spy) and the block
    is conv (raw split-K slabs) + the reducing tail.  u8: the first layer's form - the occupancy and label maps themselves
    on the one-launch path, ops.map_features' tensor on the other (14 input channels at every plane).
    Bars: the one-launch kernel's own (tests/test_gpu_map_cnn_infer.py: 3e-5 on the result of O(1) values); the fp32
    two-launch path the float64 bar of tests/kernel_bar.py.  Two runs give the same bytes."""
    from ivln_ce_amd import ops

    H, W = plane
    N = 2
    if src == "u8":
        Cin, Cout = 14, 32
    g = _gen(H, W, Cin)
    w = torch.randn(Cout, Cin, 7, 7, generator=g) / (Cin * 49) ** 0.5
    sc, sh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    if src == "u8":
        occ = torch.randint(0, 3, (N, H, W), generator=g).to(torch.uint8)
        sem = torch.randint(0, 16, (N, H, W), generator=g).to(torch.uint8)  # (labels 13 ... 15 match no channel)
        x = torch.cat([occ.float().unsqueeze(1), F.one_hot(sem.long(), 16)[..., :13].permute(0, 3, 1, 2).float()], 1)
        maps = (occ.to(DEV), sem.to(DEV))
    else:
        x = torch.randn(N, Cin, H, W, generator=g)
        maps = None

    def ref(dt):
        y = F.conv2d(x.to(dt), w.to(dt), None, padding=3)
        return F.avg_pool2d(F.relu(y * sc.to(dt).view(1, -1, 1, 1) + sh.to(dt).view(1, -1, 1, 1)), 2)

    wd, scd, shd = w.to(DEV), sc.to(DEV), sh.to(DEV)
    taken = []
    orig, spy = _spy(ops, taken)

    def block():
        xd = ops.map_features(*maps) if (maps is not None and not fused) else (None if maps is not None else x.to(DEV))
        y = ops.conv7_bn_relu_pool(xd, wd, scd, shd, maps_u8=maps if fused else None)
        if y is None:
            y = ops.scale_shift_relu_avgpool2(ops.conv2d(xd, wd, pad=3, defer=True), scd, shd)
        return (y,)

    ops.gemm_soft = spy
    try:
        (got,) = _twice(block)
    finally:
        ops.gemm_soft = orig
    pooled = [(p, ok) for p, ok in taken if p]
    if fused:
        assert pooled == [(1, True)] * 2, taken
    else:
        assert pooled == [(1, False)] * 2, taken  # (asked, declined: the two launches followed)
    assert got.shape == (N, Cout, H // 2, W // 2)
    r64, r32 = ref(torch.float64), ref(torch.float32)
    bar = _Bar(f"map cnn block {H}x{W} {src} {'one launch' if fused else 'two launches'}", LOG)
    if fused:
        err = float((got.double().cpu() - r64).abs().max())
        _log(f"{bar.case:44s} out        hip {err:.3e}  max|ref| {float(r64.abs().max()):.3e}  bar atol 3e-5 rtol 1e-4", LOG)
        assert torch.allclose(got.cpu(), r64.float(), atol=3e-5, rtol=1e-4), err
    else:
        bar.check("out", got, r64, r32)
    bar.done()


def test_cbra_train_forward_and_backward_at_a_non_square_plane():
    """CBRA.forward_hip in train mode at 3 x 14 x 32 x 48 (BatchNorm statistics from the conv epilogue's partials) and
    ops.cbra_bwd on what it saved, against float64: the pooled output, the batch mean / rstd, then dy / dgamma / dbeta with the
    saved conv output as the leaf (both sides gate the ReLU on the same y).  No gate may hang on fp32 rounding: an input
    whose pre-activations come within 1e-5 of zero is drawn again."""
    from ivln_ce_amd import encoders, ops

    N, Cin, Cout, H, W = 3, 14, 32, 32, 48
    for attempt in range(8):
        g = _gen(H, W, attempt)
        torch.manual_seed(100 + attempt)
        blk = encoders.CBRA(Cin, Cout)
        bn = blk.conv[1]
        bn.weight.data.uniform_(0.5, 1.5, generator=g)
        bn.bias.data.normal_(0.0, 0.3, generator=g)
        x = torch.randn(N, Cin, H, W, generator=g)
        dout = torch.randn(N, Cout, H // 2, W // 2, generator=g)
        blk_d = encoders.CBRA(Cin, Cout)
        blk_d.load_state_dict(blk.state_dict())
        blk_d = blk_d.to(DEV).train()
        save = []
        with torch.no_grad():
            out = blk_d.forward_hip(x.to(DEV), save)
        s = save[0]
        y_hip = s["y"].cpu()
        y64 = y_hip.double()
        mean, var = y64.mean((0, 2, 3)), y64.var((0, 2, 3), unbiased=False)
        z = (y64 - mean.view(1, -1, 1, 1)) * ((var + bn.eps).rsqrt() * bn.weight.double()).view(1, -1, 1, 1) + bn.bias.double().view(1, -1, 1, 1)
        if float(z.abs().min()) >= 1e-5:
            break
    else:
        raise AssertionError("pre-activations within 1e-5 of zero in every draw")
    assert s["train"] and s["mean"] is not None

    def fwd(dt):
        conv = blk.conv[0]
        y = F.conv2d(x.to(dt), conv.weight.to(dt), conv.bias.to(dt), padding=3)
        m, v = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
        o = F.avg_pool2d(F.relu(F.batch_norm(y, None, None, bn.weight.to(dt), bn.bias.to(dt), training=True, eps=bn.eps)), 2)
        return y, m, (v + bn.eps).rsqrt(), o

    def bwd(dt):
        y = y_hip.to(dt).requires_grad_(True)
        ga, be = bn.weight.detach().to(dt).requires_grad_(True), bn.bias.detach().to(dt).requires_grad_(True)
        F.avg_pool2d(F.relu(F.batch_norm(y, None, None, ga, be, training=True, eps=bn.eps)), 2).backward(dout.to(dt))
        return y.grad, ga.grad, be.grad

    with torch.no_grad():
        f64, f32 = fwd(torch.float64), fwd(torch.float32)
    bar = _Bar(f"cbra train {N}x{Cin}x{H}x{W}", LOG)
    for name, got, a, b in zip(("y", "mean", "rstd", "out"), (s["y"], s["mean"], s["rstd"], out), f64, f32):
        bar.check(name, got, a, b)
    got = _twice(lambda: ops.cbra_bwd(dout.to(DEV), s["y"], s["scale"], s["shift"], s["mean"], s["rstd"], True))
    for name, gv, a, b in zip(("dy", "dgamma", "dbeta"), got, bwd(torch.float64), bwd(torch.float32)):
        bar.check(name, gv, a, b)
    bar.done()
