"""CPU: every entry point of include/ivln_hip.h's backward / loss / optimizer section has a per-kernel GPU test of its own
(tests/test_gpu_train_kernels.py::COVERED), and the index arithmetic of the BatchNorm -> ReLU -> AvgPool2d(2) backward
restated in numpy, with and without the odd-size guard, against float64 autograd."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _backward_section_functions():
    src = open(os.path.join(ROOT, "include", "ivln_hip.h")).read()
    start = src.index("Backward / loss / optimizer kernels of the DAgger update")
    end = src.index("ivln_dtw_symmetric1(")
    assert 0 < start < end
    sec = re.sub(r"/\*.*?\*/", "", src[src.rindex("/*", 0, start):end], flags=re.S)
    return sorted(set(re.findall(r"\b(ivln_[a-z0-9_]+)\s*\(", sec)))


def _uncovered(names, covered, module):
    no_entry = [n for n in names if n not in covered]
    no_test = [f"{n} -> {t}" for n, t in covered.items() if not callable(getattr(module, t, None)) or not t.startswith("test_")]
    return no_entry, no_test


def test_every_backward_entry_point_has_a_kernel_test():
    import test_gpu_train_kernels as K

    names = _backward_section_functions()
    assert len(names) >= 24 and "ivln_cbra_bwd_f32" in names and "ivln_adam_step_guarded_f32" in names
    assert "ivln_dtw_symmetric1" not in names and "ivln_cma_step_fwd" not in names
    no_entry, no_test = _uncovered(names, K.COVERED, K)
    assert not no_entry, f"declared in the header's backward section without a test in COVERED: {no_entry}"
    assert not no_test, f"COVERED names tests that test_gpu_train_kernels.py does not define: {no_test}"
    stale = [n for n in K.COVERED if n not in names]
    assert not stale, f"COVERED lists functions the header's backward section does not declare: {stale}"
    # the pin itself: one entry less, or a test that does not exist, is noticed
    short = dict(K.COVERED)
    short.pop("ivln_index_sum_f32")
    assert _uncovered(names, short, K)[0] == ["ivln_index_sum_f32"]
    assert _uncovered(names, dict(K.COVERED, ivln_add2d_f32="test_that_is_not_there"), K)[1]
    # and the module's tests carry the gpu marker as a whole
    assert K.pytestmark.name == "gpu"


def _cbra_bwd_numpy(dout, y, gamma, beta, guard):
    """train-mode ivln_cbra_bwd_f32 in float64 numpy with the kernel's index arithmetic: the pooled gradient of pixel (h, w)
    is dout[(h >> 1) * Wo + (w >> 1)] of its plane; `guard` = pixels with h >= 2*Ho or w >= 2*Wo get dz = 0 instead.
    Without it the flat index runs into the next pooled row, the next plane, or past the end (read as 0 here)."""
    N, C, H, W = y.shape
    Ho, Wo = H // 2, W // 2
    mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3))
    rstd = 1.0 / np.sqrt(var + 1e-5)
    xhat = (y - mean[None, :, None, None]) * rstd[None, :, None, None]
    z = xhat * gamma[None, :, None, None] + beta[None, :, None, None]
    flat = np.concatenate((dout.reshape(-1), np.zeros(Wo + 2)))
    h, w = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dz = np.zeros_like(y)
    for n in range(N):
        for c in range(C):
            g = flat[(n * C + c) * Ho * Wo + (h >> 1) * Wo + (w >> 1)]
            if guard:
                g = np.where((h < 2 * Ho) & (w < 2 * Wo), g, 0.0)
            dz[n, c] = np.where(z[n, c] > 0, 0.25 * g, 0.0)
    M = N * H * W
    s1, s2 = dz.sum((0, 2, 3)), (dz * xhat).sum((0, 2, 3))
    dy = (gamma * rstd)[None, :, None, None] * (dz - s1[None, :, None, None] / M - xhat * s2[None, :, None, None] / M)
    return dy, s2, s1


@pytest.mark.parametrize("shape,odd", [((2, 3, 8, 8), False), ((2, 3, 6, 10), False), ((2, 3, 7, 8), True), ((2, 3, 8, 7), True),
                                       ((2, 3, 25, 25), True)])
def test_cbra_bwd_index_arithmetic_needs_the_odd_size_guard(shape, odd):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(H * 100 + W)
    y = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(C, generator=g, dtype=torch.float64) * 0.3
    dout = torch.randn(N, C, H // 2, W // 2, generator=g, dtype=torch.float64)
    yl, gl, bl = (t.clone().requires_grad_(True) for t in (y, gamma, beta))
    F.avg_pool2d(F.relu(F.batch_norm(yl, None, None, gl, bl, training=True, eps=1e-5)), 2).backward(dout)
    want = (yl.grad.numpy(), gl.grad.numpy(), bl.grad.numpy())
    fixed = _cbra_bwd_numpy(dout.numpy(), y.numpy(), gamma.numpy(), beta.numpy(), guard=True)
    old = _cbra_bwd_numpy(dout.numpy(), y.numpy(), gamma.numpy(), beta.numpy(), guard=False)
    for a, b in zip(fixed, want):
        assert np.abs(a - b).max() < 1e-12
    old_err = max(np.abs(a - b).max() for a, b in zip(old, want))
    assert (old_err > 1e-3) if odd else (old_err < 1e-12), old_err


def _gemm_gradient_wrappers():
    """top-level functions of ivln-ce_amd/ops.py from the "GEMM-shaped gradients" banner to the end of the file"""
    src = open(os.path.join(ROOT, "ivln-ce_amd", "ops.py")).read()
    return re.findall(r"^def ([A-Za-z0-9_]+)\(", src[src.index("# ---- GEMM-shaped gradients"):], flags=re.M)


def test_every_gemm_shaped_gradient_has_a_test():
    import test_gpu_train_gemms as G

    names = _gemm_gradient_wrappers()
    assert names == ["linear_bwd_input", "linear_bwd_weight", "conv2d_bwd_weight"]
    names.append("conv2d_bwd_input(composed)")  # no wrapper of its own: ops.conv2d over ops.weight_flip_transpose (train.py)
    no_entry, no_test = _uncovered(names, G.GEMM_COVERED, G)
    assert not no_entry, f"under the GEMM-shaped gradients banner without a test in GEMM_COVERED: {no_entry}"
    assert not no_test, f"GEMM_COVERED names tests that test_gpu_train_gemms.py does not define: {no_test}"
    stale = [n for n in G.GEMM_COVERED if n not in names]
    assert not stale, f"GEMM_COVERED lists wrappers that ops.py does not define there: {stale}"
    # the pin itself: one entry less, or a test that does not exist, is noticed
    short = dict(G.GEMM_COVERED)
    short.pop("conv2d_bwd_weight")
    assert _uncovered(names, short, G)[0] == ["conv2d_bwd_weight"]
    assert _uncovered(names, dict(G.GEMM_COVERED, linear_bwd_input="test_that_is_not_there"), G)[1]
    assert G.pytestmark.name == "gpu"


def test_gradient_wrappers_build_the_same_descriptor_by_default(monkeypatch):
    """The `splits` / `info` arguments of the three wrappers change nothing unless given: with the library call stubbed out,
    the descriptor each wrapper hands over is, byte for byte, the one written out here field by field (the wrappers' contract
    with ivln_gemm_f32 before those arguments existed); `splits` changes the one field and `info` attaches the counter."""
    import ctypes as C

    from ivln_ce_amd import ops

    ws = torch.empty(64)
    seen, handed = [], []
    monkeypatch.setattr(ops, "dptr", lambda t: handed.append(t) or t.data_ptr())
    monkeypatch.setattr(ops, "_p", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(ops, "splitk_ws", lambda device, floats=0, slot=0: ws)
    monkeypatch.setattr(ops, "gemm", lambda d: seen.append((bytes(d), bool(d.splits_used))))
    monkeypatch.setattr(ops, "TILE_OVERRIDE", 0)
    monkeypatch.setattr(ops, "LINEAR_BWD_SPLIT", True)

    def plain(A, B, D, M, N, K, amode, bmode, lda=0, ldb=0, sDm=0, sDn=0, accumulate=0, **more):
        d = ops.GemmDesc()
        d.A, d.B, d.D, d.M, d.N, d.K = A.data_ptr(), B.data_ptr(), D.data_ptr(), M, N, K
        d.amode, d.bmode, d.dmode, d.lda, d.ldb, d.sDm, d.sDn, d.HoWo = amode, bmode, ops.D_DENSE, lda, ldb, sDm, sDn, 1
        d.accumulate, d.ws, d.ws_floats, d.splits = accumulate, ws.data_ptr(), ws.numel(), 0
        for k, v in more.items():
            setattr(d, k, v)
        return d

    rows, O, I = 6, 8, 12
    wide = torch.zeros(rows, O + 4)
    dy, w, x = wide[:, 1:1 + O], torch.zeros(O, I), torch.zeros(rows, I)   # (dy: a column slice, row stride O + 4)
    dx, dw = torch.zeros(rows, I + 3)[:, :I], torch.zeros(O, I)
    ops.linear_bwd_input(dy, w, out=dx, accumulate=True)
    assert seen.pop() == (bytes(plain(w, dy, dx, I, rows, O, ops.A_KM, ops.B_NK, I, O + 4, 1, I + 3, 1)), False)
    ops.linear_bwd_weight(dy, x, out=dw)
    assert seen.pop() == (bytes(plain(dy, x, dw, O, I, rows, ops.A_KM, ops.B_KN, O + 4, I, I, 1)), False)
    N, Cin, H, W, Cout, k = 2, 3, 5, 6, 4, 3
    xc, dyc = torch.zeros(N, Cin, H, W), torch.zeros(N, Cout, H, W)
    del handed[:]
    out = ops.conv2d_bwd_weight(dyc, xc, k, k, 1, 1)
    assert tuple(out.shape) == (Cout, Cin, k, k) and any(t is out for t in handed)
    koff, kpos = ops.conv_tables(Cin, k, k, H, W, 1, xc.device)
    want = plain(dyc, xc, out, Cout, Cin * k * k, N * H * W, ops.A_NCHW_P, ops.B_IM2COL_T, sDm=Cin * k * k, sDn=1, Cin=Cin, Hin=H,
                 Win=W, Hout=H, Wout=W, stride=1, pad=1, dil=1, koff=koff.data_ptr(), kpos=kpos.data_ptr(),
                 split_ok=int(ops.SPLIT_BF16 and ops.SPLIT_BF16_WGRAD))
    want.HoWo = H * W
    assert seen.pop() == (bytes(want), False)
    # given: `splits` is the one field that changes, `info` attaches the host counter and reads it back
    info = {}
    ops.linear_bwd_weight(dy, x, out=dw, splits=3, info=info)
    forced = plain(dy, x, dw, O, I, rows, ops.A_KM, ops.B_KN, O + 4, I, I, 1)
    forced.splits = 3
    got, counted = seen.pop()
    off, size = ops.GemmDesc.splits_used.offset, C.sizeof(C.c_void_p)
    assert counted and info == {"splits_used": 0}
    assert got[:off] == bytes(forced)[:off] and got[off + size:] == bytes(forced)[off + size:]
