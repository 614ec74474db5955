"""Per-kernel GPU parity of the update path's backward / loss / optimizer kernels (csrc/train_ops.hip, the 24 entry points
of include/ivln_hip.h's "Backward / loss / optimizer" section), each alone, against the same operation written in plain
torch in float64 on the CPU and differentiated by autograd.  Nothing here imports ivln_ce_amd.train or oracle/.

Inputs are drawn in fp32 from a seeded generator and widened for the reference, so both sides see the same numbers.

Error bar (no tuned constants): e32 = max|fp32 torch-CPU autograd - float64| is the reference arithmetic's own fp32 noise
on the case's inputs; a kernel must stay within  4 * e32 + 4 * 2^-24 * max|float64|  (4: another summation order than
torch's).  Pure data movement and the documented-order sums are compared exactly.  Every kernel except the atomic
embedding scatter runs twice on the same inputs and must give the same bytes.  The measured hip / e32 ratio of every
case is written to train_kernels.log in the suite's log directory (beside the update tests' parity logs).

COVERED (bottom of the file) names the test of every entry point; tests/test_train_kernel_coverage.py (CPU) pins it to
the header."""
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
E_INVALID, E_UNSUPPORTED = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from kernel_bar import _Bar, _log, _log_dir, _refused, _same_bytes, _twice  # noqa: E402,F401  (shared with the other per-kernel files)


def _leaf(t, dt):
    """a fresh autograd leaf of that dtype (never the caller's tensor itself)"""
    return t.detach().to(dt).clone().requires_grad_(True)


def _strided(t, pad_l=4, pad_r=4, fill=7.0):
    """the same 2-D values as a column slice of a wider matrix (row stride > cols), on the GPU"""
    rows, cols = t.shape
    wide = torch.full((rows, pad_l + cols + pad_r), fill, dtype=t.dtype, device=DEV)
    wide[:, pad_l:pad_l + cols] = t.to(DEV)
    return wide[:, pad_l:pad_l + cols], wide


# ------------------------------------------------------------------------------------------------------------------
# BatchNorm -> ReLU -> AvgPool2d(2) backward
# ------------------------------------------------------------------------------------------------------------------
def _cbra_case(N, C, H, W, train, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(N, C, H, W, generator=g)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.3
    rm = torch.randn(C, generator=g) * 0.1
    rv = torch.rand(C, generator=g) + 0.5
    dout = torch.randn(N, C, H // 2, W // 2, generator=g)
    eps = 1e-5
    # no ReLU gate may hang on fp32 rounding: pixels whose pre-activation is within 1e-4 of zero are drawn again
    for _ in range(100):
        y64 = y.double()
        if train:
            mean, var = y64.mean((0, 2, 3)), y64.var((0, 2, 3), unbiased=False)
        else:
            mean, var = rm.double(), rv.double()
        rstd = (var + eps).rsqrt()
        z = (y64 - mean.view(1, -1, 1, 1)) * (rstd * gamma.double()).view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1)
        close = z.abs() < 1e-4
        if int(close.sum()) == 0:
            break
        y[close] = torch.randn(int(close.sum()), generator=g)
    assert int(close.sum()) <= 0, "pre-activations within 1e-4 of zero remain"
    mean32, rstd32 = mean.float(), rstd.float()
    scale = gamma * rstd32
    shift = beta - mean32 * scale
    assert int(((y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)).abs() < 5e-5).sum()) == 0
    return dict(y=y, gamma=gamma, beta=beta, rm=rm, rv=rv, dout=dout, mean=mean32, rstd=rstd32, scale=scale, shift=shift,
                eps=eps)


def _cbra_ref(c, train, dt):
    y = _leaf(c["y"], dt)
    gamma = _leaf(c["gamma"], dt)
    beta = _leaf(c["beta"], dt)
    bn = F.batch_norm(y, None if train else c["rm"].to(dt), None if train else c["rv"].to(dt), gamma, beta,
                      training=train, eps=c["eps"])
    out = F.avg_pool2d(F.relu(bn), 2)
    assert out.shape == c["dout"].shape
    out.backward(c["dout"].to(dt))
    return y.grad, gamma.grad, beta.grad


def _cbra_raw(ops, dout, y, c, train, ws, ws_floats):
    """ivln_cbra_bwd_f32 with the caller's workspace"""
    N, C, H, W = y.shape
    dgamma = torch.empty(C, device=DEV)
    dbeta = torch.empty(C, device=DEV)
    dy = torch.empty((N, C, H, W), device=DEV)
    rc = ops._T().ivln_cbra_bwd_f32(dout.data_ptr(), y.data_ptr(), c["scale"].data_ptr(), c["shift"].data_ptr(),
                                    c["mean"].data_ptr(), c["rstd"].data_ptr(), N, C, H, W, int(train), dgamma.data_ptr(),
                                    dbeta.data_ptr(), dy.data_ptr(), ws.data_ptr(), ws_floats, ops.stream_ptr())
    return rc, (dy, dgamma, dbeta)


def _misaligned(t):
    """the same contiguous values 4 bytes off a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


CBRA_SHAPES = [
    (3, 5, 8, 8),      # 16-byte path
    (3, 5, 6, 10),     # scalar path (W % 4 != 0), even sizes
    (2, 4, 7, 8),      # odd H on the 16-byte path: the last row is outside every pooling window
    (2, 4, 8, 7),      # odd W (scalar path)
    (2, 3, 25, 25),    # a 10 m map at layer 3: both odd
    (2, 3, 7, 10),     # odd H on the scalar path
    (64, 32, 16, 16),  # several image splits per channel
]


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("N,C,H,W", CBRA_SHAPES)
def test_cbra_bwd(N, C, H, W, train):
    """ivln_cbra_bwd_f32 against float64 autograd of batch_norm -> relu -> avg_pool2d(2): dy, dgamma, dbeta.  Odd H / W:
    the row / column AvgPool2d(2) drops has dz = 0 but still counts in M = N*H*W and still gets the train-mode mean
    terms."""
    from ivln_ce_amd import ops

    c = _cbra_case(N, C, H, W, train, seed=N * 1000 + C * 100 + H * 10 + W)
    r64, r32 = _cbra_ref(c, train, torch.float64), _cbra_ref(c, train, torch.float32)
    d = {k: v.to(DEV) for k, v in c.items() if torch.is_tensor(v)}
    got = _twice(lambda: ops.cbra_bwd(d["dout"], d["y"], d["scale"], d["shift"], d["mean"], d["rstd"], train))
    bar = _Bar(f"cbra_bwd {N}x{C}x{H}x{W} {'train' if train else 'eval'}")
    for name, gv, a, b in zip(("dy", "dgamma", "dbeta"), got, r64, r32):
        bar.check(name, gv, a, b)
    bar.done()


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_cbra_bwd_workspace_cap_and_misaligned_views(train):
    """The branches the wrapper's 4 MB workspace and torch's aligned allocations never take: a workspace of exactly
    4*C + 2 floats (one split per channel), and y / dout / dy views 4 bytes off a 16-byte boundary with W % 4 == 0 (the
    scalar halves of the statistics and apply kernels).  A smaller workspace is refused."""
    from ivln_ce_amd import ops

    N, C, H, W = 64, 32, 16, 16
    c = _cbra_case(N, C, H, W, train, seed=77)
    r64, r32 = _cbra_ref(c, train, torch.float64), _cbra_ref(c, train, torch.float32)
    d = {k: v.to(DEV) for k, v in c.items() if torch.is_tensor(v)}
    ws = torch.empty(4 * C + 2, device=DEV)
    bar = _Bar(f"cbra_bwd ws=4C+2 {'train' if train else 'eval'}")

    def run():
        rc, out = _cbra_raw(ops, d["dout"], d["y"], d, train, ws, ws.numel())
        assert rc == 0
        return out

    got = _twice(run)
    bars = {}
    for name, gv, a, b in zip(("dy", "dgamma", "dbeta"), got, r64, r32):
        bars[name] = bar.check(name, gv, a, b)[1]
    many = ops.cbra_bwd(d["dout"], d["y"], d["scale"], d["shift"], d["mean"], d["rstd"], train)
    for name, a, b in zip(("dy", "dgamma", "dbeta"), got, many):
        bar.within(name + " S=1/S=4", a, b, bars[name])
    rc, _ = _cbra_raw(ops, d["dout"], d["y"], d, train, ws, 4 * C + 1)
    assert rc == E_INVALID
    # misaligned views, W % 4 == 0: (3,5,8,8) and the odd-H (2,4,7,8)
    for shape in [(3, 5, 8, 8), (2, 4, 7, 8)]:
        c = _cbra_case(*shape, train, seed=sum(shape))
        r64, r32 = _cbra_ref(c, train, torch.float64), _cbra_ref(c, train, torch.float32)
        d = {k: v.to(DEV) for k, v in c.items() if torch.is_tensor(v)}
        for which in ("y", "dout"):
            dd = dict(d)
            dd[which] = _misaligned(d[which])
            got = _twice(lambda: ops.cbra_bwd(dd["dout"], dd["y"], dd["scale"], dd["shift"], dd["mean"], dd["rstd"], train))
            b2 = _Bar(f"cbra_bwd {'x'.join(map(str, shape))} {which}+4B {'train' if train else 'eval'}")
            for name, gv, a, b in zip(("dy", "dgamma", "dbeta"), got, r64, r32):
                b2.check(name, gv, a, b)
            bar.bad += b2.bad
    bar.done()


# ------------------------------------------------------------------------------------------------------------------
# attention backward + the fold of per-row key / value gradients onto shared images
# ------------------------------------------------------------------------------------------------------------------
def _index_sum_order(src, index, U):
    """ivln_index_sum_f32's documented order in fp32 on the CPU: eight contiguous chunks of ceil(rows / 8) rows, each
    summed in ascending row order, the eight partial sums added in chunk order (rows <= 8: the plain ascending sum)."""
    rows = src.shape[0]
    rpc = (rows + 7) // 8
    flat = src.reshape(rows, -1)
    dst = torch.zeros((U, flat.shape[1]), dtype=torch.float32)
    for u in range(U):
        total = None
        for ch in range(8):
            part = torch.zeros(flat.shape[1], dtype=torch.float32)
            for r in range(ch * rpc, min(rows, (ch + 1) * rpc)):
                if int(index[r]) == u:
                    part = part + flat[r]
            total = part if total is None else total + part
        dst[u] = total
    return dst.view((U,) + tuple(src.shape[1:]))


def _attn_ref(q, k_rows, v_rows, dout, valid, scale, dt):
    q = _leaf(q, dt)
    k = _leaf(k_rows, dt)
    v = _leaf(v_rows, dt)
    I = k.shape[2]
    logits = torch.einsum("rc,rci->ri", q, k) * scale
    masked = torch.arange(I).view(1, -1) >= valid.view(-1, 1)
    a = torch.softmax(logits.masked_fill(masked, float("-inf")), dim=1)
    out = torch.einsum("ri,rci->rc", a, v)
    out.backward(dout.to(dt))
    return a.detach(), q.grad, k.grad, v.grad


ATTN_SHAPES = [(5, 64, 96, 16), (7, 100, 36, 80), (3, 1024, 1024, 512), (4, 8, 8, 1)]


@pytest.mark.parametrize("mode", ["own", "shared", "one"])
@pytest.mark.parametrize("rows,Ck,Cv,I", ATTN_SHAPES)
def test_attn_bwd(rows, Ck, Cv, I, mode):
    """ivln_attn_bwd(_idx)_f32 against float64 autograd of softmax(scale * q.k) . v, with the attention weights of a
    float64 softmax whose masked tail is exactly zero.  own: every row its own key / value image (row_index NULL, k / v /
    dk / dv channel slices of one kv tensor as the update passes them); shared: row_index maps the rows onto U < rows
    images, some unused; one: every row reads image 1.  dout / q / dq are column slices of wider matrices.  The per-row
    dk / dv are folded by ivln_index_sum_f32, compared with float64 index_add_ and, bit for bit, with an fp32 sum in
    ascending row order."""
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(rows * 7 + Ck + I)
    if mode == "own":
        U, idx = rows, torch.arange(rows)
    elif mode == "shared":
        U = max(rows - 1, 2)
        idx = torch.randint(0, max(U - 1, 1), (rows,), generator=g)  # image U-1 stays unused
        idx[-1] = idx[0]
    else:
        U, idx = 3, torch.ones(rows, dtype=torch.long)
    scale = Ck ** -0.5
    q = torch.randn(rows, Ck, generator=g)
    kv = torch.randn(U, Ck + Cv, I, generator=g)
    dout = torch.randn(rows, Cv, generator=g)
    valid = torch.randint(1, I + 1, (rows,), generator=g)
    valid[0] = I
    if I > 1:
        valid[-1] = max(1, I // 3)
    k, v = kv[:, :Ck], kv[:, Ck:]
    a64, dq64, dk64, dv64 = _attn_ref(q, k[idx], v[idx], dout, valid, scale, torch.float64)
    _, dq32, dk32, dv32 = _attn_ref(q, k[idx], v[idx], dout, valid, scale, torch.float32)
    masked = torch.arange(I).view(1, -1) >= valid.view(-1, 1)
    attn = a64.float()
    assert bool((attn[masked] == 0).all())
    kv_d = kv.to(DEV)
    k_d, v_d = kv_d[:, :Ck], kv_d[:, Ck:]
    q_d, _ = _strided(q)
    do_d, _ = _strided(dout, 8, 4)
    attn_d = attn.to(DEV)
    idx_d = None if mode == "own" else idx.to(torch.int32).to(DEV)

    def run():
        dq_w = torch.full((rows, Ck + 8), 7.0, device=DEV)
        if mode == "own":
            dkv = torch.full((rows, Ck + Cv, I), float("nan"), device=DEV)
            dk, dv = dkv[:, :Ck], dkv[:, Ck:]
        else:
            dk = torch.full((rows, Ck, I), float("nan"), device=DEV)
            dv = torch.full((rows, Cv, I), float("nan"), device=DEV)
        ops.attn_bwd(do_d, attn_d, q_d, k_d, v_d, scale, dq_w[:, 4:4 + Ck], dk, dv, row_index=idx_d)
        return dq_w, dk, dv

    dq_w, dk, dv = _twice(run)
    assert bool((dq_w[:, :4] == 7.0).all()) and bool((dq_w[:, 4 + Ck:] == 7.0).all()), "dq written outside its columns"
    bar = _Bar(f"attn_bwd {rows}x{Ck}x{Cv}x{I} {mode}")
    bar.check("dq", dq_w[:, 4:4 + Ck], dq64, dq32)
    bar.check("dk(row)", dk, dk64, dk32)
    bar.check("dv(row)", dv, dv64, dv32)
    assert bool((dk.cpu()[masked.view(rows, 1, I).expand(rows, Ck, I)] == 0).all()), "dk at masked positions"
    assert bool((dv.cpu()[masked.view(rows, 1, I).expand(rows, Cv, I)] == 0).all()), "dv at masked positions"
    if mode == "own":
        # the entry point without row_index is the same launch
        dq2 = torch.empty((rows, Ck), device=DEV)
        dkv2 = torch.empty((rows, Ck + Cv, I), device=DEV)
        rc = ops._T().ivln_attn_bwd_f32(do_d.data_ptr(), do_d.stride(0), attn_d.data_ptr(), q_d.data_ptr(), q_d.stride(0),
                                        k_d.data_ptr(), k_d.stride(0), v_d.data_ptr(), v_d.stride(0), scale, rows, Ck, Cv, I,
                                        dq2.data_ptr(), dq2.stride(0), dkv2[:, :Ck].data_ptr(), dkv2.stride(0),
                                        dkv2[:, Ck:].data_ptr(), dkv2.stride(0), ops.stream_ptr())
        assert rc == 0
        assert _same_bytes(dq2, dq_w[:, 4:4 + Ck]) and _same_bytes(dkv2[:, :Ck], dk) and _same_bytes(dkv2[:, Ck:], dv)
    else:
        for name, src, r64, r32 in (("dk(fold)", dk, dk64, dk32), ("dv(fold)", dv, dv64, dv32)):
            (folded,) = _twice(lambda: (ops.index_sum(src, idx_d, U),))
            f64 = torch.zeros((U,) + tuple(r64.shape[1:]), dtype=torch.float64).index_add_(0, idx, r64)
            f32 = torch.zeros((U,) + tuple(r32.shape[1:]), dtype=torch.float32).index_add_(0, idx, r32)
            bar.check(name, folded, f64, f32)
            seq = torch.zeros(folded.shape, dtype=torch.float32)
            src_c = src.cpu()
            for r in range(rows):  # ascending r, fp32
                seq[int(idx[r])] = seq[int(idx[r])] + src_c[r]
            assert torch.equal(folded.cpu(), seq), f"{name}: not the ascending-row fp32 sum"
            assert rows > 8 or torch.equal(_index_sum_order(src_c, idx, U), seq)
    bar.done()


@pytest.mark.parametrize("rows,M,U", [(37, 12, 5), (300, 260, 3), (9, 4, 2)])
def test_index_sum_order_beyond_eight_rows(rows, M, U):
    """ivln_index_sum_f32 with more than eight rows: eight contiguous row chunks, each in ascending order, partial sums
    added in chunk order - bit for bit - and float64 index_add_ within the bar.  Refused: M % 4 != 0, a source or
    destination that is not 16-byte aligned."""
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(rows + M)
    src = torch.randn(rows, M, generator=g)
    idx = torch.randint(0, U, (rows,), generator=g)
    idx[idx == U - 1] = 0 if rows == 9 else U - 1  # (9 rows: the last image gets nothing -> zeros)
    src_d, idx_d = src.to(DEV), idx.to(torch.int32).to(DEV)
    (got,) = _twice(lambda: (ops.index_sum(src_d, idx_d, U),))
    assert torch.equal(got.cpu(), _index_sum_order(src, idx, U))
    bar = _Bar(f"index_sum {rows}x{M} U={U}")
    bar.check("dst", got, torch.zeros(U, M, dtype=torch.float64).index_add_(0, idx, src.double()),
              torch.zeros(U, M).index_add_(0, idx, src))
    bar.done()
    _refused(E_INVALID, ops.index_sum, torch.zeros(4, 6, device=DEV), idx_d[:4].contiguous(), U)
    _refused(E_INVALID, ops.index_sum, _misaligned(torch.zeros(4, 8, device=DEV)), idx_d[:4].contiguous(), U)


def test_attn_bwd_refuses_what_its_lds_cannot_hold():
    from ivln_ce_amd import ops

    def call(rows, Ck, Cv, I):
        z = torch.zeros(8, device=DEV)
        k = torch.zeros((1, 1, 1), device=DEV)
        q = torch.zeros((rows, Ck), device=DEV)
        v = torch.zeros((1, Cv, I), device=DEV)
        ops.attn_bwd(z.view(1, 8), z, q, k, v, 1.0, q, k, k)

    _refused(E_UNSUPPORTED, call, 1, 8, 8, 513)
    _refused(E_UNSUPPORTED, call, 1, 1025, 8, 4)
    _refused(E_UNSUPPORTED, call, 1, 8, 1025, 4)


# ------------------------------------------------------------------------------------------------------------------
# masked GRU BPTT
# ------------------------------------------------------------------------------------------------------------------
def _gru_case(T, N, H, seed):
    g = torch.Generator().manual_seed(seed)
    c = dict(gi=torch.randn(T, N, 3 * H, generator=g) * 0.7, h0=torch.randn(N, H, generator=g) * 0.5,
             w_hh=torch.randn(3 * H, H, generator=g) * (0.8 / H ** 0.5), b_hh=torch.randn(3 * H, generator=g) * 0.1,
             d_out=torch.randn(T, N, H, generator=g))
    masks = torch.ones(T, N, dtype=torch.uint8)
    masks[0, 0] = 0  # an episode starts at t = 0 (h0 is dropped for that row), in the middle, at the last step
    if T > 1:
        masks[T // 2, min(1, N - 1)] = 0
        masks[T - 1, N - 1] = 0
    c["masks"] = masks
    return c


def _gru_ref(c, dt):
    """float64 / fp32 masked-GRU loop (h = h * mask before each cell; gates r, z, n) with autograd"""
    T, N, H3 = c["gi"].shape
    H = H3 // 3
    gi = _leaf(c["gi"], dt)
    h0 = _leaf(c["h0"], dt)
    w = _leaf(c["w_hh"], dt)
    b = c["b_hh"].to(dt)
    h, outs, ghs, hps, sv = h0, [], [], [], []
    for t in range(T):
        hp = h * c["masks"][t].to(dt).view(N, 1)
        gh = hp @ w.t() + b
        gh.retain_grad()
        r = torch.sigmoid(gi[t, :, :H] + gh[:, :H])
        z = torch.sigmoid(gi[t, :, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[t, :, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * hp
        outs.append(h), ghs.append(gh), hps.append(hp), sv.append((r, z, n, gh[:, 2 * H:]))
    (torch.stack(outs) * c["d_out"].to(dt)).sum().backward()
    saves = [torch.stack([s[i] for s in sv]).detach() for i in range(4)]
    return dict(dgi=gi.grad, dgh=torch.stack([x.grad for x in ghs]), hp=torch.stack(hps).detach(), dw=w.grad, dh0=h0.grad,
                out=torch.stack(outs).detach(), saves=saves)


@pytest.mark.parametrize("T,N,H", [(1, 3, 8), (5, 2, 36), (4, 7, 512), (3, 20, 64)])
def test_gru_bptt_kernels(T, N, H):
    """ivln_gru_bwd_elem_f32, ivln_linear_skinny_ex_f32, ivln_gru_bwd_step_f32 and ivln_cma_seq_bwd_f32 (per-step path,
    sync_ws = NULL) against float64 autograd of the masked-GRU loop; the forward's saves are the float64 loop's, rounded
    to fp32.  Compared: dgi, dgh, hp, the implied dW_hh = dgh^T . hp and dh0 = (dgh_0 . W_hh + dhz) * mask_0.
    Chain A: elem + skinny_ex per step; chain B: elem, then the fused step kernel; chain C: the one-call entry point.
    B and C launch the same kernels with the same arguments: identical bytes.  A and C differ at most by how the compiler
    contracts the element formulas in two kernels: within the bar."""
    from ivln_ce_amd import ops

    c = _gru_case(T, N, H, seed=T * 100 + N * 10 + H)
    r64, r32 = _gru_ref(c, torch.float64), _gru_ref(c, torch.float32)
    R = T * N
    sv = [s.float().reshape(R, H).to(DEV) for s in r64["saves"]]
    out = r64["out"].float().reshape(R, H).to(DEV)
    d_out, _ = _strided(c["d_out"].reshape(R, H))
    h0, _ = _strided(c["h0"])
    masks = c["masks"].reshape(R).to(DEV)
    w_hh = c["w_hh"].to(DEV)
    whh_t = w_hh.t().contiguous()

    def fresh():
        return (torch.full((R, 3 * H), float("nan"), device=DEV), torch.full((R, 3 * H), float("nan"), device=DEV),
                torch.full((R, H), float("nan"), device=DEV), torch.full((N, H), float("nan"), device=DEV))

    def h_prev(t):
        return h0 if t == 0 else out[(t - 1) * N:t * N]

    def sl(x, t):
        return x[t * N:(t + 1) * N]

    def chain_a():
        dgi, dgh, hp, dhz = fresh()
        carry = None
        for t in range(T - 1, -1, -1):
            ops.gru_bwd_elem(sl(d_out, t), carry, *[sl(s, t) for s in sv], h_prev(t), sl(masks, t), sl(dgi, t), sl(dgh, t),
                             dhz, sl(hp, t))
            carry = ops.linear_skinny_ex(sl(dgh, t), whh_t, dhz, sl(masks, t), torch.empty((N, H), device=DEV))
        return dgi, dgh, hp, dhz, carry

    def chain_b():
        dgi, dgh, hp, dhz = fresh()
        t = T - 1
        ops.gru_bwd_elem(sl(d_out, t), None, *[sl(s, t) for s in sv], h_prev(t), sl(masks, t), sl(dgi, t), sl(dgh, t), dhz,
                         sl(hp, t))
        for t in range(T - 1, 0, -1):
            ops.gru_bwd_step(sl(dgh, t), whh_t, sl(masks, t), sl(d_out, t - 1), *[sl(s, t - 1) for s in sv], h_prev(t - 1),
                             sl(masks, t - 1), dhz, sl(dgi, t - 1), sl(dgh, t - 1), sl(hp, t - 1))
        dh0 = ops.linear_skinny_ex(sl(dgh, 0), whh_t, dhz, sl(masks, 0), torch.empty((N, H), device=DEV))
        return dgi, dgh, hp, dhz, dh0

    def chain_c():
        dgi, dgh, hp, dhz = fresh()
        ops.SEQ_PERSISTENT = False  # sync_ws = NULL: one launch per timestep
        try:
            ops.gru_seq_bwd(d_out, *sv, out, h0, masks, whh_t, T, N, dgi, dgh, hp, dhz)
        finally:
            ops.SEQ_PERSISTENT = True
        dh0 = ops.linear_skinny_ex(sl(dgh, 0), whh_t, dhz, sl(masks, 0), torch.empty((N, H), device=DEV))
        return dgi, dgh, hp, dhz, dh0

    A, B, Cc = _twice(chain_a), _twice(chain_b), _twice(chain_c)
    for i, (x, y) in enumerate(zip(B, Cc)):
        assert _same_bytes(x, y), f"fused-step chain and ivln_cma_seq_bwd_f32 differ in output {i}"
    bar = _Bar(f"gru_bptt T={T} N={N} H={H}")
    bars = {}
    for tag, res in (("A", A), ("C", Cc)):
        dgi, dgh, hp, _, dh0 = res
        for name, gv, key in (("dgi", dgi, "dgi"), ("dgh", dgh, "dgh"), ("hp", hp, "hp"), ("dh0", dh0, "dh0")):
            bars[name] = bar.check(f"{tag}:{name}", gv, r64[key], r32[key])[1]
        dw = dgh.double().cpu().t() @ hp.double().cpu()
        bar.check(f"{tag}:dW_hh", dw, r64["dw"], r32["dw"])
    for i, name in enumerate(("dgi", "dgh", "hp")):
        bar.within(f"A/C:{name}", A[i], Cc[i], bars[name])
    bar.within("A/C:dh0", A[4], Cc[4], bars["dh0"])
    # hp is the masked previous state itself: data movement
    want_hp = torch.cat([h_prev(t) * sl(masks, t).view(N, 1).float() for t in range(T)])
    assert torch.equal(Cc[2], want_hp) and torch.equal(A[2], want_hp)
    bar.done()


def test_gru_bptt_refusals():
    """H % 4 != 0 (the fused step and the one-call entry point read 16 bytes at a time), K % 4 / ldx % 4 of skinny_ex."""
    from ivln_ce_amd import ops

    H, N = 6, 2
    z = lambda *s: torch.zeros(s, device=DEV)  # noqa: E731
    m = torch.ones(N, dtype=torch.uint8, device=DEV)
    _refused(E_INVALID, ops.gru_bwd_step, z(N, 3 * H), z(H, 3 * H), m, z(N, H), z(N, H), z(N, H), z(N, H), z(N, H), z(N, H), m,
             z(N, H), z(N, 3 * H), z(N, 3 * H), z(N, H))
    ops.SEQ_PERSISTENT = False
    try:
        _refused(E_INVALID, ops.gru_seq_bwd, z(N, H), z(N, H), z(N, H), z(N, H), z(N, H), z(N, H), z(N, H), m, z(H, 3 * H), 1, N,
                 z(N, 3 * H), z(N, 3 * H), z(N, H), z(N, H))
    finally:
        ops.SEQ_PERSISTENT = True
    _refused(E_INVALID, ops.linear_skinny_ex, z(N, 6), z(3, 6), None, None, z(N, 3))        # K % 4
    _refused(E_INVALID, ops.linear_skinny_ex, z(N, 10)[:, :8], z(3, 8), None, None, z(N, 3))  # ldx % 4


@pytest.mark.parametrize("rows,K,O", [(1, 4, 1), (9, 24, 5), (17, 1536, 33)])
def test_linear_skinny_ex(rows, K, O):
    """y = (W.x + add) * rowmask with and without add / rowmask, strided x / add / y, rows that do not fill the last pass
    of eight."""
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(rows + K + O)
    x, W, add = torch.randn(rows, K, generator=g), torch.randn(O, K, generator=g) / K ** 0.5, torch.randn(rows, O, generator=g)
    mask = (torch.rand(rows, generator=g) > 0.3).to(torch.uint8)
    mask[0] = 0
    x_d, _ = _strided(x)
    add_d, _ = _strided(add, 3, 2)
    W_d, mask_d = W.to(DEV), mask.to(DEV)
    bar = _Bar(f"linear_skinny_ex {rows}x{K}x{O}")
    for use_add, use_mask in [(True, True), (False, False), (True, False), (False, True)]:
        def ref(dt):
            y = x.to(dt) @ W.to(dt).t()
            if use_add:
                y = y + add.to(dt)
            return y * mask.to(dt).view(-1, 1) if use_mask else y

        def run():
            wide = torch.full((rows, O + 5), 7.0, device=DEV)
            ops.linear_skinny_ex(x_d, W_d, add_d if use_add else None, mask_d if use_mask else None, wide[:, 2:2 + O])
            return (wide,)

        (wide,) = _twice(run)
        assert bool((wide[:, :2] == 7.0).all()) and bool((wide[:, 2 + O:] == 7.0).all())
        bar.check(f"add={int(use_add)} m={int(use_mask)}", wide[:, 2:2 + O], ref(torch.float64), ref(torch.float32))
    bar.done()


# ------------------------------------------------------------------------------------------------------------------
# bidirectional LSTM BPTT
# ------------------------------------------------------------------------------------------------------------------
def _lstm_ref(gx_f, gx_r, whh_f, whh_r, bhh_f, bhh_r, lens, dout, B, L, H, dt):
    """torch.nn.LSTM(bidirectional) on packed sequences; its input is [gx_f | gx_r] and W_ih = [I | 0] / [0 | I], so the
    leaf's gradient is the gradient with respect to the gate pre-activations"""
    G = 4 * H
    rnn = nn.LSTM(2 * G, H, bidirectional=True, batch_first=True).to(dt)
    eye, zero = torch.eye(G, dtype=dt), torch.zeros(G, G, dtype=dt)
    with torch.no_grad():
        rnn.weight_ih_l0.copy_(torch.cat((eye, zero), 1))
        rnn.weight_ih_l0_reverse.copy_(torch.cat((zero, eye), 1))
        rnn.bias_ih_l0.zero_(), rnn.bias_ih_l0_reverse.zero_()
        rnn.weight_hh_l0.copy_(whh_f.to(dt)), rnn.weight_hh_l0_reverse.copy_(whh_r.to(dt))
        rnn.bias_hh_l0.copy_(bhh_f.to(dt)), rnn.bias_hh_l0_reverse.copy_(bhh_r.to(dt))
    x = torch.cat((gx_f.view(B, L, G), gx_r.view(B, L, G)), 2).to(dt).requires_grad_(True)
    packed = nn.utils.rnn.pack_padded_sequence(x, torch.tensor(lens), batch_first=True, enforce_sorted=False)
    out = nn.utils.rnn.pad_packed_sequence(rnn(packed)[0], batch_first=True, total_length=L)[0]  # (B, L, 2H)
    (out.permute(0, 2, 1) * dout.to(dt)).sum().backward()
    out = out.detach()
    hp_f, hp_r = torch.zeros(B, L, H, dtype=dt), torch.zeros(B, L, H, dtype=dt)
    for b, n in enumerate(lens):
        hp_f[b, 1:n] = out[b, :n - 1, :H]   # h_{t-1} in processing order
        hp_r[b, :n - 1] = out[b, 1:n, H:]
    return (x.grad[:, :, :G].reshape(B * L, G), x.grad[:, :, G:].reshape(B * L, G), hp_f.view(B * L, H), hp_r.view(B * L, H),
            out.permute(0, 2, 1))


@pytest.mark.parametrize("B,L,lens", [(1, 1, [1]), (3, 5, [5, 7, 1]), (4, 80, [80, 37, 37, 100]), (3, 5, [3, 0, 5])])
def test_lstm_bidir_bwd(B, L, lens):
    """ivln_lstm_dirs_bwd_f32 (forward saves from ops.lstm_bidir(save=True)) against float64 autograd of a packed
    torch.nn.LSTM: gradients of the gate pre-activations and h_{t-1} per direction.  Lengths 1, L, beyond L (clamped like
    the forward), two equal ones.  Length 0, which pack_padded_sequence refuses: the forward runs no step and writes zeros,
    the backward's contract is dgx = 0, hprev = 0 for that row - asserted; the reference runs that row with length 1 and
    the row is left out of the comparison.  dout is non-zero at padded positions, where it must be ignored; padded
    positions of dgx / hprev are exactly zero."""
    from ivln_ce_amd import ops

    H, G = 128, 512
    g = torch.Generator().manual_seed(B * 100 + L)
    gx_f, gx_r = torch.randn(B * L, G, generator=g) * 0.6, torch.randn(B * L, G, generator=g) * 0.6
    whh_f, whh_r = torch.randn(G, H, generator=g) * 0.07, torch.randn(G, H, generator=g) * 0.07
    bhh_f, bhh_r = torch.randn(G, generator=g) * 0.1, torch.randn(G, generator=g) * 0.1
    dout = torch.randn(B, 2 * H, L, generator=g)
    eff = [min(n, L) for n in lens]
    ref_lens = [max(n, 1) for n in eff]
    r64 = _lstm_ref(gx_f, gx_r, whh_f, whh_r, bhh_f, bhh_r, ref_lens, dout, B, L, H, torch.float64)
    r32 = _lstm_ref(gx_f, gx_r, whh_f, whh_r, bhh_f, bhh_r, ref_lens, dout, B, L, H, torch.float32)
    d = [t.to(DEV) for t in (gx_f, gx_r, whh_f, whh_r, bhh_f, bhh_r)]
    lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
    out, gates, cs = ops.lstm_bidir(*d, lengths, B, L, H, save=True)
    dout_d = dout.to(DEV)
    got = _twice(lambda: ops.lstm_bidir_bwd(dout_d, out, gates, cs, d[2], d[3], lengths, B, L, H))
    keep = torch.tensor([n > 0 for n in eff]).view(B, 1).expand(B, L).reshape(B * L)
    pad = torch.tensor([[t >= n for t in range(L)] for n in eff]).view(B * L)
    bar = _Bar(f"lstm_bidir_bwd B={B} L={L} lens={lens}")
    for name, gv, a, b in zip(("dgx_f", "dgx_r", "hprev_f", "hprev_r"), got, r64, r32):
        gv = gv.cpu()
        assert bool((gv[pad] == 0).all()), f"{name}: padded positions are not exactly zero"
        bar.check(name, gv[keep], a[keep], b[keep])
    bar.check("out(fwd)", out.cpu()[torch.tensor([n > 0 for n in eff])], r64[4][torch.tensor([n > 0 for n in eff])],
              r32[4][torch.tensor([n > 0 for n in eff])])
    # hprev is the forward's own output shifted by one step: data movement
    o = out.cpu()
    for b_, n in enumerate(eff):
        hf, hr = got[2].cpu().view(B, L, H)[b_], got[3].cpu().view(B, L, H)[b_]
        assert torch.equal(hf[1:n], o[b_, :H, :max(n - 1, 0)].t()) and (n == 0 or bool((hf[0] == 0).all()))
        assert torch.equal(hr[:max(n - 1, 0)], o[b_, H:, 1:n].t()) and (n == 0 or bool((hr[n - 1] == 0).all()))
        if n == 0:
            assert bool((o[b_] == 0).all())
    bar.done()


def test_lstm_bidir_bwd_refuses_other_hidden_sizes():
    from ivln_ce_amd import ops

    z = torch.zeros(16, device=DEV)
    lengths = torch.ones(1, dtype=torch.int32, device=DEV)
    for H in (64, 256, 127):
        _refused(E_UNSUPPORTED, ops.lstm_bidir_bwd, z, z, z, z, z, z, lengths, 1, 1, H)


# ------------------------------------------------------------------------------------------------------------------
# embedding gradients
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padding_idx", [0, None])
@pytest.mark.parametrize("rows,E,V", [(3000, 50, 37), (5, 1, 3), (700, 200, 11)])
def test_embedding_scatter_add(rows, E, V, padding_idx):
    """ivln_embedding_scatter_add_f32 against float64 autograd of F.embedding over the in-range tokens, added onto a
    non-zero table gradient.  One token fills more than a third of the rows (1200 of 3000), tokens outside [0, V) are
    skipped, E is not a multiple of 64.  The kernel adds with float atomics: the order of the additions is not fixed, so
    it is compared within the bar and is the one kernel here that is NOT required to repeat its bytes."""
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(rows + E)
    tokens = torch.randint(-2, V + 3, (rows,), generator=g)
    hot = torch.randperm(rows, generator=g)[:(rows * 2) // 5]
    tokens[hot] = min(5, V - 1)
    tokens[0] = 0
    d = torch.randn(rows, E, generator=g)
    grad0 = torch.randn(V, E, generator=g)
    valid = (tokens >= 0) & (tokens < V)
    assert rows < 3000 or int((tokens == 5).sum()) > 1000
    assert int((~valid).sum()) > 0 or rows < 100

    def ref(dt):
        table = torch.zeros(V, E, dtype=dt, requires_grad=True)
        (F.embedding(tokens[valid], table, padding_idx=padding_idx) * d[valid].to(dt)).sum().backward()
        return grad0.to(dt) + table.grad

    grad = grad0.clone().to(DEV)
    ops.embedding_scatter_add(tokens.to(DEV), d.to(DEV), grad, padding_idx)
    bar = _Bar(f"embedding_scatter_add {rows}x{E} V={V} pad={padding_idx}")
    bar.check("grad", grad, ref(torch.float64), ref(torch.float32))
    if padding_idx is not None:
        assert torch.equal(grad[padding_idx].cpu(), grad0[padding_idx]), "padding row touched"
    bar.done()


@pytest.mark.parametrize("second", ["none", "strided"])
@pytest.mark.parametrize("rows,E,n_emb", [(517, 32, 5), (5, 1, 5), (13, 7, 2), (64, 32, 1)])
def test_prev_action_embed_bwd(rows, E, n_emb, second):
    """ivln_prev_action_embed_bwd_f32 against float64 autograd of table[clamp((a + 1) * mask)]: masked rows select row 0,
    actions at n_emb - 1 and beyond (and below -1) are clamped as in the forward; d1 strided, d2 absent or strided; rows
    not a multiple of 8; E = 33 is refused."""
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(rows + E + n_emb)
    pa = torch.randint(-3, n_emb + 2, (rows,), generator=g)
    mask = (torch.rand(rows, generator=g) > 0.25).to(torch.uint8)
    mask[0] = 0
    d1, d2 = torch.randn(rows, E, generator=g), torch.randn(rows, E, generator=g)
    use2 = second != "none"
    idx = ((pa.float() + 1.0) * mask.float()).long().clamp(0, n_emb - 1)

    def ref(dt):
        table = torch.zeros(n_emb, E, dtype=dt, requires_grad=True)
        emb = table[idx]
        loss = (emb * d1.to(dt)).sum()
        if use2:
            loss = loss + (emb * d2.to(dt)).sum()
        loss.backward()
        return table.grad

    d1_d, _ = _strided(d1)
    d2_d = _strided(d2, 1, 3)[0] if use2 else None
    pa_d, mask_d = pa.to(DEV), mask.to(DEV)
    (got,) = _twice(lambda: (ops.prev_action_embed_bwd(pa_d, mask_d, d1_d, d2_d, n_emb),))
    bar = _Bar(f"prev_action_embed_bwd {rows}x{E} n_emb={n_emb} d2={second}")
    bar.check("grad", got, ref(torch.float64), ref(torch.float32))
    bar.done()
    _refused(E_UNSUPPORTED, ops.prev_action_embed_bwd, pa_d, mask_d, torch.zeros(rows, 33, device=DEV), None, n_emb)


# ------------------------------------------------------------------------------------------------------------------
# losses
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_scale", [1.0, 0.37])
@pytest.mark.parametrize("T,N,A", [(1, 1, 4), (64, 8, 4), (200, 20, 6), (3, 17, 2)])
def test_ce_iw_loss(T, N, A, loss_scale):
    """ivln_ce_iw_loss_f32 against float64 autograd of the inflection-weighted cross entropy
    mean_n(sum_t w * ce / sum_t w): more than 16 trajectories (waves loop), more than 64 steps (lanes loop), zero-weight
    tails, logits shifted by +-80 and spread so the softmax saturates (log-sum-exp must be stable); dlogits carries
    loss_scale, the loss does not."""
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(T * 31 + N)
    logits = torch.randn(T, N, A, generator=g) * 3
    logits[:, ::2] += 80.0
    logits[:, 1::3] -= 80.0
    logits[T // 2] *= 6.0
    tgt = torch.randint(0, A, (T, N), generator=g)
    w = torch.where(torch.rand(T, N, generator=g) < 0.3, torch.tensor(3.2), torch.tensor(1.0))
    for n in range(N):
        w[1 + (n * 7) % T:, n] = 0  # zero-weight tail; step 0 always counts
    assert bool((w.sum(0) > 0).all())

    def ref(dt):
        lg = _leaf(logits, dt)
        ce = F.cross_entropy(lg.permute(0, 2, 1), tgt, reduction="none")
        loss = ((w.to(dt) * ce).sum(0) / w.to(dt).sum(0)).mean()
        (loss * loss_scale).backward()
        return loss.detach().reshape(1), lg.grad

    (l64, d64), (l32, d32) = ref(torch.float64), ref(torch.float32)
    lg_d, tgt_d, w_d = logits.to(DEV), tgt.to(DEV), w.to(DEV)
    loss, dl = _twice(lambda: ops.ce_iw_loss(lg_d, tgt_d, w_d, loss_scale))
    bar = _Bar(f"ce_iw_loss {T}x{N}x{A} scale={loss_scale}")
    bar.check("loss", loss, l64, l32)
    bar.check("dlogits", dl, d64, d32)
    assert bool((dl.cpu()[w == 0] == 0).all()), "zero-weight steps carry a gradient"
    bar.done()


def _pm_chunked_ref(pre, p, mask, gout, alpha, dt, chunk=1024):
    """alpha * gout * mean over L[:, mask] of L[j][i] = (tanh(pre_i) - p_j)^2 and its gradient, by autograd over blocks of
    columns (the n x n matrix is never whole in memory)"""
    n = pre.numel()
    pre = _leaf(pre, dt)
    p, count = p.to(dt), n * int(mask.sum())
    total = torch.zeros((), dtype=dt)
    for i0 in range(0, n, chunk):
        m = mask[i0:i0 + chunk].bool()
        if not bool(m.any()):
            continue
        hat = torch.tanh(pre[i0:i0 + chunk])[m]
        part = ((hat.view(1, -1) - p.view(-1, 1)) ** 2).sum() / count
        (part * alpha * float(gout)).backward()
        total = total + part.detach()
    grad = pre.grad if pre.grad is not None else torch.zeros(n, dtype=dt)
    return total.reshape(1), grad


def _pm_mask(n, kind, g):
    if kind == "ones":
        return torch.ones(n, dtype=torch.uint8)
    if kind == "single":
        m = torch.zeros(n, dtype=torch.uint8)
        m[n // 2] = 1
        return m
    m = (torch.rand(n, generator=g) < 0.6).to(torch.uint8)
    m[0] = 1
    m[n - 1] = 1
    return m


@pytest.mark.parametrize("n,kind", [(n, k) for n in (1, 17, 512) for k in ("ones", "single", "pattern")] + [(11000, "pattern")])
def test_pm_loss_and_masked_mean(n, kind):
    """ivln_pm_loss_fwd/bwd_f32 and ivln_pm_masked_mean_fwd/bwd_f32 against float64 autograd of the progress monitor's
    (n, n) broadcast loss L[j][i] = (tanh(pre_i) - p_j)^2.  n = 11000 keeps one float64 n x n block of the reference
    under 1 GB (it is walked in column blocks).  The masked mean must also be the mean of the matrix ivln_pm_loss_fwd_f32
    materialises, over the selected columns, and its backward the gradient of alpha * gout * that mean."""
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(n)
    pre, p = torch.randn(n, generator=g), torch.rand(n, generator=g)
    mask = _pm_mask(n, kind, g)
    alpha, gout = 0.7, 1.3
    pre_d, p_d, mask_d = pre.to(DEV), p.to(DEV), mask.to(DEV)
    bar = _Bar(f"pm n={n} mask={kind}")
    hat, Lm = _twice(lambda: ops.pm_loss_fwd(pre_d, p_d))
    bar.check("hat", hat, torch.tanh(pre.double()), torch.tanh(pre))
    worst = None
    for i0 in range(0, n, 1024):  # the matrix in column blocks
        a = (torch.tanh(pre.double()[i0:i0 + 1024]).view(1, -1) - p.double().view(-1, 1)) ** 2
        b = (torch.tanh(pre[i0:i0 + 1024]).view(1, -1) - p.view(-1, 1)) ** 2
        gv = Lm[:, i0:i0 + 1024].cpu().double()
        err, e32, mx = float((gv - a).abs().max()), float((b.double() - a).abs().max()), float(a.abs().max())
        if worst is None or err - (4 * e32 + 4 * EPS * mx) > worst[0] - (4 * worst[1] + 4 * EPS * worst[2]):
            worst = (err, e32, mx)
    err, e32, mx = worst
    ok = err <= 4 * e32 + 4 * EPS * mx
    _log(f"{bar.case:44s} {'L':10s} hip {err:.3e}  e32 {e32:.3e}  hip/e32 {err / e32 if e32 else 0.0:8.2f}  max|ref| {mx:.3e}  "
         f"bar {4 * e32 + 4 * EPS * mx:.3e}  {'ok' if ok else 'OVER'} (worst column block)")
    if not ok:
        bar.bad.append(f"L: {err:.3e} over {4 * e32 + 4 * EPS * mx:.3e}")
    # masked mean
    out2, hat2, dsum = _twice(lambda: ops.pm_masked_mean_fwd(pre_d, p_d, mask_d))
    assert _same_bytes(hat2, hat)
    (m64, g64), (m32, g32) = (_pm_chunked_ref(pre, p, mask, gout, alpha, dt) for dt in (torch.float64, torch.float32))
    mean_bar = bar.check("mean", out2[:1], m64, m32)[1]
    count = float(n) * float(mask.sum())
    assert abs(float(out2[1]) - count) <= 4 * EPS * count, (float(out2[1]), count)
    sel = mask_d.bool()
    mat_mean = Lm[:, sel].double().mean().reshape(1)  # of the materialised matrix (float64 sum of its fp32 entries)
    bar.within("mean/matrix", out2[:1], mat_mean, mean_bar)
    gout_d = torch.tensor([gout], device=DEV)
    (dpre,) = _twice(lambda: (ops.pm_masked_mean_bwd(gout_d, hat2, dsum, mask_d, out2, alpha),))
    bar.check("dpre(mean)", dpre, g64, g32)
    assert bool((dpre.cpu()[mask == 0] == 0).all())
    # matrix backward with a dense upstream gradient
    dL = torch.randn(n, n, generator=g)
    dL_d = dL.to(DEV)
    (dpre_m,) = _twice(lambda: (ops.pm_loss_bwd(dL_d, hat, p_d),))

    def ref(dt, chunk=1024):
        x = _leaf(pre, dt)
        for i0 in range(0, n, chunk):
            L = (torch.tanh(x[i0:i0 + chunk]).view(1, -1) - p.to(dt).view(-1, 1)) ** 2
            (L * dL[:, i0:i0 + chunk].to(dt)).sum().backward()
        return x.grad

    bar.check("dpre(matrix)", dpre_m, ref(torch.float64), ref(torch.float32))
    bar.done()


def test_pm_masked_mean_at_its_limit():
    """n = 14999 of the 15000 progress values the one-workgroup kernel's LDS holds (reference in column blocks); 15001 is
    refused."""
    from ivln_ce_amd import ops

    n = 14999
    g = torch.Generator().manual_seed(n)
    pre, p = torch.randn(n, generator=g), torch.rand(n, generator=g)
    mask = _pm_mask(n, "pattern", g)
    pre_d, p_d, mask_d = pre.to(DEV), p.to(DEV), mask.to(DEV)
    out2, hat, dsum = _twice(lambda: ops.pm_masked_mean_fwd(pre_d, p_d, mask_d))
    gout_d = torch.tensor([1.0], device=DEV)
    (dpre,) = _twice(lambda: (ops.pm_masked_mean_bwd(gout_d, hat, dsum, mask_d, out2, 1.0),))
    (m64, g64), (m32, g32) = (_pm_chunked_ref(pre, p, mask, 1.0, 1.0, dt) for dt in (torch.float64, torch.float32))
    bar = _Bar(f"pm n={n} (limit)")
    bar.check("mean", out2[:1], m64, m32)
    bar.check("dpre(mean)", dpre, g64, g32)
    bar.done()
    big = torch.zeros(15001, device=DEV)
    _refused(E_INVALID, ops.pm_masked_mean_fwd, big, big, torch.ones(15001, dtype=torch.uint8, device=DEV))


# ------------------------------------------------------------------------------------------------------------------
# element / data-movement / reduction kernels
# ------------------------------------------------------------------------------------------------------------------
RAGGED = [(1, 1), (17, 33), (300, 70)]


@pytest.mark.parametrize("rows,cols", RAGGED)
def test_relu_bwd_and_add2d_exact(rows, cols):
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(rows)
    dy, y, b = (torch.randn(rows, cols, generator=g) for _ in range(3))
    y[0, 0] = 0.0
    y[-1, -1] = -0.0
    dy_d, y_d, b_d = _strided(dy)[0], _strided(y, 8, 0)[0], _strided(b, 0, 1)[0]

    def run():
        w1 = torch.full((rows, cols + 3), 7.0, device=DEV)
        w2 = torch.full((rows, cols + 3), 7.0, device=DEV)
        ops.relu_bwd(dy_d, y_d, w1[:, 1:1 + cols])
        ops.add2d(dy_d, b_d, w2[:, 2:2 + cols])
        return w1, w2, ops.relu_bwd(dy_d, y_d), ops.add2d(dy_d, b_d)

    w1, w2, dx, s = _twice(run)
    want = torch.where(y > 0, dy, torch.zeros(()))
    assert torch.equal(dx.cpu(), want) and torch.equal(w1[:, 1:1 + cols].cpu(), want)
    assert torch.equal(s.cpu(), dy + b) and torch.equal(w2[:, 2:2 + cols].cpu(), dy + b)
    assert bool((w1[:, 0] == 7.0).all()) and bool((w1[:, 1 + cols:] == 7.0).all())
    assert bool((w2[:, :2] == 7.0).all()) and bool((w2[:, 2 + cols:] == 7.0).all())


@pytest.mark.parametrize("rows,cols", RAGGED + [(16, 16), (33, 17)])
def test_transpose_exact(rows, cols):
    from ivln_ce_amd import ops

    x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(cols))
    x_d = x.to(DEV)
    (y,) = _twice(lambda: (ops.transpose(x_d),))
    assert torch.equal(y.cpu(), x.t().contiguous())


@pytest.mark.parametrize("O,I,KH,KW", [(1, 1, 1, 1), (3, 5, 7, 7), (4, 2, 3, 5), (17, 33, 1, 2), (6, 3, 5, 1)])
def test_weight_flip_transpose_exact(O, I, KH, KW):
    from ivln_ce_amd import ops

    w = torch.randn(O, I, KH, KW, generator=torch.Generator().manual_seed(O + KW))
    w_d = w.to(DEV)
    (wt,) = _twice(lambda: (ops.weight_flip_transpose(w_d),))
    assert torch.equal(wt.cpu(), w.flip(2, 3).permute(1, 0, 2, 3).contiguous())


def _chansum_raw(ops, x, ws, ws_floats):
    N, C, H, W = x.shape
    out = torch.full((C,), float("nan"), device=DEV)
    rc = ops._T().ivln_nchw_chansum_f32(x.data_ptr(), N, C, H * W, out.data_ptr(), ws.data_ptr(), ws_floats,
                                        ops.stream_ptr())
    return rc, out


@pytest.mark.parametrize("N,C,H,W", [(20, 7, 4, 4), (600, 3, 4, 4), (3, 5, 64, 64), (2, 3, 13, 11), (1, 1, 1, 1), (9, 4, 5, 7)])
def test_nchw_chansum(N, C, H, W):
    """Both paths of ivln_nchw_chansum_f32 - short rows (HW <= 128: column sums, then HW columns per channel) and long rows
    (image splits per channel, 16-byte or scalar loads) - with the wrapper's workspace and with one of exactly C floats,
    which sends short rows down the long-row path with one split; an x that is 4 bytes off a 16-byte boundary; a
    workspace below C floats is refused."""
    from ivln_ce_amd import ops

    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(N + H))
    r64, r32 = x.double().sum((0, 2, 3)), x.sum((0, 2, 3))
    x_d = x.to(DEV)
    bar = _Bar(f"nchw_chansum {N}x{C}x{H}x{W}")
    (a,) = _twice(lambda: (ops.nchw_chansum(x_d),))
    bar.check("wrapper", a, r64, r32)
    ws = torch.empty(C, device=DEV)

    def tiny(xx):
        rc, out = _chansum_raw(ops, xx, ws, C)
        assert rc == 0
        return (out,)

    (b,) = _twice(lambda: tiny(x_d))
    bar.check("ws=C", b, r64, r32)
    x_m = _misaligned(x_d)
    (c,) = _twice(lambda: tiny(x_m))
    bar.check("ws=C,+4B", c, r64, r32)
    (d,) = _twice(lambda: (ops.nchw_chansum(x_m),))
    bar.check("+4B", d, r64, r32)
    assert _chansum_raw(ops, x_d, ws, C - 1)[0] == E_INVALID
    bar.done()


def _colsum_raw(ops, x, out, accumulate, ws, ws_floats):
    return ops._T().ivln_colsum_f32(x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], out.data_ptr(), int(accumulate),
                                    ws.data_ptr(), ws_floats, ops.stream_ptr())


@pytest.mark.parametrize("rows,cols", RAGGED + [(700, 5), (1000, 130), (256 * 130 + 3, 2)])
def test_colsum(rows, cols):
    """ivln_colsum_f32: strided rows, accumulate = 1, a ragged last split (700 rows -> 234 + 234 + 232), more rows than 128
    splits of 256, and a workspace that caps the splits (2 * cols floats; cols - 1 floats are refused)."""
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(rows + cols)
    x, out0 = torch.randn(rows, cols, generator=g), torch.randn(cols, generator=g)
    x_d, _ = _strided(x, 4, 3)
    bar = _Bar(f"colsum {rows}x{cols}")
    (a,) = _twice(lambda: (ops.colsum(x_d),))
    bar.check("sum", a, x.double().sum(0), x.sum(0))
    (b,) = _twice(lambda: (ops.colsum(x_d, out0.clone().to(DEV), accumulate=True),))
    bar.check("accumulate", b, out0.double() + x.double().sum(0), out0 + x.sum(0))
    ws = torch.empty(2 * cols, device=DEV)

    def capped():
        out = torch.full((cols,), float("nan"), device=DEV)
        assert _colsum_raw(ops, x_d, out, 0, ws, ws.numel()) == 0
        return (out,)

    (c,) = _twice(capped)
    bar.check("ws=2*cols", c, x.double().sum(0), x.sum(0))
    assert _colsum_raw(ops, x_d, torch.empty(cols, device=DEV), 0, ws, cols - 1) == E_INVALID
    bar.done()


# ------------------------------------------------------------------------------------------------------------------
# Adam with the device-side guard
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 2, 257])
def test_adam_step_guarded(n):
    """ivln_adam_step_guarded_f32 with per-segment learning rates (seg_of / seg_lr), n not a multiple of 256, step 3 on
    non-zero moments.  Guard non-zero: parameters, moments and gradients keep their bytes (zero_grad included).  Guard
    zero: the bytes of ivln_adam_step_f32, which is within the bar of torch.optim.Adam in float64.  step < 1 is
    refused."""
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(n)
    p0, g0, m0 = (torch.randn(n, generator=g) for _ in range(3))
    v0 = torch.rand(n, generator=g) * 0.1
    cut = max(1, n // 3)
    seg = torch.cat((torch.zeros(cut, dtype=torch.int32), torch.ones(n - cut, dtype=torch.int32)))
    lrs = [2.5e-4, 1e-2]
    step, gs, b1, b2, eps = 3, 0.5, 0.9, 0.999, 1e-8
    seg_d, lr_d = seg.to(DEV), torch.tensor(lrs, device=DEV)

    def run(guard_val, raw=False):
        p, gr, m, v = (t.clone().to(DEV) for t in (p0, g0, m0, v0))
        if raw:
            rc = ops._T().ivln_adam_step_f32(p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1.0, seg_d.data_ptr(),
                                             lr_d.data_ptr(), b1, b2, eps, step, gs, 1, ops.stream_ptr())
            assert rc == 0
        else:
            guard = None if guard_val is None else torch.tensor([guard_val], dtype=torch.int32, device=DEV)
            ops.adam_step(p, gr, m, v, 1.0, step, b1, b2, eps, seg_of=seg_d, seg_lr=lr_d, grad_scale=gs, zero_grad=True,
                          guard=guard)
        return p, gr, m, v

    held = _twice(lambda: run(1))
    for name, a, b in zip(("params", "grads", "exp_avg", "exp_avg_sq"), held, (p0, g0, m0, v0)):
        assert _same_bytes(a.cpu(), b), f"guard set: {name} changed"
    for a, b in zip(run(0x10000), (p0, g0, m0, v0)):  # any non-zero word
        assert _same_bytes(a.cpu(), b)
    open_ = _twice(lambda: run(0))
    for other in (run(None), run(None, raw=True)):
        for a, b in zip(open_, other):
            assert _same_bytes(a, b), "guard zero / NULL / ivln_adam_step_f32 differ"
    assert float(open_[1].abs().max()) == 0.0  # zero_grad

    def ref(dt):
        ps = [p0[:cut].to(dt).clone().requires_grad_(True), p0[cut:].to(dt).clone().requires_grad_(True)]
        opt = torch.optim.Adam([{"params": [ps[0]], "lr": lrs[0]}, {"params": [ps[1]], "lr": lrs[1]}], betas=(b1, b2), eps=eps)
        for q, s in zip(ps, (slice(0, cut), slice(cut, n))):
            q.grad = g0[s].to(dt) * gs
            opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0[s].to(dt).clone(),
                            "exp_avg_sq": v0[s].to(dt).clone()}
        opt.step()
        return (torch.cat([q.detach() for q in ps]), torch.cat([opt.state[q]["exp_avg"] for q in ps]),
                torch.cat([opt.state[q]["exp_avg_sq"] for q in ps]))

    bar = _Bar(f"adam_step_guarded n={n}")
    for name, gv, a, b in zip(("params", "exp_avg", "exp_avg_sq"), (open_[0], open_[2], open_[3]), ref(torch.float64),
                              ref(torch.float32)):
        bar.check(name, gv, a, b)
    bar.done()
    z = torch.zeros(4, device=DEV)
    _refused(E_INVALID, ops.adam_step, z, z.clone(), z.clone(), z.clone(), 1e-3, 0)


# every entry point of the header's backward / loss / optimizer section -> the test that calls it
COVERED = {
    "ivln_relu_bwd_f32": "test_relu_bwd_and_add2d_exact",
    "ivln_add2d_f32": "test_relu_bwd_and_add2d_exact",
    "ivln_colsum_f32": "test_colsum",
    "ivln_nchw_chansum_f32": "test_nchw_chansum",
    "ivln_transpose_f32": "test_transpose_exact",
    "ivln_weight_flip_transpose_f32": "test_weight_flip_transpose_exact",
    "ivln_attn_bwd_f32": "test_attn_bwd",
    "ivln_attn_bwd_idx_f32": "test_attn_bwd",
    "ivln_index_sum_f32": "test_index_sum_order_beyond_eight_rows",
    "ivln_gru_bwd_elem_f32": "test_gru_bptt_kernels",
    "ivln_gru_bwd_step_f32": "test_gru_bptt_kernels",
    "ivln_cma_seq_bwd_f32": "test_gru_bptt_kernels",
    "ivln_linear_skinny_ex_f32": "test_linear_skinny_ex",
    "ivln_lstm_dirs_bwd_f32": "test_lstm_bidir_bwd",
    "ivln_cbra_bwd_f32": "test_cbra_bwd",
    "ivln_embedding_scatter_add_f32": "test_embedding_scatter_add",
    "ivln_prev_action_embed_bwd_f32": "test_prev_action_embed_bwd",
    "ivln_ce_iw_loss_f32": "test_ce_iw_loss",
    "ivln_pm_loss_fwd_f32": "test_pm_loss_and_masked_mean",
    "ivln_pm_loss_bwd_f32": "test_pm_loss_and_masked_mean",
    "ivln_pm_masked_mean_fwd_f32": "test_pm_loss_and_masked_mean",
    "ivln_pm_masked_mean_bwd_f32": "test_pm_loss_and_masked_mean",
    "ivln_adam_step_f32": "test_adam_step_guarded",
    "ivln_adam_step_guarded_f32": "test_adam_step_guarded",
}
