"""ivln_se_gate_f32 and ivln_se_apply_f32 (csrc/group_conv.hip, include/ivln_depth_backbones.h), each alone, against
float64: the squeeze-and-excite tail of the SE depth backbones.  Error bar and run-twice-same-bytes check of
tests/kernel_bar.py (4 * e32 + 4 * 2^-24 * max|ref|, e32 = the same formula in fp32 on the CPU); every comparison is logged
before anything is asserted (se_kernels.log in the suite's log directory).

C = 128 and 1024 (the SE-ResNeXt backbones' narrowest and widest block outputs, C/16 = 8 and 64 hidden units), HW = 16
and 1024 (their smallest and largest planes) and once 35 (odd: no vector width divides it), batches 1 and 3, the input
as a plain tensor and as `Deferred` split-K slabs, the identity as a tensor and as a second group-normalised operand, and
gates driven to both saturated ends."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_bar import _Bar, _twice  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LOG = "se_kernels.log"
GROUPS, EPS = 16, 1e-5
SHAPES = [(128, 16), (128, 1024), (1024, 16), (1024, 1024), (128, 35)]  # (C, HW)
PLANE = {16: (4, 4), 1024: (32, 32), 35: (5, 7)}


def _operand(t, splits, g):
    """NCHW CPU tensor -> (what the kernel takes, its exact value in float64, its value summed in fp32).  splits == 0: the
    tensor itself; else a `Deferred` of that many random slabs of its [C][N*HW] matrix."""
    from ivln_ce_amd import ops

    if splits == 0:
        return t.to(DEV), t.double(), t
    N, Cc, H, W = t.shape
    m = t.permute(1, 0, 2, 3).reshape(Cc, N * H * W)
    parts = [torch.randn(m.shape, generator=g) for _ in range(splits - 1)]
    parts.append(m - sum(parts) if parts else m)
    st = torch.stack(parts).contiguous()
    back = lambda s: s.view(Cc, N, H, W).permute(1, 0, 2, 3).contiguous()  # noqa: E731
    s32 = st[0].clone()
    for z in range(1, splits):
        s32 += st[z]
    return ops.Deferred(st.view(-1).to(DEV), splits, N, Cc, H, W), back(st.double().sum(0)), back(s32)


def _excite(Cc, g, bias2=0.0, scale2=1.0):
    Cr = Cc // 16
    w1 = torch.randn(Cr, Cc, generator=g) * (2.0 / Cc) ** 0.5
    b1 = 0.1 * torch.randn(Cr, generator=g)
    w2 = scale2 * torch.randn(Cc, Cr, generator=g) * (2.0 / Cr) ** 0.5
    b2 = 0.1 * torch.randn(Cc, generator=g) + bias2
    return w1, b1, w2, b2


def _gate_ref(x, gamma, beta, w1, b1, w2, b2):
    dt = x.dtype
    z = F.group_norm(x, GROUPS, gamma.to(dt), beta.to(dt), EPS)
    s = z.mean(dim=(2, 3))
    return torch.sigmoid(F.linear(F.relu(F.linear(s, w1.to(dt), b1.to(dt))), w2.to(dt), b2.to(dt)))


@pytest.mark.parametrize("splits", [0, 1, 5])
@pytest.mark.parametrize("Cc,HW", SHAPES)
def test_se_gate_matches_float64(Cc, HW, splits):
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(Cc + HW + splits)
    bar = _Bar(f"se_gate C {Cc} HW {HW} splits {splits}", LOG)
    H, W = PLANE[HW]
    for N in (1, 3):
        x = torch.randn(N, Cc, H, W, generator=g) * (1.0 + torch.rand(1, Cc, 1, 1, generator=g)) + 0.3 * torch.randn(1, Cc, 1, 1, generator=g)
        gamma, beta = 1.0 + 0.2 * torch.randn(Cc, generator=g), 0.2 * torch.randn(Cc, generator=g)
        e = _excite(Cc, g)
        xd, x64, x32 = _operand(x, splits, g)
        dev = [t.to(DEV) for t in (gamma, beta) + e]
        (got,) = _twice(lambda: (ops.se_gate(xd, dev[0], dev[1], GROUPS, EPS, *dev[2:]),))
        bar.check(f"N{N}", got, _gate_ref(x64, gamma, beta, *e), _gate_ref(x32, gamma, beta, *e))
    bar.done()


@pytest.mark.parametrize("end,bias2", [("open", 40.0), ("shut", -40.0), ("both", 0.0)])
def test_se_gate_saturates_at_both_ends(end, bias2):
    """Large pre-activations: +-40 from the last bias (sigmoid = 1 - 4e-18 / 4e-18), and +-hundreds from weights scaled by
    300 (exp overflows on the shut side: the gate is 0 there, not NaN)."""
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(3)
    bar = _Bar(f"se_gate saturated {end}", LOG)
    Cc, N = 128, 3
    x = torch.randn(N, Cc, 4, 4, generator=g)
    gamma, beta = 1.0 + 0.2 * torch.randn(Cc, generator=g), 0.5 + 0.2 * torch.randn(Cc, generator=g)
    e = _excite(Cc, g, bias2=bias2, scale2=300.0 if end == "both" else 1.0)
    dev = [t.to(DEV) for t in (gamma, beta) + e]
    (got,) = _twice(lambda: (ops.se_gate(x.to(DEV), dev[0], dev[1], GROUPS, EPS, *dev[2:]),))
    ref = _gate_ref(x.double(), gamma, beta, *e)
    assert bool(torch.isfinite(got).all())
    if end == "open":
        assert float(ref.min()) > 1 - 1e-12 and float(got.min()) == 1.0
    elif end == "shut":
        assert float(ref.max()) < 1e-12 and float(got.max()) < 1e-12
    else:
        assert float(ref.min()) < 1e-30 and float(ref.max()) > 1 - 1e-12  # (both ends are reached)
    bar.check("gate", got, ref, _gate_ref(x, gamma, beta, *e))
    bar.done()


def _apply_ref(x, gamma, beta, gate, residual=None, x2=None, gamma2=None, beta2=None):
    dt = x.dtype
    z = F.group_norm(x, GROUPS, gamma.to(dt), beta.to(dt), EPS)
    idv = residual.to(dt) if residual is not None else F.group_norm(x2, GROUPS, gamma2.to(dt), beta2.to(dt), EPS)
    return F.relu(gate.to(dt)[:, :, None, None] * z + idv)


@pytest.mark.parametrize("identity", ["tensor", "groupnorm"])
@pytest.mark.parametrize("splits", [0, 1, 5])
@pytest.mark.parametrize("Cc,HW", SHAPES)
def test_se_apply_matches_float64(Cc, HW, splits, identity):
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(7 * Cc + HW + splits + len(identity))
    bar = _Bar(f"se_apply C {Cc} HW {HW} splits {splits} {identity}", LOG)
    H, W = PLANE[HW]
    for N in (1, 3):
        x = torch.randn(N, Cc, H, W, generator=g) * (1.0 + torch.rand(1, Cc, 1, 1, generator=g)) + 0.3 * torch.randn(1, Cc, 1, 1, generator=g)
        gamma, beta = 1.0 + 0.2 * torch.randn(Cc, generator=g), 0.2 * torch.randn(Cc, generator=g)
        gate = torch.rand(N, Cc, generator=g)
        gate[:, ::7], gate[:, 3::7] = 0.0, 1.0  # (the saturated ends among them)
        xd, x64, x32 = _operand(x, splits, g)
        pd = [t.to(DEV) for t in (gamma, beta, gate)]
        if identity == "tensor":
            res = torch.randn(N, Cc, H, W, generator=g)
            rd = res.to(DEV)
            run = lambda: (ops.se_apply(xd, pd[0], pd[1], GROUPS, EPS, pd[2], residual=rd),)  # noqa: E731
            r64 = _apply_ref(x64, gamma, beta, gate, residual=res)
            r32 = _apply_ref(x32, gamma, beta, gate, residual=res)
        else:
            x2 = 2.0 * torch.randn(N, Cc, H, W, generator=g) + 0.5
            gamma2, beta2 = 1.0 + 0.2 * torch.randn(Cc, generator=g), 0.2 * torch.randn(Cc, generator=g)
            x2d, x2_64, x2_32 = _operand(x2, 3 if splits else 0, g)
            qd = [gamma2.to(DEV), beta2.to(DEV)]
            run = lambda: (ops.se_apply(xd, pd[0], pd[1], GROUPS, EPS, pd[2], x2=x2d, gamma2=qd[0], beta2=qd[1]),)  # noqa: E731
            r64 = _apply_ref(x64, gamma, beta, gate, x2=x2_64, gamma2=gamma2, beta2=beta2)
            r32 = _apply_ref(x32, gamma, beta, gate, x2=x2_32, gamma2=gamma2, beta2=beta2)
        (got,) = _twice(run)
        bar.check(f"N{N}", got, r64, r32)
    bar.done()


def test_se_apply_with_open_gates_is_the_groupnorm_launch():
    """gate == 1 everywhere: the tail is the block's ordinary last GroupNorm (+ identity, ReLU) - within that quantity's
    bar of ops.groupnorm on the same `Deferred` input (another summation order, not another quantity)."""
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(21)
    bar = _Bar("se_apply open gates vs groupnorm", LOG)
    N, Cc, H, W = 2, 128, 32, 32
    x = torch.randn(N, Cc, H, W, generator=g)
    gamma, beta = 1.0 + 0.2 * torch.randn(Cc, generator=g), 0.2 * torch.randn(Cc, generator=g)
    res = torch.randn(N, Cc, H, W, generator=g)
    xd, x64, x32 = _operand(x, 4, g)
    gd, bd, rd = gamma.to(DEV), beta.to(DEV), res.to(DEV)
    a = ops.se_apply(xd, gd, bd, GROUPS, EPS, torch.ones(N, Cc, device=DEV), residual=rd)
    b = ops.groupnorm(xd, gd, bd, GROUPS, EPS, relu=True, residual=rd)
    r64 = _apply_ref(x64, gamma, beta, torch.ones(N, Cc), residual=res)
    r32 = _apply_ref(x32, gamma, beta, torch.ones(N, Cc), residual=res)
    _, bar_a = bar.check("se_apply", a, r64, r32)
    bar.check("groupnorm", b, r64, r32)
    bar.within("apart", a, b, 2 * bar_a)
    bar.done()


def test_se_refusals():
    from kernel_bar import _refused

    from ivln_ce_amd import ops

    x = torch.randn(1, 4096, 2, 2, device=DEV)
    p = torch.ones(4096, device=DEV)
    w1, b1, w2, b2 = (torch.zeros(s, device=DEV) for s in ((256, 4096), (256,), (4096, 256), (4096,)))
    _refused(-5, ops.se_gate, x, p, p, 16, EPS, w1, b1, w2, b2)                      # C > 2048 (and C / r > 128)
    x = torch.randn(1, 32, 2, 2, device=DEV)
    p = torch.ones(32, device=DEV)
    gate = torch.ones(1, 32, device=DEV)
    _refused(-5, ops.se_apply, x, p, p, 16, EPS, gate)                                 # no identity
    _refused(-5, ops.se_apply, x, p, p, 16, EPS, gate, residual=x, x2=x, gamma2=p, beta2=p)  # two identities
    _refused(-5, ops.se_apply, x, p, p, 5, EPS, gate, residual=x)                      # C % groups != 0
    torch.cuda.synchronize()
