"""ivln_gconv3x3_f32 (csrc/group_conv.hip, include/ivln_depth_backbones.h) alone against F.conv2d(groups=...) in float64:
the grouped 3x3 conv of the ResNeXt depth backbones.  Error bar and run-twice-same-bytes check of tests/kernel_bar.py
(4 * e32 + 4 * 2^-24 * max|ref|, e32 = the fp32 torch-CPU conv's own error); every comparison is logged before anything
is asserted (group_conv_kernels.log in the suite's log directory).

Channels per group 1, 3, 4, 8 (VALU form: several groups per workgroup where the count divides 16, one group otherwise),
16, 32, 64 (fp32 MFMA form, 1 / 2 / 4 staged chunks of 16 input channels); planes 4x4, 5x7, 8x8, 16x16 (the three tile
shapes 4 / 8 / 16 columns wide) and 33x32 (a partial column tile and, at stride 2, an odd edge); batches 1 and 3 (tile rows
run over the batch: a tile's rows belong to several images)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_bar import _Bar, _refused, _twice  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LOG = "group_conv_kernels.log"
PLANES = [(4, 4), (5, 7), (8, 8), (16, 16), (33, 32)]


def _case(bar, name, N, cpg, groups, H, W, stride, g, pad_channels=0):
    from ivln_ce_amd import ops

    Cc = cpg * groups
    x = torch.randn(N, Cc + pad_channels, H, W, generator=g)
    w = torch.randn(Cc, cpg, 3, 3, generator=g) / (3.0 * cpg ** 0.5)
    xs = x[:, :Cc]
    ref64 = F.conv2d(xs.double(), w.double(), stride=stride, padding=1, groups=groups)
    ref32 = F.conv2d(xs.contiguous(), w, stride=stride, padding=1, groups=groups)
    xd, wd = x.to(DEV), w.to(DEV)
    if pad_channels:  # a channel slice of a wider buffer: images further apart than C * H * W
        run = lambda: (ops.gconv3x3(xd[:, :Cc], wd, groups, stride=stride, in_img_stride=(Cc + pad_channels) * H * W),)  # noqa: E731
    else:
        run = lambda: (ops.gconv3x3(xd, wd, groups, stride=stride),)  # noqa: E731
    (got,) = _twice(run)
    assert tuple(got.shape) == tuple(ref64.shape), (name, got.shape, ref64.shape)
    bar.check(name, got, ref64, ref32)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cpg,groups", [(c, 16) for c in (1, 3, 4, 8, 16, 32, 64)] + [(3, 2), (8, 2), (32, 2)])
def test_gconv3x3_matches_float64(cpg, groups, stride):
    g = torch.Generator().manual_seed(1000 * cpg + 10 * groups + stride)
    bar = _Bar(f"gconv3x3 cpg {cpg} groups {groups} stride {stride}", LOG)
    for H, W in PLANES:
        for N in (1, 3):
            _case(bar, f"{H}x{W} N{N}", N, cpg, groups, H, W, stride, g)
    bar.done()


@pytest.mark.parametrize("cpg,stride", [(4, 1), (4, 2), (32, 1), (32, 2), (3, 2)])
def test_gconv3x3_reads_a_strided_batch(cpg, stride):
    g = torch.Generator().manual_seed(77 + cpg + stride)
    bar = _Bar(f"gconv3x3 image stride cpg {cpg} stride {stride}", LOG)
    _case(bar, "8x8 N3", 3, cpg, 16, 8, 8, stride, g, pad_channels=5)
    _case(bar, "33x32 N2", 2, cpg, 16, 33, 32, stride, g, pad_channels=1)
    bar.done()


def test_gconv3x3_backbone_shapes():
    """The forms the ResNeXt backbones run (baseplanes 32: 16 groups of 4, 8, 16, 32 channels on 32^2, 16^2, 8^2, 4^2;
    the first block of layers 2-4 at stride 2 from the plane above), at batch 2."""
    g = torch.Generator().manual_seed(9)
    bar = _Bar("gconv3x3 backbone shapes", LOG)
    for cpg, S in ((4, 32), (8, 16), (16, 8), (32, 4)):
        _case(bar, f"cpg{cpg} {S}^2 s1", 2, cpg, 16, S, S, 1, g)
        if cpg > 4:
            _case(bar, f"cpg{cpg} {2 * S}^2 s2", 2, cpg, 16, 2 * S, 2 * S, 2, g)
    bar.done()


def test_gconv3x3_refusals():
    from ivln_ce_amd import ops

    x = torch.randn(1, 8, 4, 4, device=DEV)
    _refused(-5, ops.gconv3x3, x, torch.randn(8, 2, 3, 3, device=DEV), 3)             # C % groups != 0
    _refused(-5, ops.gconv3x3, x, torch.randn(8, 2, 3, 3, device=DEV), 4, stride=3)   # stride 3
    _refused(-5, ops.gconv3x3, x, torch.randn(8, 2, 3, 3, device=DEV), 4, stride=0)
    x = torch.randn(1, 130, 4, 4, device=DEV)
    _refused(-5, ops.gconv3x3, x, torch.randn(130, 65, 3, 3, device=DEV), 2)          # 65 channels per group
    x = torch.randn(2, 8, 4, 4, device=DEV)
    _refused(-5, ops.gconv3x3, x, torch.randn(8, 2, 3, 3, device=DEV), 4, in_img_stride=8 * 16 - 1)  # images overlap
    torch.cuda.synchronize()
