"""GPU: the segmentation kernels of csrc/seg_loss.hip alone (include/ivln_seg_train.h).

Pixel cross-entropy: reference = torch's own F.cross_entropy(weight=, ignore_index=, reduction="mean") in float64 on the
labels down-sampled by nearest neighbour (labels[:, ::s, ::s] - what F.interpolate(mode="nearest") picks for an integer
factor), its gradient by float64 autograd times the scale.  Bar for the loss and for dscores: 4 x the error of torch's fp32
F.cross_entropy on the same inputs against float64 + 1e-7 * max|ref| (the kernel computes in double and rounds once to f32:
half an f32 ulp, 6e-8 relative).  Every figure goes to the suite's log directory before it is asserted.
Confusion counts: equal to numpy.bincount exactly."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from kernel_bar import _log  # noqa: E402

DEV = torch.device("cuda:0")
LOG = "seg_loss.log"
IGN = 255
SIZES = ((1, 1), (3, 5), (8, 8), (7, 64))  # h * w % 4 != 0 (4-byte accesses): (1, 1), (3, 5); several workgroups: (7, 64)
STRIDES = (1, 2, 16)


def _case(C, h, w, s, amp, weights, ignore, seed, N=2):
    g = torch.Generator().manual_seed(seed)
    scores = (torch.rand(N, C, h, w, generator=g) * 2 - 1) * amp
    labels = torch.randint(0, C, (N, h * s, w * s), generator=g, dtype=torch.int64).to(torch.uint8)
    if ignore:
        labels[torch.rand(labels.shape, generator=g) < 0.25] = IGN
    labels[0, 0, 0] = C - 1  # (a labelled pixel of a class with weight > 0: the mean has a denominator)
    wt = None
    if weights:
        wt = torch.rand(C, generator=g) + 0.5
        wt[0] = 0.0
    return scores, labels, wt


def _torch_ce(scores, labels, s, wt, ignore, scale, dtype):
    x = scores.to(dtype).requires_grad_(True)
    tgt = labels[:, ::s, ::s].long()
    loss = F.cross_entropy(x, tgt, weight=None if wt is None else wt.to(dtype), ignore_index=IGN if ignore else -100,
                           reduction="mean")
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), g * scale


def _bar(name, got, r64, r32, bad):
    err = float((got.detach().cpu().double() - r64).abs().max())
    e32 = float((r32.double() - r64).abs().max())
    mx = float(r64.abs().max())
    bar = 4 * e32 + 1e-7 * mx
    ok = err <= bar
    _log(f"{name:58s} hip {err:.3e}  torch-fp32 {e32:.3e}  max|ref| {mx:.3e}  bar {bar:.3e}  {'ok' if ok else 'OVER'}", LOG)
    if not ok:
        bad.append(f"{name}: {err:.3e} > {bar:.3e}")


@pytest.mark.parametrize("amp", [10.0, 80.0])  # (+-80: exp overflows f32 without the max subtraction)
@pytest.mark.parametrize("C", [13, 2])
def test_pixel_ce_loss_and_gradient_against_float64_cross_entropy(C, amp):
    from ivln_ce_amd import ops

    bad, n = [], 0
    for (h, w), s, weights, ignore in itertools.product(SIZES, STRIDES, (False, True), (False, True)):
        scores, labels, wt = _case(C, h, w, s, amp, weights, ignore, seed=100 * h + w + s)
        scale = 0.4 if weights else 1.0
        loss, d = ops.seg_ce(scores.to(DEV), labels.to(DEV), s, None if wt is None else wt.to(DEV), IGN if ignore else None,
                             scale=scale)
        l64, g64 = _torch_ce(scores, labels, s, wt, ignore, scale, torch.float64)
        l32, g32 = _torch_ce(scores, labels, s, wt, ignore, scale, torch.float32)
        name = f"C{C} amp{amp:g} {h}x{w} s{s} w{int(weights)} ign{int(ignore)}"
        _bar(name + " loss", loss.reshape(()), l64, l32, bad)
        _bar(name + " dscores", d, g64, g32, bad)
        assert tuple(d.shape) == tuple(scores.shape)
        if ignore:
            gone = (labels[:, ::s, ::s] == IGN).unsqueeze(1).expand_as(scores)
            assert float(d.cpu()[gone].abs().max()) == 0.0 if gone.any() else True
        n += 1
    assert n == 48
    assert not bad, "\n".join(bad)


def test_pixel_ce_every_pixel_ignored_gives_zero_loss_and_zero_gradient():
    from ivln_ce_amd import ops

    for (h, w), s in itertools.product(SIZES, (1, 2)):
        scores = torch.randn(2, 13, h, w, generator=torch.Generator().manual_seed(h))
        labels = torch.full((2, h * s, w * s), IGN, dtype=torch.uint8)
        loss, d = ops.seg_ce(scores.to(DEV), labels.to(DEV), s, None, IGN, scale=1.0,
                             loss=torch.full((1,), 7.0, device=DEV), dscores=torch.full(scores.shape, 7.0, device=DEV))
        assert float(loss) == 0.0 and float(d.abs().max()) == 0.0, (h, w, s)
    # ... and so does a call whose only labelled pixels carry weight 0 (torch: 0 / 0)
    wt = torch.ones(13)
    wt[3] = 0.0
    labels = torch.full((2, 8, 8), 3, dtype=torch.uint8)
    loss, d = ops.seg_ce(torch.randn(2, 13, 8, 8).to(DEV), labels.to(DEV), 1, wt.to(DEV), IGN)
    assert float(loss) == 0.0 and float(d.abs().max()) == 0.0


def test_pixel_ce_two_runs_give_the_same_bytes():
    from ivln_ce_amd import ops

    for (h, w), s in (((7, 64), 2), ((3, 5), 1), ((64, 64), 1)):
        scores, labels, wt = _case(13, h, w, s, 10.0, True, True, seed=5, N=4)
        runs = []
        for _ in range(2):
            loss, d = ops.seg_ce(scores.to(DEV), labels.to(DEV), s, wt.to(DEV), IGN, scale=0.7)
            runs.append((loss.cpu().view(torch.int32), d.cpu().view(torch.int32)))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), (h, w, s)


@pytest.mark.parametrize("h,w,s", [(3, 5, 2), (8, 8, 1)])
def test_pixel_ce_refuses_an_out_of_range_label_and_writes_nothing(h, w, s):
    from ivln_ce_amd import ops
    from ivln_ce_amd._lib import IvlnError

    scores, labels, _ = _case(13, h, w, s, 10.0, False, True, seed=9)
    good = labels.clone()
    labels[1, (h - 1) * s, (w - 1) * s] = 13  # (a sampled pixel: neither a class nor the ignore label)
    loss = torch.full((1,), 7.0, device=DEV)
    d = torch.full(scores.shape, 7.0, device=DEV)
    with pytest.raises(IvlnError):
        ops.seg_ce(scores.to(DEV), labels.to(DEV), s, None, IGN, loss=loss, dscores=d)
    assert float(loss) == 7.0 and bool((d == 7.0).all()), "a refused call leaves its outputs alone"
    # an unsampled pixel may hold anything, and the refusal does not stick to the next call
    if s > 1:
        good[0, 1, 1] = 200
    loss, d = ops.seg_ce(scores.to(DEV), good.to(DEV), s, None, IGN, loss=loss, dscores=d)
    l64, _ = _torch_ce(scores, good, s, None, True, 1.0, torch.float64)
    assert abs(float(loss) - float(l64)) <= 1e-6 * abs(float(l64)) and bool((d != 7.0).all())


def test_pixel_ce_refuses_shapes_it_cannot_take():
    from ivln_ce_amd import ops
    from ivln_ce_amd._lib import IvlnError

    scores = torch.zeros(2, 13, 4, 4, device=DEV)
    with pytest.raises(IvlnError):
        ops.seg_ce(scores, torch.zeros(2, 8, 7, dtype=torch.uint8, device=DEV), 2)
    with pytest.raises(IvlnError):
        ops.seg_ce(torch.zeros(2, 65, 4, 4, device=DEV), torch.zeros(2, 4, 4, dtype=torch.uint8, device=DEV), 1)
    with pytest.raises(IvlnError):
        ops.seg_ce(torch.zeros(2, 1, 4, 4, device=DEV), torch.zeros(2, 4, 4, dtype=torch.uint8, device=DEV), 1)


@pytest.mark.parametrize("n", [2 * 37 * 53, 5, 300001])  # (no multiple of the 256-lane workgroup; more than one workgroup)
def test_confusion_counts_equal_bincount(n):
    from ivln_ce_amd import ops
    from ivln_ce_amd.rednet_train import metrics_from_counts

    C = 13
    g = torch.Generator().manual_seed(n)
    pred = torch.randint(0, C, (n,), generator=g).to(torch.uint8)
    truth = torch.randint(0, C, (n,), generator=g).to(torch.uint8)
    truth[torch.rand(n, generator=g) < 0.2] = IGN
    truth[0] = 4
    counts = ops.seg_confusion(pred.to(DEV), truth.to(DEV), C, IGN)
    keep = truth.numpy() != IGN
    ref = np.bincount(truth.numpy()[keep].astype(np.int64) * C + pred.numpy()[keep], minlength=C * C).reshape(C, C)
    assert counts.dtype == torch.int64 and np.array_equal(counts.cpu().numpy(), ref)
    again = ops.seg_confusion(pred.to(DEV), truth.to(DEV), C, IGN, counts=counts)  # accumulates
    assert again is counts and np.array_equal(counts.cpu().numpy(), 2 * ref)
    none = ops.seg_confusion(pred.to(DEV), truth.clamp(max=C - 1).to(DEV), C, None)
    t2 = truth.clamp(max=C - 1).numpy().astype(np.int64)
    assert np.array_equal(none.cpu().numpy(), np.bincount(t2 * C + pred.numpy(), minlength=C * C).reshape(C, C))
    m = metrics_from_counts(torch.from_numpy(ref))
    tp = np.diag(ref).astype(np.float64)
    assert m["pixel_acc"] == pytest.approx(tp.sum() / ref.sum())
    union = ref.sum(0) + ref.sum(1) - tp  # (a class that neither occurs nor is predicted has no IoU: nan, left out of the mean)
    assert np.allclose(m["iou"][union > 0], tp[union > 0] / union[union > 0]) and np.isnan(m["iou"][union == 0]).all()
    assert m["miou"] == pytest.approx(float(np.mean(tp[union > 0] / union[union > 0])))


def test_confusion_counts_refuse_a_label_that_is_no_class():
    from ivln_ce_amd import ops
    from ivln_ce_amd._lib import IvlnError

    pred = torch.zeros(100, dtype=torch.uint8, device=DEV)
    truth = torch.zeros(100, dtype=torch.uint8, device=DEV)
    truth[7] = 13
    with pytest.raises(IvlnError):
        ops.seg_confusion(pred, truth, 13, IGN)
