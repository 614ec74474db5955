"""GPU: the class statistics of csrc/seg_augment.hip alone (ivln_seg_class_counts_u8, include/ivln_seg_augment.h) against
numpy: pixels[c] = the pixels of class c, present[c] = the labelled pixels of the images in which c occurs.  Integers: equal."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from kernel_bar import _log  # noqa: E402

DEV = torch.device("cuda:0")
LOG = "seg_class_counts.log"
IGN = 255


def _labels(B, hw, C, ignore, seed):
    g = np.random.default_rng(seed)
    lab = g.integers(0, C, (B, hw), dtype=np.uint8)
    for b in range(B):  # every image misses some classes of its own, so `present` differs from class to class
        gone = g.integers(0, C, size=max(1, C // 3))
        lab[b][np.isin(lab[b], gone)] = g.integers(0, C)
    if ignore:
        lab[g.random((B, hw)) < 0.25] = IGN
    return lab


def _numpy_counts(lab, C, ignore):
    pixels, present = np.zeros(C, dtype=np.int64), np.zeros(C, dtype=np.int64)
    for img in lab:
        kept = img[img != IGN] if ignore else img
        h = np.bincount(kept.astype(np.int64), minlength=C)[:C]
        pixels += h
        present[h > 0] += int(h.sum())
    return pixels, present


def test_both_vectors_equal_numpy_and_accumulate_across_calls():
    from ivln_ce_amd import ops

    n = 0
    for hw, C, ignore in itertools.product((1, 15, 64, 448), (2, 13, 64), (False, True)):
        a, b = _labels(3, hw, C, ignore, seed=hw + C), _labels(2, hw, C, ignore, seed=hw + C + 1)
        pa, ra = _numpy_counts(a, C, ignore)
        pb, rb = _numpy_counts(b, C, ignore)
        pixels, present = ops.seg_class_counts(torch.from_numpy(a).to(DEV), C, IGN if ignore else None)
        ok1 = np.array_equal(pixels.cpu().numpy(), pa) and np.array_equal(present.cpu().numpy(), ra)
        p2, r2 = ops.seg_class_counts(torch.from_numpy(b).to(DEV), C, IGN if ignore else None, pixels, present)
        ok2 = p2 is pixels and r2 is present and np.array_equal(pixels.cpu().numpy(), pa + pb) and np.array_equal(present.cpu().numpy(), ra + rb)
        _log(f"hw {hw:4d} C {C:2d} ignore {int(ignore)}: pixels {int(pa.sum())} present {int(ra.sum())}  first call "
             f"{'equal' if ok1 else 'DIFFER'}  accumulated {'equal' if ok2 else 'DIFFER'}", LOG)
        assert pixels.dtype == present.dtype == torch.int64 and ok1 and ok2, (hw, C, ignore)
        assert int(pa.sum()) == int((a != IGN).sum() if ignore else a.size)
        n += 1
    assert n == 24


def test_the_batch_form_takes_observations_and_gives_the_weights_numpy_gives():
    from ivln_ce_amd.rednet_train import class_counts, median_frequency_weights

    C = 13
    batches = [_labels(2, 8 * 8, C, True, seed=s).reshape(2, 8, 8, 1) for s in (1, 2, 3)]
    pixels, present = class_counts([{"semantic12": torch.from_numpy(b).to(DEV)} for b in batches], C, IGN)
    px, pr = _numpy_counts(np.concatenate(batches).reshape(6, 64), C, True)
    assert pixels.device.type == "cpu" and np.array_equal(pixels.numpy(), px) and np.array_equal(present.numpy(), pr)
    w = median_frequency_weights(pixels, present)
    freq = px[px > 0] / pr[px > 0]
    want = np.ones(C)
    want[px > 0] = np.median(freq) / freq
    assert np.array_equal(w.numpy(), want.astype(np.float32))


@pytest.mark.parametrize("hw", [15, 448])
def test_an_out_of_range_label_sets_the_error_word_and_changes_neither_vector(hw):
    from ivln_ce_amd import ops
    from ivln_ce_amd._lib import IvlnError

    C = 13
    lab = _labels(3, hw, C, True, seed=7)
    good = torch.from_numpy(lab.copy()).to(DEV)
    lab[2, hw - 1] = C  # (the last pixel of the last image: neither a class nor the ignore label)
    pixels = torch.full((C,), 5, dtype=torch.int64, device=DEV)
    present = torch.full((C,), 9, dtype=torch.int64, device=DEV)
    with pytest.raises(IvlnError):
        ops.seg_class_counts(torch.from_numpy(lab).to(DEV), C, IGN, pixels, present)
    assert bool((pixels == 5).all()) and bool((present == 9).all()), "a refused call leaves both vectors alone"
    # seg_check cleared the word: the next call counts
    px, pr = _numpy_counts(good.cpu().numpy(), C, True)
    ops.seg_class_counts(good, C, IGN, pixels, present)
    assert np.array_equal(pixels.cpu().numpy(), px + 5) and np.array_equal(present.cpu().numpy(), pr + 9)
    # without the read-back the word stays set until seg_check raises and clears it
    ops.seg_class_counts(torch.from_numpy(lab).to(DEV), C, IGN, pixels, present, check_labels=False)
    with pytest.raises(IvlnError):
        ops.seg_check(DEV, "test")
    ops.seg_check(DEV, "test")
    assert np.array_equal(pixels.cpu().numpy(), px + 5)
    # with no ignore label, 255 is out of range as well
    with pytest.raises(IvlnError):
        ops.seg_class_counts(torch.full((1, hw), 255, dtype=torch.uint8, device=DEV), C, None)
