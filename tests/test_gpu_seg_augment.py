"""GPU: the augmentation kernel of csrc/seg_augment.hip alone (include/ivln_seg_augment.h), B = 2 with different records
for the two images, against the numpy restatement tests/seg_augment_ref.py.

labels_a: equal to the twin.  depth_n: the bytes of ops.affine on the depth gathered with the twin's integer indices (0
outside).  rgb_n: kernel_bar's bar against float64, factor 4, with
  e32 = the float32 twin's error MAXIMISED over the size family for the same record (q, offset side, flip, photo), so that a
        1 x 1 case cannot draw a zero bar by luck, and
  mag = (max(1, kv * max(1, ks)) + |dv| / 255) / 0.224: the magnitude the arithmetic rounds at before the normalisation.
Oracles that need no twin: the identity record gives ops.rgb_resize_normalize's and ops.affine's bytes; a flip-only record
gives torch.flip of the identity outputs, byte for byte.  Every figure goes to seg_augment.log before anything is asserted."""
import functools
import itertools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import seg_augment_ref as AR  # noqa: E402
from kernel_bar import _Bar, _log, _same_bytes, _twice  # noqa: E402

DEV = torch.device("cuda:0")
LOG = "seg_augment.log"
IGN = 255
# (H, W) <- (h, w).  W % 4 != 0 (4-byte / 1-byte stores): (1, 1), (3, 5); 16-byte stores: (8, 8), (7, 64); (7, 64): 2 images x
# 112 lanes of four pixels - with (3, 5) <- (2, 3) an up-sampled, with (8, 8) <- (16, 16) a down-sampled rgb frame
SIZES = (((1, 1), (1, 1)), ((3, 5), (3, 5)), ((3, 5), (2, 3)), ((8, 8), (16, 16)), ((7, 64), (7, 64)))
QS = (4096, 4097, 5734, 8192, 2048, 3000)
PHOTOS = ((1.0, 1.0, 0.0), (0.0, 1.0, 0.0), (2.0, 1.5, 40.0), (0.9, 1.1, -25.0), (1.0, 1.0, -300.0))
# a record = (q, offset side: 0 both low / 1 both high, flip, photo); consecutive records share an image pair (B = 2)
RECORDS = tuple(itertools.product(QS, (0, 1), (0, 1), PHOTOS))
IDENT = ((4096, 0, 0, 0), (1.0, 1.0, 0.0, 0.0))


def _inputs(size):
    (H, W), (h, w) = size
    g = np.random.default_rng(1000 * H + 10 * W + h)
    return (g.integers(0, 256, (2, h, w, 3), dtype=np.uint8), g.random((2, H, W), dtype=np.float32) * 3,
            g.integers(0, 13, (2, H, W), dtype=np.uint8))


def _record(size, rec):
    (H, W), _ = size
    q, side, flip, photo = rec
    return (q, AR.offset_range(H, q)[side], AR.offset_range(W, q)[side], flip), tuple(photo) + (0.0,)


@functools.lru_cache(maxsize=None)
def _twins():
    """{(size, record index): (float64 twin, float32 twin)} and {record index: e32 over the size family}; record i always
    runs on image i % 2 of its size's inputs.  Computed once for the module."""
    out, e32 = {}, {}
    for size in SIZES:
        rgb, depth, labels = _inputs(size)
        for i, rec in enumerate(RECORDS):
            geom, photo = _record(size, rec)
            b = i % 2
            r64 = AR.augment_image(rgb[b], depth[b], labels[b], geom, photo, IGN, np.float64)
            r32 = AR.augment_image(rgb[b], depth[b], labels[b], geom, photo, IGN, np.float32)
            assert np.array_equal(r64["labels_a"], r32["labels_a"]) and np.array_equal(r64["depth_src"], r32["depth_src"])
            out[size, i] = (r64, r32)
            e32[i] = max(e32.get(i, 0.0), float(np.abs(r32["rgb_n"].astype(np.float64) - r64["rgb_n"]).max()))
    return out, e32


def _run(size, geom, photo, out=None, ignore=IGN):
    from ivln_ce_amd import ops

    rgb, depth, labels = _inputs(size)
    return ops.seg_augment(torch.from_numpy(rgb).to(DEV), torch.from_numpy(depth).to(DEV), torch.from_numpy(labels).to(DEV),
                           torch.tensor(geom, dtype=torch.int32), torch.tensor(photo, dtype=torch.float32), ignore, out=out)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}_from_{s[1][0]}x{s[1][1]}")
def test_every_record_against_the_twin(size):
    from ivln_ce_amd import ops

    twins, e32 = _twins()
    (H, W), (h, w) = size
    fill = ops.affine(torch.zeros(1, device=DEV), 0.213, 0.285).cpu()
    bad, bar = [], _Bar(f"{H}x{W}<-{h}x{w}", LOG)
    assert len(RECORDS) == 120
    for i in range(0, len(RECORDS), 2):
        recs = [_record(size, RECORDS[i]), _record(size, RECORDS[i + 1])]
        assert recs[0] != recs[1]
        rgb_n, depth_n, labels_a = _run(size, [r[0] for r in recs], [r[1] for r in recs])
        assert tuple(rgb_n.shape) == (2, 3, H, W) and tuple(depth_n.shape) == (2, 1, H, W) and tuple(labels_a.shape) == (2, H, W)
        # depth: ops.affine on the depth gathered with the twin's integer indices
        src = torch.from_numpy(np.stack([twins[size, i + b][0]["depth_src"] for b in range(2)]))
        want_d = ops.affine(src.to(DEV).view(2, 1, H, W), 0.213, 0.285)
        for b in range(2):
            r64, _ = twins[size, i + b]
            q, side, flip, photo = RECORDS[i + b]
            name = f"q{q} o{side} f{flip} p{photo}"
            same_l = np.array_equal(labels_a[b].cpu().numpy(), r64["labels_a"])
            same_d = _same_bytes(depth_n[b], want_d[b])
            outside = torch.from_numpy(~r64["inside"])
            fill_ok = bool((depth_n[b, 0].cpu()[outside].view(torch.int32) == fill.view(torch.int32)).all())
            _log(f"{bar.case:16s} {name:36s} labels {'equal' if same_l else 'DIFFER'}  depth {'equal' if same_d else 'DIFFER'}  "
                 f"outside {int(outside.sum())} fill {'ok' if fill_ok else 'WRONG'}", LOG)
            if not (same_l and same_d and fill_ok):
                bad.append(f"{name}: labels {same_l} depth {same_d} fill {fill_ok}")
            ks, kv, dv = photo
            mag = (max(1.0, kv * max(1.0, ks)) + abs(dv) / 255.0) / 0.224
            r = torch.from_numpy(r64["rgb_n"])
            # (ref32 = ref64 + the family's e32: _Bar.check derives its e32 from the pair it is given)
            bar.case = f"{H}x{W}<-{h}x{w} {name}"
            bar.check("rgb_n", rgb_n[b], r, r + e32[i + b], factor=4.0, mag=mag)
            bar.case = f"{H}x{W}<-{h}x{w}"
            assert r64["inside"].all() == (AR.scaled_size(H, q) >= H and AR.scaled_size(W, q) >= W)
    assert not bad, "\n".join(bad)
    bar.done()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}_from_{s[1][0]}x{s[1][1]}")
def test_identity_and_flip_records_against_the_inference_path(size):
    from ivln_ce_amd import ops

    (H, W), (h, w) = size
    rgb, depth, labels = _inputs(size)
    ident = _twice(lambda: _run(size, [IDENT[0]] * 2, [IDENT[1]] * 2, ignore=None)[:2])
    rgb_i, depth_i, labels_i = _run(size, [IDENT[0]] * 2, [IDENT[1]] * 2, ignore=None)
    assert _same_bytes(rgb_i, ident[0]) and _same_bytes(depth_i, ident[1])
    want_rgb = ops.rgb_resize_normalize(torch.from_numpy(rgb).to(DEV), H, W)
    want_d = ops.affine(torch.from_numpy(depth).to(DEV).view(2, 1, H, W), 0.213, 0.285)
    assert _same_bytes(depth_i, want_d) and torch.equal(labels_i.cpu(), torch.from_numpy(labels))
    d = float((rgb_i - want_rgb).abs().max())
    _log(f"identity {H}x{W}<-{h}x{w}: rgb_n vs rgb_resize_normalize {d:.3e} apart", LOG)
    if (h, w) == (H, W):
        assert _same_bytes(rgb_i, want_rgb), "both forms round u8 / 255 once"
    else:  # (another order of the same interpolation: within the bar against float64)
        r64 = np.stack([AR.augment_image(rgb[b], depth[b], labels[b], *IDENT, None, np.float64)["rgb_n"] for b in range(2)])
        r32 = np.stack([AR.augment_image(rgb[b], depth[b], labels[b], *IDENT, None, np.float32)["rgb_n"] for b in range(2)])
        bar = _Bar(f"identity {H}x{W}<-{h}x{w}", LOG)
        _, limit = bar.check("rgb_n", rgb_i, torch.from_numpy(r64), torch.from_numpy(r32), factor=4.0, mag=1.0 / 0.224)
        bar.within("vs_resize", rgb_i, want_rgb, limit)
        bar.done()
    # flip only, in one image and in both: torch.flip of the identity outputs, byte for byte
    flip = ((4096, 0, 0, 1), IDENT[1])
    rgb_f, depth_f, labels_f = _run(size, [flip[0], IDENT[0]], [flip[1], IDENT[1]], ignore=None)
    assert _same_bytes(rgb_f[0], torch.flip(rgb_i[0], dims=[-1])) and _same_bytes(rgb_f[1], rgb_i[1])
    assert _same_bytes(depth_f[0], torch.flip(depth_i[0], dims=[-1])) and _same_bytes(depth_f[1], depth_i[1])
    assert torch.equal(labels_f[0], torch.flip(labels_i[0], dims=[-1])) and torch.equal(labels_f[1], labels_i[1])
    rgb_f, depth_f, labels_f = _run(size, [flip[0]] * 2, [flip[1]] * 2, ignore=None)
    assert _same_bytes(rgb_f, torch.flip(rgb_i, dims=[-1])) and _same_bytes(depth_f, torch.flip(depth_i, dims=[-1]))
    assert torch.equal(labels_f, torch.flip(labels_i, dims=[-1]))


@pytest.mark.parametrize("shift", [0, 1])  # (1: outputs off their 16-byte / 4-byte alignment - the narrow stores at W % 4 == 0)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}_from_{s[1][0]}x{s[1][1]}")
def test_nothing_is_written_around_the_outputs_and_two_runs_agree(size, shift):
    (H, W), _ = size
    recs = [_record(size, (5734, 1, 1, PHOTOS[3])), _record(size, (3000, 0, 0, PHOTOS[2]))]
    geom, photo = [r[0] for r in recs], [r[1] for r in recs]
    GUARD = 64

    def fresh():
        bufs, views = [], []
        for shape, dtype, mark in (((2, 3, H, W), torch.float32, -7.0), ((2, 1, H, W), torch.float32, -7.0), ((2, H, W), torch.uint8, 77)):
            n = int(np.prod(shape))
            buf = torch.full((GUARD + shift + n + GUARD,), mark, dtype=dtype, device=DEV)
            bufs.append((buf, n, mark))
            views.append(buf[GUARD + shift:GUARD + shift + n].view(shape))
        return bufs, tuple(views)

    def run():
        bufs, views = fresh()
        _run(size, geom, photo, out=views)
        for buf, n, mark in bufs:
            assert bool((buf[:GUARD + shift] == mark).all()) and bool((buf[GUARD + shift + n:] == mark).all()), "guard overwritten"
        return tuple(v.clone() for v in views)

    a = _twice(lambda: run()[:2])
    free = _run(size, geom, photo)  # (fresh, aligned outputs: the same values whichever stores wrote them)
    mine = run()
    assert _same_bytes(mine[0], a[0]) and _same_bytes(mine[0], free[0]) and _same_bytes(mine[1], free[1])
    assert torch.equal(mine[2], free[2])
    assert bool((free[2] == IGN).any()) == (AR.scaled_size(H, 3000) < H), "the q = 3000 image pads (a 1 x 1 frame cannot)"


def test_a_bad_record_is_refused_with_gpu_operands_too():
    from kernel_bar import _refused

    size = SIZES[4]
    _refused(-1, _run, size, [IDENT[0], (4096, 1, 0, 0)], [IDENT[1]] * 2)
    _refused(-1, _run, size, [IDENT[0], (3000, 0, 0, 0)], [IDENT[1]] * 2, ignore=None)
    _refused(-1, _run, size, [IDENT[0]] * 2, [IDENT[1], (1.0, float("nan"), 0.0, 0.0)])
