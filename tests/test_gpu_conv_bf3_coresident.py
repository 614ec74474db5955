"""The four-wave (co-resident) instantiations of the two K-split kernels of csrc/conv_bf3.hip - k_conv_bf3_ks<.., NW = 4> (3x3 on
64-pixel tiles of 8-, 16- and 32-wide maps, the stacked 2 x 2 transposed form) and k_conv1x1_bf3_ks<false, 4> - each alone
behind ivln_gemm_f32, pinned by tile_override 17 / 19, against the same operation in torch float64 on the CPU.  The launch,
the inputs (`dense` and `single_tap`), the NaN / sentinel-banded destinations and the references are those of
tests/test_gpu_conv_bf3_kernels.py, imported, with this file's own case table; the bar is _Bar.check of tests/kernel_bar.py,
unchanged: 4 * e32 + 4 * 2^-24 * max|float64|.  Every comparison goes to conv_bf3_coresident.log before anything is asserted.

Every case also runs its eight-wave pin (16 / 18): both wave counts are held to the same bar; they need not equal each other
(four partial tiles of longer K slices against eight).  Observed per launch: the kernel name (family timing sink), the delta
of ivln_conv_split_kinds (the form index does not depend on the wave count), the delta of ivln_conv_ks_waves (the wave count
that ran), splits_used = 1, the same bytes on a second run.  A refusal of a pinned case raises out of ops.gemm: a failure.

Shapes: the smallest that reach every edge of the four-wave code -
  3x3: 3 images, two tile rows, M = 40 (a second, masked channel tile); Cin = 128 (8 chunks, two per wave) and 144 (9 chunks:
       slices 3, 3, 3, 0 - the empty wave must bring zeros to the reduction); forms `plain` and `full`; one image-grouped case
       (4 images, 2 weight sets) equal bit for bit to one pinned four-wave launch per set;
  2x2: the stacked transposed form at width 16, Cin = 128, rows M = 40, the 2 x 2-block store epilogue (two passes of 256 threads);
  1x1: M = 40; Cin = 80 (5 chunks: slices 2, 2, 1, 0) and 512 (32 chunks); 3 images of 4 x 8 pixels (a partial 128-pixel tile);
       2 images of 8 x 16 pixels as two weight sets; forms plain, full, the residual behind the ReLU, accumulate, and the
       2 x 2-block store (`up`) form - four passes of 256 threads over the 1024 epilogue items.

Measured on an MI355X (256 CUs; 16 tests, 112 comparisons, none OVER, 1.4 s for the file): the largest hip / e32 ratio is 2.37
for both wave counts (`single_tap`, where e32 is one fp32 rounding of one product); on the image-grouped 3x3 case `dense`
`plain` the four-wave sum is 1.27e-06 from float64 and the eight-wave sum 9.4e-07, bar 5.5e-06."""
import ctypes as C

import pytest
import torch

import test_gpu_conv_bf3_kernels as K
from kernel_bar import _Bar, _same_bytes, _twice

pytestmark = pytest.mark.gpu
LOG = "conv_bf3_coresident.log"
# tile_override pins: (eight waves, four waves) and the counter of ivln_conv_ks_waves each lands in
PINS3, PINS1 = (16, 17), (18, 19)
WAVES_IDX = {16: 0, 17: 1, 18: 2, 19: 3}
KIND_IDX = {16: 1, 17: 1, 18: 2, 19: 2}   # ivln_conv_split_kinds: 3x3 K-split | 1x1 K-split

_X1 = dict(KS=1, imgs=3, Cin=80, H=4, W=8, M=40)
CASES = (
    [dict(tag="co3-w%d-c%d" % (W, cin), KS=3, imgs=3, Cin=cin, H=2 * (64 // W), W=W, M=40) for W in (8, 16, 32) for cin in (128, 144)] +
    [dict(tag="co3-w8-grp", KS=3, imgs=4, Cin=128, H=8, W=8, M=40, grp=2),
     dict(tag="co2-w16", KS=2, imgs=3, Cin=128, H=8, W=16, M=40),
     dict(_X1, tag="co1-c80"),
     dict(_X1, tag="co1-c512", Cin=512),
     dict(_X1, tag="co1-grp", imgs=2, H=8, W=16, grp=1),
     dict(_X1, tag="co1-post", post=True),
     dict(_X1, tag="co1-acc", acc=True),
     dict(_X1, tag="co1-up", up=True)]
)
_BY_TAG = {c["tag"]: c for c in CASES}
_REFS = {}


def _pins(c):
    return PINS1 if c["KS"] == 1 else PINS3


def _refs(c, which, form):
    """float64 and fp32 references of (case, input set, form): computed once, shared by both wave counts"""
    key = (c["tag"], which, form)
    if key not in _REFS:
        _REFS[key] = (K._reference(c, which, form, torch.float64), K._reference(c, which, form, torch.float32))
    return _REFS[key]


def _waves():
    from ivln_ce_amd import ops

    L = ops._L()
    L.ivln_conv_ks_waves.argtypes = [C.POINTER(C.c_longlong), C.c_int]
    out = (C.c_longlong * 4)()
    assert L.ivln_conv_ks_waves(out, 0) == 0
    return list(out)


def _run(c, ov, which, form, bar=None, **kw):
    """the case pinned to tile_override `ov`, twice under the timing sink; tallies and kernel name asserted; -> the output"""
    cc = dict(c, ov=ov)
    res = []
    kinds0, waves0 = K._kinds(), _waves()

    def once():
        r = K._launch(cc, which, form, **kw)
        res.append(r)
        return (r["out"],)

    outs, ran = K._observed(lambda: _twice(once))
    name = "k_conv1x1_bf3_ks" if c["KS"] == 1 else "k_conv_bf3_ks"
    assert ran == {name: 2}, (c["tag"], ov, ran)
    dk = [a - b for a, b in zip(K._kinds(), kinds0)]
    dw = [a - b for a, b in zip(_waves(), waves0)]
    assert dk == [2 if i == KIND_IDX[ov] else 0 for i in range(4)], (c["tag"], ov, dk)
    assert dw == [2 if i == WAVES_IDX[ov] else 0 for i in range(4)], (c["tag"], ov, dw)
    assert res[0]["splits_used"] == 1, (c["tag"], ov, res[0]["splits_used"])
    if bar is not None:
        r64, r32 = _refs(c, which, form)
        bar.check(f"{which[:5]} {form[:5]} nw{4 if ov in (17, 19) else 8}", outs[0], r64, r32)
    return outs[0]


@pytest.mark.parametrize("tag", [c["tag"] for c in CASES])
def test_four_wave_form_against_float64(tag):
    """both wave counts, both input sets, both epilogue forms: each within the bar of its float64 reference"""
    c = _BY_TAG[tag]
    bar = _Bar(tag, LOG)
    for which in K.SETS:
        for form in K.P.FORMS:
            for ov in _pins(c):
                _run(c, ov, which, form, bar)
    bar.done()


@pytest.mark.parametrize("tag", ["co3-w8-grp", "co1-grp"])
def test_four_wave_grouped_weights_equal_one_launch_per_set(tag):
    """image-grouped weights == one pinned four-wave launch per weight set, bit for bit"""
    c = _BY_TAG[tag]
    ov = _pins(c)[1]
    per = c["grp"]
    for form in K.P.FORMS:
        whole = _run(c, ov, "dense", form)
        for gi in range(c["imgs"] // per):
            part = _run(c, ov, "dense", form, only_group=gi)
            assert _same_bytes(whole[gi * per:(gi + 1) * per], part), (tag, form, gi)
