"""GPU: the front kernels of the instruction encoder over pre-computed text features alone (csrc/text_feat.hip,
include/ivln_text_feat.h).  ivln_text_feat_front_f32: lengths exact against numpy - the NUMBER of rows with an element
!= 0 (instruction_encoder.py:77-78) - and the per-episode cache's contract (bitwise compare, clean rows keep their bytes, the
scratch re-arms itself).  ivln_text_feat_gates_f32: the W_ih projection against float64 under kernel_bar's rule, flagged
rows only."""
import numpy as np
import pytest
import torch

from kernel_bar import _Bar, _refused, _same_bytes, _twice

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOG = "text_feat_kernels.log"
SHAPES = [(3, 1, 1), (3, 5, 3), (2, 17, 65), (3, 64, 64), (2, 512, 768)]


def _np_lengths(x):
    a = x.detach().cpu().numpy()
    return ((a != 0).sum(2) != 0).sum(1).astype(np.int32)


def _features(B, L, E, seed=0):
    """random features with a zero tail of another length per sequence and a zero row in the middle of sequence 0"""
    g = torch.Generator().manual_seed(seed + 1000 * B + 10 * L + E)
    x = torch.randn(B, L, E, generator=g)
    for b in range(B):
        x[b, max(1, L - (b * L) // (B + 1)):] = 0
    if L >= 3:
        x[0, 1] = 0
    return x


def _cache(B, L, E):
    from ivln_ce_amd import ops

    return ops.InstructionStepCache(B, L, 4, 128, torch.device(DEV), key=None, ndir=1, feat=E)


@pytest.mark.parametrize("B,L,E", SHAPES)
def test_lengths_are_exact_row_counts(B, L, E):
    from ivln_ce_amd import ops

    x = _features(B, L, E)
    got = _twice(lambda: (ops.text_feat_front(x.to(DEV)),))[0]
    assert got.dtype == torch.int32 and got.cpu().numpy().tolist() == _np_lengths(x).tolist()
    if L >= 3:
        assert int(got[0]) == L - 1 and bool((x[0, 2] != 0).any())  # (the zero row in the middle shortened the count)


def test_scalar_path_on_a_four_byte_aligned_view():
    from ivln_ce_amd import ops

    B, L, E = 2, 9, 8
    flat = torch.zeros(B * L * E + 1, device=DEV)
    x = _features(B, L, E, seed=3)
    view = flat[1:].view(B, L, E)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    assert ops.text_feat_front(view).cpu().numpy().tolist() == _np_lengths(x).tolist()
    cache = _cache(B, L, E)
    ops.text_feat_front(view, cache=cache)
    assert cache.dirty.tolist() == [1, 1] and _same_bytes(cache.cache_feat, view)
    ops.text_feat_front(view, cache=cache)
    assert cache.dirty.tolist() == [0, 0]


def test_negative_zero_nan_and_empty_sequences():
    from ivln_ce_amd import ops

    B, L, E = 4, 6, 12
    x = torch.zeros(B, L, E)
    x[0, :3] = -0.0          # rows of -0.0 are zero rows
    x[0, 4, 5] = 2.0         # ... one real row: count 1
    x[1, 2, 7] = float("nan")  # a NaN element is non-zero: count 1
    x[2, 0, 0] = 1e-42       # (a denormal is not zero either, as in numpy)
    x[2, 1] = 1.0
    x[2, 3] = -1.0           # rows 0, 1, 3 with a zero row between: count 3
    got = ops.text_feat_front(x.to(DEV)).cpu().numpy().tolist()
    assert got == [1, 1, 3, 0] == _np_lengths(x).tolist()
    # an all-zero sequence downstream, as on the token path: the recurrence leaves exact zeros for it
    gx = torch.randn(B * L, 512, device=DEV)
    whh, bhh = torch.randn(512, 128, device=DEV) * 0.05, torch.zeros(512, device=DEV)
    out, _, _ = ops.lstm_bidir(gx, None, whh, None, bhh, None, torch.tensor(got, dtype=torch.int32, device=DEV), B, L, 128, ndir=1)
    assert bool((out[3] == 0).all()) and bool((out[0, :, 1:] == 0).all()) and bool((out[0, :, 0] != 0).any())


@pytest.mark.parametrize("B,L,E", [(3, 5, 3), (3, 64, 64), (2, 512, 768)])
def test_cache_contract(B, L, E):
    from ivln_ce_amd import ops

    x = _features(B, L, E, seed=1).to(DEV)
    want = torch.from_numpy(_np_lengths(x))
    cache = _cache(B, L, E)
    assert ops.text_feat_front(x, cache=cache) is cache.lengths
    assert cache.dirty.tolist() == [1] * B and cache.valid.tolist() == [1] * B
    assert _same_bytes(cache.cache_feat, x) and torch.equal(cache.lengths.cpu(), want)
    assert not bool(cache.ws.any())  # (the scratch re-armed itself)
    # the same input again: nothing dirty, clean rows are not rewritten
    cache.lengths.fill_(-7)
    before = cache.cache_feat.clone()
    ops.text_feat_front(x, cache=cache)
    assert cache.dirty.tolist() == [0] * B and cache.lengths.tolist() == [-7] * B and _same_bytes(cache.cache_feat, before)
    cache.lengths.copy_(want)
    # one word changed in the last element of the last row of one sequence, then in the first
    for b, (t, e) in ((B - 1, (L - 1, E - 1)), (0, (0, 0))):
        y = x.clone()
        y[b, t, e] = 3.5
        cache.lengths.fill_(-7)
        ops.text_feat_front(y, cache=cache)
        assert cache.dirty.tolist() == [int(i == b) for i in range(B)]
        assert _same_bytes(cache.cache_feat, y)
        lens_y = _np_lengths(y).tolist()
        assert cache.lengths.tolist() == [lens_y[i] if i == b else -7 for i in range(B)]
        x = y
    # 0.0 -> -0.0: the compare is bitwise (the count does not move)
    z = x.clone()
    z[1, L - 1, 0] = 0.0
    ops.text_feat_front(z, cache=cache)
    z2 = z.clone()
    z2[1, L - 1, 0] = -0.0
    ops.text_feat_front(z2, cache=cache)
    assert cache.dirty.tolist() == [int(i == 1) for i in range(B)] and _same_bytes(cache.cache_feat, z2)
    # after invalidate(): all dirty, through ops.invalidate_step_caches as FlatAdam.step reaches it
    ops.invalidate_step_caches()
    assert cache.valid.tolist() == [0] * B
    ops.text_feat_front(z2, cache=cache)
    assert cache.dirty.tolist() == [1] * B and cache.valid.tolist() == [1] * B
    assert cache.lengths.cpu().numpy().tolist() == _np_lengths(z2).tolist()
    assert not bool(cache.ws.any())


def test_two_runs_give_identical_bytes():
    from ivln_ce_amd import ops

    B, L, E = 2, 512, 768
    x = _features(B, L, E, seed=2).to(DEV)

    def run():
        cache = _cache(B, L, E)
        ops.text_feat_front(x, cache=cache)
        return cache.lengths.float(), cache.dirty.float(), cache.cache_feat, cache.valid.float()

    _twice(run)


def test_refusals():
    from ivln_ce_amd import ops

    x = torch.zeros(2, 3, 4, device=DEV)
    cache = _cache(2, 3, 4)
    T = ops._TF()
    ws, ln = cache.ws.data_ptr(), cache.lengths.data_ptr()

    def front(*a):
        ops.check(T.ivln_text_feat_front_f32(*a), "ivln_text_feat_front_f32")

    _refused(-1, front, None, 2, 3, 4, ln, None, None, None, ws, None)
    _refused(-1, front, x.data_ptr(), 0, 3, 4, ln, None, None, None, ws, None)
    _refused(-1, front, x.data_ptr(), 2, -1, 4, ln, None, None, None, ws, None)
    _refused(-1, front, x.data_ptr(), 2, 3, 0, ln, None, None, None, ws, None)
    _refused(-1, front, x.data_ptr(), 2, 3, 4, None, None, None, None, ws, None)
    _refused(-1, front, x.data_ptr(), 2, 3, 4, ln, None, None, None, None, None)
    _refused(-1, front, x.data_ptr(), 2, 3, 4, ln, cache.cache_feat.data_ptr(), None, cache.dirty.data_ptr(), ws, None)
    _refused(-1, front, x.data_ptr(), 2, 3, 4, ln, None, cache.valid.data_ptr(), None, ws, None)

    def gates(*a):
        ops.check(T.ivln_text_feat_gates_f32(*a), "ivln_text_feat_gates_f32")

    w = torch.zeros(8, 4, device=DEV)
    out = torch.zeros(6, 8, device=DEV)
    _refused(-1, gates, None, 2, 3, 4, w.data_ptr(), None, 8, None, out.data_ptr(), None)
    _refused(-1, gates, x.data_ptr(), 2, 3, 4, None, None, 8, None, out.data_ptr(), None)
    _refused(-1, gates, x.data_ptr(), 2, 3, 4, w.data_ptr(), None, 0, None, out.data_ptr(), None)
    _refused(-1, gates, x.data_ptr(), 2, 3, 4, w.data_ptr(), None, 8, None, None, None)
    with pytest.raises(ops._lib.IvlnError):
        ops.text_feat_front(x, cache=_cache(2, 3, 8))  # a cache of another feature width


# ------------------------------------------------------------------------------------------------------------------
# the gate projection
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,E,G", [(3, 6, 8, 512), (2, 5, 3, 6), (3, 17, 65, 384), (5, 64, 64, 70), (3, 6, 8, 68),
                                     (2, 512, 768, 512)])
def test_gate_projection_against_float64(B, L, E, G):
    """gx = feat . W^T + b: float64 torch is the reference, torch's fp32 addmm its e32 (kernel_bar's rule, factor 4: another
    summation order than torch's).  Sizes: E below / not a multiple of the 32-deep K slice and of 4 (scalar loads), G not
    a multiple of the 64-row tile or of 4 (scalar stores), G = 68 (16-byte stores with a partial last tile: the `m >= G`
    guard), more rows than one tile, the RxR shape."""
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(B * 100 + E)
    x = torch.randn(B, L, E, generator=g)
    w = torch.randn(G, E, generator=g) / E ** 0.5
    b = torch.randn(G, generator=g) * 0.1
    r64 = x.double().view(B * L, E) @ w.double().t() + b.double()
    r32 = torch.addmm(b, x.view(B * L, E), w.t())
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    got = _twice(lambda: (ops.text_feat_gates(xd, wd, bd),))[0]
    bar = _Bar(f"text_feat_gates B={B} L={L} E={E} G={G}", LOG)
    bar.check("gx", got, r64, r32)
    # flagged: only the dirty sequences' rows are written, with the unflagged call's bytes
    dirty = torch.tensor([b_ % 2 for b_ in range(B)], dtype=torch.int32, device=DEV)
    out = torch.full((B * L, G), 7.0, device=DEV)
    ops.text_feat_gates(xd, wd, bd, dirty=dirty, out=out)
    o3, g3 = out.view(B, L, G), got.view(B, L, G)
    for b_ in range(B):
        assert _same_bytes(o3[b_], g3[b_]) if b_ % 2 else bool((o3[b_] == 7.0).all()), f"sequence {b_}"
    nob = ops.text_feat_gates(xd, wd, None)
    bar.check("gx-nobias", nob, r64 - b.double(), torch.mm(x.view(B * L, E), w.t()))
    bar.done()


def test_gate_projection_with_four_byte_aligned_weights_and_output():
    """w and gx whose base pointers are only 4-byte aligned (E % 4 == 0, G % 4 == 0): the scalar loads and the scalar
    stores - the same bytes as the aligned call"""
    from ivln_ce_amd import ops

    B, L, E, G = 3, 6, 8, 68
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, L, E, generator=g).to(DEV)
    w = (torch.randn(G, E, generator=g) / E ** 0.5).to(DEV)
    b = (torch.randn(G, generator=g) * 0.1).to(DEV)
    want = ops.text_feat_gates(x, w, b)
    wbuf, obuf = torch.zeros(G * E + 1, device=DEV), torch.full((B * L * G + 2,), 7.0, device=DEV)
    w1, out1 = wbuf[1:].view(G, E), obuf[1:1 + B * L * G].view(B * L, G)
    w1.copy_(w)
    assert w1.data_ptr() % 16 == 4 and out1.data_ptr() % 16 == 4
    ops.text_feat_gates(x, w1, b, out=out1)
    assert _same_bytes(out1, want) and float(obuf[0]) == 7.0 and float(obuf[-1]) == 7.0  # (nothing outside the view)
