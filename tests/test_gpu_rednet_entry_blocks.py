"""RedNet's stride-2 entry blocks (layers 2-4) with the downsample branch inside conv3's K (rednet.MERGE_ENTRY_CONV3) and the
fusion add that also emits the block's gathered input (rednet.FUSE_ADD_GATHER, k_add_subsample2_x4): each piece alone, then
the network at B = 2 against the CPU oracle, the old launch sequence and the recorded plan."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
DEV = "cuda:0"
SENTINEL = -12345.678


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("N,Cc,H,W", [(2, 3, 4, 8), (4, 5, 6, 16), (2, 16, 2, 8)])
@pytest.mark.parametrize("coff", [0, 3])
def test_add_subsample2_is_add_then_gather_then_slice_copy(N, Cc, H, W, coff):
    """k_add_subsample2_x4 against ops.add + ops.pool2d(x, 1, 2, 0, "max") + a slice copy, bit for bit: the RGB half summed in
    place, the depth half untouched, the gather of both in dst[:, coff : coff + C], every other channel of dst still the
    sentinel's bits.  Then the gather-only form (add=False) of the same tensor."""
    from ivln_ce_amd import ops

    B = N // 2
    g = torch.Generator().manual_seed(N * 100 + Cc * 10 + H + coff)
    x0 = torch.randn(N, Cc, H, W, generator=g).to(DEV)
    s = ops.add(x0[:B].contiguous(), x0[B:].contiguous())
    full = torch.cat([s, x0[B:]]).contiguous()
    sub = ops.pool2d(full, 1, 2, 0, "max")
    want = torch.full((N, Cc + 5, H // 2, W // 2), SENTINEL, device=DEV)
    want[:, coff:coff + Cc] = sub
    x = x0.clone()
    dst = torch.full((N, Cc + 5, H // 2, W // 2), SENTINEL, device=DEV)
    fused = ops.add_subsample2(x, B, dst, coff)
    assert fused.data_ptr() == x.data_ptr() and tuple(fused.shape) == (B, Cc, H, W)
    assert torch.equal(_bits(x), _bits(full)), "x[:B] += x[B:] in place, x[B:] as it was"
    assert torch.equal(_bits(dst), _bits(want))
    # the gather alone: nothing written to x
    dst2 = torch.full((N, Cc + 5, H // 2, W // 2), SENTINEL, device=DEV)
    y = full.clone()
    ops.add_subsample2(y, N, dst2, coff, add=False)
    assert torch.equal(_bits(y), _bits(full)) and torch.equal(_bits(dst2), _bits(want))


def _conv_spy(ops, *a, **kw):
    """ops.conv2d, and the split count the launch used (ivln_gemm_desc.splits_used)."""
    used, orig = C.c_int32(0), ops.gemm

    def spy(desc):
        desc.splits_used = C.pointer(used)
        orig(desc)

    ops.gemm = spy
    try:
        y = ops.conv2d(*a, **kw)
    finally:
        ops.gemm = orig
    return y, used.value


@pytest.mark.parametrize("N,Cin,Ho,Wo,G", [(2, 16, 8, 8, 0), (4, 32, 8, 8, 0), (2, 32, 16, 32, 0), (4, 32, 16, 32, 2)])
def test_stride2_conv3x3_writes_a_channel_slice_in_both_forms(N, Cin, Ho, Wo, G):
    """conv2 of a merged entry block writes buf[:, Cin:] (ivln_gemm_desc.Ctot): the stride-2 3x3 split-bf16 kernel in its plain
    form and - from two 16-channel chunks - with the chunks split over blockIdx.z + k_splitk_epilogue4, each bit-identical to
    the same launch into a dense tensor, the channels in front still the sentinel's bits."""
    from ivln_ce_amd import ops

    Cout = 32
    g = torch.Generator().manual_seed(N + Cin + Wo)
    x = torch.randn(N, Cin, 2 * Ho, 2 * Wo, generator=g).to(DEV)
    wshape = (G, Cout, Cin, 3, 3) if G else (Cout, Cin, 3, 3)
    w = (torch.randn(*wshape, generator=g) / (Cin * 9) ** 0.5).to(DEV)
    sc, sh = (torch.rand(max(G, 1) * Cout, generator=g) + 0.5).to(DEV), torch.randn(max(G, 1) * Cout, generator=g).to(DEV)
    ref = torch.cat([F.conv2d(x[i * (N // max(G, 1)):(i + 1) * (N // max(G, 1))].double().cpu(), (w[i] if G else w).double().cpu(), stride=2, padding=1)
                     for i in range(max(G, 1))])
    forms = [("plain", dict(splitk=False))] + ([("z-split", dict())] if Cin >= 32 else [])
    try:
        ops.TILE_OVERRIDE = 9
        for name, kw in forms:
            dense, used = _conv_spy(ops, x, w, stride=2, pad=1, scale=sc, shift=sh, relu=True, **kw)
            assert (used == 1) if name == "plain" else (used > 1), (name, used)
            buf = torch.full((N, Cin + Cout, Ho, Wo), SENTINEL, device=DEV)
            _, used2 = _conv_spy(ops, x, w, stride=2, pad=1, scale=sc, shift=sh, relu=True, out=buf[:, Cin:], out_ctot=Cin + Cout, **kw)
            assert used2 == used
            assert torch.equal(_bits(buf[:, Cin:]), _bits(dense)), name
            assert torch.equal(_bits(buf[:, :Cin]), _bits(torch.full((N, Cin, Ho, Wo), SENTINEL))), name
        raw, _ = _conv_spy(ops, x, w, stride=2, pad=1, splitk=False)
    finally:
        ops.TILE_OVERRIDE = 0
    assert float((raw.double().cpu() - ref).abs().max()) <= 3e-6 * float(ref.abs().max())


@pytest.mark.parametrize("K", [384, 768, 1536])
@pytest.mark.parametrize("form", [12, 13])
@pytest.mark.parametrize("M,N,G", [(64, 2, 0), (48, 2, 0), (64, 4, 2)])
def test_merged_conv3_matches_float64_conv_of_the_concatenation(K, form, M, N, G):
    """The merged conv3 as the library sees it - a 1x1 conv over Cin + Cmid = 384 / 768 / 1536 channels with no scale, a shift
    and the ReLU - on both forms of k_conv1x1_bf3_ks (tile_override 12 = K split over the waves, 13 = wave tiles; 96 chunks
    are beyond the wave-tile form, which the launcher then runs K-split), a ragged channel tile, image-grouped weights:
    within 3e-6 of the largest output of the float64 conv (tests/test_gpu_kernels.py's bound for this kernel)."""
    from ivln_ce_amd import ops
    from test_gpu_kernels import _close

    Cin = K * 2 // 3
    g = torch.Generator().manual_seed(K + form + M + N)
    xs, y2 = torch.randn(N, Cin, 8, 8, generator=g), torch.randn(N, K - Cin, 8, 8, generator=g).abs()
    wshape = (G, M, K, 1, 1) if G else (M, K, 1, 1)
    w = torch.randn(*wshape, generator=g) / K ** 0.5
    sh = torch.randn(max(G, 1) * M, generator=g)
    cat = torch.cat([xs, y2], dim=1).double()
    per = N // max(G, 1)
    ref = torch.cat([F.relu(F.conv2d(cat[i * per:(i + 1) * per], (w[i] if G else w).double()) + sh[i * M:(i + 1) * M].double().view(1, -1, 1, 1))
                     for i in range(max(G, 1))])
    buf = torch.empty(N, K, 8, 8, device=DEV)
    buf[:, :Cin], buf[:, Cin:] = xs.to(DEV), y2.to(DEV)
    try:
        ops.TILE_OVERRIDE = form
        got = ops.conv2d(buf, w.to(DEV), shift=sh.to(DEV), relu=True)
        again = ops.conv2d(buf, w.to(DEV), shift=sh.to(DEV), relu=True)
    finally:
        ops.TILE_OVERRIDE = 0
    err, scale = float((got.double().cpu() - ref).abs().max()), float(ref.abs().max())
    print(f"merged 1x1 K={K} form={form} M={M} N={N} G={G}: max|err|={err:.3e} of {scale:.3f}")
    assert err <= 3e-6 * scale
    _close(got, ref.float(), 3e-5)
    assert torch.equal(got, again)


def test_rednet_B2_merged_entry_blocks_match_oracle_old_path_and_plan():
    """RedNet at B = 2, 256 x 256 with the merged entry blocks: scores within 3e-4 of the fp32 CPU oracle and >= 99.9 % label
    agreement (tests/test_gpu_predsem.py's bounds), within the same 3e-4 of the old launch sequence, and the recorded plan
    (ivln_rednet_fwd, eager) returns the layer walk's labels bit for bit - with the three fused add + gather launches in it."""
    from det_init import det_fill

    from ivln_ce_amd import ops, rednet
    from ivln_ce_amd.synthetic import SyntheticRollout
    from oracle.rednet_ref import RedNetRef, predict_semantics_ref

    torch.set_num_threads(8)
    o = SyntheticRollout(B=2, seed=77, with_rgb=True).step()
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in o.items()}
    ps = rednet.PredictSemantics(torch.device(DEV), load_weights=False)
    ps.setup()
    det_fill(ps.model, seed=1, conv_gain=0.6)
    ps.model.invalidate_folded()
    ref_net = det_fill(RedNetRef(), seed=1, conv_gain=0.6).eval()
    scores_ref, labels_ref, _ = predict_semantics_ref(ref_net, o["rgb"], o["depth"])
    assert rednet.MERGE_ENTRY_CONV3 and rednet.FUSE_ADD_GATHER and rednet.GROUP_ENCODERS
    with ops.recording() as rec:
        scores = ps.scores(d)
    kinds = [op.kind for op in rec.ops]
    assert kinds.count(ops.OP_ADD_SUBSAMPLE2) == 3
    labels = ops.argmax_channels_u8(scores).cpu()
    err = float((scores.cpu() - scores_ref).abs().max())
    agree = float((labels == labels_ref).float().mean())
    print(f"rednet B=2 256x256 merged: max|err|={err:.3e} labels agree={agree:.5f}")
    assert err < 3e-4 and agree >= 0.999
    # the old sequence: downsample conv, conv3 + residual, add and gather as launches of their own
    try:
        rednet.MERGE_ENTRY_CONV3 = False
        with ops.recording() as rec_old:
            scores_old = ps.scores(d)
    finally:
        rednet.MERGE_ENTRY_CONV3 = True
    assert [op.kind for op in rec_old.ops].count(ops.OP_ADD_SUBSAMPLE2) == 0 and len(rec_old.ops) > len(rec.ops)
    diff = float((scores - scores_old).abs().max())
    print(f"merged vs old sequence: max|diff|={diff:.3e}")
    assert diff < 3e-4
    # separate encoder chains (Bottleneck.forward_hip, the gather-only form)
    try:
        rednet.GROUP_ENCODERS = False
        scores_sep = ps.scores(d)
    finally:
        rednet.GROUP_ENCODERS = True
    assert float((scores - scores_sep).abs().max()) < 3e-4
    # the plan: first call records (layer walk), the second replays the table through ivln_rednet_fwd
    if ps.USE_PLAN:
        first = ps(d).cpu()
        replay = ps(d).cpu()
        assert torch.equal(first, labels) and torch.equal(replay, labels)
