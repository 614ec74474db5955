"""The map CNN at rollout batch: every CBRA block (7x7 conv -> eval BatchNorm -> ReLU -> AvgPool(2)) as one launch of
k_conv7_pool_bf3 (csrc/conv_bf3.hip, ops.conv7_bn_relu_pool), the first block staging the u8 maps itself."""
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _close(got, ref, atol, rtol=1e-4):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    err = (got - ref).abs().max().item()
    assert torch.allclose(got, ref, atol=atol, rtol=rtol), f"max err {err:.3e}, ref max {ref.abs().max().item():.3e}"


def _two_launches(ops, x, w, scale, shift):
    """the path before this kernel: fp32 conv leaving raw split-K slabs + the reducing BN / ReLU / pool tail"""
    return ops.scale_shift_relu_avgpool2(ops.conv2d(x, w, pad=3, defer=True), scale, shift)


@pytest.mark.parametrize("N,Cin,Cout,S", [(1, 14, 32, 64), (3, 14, 32, 64), (2, 32, 64, 32), (5, 64, 128, 16), (3, 128, 256, 8),
                                          (9, 128, 256, 8), (8, 128, 256, 8), (2, 64, 40, 16)])
def test_block_against_float64(N, Cin, Cout, S):
    """Each layer form (1, 2, 4, 8 waves = 16-channel chunks; ragged image counts; a masked channel tile) against
    F.conv2d -> scale / shift -> relu -> avg_pool2d(2) in float64.  The conv part (identity scale, zero shift, the reference
    pooled from the float64 conv) is held to the bar of test_conv2d_split_bf16_kernel: 3e-6 of the largest output and at most
    twice the fp32 kernel's error + 1e-6; the fused result to 3e-5; two runs give the same bits."""
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(N * 1000 + Cin + Cout)
    x = torch.randn(N, Cin, S, S, generator=g)
    w = torch.randn(Cout, Cin, 7, 7, generator=g) / (Cin * 49) ** 0.5
    sc, sh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    ref0 = F.conv2d(x.double(), w.double(), None, stride=1, padding=3)
    ref_id = F.avg_pool2d(F.relu(ref0), 2)
    ref = F.avg_pool2d(F.relu(ref0 * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)), 2)
    xd, wd, scd, shd = x.to(DEV), w.to(DEV), sc.to(DEV), sh.to(DEV)
    one, zero = torch.ones(Cout, device=DEV), torch.zeros(Cout, device=DEV)
    got_id = ops.conv7_bn_relu_pool(xd, wd, one, zero)
    assert got_id is not None and got_id.shape == (N, Cout, S // 2, S // 2)
    fp32_id = _two_launches(ops, xd, wd, one, zero)
    largest = float(ref_id.abs().max())
    e_split = float((got_id.double().cpu() - ref_id).abs().max()) / largest
    e_fp32 = float((fp32_id.double().cpu() - ref_id).abs().max()) / largest
    print(f"conv part: split-bf16 {e_split:.3e}, fp32 {e_fp32:.3e} of the largest output")
    assert e_split <= 3e-6 and e_split <= 2.0 * e_fp32 + 1e-6, (e_split, e_fp32)
    got = ops.conv7_bn_relu_pool(xd, wd, scd, shd)
    again = ops.conv7_bn_relu_pool(xd, wd, scd, shd)
    assert torch.equal(got, again)
    _close(got, ref.float(), 3e-5)


@pytest.mark.parametrize("N,H,W", [(2, 64, 64), (3, 8, 16)])
def test_first_block_stages_the_u8_maps(N, H, W):
    """Layer 1 fed the u8 occupancy and label maps (every byte value 0 ... 255 occurs; labels >= 13 match no channel) gives,
    bit for bit, what the same kernel gives on ops.map_features' fp32 tensor."""
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(H + N)
    occ = torch.randint(0, 256, (N, H, W), generator=g).to(torch.uint8)
    sem = torch.randint(0, 256, (N, H, W), generator=g).to(torch.uint8)
    occ.view(-1)[:256] = torch.arange(256).to(torch.uint8)
    sem.view(-1)[:256] = torch.arange(255, -1, -1).to(torch.uint8)
    sem.view(-1)[256:] = sem.view(-1)[256:] % 20  # (most labels inside the 13 classes, some past them)
    w = (torch.randn(32, 14, 7, 7, generator=g) / (14 * 49) ** 0.5).to(DEV)
    sc, sh = (torch.rand(32, generator=g) + 0.5).to(DEV), torch.randn(32, generator=g).to(DEV)
    occd, semd = occ.to(DEV), sem.to(DEV)
    feats = ops.map_features(occd, semd)
    via_f32 = ops.conv7_bn_relu_pool(feats, w, sc, sh)
    via_u8 = ops.conv7_bn_relu_pool(None, w, sc, sh, maps_u8=(occd, semd))
    assert via_f32 is not None and via_u8 is not None
    assert torch.equal(via_u8, via_f32)


def _space(H, W):
    box = types.SimpleNamespace(shape=(H, W))
    return types.SimpleNamespace(spaces={"occupancy_map": box, "semantic_map": box})


def _encoder(H, W, seed, blocks=None):
    from ivln_ce_amd import encoders

    torch.manual_seed(seed)
    enc = encoders.SemanticMapEncoder(_space(H, W))
    if blocks is not None:
        enc.cnn = blocks
    for blk in enc.cnn:  # (running statistics and affine parameters a trained BatchNorm would hold)
        bn = blk.conv[1]
        bn.running_mean.normal_(0.0, 0.2)
        bn.running_var.uniform_(0.5, 1.5)
        bn.weight.data.uniform_(0.5, 1.5)
        bn.bias.data.normal_(0.0, 0.2)
    return enc.to(DEV).eval()


def _maps(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return {"occupancy_map": torch.randint(0, 3, (B, H, W), generator=g).to(torch.uint8).to(DEV),
            "semantic_map": torch.randint(0, 16, (B, H, W), generator=g).to(torch.uint8).to(DEV)}


def _run(enc, obs, fused):
    from ivln_ce_amd import encoders

    keep = encoders.MAP_CNN_FUSED
    try:
        encoders.MAP_CNN_FUSED = fused
        with torch.no_grad():
            return enc(obs)
    finally:
        encoders.MAP_CNN_FUSED = keep


@pytest.mark.parametrize("case", ["odd_h", "k5", "stride2", "map12"])
def test_refused_shapes_take_the_two_launch_path(case):
    """What the kernel does not hold - odd H, other kernel sizes, stride 2, maps its 4 x 8 tile does not divide - is refused and
    SemanticMapEncoder.forward gives the bits of the path before it (an odd H: the same error)."""
    from ivln_ce_amd import encoders, ops

    H, W = {"odd_h": (17, 16), "map12": (12, 12)}.get(case, (16, 16))
    blk = encoders.CBRA(14, 32)
    if case == "k5":
        blk.conv[0] = nn.Conv2d(14, 32, kernel_size=5, padding=3)
    if case == "stride2":
        blk.conv[0] = nn.Conv2d(14, 32, kernel_size=7, padding=3, stride=2)
    enc = _encoder(H, W, 5, blocks=nn.Sequential(blk))
    obs = _maps(3, H, W, 6)
    taken = []
    orig = ops.gemm_soft

    def spy(desc):
        ok = orig(desc)
        taken.append((int(desc.pool2), ok))
        return ok

    ops.gemm_soft = spy
    try:
        if case == "odd_h":  # (the path before refuses an odd map outright - the pooling tail's argument check: so does this one)
            from ivln_ce_amd._lib import IvlnError

            with pytest.raises(IvlnError):
                _run(enc, obs, False)
            with pytest.raises(IvlnError):
                _run(enc, obs, True)
            assert not any(ok for pool2, ok in taken if pool2), taken
            return
        new = _run(enc, obs, True)
    finally:
        ops.gemm_soft = orig
    assert not any(ok for pool2, ok in taken if pool2), taken
    old = _run(enc, obs, False)
    assert torch.equal(new, old)


_REF = {}


def _float64_encoder(enc, obs):
    occ, sem = obs["occupancy_map"].cpu(), obs["semantic_map"].cpu()
    x = torch.cat([occ.double().unsqueeze(1), F.one_hot(sem.long(), 256)[..., :13].permute(0, 3, 1, 2).double()], 1)
    for blk in enc.cnn:
        conv, bn = blk.conv[0], blk.conv[1]
        y = F.conv2d(x, conv.weight.double().cpu(), conv.bias.double().cpu(), padding=3)
        y = F.batch_norm(y, bn.running_mean.double().cpu(), bn.running_var.double().cpu(), bn.weight.double().cpu(), bn.bias.double().cpu(),
                         False, 0.0, bn.eps)
        x = F.avg_pool2d(F.relu(y), 2)
    return x


@pytest.mark.parametrize("B", [1, 4, 8])
def test_whole_encoder(B):
    """The rollout's encoder at 1, 4 and 8 envs: four launches, against the path before (eight + the feature launch) and a
    float64 restatement in torch - the new path's error is at most twice the old path's + 1e-6 of the largest feature."""
    from ivln_ce_amd import ops

    if "enc" not in _REF:
        _REF["enc"] = _encoder(64, 64, 11)
    enc = _REF["enc"]
    obs = _maps(B, 64, 64, 20 + B)
    ref = _float64_encoder(enc, obs)
    taken = []
    orig = ops.gemm_soft

    def spy(desc):
        ok = orig(desc)
        taken.append((int(desc.pool2), ok))
        return ok

    ops.gemm_soft = spy
    try:
        new = _run(enc, obs, True)
    finally:
        ops.gemm_soft = orig
    assert taken == [(1, True)] * 4, taken
    old = _run(enc, obs, False)
    assert new.shape == old.shape == (B, 256, 4, 4)
    largest = float(ref.abs().max())
    e_new = float((new.double().cpu() - ref).abs().max()) / largest
    e_old = float((old.double().cpu() - ref).abs().max()) / largest
    print(f"B={B}: new {e_new:.3e}, old {e_old:.3e} of the largest feature")
    assert e_new <= 2.0 * e_old + 1e-6, (e_new, e_old)
    assert torch.equal(new, _run(enc, obs, True))
