"""GPU: RedNet's train-mode forward (RedNet.forward_train) and hand-written backward (train.rednet_backward) - each
TransBasicBlock form alone, the whole net with every parameter training, with every BatchNorm in eval mode, and with the
encoders frozen.

Reference: the mask-frozen float64 twin (tests/rednet_twin.py, pinned to the reference by tests/test_rednet_train_twin.py),
with the ReLU masks and max-pool indices taken from the HIP pass's saves.  Bars are those of
tests/test_gpu_rgb_encoder_train.py: forward outputs and running statistics 4 x what torch's fp32 pass is away from ITS twin
+ 2e-5 max|ref|; gradients the project's gradient bar per tensor (max|got - ref| <= 1e-3 max|ref| + 2e-7, cosine >= 1 - 1e-6)
and, where torch's own fp32 autograd is near that bar itself, 4 x its error (rgb_twin.compare_with_allowance).  Every
figure is written to the suite's log directory before it is asserted."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "golden"))
import rednet_twin as RW  # noqa: E402

DEV = torch.device("cuda:0")
FWD_REL = 2e-5
CFG = {"n_classes": 13}


def _write(name, lines):
    from kernel_bar import _log_dir

    os.makedirs(_log_dir(), exist_ok=True)
    open(os.path.join(_log_dir(), name), "w").write("\n".join(lines) + "\n")


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.detach().cpu().contiguous().reshape(-1).view(torch.uint8),
                                             b.detach().cpu().contiguous().reshape(-1).view(torch.uint8))


class _Fwd:
    """Collects forward / statistics figures against the 4 x e32 + 2e-5 max|ref| bar."""

    def __init__(self):
        self.lines, self.bad = [], []

    def within(self, what, g, r64, e32):
        err, mx = float((g.detach().cpu().double() - r64.double()).abs().max()), float(r64.abs().max())
        bar = 4 * e32 + FWD_REL * mx
        self.lines.append(f"{what}: max|ref| {mx:.3e} hip {err:.3e} torch-fp32 {e32:.3e} bar {bar:.3e} {'ok' if err <= bar else 'OVER'}")
        if not err <= bar:
            self.bad.append(self.lines[-1])


# ------------------------------------------------------------------------------------------------
# each TransBasicBlock form alone
# ------------------------------------------------------------------------------------------------
def _block_pass(state, cin, planes, up, x, d_out, masks, dtype):
    """One pass of the oracle block in `dtype`, free (masks None) or frozen -> dict(out, grads incl. "input", bufs, masks)."""
    blk = RW.twin_block(cin, planes, up)
    blk.load_state_dict(state)
    blk = blk.to(dtype).train()
    xi = x.detach().clone().to(dtype).requires_grad_(True)
    k = RW.Kinks(masks)
    out = RW.transblock(blk, xi, k)
    assert k.used_all()
    out.backward(d_out.to(dtype))
    grads = {n: p.grad.detach() for n, p in blk.named_parameters()}
    grads["input"] = xi.grad.detach()
    return dict(out=out.detach(), grads=grads, bufs={n: b.detach().clone() for n, b in blk.named_buffers()}, masks=k.masks)


@pytest.mark.parametrize("up,cin,planes,h,w", [(False, 64, 64, 2, 2), (False, 64, 64, 3, 5), (True, 128, 64, 2, 2), (True, 128, 64, 3, 5)])
def test_transbasicblock_forward_statistics_and_every_gradient_against_the_frozen_twin(up, cin, planes, h, w):
    from ivln_ce_amd import rednet, train

    torch.set_num_threads(min(8, torch.get_num_threads()))
    B = 2
    g = torch.Generator().manual_seed(10 * h + w + int(up))
    tb = RW.rand_bn_(RW.twin_block(cin, planes, up), g)
    state = {k: v.clone() for k, v in tb.state_dict().items()}
    upsample = None
    if up:
        upsample = torch.nn.Sequential(torch.nn.ConvTranspose2d(cin, planes, 2, 2, 0, bias=False), torch.nn.BatchNorm2d(planes))
    hip = rednet.TransBasicBlock(cin, planes, 2 if up else 1, upsample)
    hip.load_state_dict(state)
    hip = hip.to(DEV).train()
    x = torch.randn(B, cin, h, w, generator=g)
    o = 2 if up else 1
    d_out = torch.randn(B, planes, h * o, w * o, generator=g)
    save = []
    with torch.no_grad():
        out = rednet._transblock_train(hip, x.to(DEV), save).clone()
    assert tuple(out.shape) == tuple(d_out.shape) and len(save) == 1 and (save[0]["up"] is not None) == up
    masks = RW.block_masks(save)
    bufs = {k: v.detach().cpu().clone() for k, v in hip.named_buffers()}
    G = {}
    with torch.no_grad():
        dx = train._transblock_backward(hip, save.pop(), d_out.to(DEV), G)
    torch.cuda.synchronize()
    names = {p: k for k, p in hip.named_parameters()}
    got = {names[p]: v for p, v in G.items()}
    got["input"] = dx
    assert len(got) == len(names) + 1 and all(got[k].shape == p.shape for k, p in hip.named_parameters())

    ref = _block_pass(state, cin, planes, up, x, d_out, masks, torch.float64)
    f32 = _block_pass(state, cin, planes, up, x, d_out, None, torch.float32)
    f64 = _block_pass(state, cin, planes, up, x, d_out, f32["masks"], torch.float64)
    e32 = {k: float((v.double() - f64["grads"][k]).abs().max()) for k, v in f32["grads"].items()}
    F = _Fwd()
    F.within("out", out, ref["out"], float((f32["out"].double() - f64["out"]).abs().max()))
    for k, v in ref["bufs"].items():
        if k.endswith("num_batches_tracked"):
            assert int(bufs[k]) == int(v) == 1, k
        else:
            F.within(k, bufs[k], v, float((f32["bufs"][k].double() - f64["bufs"][k]).abs().max()))
    log, over = RW.compare_with_allowance(got, ref["grads"], e32)
    _write(f"rednet_transblock_{'up' if up else 'plain'}_{h}x{w}.log", F.lines + log)
    assert not F.bad, "\n".join(F.bad)
    assert not over, "\n".join(over)


# ------------------------------------------------------------------------------------------------
# the whole net
# ------------------------------------------------------------------------------------------------
def _state():
    from det_init import det_fill

    return {k: v.clone() for k, v in det_fill(RW.RedNetTwin(), seed=1, conv_gain=0.6).state_dict().items()}


def _model(state, train):
    from ivln_ce_amd.rednet import RedNet

    m = RedNet(CFG)
    m.load_state_dict(state)
    return m.to(DEV).train(train)


def _inputs(B=2, H=64, seed=21):
    g = torch.Generator().manual_seed(seed)
    rgb, depth = torch.randn(B, 3, H, H, generator=g), torch.randn(B, 1, H, H, generator=g)
    d_outs = [torch.randn(B, 13, H >> i, H >> i, generator=g) for i in range(5)]
    return rgb, depth, d_outs


def _hip_pass(model, rgb, depth, d_outs, trainable="all", want_masks=True):
    from ivln_ce_amd import train

    save = {}
    with torch.no_grad():
        outs = [o.clone() for o in model.forward_train(rgb.to(DEV), depth.to(DEV), save, trainable=trainable)]
    flags = _train_flags(save)
    masks, pools = RW.masks_from_saves(save) if want_masks else (None, None)
    bufs = {k: v.detach().cpu().clone() for k, v in model.named_buffers()}
    G = {}
    with torch.no_grad():
        train.rednet_backward(model, save, [d.to(DEV) for d in d_outs], G)
    torch.cuda.synchronize()
    assert not save, f"the saves are released as the backward walks them: {sorted(save)}"
    names = {p: k for k, p in model.named_parameters()}
    return dict(outs=outs, masks=masks, pools=pools, bufs=bufs, grads={names[p]: v for p, v in G.items()}, flags=flags)


def _train_flags(save):
    """The `train` flag of every BatchNorm save of the pass."""
    flags = []

    def walk(o):
        if isinstance(o, dict):
            if "train" in o and "raw" in o:
                flags.append(bool(o["train"]))
            for v in o.values():
                walk(v)
        elif isinstance(o, (list, tuple)):
            for v in o:
                walk(v)

    walk(save)
    return flags


def _hold(tag, hip, state, rgb, depth, d_outs, train):
    ref = RW.run(state, rgb, depth, d_outs, hip["masks"], hip["pools"], torch.float64, train)
    e = RW.fp32_error(state, rgb, depth, d_outs, train)
    F = _Fwd()
    for i, (o, r) in enumerate(zip(hip["outs"], ref["outs"])):
        assert tuple(o.shape) == tuple(r.shape) == (rgb.shape[0], 13, rgb.shape[2] >> i, rgb.shape[3] >> i)
        F.within(("out", "out2", "out3", "out4", "out5")[i], o, r, e["outs"][i])
    for k, v in ref["bufs"].items():
        if k.endswith("num_batches_tracked"):
            assert int(hip["bufs"][k]) == int(v) == (1 if train else 0), k
        elif train:
            F.within(k, hip["bufs"][k], v, e["bufs"][k])
        else:
            assert _same(hip["bufs"][k], state[k]), k
    log, over = RW.compare_with_allowance(hip["grads"], ref["grads"], e["grads"])
    _write(f"rednet_train_{tag}.log", F.lines + log)
    print(f"{tag}: {len(F.bad)} forward / statistics figures and {len(over)} of {len(ref['grads'])} gradients over the bar")
    assert not F.bad, "\n".join(F.bad)
    assert not over, "\n".join(over)


def test_whole_net_outputs_statistics_and_every_gradient_against_the_frozen_twin():
    torch.set_num_threads(min(8, torch.get_num_threads()))
    state = _state()
    model = _model(state, True)
    n_par = len(list(model.parameters()))
    rgb, depth, d_outs = _inputs()
    hip = _hip_pass(model, rgb, depth, d_outs)
    assert len(hip["grads"]) == n_par == 469
    assert all(hip["grads"][k].shape == p.shape for k, p in model.named_parameters())
    assert all(hip["flags"]) and len(hip["flags"]) == 2 + 2 * (16 * 3 + 4) + 5 + 2 * 19 + 4
    _hold("all", hip, state, rgb, depth, d_outs, True)


def test_whole_net_with_every_batchnorm_in_eval_mode_uses_the_running_statistics():
    torch.set_num_threads(min(8, torch.get_num_threads()))
    state = _state()
    model = _model(state, False)
    rgb, depth, d_outs = _inputs(seed=22)
    hip = _hip_pass(model, rgb, depth, d_outs)
    assert not any(hip["flags"]) and len(hip["flags"]) == 2 + 2 * (16 * 3 + 4) + 5 + 2 * 19 + 4
    for k, v in model.state_dict().items():
        assert _same(v, state[k]), f"{k} moved in eval mode"
    assert len(hip["grads"]) == 469
    _hold("eval", hip, state, rgb, depth, d_outs, False)


def test_decoder_only_leaves_the_encoders_alone_and_gives_the_same_decoder_gradients():
    """trainable="decoder", every BatchNorm in eval mode in both runs so that both compute the same function: G holds the
    decoder, agant and head parameters only, the encoders' parameters and buffers keep their bits, and the gradients equal the
    "all" run's within the gradient bar."""
    from ivln_ce_amd import ops

    state = _state()
    rgb, depth, d_outs = _inputs(seed=23)
    full = _hip_pass(_model(state, False), rgb, depth, d_outs, want_masks=False)
    model = _model(state, False)
    want = {k for k, _ in model.trainable_parameters("decoder")}
    enc = ("conv1.", "bn1.", "conv1_d.", "bn1_d.", "layer")
    assert len(want) == 151 and not any(k.startswith(enc) for k in want)
    assert all(k.startswith(("agant", "deconv", "final_", "out")) for k in want)

    def never(*a, **k):
        raise AssertionError("a backward kernel of the encoders ran for frozen encoders")

    keep = ops.maxpool3s2_bwd
    ops.maxpool3s2_bwd = never
    try:
        dec = _hip_pass(model, rgb, depth, d_outs, trainable="decoder", want_masks=False)
    finally:
        ops.maxpool3s2_bwd = keep
    assert set(dec["grads"]) == want
    for k, v in model.state_dict().items():
        if k.startswith(enc):
            assert _same(v, state[k]), f"{k} moved"
    log, bad = RW.compare(dec["grads"], {k: full["grads"][k].detach().cpu() for k in want})
    errs = [float((a - b).abs().max()) for a, b in zip(dec["outs"], full["outs"])]
    _write("rednet_train_decoder.log", [f"outputs, folded encoders vs layer-by-layer: {errs}"] + log)
    assert not bad, "\n".join(bad)
