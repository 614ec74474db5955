"""The mask-frozen float64 twin of the RGB ResNet-50 that the trainable-encoder tests compare gradients with, and the small
helpers they share.  Not a conftest: plain functions, imported by name.

Why a twin and not free float64 autograd: tests/depth_twin.py gives the reason - here the network has 49 ReLUs and a
max-pool whose kinks flip between fp32 and float64, and train-mode BatchNorm couples every pixel of a channel, so one flip
moves the whole batch.  The twin is oracle/torchvision_ref.py's ResNet-50, sliced as the reference slices it
(resnet_encoders.py:153-163: children [conv1, bn1, relu, maxpool, layer1..4], then adaptive_avg_pool2d to 4 x 4), in
float64 with BatchNorm in train mode, every ReLU replaced by a multiplication with the fp32 pass's `out > 0` and the
max-pool by a gather at the fp32 pass's argmax: the piecewise-smooth function the fp32 pass differentiated."""
import itertools
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from depth_twin import compare  # noqa: E402,F401  (the project's gradient bar, per tensor)


def oracle_cnn(state_dict=None, seed=5):
    """The reference's `rgb_encoder.cnn` (without the pool) on the CPU, fp32, train mode, every parameter trainable;
    BatchNorm affine randomised (or everything loaded from `state_dict`, running statistics included)."""
    from oracle import torchvision_ref as TV

    torch.manual_seed(seed)
    cnn = nn.Sequential(*list(TV.resnet50().children())[:-2])  # [:-1] drops fc, the reference's second [:-1] avgpool
    if state_dict is not None:
        cnn.load_state_dict({k: v.detach().cpu() for k, v in state_dict.items()})
    else:
        with torch.no_grad():
            for m in cnn.modules():
                if isinstance(m, nn.BatchNorm2d):
                    m.weight.normal_(1.0, 0.2)
                    m.bias.normal_(0.0, 0.2)
    for p in cnn.parameters():
        p.requires_grad_(True)
    return cnn.train()


def to_input(rgb_u8):
    """(B, H, W, 3) u8 frames -> what the reference feeds `cnn`: NCHW / 255 (resnet_encoders.py:182,198)."""
    return rgb_u8.permute(0, 3, 1, 2).contiguous().float() / 255.0


def features(cnn, x):
    return F.adaptive_avg_pool2d(cnn(x), (4, 4))


def _relus(cnn):
    out = [m for m in cnn.modules() if isinstance(m, nn.ReLU)]
    for m in out:
        m.inplace = False
    return out


def record_masks(cnn, x):
    """One pass with autograd -> (features, the 49 masks in call order, pool indices): what a frozen twin of it needs."""
    masks, pool = [], []
    hooks = [m.register_forward_hook(lambda _m, _i, o: masks.append(o.detach() > 0)) for m in _relus(cnn)]
    hooks.append(cnn[3].register_forward_hook(
        lambda _m, i, _o: pool.append(F.max_pool2d(i[0].detach(), 3, 2, 1, return_indices=True)[1])))
    try:
        feats = features(cnn, x)
    finally:
        for h in hooks:
            h.remove()
    return feats, masks, pool[0]


def twin_gradients(state_dict, x, masks, pool_idx, d_feats):
    """The float64 twin under the upstream gradient d_feats (B, 2048, 4, 4): each ReLU (in call order) a multiplication
    with masks[i], the max-pool a gather at pool_idx.  `state_dict`: the state BEFORE the pass (train-mode BatchNorm moves
    the running statistics).  -> ({name: float64 gradient}, float64 features, {name: buffer after the pass})."""
    cnn = oracle_cnn(state_dict).double()
    it = itertools.count()
    ms = [m.cpu().to(torch.float64) for m in masks]
    hooks = [m.register_forward_hook(lambda _m, i, _o: i[0] * ms[next(it)]) for m in _relus(cnn)]
    idx = pool_idx.cpu()

    def gather(_m, i, o):
        return i[0].flatten(2).gather(2, idx.flatten(2)).view_as(o)

    hooks.append(cnn[3].register_forward_hook(gather))
    try:
        feats = features(cnn, x.detach().cpu().double())
        feats.backward(d_feats.detach().cpu().double().reshape(feats.shape))
    finally:
        for h in hooks:
            h.remove()
    assert next(it) == len(ms), "every mask was used exactly once"
    return ({k: p.grad.detach() for k, p in cnn.named_parameters()}, feats.detach(),
            {k: v.detach().clone() for k, v in cnn.named_buffers()})


def fp32_autograd_error(state_dict, x, d_feats):
    """What torch's own fp32 autograd is away from ITS frozen twin on these inputs, per tensor: {name: max|fp32 - twin|}.
    The reference arithmetic's own rounding noise - BatchNorm over a handful of values amplifies it - and nothing of the code
    under test.  -> dict(e32 = the errors, fp32 / twin = the gradients, feats32 / feats64 = the features, bufs32 / bufs64 =
    the BatchNorm buffers after the pass, masks, pool_idx)"""
    cnn = oracle_cnn(state_dict)
    feats, masks, pool_idx = record_masks(cnn, x.detach().cpu().float())
    feats.backward(d_feats.detach().cpu().float().reshape(feats.shape))
    fp32 = {k: p.grad.detach().clone() for k, p in cnn.named_parameters()}
    twin, feats64, bufs64 = twin_gradients(state_dict, x, masks, pool_idx, d_feats)
    return dict(e32={k: float((fp32[k].double() - twin[k]).abs().max()) for k in twin}, fp32=fp32, twin=twin,
                feats32=feats.detach(), feats64=feats64, bufs32={k: v.detach().clone() for k, v in cnn.named_buffers()},
                bufs64=bufs64, masks=masks, pool_idx=pool_idx)


def masks_from_saves(save):
    """(masks in the oracle's ReLU call order, pool indices) from what _ResNet50Body.forward_train saved, on the CPU."""
    stem = save["stem"]["out"].detach().cpu()
    masks = [stem > 0]
    for s in save["blocks"]:
        masks += [s["l1"]["out"].detach().cpu() > 0, s["l2"]["out"].detach().cpu() > 0, s["out"].detach().cpu() > 0]
    return masks, F.max_pool2d(stem, 3, 2, 1, return_indices=True)[1]


def compare_with_allowance(got, ref, e32):
    """depth_twin.compare's bar per tensor (max|got - ref| <= 1e-3 max|ref| + 2e-7, cosine >= 1 - 1e-6), and where torch's
    own fp32 autograd is near that bar itself (e32[k], fp32_autograd_error on the same inputs): 4 x e32[k] instead.
    -> (log lines with both figures, lines over both)."""
    log, bad = compare(got, ref)
    over = set(bad)
    out_log, out_bad = [], []
    for line in log:
        k = line.split(":", 1)[0]
        err = float((got[k].detach().cpu().double().reshape(-1) - ref[k].double().reshape(-1)).abs().max())
        full = f"{line} | fp32 autograd vs its twin {e32[k]:.3e}, 4x = {4 * e32[k]:.3e}"
        out_log.append(full)
        if line in over and not err <= 4 * e32[k]:
            out_bad.append(full)
    return out_log, out_bad
