"""The mask-frozen float64 twin of the depth ResNet that the trainable-encoder tests compare gradients with, and the small
helpers they share.  Not a conftest: plain functions, imported by name.

Why a twin and not free float64 autograd: the encoder has 50 ReLUs and a max-pool.  Between fp32 and float64 a share of
their kinks flips (a pre-activation of +1e-8 in one precision is -1e-8 in the other), and every flip changes the gradient
of everything upstream by a finite amount - a correct fp32 backward is 1e-2-relative away from free float64 autograd
(tests/test_depth_twin.py pins that).  The twin is the oracle's ResNetEncoder in float64 with every ReLU replaced by a
multiplication with the fp32 pass's `out > 0` and the max-pool by a gather at the fp32 pass's argmax indices: the same
piecewise-linear function the fp32 pass differentiated, evaluated exactly."""
import itertools
import os
import sys
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def oracle_encoder(state_dict=None, seed=5):
    """The oracle's habitat-lab ResNetEncoder for a (256, 256, 1) depth space on the CPU, fp32, GroupNorm affine
    randomised as tests/test_gpu_depth_net.py does (or loaded from `state_dict`), every parameter trainable."""
    from oracle import habitat_ext_ref as R

    space = types.SimpleNamespace(spaces={"depth": types.SimpleNamespace(shape=(256, 256, 1))})
    torch.manual_seed(seed)
    enc = R.ResNetEncoder(space, baseplanes=32, ngroups=16, make_backbone=R.resnet50)
    if state_dict is not None:
        enc.load_state_dict({k: v.detach().cpu() for k, v in state_dict.items()})
    else:
        with torch.no_grad():
            for m in enc.modules():
                if isinstance(m, nn.GroupNorm):
                    m.weight.normal_(1.0, 0.2)
                    m.bias.normal_(0.0, 0.2)
    for p in enc.parameters():
        p.requires_grad_(True)
    return enc


def _relus(enc):
    """The encoder's ReLU modules, not in place (a forward hook replaces their output)."""
    out = [m for m in enc.modules() if isinstance(m, nn.ReLU)]
    for m in out:
        m.inplace = False
    return out


def record_masks(enc, depth):
    """One fp32 (or whatever `enc` is) pass with autograd -> (features, masks in call order, pool indices): what a frozen
    twin of this pass needs.  The ReLUs are made out-of-place."""
    masks, pool = [], []
    hooks = [m.register_forward_hook(lambda _m, _i, o: masks.append(o.detach() > 0)) for m in _relus(enc)]
    hooks.append(enc.backbone.maxpool.register_forward_hook(
        lambda _m, i, _o: pool.append(F.max_pool2d(i[0].detach(), 3, 2, 1, return_indices=True)[1])))
    try:
        feats = enc({"depth": depth})
    finally:
        for h in hooks:
            h.remove()
    return feats, masks, pool[0]


def twin_gradients(state_dict, depth, masks, pool_idx, d_feats):
    """Gradients of the float64 twin: the oracle encoder with `state_dict`, each ReLU (in call order) a multiplication with
    masks[i], the max-pool a gather at pool_idx, differentiated under the upstream gradient d_feats.
    -> ({name: float64 gradient}, float64 features)."""
    enc = oracle_encoder(state_dict).double()
    it = itertools.count()
    ms = [m.to(torch.float64) for m in masks]
    hooks = [m.register_forward_hook(lambda _m, i, _o: i[0] * ms[next(it)]) for m in _relus(enc)]
    idx = pool_idx.cpu()

    def gather(_m, i, o):
        return i[0].flatten(2).gather(2, idx.flatten(2)).view_as(o)

    hooks.append(enc.backbone.maxpool.register_forward_hook(gather))
    try:
        feats = enc({"depth": depth.detach().cpu().double()})
        feats.backward(d_feats.detach().cpu().double().reshape(feats.shape))
    finally:
        for h in hooks:
            h.remove()
    assert next(it) == len(ms), "every mask was used exactly once"
    return {k: p.grad.detach() for k, p in enc.named_parameters()}, feats.detach()


def masks_from_saves(save):
    """(masks in the oracle's ReLU call order, pool indices) from what ResNetEncoder.forward_train saved, on the CPU."""
    stem = save["stem"]["out"].detach().cpu()
    masks = [stem > 0]
    for s in save["blocks"]:
        masks += [s["l1"]["out"].detach().cpu() > 0, s["l2"]["out"].detach().cpu() > 0, s["out"].detach().cpu() > 0]
    masks.append(save["comp"]["out"].detach().cpu() > 0)
    return masks, F.max_pool2d(stem, 3, 2, 1, return_indices=True)[1]


def compare(got, ref, rel=1e-3, abs_=2e-7, cos_min=1 - 1e-6):
    """The project's gradient bar (tests/test_gpu_train.py) per tensor: max|got - ref| <= rel * max|ref| + abs_ and the
    direction cosine >= cos_min.  -> (log lines, lines over the bar)."""
    log, bad = [], []
    assert sorted(got) == sorted(ref), (sorted(set(got) ^ set(ref)))
    for k in ref:
        g, r = got[k].detach().cpu().double().reshape(-1), ref[k].double().reshape(-1)
        scale, err = float(r.abs().max()), float((g - r).abs().max())
        cos = float(torch.dot(g, r) / (g.norm() * r.norm()).clamp_min(1e-300)) if scale > 0 else 1.0
        log.append(f"{k}: max|ref| {scale:.3e} max|err| {err:.3e} rel {err / max(scale, 1e-300):.2e} cos-1 {cos - 1:.1e}")
        if not (err <= rel * scale + abs_ and (cos >= cos_min or scale < 1e-6)):
            bad.append(log[-1])
    return log, bad
