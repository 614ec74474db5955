"""TEST INFRASTRUCTURE: the twin of RedNet's five-output training pass that the fine-tuning tests compare with, and the
small helpers they share.  Not a conftest: plain classes and functions, imported by name.

`RedNetTwin` is oracle/rednet_ref.py's RedNetRef (pinned to the reference's eval forward by tests/test_oracle_rednet.py)
with the training forward of the reference (rednet.py:224-256: out, out2, out3, out4, out5), in float32 or float64.
tests/test_rednet_train_twin.py pins it to the reference's own train-mode outputs and running statistics.

Why mask-frozen: tests/rgb_twin.py and tests/test_rgb_twin.py give the reasoning, which applies unchanged - RedNet has 151
ReLUs and two max-pools whose kinks flip between fp32 and float64, and train-mode BatchNorm couples every pixel of a
channel.  With `masks` / `pools` every ReLU is a multiplication with a recorded mask (in call order) and each max-pool a
gather at recorded indices: the piecewise-smooth function the fp32 pass differentiated.  `masks_from_saves` takes both from
what RedNet.forward_train saved."""
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from depth_twin import compare  # noqa: E402,F401  (the project's gradient bar, per tensor)
from rgb_twin import compare_with_allowance  # noqa: E402,F401

from oracle.rednet_ref import RedNetRef, _TransBlock  # noqa: E402

LAYERS = (3, 4, 6, 3)


class Kinks:
    """The ReLUs and max-pools of one pass: free (and recorded) or frozen to recorded masks / indices."""

    def __init__(self, masks=None, pools=None):
        self.frozen = masks is not None
        self.masks = [m.cpu() for m in masks] if self.frozen else []
        self.pools = [p.cpu() for p in pools] if pools is not None else []
        self.i = self.j = 0

    def relu(self, x):
        if not self.frozen:
            y = F.relu(x)
            self.masks.append(y.detach() > 0)
            return y
        m = self.masks[self.i]
        self.i += 1
        assert m.shape == x.shape, (self.i, m.shape, x.shape)
        return x * m.to(x.dtype)

    def pool(self, x):
        if not self.frozen:
            y, idx = F.max_pool2d(x, 3, 2, 1, return_indices=True)
            self.pools.append(idx)
            return y
        idx = self.pools[self.j]
        self.j += 1
        return x.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)

    def used_all(self):
        return not self.frozen or (self.i == len(self.masks) and self.j == len(self.pools))


def bottleneck(b, x, k):
    r = x if b.downsample is None else b.downsample(x)
    y = k.relu(b.bn1(b.conv1(x)))
    y = k.relu(b.bn2(b.conv2(y)))
    return k.relu(b.bn3(b.conv3(y)) + r)


def transblock(b, x, k):
    """oracle.rednet_ref._TransBlock.forward with the kinks routed through `k`."""
    r = x if b.upsample is None else b.upsample(x)
    y = k.relu(b.bn1(b.conv1(x)))
    return k.relu(b.bn2(b.conv2(y)) + r)


def _seq(fn, seq, x, k):
    for b in seq:
        x = fn(b, x, k)
    return x


def _agant(layer, x, k):
    return k.relu(layer[1](layer[0](x)))


class RedNetTwin(RedNetRef):
    def forward_train(self, rgb, depth, k: Kinks = None):
        """(out, out2, out3, out4, out5).  Kink order: RGB stem, depth stem, [RGB pool, depth pool], per layer the RGB blocks
        then the depth blocks (3 ReLUs each), agant4, per decoder stage its blocks (2 ReLUs each) then its agant, final_conv."""
        k = k or Kinks()
        x = k.relu(self.bn1(self.conv1(rgb)))
        d = k.relu(self.bn1_d(self.conv1_d(depth)))
        fuses = [x + d]
        x, d = k.pool(fuses[0]), k.pool(d)
        for la, lb in ((self.layer1, self.layer1_d), (self.layer2, self.layer2_d), (self.layer3, self.layer3_d),
                       (self.layer4, self.layer4_d)):
            x, d = _seq(bottleneck, la, x, k), _seq(bottleneck, lb, d, k)
            fuses.append(x + d)
            x = fuses[-1]
        x = _agant(self.agant4, fuses[4], k)
        outs = []
        for seq, head, ag, f in ((self.deconv1, self.out5_conv_custom, self.agant3, fuses[3]),
                                 (self.deconv2, self.out4_conv_custom, self.agant2, fuses[2]),
                                 (self.deconv3, self.out3_conv_custom, self.agant1, fuses[1]),
                                 (self.deconv4, self.out2_conv_custom, self.agant0, fuses[0])):
            x = _seq(transblock, seq, x, k)
            outs.append(head(x))
            x = x + _agant(ag, f, k)
        x = _seq(transblock, self.final_conv, x, k)
        out5, out4, out3, out2 = outs
        return self.final_deconv_custom(x), out2, out3, out4, out5


def golden_inputs():
    """The normalised (rgb, depth) of tests/golden/rednet_train.npz: B = 2, 64 x 64."""
    g = torch.Generator().manual_seed(11)
    return torch.randn(2, 3, 64, 64, generator=g), torch.randn(2, 1, 64, 64, generator=g)


def masks_from_saves(save):
    """(masks in RedNetTwin's kink order, [RGB pool indices, depth pool indices]) from what RedNet.forward_train(...,
    trainable="all") saved, on the CPU.  Take them before the backward runs: it overwrites the saved activations."""
    def m(t):
        return t.detach().cpu() > 0

    masks = [m(save["stem"]["out"]), m(save["stem_d"]["out"])]
    pools = [F.max_pool2d(save["fuse0"].detach().cpu(), 3, 2, 1, return_indices=True)[1],
             F.max_pool2d(save["stem_d"]["out"].detach().cpu(), 3, 2, 1, return_indices=True)[1]]
    o = 0
    for n in LAYERS:
        for blocks in (save["blocks"], save["blocks_d"]):
            for s in blocks[o:o + n]:
                masks += [m(s["l1"]["out"]), m(s["l2"]["out"]), m(s["out"])]
        o += n
    masks.append(m(save["agant"][4]["out"]))
    for k in range(4):
        masks += block_masks(save["deconv"][k])
        masks.append(m(save["agant"][3 - k]["out"]))
    masks += block_masks(save["deconv"][4])
    return masks, pools


def block_masks(blocks):
    """The two ReLU masks of each saved TransBasicBlock (rednet._transblock_train), in order."""
    out = []
    for s in blocks:
        out += [s["l1"]["out"].detach().cpu() > 0, s["out"].detach().cpu() > 0]
    return out


def build(state, dtype=torch.float64, train=True):
    net = RedNetTwin()
    net.load_state_dict({k: v.detach().cpu() for k, v in state.items()})
    net = net.to(dtype)
    for p in net.parameters():
        p.requires_grad_(True)
    return net.train(train)


def run(state, rgb, depth, d_outs, masks=None, pools=None, dtype=torch.float64, train=True):
    """One pass of the twin built from `state` (the state BEFORE the pass) under the upstream gradients d_outs of the five
    outputs -> dict(outs, grads {name: gradient}, bufs {name: buffer after the pass}, masks, pools)."""
    net = build(state, dtype, train)
    k = Kinks(masks, pools)
    outs = net.forward_train(rgb.detach().cpu().to(dtype), depth.detach().cpu().to(dtype), k)
    assert k.used_all(), "every mask and every pool index was used exactly once"
    total = sum((o * g.detach().cpu().to(dtype)).sum() for o, g in zip(outs, d_outs))
    total.backward()
    return dict(outs=[o.detach() for o in outs], grads={n: p.grad.detach() for n, p in net.named_parameters()},
                bufs={n: b.detach().clone() for n, b in net.named_buffers()}, masks=k.masks, pools=k.pools)


def fp32_error(state, rgb, depth, d_outs, train=True):
    """What torch's own fp32 pass is away from ITS frozen float64 twin on these inputs: the reference arithmetic's rounding
    noise and nothing of the code under test.  -> dict(grads {name: max|fp32 - twin|}, outs [5 figures], bufs {name: figure})"""
    r32 = run(state, rgb, depth, d_outs, dtype=torch.float32, train=train)
    r64 = run(state, rgb, depth, d_outs, r32["masks"], r32["pools"], torch.float64, train)

    def err(a, b):
        return float((a.double() - b.double()).abs().max())

    return dict(grads={n: err(g, r64["grads"][n]) for n, g in r32["grads"].items()},
                outs=[err(a, b) for a, b in zip(r32["outs"], r64["outs"])],
                bufs={n: err(b, r64["bufs"][n]) for n, b in r32["bufs"].items()})


def twin_block(inplanes, planes, upsampling):
    """One oracle TransBasicBlock in the plain (conv3x3, conv3x3, identity) or the upsampling form."""
    up = None
    if upsampling:
        up = nn.Sequential(nn.ConvTranspose2d(inplanes, planes, 2, 2, 0, bias=False), nn.BatchNorm2d(planes))
    return _TransBlock(inplanes, planes, 2 if upsampling else 1, up)


def rand_bn_(module, g):
    """BatchNorm affine pairs and running statistics away from their defaults."""
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(1.0 + 0.2 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.bias.shape, generator=g))
    return module


# ------------------------------------------------------------------------------------------------
# the trainer tests' batch, loss and CPU learner
# ------------------------------------------------------------------------------------------------
def structured_batch(B=4, H=64, seed=0, bands=4):
    """A batch a segmentation net can learn from: depth (B, H, H, 1) in [0, 1] made of a few low-frequency waves, rgb u8
    noise, label = the depth quantised into `bands` bands (u8 (B, H, H, 1))."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, H), indexing="ij")
    depth = torch.zeros(B, H, H)
    for b in range(B):
        for _ in range(3):
            fx, fy, ph = (torch.rand(3, generator=g) * torch.tensor([3.0, 3.0, 6.28])).tolist()
            depth[b] += torch.sin(6.28 * (fx * xx + fy * yy) + ph)
    depth = (depth - depth.amin()) / (depth.amax() - depth.amin())
    labels = (depth * bands).floor().clamp(0, bands - 1).to(torch.uint8)
    rgb = torch.randint(0, 256, (B, H, H, 3), generator=g, dtype=torch.uint8)
    return dict(rgb=rgb, depth=depth.unsqueeze(-1).contiguous(), semantic12=labels.unsqueeze(-1).contiguous())


def normalise(obs, dtype=torch.float64):
    """mapper.py:781-800 in `dtype`: rgb / 255 -> bilinear to the depth's size -> ImageNet normalisation; depth normalised."""
    H, W = obs["depth"].shape[1:3]
    rgb = F.interpolate(obs["rgb"].permute(0, 3, 1, 2).to(dtype) / 255.0, size=(H, W), mode="bilinear")
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=dtype).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], dtype=dtype).view(1, 3, 1, 1)
    return (rgb - mean) / std, (obs["depth"].permute(0, 3, 1, 2).to(dtype) - 0.213) / 0.285


def five_scale_loss(outs, labels_u8, class_weights=None, ignore_label=None, scale_weights=(1, 1, 1, 1, 1)):
    """The fine-tuning loss as torch states it: sum_i scale_weights[i] * F.cross_entropy(out_i, nearest-down-sampled labels)."""
    lab = labels_u8.reshape(labels_u8.shape[0], labels_u8.shape[1], labels_u8.shape[2]).long()
    total, per = 0.0, []
    for o, sw in zip(outs, scale_weights):
        s = lab.shape[1] // o.shape[2]
        per.append(F.cross_entropy(o, lab[:, ::s, ::s], weight=class_weights, reduction="mean",
                                   ignore_index=-100 if ignore_label is None else ignore_label))
        total = total + sw * per[-1]
    return total, per


def miou(pred, labels_u8, classes=13):
    """Mean IoU over the classes that occur or are predicted."""
    t, p = labels_u8.reshape(-1).long(), pred.reshape(-1).long()
    c = torch.bincount(t * classes + p, minlength=classes * classes).view(classes, classes).double()
    tp = c.diag()
    union = c.sum(0) + c.sum(1) - tp
    return float((tp[union > 0] / union[union > 0]).mean())


def twin_overfit(state, obs, lr, steps):
    """The fp32 twin with torch.optim.Adam on one fixed batch -> (losses per step, eval-mode mIoU before, after)."""
    net = build(state, torch.float32, True)
    rgb, dep = normalise(obs, torch.float32)
    opt = torch.optim.Adam(net.parameters(), lr=lr)

    def score():
        net.eval()
        with torch.no_grad():
            m = miou(net(rgb, dep).argmax(1), obs["semantic12"])
        net.train()
        return m

    before, losses = score(), []
    for _ in range(steps):
        opt.zero_grad()
        loss, _ = five_scale_loss(net.forward_train(rgb, dep), obs["semantic12"])
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, before, score()
