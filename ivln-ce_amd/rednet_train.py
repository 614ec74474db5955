"""Fine-tuning RedNet on HIP: the pixel cross-entropy over its five training outputs, segmentation metrics and a trainer.

The reference ships the network (ivlnce_baselines/common/mapping_module/rednet.py) with a five-output training forward
(:224-256) and a checkpoint fine-tuned elsewhere, but no loss and no training loop for it.  The loss is therefore defined
here: per output, torch's F.cross_entropy(weight=, ignore_index=, reduction="mean") against the labels down-sampled by
nearest neighbour to that output's size, and the total is the weighted sum of the five means (include/ivln_seg_train.h).
Forward: rednet.RedNet.forward_train; backward: train.rednet_backward; both hand-written HIP, no autograd.
The data is the stream tools/build_known_maps.py consumes: rgb u8, depth, semantic12 u8.
"""
from typing import Dict, Iterable, Optional, Sequence

import numpy as np
import torch

from . import ops, train
from .rednet import PredictSemantics, RedNet
from .trainers import FlatAdam

SCALE_WEIGHTS = (1.0, 1.0, 1.0, 1.0, 1.0)


def _labels3(labels):
    """(B, H, W, 1) | (B, 1, H, W) | (B, H, W) u8 -> (B, H, W) contiguous (a view where the memory already is that)."""
    if labels.dtype != torch.uint8:
        raise ValueError(f"labels are uint8 class indices, got {labels.dtype}")
    if labels.dim() == 4:
        if labels.shape[-1] == 1:
            labels = labels[..., 0]
        elif labels.shape[1] == 1:
            labels = labels[:, 0]
        else:
            raise ValueError(f"labels (B, H, W, 1), got {tuple(labels.shape)}")
    if labels.dim() != 3:
        raise ValueError(f"labels (B, H, W), got {tuple(labels.shape)}")
    return labels.contiguous()


def _strides(outs, labels):
    """The integer factor between the labels and every output; anything else is refused before a launch."""
    B, H, W = labels.shape
    strides = []
    for i, o in enumerate(outs):
        if o.dim() != 4 or o.shape[0] != B:
            raise ValueError(f"output {i}: (B = {B}, classes, h, w), got {tuple(o.shape)}")
        h, w = int(o.shape[2]), int(o.shape[3])
        s = H // h if h > 0 else 0
        if s < 1 or h * s != H or w * s != W:
            raise ValueError(f"output {i} is {h} x {w}: not {H} x {W} labels divided by one integer")
        strides.append(s)
    return strides


def seg_loss(outs: Sequence[torch.Tensor], labels: torch.Tensor, class_weights: Optional[torch.Tensor] = None,
             ignore_label: Optional[int] = None, scale_weights: Sequence[float] = SCALE_WEIGHTS):
    """outs = RedNet.forward_train's (out, out2, out3, out4, out5) (any number of score maps at H / s), labels u8 at full
    resolution -> (loss, per-scale losses, d_outs): loss (1,) = sum_i scale_weights[i] * CE_i on the device, the per-scale
    means (len(outs),) on the device, d_outs[i] = d loss / d outs[i].  A scale whose pixels are all ignored contributes 0
    (torch: NaN).  A label outside [0, classes) that is not `ignore_label` raises; nothing was written then."""
    labels = _labels3(labels)
    strides = _strides(outs, labels)
    if len(scale_weights) != len(outs):
        raise ValueError(f"{len(outs)} outputs, {len(scale_weights)} scale weights")
    dev = outs[0].device
    if class_weights is not None:
        class_weights = class_weights.to(device=dev, dtype=torch.float32).contiguous()
    per = torch.empty(len(outs), dtype=torch.float32, device=dev)
    d_outs = []
    for i, (o, s, sw) in enumerate(zip(outs, strides, scale_weights)):
        _, d = ops.seg_ce(o.contiguous(), labels, s, class_weights, ignore_label, scale=float(sw), loss=per[i:i + 1],
                          check_labels=False)
        d_outs.append(d)
    ops.seg_check(dev, "seg_loss")
    sw = torch.tensor([float(x) for x in scale_weights], dtype=torch.float64)
    total = (per.detach().cpu().double() * sw).sum().to(torch.float32).reshape(1)  # (five numbers: on the host, in double)
    return total, per, d_outs


def metrics_from_counts(counts) -> Dict:
    """(C, C) confusion counts [truth][prediction] -> pixel accuracy, per-class IoU (nan for a class that neither occurs nor
    is predicted) and their mean over the classes that do."""
    c = np.asarray(counts.detach().cpu() if torch.is_tensor(counts) else counts, dtype=np.float64)
    tp = np.diag(c)
    total = c.sum()
    union = c.sum(0) + c.sum(1) - tp
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.where(union > 0, tp / union, np.nan)
    seen = union > 0
    return dict(pixel_acc=float(tp.sum() / total) if total > 0 else float("nan"), iou=iou,
                miou=float(iou[seen].mean()) if seen.any() else float("nan"), counts=c.astype(np.int64))


def checkpoint_dict(model: RedNet) -> Dict:
    """What `save` writes: the key PredictSemantics.setup and the reference's load_model (mapper.py:758-761) read."""
    return {"model_state": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}}


class RedNetTrainer:
    """One Adam step per `step(observations)` on RedNet's five-output loss.  trainable="decoder" keeps the two encoders
    frozen (their folded forward, no saves, no gradients, parameters and buffers untouched)."""

    def __init__(self, model: RedNet, lr: float = 2e-4, trainable: str = "all", class_weights=None, ignore_label=None,
                 scale_weights: Sequence[float] = SCALE_WEIGHTS):
        names = {k for k, _ in model.trainable_parameters(trainable)}
        for k, p in model.named_parameters():
            p.requires_grad_(k in names)
        self.model, self.trainable = model, trainable
        self.opt = FlatAdam(model, lr=lr)
        assert set(self.opt.names) == names
        self._void_folded()  # (the parameters moved into the optimizer's flat bucket)
        self._ps = PredictSemantics(next(model.parameters()).device, model=model)
        dev = next(model.parameters()).device
        self.class_weights = None if class_weights is None else torch.as_tensor(class_weights, dtype=torch.float32).to(dev)
        self.ignore_label, self.scale_weights = ignore_label, tuple(float(x) for x in scale_weights)
        self.classes = model.final_deconv_custom.out_channels
        self.last_per_scale = None

    @staticmethod
    def inputs(observations):
        """The normalised (rgb, depth) PredictSemantics.scores feeds the network, and the labels."""
        depth = observations["depth"].to(torch.float32).contiguous()  # (B, H, W, 1)
        B, H, W, _ = depth.shape
        rgb = ops.rgb_resize_normalize(observations["rgb"].to(torch.uint8).contiguous(), H, W)
        return rgb, ops.affine(depth.view(B, 1, H, W), 0.213, 0.285)

    @torch.no_grad()
    def loss_and_gradients(self, observations):
        """Forward, loss and backward without the update -> (loss tensor (1,), per-scale tensor, G)."""
        rgb, dn = self.inputs(observations)
        save: Dict = {}
        outs = self.model.forward_train(rgb, dn, save, trainable=self.trainable)
        # (forward_train has voided the folded cache where a train-mode BatchNorm moved its running statistics)
        loss, per, d_outs = seg_loss(outs, observations["semantic12"], self.class_weights, self.ignore_label, self.scale_weights)
        G: Dict = {}
        train.rednet_backward(self.model, save, d_outs, G)
        return loss, per, G

    def _void_folded(self):
        self.model.invalidate_folded()
        ops.WEIGHT_EPOCH += 1

    @torch.no_grad()
    def step(self, observations) -> float:
        """rgb u8 (B, h, w, 3), depth (B, H, W, 1), semantic12 u8 (B, H, W, 1): one update; returns the loss as a float
        (`last_per_scale`: the five per-scale means as floats)."""
        loss, per, G = self.loss_and_gradients(observations)
        missing = [k for k, p in zip(self.opt.names, self.opt.params) if p not in G]
        if missing:
            raise RuntimeError(f"rednet_backward left {len(missing)} trainable parameters without a gradient: {missing[:3]}")
        ops.add_multi([(G[p].contiguous(), p.grad) for p in self.opt.params])
        self.opt.step()  # (bumps ops.WEIGHT_EPOCH: PredictSemantics plans rebuild on their own)
        self.model.invalidate_folded()
        self.last_per_scale = [float(x) for x in per.cpu()]
        return float(loss)

    @torch.no_grad()
    def predict(self, observations):
        """The frozen forward's labels (B, 1, H, W) u8 - what the mapper would see with these weights."""
        was = self.model.training
        self.model.eval()
        try:
            return self._ps(observations)
        finally:
            self.model.train(was)

    @torch.no_grad()
    def evaluate(self, batches: Iterable[Dict]) -> Dict:
        """The frozen forward plus confusion counts over `batches` of observations -> dict(pixel_acc, iou, miou, counts)."""
        counts = None
        for obs in batches:
            pred = self.predict(obs)
            truth = _labels3(obs["semantic12"])
            counts = ops.seg_confusion(pred.view(-1), truth.view(-1), self.classes, self.ignore_label, counts=counts)
        if counts is None:
            raise ValueError("evaluate: no batches")
        return metrics_from_counts(counts)

    def save(self, path):
        torch.save(checkpoint_dict(self.model), path)
