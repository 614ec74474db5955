"""Fine-tuning RedNet on HIP: the pixel cross-entropy over its five training outputs, segmentation metrics and a trainer.

The reference ships the network (ivlnce_baselines/common/mapping_module/rednet.py) with a five-output training forward
(:224-256) and a checkpoint fine-tuned elsewhere, but no loss and no training loop for it.  The loss is therefore defined
here: per output, torch's F.cross_entropy(weight=, ignore_index=, reduction="mean") against the labels down-sampled by
nearest neighbour to that output's size, and the total is the weighted sum of the five means (include/ivln_seg_train.h).
Forward: rednet.RedNet.forward_train; backward: train.rednet_backward; both hand-written HIP, no autograd.
The data is the stream tools/build_known_maps.py consumes: rgb u8, depth, semantic12 u8.
Training-time augmentation (scale, crop / pad, flip, saturation / value jitter - one launch from the raw frames to the
network's inputs) and median-frequency class weights: include/ivln_seg_augment.h; the records are drawn here, on the host.
"""
import math
from dataclasses import dataclass
from typing import Dict, Iterable, Optional, Sequence, Tuple

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


# ---- augmentation records and class weights (include/ivln_seg_augment.h) ---------------------------------------------
AUG_ONE = 4096  # the scale is the rational q / 4096
AUG_Q_MIN, AUG_Q_MAX = 2048, 8192


@dataclass(frozen=True)
class AugmentConfig:
    """The ranges one record per image is drawn from (RedNet's recipe without the hue scaling): scale = q / 4096, the crop
    (scale >= 1) or pad (scale < 1) offset uniform over its valid range, a horizontal flip with probability `flip`, and the
    photometry c' = clamp(gain * max(v - saturation * (v - c), 0) + offset, 0, 255), v = max(r, g, b), on the 0..255 scale."""
    scale: Tuple[float, float] = (1.0, 1.4)
    flip: float = 0.5
    saturation: Tuple[float, float] = (0.9, 1.1)
    gain: Tuple[float, float] = (0.9, 1.1)
    offset: Tuple[float, float] = (-25.0, 25.0)

    def validate(self, ignore_label=None):
        for name in ("scale", "saturation", "gain", "offset"):
            r = getattr(self, name)
            if len(r) != 2 or not all(math.isfinite(float(x)) for x in r) or float(r[0]) > float(r[1]):
                raise ValueError(f"AugmentConfig.{name}: a finite (low, high) with low <= high, got {r}")
        if self.scale[0] * AUG_ONE < AUG_Q_MIN or self.scale[1] * AUG_ONE > AUG_Q_MAX:
            raise ValueError(f"AugmentConfig.scale inside [0.5, 2], got {self.scale}")
        if not 0.0 <= float(self.flip) <= 1.0:
            raise ValueError(f"AugmentConfig.flip is a probability, got {self.flip}")
        if self.saturation[0] < 0 or self.gain[0] < 0:
            raise ValueError("AugmentConfig: saturation and gain are not negative")
        if self.scale[0] < 1.0 and ignore_label is None:
            raise ValueError("AugmentConfig.scale[0] < 1 pads the frame: the padded pixels need an ignore_label")
        return self


def scaled_size(n: int, q: int) -> int:
    return (n * q + AUG_ONE // 2) // AUG_ONE


def offset_range(n: int, q: int) -> Tuple[int, int]:
    """The valid (low, high) of an offset along an axis of n pixels at scale q / 4096: a crop window or a pad."""
    d = scaled_size(n, q) - n
    return (0, d) if d >= 0 else (d, 0)


def sample_augment(cfg: AugmentConfig, B: int, H: int, W: int, generator: torch.Generator):
    """One record per image -> (geom int32 (B, 4) {q, oy, ox, flip}, photo f32 (B, 4) {ks, kv, dv, 0}) on the CPU.  Seven
    float64 uniforms per image from `generator`, everything after them in Python integers and doubles: the same seed gives
    the same records on any machine."""
    u = torch.rand(B, 7, generator=generator, dtype=torch.float64).tolist()
    geom = torch.zeros(B, 4, dtype=torch.int32)
    photo = torch.zeros(B, 4, dtype=torch.float32)

    def span(r, x):
        return float(r[0]) + x * (float(r[1]) - float(r[0]))

    def pick(lo, hi, x):  # an integer of [lo, hi], uniform
        return min(lo + int(x * (hi - lo + 1)), hi)

    for b, (us, uy, ux, uf, uk, ug, uo) in enumerate(u):
        q = min(max(int(math.floor(span(cfg.scale, us) * AUG_ONE + 0.5)), AUG_Q_MIN), AUG_Q_MAX)
        geom[b] = torch.tensor([q, pick(*offset_range(H, q), uy), pick(*offset_range(W, q), ux), int(uf < float(cfg.flip))],
                               dtype=torch.int32)
        photo[b] = torch.tensor([span(cfg.saturation, uk), span(cfg.gain, ug), span(cfg.offset, uo), 0.0], dtype=torch.float64)
    return geom, photo


def class_counts(batches: Iterable[Dict], classes: int, ignore_label: Optional[int] = None):
    """batches of observations -> (pixels, present) int64 (classes,) on the host: pixels[c] = the pixels of class c,
    present[c] = the labelled pixels of the images in which c occurs (ops.seg_class_counts)."""
    pixels = present = None
    dev = None
    for batch in batches:
        labels = _labels3(batch["semantic12"])
        dev = labels.device
        pixels, present = ops.seg_class_counts(labels, classes, ignore_label, pixels, present, check_labels=False)
    if pixels is None:
        raise ValueError("class_counts: no batches")
    ops.seg_check(dev, "class_counts")
    return pixels.cpu(), present.cpu()


def median_frequency_weights(pixels, present) -> torch.Tensor:
    """Median-frequency balancing, on the host in double: freq_c = pixels_c / present_c over the classes with pixels_c > 0,
    w_c = median(freq) / freq_c; a class never seen keeps w_c = 1.  -> f32 (C,)."""
    px = np.asarray(pixels.cpu() if torch.is_tensor(pixels) else pixels, dtype=np.float64)
    pr = np.asarray(present.cpu() if torch.is_tensor(present) else present, dtype=np.float64)
    if px.shape != pr.shape or px.ndim != 1:
        raise ValueError(f"median_frequency_weights: two vectors of one length, got {px.shape} and {pr.shape}")
    seen = px > 0
    if (pr[seen] <= 0).any():
        raise ValueError("median_frequency_weights: a class with pixels occurs in no image")
    w = np.ones_like(px)
    if seen.any():
        freq = px[seen] / pr[seen]
        w[seen] = np.median(freq) / freq
    return torch.from_numpy(w.astype(np.float32))


def checkpoint_dict(model: RedNet) -> Dict:
    """What `save` writes: the key PredictSemantics.setup and the reference's load_model (mapper.py:758-761) read."""
    return {"model_state": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}}


class RedNetTrainer:
    """One Adam step per `step(observations)` on RedNet's five-output loss.  trainable="decoder" keeps the two encoders
    frozen (their folded forward, no saves, no gradients, parameters and buffers untouched).  augment: `step` draws one
    record per image (sample_augment, a CPU generator seeded with `seed`) and trains on ops.seg_augment's outputs; None: the
    raw frames.  `inputs`, `predict` and `evaluate` never augment."""

    def __init__(self, model: RedNet, lr: float = 2e-4, trainable: str = "all", class_weights=None, ignore_label=None,
                 scale_weights: Sequence[float] = SCALE_WEIGHTS, augment: Optional[AugmentConfig] = None, seed: int = 0):
        self.augment = None if augment is None else augment.validate(ignore_label)
        self._gen = torch.Generator().manual_seed(int(seed))
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
    def loss_and_gradients(self, observations, records=None):
        """Forward, loss and backward without the update -> (loss tensor (1,), per-scale tensor, G).  records = (geom, photo)
        of sample_augment: the network and the loss see ops.seg_augment's (rgb, depth, labels) instead of the raw frames."""
        if records is None:
            rgb, dn = self.inputs(observations)
            labels = observations["semantic12"]
        else:
            rgb, dn, labels = ops.seg_augment(observations["rgb"].to(torch.uint8).contiguous(),
                                              observations["depth"].to(torch.float32).contiguous(),
                                              _labels3(observations["semantic12"]), records[0], records[1], self.ignore_label)
        save: Dict = {}
        outs = self.model.forward_train(rgb, dn, save, trainable=self.trainable)
        # (forward_train has voided the folded cache where a train-mode BatchNorm moved its running statistics)
        loss, per, d_outs = seg_loss(outs, labels, self.class_weights, self.ignore_label, self.scale_weights)
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
        records = None
        if self.augment is not None:
            B, H, W = observations["depth"].shape[:3]
            records = sample_augment(self.augment, int(B), int(H), int(W), self._gen)
        loss, per, G = self.loss_and_gradients(observations, records)
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
