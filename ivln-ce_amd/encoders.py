"""Encoders of the MapCMA policy with the reference's module / parameter names, forward on HIP.

torch.nn modules are used ONLY as parameter containers (identical `state_dict()` keys, init,
`.to()/.train()/.eval()` semantics); every forward below calls the HIP kernels through ops.py.

  SemanticMapEncoder / CBRA   ivlnce_baselines/models/encoders/map_encoder.py:8-97
  InstructionEncoder          ivlnce_baselines/models/encoders/instruction_encoder.py:11-94
  VlnResnetDepthEncoder       ivlnce_baselines/models/encoders/resnet_encoders.py:17-115
  ResNetEncoder / resnet50    habitat-lab v0.1.7 ddppo policy (un-vendored)
  RNNStateEncoder             habitat-lab v0.1.7 rnn_state_encoder (Appendix A.2)
"""
import gzip
import json
from typing import Optional

import torch
import torch.nn as nn

from . import depth_net, ops


# ------------------------------------------------------------------------------------------------
# Semantic map encoder
# ------------------------------------------------------------------------------------------------
class CBRA(nn.Module):
    """Conv(7x7 same) -> BatchNorm -> ReLU -> AvgPool(2)."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv = nn.Sequential(
            nn.Conv2d(in_channels, out_channels, kernel_size=7, padding=3),
            nn.BatchNorm2d(out_channels),
            nn.ReLU(inplace=True),
            nn.AvgPool2d(2),
        )

    def forward_hip(self, x, save=None):
        conv, bn = self.conv[0], self.conv[1]
        # train mode: the conv's epilogue leaves per-tile {count, mean, M2} of what it stores, so the BatchNorm statistics
        # need no pass of their own over y (two reads of the largest tensors of the update)
        stats = [] if (bn.training and ops.CONV_STATS) else None
        y = ops.conv2d(x, conv.weight, stride=1, pad=3, shift=conv.bias, stats=stats)
        C = bn.num_features
        scale = torch.empty(C, dtype=torch.float32, device=x.device)
        shift = torch.empty(C, dtype=torch.float32, device=x.device)
        if bn.training:
            sm = sr = None
            if save is not None:
                sm = torch.empty(C, dtype=torch.float32, device=x.device)
                sr = torch.empty(C, dtype=torch.float32, device=x.device)
            if stats:
                ops.bn_stats_from_partials(stats[0][0], stats[0][1], bn, scale, shift, sm, sr)
            else:  # (the launch went another way - split K, scalar-gather GEMM: statistics from y)
                ops.bn_train_stats(y, bn, scale, shift, sm, sr)
            if bn.num_batches_tracked is not None:
                bn.num_batches_tracked += 1
            if save is not None:
                save.append(dict(x=x, y=y, scale=scale, shift=shift, mean=sm, rstd=sr, train=True))
        else:
            ops.bn_fold(bn, scale, shift)
            if save is not None:
                save.append(dict(x=x, y=y, scale=scale, shift=shift, train=False))
        return ops.scale_shift_relu_avgpool2(y, scale, shift)

    def _folded(self):
        """Eval-mode BatchNorm folded with the conv bias, cached until the weights change."""
        conv, bn = self.conv[0], self.conv[1]
        key = (ops.WEIGHT_EPOCH, bn.weight._version, bn.bias._version, bn.running_mean._version,
               bn.running_var._version, conv.bias._version, bn.weight.data_ptr())
        if getattr(self, "_fold_key", None) != key:
            C = bn.num_features
            scale = torch.empty(C, dtype=torch.float32, device=bn.weight.device)
            shift = torch.empty(C, dtype=torch.float32, device=bn.weight.device)
            ops.bn_fold(bn, scale, shift, conv.bias)
            self._fold_key, self._fold = key, (scale, shift)
        return self._fold

    def forward_infer(self, x):
        """Rollout path (BatchNorm in eval mode, nothing saved): conv leaves raw split-K slabs, one
        kernel reduces them + folded BN + ReLU + AvgPool: 2 launches per block."""
        scale, shift = self._folded()
        return ops.scale_shift_relu_avgpool2(ops.conv2d(x, self.conv[0].weight, pad=3, defer=True), scale, shift)


    def forward_fused(self, x, maps_u8=None):
        """Rollout path, one launch per block (ops.conv7_bn_relu_pool): the conv reduces K inside its workgroups and applies
        folded BN + ReLU + AvgPool in its epilogue; `maps_u8` = the first block's u8 (occupancy, labels) instead of `x`.
        None: the library declined the shape - the caller takes `forward_infer`."""
        conv = self.conv[0]
        if conv.kernel_size != (7, 7) or conv.stride != (1, 1) or conv.padding != (3, 3) or conv.dilation != (1, 1) or conv.groups != 1:
            return None
        scale, shift = self._folded()
        return ops.conv7_bn_relu_pool(x, conv.weight, scale, shift, maps_u8=maps_u8)


MAP_CNN_FUSED = True  # A/B, tests: False = the rollout's map CNN as conv (raw split-K slabs) + reducing tail, two launches per block


class SemanticMapEncoder(nn.Module):
    def __init__(self, observation_space, num_semantic_classes: int = 13, ch: int = 32, last_ch_mult: int = 8,
                 trainable: bool = True, from_pretrained: bool = False, checkpoint: Optional[str] = None):
        super().__init__()
        for k in ["occupancy_map", "semantic_map"]:
            if k not in observation_space.spaces:
                raise ValueError(f"key `{k}` expected in observation space.")
        self._map_dimensions = observation_space.spaces["occupancy_map"].shape
        self._num_semantic_classes = num_semantic_classes
        self.last_ch_mult = last_ch_mult
        self._ch = ch
        self.cnn = nn.Sequential(CBRA(14, ch), CBRA(ch, ch * 2), CBRA(ch * 2, ch * 4), CBRA(ch * 4, ch * last_ch_mult))
        if from_pretrained:
            ckpt = torch.load(checkpoint, map_location="cpu")["state_dict"]
            prefix = "encoder.cnn."
            self.cnn.load_state_dict({k[len(prefix):]: v for k, v in ckpt.items() if k.startswith(prefix)})
        for param in self.cnn.parameters():
            param.requires_grad_(trainable)
        if not trainable:
            self.eval()

    @property
    def output_shape(self):
        return (self._ch * self.last_ch_mult, self._map_dimensions[0] // 16, self._map_dimensions[1] // 16)

    def generate_map_features(self, observations):
        occ = observations["occupancy_map"].to(torch.uint8).contiguous()
        sem = observations["semantic_map"].to(torch.uint8).contiguous()
        return ops.map_features(occ, sem, self._num_semantic_classes)

    def forward(self, observations, save=None):
        for k in ["occupancy_map", "semantic_map"]:
            if k not in observations:
                raise ValueError(f"Observation `{k}` is missing.")
        x = None
        for k, blk in enumerate(self.cnn):
            infer = save is None and not blk.conv[1].training
            y = None
            if infer and MAP_CNN_FUSED:
                if k == 0 and self._num_semantic_classes == 13:  # (the u8 maps themselves: no feature tensor)
                    occ = observations["occupancy_map"].to(torch.uint8).contiguous()
                    sem = observations["semantic_map"].to(torch.uint8).contiguous()
                    if occ.dim() == 3 and sem.dim() == 3:
                        y = blk.forward_fused(None, maps_u8=(occ, sem))
                if y is None:
                    if k == 0:
                        x = self.generate_map_features(observations)
                    y = blk.forward_fused(x)
            if y is None:
                if k == 0 and x is None:
                    x = self.generate_map_features(observations)
                y = blk.forward_infer(x) if infer else blk.forward_hip(x, save)
            x = y
        return x


# ------------------------------------------------------------------------------------------------
# Instruction encoder
# ------------------------------------------------------------------------------------------------
class InstructionEncoder(nn.Module):
    """instruction_encoder.py:11-94.  `rnn_type` selects nn.GRU or nn.LSTM and `bidirectional` the direction count (:27-32);
    the output width is hidden_size * (1 + bidirectional) (:49).  The torch module only holds the parameters, so the
    state-dict keys are the reference's: no `*_reverse` entries when unidirectional."""

    def __init__(self, config) -> None:
        super().__init__()
        self.config = config
        kind = str(config.rnn_type).upper()
        if kind not in ("GRU", "LSTM"):
            raise ValueError(f"MODEL.INSTRUCTION_ENCODER.rnn_type must be GRU or LSTM, got {config.rnn_type!r}")
        rnn = nn.GRU if kind == "GRU" else nn.LSTM
        self.encoder_rnn = rnn(input_size=config.embedding_size, hidden_size=config.hidden_size,
                               bidirectional=bool(config.bidirectional))
        if config.sensor_uuid == "instruction":
            if config.use_pretrained_embeddings:
                self.embedding_layer = nn.Embedding.from_pretrained(
                    embeddings=self._load_embeddings(), freeze=not config.fine_tune_embeddings
                )
            else:
                self.embedding_layer = nn.Embedding(
                    num_embeddings=config.vocab_size, embedding_dim=config.embedding_size, padding_idx=0
                )

    @property
    def output_size(self):
        return self.config.hidden_size * (1 + int(bool(self.config.bidirectional)))

    @property
    def uses_features(self):
        """The sensor delivers pre-computed (L, E) text features, not token ids: any sensor_uuid but "instruction"
        (instruction_encoder.py:34-45) - no embedding layer exists and W_ih reads the features directly."""
        return self.config.sensor_uuid != "instruction"

    @property
    def obs_key(self):
        """The observation the encoder reads (instruction_encoder.py:70-76)."""
        return "rxr_instruction" if self.uses_features else "instruction"

    @property
    def is_gru(self):
        return isinstance(self.encoder_rnn, nn.GRU)

    @property
    def ndir(self):
        return 2 if self.encoder_rnn.bidirectional else 1

    @property
    def gates(self):
        """Gate rows per hidden unit: 3 (GRU: r, z, n) or 4 (LSTM: i, f, g, o)."""
        return 3 if self.is_gru else 4

    def dir_params(self, stem):
        """The `stem` parameter ("weight_ih", "weight_hh", "bias_ih", "bias_hh") of every direction that exists:
        (forward,) or (forward, reverse)."""
        rnn = self.encoder_rnn
        names = (stem + "_l0",) if self.ndir == 1 else (stem + "_l0", stem + "_l0_reverse")
        return tuple(getattr(rnn, n) for n in names)

    def _load_embeddings(self):
        with gzip.open(self.config.embedding_file, "rt") as f:
            return torch.tensor(json.load(f))

    def _gate_table(self):
        """(table (V, ndir * gates * H), row_nonzero u8 (V)) of ivln_embed_gates_dirs_f32, cached until a weight changes; None
        while a stream capture is running and no valid table exists (the caller then runs the unfolded launches)."""
        E = self.embedding_layer.weight
        ws, bs = self.dir_params("weight_ih"), self.dir_params("bias_ih")
        ps = (E,) + ws + bs
        key = (ops.WEIGHT_EPOCH,) + tuple(p._version for p in ps) + tuple(p.data_ptr() for p in ps)
        c = self.__dict__.get("_gate_cache")
        if c is None or c[0] != key:
            if torch.cuda.is_current_stream_capturing():
                return None
            with torch.no_grad():
                W = torch.cat(list(ws)).contiguous()
                b = torch.cat(list(bs)).contiguous()
                table = ops.linear_gemm(E.detach().contiguous(), W, b)
                nz = (E.detach() != 0).any(dim=1).to(torch.uint8).contiguous()
            c = self.__dict__["_gate_cache"] = (key, (table, nz))
        return c[1]

    def step_cache(self, rows, L, device, feat=None):
        """The per-episode cache of a rollout batch shape (ops.InstructionStepCache), or None: switched off, a capture in
        progress that would have to create or invalidate it (the warm-up steps before a capture do that), no folded table.
        A cache made for other weights (recurrent / embedding versions, ops.WEIGHT_EPOCH) is invalidated, not rebuilt:
        captured graphs hold its buffers.  The key names the recurrent parameters that exist for the combination.
        `feat` = E: the feature flavour (`uses_features`), which compares (L, E) features instead of tokens."""
        if not ops.CACHE_INSTRUCTION:
            return None
        gate_key = (self.__dict__.get("_gate_cache") or (None,))[0]
        rnn = self.encoder_rnn
        ws, bs = self.dir_params("weight_hh"), self.dir_params("bias_hh")
        ps = ws + bs
        if feat is not None:  # (no folded table: the input-side weights are read at every re-encoding, so they key the cache)
            gate_key = ops.WEIGHT_EPOCH
            ps = ps + self.dir_params("weight_ih") + self.dir_params("bias_ih")
        key = (gate_key,) + tuple(p._version for p in ps) + tuple(p.data_ptr() for p in ps)
        caches = self.__dict__.setdefault("_step_caches", {})
        shape = (rows, L, str(device)) if feat is None else (rows, L, str(device), int(feat))
        c = caches.get(shape)
        capturing = torch.cuda.is_current_stream_capturing()
        if c is None:
            if capturing:
                return None
            if len(caches) >= 4:  # (batch shapes come and go as envs pause: keep the table small)
                caches.pop(next(iter(caches)))
            c = caches[shape] = ops.InstructionStepCache(rows, L, self.gates * rnn.hidden_size, rnn.hidden_size, device, key,
                                                         ndir=self.ndir, feat=feat)
        elif c.key != key:
            if capturing:
                return None
            c.invalidate()
            c.key = key
        return c

    def _recurrence(self, gx_f, gx_r, lengths, B, L, save=False, cache=None):
        """The packed-sequence recurrence of the configured cell and direction count -> (out (B, ndir*H, L), saves dict)."""
        H, nd = self.encoder_rnn.hidden_size, self.ndir
        whh, bhh = self.dir_params("weight_hh"), self.dir_params("bias_hh")
        whh_r, bhh_r = (whh[1], bhh[1]) if nd == 2 else (None, None)
        if self.is_gru:
            # (no ticket / spare form of the GRU kernel: graphed.py leaves lstm_spare at 1 for a GRU encoder)
            out, sv = ops.gru_dirs(gx_f, gx_r, whh[0], whh_r, bhh[0], bhh_r, lengths, B, L, H, ndir=nd, save=save, cache=cache)
            return out, dict(gru=sv)
        out, gates, cs = ops.lstm_bidir(gx_f, gx_r, whh[0], whh_r, bhh[0], bhh_r, lengths, B, L, H, save=save,
                                        spare=getattr(self, "lstm_spare", 1), ticket=getattr(self, "lstm_ticket", None),
                                        cache=cache, ndir=nd)
        return out, dict(gates=gates, cs=cs)

    def forward(self, observations, save=None):
        """(B, L) tokens -> (B, ndir*H, L) channel-major outputs, zero for t >= length; also returns
        lengths (device int32).  The reference returns (B, ndir*H, Lmax); the extra columns here are
        exactly the masked (zero-weight) attention positions.
        Rollout steps (no `save`, no autograd): the encoding is cached per row and recomputed only where the tokens
        changed (`step_cache`; the decision is taken on the device, ops.embed_gates) - `self.last_cache` then names the
        cache whose `dirty` flags belong to this call, else it is None."""
        if self.uses_features:
            return self._forward_features(observations, save)
        tokens = observations["instruction"].long().contiguous()
        B, L = tokens.shape
        nd = self.ndir
        fold = self._gate_table() if (save is None and ops.FOLD_INSTRUCTION_GATES) else None
        self.last_cache = None
        if fold is not None and tokens.is_cuda and not torch.is_grad_enabled():
            cache = self.step_cache(B, L, tokens.device)
            if cache is not None:
                gx_f, gx_r, lengths = ops.embed_gates(tokens, *fold, cache=cache, ndir=nd)
                out, _ = self._recurrence(gx_f, gx_r, lengths, B, L, cache=cache)
                self.last_cache = cache
                return out, lengths
        if fold is not None:  # inference: embedding lookup + the W_ih projections = one lookup in a folded table
            emb = None
            gx_f, gx_r, lengths = ops.embed_gates(tokens, *fold, ndir=nd)
        else:
            emb, lengths = ops.embed_lengths(tokens, self.embedding_layer.weight)
            wih, bih = self.dir_params("weight_ih"), self.dir_params("bias_ih")
            gx_f = ops.linear_gemm(emb, wih[0], bih[0])
            gx_r = ops.linear_gemm(emb, wih[1], bih[1]) if nd == 2 else None
        out, sv = self._recurrence(gx_f, gx_r, lengths, B, L, save=save is not None)
        if save is not None:
            save.update(emb=emb, lengths=lengths, out=out, tokens=tokens, **sv)
        return out, lengths


    def _forward_features(self, observations, save=None):
        """`forward` for pre-computed features: observations["rxr_instruction"] (B, L, E) f32 (instruction_encoder.py:74-78).  lengths = the
        number of non-zero rows and the recurrence runs over the first `lengths[b]` rows, as pack_padded_sequence does.
        Update pass (`save`): ops.linear_gemm per direction; save["emb"] is the feature matrix itself, no save["tokens"].
        Rollout pass: the step cache compares features on the device (ops.text_feat_front) and only the dirty rows are
        projected and re-run.  Cached and uncached calls share the projection kernel, so they agree byte for byte."""
        feat = observations[self.obs_key].to(torch.float32).contiguous()
        if feat.dim() != 3 or feat.shape[2] != self.encoder_rnn.input_size:
            raise ValueError(f"`{self.obs_key}` must be (B, L, {self.encoder_rnn.input_size}) features, got {tuple(feat.shape)}")
        B, L, E = feat.shape
        nd = self.ndir
        wih, bih = self.dir_params("weight_ih"), self.dir_params("bias_ih")
        self.last_cache = None
        if save is not None:
            lengths = ops.text_feat_front(feat)
            emb = feat.view(B * L, E)
            gx_f = ops.linear_gemm(emb, wih[0], bih[0])
            gx_r = ops.linear_gemm(emb, wih[1], bih[1]) if nd == 2 else None
            out, sv = self._recurrence(gx_f, gx_r, lengths, B, L, save=True)
            save.update(emb=emb, lengths=lengths, out=out, **sv)
            return out, lengths
        if feat.is_cuda and not torch.is_grad_enabled():
            cache = self.step_cache(B, L, feat.device, feat=E)
            if cache is not None:
                lengths = ops.text_feat_front(feat, cache=cache)
                ops.text_feat_gates(feat, wih[0], bih[0], dirty=cache.dirty, out=cache.gx_f)
                if nd == 2:
                    ops.text_feat_gates(feat, wih[1], bih[1], dirty=cache.dirty, out=cache.gx_r)
                out, _ = self._recurrence(cache.gx_f, cache.gx_r, lengths, B, L, cache=cache)
                self.last_cache = cache
                return out, lengths
        lengths = ops.text_feat_front(feat)
        gx_f = ops.text_feat_gates(feat, wih[0], bih[0])
        gx_r = ops.text_feat_gates(feat, wih[1], bih[1]) if nd == 2 else None
        out, _ = self._recurrence(gx_f, gx_r, lengths, B, L)
        return out, lengths


# ------------------------------------------------------------------------------------------------
# DD-PPO depth ResNet50 (GroupNorm), parameter tree named like habitat-lab's
# ------------------------------------------------------------------------------------------------
def _conv(cin, cout, k, stride=1, pad=0):
    return nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=pad, bias=False)


# MODEL.DEPTH_ENCODER.backbone (resnet_encoders.py:41 hands the key to getattr(resnet, backbone)): name -> (blocks per
# layer, ResNeXt bottlenecks, squeeze-and-excite tails) of habitat-lab v0.1.7 rl/ddppo/policy/resnet.py
DEPTH_BACKBONES = {
    "resnet50": ((3, 4, 6, 3), False, False),
    "resneXt50": ((3, 4, 6, 3), True, False),
    "se_resnet50": ((3, 4, 6, 3), False, True),
    "se_resneXt50": ((3, 4, 6, 3), True, True),
    "se_resneXt101": ((3, 4, 23, 3), True, True),
}


def depth_backbone_spec(backbone):
    """-> (blocks per layer, resneXt, se); ValueError for any other name (resnet18 has another block and is not built)."""
    spec = DEPTH_BACKBONES.get(backbone)
    if spec is None:
        raise ValueError(f"MODEL.DEPTH_ENCODER.backbone must be one of {', '.join(DEPTH_BACKBONES)}; got {backbone!r}")
    return spec


class _SE(nn.Module):
    """habitat-lab's SE branch: squeeze = global average pool, excite = Linear(C, C/r) - ReLU - Linear(C/r, C) - Sigmoid.
    The HIP path never calls it as a module: ops.se_gate reads its parameters (state-dict keys se.excite.{0,2}.*)."""

    def __init__(self, planes, r=16):
        super().__init__()
        self.squeeze = nn.AdaptiveAvgPool2d(1)
        self.excite = nn.Sequential(nn.Linear(planes, int(planes / r)), nn.ReLU(True), nn.Linear(int(planes / r), planes),
                                    nn.Sigmoid())


class _Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, ngroups, stride=1, downsample=None, expansion=4, cardinality=1, se=False):
        super().__init__()
        self.expansion = expansion
        self.convs = nn.Sequential(
            _conv(inplanes, planes, 1), nn.GroupNorm(ngroups, planes), nn.ReLU(True),
            nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False, groups=cardinality),
            nn.GroupNorm(ngroups, planes), nn.ReLU(True),
            _conv(planes, planes * expansion, 1), nn.GroupNorm(ngroups, planes * expansion),
        )
        if se:
            self.se = _SE(planes * expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    @property
    def plain(self):
        """The ResNet-50 bottleneck: dense 3x3 conv, no SE branch - what the chain, nconv, persistent and training forms
        are written for.  Anything else runs the conv + GroupNorm pair form only."""
        return self.convs[3].groups == 1 and getattr(self, "se", None) is None

    def forward_hip(self, x):
        """conv -> GroupNorm(+ReLU) pairs: the conv leaves raw (split-K) slabs in the workspace and the
        GroupNorm kernel reduces + normalises them, 2 launches per pair."""
        c = self.convs
        y, ds = self.body_hip(x)
        se = getattr(self, "se", None)
        if se is not None:
            # SE tail, two launches: the gate from the raw conv3 output and GroupNorm 3's statistics, then
            # relu(gate * GroupNorm3 + identity) in place of the block's last GroupNorm launch
            e, g3 = se.excite, c[7]
            gate = ops.se_gate(y, g3.weight, g3.bias, g3.num_groups, g3.eps, e[0].weight, e[0].bias, e[2].weight, e[2].bias)
            if ds is not None:
                gn = self.downsample[1]
                return ops.se_apply(y, g3.weight, g3.bias, g3.num_groups, g3.eps, gate, x2=ds, gamma2=gn.weight, beta2=gn.bias)
            return ops.se_apply(y, g3.weight, g3.bias, g3.num_groups, g3.eps, gate, residual=x)
        if ds is not None:
            gn = self.downsample[1]
            return ops.groupnorm(y, c[7].weight, c[7].bias, c[7].num_groups, c[7].eps, relu=True, x2=ds,
                                 gamma2=gn.weight, beta2=gn.bias)
        return ops.groupnorm(y, c[7].weight, c[7].bias, c[7].num_groups, c[7].eps, relu=True, residual=x)

    def body_hip(self, x):
        """Everything but the block's last GroupNorm: -> (raw conv3 output, raw downsample conv output | None), both
        left as split-K slabs in the two workspaces."""
        c = self.convs
        ds = None
        if self.downsample is not None:
            # the downsample conv leaves its slabs in the second workspace; its GroupNorm is folded into the
            # block's last GroupNorm launch (same channels, same groups)
            gn = self.downsample[1]
            assert gn.num_groups == c[7].num_groups and gn.eps == c[7].eps
            ds = ops.conv2d(x, self.downsample[0].weight, stride=self.stride, defer=True, ws_slot=1)
        y = ops.conv2d(x, c[0].weight, defer=True)
        y = ops.groupnorm(y, c[1].weight, c[1].bias, c[1].num_groups, c[1].eps, relu=True)
        if c[3].groups == 1:
            y = ops.conv2d(y, c[3].weight, stride=self.stride, pad=1, defer=True)
        else:  # ResNeXt: the grouped 3x3 conv leaves a plain tensor, which the same GroupNorm launch takes
            y = ops.gconv3x3(y, c[3].weight, c[3].groups, stride=self.stride)
        y = ops.groupnorm(y, c[4].weight, c[4].bias, c[4].num_groups, c[4].eps, relu=True)
        return ops.conv2d(y, c[6].weight, defer=True), ds

    def forward_train(self, x, save):
        """The block with every conv output materialised and every GroupNorm's statistics kept: what
        train.depth_encoder_backward walks.  Appends dict(x, l1, l2, l3, ds | None, out) to `save`; l* / ds =
        dict(raw, mean, rstd[, out]) of one conv -> GroupNorm (-> ReLU) layer."""
        c = self.convs
        r1 = ops.conv2d(x, c[0].weight)
        l1 = _gn_train(r1, c[1], relu=True)
        r2 = ops.conv2d(l1["out"], c[3].weight, stride=self.stride, pad=1)
        l2 = _gn_train(r2, c[4], relu=True)
        r3 = ops.conv2d(l2["out"], c[6].weight)
        ds, identity = None, x
        if self.downsample is not None:
            rd = ops.conv2d(x, self.downsample[0].weight, stride=self.stride)
            ds = _gn_train(rd, self.downsample[1], relu=False)
            identity = ds.pop("out")  # (only the tail reads it)
        l3 = _gn_train(r3, c[7], relu=True, residual=identity)
        out = l3.pop("out")
        save.append(dict(x=x, l1=l1, l2=l2, l3=l3, ds=ds, out=out))
        return out


def _gn_train(raw, gn, relu, residual=None):
    """GroupNorm (+ residual) (+ ReLU) of a materialised conv output with the statistics saved -> dict(raw, mean, rstd, out)."""
    n = raw.shape[0] * gn.num_groups
    mean = torch.empty(n, dtype=torch.float32, device=raw.device)
    rstd = torch.empty(n, dtype=torch.float32, device=raw.device)
    out = ops.groupnorm(raw, gn.weight, gn.bias, gn.num_groups, gn.eps, relu=relu, residual=residual, save_mean=mean,
                        save_rstd=rstd)
    return dict(raw=raw, mean=mean, rstd=rstd, out=out)


class _ResNet50GN(nn.Module):
    """habitat-lab's GroupNorm ResNet: ResNet-50 by default; `layers`, `resnext` and `se` make the other DD-PPO backbones
    (DEPTH_BACKBONES).  ResNeXt: expansion 2, the four layers on doubled planes (the stem keeps `base_planes`), 3x3 convs
    with cardinality = base_planes / 2 groups, in every block of a layer."""

    def __init__(self, in_channels, base_planes, ngroups, layers=(3, 4, 6, 3), resnext=False, se=False):
        super().__init__()
        self.expansion = 2 if resnext else 4
        self.cardinality = int(base_planes / 2) if resnext else 1
        self.has_se = bool(se)
        self.conv1 = nn.Sequential(
            nn.Conv2d(in_channels, base_planes, kernel_size=7, stride=2, padding=3, bias=False),
            nn.GroupNorm(ngroups, base_planes), nn.ReLU(True),
        )
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.inplanes = base_planes
        if resnext:
            base_planes *= 2
        self.layer1 = self._make_layer(ngroups, base_planes, layers[0])
        self.layer2 = self._make_layer(ngroups, base_planes * 2, layers[1], stride=2)
        self.layer3 = self._make_layer(ngroups, base_planes * 4, layers[2], stride=2)
        self.layer4 = self._make_layer(ngroups, base_planes * 8, layers[3], stride=2)
        self.final_channels = self.inplanes
        self.final_spatial_compress = 1.0 / (2 ** 5)

    def _make_layer(self, ngroups, planes, blocks, stride=1):
        downsample = None
        ex = self.expansion
        kw = dict(expansion=ex, cardinality=self.cardinality, se=self.has_se)
        if stride != 1 or self.inplanes != planes * ex:
            downsample = nn.Sequential(_conv(self.inplanes, planes * ex, 1, stride), nn.GroupNorm(ngroups, planes * ex))
        layers = [_Bottleneck(self.inplanes, planes, ngroups, stride, downsample, **kw)]
        self.inplanes = planes * ex
        for _ in range(1, blocks):
            layers.append(_Bottleneck(self.inplanes, planes, ngroups, **kw))
        return nn.Sequential(*layers)

    @property
    def plain(self):
        """Every block is the ResNet-50 bottleneck (dense 3x3 conv, no SE): the chain, persistent and training forms apply."""
        return all(b.plain for layer in (self.layer1, self.layer2, self.layer3, self.layer4) for b in layer)

    def forward_chain(self, x, tail):
        """The whole backbone as a chain of ops.gn_conv launches: every GroupNorm kernel also computes its slice of
        the NEXT conv (csrc/gn_conv.hip), so a bottleneck is 3 launches and no conv launch remains after the stem.
        `tail` = (weight, stride, pad) of the conv that follows the backbone (the encoder's compression conv).
        Returns that conv's raw output (a `Deferred`), or None when a shape is outside the kernel's envelope."""
        blocks = [b for layer in (self.layer1, self.layer2, self.layer3, self.layer4) for b in layer]
        if not self.plain:  # a grouped conv or an SE gate: the chain's kernels have neither (the caller runs the pairs)
            return None

        def feeds(blk):  # what the kernel that produces `blk`'s input has to emit for it
            ds = None if blk.downsample is None else (blk.downsample[0].weight, blk.stride)
            return dict(conv_a=(blk.convs[0].weight, 1, 0), conv_b=ds, want_act=ds is None)

        c, gn = self.conv1[0], self.conv1[1]
        y = ops.conv2d(x, c.weight, stride=2, pad=3, defer=True)
        first = ops.CHAIN_FROM_BLOCK if ops.CHAIN_FROM_BLOCK >= 0 else (3 if x.shape[0] <= 5 else 7)
        first = min(first, len(blocks))  # blocks before it run as conv + GroupNorm pairs
        if first == 0:
            r = ops.gn_conv(y, gn, relu=True, pool=True, **feeds(blocks[0]))
        else:
            r0 = ops.gn_conv(y, gn, relu=True, pool=True, want_act=True)  # stem GroupNorm + ReLU + MaxPool in one launch
            act = r0[0] if r0 is not None else \
                ops.pool2d(ops.groupnorm(y, gn.weight, gn.bias, gn.num_groups, gn.eps, relu=True), 3, 2, 1, "max")
            nxt = feeds(blocks[first]) if first < len(blocks) else dict(conv_a=tail)
            # the leading blocks as ivln_nconv_f32 launches (layer 1, or more: NCONV_BLOCKS), then pairs up to `first`
            nb_auto = ops.NCONV_BLOCKS if ops.NCONV_BLOCKS >= 0 else (3 if x.shape[0] <= 5 else 7)
            done = min(first, nb_auto) if ops.NCONV_FRONT else 0
            r = self._front_blocks_nconv(blocks[:done], act, nxt if done == first else None) if done else None
            if r is not None and done < first:
                act, r = r, None  # (the run ended before the chain starts: `r` is the activated output of its last block)
            elif r is None:
                done = 0
            if r is None:
                for blk in blocks[done:first - 1]:
                    act = blk.forward_hip(act)
                # the last pairwise block hands over: its final GroupNorm is the chain's first launch
                blk = blocks[first - 1]
                y3, ds = blk.body_hip(act)
                if ds is not None:
                    r = ops.gn_conv(y3, blk.convs[7], x2=ds, gn2=blk.downsample[1], **nxt)
                else:
                    r = ops.gn_conv(y3, blk.convs[7], residual=act, **nxt)
        for i, blk in enumerate(blocks):
            if i < first:
                continue
            if r is None:
                return None
            act, ya, yb = r
            c = blk.convs
            r = ops.gn_conv(ya, c[1], conv_a=(c[3].weight, blk.stride, 1))
            if r is None:
                return None
            nxt = feeds(blocks[i + 1]) if i + 1 < len(blocks) else dict(conv_a=tail)
            tail_in = dict(x2=yb, gn2=blk.downsample[1]) if blk.downsample is not None else dict(residual=act)
            r2 = None
            if i >= ops.CHAIN_PAIR_FROM_BLOCK:  # GN2 -> conv3 -> GN3 tail -> next conv1 in one launch
                r2 = ops.gn_conv(None, c[7], front=(r[1], c[4], c[6].weight), **tail_in, **nxt)
            if r2 is None:
                r = ops.gn_conv(r[1], c[4], conv_a=(c[6].weight, 1, 0))
                if r is None:
                    return None
                r2 = ops.gn_conv(r[1], c[7], **tail_in, **nxt)
            r = r2
        return None if r is None else r[1]

    @staticmethod
    def _front_blocks_nconv(blocks, act, nxt):
        """The bottlenecks BEFORE the gn_conv chain (large maps: layer 1) as one ivln_nconv_f32 launch per conv layer:
        every conv normalises its input on load from the statistics partials its producer left and emits those of its
        own output - complete tensors, no slabs, no GroupNorm launches.  `act`: the activated input of the first block;
        `nxt`: what the chain's first launch has to emit.  Returns that launch's result, or None (a stride or a shape
        outside the kernel's envelope: the caller runs the conv + GroupNorm pairs).  With `nxt` None the run ends before
        the chain starts: the activated output of the last block is returned instead."""
        identity, x1, xds = act, None, None
        for i, blk in enumerate(blocks):
            c = blk.convs
            G1, G3 = c[1].num_groups, c[7].num_groups
            if i == 0:  # first block: its convs read the activated tensor as it is
                ds = None if blk.downsample is None else (blk.downsample[0].weight, blk.downsample[1].num_groups, blk.stride)
                r = ops.nconv(act, None, relu=False, conv_a=(c[0].weight, G1), conv_b=ds)
                if r is None:
                    return None
                x1, xds = r[1], r[2]
            r = ops.nconv(x1, c[1], conv_a=(c[3].weight, c[4].num_groups, blk.stride))  # GroupNorm 1 + ReLU on load -> 3x3
            if r is None:
                return None
            r = ops.nconv(r[1], c[4], conv_a=(c[6].weight, G3))                  # GroupNorm 2 + ReLU on load -> 1x1
            if r is None:
                return None
            x3 = r[1]
            tail = dict(x2=xds, gn2=blk.downsample[1]) if blk.downsample is not None else dict(residual=identity)
            if i + 1 < len(blocks):  # the block's tail is built on load by the next block's first conv(s)
                nb = blocks[i + 1]
                ds = None if nb.downsample is None else (nb.downsample[0].weight, nb.downsample[1].num_groups, nb.stride)
                r = ops.nconv(x3, c[7], conv_a=(nb.convs[0].weight, nb.convs[1].num_groups), conv_b=ds,
                              want_act=nb.downsample is None, **tail)
                if r is None:
                    return None
                identity, x1, xds = r[0], r[1], r[2]
            elif nxt is not None:  # hand over to the chain: its first launch takes the raw tensors as one-slab inputs
                if blk.downsample is not None:
                    return ops.gn_conv(x3.deferred(), c[7], x2=xds.deferred(), gn2=blk.downsample[1], **nxt)
                return ops.gn_conv(x3.deferred(), c[7], residual=identity, **nxt)
            else:  # hand over to conv + GroupNorm pairs: materialise the block's output
                if blk.downsample is not None:
                    gd = blk.downsample[1]
                    return ops.groupnorm(x3.deferred(), c[7].weight, c[7].bias, G3, c[7].eps, relu=True, x2=xds.deferred(),
                                         gamma2=gd.weight, beta2=gd.bias)
                return ops.groupnorm(x3.deferred(), c[7].weight, c[7].bias, G3, c[7].eps, relu=True, residual=identity)
        return None

    def forward_hip(self, x):
        c, gn = self.conv1[0], self.conv1[1]
        y = ops.conv2d(x, c.weight, stride=2, pad=3, defer=True)
        y = ops.groupnorm(y, gn.weight, gn.bias, gn.num_groups, gn.eps, relu=True)
        y = ops.pool2d(y, 3, 2, 1, "max")
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                y = blk.forward_hip(y)
        return y

    def forward_train(self, x, save):
        """forward_hip with materialised conv outputs and saved statistics (a trainable encoder's update pass):
        save["stem"] = dict(x, raw, mean, rstd, out = the activation in front of the max-pool), save["blocks"] = one
        entry per bottleneck (_Bottleneck.forward_train)."""
        c, gn = self.conv1[0], self.conv1[1]
        stem = _gn_train(ops.conv2d(x, c.weight, stride=2, pad=3), gn, relu=True)
        stem["x"] = x
        save["stem"], save["blocks"] = stem, []
        y = ops.pool2d(stem["out"], 3, 2, 1, "max")
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                y = blk.forward_train(y, save["blocks"])
        return y


class ResNetEncoder(nn.Module):
    """habitat-lab ResNetEncoder for a depth-only observation space: avg_pool2d(2) -> GN-ResNet50 (or another DD-PPO
    `backbone`, DEPTH_BACKBONES) -> 3x3 compression conv + GroupNorm(1) + ReLU -> (B,128,4,4)."""

    def __init__(self, depth_shape, baseplanes=32, ngroups=16, backbone="resnet50"):
        super().__init__()
        layers, resnext, se = depth_backbone_spec(backbone)
        self.backbone_name = backbone
        spatial_size = depth_shape[0] // 2
        self._n_input_depth = depth_shape[2]
        self.running_mean_and_var = nn.Sequential()
        if backbone == "resnet50":
            self.backbone = _ResNet50GN(self._n_input_depth, baseplanes, ngroups)
        else:
            self.backbone = _ResNet50GN(self._n_input_depth, baseplanes, ngroups, layers=layers, resnext=resnext, se=se)
        final_spatial = int(spatial_size * self.backbone.final_spatial_compress)
        num_compression_channels = int(round(2048 / (final_spatial ** 2)))
        self.compression = nn.Sequential(
            nn.Conv2d(self.backbone.final_channels, num_compression_channels, kernel_size=3, padding=1, bias=False),
            nn.GroupNorm(1, num_compression_channels), nn.ReLU(True),
        )
        self.output_shape = (num_compression_channels, final_spatial, final_spatial)
        for layer in self.modules():
            if isinstance(layer, (nn.Conv2d, nn.Linear)):
                nn.init.kaiming_normal_(layer.weight, nn.init.calculate_gain("relu"))
                if layer.bias is not None:
                    nn.init.constant_(layer.bias, val=0)

    @property
    def is_blind(self):
        return self._n_input_depth == 0

    @property
    def trains(self):
        """A parameter of the encoder takes a gradient (MODEL.DEPTH_ENCODER.trainable, resnet_encoders.py:31-43)."""
        return any(p.requires_grad for p in self.parameters())

    def forward_train(self, observations, save, out=None, out_ctot=0):
        """The update pass of a trainable encoder: the same network as `forward`, layer by layer with materialised conv
        outputs, and in `save` (a dict) per layer the conv input, the raw GroupNorm input, its mean / rstd and the activated
        output - what train.depth_encoder_backward reads.  Callers take it only for a pass that will be differentiated
        (the policy's training forward with a `save` dict, which runs under the autograd Function's no_grad) and only when
        `trains`; every other call keeps the chain, pair and persistent paths of `forward`."""
        depth = observations["depth"].to(torch.float32).contiguous()
        B, H, W, Cd = depth.shape
        assert Cd == 1, "depth-only encoder"
        c, gn = self.compression[0], self.compression[1]
        hw = self.output_shape[1] * self.output_shape[2]
        x = ops.pool2d(depth.view(B, 1, H, W), 2, 2, 0, "avg")  # F.avg_pool2d(x, 2)
        y = self.backbone.forward_train(x, save)
        raw = ops.conv2d(y, c.weight, pad=1)
        mean = torch.empty(B * gn.num_groups, dtype=torch.float32, device=depth.device)
        rstd = torch.empty(B * gn.num_groups, dtype=torch.float32, device=depth.device)
        # (the backward masks with a dense copy of the output: `out` may be a channel slice of the policy's buffer)
        feats = ops.groupnorm(raw, gn.weight, gn.bias, gn.num_groups, gn.eps, relu=True, save_mean=mean, save_rstd=rstd)
        save["comp"] = dict(x=y, raw=raw, mean=mean, rstd=rstd, out=feats)
        if out is None:
            return feats
        ops.copy2d(feats.view(B, -1), out.view(B, -1), B, self.output_shape[0] * hw)  # (rows of the wider buffer)
        return out

    def forward(self, observations, out=None, out_ctot=0, save=None):
        """observations["depth"]: (B,H,W,1) f32.  `out`: optional (B,128,4,4) channel slice of a wider
        NCHW buffer with `out_ctot` channels (the policy passes its depth+spatial-embedding buffer).
        `save`: a dict = the differentiated pass of a trainable encoder (forward_train)."""
        if save is not None:
            return self.forward_train(observations, save, out, out_ctot)
        depth = observations["depth"].to(torch.float32).contiguous()
        B, H, W, Cd = depth.shape
        assert Cd == 1, "depth-only encoder"
        c, gn = self.compression[0], self.compression[1]
        hw = self.output_shape[1] * self.output_shape[2]
        want = ops.DEPTH_NET == 2 or (ops.DEPTH_NET == 1 and (not getattr(self, "beside_other_work", False)
                                                                or B >= ops.DEPTH_NET_SPLIT_MIN))
        if (want and B <= depth_net.DepthNetPlan.MAX_IMAGES and (H, W) == (256, 256) and not torch.is_grad_enabled()
                and getattr(self, "latency_bound", True) and not getattr(self, "no_persistent", False)):
            # rollout batches: the whole encoder as ONE persistent launch, a cluster of 32 workgroups per image
            # (csrc/depth_net.hip); declined (False) when the device cannot keep all its workgroups resident
            plan = depth_net.plan_for(self, depth.device)
            dst = out if out is not None else torch.empty((B,) + tuple(self.output_shape), dtype=torch.float32, device=depth.device)
            if plan is not None and plan.run(depth, dst, out_ctot * hw if out is not None else self.output_shape[0] * hw):
                return dst
        x = ops.pool2d(depth.view(B, 1, H, W), 2, 2, 0, "avg")  # F.avg_pool2d(x, 2)
        chain = ops.CHAIN_GN_CONV and B <= ops.CHAIN_MAX_IMAGES and getattr(self, "latency_bound", True)
        y = self.backbone.forward_chain(x, (c.weight, 1, 1)) if chain else None
        if y is None:
            x = self.backbone.forward_hip(x)
            y = ops.conv2d(x, c.weight, pad=1, defer=True)
        if out is None:
            return ops.groupnorm(y, gn.weight, gn.bias, gn.num_groups, gn.eps, relu=True)
        return ops.groupnorm(y, gn.weight, gn.bias, gn.num_groups, gn.eps, relu=True, out=out,
                             y_img_stride=out_ctot * hw)


class VlnResnetDepthEncoder(nn.Module):
    def __init__(self, observation_space, output_size: int = 128, checkpoint: str = "NONE", backbone: str = "resnet50",
                 resnet_baseplanes: int = 32, normalize_visual_inputs: bool = False, trainable: bool = False,
                 spatial_output: bool = False) -> None:
        super().__init__()
        assert not normalize_visual_inputs and spatial_output
        depth_backbone_spec(backbone)  # (ValueError that lists the accepted names)
        if trainable and backbone != "resnet50":
            raise ValueError(f"MODEL.DEPTH_ENCODER.trainable needs backbone resnet50 (the HIP backward walks ResNet-50 "
                             f"bottlenecks only); got {backbone!r}")
        depth_shape = observation_space.spaces["depth"].shape
        if len(depth_shape) == 4:  # single_frame_box_shape (common/utils.py:38-48)
            depth_shape = depth_shape[1:]
        self.visual_encoder = ResNetEncoder(depth_shape, baseplanes=resnet_baseplanes, ngroups=resnet_baseplanes // 2,
                                            backbone=backbone)
        for param in self.visual_encoder.parameters():
            param.requires_grad_(trainable)
        if checkpoint != "NONE":
            ddppo_weights = torch.load(checkpoint, map_location="cpu")
            weights_dict = {}
            for k, v in ddppo_weights["state_dict"].items():  # resnet_encoders.py:48-61
                split_layer_name = k.split(".")[2:]
                if split_layer_name[0] != "visual_encoder":
                    continue
                weights_dict[".".join(split_layer_name[1:])] = v
            del ddppo_weights
            self.visual_encoder.load_state_dict(weights_dict, strict=True)
        self.spatial_output = spatial_output
        c, h, w = self.visual_encoder.output_shape
        self.spatial_embeddings = nn.Embedding(h * w, 64)
        self.output_shape = (c + self.spatial_embeddings.embedding_dim, h, w)

    @property
    def is_blind(self):
        return self.visual_encoder.is_blind

    def forward(self, observations, save=None):
        """-> (B, 192, 4, 4): visual features ++ the learned spatial embedding (a raw `.view` of the
        (16,64) table as (64,4,4), resnet_encoders.py:97-113).  `save`: a dict that receives the visual encoder's
        per-layer saves (ResNetEncoder.forward_train) - the update pass of a trainable encoder fed with depth frames;
        it stays empty when the features come cached."""
        c, h, w = self.visual_encoder.output_shape
        E = self.spatial_embeddings.embedding_dim
        if "depth_features" in observations:
            feats = observations["depth_features"].to(torch.float32).contiguous()
            B = feats.shape[0]
            out = torch.empty((B, c + E, h, w), dtype=torch.float32, device=feats.device)
            ops.copy2d(feats.view(B, -1), out.view(B, -1), B, c * h * w)
        else:
            B = observations["depth"].shape[0]
            dev = observations["depth"].device
            sw = self.spatial_embeddings.weight
            if save is None and not torch.is_grad_enabled():
                # inference: the embedding half of the output is constant between weight updates - keep one output
                # buffer per batch size with that half filled once instead of one copy launch per step.  (Created
                # outside graph capture only: a buffer from a graph's private pool must not outlive that graph.)
                # Buffers are never freed or reallocated (a captured graph keeps raw pointers to them); a weight
                # update refills the embedding half in place.
                stamp = (ops.WEIGHT_EPOCH, sw._version, sw.data_ptr())
                cache = self.__dict__.setdefault("_out_cache", {})
                ent = cache.get((B, str(dev)))
                if (ent is None or ent[0] != stamp) and not torch.cuda.is_current_stream_capturing():
                    buf = ent[1] if ent is not None else torch.empty((B, c + E, h, w), dtype=torch.float32, device=dev)
                    ops.copy2d(sw.view(1, -1), buf.view(B, -1)[:, c * h * w:], B, E * h * w, broadcast_rows=True)
                    ent = cache[(B, str(dev))] = (stamp, buf)
                if ent is not None and ent[0] == stamp:
                    self.visual_encoder(observations, out=ent[1][:, :c], out_ctot=c + E)
                    return ent[1]
            out = torch.empty((B, c + E, h, w), dtype=torch.float32, device=dev)
            self.visual_encoder(observations, out=out[:, :c], out_ctot=c + E, save=save)
        ops.copy2d(self.spatial_embeddings.weight.view(1, -1), out.view(B, -1)[:, c * h * w:], B, E * h * w,
                   broadcast_rows=True)
        return out


# ------------------------------------------------------------------------------------------------
# RNN state encoders (masked GRU; masked LSTM)
# ------------------------------------------------------------------------------------------------
class RNNStateEncoder(nn.Module):
    def __init__(self, input_size: int, hidden_size: int, num_layers: int = 1):
        super().__init__()
        assert num_layers == 1
        self.num_recurrent_layers = num_layers
        self.rnn = nn.GRU(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers)
        for name, param in self.rnn.named_parameters():
            if "weight" in name:
                nn.init.orthogonal_(param)
            elif "bias" in name:
                nn.init.constant_(param, 0)

    def forward(self, x, h0, masks_u8, out, state_out, save=None):
        """x (rows,I); h0 (N,H) view (row-strided) of the incoming state; masks u8 (rows); `out`
        (rows,H) row-strided destination of the per-step outputs; state_out (N,H) view for the final
        hidden state.  rows == N -> single step, else time-major sequence of T = rows/N steps."""
        rnn = self.rnn
        rows, N = x.shape[0], h0.shape[0]
        H = rnn.hidden_size
        if rows == N:
            saves = None
            if save is not None:
                saves = tuple(torch.empty((rows, H), dtype=torch.float32, device=x.device) for _ in range(4))
                save.update(r=saves[0], z=saves[1], n=saves[2], ghn=saves[3], T=1, N=N, x=x, h0=h0, masks=masks_u8, out=out)
            ops.gru_step(x, None, h0, masks_u8, rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0,
                         out, state_out, saves)
            return out
        T = rows // N
        gi = ops.linear_gemm(x, rnn.weight_ih_l0, rnn.bias_ih_l0)
        saves = None
        if save is not None:
            saves = tuple(torch.empty((rows, H), dtype=torch.float32, device=x.device) for _ in range(4))
            save.update(r=saves[0], z=saves[1], n=saves[2], ghn=saves[3], T=T, N=N, x=x, h0=h0, masks=masks_u8, out=out)
        ops.gru_seq(gi, h0, masks_u8, rnn.weight_hh_l0, rnn.bias_hh_l0, out, state_out, T, N, saves)
        return out


class LSTMStateEncoder(nn.Module):
    """STATE_ENCODER.rnn_type LSTM: habitat-lab's RNNStateEncoder over nn.LSTM (the reference passes the key through,
    map_cma_policy.py:183,229).  Two recurrent "layers" in the batch-first state: slot 0 is h, slot 1 is c."""

    def __init__(self, input_size: int, hidden_size: int, num_layers: int = 1):
        super().__init__()
        assert num_layers == 1
        self.num_recurrent_layers = 2 * num_layers
        self.rnn = nn.LSTM(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers)
        for name, param in self.rnn.named_parameters():
            if "weight" in name:
                nn.init.orthogonal_(param)
            elif "bias" in name:
                nn.init.constant_(param, 0)

    def forward(self, x, state_in, masks_u8, out, state_out, save=None):
        """The RNNStateEncoder.forward contract with (N,2,H) state views: x (rows,I); state_in / state_out (N,2,H)
        row-strided slices [h | c] of the incoming / outgoing state; masks u8 (rows); `out` (rows,H) row-strided
        destination of the per-step outputs.  rows == N -> single step, else time-major sequence of T = rows/N steps."""
        rnn = self.rnn
        rows, N = x.shape[0], state_in.shape[0]
        H = rnn.hidden_size
        h0, c0 = state_in[:, 0], state_in[:, 1]
        T = rows // N
        saves = None
        if save is not None:
            saves = tuple(torch.empty((rows, H), dtype=torch.float32, device=x.device) for _ in range(5))
            save.update(saves=saves, T=T, N=N, x=x, h0=h0, c0=c0, masks=masks_u8, out=out)
        if rows == N:
            ops.lstm_step(x, None, h0, c0, masks_u8, rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0,
                          out, state_out[:, 1], state_out[:, 0], saves)
            return out
        gi = ops.linear_gemm(x, rnn.weight_ih_l0, rnn.bias_ih_l0)
        ops.lstm_seq(gi, h0, c0, masks_u8, rnn.weight_hh_l0, rnn.bias_hh_l0, out, state_out[:, 0], state_out[:, 1], T, N,
                     saves)
        return out


def build_rnn_state_encoder(input_size: int, hidden_size: int, rnn_type: str = "GRU", num_layers: int = 1):
    kind = str(rnn_type).lower()
    if kind == "gru":
        return RNNStateEncoder(input_size, hidden_size, num_layers)
    if kind == "lstm":
        return LSTMStateEncoder(input_size, hidden_size, num_layers)
    raise ValueError(f"MODEL.STATE_ENCODER.rnn_type must be GRU or LSTM, got {rnn_type!r}")
