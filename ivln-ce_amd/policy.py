"""MapCMA policy plugin: same registry name, constructor, `act` / `act_iterative` /
`build_distribution` surface and `state_dict()` keys as the reference
(ivlnce_baselines/models/map_cma_policy.py:28-368, models/policy.py:12-83,
common/utils.py:149-185), forward AND backward on HIP kernels.

torch.nn modules hold parameters only.  The whole net forward is one torch.autograd.Function whose
backward runs the hand-written HIP backward kernels (train.py), so `loss.backward()` in a trainer
(base_il_trainer.py:211) works unchanged.
"""
from collections import namedtuple
from typing import Tuple

import numpy as np
import torch
import torch.nn as nn
from torch import Tensor

from . import ops
from .aux_losses import AuxLosses
from .encoders import (InstructionEncoder, LSTMStateEncoder, RNNStateEncoder, SemanticMapEncoder,
                       VlnResnetDepthEncoder, build_rnn_state_encoder)
from .registry import baseline_registry

try:  # pragma: no cover
    from habitat_baselines.rl.ppo.policy import Net, Policy  # type: ignore
except Exception:  # noqa: BLE001

    class Net(nn.Module):
        pass

    class Policy(nn.Module):
        pass


class CustomFixedCategorical(torch.distributions.Categorical):
    """common/utils.py:149-169."""

    def sample(self, sample_shape=torch.Size()):  # noqa: B008
        return super().sample(sample_shape).unsqueeze(-1)

    def log_prob(self, actions: Tensor) -> Tensor:
        return super().log_prob(actions.squeeze(-1)).view(actions.size(0), -1).sum(-1).unsqueeze(-1)

    def mode(self):
        return self.probs.argmax(dim=-1, keepdim=True)


class CategoricalNet(nn.Module):
    """common/utils.py:172-185; the 512->4 linear runs on the HIP skinny/MFMA linear."""

    def __init__(self, num_inputs: int, num_outputs: int) -> None:
        super().__init__()
        self.linear = nn.Linear(num_inputs, num_outputs)
        self.num_outputs = num_outputs
        nn.init.orthogonal_(self.linear.weight, gain=0.01)
        nn.init.constant_(self.linear.bias, 0)

    def raw_logits(self, x: Tensor) -> Tensor:
        if x.shape[-1] != self.num_outputs:
            if x.requires_grad or (torch.is_grad_enabled() and self.linear.weight.requires_grad):
                from .train import LinearFn

                x = LinearFn.apply(x, self.linear.weight, self.linear.bias)
            else:
                x = ops.linear(x.contiguous(), self.linear.weight, self.linear.bias)
        return x

    def forward(self, x: Tensor) -> CustomFixedCategorical:
        return CustomFixedCategorical(logits=self.raw_logits(x))


class StepGeometry(namedtuple("StepGeometry", "d_out m_out E x2w o_txt o_dep o_map o_prev")):
    """Column layout of the two row buffers of a MapCMANet step: state_in = [dep_in | map_in | prev] (d_out, m_out, E
    wide), x2 = [state | text | dep' | map' | prev] (x2w wide; text / dep' / map' / prev begin at the four offsets)."""

    def buffers(self, rows, device):
        """-> (state_in, x2) for `rows` rows."""
        return (torch.empty((rows, self.d_out + self.m_out + self.E), dtype=torch.float32, device=device),
                torch.empty((rows, self.x2w), dtype=torch.float32, device=device))


# What one graphed.GraphedRollout in split mode shares between MapCMANet's three stages: the persistent row buffers, and
# where the instruction branch runs - in the depth stage behind (txt_with_dep True) or in front of ("first") the depth
# encoder, else in the pre stage, as its last branch (txt_last) or its first.  ("first" is a measurement variant kept from
# the 8-image experiments: no caller in the repository passes it.)
SplitStep = namedtuple("SplitStep", "state_in x2 txt_with_dep txt_last", defaults=(False, False))


class MapCMANet(Net):
    """Cross-modal attention network: instruction bi-LSTM, DD-PPO depth ResNet, semantic-map CNN,
    two recurrent state encoders (GRU, or LSTM with STATE_ENCODER.rnn_type LSTM) and three attentions
    (map_cma_policy.py:103-368)."""

    def __init__(self, observation_space, config, num_actions):
        super().__init__()
        model_config = config.MODEL
        self.model_config = model_config
        model_config.defrost()
        model_config.INSTRUCTION_ENCODER.final_state_only = False
        model_config.freeze()

        assert model_config.SEMANTIC_MAP_ENCODER.classname in [
            "SemanticMapEncoder"
        ], "SEMANTIC_MAP_ENCODER.classname must be SemanticMapEncoder"
        sm = model_config.SEMANTIC_MAP_ENCODER
        self.map_encoder = SemanticMapEncoder(
            observation_space, sm.num_semantic_classes, sm.channels, sm.last_ch_mult, sm.trainable, sm.from_pretrained,
            sm.checkpoint,
        )
        self.check_map_size(observation_space.spaces["occupancy_map"].shape)
        self.instruction_encoder = InstructionEncoder(model_config.INSTRUCTION_ENCODER)
        assert model_config.DEPTH_ENCODER.cnn_type in [
            "VlnResnetDepthEncoder"
        ], "DEPTH_ENCODER.cnn_type must be VlnResnetDepthEncoder"
        self.depth_encoder = VlnResnetDepthEncoder(
            observation_space,
            output_size=model_config.DEPTH_ENCODER.output_size,
            checkpoint=model_config.DEPTH_ENCODER.ddppo_checkpoint,
            backbone=model_config.DEPTH_ENCODER.backbone,
            # (the reference's policies never hand the key to the encoder: there it only stops the trainers' feature
            #  cache and the ResNet stays frozen; here a trainable encoder trains - train.depth_encoder_backward)
            trainable=bool(model_config.DEPTH_ENCODER.trainable),
            spatial_output=True,
        )
        self.prev_action_embedding = nn.Embedding(num_actions + 1, 32)
        hidden_size = model_config.STATE_ENCODER.hidden_size
        self._hidden_size = hidden_size
        self.depth_linear = nn.Sequential(
            nn.Flatten(),
            nn.Linear(int(np.prod(self.depth_encoder.output_shape)), model_config.DEPTH_ENCODER.output_size),
            nn.ReLU(True),
        )
        self.map_linear = nn.Sequential(
            nn.Flatten(),
            nn.Linear(int(np.prod(self.map_encoder.output_shape)), model_config.SEMANTIC_MAP_ENCODER.output_size),
            nn.ReLU(True),
        )
        rnn_input_size = (
            model_config.DEPTH_ENCODER.output_size
            + model_config.SEMANTIC_MAP_ENCODER.output_size
            + self.prev_action_embedding.embedding_dim
        )
        self.state_encoder = build_rnn_state_encoder(
            input_size=rnn_input_size, hidden_size=hidden_size, rnn_type=model_config.STATE_ENCODER.rnn_type, num_layers=1
        )
        self._output_size = (
            hidden_size
            + model_config.DEPTH_ENCODER.output_size
            + self.instruction_encoder.output_size
            + model_config.SEMANTIC_MAP_ENCODER.output_size
        )
        self.dep_kv = nn.Conv1d(
            self.depth_encoder.output_shape[0], hidden_size // 2 + model_config.DEPTH_ENCODER.output_size, 1
        )
        self.map_kv = nn.Conv1d(
            self.map_encoder.output_shape[0], hidden_size // 2 + model_config.SEMANTIC_MAP_ENCODER.output_size, 1
        )
        self.state_q = nn.Linear(hidden_size, hidden_size // 2)
        self.text_k = nn.Conv1d(self.instruction_encoder.output_size, hidden_size // 2, 1)
        self.text_q = nn.Linear(self.instruction_encoder.output_size, hidden_size // 2)
        self.register_buffer("_scale", torch.tensor(1.0 / ((hidden_size // 2) ** 0.5)))
        self.second_state_compress = nn.Sequential(
            nn.Linear(self._output_size + self.prev_action_embedding.embedding_dim, self._hidden_size), nn.ReLU(True)
        )
        self.second_state_encoder = build_rnn_state_encoder(
            input_size=self._hidden_size, hidden_size=self._hidden_size,
            rnn_type=model_config.STATE_ENCODER.rnn_type, num_layers=1,
        )
        self._output_size = model_config.STATE_ENCODER.hidden_size
        self.progress_monitor = nn.Linear(self.output_size, 1)
        self._init_layers()
        self.train()
        if not model_config.SEMANTIC_MAP_ENCODER.trainable:
            self.map_encoder.eval()
        self._scale_f = float(1.0 / ((hidden_size // 2) ** 0.5))

    @staticmethod
    def check_map_size(map_shape):
        """Raises for egocentric maps the map branch cannot take: the map CNN halves the plane four times and its pooling
        tail reads pixel pairs (an odd plane is refused by the kernel, where the reference's AvgPool2d floors), and the
        head's map attention covers up to 256 positions."""
        rows, cols = int(map_shape[0]), int(map_shape[1])
        n_pos = (rows // 16) * (cols // 16)
        if rows <= 0 or cols <= 0 or rows % 16 or cols % 16 or n_pos > 256:
            raise ValueError(
                f"EGOCENTRIC_MAPPER.height_meters / width_meters / resolution_meters give a map of {rows} x {cols} cells "
                f"(height_meters / resolution_meters x width_meters / resolution_meters); MapCMANet takes maps whose sides "
                f"are multiples of 16 cells with (rows // 16) * (cols // 16) <= 256 attention positions (here {n_pos})")

    @property
    def output_size(self):
        return self._output_size

    @property
    def is_blind(self):
        return self.depth_encoder.is_blind

    @property
    def num_recurrent_layers(self):
        return self.state_encoder.num_recurrent_layers + self.second_state_encoder.num_recurrent_layers

    @property
    def _gru_encoders(self):
        """Both state encoders are GRUs: what the fused recurrent head (ivln_cma_step_fwd, GRU arithmetic) requires."""
        return isinstance(self.state_encoder, RNNStateEncoder) and isinstance(self.second_state_encoder, RNNStateEncoder)

    @property
    def fused_head_form(self):
        """The form of the fused recurrent head (csrc/cma_step.hip) the two state encoders allow: "gru"
        (ivln_cma_step_fwd), "lstm" (ivln_cma_step_lstm_fwd), or None - the unfused chain."""
        if self._gru_encoders:
            return "gru"
        if isinstance(self.state_encoder, LSTMStateEncoder) and isinstance(self.second_state_encoder, LSTMStateEncoder):
            return "lstm"
        return None

    @staticmethod
    def _state_slot(states, first, n):
        """The n recurrent layers from `first` on of a batch-first (N, L, H) state, as an encoder takes them: (N, H) for
        the GRU's single layer, (N, n, H) otherwise (map_cma_policy.py:290-351 slices by num_recurrent_layers)."""
        return states[:, first] if n == 1 else states[:, first:first + n]

    def _cma_fold_weights(self):
        """Instruction-side folds of the fused rollout head (csrc/cma_step.hip), cached until the weights change:
        rows 0..H-1 = W_q^T W_k, row H = b_q^T W_k (shift: the same rows applied to b_k), then W_tq / b_tq - one
        (H + 1 + h2) x 256 weight for a single 1x1 conv over the instruction encoder's output."""
        ps = (self.state_q.weight, self.state_q.bias, self.text_k.weight, self.text_k.bias, self.text_q.weight,
              self.text_q.bias)
        key = (ops.WEIGHT_EPOCH,) + tuple(p._version for p in ps) + tuple(p.data_ptr() for p in ps)
        if getattr(self, "_cma_fold_key", None) != key:
            with torch.no_grad():
                wq, bq, wk, bk, wtq, btq = [p.detach() for p in ps]
                a = torch.cat([ops.transpose(wq.contiguous()), bq.view(1, -1)], 0).contiguous()  # (H+1, h2)
                wk2 = torch.cat([wk.view(wk.shape[0], -1), bk.view(-1, 1)], 1).contiguous()       # (h2, Ct + 1)
                y = ops.linear_gemm(a, ops.transpose(wk2))                                        # (H+1, Ct + 1)
                ct = wk.shape[1]
                wf = torch.cat([y[:, :ct], wtq.view(wtq.shape[0], -1)], 0).contiguous()
                bf = torch.cat([y[:, ct], btq], 0).contiguous()
            self._cma_fold_key, self._cma_fold = key, (wf, bf)
        return self._cma_fold

    @staticmethod
    def _fused_head_ops(form):
        """(scratch, entry point) of a fused head form in `ops`; None for the unfused chain."""
        return {"gru": (ops.cma_step_ws, ops.cma_step), "lstm": (ops.cma_step_lstm_ws, ops.cma_step_lstm)}.get(form)

    def prepare_capture(self, example_obs):
        """Create everything the rollout step caches lazily BEFORE a stream capture (graphed.py): a buffer born inside
        a capture lives in that graph's private pool and must not survive in a process-wide cache."""
        head = self._fused_head_ops(self.fused_head_form)
        key = self.instruction_encoder.obs_key
        if ops.CMA_STEP_MODE < 0 or key not in example_obs or head is None:
            return
        rows, L = example_obs[key].shape[0], example_obs[key].shape[1]
        P = self.depth_encoder.output_shape[1] * self.depth_encoder.output_shape[2]
        Pm = self.map_encoder.output_shape[1] * self.map_encoder.output_shape[2]
        if P > 16 or Pm != P or L > 512:
            return  # outside the fused head's envelope: the step takes the unfused chain
        self._cma_fold_weights()
        head[0](rows, L, P, self._hidden_size, example_obs[key].device)

    def _init_layers(self):
        if self.model_config.PROGRESS_MONITOR.use:
            nn.init.kaiming_normal_(self.progress_monitor.weight, nonlinearity="tanh")
            nn.init.constant_(self.progress_monitor.bias, 0)

    # ---- the parts of one step ----------------------------------------------------------------
    @property
    def step_geometry(self):
        d_out, m_out = self.depth_linear[1].out_features, self.map_linear[1].out_features
        E, o_txt = self.prev_action_embedding.embedding_dim, self._hidden_size
        o_dep = o_txt + self.instruction_encoder.output_size
        o_map, o_prev = o_dep + d_out, o_dep + d_out + m_out
        return StepGeometry(d_out, m_out, E, o_prev + E, o_txt, o_dep, o_map, o_prev)

    @staticmethod
    def _step_inputs(rnn_states, prev_actions, action_masks):
        """The step's inputs as the kernels take them: float32 states, (rows,) uint8 masks, (rows,) int64 actions."""
        return (rnn_states.to(torch.float32).contiguous(), action_masks.reshape(-1).to(torch.uint8).contiguous(),
                prev_actions.reshape(-1).long().contiguous())

    def _fused_head_eligible(self, observations, save):
        """The fused recurrent head (ivln_cma_step_fwd; ivln_cma_step_lstm_fwd with LSTM encoders - the fold does not
        depend on the cell) wants the instruction branch to emit the folded [Mq | TQb] operand instead of text_k, so its
        eligibility is decided from shapes known before any branch runs (the encoders' static output shapes, the token
        axis, the widths' divisibility rules of csrc/cma_step.hip) - anything outside the kernel's envelope takes the
        unfused chain with a real text_k."""
        mc, geo = self.model_config, self.step_geometry
        H, h2 = self._hidden_size, self._hidden_size // 2
        P_static = self.depth_encoder.output_shape[1] * self.depth_encoder.output_shape[2]
        key = self.instruction_encoder.obs_key  # (tokens (rows, L); features (rows, L, E): the token axis is axis 1)
        L_static = observations[key].shape[1] if key in observations else 0
        return (save is None and ops.CMA_STEP_MODE >= 0 and self.fused_head_form is not None
                and not (mc.ablate_instruction or mc.ablate_depth or mc.ablate_map)
                and P_static <= 16 and 0 < L_static <= 512
                and self.map_encoder.output_shape[1] * self.map_encoder.output_shape[2] == P_static
                and H % 64 == 0 and h2 % 64 == 0 and geo.d_out % 16 == 0 and geo.m_out % 16 == 0
                and self.instruction_encoder.output_size % 64 == 0)

    def _txt_branch(self, observations, fused_head, sv, inv=None):
        """Instruction encoder + what the head reads the instruction through: -> (txt (rows | U, 256, L), lengths, tk),
        tk = text_k's keys, or the folded [Mq | TQb] operand when `fused_head`.  `inv`: see forward_hip."""
        mc, h2 = self.model_config, self._hidden_size // 2
        key = self.instruction_encoder.obs_key
        src = observations if inv is None else {key: observations[key + "_unique"]}
        t, ln = self.instruction_encoder(src, sv)  # (rows | U, 256, L)
        if mc.ablate_instruction:
            t = torch.zeros_like(t)
        r_, L_ = t.shape[0], t.shape[2]
        if fused_head:
            # rollout: text_k, state_q and text_q folded over the instruction (csrc/cma_step.hip): ONE 1x1 conv
            # yields Mq (H+1 channels) and TQb (h2 channels) for the fused head, no text_k tensor is made
            wf, bf = self._cma_fold_weights()
            cache = self.instruction_encoder.last_cache if sv is None else None
            if cache is not None and getattr(cache, "fold_behind", False):
                # an earlier cached call re-encoded rows without folding them (the unfused head, or a capture that had
                # to drop the cache): `dirty` only names THIS call's rows, so every row is folded again
                if torch.cuda.is_current_stream_capturing():
                    cache = None
                else:
                    cache.dirty.fill_(1)
                    cache.fold_behind = False
            if cache is not None:
                # per-episode cache (encoders.InstructionEncoder.step_cache): the folded operands live in the cache's
                # persistent buffer and only the rows the encoder just re-encoded (cache.dirty) are recomputed
                fkey = getattr(self, "_cma_fold_key", None)
                if cache.fold is None or cache.fold_key != fkey:
                    if torch.cuda.is_current_stream_capturing():
                        cache.fold_behind = True  # (the replays advance the cache's tokens without its fold)
                        cache = None  # (cannot be created / invalidated inside a capture: plain conv below)
                    else:
                        if cache.fold is None:
                            cache.fold = torch.zeros((r_, wf.shape[0], 1, L_), dtype=torch.float32, device=t.device)
                        cache.fold_key = fkey
                        cache.dirty.fill_(1)  # (folded for other weights, or never: every row's operands are made now)
            if cache is not None:
                ops.conv2d(t.view(r_, -1, 1, L_), wf.view(wf.shape[0], -1, 1, 1), shift=bf, splitk=False, out=cache.fold,
                           run_flags=cache.dirty)
                return t, ln, cache.fold.view(r_, -1, L_)
            # (no cache: every row is "dirty" - the same kernel as the cached call, so that the two agree bit for bit
            #  whatever the tile heuristics make of a plain 1x1 conv of this shape)
            fold = ops.conv2d(t.view(r_, -1, 1, L_), wf.view(wf.shape[0], -1, 1, 1), shift=bf, splitk=False,
                              run_flags=ops.all_rows_flags(r_, t.device))
            return t, ln, fold.view(r_, -1, L_)
        if sv is None and self.instruction_encoder.last_cache is not None:
            self.instruction_encoder.last_cache.fold_behind = True  # (cached encoding, no fold made for its dirty rows)
        tk_ = ops.conv2d(t.view(r_, -1, 1, L_), self.text_k.weight.view(h2, -1, 1, 1), shift=self.text_k.bias,
                         splitk=False)
        return t, ln, tk_

    def _kv_branch(self, x, kv_conv, lin, out):
        """An image branch's tail: the k/v projection of the features x (rows, C, h, w) -> returned, and `lin` + ReLU of
        them -> `out` (a column block of state_in).  The projections depend only on their own encoder, so they run
        inside the branches: one launch for rollout batches, else the MFMA GEMM + the skinny linear."""
        r_, C_, P_ = x.shape[0], x.shape[1], x.shape[2] * x.shape[3]
        kv = ops.kv_linear(x, kv_conv.weight, kv_conv.bias, lin.weight, lin.bias, out)
        if kv is None:
            kv = ops.conv2d(x.view(r_, C_, 1, P_), kv_conv.weight.view(-1, C_, 1, 1), shift=kv_conv.bias, splitk=False)
            ops.linear(x.view(r_, -1), lin.weight, lin.bias, relu=True, out=out)
        return kv

    def _map_branch(self, observations, state_in, sv):
        """Semantic-map CNN -> (features (rows,128,4,4), k/v); map_linear fills its columns of state_in."""
        geo = self.step_geometry
        m = self.map_encoder(observations, sv)
        if self.model_config.ablate_map:
            m = torch.zeros_like(m)
        return m, self._kv_branch(m, self.map_kv, self.map_linear[1], state_in[:, geo.d_out:geo.d_out + geo.m_out])

    def _dep_branch(self, observations, state_in, sv=None):
        """Depth ResNet -> (features (rows,192,4,4), k/v); depth_linear fills its columns of state_in.  `sv`: a dict of the
        update pass that receives the visual encoder's per-layer saves when that encoder trains on depth frames
        (MODEL.DEPTH_ENCODER.trainable) and the branch is not ablated (its features are multiplied by 0 then: the
        encoder's gradient is exactly zero and nothing is saved); it stays empty otherwise."""
        want = (sv is not None and not self.model_config.ablate_depth and "depth_features" not in observations
                and self.depth_encoder.visual_encoder.trains)
        d = self.depth_encoder(observations, save=sv) if want else self.depth_encoder(observations)
        if self.model_config.ablate_depth:
            d = torch.zeros_like(d)
        return d, self._kv_branch(d, self.dep_kv, self.depth_linear[1], state_in[:, :self.step_geometry.d_out])

    def _prev_embed(self, prev_actions, masks_u8, state_in, x2):
        geo = self.step_geometry
        ops.prev_action_embed(prev_actions, masks_u8, self.prev_action_embedding.weight,
                              state_in[:, geo.d_out + geo.m_out:], x2[:, geo.o_prev:])

    def _head(self, rnn_states, masks_u8, state_in, x2, txt3, dep2, map2, fused_head, rnn_out=None, save=None, inv=None):
        """Recurrent / attention head over the three branches' results txt3 = (txt, lengths, tk), dep2 = (dep, dkv),
        map2 = (mp, mkv) -> (features (rows, H), rnn_out).  `rnn_out`: where the new states go (graphed.py: a persistent
        buffer).  The unfused chain leaves what the HIP backward needs of it in `save`."""
        (txt, lengths, tk), (dep, dkv), (mp, mkv) = txt3, dep2, map2
        geo, dev = self.step_geometry, rnn_states.device
        H, h2, rows = self._hidden_size, self._hidden_size // 2, masks_u8.shape[0]
        # (two key counts: the depth grid's P, and the map's Pm = (rows / 16) * (cols / 16) cells of the egocentric map)
        L, P, Pm = txt.shape[2], dep.shape[2] * dep.shape[3], mp.shape[2] * mp.shape[3]
        rnn_out = torch.empty_like(rnn_states) if rnn_out is None else rnn_out
        feats = torch.empty((rows, H), dtype=torch.float32, device=dev)
        if fused_head and P <= 16 and Pm == P and L <= 512 and tk.shape[1] == H + 1 + h2:
            # GRU-1 -> text attention -> depth / map attention -> compress -> GRU-2 as one C-ABI call (five phase kernels,
            # csrc/cma_step.hip); `tk` holds the folded [Mq | TQb] operand here.  With LSTM encoders the same descriptor
            # goes to the LSTM form: 4H weight rows, and the (rows, 4, H) states [h1 | c1 | h2 | c2]
            g1, g2, sc = self.state_encoder.rnn, self.second_state_encoder.rnn, self.second_state_compress[0]
            d = ops.CmaStepDesc()
            d.rows, d.L, d.P, d.H, d.Hq, d.Ct = rows, L, P, H, h2, txt.shape[1]
            d.d_out, d.m_out, d.E, d.x2w = geo.d_out, geo.m_out, geo.E, geo.x2w
            d.state_in, d.h_in, d.ld_h, d.mask = ops.dptr(state_in), ops.dptr(rnn_states), rnn_states.stride(0), ops.dptr(masks_u8)
            d.w_ih1, d.w_hh1, d.b_ih1, d.b_hh1 = (ops.dptr(g1.weight_ih_l0), ops.dptr(g1.weight_hh_l0),
                                                  ops.dptr(g1.bias_ih_l0), ops.dptr(g1.bias_hh_l0))
            d.Mq, d.Mq_img = ops._p(tk), tk.stride(0)
            d.TQb, d.TQb_img = ops._p(tk[:, H + 1:]), tk.stride(0)
            d.lengths, d.txt = ops.dptr(lengths), ops.dptr(txt)
            d.dkv, d.mkv, d.scale = ops.dptr(dkv), ops.dptr(mkv), self._scale_f
            d.w_c, d.b_c = ops.dptr(sc.weight), ops.dptr(sc.bias)
            d.w_ih2, d.w_hh2, d.b_ih2, d.b_hh2 = (ops.dptr(g2.weight_ih_l0), ops.dptr(g2.weight_hh_l0),
                                                  ops.dptr(g2.bias_ih_l0), ops.dptr(g2.bias_hh_l0))
            d.x2, d.h_out, d.ld_ho, d.feats = ops.dptr(x2), ops.dptr(rnn_out), rnn_out.stride(0), ops.dptr(feats)
            scratch, step = self._fused_head_ops(self.fused_head_form)
            d.ws = ops.dptr(scratch(rows, L, P, H, dev))
            step(d)
            return feats, rnn_out
        s_g1, s_g2 = ({}, {}) if save is not None else (None, None)
        state = x2[:, :H]
        n1, n2 = self.state_encoder.num_recurrent_layers, self.second_state_encoder.num_recurrent_layers
        self.state_encoder(state_in, self._state_slot(rnn_states, 0, n1), masks_u8, state,
                           self._state_slot(rnn_out, 0, n1), s_g1)

        q1 = ops.linear(state, self.state_q.weight, self.state_q.bias)
        a_txt = torch.empty((rows, L), dtype=torch.float32, device=dev) if save is not None else None
        text = x2[:, geo.o_txt:geo.o_dep]
        ops.attn(q1, tk.view(tk.shape[0], h2, L), txt, lengths, self._scale_f, text, a_txt, row_index=inv)

        dkv, mkv = dkv.view(rows, -1, P), mkv.view(rows, -1, Pm)
        q2 = ops.linear(text, self.text_q.weight, self.text_q.bias)
        a_dep = torch.empty((rows, P), dtype=torch.float32, device=dev) if save is not None else None
        a_map = torch.empty((rows, Pm), dtype=torch.float32, device=dev) if save is not None else None
        x2_dep, x2_map = x2[:, geo.o_dep:geo.o_map], x2[:, geo.o_map:geo.o_prev]
        if save is None and Pm == P and P <= 32:
            # rollout head: both short-axis attentions (they share the query) in one launch
            ops.attn_small2(q2, dkv[:, :h2], dkv[:, h2:], x2_dep, mkv[:, :h2], mkv[:, h2:], x2_map, self._scale_f)
        elif save is None and ops.ATTN_PAIR and max(P, Pm) <= 256:
            # a map of another size: the same launch with a key count per set (include/ivln_map_sizes.h)
            ops.attn_pair(q2, dkv[:, :h2], dkv[:, h2:], x2_dep, mkv[:, :h2], mkv[:, h2:], x2_map, self._scale_f)
        else:
            ops.attn(q2, dkv[:, :h2], dkv[:, h2:], None, self._scale_f, x2_dep, a_dep)
            ops.attn(q2, mkv[:, :h2], mkv[:, h2:], None, self._scale_f, x2_map, a_map)

        sc = self.second_state_compress[0]
        c2 = ops.linear(x2, sc.weight, sc.bias, relu=True)
        self.second_state_encoder(c2, self._state_slot(rnn_states, n1, n2), masks_u8, feats,
                                  self._state_slot(rnn_out, n1, n2), s_g2)

        if save is not None:
            save.update(
                g1=s_g1, g2=s_g2, dep=dep, mp=mp, txt_out=txt, lengths=lengths,
                state_in=state_in, x2=x2, q1=q1, tk=tk, a_txt=a_txt, dkv=dkv, mkv=mkv, q2=q2, a_dep=a_dep,
                a_map=a_map, c2=c2, feats=feats, rows=rows, L=L, P=P, Pm=Pm,
                offs=(geo.o_txt, geo.o_dep, geo.o_map, geo.o_prev), masks=masks_u8, inv=inv,
            )
        return feats, rnn_out

    # ------------------------------------------------------------------------------------------
    def forward_hip(self, observations, rnn_states, prev_actions, action_masks, save=None, *, side_streams=None,
                    rnn_out=None):
        """HIP forward of map_cma_policy.py:276-353.  Returns (features (rows,512), rnn_states_out
        (N, num_recurrent_layers, H)).  `save` (dict) collects what the HIP backward needs.  A captured rollout step
        (graphed.py) may name two `side_streams` to fork the instruction and map branches onto, and the buffer
        `rnn_out` the new states are written to."""
        dev = rnn_states.device
        rnn_states, masks_u8, prev_actions = self._step_inputs(rnn_states, prev_actions, action_masks)
        state_in, x2 = self.step_geometry.buffers(masks_u8.shape[0], dev)
        # (the fused head is ONE step of `rows` states: a time-major batch over fewer states takes the unfused chain)
        fused_head = self._fused_head_eligible(observations, save) and masks_u8.shape[0] == rnn_states.shape[0]
        s_txt, s_map = ({}, []) if save is not None else (None, None)
        s_dep = {} if save is not None else None  # (filled only by a trainable depth encoder: _dep_branch)

        # update batches: the instruction of a trajectory is the same at every timestep, so the loader hands over the
        # UNIQUE token rows and each row's index into them (trainers.PrefetchLoader); the encoder, text_k and their
        # backward then run on U sequences instead of T*N (8-9 instead of 512 at the benched shape)
        inv = None
        ikey = self.instruction_encoder.obs_key
        if save is not None and ikey + "_index" in observations and ikey + "_unique" in observations:
            inv = observations[ikey + "_index"].reshape(-1).to(torch.int32).contiguous()

        if side_streams is None:
            from . import train as _train

            overlap = save is not None and _train.OVERLAP_INSTRUCTION and not torch.cuda.is_current_stream_capturing()
            if overlap:  # training pass: the instruction bi-LSTM runs beside the map CNN (train.py)
                cur, st = torch.cuda.current_stream(), _train.side_stream(dev)
                st.wait_stream(cur)
                _train.share_with_stream((observations.get(ikey), observations.get(ikey + "_unique")), st)
                with torch.cuda.stream(st):
                    txt3 = self._txt_branch(observations, fused_head, s_txt, inv)
            else:
                txt3 = self._txt_branch(observations, fused_head, s_txt, inv)
            dep2 = self._dep_branch(observations, state_in, s_dep)
            map2 = self._map_branch(observations, state_in, s_map)
            if overlap:
                cur.wait_stream(st)
                _train.share_with_stream((*txt3, s_txt), cur)
        else:
            # three independent, latency-bound branches on forked streams (graphed.py): depth ResNet
            # (critical path, submitted first) || instruction bi-LSTM || (mapper ->) map CNN
            cur = torch.cuda.current_stream()
            st_txt, st_map = side_streams
            st_txt.wait_stream(cur)
            st_map.wait_stream(cur)
            dep2 = self._dep_branch(observations, state_in)
            with torch.cuda.stream(st_txt):
                txt3 = self._txt_branch(observations, fused_head, None)
            with torch.cuda.stream(st_map):
                map2 = self._map_branch(observations, state_in, None)
            cur.wait_stream(st_txt)
            cur.wait_stream(st_map)
        self._prev_embed(prev_actions, masks_u8, state_in, x2)
        feats, rnn_out = self._head(rnn_states, masks_u8, state_in, x2, txt3, dep2, map2, fused_head, rnn_out, save, inv)
        if save is not None:
            save.update(txt=s_txt, map=s_map, depth_enc=s_dep or None, N=rnn_states.shape[0], prev_actions=prev_actions,
                        depth_from_features="depth_features" in observations)
        return feats, rnn_out

    # ---- the same step as the three graphs of graphed.GraphedRollout's split mode: `step` is the runner's SplitStep, and
    #      what a stage returns lives in its graph's pool - the runner keeps it and hands it to the next stage
    def stage_depth(self, observations, rnn_states, prev_actions, action_masks, step):
        """Depth ResNet + its k/v projection + depth_linear as one graph on a side stream (they depend on nothing but
        the new depth image); results land in the persistent buffers.  -> (dep2, txt3 or None)."""
        # (every stage converts the step's inputs, used or not: the conversions are launches, kept so that the three graphs
        #  stay launch for launch what they were - dropping the unused ones changes the graphs: a measured follow-up)
        self._step_inputs(rnn_states, prev_actions, action_masks)
        fused_head = self._fused_head_eligible(observations, None)
        txt3 = None
        if step.txt_with_dep == "first":
            # 8 images: the persistent depth encoder leaves no XCD for the bi-LSTM, which then runs in front of it
            txt3 = self._txt_branch(observations, fused_head, None)
        dep2 = self._dep_branch(observations, step.state_in)
        if step.txt_with_dep is True:
            # predicted semantics: the main stream is RedNet's critical path, the instruction encoder moves here
            txt3 = self._txt_branch(observations, fused_head, None)
        return dep2, txt3

    def stage_pre(self, observations, rnn_states, prev_actions, action_masks, step, txt3=None):
        """... while the instruction and map branches (and the previous-action embedding) run as a second graph on
        the main stream.  `txt3`: the instruction branch's result when stage_depth ran it.  -> (txt3, map2)."""
        _, masks_u8, prev_actions = self._step_inputs(rnn_states, prev_actions, action_masks)
        fused_head = self._fused_head_eligible(observations, None)
        # (order: when the persistent depth encoder is the neighbour, the bi-LSTM - 340 registers per SIMD lane - cannot
        #  be scheduled before that launch ends; last in this graph it delays nothing else - graphed.py sets txt_last)
        last = step.txt_last and not step.txt_with_dep
        if not last and not step.txt_with_dep:
            txt3 = self._txt_branch(observations, fused_head, None)
        map2 = self._map_branch(observations, step.state_in, None)
        if last:
            txt3 = self._txt_branch(observations, fused_head, None)
        self._prev_embed(prev_actions, masks_u8, step.state_in, step.x2)
        return txt3, map2

    def stage_post(self, observations, rnn_states, prev_actions, action_masks, step, dep2, pre, rnn_out=None):
        """The head, behind both other graphs: `dep2` from stage_depth, `pre` = (txt3, map2) from stage_pre."""
        rnn_states, masks_u8, _ = self._step_inputs(rnn_states, prev_actions, action_masks)
        return self._head(rnn_states, masks_u8, step.state_in, step.x2, pre[0], dep2, pre[1],
                          self._fused_head_eligible(observations, None), rnn_out)

    def forward(self, observations, rnn_states, prev_actions, action_masks, episode_masks=None, tour_masks=None):
        """Same signature/return as the reference forward (map_cma_policy.py:276-368); the MapCMA net
        only consumes `action_masks` (episode/tour masks default to it, :284-287)."""
        from .train import MapCMAForwardFn, all_params

        needs_grad = torch.is_grad_enabled() and any(p.requires_grad for p in all_params(self))
        if needs_grad:
            feats, rnn_out = MapCMAForwardFn.run(self, observations, rnn_states, prev_actions, action_masks)
        else:
            feats, rnn_out = self.forward_hip(observations, rnn_states, prev_actions, action_masks)
        if self.model_config.PROGRESS_MONITOR.use and AuxLosses.is_active():
            from .train import progress_monitor_loss

            loss = progress_monitor_loss(self, feats, observations["progress"])
            AuxLosses.register_loss("progress_monitor", loss, self.model_config.PROGRESS_MONITOR.alpha)
        return feats, rnn_out


class ILPolicy(Policy):
    """models/policy.py:12-83."""

    def __init__(self, net, dim_actions):
        nn.Module.__init__(self)
        self.net = net
        self.dim_actions = dim_actions
        self.action_distribution = CategoricalNet(self.net.output_size, self.dim_actions)

    def forward(self, *x):
        raise NotImplementedError

    # keys a collection loop adds to the observation dict to have the sampled action drawn (and beta-mixed) on the
    # device from host-supplied uniforms; without them `sample()` is torch's own Categorical draw
    U_SAMPLE, U_BETA = "_u_sample", "_u_beta"
    collect_mix = None  # {"beta": float, "expert_uuid": str} while a DAgger collection mixes in-kernel

    def _act(self, features, deterministic, observations=None, out=None):
        """Action head.  `out`: the buffer a captured step (graphed.py) wants the action kernel to write into."""
        lin = self.action_distribution.linear
        small = features.is_cuda and lin.out_features <= 8 and features.stride(-1) == 1
        if deterministic:  # distribution.mode() == argmax of probs == argmax of logits: head + argmax, one launch
            if small:
                return ops.linear_argmax(features, lin.weight, lin.bias, out=out)
            logits = self.action_distribution.raw_logits(features)
            return ops.argmax_rows(logits.contiguous(), out=out)
        if small and observations is not None and self.U_SAMPLE in observations:
            # inverse-CDF draw from the caller's uniforms (+ expert mixing / the -1 rule of a DAgger collection) in the
            # head's own launch: a pure function of the step's inputs, so the sampled step replays as a hipGraph
            mix = self.collect_mix
            u_beta = observations.get(self.U_BETA) if mix else None
            expert = observations[mix["expert_uuid"]].view(-1) if mix else None
            return ops.linear_sample(features, lin.weight, lin.bias, observations[self.U_SAMPLE].view(-1),
                                     None if u_beta is None else u_beta.view(-1), mix["beta"] if mix else 0.0, expert,
                                     out=out)
        logits = self.action_distribution.raw_logits(features)
        return CustomFixedCategorical(logits=logits).sample()

    def act(self, observations, rnn_states, prev_actions, masks, deterministic=False):
        features, rnn_states = self.net(observations, rnn_states, prev_actions, masks)
        return self._act(features, deterministic, observations), rnn_states

    def act_iterative(self, observations, rnn_hidden_states, prev_actions, agent_episode_not_done_masks,
                      sim_episode_not_done_masks, tour_not_done_masks, action_masks, deterministic=False):
        return self.act(observations, rnn_hidden_states, prev_actions, agent_episode_not_done_masks,
                        deterministic=deterministic)

    def get_value(self, *args, **kwargs):
        raise NotImplementedError

    def evaluate_actions(self, *args, **kwargs):
        raise NotImplementedError

    def build_distribution(self, observations, rnn_states, prev_actions, masks) -> CustomFixedCategorical:
        features, rnn_states = self.net(observations, rnn_states, prev_actions, masks)
        return self.action_distribution(features)


@baseline_registry.register_policy
class MapCMAPolicy(ILPolicy):
    def __init__(self, observation_space, action_space, config):
        super().__init__(
            MapCMANet(observation_space=observation_space, config=config, num_actions=action_space.n),
            action_space.n,
        )

    def act_iterative(self, observations, rnn_hidden_states, prev_actions, agent_episode_not_done_masks,
                      sim_episode_not_done_masks, tour_not_done_masks, action_masks, deterministic=False):
        # quirk Q11: only the agent-episode mask reaches the net (map_cma_policy.py:56-63)
        features, rnn_hidden_states = self.net(
            observations, rnn_hidden_states, prev_actions, action_masks=agent_episode_not_done_masks,
            episode_masks=None, tour_masks=None,
        )
        return self._act(features, deterministic, observations), rnn_hidden_states

    def build_features(self, observations, rnn_hidden_states, prev_actions, agent_episode_not_done_masks,
                       tour_not_done_masks=None) -> Tuple[Tensor, Tensor]:
        """The net half of `build_distribution` (the fused CE kernel of the HIP update takes raw logits)."""
        return self.net(observations, rnn_hidden_states, prev_actions, action_masks=agent_episode_not_done_masks)

    def build_distribution(self, observations, rnn_hidden_states, prev_actions, agent_episode_not_done_masks,
                           tour_not_done_masks=None) -> Tuple[CustomFixedCategorical, Tensor]:
        features, rnn_hidden_states = self.build_features(observations, rnn_hidden_states, prev_actions,
                                                          agent_episode_not_done_masks, tour_not_done_masks)
        return self.action_distribution(features), rnn_hidden_states

    @classmethod
    def from_config(cls, config, observation_space, action_space):
        return cls(observation_space=observation_space, action_space=action_space, config=config)
