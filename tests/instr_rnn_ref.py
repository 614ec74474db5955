"""TEST INFRASTRUCTURE ONLY - float64 / float32 torch references of the instruction encoder's options
(`MODEL.INSTRUCTION_ENCODER.rnn_type` GRU | LSTM, `bidirectional` True | False), shared by
tests/test_instruction_options_host.py and tests/test_gpu_instruction_options.py.

  module_ref    torch.nn.GRU / nn.LSTM on pack_padded_sequence, which is what the reference calls.  Its input is
                [gx_f | gx_r] and W_ih a selector ([I | 0], [0 | I]) with b_ih = 0, so the leaf's gradient is the gradient of
                the input-side gate pre-activations (the recipe of tests/test_gpu_train_kernels.py::_lstm_ref)
  gru_cell_loop the same GRU written out cell by cell: nn.GRU does not expose W_hh h + b_hh, whose gradient (dgh: the n
                rows carry the factor r) the kernel has to produce.  The host test pins the loop to nn.GRU at 1e-12.
  options_config / make_policy / oracle nets: the small policy configs of the GPU tests and a torch oracle that swaps only
                the instruction encoder (and the layers whose width follows it).
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))  # det_init

COMBOS = [("LSTM", True), ("LSTM", False), ("GRU", True), ("GRU", False)]
NON_DEFAULT = COMBOS[1:]
SFX = ("", "_reverse")


def gates_of(cell):
    return 3 if cell == "GRU" else 4


def module_ref(cell, ndir, gx, whh, bhh, lens, dout, B, L, H, dt):
    """gx / whh / bhh: one tensor per direction; lens >= 1.  -> dict(out (B, ndir*H, L), dgi [(B*L, G)], hp [(B*L, H)])"""
    G = gates_of(cell) * H
    rnn = getattr(nn, cell)(ndir * G, H, bidirectional=ndir == 2, batch_first=True).to(dt)
    with torch.no_grad():
        for d in range(ndir):
            sel = torch.zeros(G, ndir * G, dtype=dt)
            sel[:, d * G:(d + 1) * G] = torch.eye(G, dtype=dt)
            getattr(rnn, "weight_ih_l0" + SFX[d]).copy_(sel)
            getattr(rnn, "bias_ih_l0" + SFX[d]).zero_()
            getattr(rnn, "weight_hh_l0" + SFX[d]).copy_(whh[d].to(dt))
            getattr(rnn, "bias_hh_l0" + SFX[d]).copy_(bhh[d].to(dt))
    x = torch.cat([g.view(B, L, G) for g in gx], 2).to(dt).requires_grad_(True)
    packed = nn.utils.rnn.pack_padded_sequence(x, torch.tensor(lens), batch_first=True, enforce_sorted=False)
    out = nn.utils.rnn.pad_packed_sequence(rnn(packed)[0], batch_first=True, total_length=L)[0]  # (B, L, ndir*H)
    (out.permute(0, 2, 1) * dout.to(dt)).sum().backward()
    out = out.detach()
    hp = [torch.zeros(B, L, H, dtype=dt) for _ in range(ndir)]
    for b, n in enumerate(lens):  # h_{t-1} in processing order
        hp[0][b, 1:n] = out[b, :n - 1, :H]
        if ndir == 2:
            hp[1][b, :n - 1] = out[b, 1:n, H:]
    return dict(out=out.permute(0, 2, 1).contiguous(), dgi=[x.grad[:, :, d * G:(d + 1) * G].reshape(B * L, G) for d in range(ndir)],
                hp=[h.view(B * L, H) for h in hp])


def gru_cell_loop(ndir, gx, whh, bhh, lens, dout, B, L, H, dt):
    """torch's GRU cell by hand over each row's own length (gate order r, z, n), with autograd.
    -> dict(out, dgi, hp as module_ref; dgh [(B*L, 3H)] = d(loss)/d(W_hh h + b_hh))"""
    G = 3 * H
    xs = [g.view(B, L, G).to(dt).clone().requires_grad_(True) for g in gx]
    out = torch.zeros(B, ndir * H, L, dtype=dt)
    hp = [torch.zeros(B, L, H, dtype=dt) for _ in range(ndir)]
    ghs, total = {}, torch.zeros((), dtype=dt)
    for d in range(ndir):
        W, bb = whh[d].to(dt), bhh[d].to(dt)
        for b, n in enumerate(lens):
            h = torch.zeros(H, dtype=dt)
            for t in (range(n) if d == 0 else range(n - 1, -1, -1)):
                hp[d][b, t] = h.detach()
                gi, gh = xs[d][b, t], W @ h + bb
                gh = gh.requires_grad_(True) if gh.is_leaf else gh  # (first step: h = 0 and constants - a leaf of its own)
                gh.retain_grad()
                ghs[(d, b, t)] = gh
                r, z = torch.sigmoid(gi[:H] + gh[:H]), torch.sigmoid(gi[H:2 * H] + gh[H:2 * H])
                nn_ = torch.tanh(gi[2 * H:] + r * gh[2 * H:])
                h = (1 - z) * nn_ + z * h
                out[b, d * H:(d + 1) * H, t] = h.detach()
                total = total + (h * dout[b, d * H:(d + 1) * H, t].to(dt)).sum()
    total.backward()
    dgh = [torch.zeros(B, L, G, dtype=dt) for _ in range(ndir)]
    for (d, b, t), gh in ghs.items():
        dgh[d][b, t] = gh.grad
    return dict(out=out, dgi=[x.grad.reshape(B * L, G) for x in xs], dgh=[g.view(B * L, G) for g in dgh],
                hp=[h.view(B * L, H) for h in hp])


def make_case(cell, ndir, B, L, H=128):
    g = torch.Generator().manual_seed(1000 * B + 10 * L + ndir + (5 if cell == "GRU" else 0))
    G = gates_of(cell) * H
    return dict(gx=[torch.randn(B * L, G, generator=g) * 0.6 for _ in range(ndir)],
                whh=[torch.randn(G, H, generator=g) * 0.07 for _ in range(ndir)],
                bhh=[torch.randn(G, generator=g) * 0.1 for _ in range(ndir)],
                dout=torch.randn(B, ndir * H, L, generator=g))


# ------------------------------------------------------------------------------------------------------------------
# policies
# ------------------------------------------------------------------------------------------------------------------
def options_config(cell, bidirectional, policy_name="MapCMAPolicy", use_pm=False, extra=()):
    from ivln_ce_amd.config import get_config

    return get_config(opts=[
        "MODEL.policy_name", policy_name, "MODEL.INSTRUCTION_ENCODER.use_pretrained_embeddings", False,
        "MODEL.DEPTH_ENCODER.ddppo_checkpoint", "NONE", "MODEL.PROGRESS_MONITOR.use", use_pm,
        "MODEL.INSTRUCTION_ENCODER.rnn_type", cell, "MODEL.INSTRUCTION_ENCODER.bidirectional", bidirectional, *extra,
    ])


def policy_space(policy_name="MapCMAPolicy"):
    from ivln_ce_amd.spaces import Box, Dict

    if policy_name == "LatentCMAPolicy":
        return Dict({"depth": Box(0.0, 1.0, (256, 256, 1), np.float32), "rgb": Box(0, 255, (224, 224, 3), np.uint8),
                     "instruction": Box(0, 2504, (200,), np.int64)})
    return Dict({
        "depth": Box(0.0, 1.0, (256, 256, 1), np.float32), "occupancy_map": Box(0, 255, (64, 64), np.uint8),
        "semantic_map": Box(0, 255, (64, 64), np.uint8), "instruction": Box(0, 2504, (200,), np.int64),
    })


def make_policy(cell, bidirectional, policy_name="MapCMAPolicy", use_pm=False, fill=True):
    """The policy of that instruction-encoder combination on the CPU, filled by the shared deterministic initialiser"""
    from det_init import det_fill

    import ivln_ce_amd  # noqa: F401
    from ivln_ce_amd import latent_policy, policy  # noqa: F401
    from ivln_ce_amd.registry import baseline_registry
    from ivln_ce_amd.spaces import Discrete

    pol = baseline_registry.get_policy(policy_name).from_config(
        options_config(cell, bidirectional, policy_name, use_pm), policy_space(policy_name), Discrete(4))
    if fill:
        det_fill(pol, seed=0, conv_gain=1.0 if policy_name == "LatentCMAPolicy" else 2.0 ** 0.5)
    return pol


class InstructionEncoderOptRef(nn.Module):
    """instruction_encoder.py:11-94 with its two options: the torch module on packed sequences"""

    def __init__(self, cell, bidirectional, vocab=2504, emb=50, hidden=128):
        super().__init__()
        self.encoder_rnn = getattr(nn, cell)(input_size=emb, hidden_size=hidden, bidirectional=bidirectional)
        self.embedding_layer = nn.Embedding(vocab, emb, padding_idx=0)
        self.output_size = hidden * (1 + int(bidirectional))

    def forward(self, obs, total_length=None):
        x = self.embedding_layer(obs["instruction"].long())
        lengths = ((x != 0.0).long().sum(dim=2) != 0).long().sum(dim=1).cpu()
        packed = nn.utils.rnn.pack_padded_sequence(x, lengths, batch_first=True, enforce_sorted=False)
        out, _ = self.encoder_rnn(packed)
        return nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=total_length)[0].permute(0, 2, 1)


def mapcma_oracle(cell, bidirectional, use_pm=False):
    """oracle.policy_ref.MapCMAPolicyRef with only the instruction encoder (and the three layers whose width follows it)
    swapped; forward / logits / update_loss are the oracle's own"""
    from oracle.policy_ref import MapCMAPolicyRef

    ref = MapCMAPolicyRef(use_pm=use_pm)
    net = ref.net
    enc = InstructionEncoderOptRef(cell, bidirectional)
    Ct, hidden = enc.output_size, net._hidden_size
    net.instruction_encoder = enc
    net.text_k = nn.Conv1d(Ct, hidden // 2, 1)
    net.text_q = nn.Linear(Ct, hidden // 2)
    old = net.second_state_compress[0]
    net.second_state_compress = nn.Sequential(nn.Linear(old.in_features - 256 + Ct, hidden), nn.ReLU(True))
    return ref


class _FeaturesPlusSpatialRef(nn.Module):
    """An image encoder fed with its cached backbone features (`<name>_features`, as the trainers feed updates): the
    (B, C, 4, 4) features followed by the learned (16, 64) spatial table viewed raw as (64, 4, 4)"""

    def __init__(self, key, channels):
        super().__init__()
        self.key = key
        self.spatial_embeddings = nn.Embedding(16, 64)
        self.output_shape = (channels + 64, 4, 4)

    def forward(self, obs):
        x = obs[self.key]
        sp = self.spatial_embeddings.weight.view(1, 64, 4, 4).expand(x.size(0), 64, 4, 4)
        return torch.cat([x, sp.to(x.dtype)], dim=1)


class LatentCMANetOptRef(nn.Module):
    """Test-local torch oracle of the Latent-CMA head (episodic memory, no tour-memory slot) on cached image features, with
    the instruction encoder's options: two GRU state encoders, text attention keyed by the first state, RGB / depth
    attentions keyed by the attended text.  Module names are the policy's, so its state dict loads strictly once the two
    frozen backbones (not part of this oracle) are left out."""

    def __init__(self, cell, bidirectional, num_actions=4, hidden=512, rgb_out=256, depth_out=128):
        super().__init__()
        from oracle import habitat_ext_ref as ext

        self._hidden_size = hidden
        self.instruction_encoder = InstructionEncoderOptRef(cell, bidirectional)
        Ct = self.instruction_encoder.output_size
        self.depth_encoder = _FeaturesPlusSpatialRef("depth_features", 128)
        self.rgb_encoder = _FeaturesPlusSpatialRef("rgb_features", 2048)
        self.prev_action_embedding = nn.Embedding(num_actions + 1, 32)
        self.rgb_linear = nn.Sequential(nn.AdaptiveAvgPool1d(1), nn.Flatten(), nn.Linear(2112, rgb_out), nn.ReLU(True))
        self.depth_linear = nn.Sequential(nn.Flatten(), nn.Linear(192 * 16, depth_out), nn.ReLU(True))
        self.state_encoder = ext.build_rnn_state_encoder(rgb_out + depth_out + 32, hidden, "GRU", 1)
        self.rgb_kv = nn.Conv1d(2112, hidden // 2 + rgb_out, 1)
        self.depth_kv = nn.Conv1d(192, hidden // 2 + depth_out, 1)
        self.state_q = nn.Linear(hidden, hidden // 2)
        self.text_k = nn.Conv1d(Ct, hidden // 2, 1)
        self.text_q = nn.Linear(Ct, hidden // 2)
        self.register_buffer("_scale", torch.tensor(1.0 / ((hidden // 2) ** 0.5)))
        self.second_state_compress = nn.Sequential(nn.Linear(hidden + Ct + rgb_out + depth_out + 32, hidden), nn.ReLU(True))
        self.second_state_encoder = ext.build_rnn_state_encoder(hidden, hidden, "GRU", 1)
        self.progress_monitor = nn.Linear(hidden, 1)
        self.output_size = hidden

    def _attn(self, q, k, v, mask=None):
        logits = torch.einsum("nc, nci -> ni", q, k)
        if mask is not None:
            logits = logits - mask.to(logits.dtype) * 1e8
        return torch.einsum("ni, nci -> nc", torch.softmax(logits * self._scale, dim=1), v)

    def forward(self, obs, rnn_states, prev_actions, masks):
        txt = self.instruction_encoder(obs)
        dep = torch.flatten(self.depth_encoder(obs), 2)
        rgb = torch.flatten(self.rgb_encoder(obs), 2)
        pa = self.prev_action_embedding(((prev_actions.to(txt.dtype) + 1) * masks).long().view(-1))
        state_in = torch.cat([self.rgb_linear(rgb), self.depth_linear(dep), pa], dim=1)
        out_states = rnn_states.detach().clone()
        state, out_states[:, 0:1] = self.state_encoder(state_in, rnn_states[:, 0:1], masks)
        text = self._attn(self.state_q(state), self.text_k(txt), txt, (txt == 0.0).all(dim=1))
        h2 = self._hidden_size // 2
        rgb_k, rgb_v = torch.split(self.rgb_kv(rgb), h2, dim=1)
        dep_k, dep_v = torch.split(self.depth_kv(dep), h2, dim=1)
        tq = self.text_q(text)
        x = torch.cat([state, text, self._attn(tq, rgb_k, rgb_v), self._attn(tq, dep_k, dep_v), pa], dim=1)
        x = self.second_state_compress(x)
        x, out_states[:, 1:2] = self.second_state_encoder(x, rnn_states[:, 1:2], masks)
        return x, out_states


class LatentCMAPolicyOptRef(nn.Module):
    BACKBONES = ("net.rgb_encoder.cnn.", "net.depth_encoder.visual_encoder.")

    def __init__(self, cell, bidirectional, num_actions=4):
        super().__init__()
        from oracle.policy_ref import _CategoricalNetRef

        self.net = LatentCMANetOptRef(cell, bidirectional, num_actions)
        self.action_distribution = _CategoricalNetRef(self.net.output_size, num_actions)

    def load_from(self, pol):
        """strict, from the HIP policy's state dict without the two frozen backbones"""
        self.load_state_dict({k: v.cpu() for k, v in pol.state_dict().items() if not k.startswith(self.BACKBONES)})
        return self

    def logits(self, obs, rnn_states, prev_actions, masks):
        feats, states = self.net(obs, rnn_states, prev_actions, masks)
        return self.action_distribution(feats), states, feats

    def update_loss(self, obs, prev_actions, not_done_masks, corrected_actions, weights):
        """the inflection-weighted cross entropy of one DAgger update over a time-major (T, N) batch, zero initial state"""
        T, N = corrected_actions.size()
        h0 = torch.zeros(N, 2, self.net._hidden_size, dtype=weights.dtype)
        logits, _, _ = self.logits(obs, h0, prev_actions, not_done_masks)
        ce = torch.nn.functional.cross_entropy(logits.view(T, N, -1).permute(0, 2, 1), corrected_actions, reduction="none")
        return ((weights * ce).sum(0) / weights.sum(0)).mean()
