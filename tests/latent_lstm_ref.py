"""TEST INFRASTRUCTURE ONLY - a torch oracle of the Latent-CMA head with two LSTM state encoders
(`MODEL.STATE_ENCODER.rnn_type: LSTM`), the tour-long memory slot and `memory_at_end`, shared by
tests/test_latent_lstm_host.py and tests/test_gpu_latent_lstm.py.  Hand-written after
ivlnce_baselines/models/latent_cma_policy.py:124-179 (build_distribution) and :375-497 (forward) in the style of
tests/instr_rnn_ref.LatentCMANetOptRef, which has GRU encoders and no memory slot; it runs in the dtype it is cast to
(float64 in the tests) on cached image features.

State (N, L, H): [h1, c1, h2, c2] and, with `tour_memory_variant`, the memory at index 4.
LSTM + `tour_memory_variant`: the reference raises there (it max-pools the (N, 1, H) slot with the (N, 2, H) [h | c] slice;
tests/golden/latent_lstm_tour.npz records the exception).  The definition of this project ("Recurrent state
encoders"): the slot is pooled with h, slot 0 of the first encoder - the encoder's output, as in the GRU case.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from instr_rnn_ref import InstructionEncoderOptRef, _FeaturesPlusSpatialRef
from lstm_state_ref import LSTMStateEncoderRef

MODES = ("plain", "tour", "variant")


def mode_opts(mode):
    """the config keys of a memory mode, as tests/golden/gen_latent_update_golden.py sets them"""
    return ["MODEL.tour_memory", mode == "tour", "MODEL.tour_memory_variant", mode == "variant",
            "MODEL.memory_at_end", mode == "variant"]


def latent_config(rnn_type, mode, use_pm=False, extra=()):
    from ivln_ce_amd.config import get_config

    return get_config(opts=["MODEL.policy_name", "LatentCMAPolicy", "MODEL.INSTRUCTION_ENCODER.use_pretrained_embeddings",
                            False, "MODEL.DEPTH_ENCODER.ddppo_checkpoint", "NONE", "MODEL.PROGRESS_MONITOR.use", use_pm,
                            "MODEL.STATE_ENCODER.rnn_type", rnn_type, "MODEL.STATE_ENCODER.latent_lstm", rnn_type != "GRU",
                            *mode_opts(mode), *extra])


def make_policy(rnn_type, mode, use_pm=False, fill=True, extra=()):
    """LatentCMAPolicy of that state-encoder type and memory mode on the CPU, filled by the shared initialiser"""
    from det_init import det_fill
    from instr_rnn_ref import policy_space

    import ivln_ce_amd  # noqa: F401
    from ivln_ce_amd import latent_policy  # noqa: F401
    from ivln_ce_amd.registry import baseline_registry
    from ivln_ce_amd.spaces import Discrete

    pol = baseline_registry.get_policy("LatentCMAPolicy").from_config(
        latent_config(rnn_type, mode, use_pm, extra), policy_space("LatentCMAPolicy"), Discrete(4))
    return det_fill(pol, seed=0, conv_gain=1.0) if fill else pol


class LatentCMANetLSTMRef(nn.Module):
    def __init__(self, mode, use_pm=False, pm_alpha=1.0, num_actions=4, hidden=512, rgb_out=256, depth_out=128):
        super().__init__()
        assert mode in MODES
        self.variant = mode == "variant"
        self.memory_at_end = mode == "variant"
        self.use_pm, self.pm_alpha = use_pm, pm_alpha
        self._hidden_size = hidden
        self.instruction_encoder = InstructionEncoderOptRef("LSTM", True)
        Ct = self.instruction_encoder.output_size
        self.depth_encoder = _FeaturesPlusSpatialRef("depth_features", 128)
        self.rgb_encoder = _FeaturesPlusSpatialRef("rgb_features", 2048)
        self.prev_action_embedding = nn.Embedding(num_actions + 1, 32)
        self.rgb_linear = nn.Sequential(nn.AdaptiveAvgPool1d(1), nn.Flatten(), nn.Linear(2112, rgb_out), nn.ReLU(True))
        self.depth_linear = nn.Sequential(nn.Flatten(), nn.Linear(192 * 16, depth_out), nn.ReLU(True))
        self.state_encoder = LSTMStateEncoderRef(rgb_out + depth_out + 32 + (hidden if self.variant else 0), hidden)
        self.rgb_kv = nn.Conv1d(2112, hidden // 2 + rgb_out, 1)
        self.depth_kv = nn.Conv1d(192, hidden // 2 + depth_out, 1)
        self.state_q = nn.Linear(hidden, hidden // 2)
        self.text_k = nn.Conv1d(Ct, hidden // 2, 1)
        self.text_q = nn.Linear(Ct, hidden // 2)
        self.register_buffer("_scale", torch.tensor(1.0 / ((hidden // 2) ** 0.5)))
        self.second_state_compress = nn.Sequential(nn.Linear(hidden + Ct + rgb_out + depth_out + 32, hidden), nn.ReLU(True))
        self.second_state_encoder = LSTMStateEncoderRef(hidden, hidden)
        if self.memory_at_end:
            self.out_layer = nn.Sequential(nn.Linear(hidden * 2, hidden), nn.ReLU(True))
        self.progress_monitor = nn.Linear(hidden, 1)
        self.output_size = hidden
        self.num_recurrent_layers = 4 + int(self.variant)
        self.aux = []

    def _attn(self, q, k, v, mask=None):
        logits = torch.einsum("nc, nci -> ni", q, k)
        if mask is not None:
            logits = logits - mask.to(logits.dtype) * 1e8
        return torch.einsum("ni, nci -> nc", torch.softmax(logits * self._scale, dim=1), v)

    def forward(self, obs, rnn_states, prev_actions, action_masks, episode_masks=None, tour_masks=None, want_aux=False):
        """latent_cma_policy.py:375-497; rows == N, or T*N time-major in the modes the reference runs as a sequence"""
        episode_masks = action_masks if episode_masks is None else episode_masks
        tour_masks = episode_masks if tour_masks is None else tour_masks
        dt = rnn_states.dtype
        rnn_states = rnn_states.clone()
        if self.variant:
            rnn_states[:, 4:] = tour_masks.view(-1, 1, 1).to(dt) * rnn_states[:, 4:]
        txt = self.instruction_encoder(obs)
        dep = torch.flatten(self.depth_encoder(obs), 2)
        rgb = torch.flatten(self.rgb_encoder(obs), 2)
        pa = self.prev_action_embedding(((prev_actions.to(dt) + 1) * action_masks.to(dt)).long().view(-1))
        state_inputs = [self.rgb_linear(rgb), self.depth_linear(dep), pa]
        if self.variant:
            state_inputs.append(rnn_states[:, 4])
        out_states = rnn_states.detach().clone()
        state, out_states[:, 0:2] = self.state_encoder(torch.cat(state_inputs, dim=1), rnn_states[:, 0:2], episode_masks)
        if self.variant:
            with torch.no_grad():  # pooled with h, the encoder's output: THIS project's definition for the LSTM
                out_states[:, 4] = torch.max(out_states[:, 4], out_states[:, 0])
        text = self._attn(self.state_q(state), self.text_k(txt), txt, (txt == 0.0).all(dim=1))
        h2 = self._hidden_size // 2
        rgb_k, rgb_v = torch.split(self.rgb_kv(rgb), h2, dim=1)
        dep_k, dep_v = torch.split(self.depth_kv(dep), h2, dim=1)
        tq = self.text_q(text)
        x = torch.cat([state, text, self._attn(tq, rgb_k, rgb_v), self._attn(tq, dep_k, dep_v), pa], dim=1)
        x = self.second_state_compress(x)
        x, out_states[:, 2:4] = self.second_state_encoder(x, rnn_states[:, 2:4], episode_masks)
        if self.memory_at_end:
            x = self.out_layer(torch.cat([x, rnn_states[:, 4]], dim=1))
        if self.use_pm and want_aux:
            hat = torch.tanh(self.progress_monitor(x))
            # (the reference's shapes, :485-490: (rows,) against (rows, 1) broadcast to (rows, rows))
            self.aux.append((F.mse_loss(hat.squeeze(1), obs["progress"], reduction="none"), self.pm_alpha))
        return x, out_states


class LatentCMAPolicyLSTMRef(nn.Module):
    BACKBONES = ("net.rgb_encoder.cnn.", "net.depth_encoder.visual_encoder.")

    def __init__(self, mode, use_pm=False, num_actions=4, train_unrolled=False):
        super().__init__()
        from oracle.policy_ref import _CategoricalNetRef

        self.mode, self.train_unrolled = mode, train_unrolled
        self.net = LatentCMANetLSTMRef(mode, use_pm, num_actions=num_actions)
        self.action_distribution = _CategoricalNetRef(self.net.output_size, num_actions)

    def load_from(self, pol):
        """strict, from the HIP policy's state dict without the two frozen backbones"""
        self.load_state_dict({k: v.cpu() for k, v in pol.state_dict().items() if not k.startswith(self.BACKBONES)})
        return self

    def act_step(self, obs, rnn_states, prev_actions, ep_masks, tour_masks):
        """act_iterative's mask routing (latent_cma_policy.py:60-92) -> logits, states, features"""
        if self.mode == "variant":
            feats, states = self.net(obs, rnn_states, prev_actions, ep_masks, ep_masks, tour_masks)
        else:
            feats, states = self.net(obs, rnn_states, prev_actions, ep_masks, tour_masks if self.mode == "tour" else None)
        return self.action_distribution(feats), states, feats

    def build_logits(self, obs, rnn_states, prev_actions, ep_masks, tour_masks, want_aux=False):
        """build_distribution (latent_cma_policy.py:124-179) over time-major rows -> logits (T*N, A), states, features"""
        self.net.aux = []
        N = rnn_states.size(0)
        T = ep_masks.size(0) // N
        if self.mode == "variant" or self.train_unrolled:
            feats = []
            for t in range(T):
                sl = slice(t * N, (t + 1) * N)
                f, rnn_states = self.net({k: v[sl] for k, v in obs.items()}, rnn_states, prev_actions[sl], ep_masks[sl],
                                         ep_masks[sl], tour_masks[sl], want_aux)
                feats.append(f)
            feats = torch.cat(feats, 0)
        else:
            feats, rnn_states = self.net(obs, rnn_states, prev_actions, ep_masks, tour_masks if self.mode == "tour" else None,
                                         None, want_aux)
        return self.action_distribution(feats), rnn_states, feats

    def update_loss(self, obs, h0, prev_actions, ep_masks, tour_masks, corrected_actions, weights):
        """IterativeDaggerTrainer._update_agent's loss (iterative_dagger_trainer.py:33-94) -> loss, action loss, aux, logits,
        states"""
        T, N = corrected_actions.size()
        logits, states, _ = self.build_logits(obs, h0, prev_actions, ep_masks, tour_masks, want_aux=True)
        logits = logits.view(T, N, -1)
        ce = F.cross_entropy(logits.permute(0, 2, 1), corrected_actions, reduction="none")
        action_loss = ((weights * ce).sum(0) / weights.sum(0)).mean()
        aux = 0.0
        for loss, alpha in self.net.aux:
            aux = aux + alpha * torch.masked_select(loss, (weights > 0).view(-1)).mean()
        return action_loss + aux, action_loss, aux, logits, states


def golden_inputs(g, dt=torch.float64):
    """observations and the other arguments of a tests/golden/latent_lstm_*.npz case (the features come from seeds)"""
    from gen_latent_update_features import features

    T, N = int(g["T"]), int(g["N"])
    rgb_np, dep_np = features(int(g["seed"]), T, N)
    obs = {"rgb_features": torch.from_numpy(rgb_np).to(dt), "depth_features": torch.from_numpy(dep_np).to(dt),
           "instruction": torch.from_numpy(g["instruction"]), "progress": torch.from_numpy(g["progress"]).to(dt)}
    return dict(obs=obs, h0=torch.from_numpy(g["h0"]).to(dt), prev=torch.from_numpy(g["prev"]),
                ep=torch.from_numpy(g["ep"]), tour=torch.from_numpy(g["tour"]), targets=torch.from_numpy(g["targets"]),
                weights=torch.from_numpy(g["weights"]).to(dt), T=T, N=N)
