"""TEST INFRASTRUCTURE ONLY - torch references of the instruction encoder over pre-computed text features
(`MODEL.INSTRUCTION_ENCODER.sensor_uuid = "rxr_instruction"`, instruction_encoder.py:34-45, 70-78), shared by
tests/test_text_feat_host.py and the GPU tests of the feature path.

  row_counts        lengths as the reference forms them: the NUMBER of rows with a non-zero element
  TextFeatEncoderRef the encoder in any dtype: no embedding layer, nn.GRU / nn.LSTM on pack_padded_sequence over the first
                    `lengths[b]` rows.  tests/test_text_feat_host.py holds it to tests/golden/rxr_instruction.npz (the
                    reference's own module), so the GPU tests may use its float64 form as their reference.
  rxr_config / make_rxr_policy / mapcma_rxr_oracle / MapCMALSTMRxrRef / LatentRxrRef: the policies built from an RxR
                    config and the torch oracles of tests/instr_rnn_ref.py and tests/lstm_state_ref.py (LSTM state
                    encoders) with only the instruction encoder swapped.
"""
import numpy as np
import torch
import torch.nn as nn

from instr_rnn_ref import InstructionEncoderOptRef, LatentCMAPolicyOptRef, mapcma_oracle, options_config
from lstm_state_ref import MapCMAPolicyLSTMRef

KEY = "rxr_instruction"


def row_counts(feat):
    """(B, L, E) -> (B,) int64: instruction_encoder.py:77-78"""
    return ((feat != 0.0).long().sum(dim=2) != 0).long().sum(dim=1)


class TextFeatEncoderRef(InstructionEncoderOptRef):
    """InstructionEncoderOptRef without its embedding layer, reading the features"""

    def __init__(self, cell, bidirectional, emb, hidden=128):
        super().__init__(cell, bidirectional, vocab=1, emb=emb, hidden=hidden)
        del self.embedding_layer

    def forward(self, obs, total_length=None):
        x = obs[KEY].to(self.encoder_rnn.weight_ih_l0.dtype)
        lengths = row_counts(x).cpu()
        # (an all-zero sequence, which pack_padded_sequence refuses: run with length 1 and blanked - the kernels leave zeros)
        packed = nn.utils.rnn.pack_padded_sequence(x, lengths.clamp(min=1), batch_first=True, enforce_sorted=False)
        out, _ = self.encoder_rnn(packed)
        out = nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=total_length)[0]
        out = out * (lengths > 0).to(out.dtype).view(-1, 1, 1)
        return out.permute(0, 2, 1)


def encoder_ref(enc, dt):
    """the torch restatement of an `encoders.InstructionEncoder` built for features, in dtype `dt`, with its weights"""
    ref = TextFeatEncoderRef("GRU" if enc.is_gru else "LSTM", enc.ndir == 2, enc.encoder_rnn.input_size,
                             enc.encoder_rnn.hidden_size)
    ref.load_state_dict({k: v.detach().cpu() for k, v in enc.state_dict().items()})  # strict: no embedding_layer key
    return ref.to(dt)


def patterned_features(rows_per_seq, L, E, seed):
    """(B, L, E) f32 with standard-normal rows at the listed positions of each sequence and zero rows elsewhere"""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(len(rows_per_seq), L, E)
    for b, rows in enumerate(rows_per_seq):
        rows = list(rows)
        if rows:
            x[b, rows] = torch.randn(len(rows), E, generator=g)
    return x


# ------------------------------------------------------------------------------------------------------------------
# policies
# ------------------------------------------------------------------------------------------------------------------
def rxr_config(cell, bidirectional, policy_name="MapCMAPolicy", use_pm=False, L=512, E=768, state_rnn="GRU"):
    return options_config(cell, bidirectional, policy_name, use_pm, extra=(
        "MODEL.STATE_ENCODER.rnn_type", state_rnn,
        "MODEL.INSTRUCTION_ENCODER.sensor_uuid", KEY, "MODEL.INSTRUCTION_ENCODER.embedding_size", E,
        "TASK_CONFIG.TASK.INSTRUCTION_SENSOR_UUID", KEY, "TASK_CONFIG.TASK.RXR_INSTRUCTION_SENSOR.max_text_len", L))


def rxr_space(policy_name="MapCMAPolicy", L=512, E=768):
    from ivln_ce_amd.spaces import Box, Dict

    sp = {"depth": Box(0.0, 1.0, (256, 256, 1), np.float32), KEY: Box(-np.inf, np.inf, (L, E), np.float32)}
    if policy_name == "LatentCMAPolicy":
        sp["rgb"] = Box(0, 255, (224, 224, 3), np.uint8)
    else:
        sp["occupancy_map"] = Box(0, 255, (64, 64), np.uint8)
        sp["semantic_map"] = Box(0, 255, (64, 64), np.uint8)
    return Dict(sp)


def make_rxr_policy(cell, bidirectional, policy_name="MapCMAPolicy", use_pm=False, L=512, E=768, state_rnn="GRU"):
    from det_init import det_fill

    import ivln_ce_amd  # noqa: F401
    from ivln_ce_amd import latent_policy, policy  # noqa: F401
    from ivln_ce_amd.registry import baseline_registry
    from ivln_ce_amd.spaces import Discrete

    pol = baseline_registry.get_policy(policy_name).from_config(
        rxr_config(cell, bidirectional, policy_name, use_pm, L, E, state_rnn), rxr_space(policy_name, L, E), Discrete(4))
    det_fill(pol, seed=0, conv_gain=1.0 if policy_name == "LatentCMAPolicy" else 2.0 ** 0.5)
    return pol


def mapcma_rxr_oracle(cell, bidirectional, E, use_pm=False):
    ref = mapcma_oracle(cell, bidirectional, use_pm=use_pm)
    ref.net.instruction_encoder = TextFeatEncoderRef(cell, bidirectional, E)
    return ref


class MapCMALSTMRxrRef(MapCMAPolicyLSTMRef):
    """tests/lstm_state_ref.py's oracle of `STATE_ENCODER.rnn_type: LSTM` with the instruction encoder swapped for the
    feature encoder (and the three layers whose width follows it, as instr_rnn_ref.mapcma_oracle does)"""

    def __init__(self, cell, bidirectional, E, **kw):
        super().__init__(**kw)
        net = self.net
        enc = TextFeatEncoderRef(cell, bidirectional, E)
        Ct, hidden = enc.output_size, net._hidden_size
        net.instruction_encoder = enc
        net.text_k = nn.Conv1d(Ct, hidden // 2, 1)
        net.text_q = nn.Linear(Ct, hidden // 2)
        old = net.second_state_compress[0]
        net.second_state_compress = nn.Sequential(nn.Linear(old.in_features - 256 + Ct, hidden), nn.ReLU(True))


class LatentRxrRef(LatentCMAPolicyOptRef):
    def __init__(self, cell, bidirectional, E, num_actions=4):
        super().__init__(cell, bidirectional, num_actions)
        self.net.instruction_encoder = TextFeatEncoderRef(cell, bidirectional, E)
