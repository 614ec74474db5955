"""CPU: `MODEL.STATE_ENCODER.rnn_type: LSTM` on the host side - the encoder factory, the module tree / state_dict keys
of a MapCMAPolicy built with it, and Latent-CMA's refusal.  (The arithmetic is tests/test_gpu_lstm_state.py.)"""
import pytest
import torch

from lstm_state_ref import MapCMAPolicyLSTMRef, make_policy, policy_config


def test_factory_builds_the_lstm_encoder():
    from ivln_ce_amd.encoders import LSTMStateEncoder, RNNStateEncoder, build_rnn_state_encoder

    I, H = 20, 32
    enc = build_rnn_state_encoder(I, H, "LSTM")
    assert isinstance(enc, LSTMStateEncoder) and enc.num_recurrent_layers == 2
    assert {k: tuple(v.shape) for k, v in enc.state_dict().items()} == {
        "rnn.weight_ih_l0": (4 * H, I), "rnn.weight_hh_l0": (4 * H, H), "rnn.bias_ih_l0": (4 * H,), "rnn.bias_hh_l0": (4 * H,)}
    # the GRU encoder's initialisation: orthogonal weights (the tall (4H, K) matrices have orthonormal columns), zero biases
    for w in (enc.rnn.weight_ih_l0, enc.rnn.weight_hh_l0):
        w = w.detach().double()
        assert float((w.t() @ w - torch.eye(w.shape[1], dtype=torch.float64)).abs().max()) < 1e-5
    assert float(enc.rnn.bias_ih_l0.detach().abs().max()) == 0.0 and float(enc.rnn.bias_hh_l0.detach().abs().max()) == 0.0


def test_factory_matches_rnn_type_case_insensitively_and_names_the_key_otherwise():
    from ivln_ce_amd.encoders import LSTMStateEncoder, RNNStateEncoder, build_rnn_state_encoder

    assert isinstance(build_rnn_state_encoder(8, 8, "lstm"), LSTMStateEncoder)
    for name in ("gru", "GRU"):
        enc = build_rnn_state_encoder(8, 8, name)
        assert isinstance(enc, RNNStateEncoder) and enc.num_recurrent_layers == 1 and isinstance(enc.rnn, torch.nn.GRU)
    with pytest.raises(ValueError, match="STATE_ENCODER.rnn_type"):
        build_rnn_state_encoder(8, 8, "RNN")


def test_map_cma_policy_with_lstm_has_four_state_slots_and_the_oracle_keys():
    pol = make_policy("LSTM")
    assert pol.net.num_recurrent_layers == 4
    assert pol.net.state_encoder.num_recurrent_layers == 2 and pol.net.second_state_encoder.num_recurrent_layers == 2
    ref = MapCMAPolicyLSTMRef()
    a = {k: tuple(v.shape) for k, v in pol.state_dict().items()}
    b = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert a == b
    assert a["net.state_encoder.rnn.weight_hh_l0"] == (2048, 512) and a["net.second_state_encoder.rnn.weight_ih_l0"] == (2048, 512)
    ref.load_state_dict(pol.state_dict())  # a checkpoint of one loads into the other
    assert make_policy("GRU").net.num_recurrent_layers == 2


def test_latent_cma_refuses_lstm():
    import ivln_ce_amd  # noqa: F401
    from ivln_ce_amd import latent_policy  # noqa: F401
    from ivln_ce_amd.registry import baseline_registry
    from ivln_ce_amd.spaces import Box, Dict, Discrete

    import numpy as np

    space = Dict({"depth": Box(0.0, 1.0, (256, 256, 1), np.float32), "rgb": Box(0, 255, (224, 224, 3), np.uint8),
                  "instruction": Box(0, 2504, (200,), np.int64)})
    with pytest.raises(ValueError, match="rnn_type"):
        baseline_registry.get_policy("LatentCMAPolicy").from_config(policy_config("LSTM", policy_name="LatentCMAPolicy"), space,
                                                                    Discrete(4))
