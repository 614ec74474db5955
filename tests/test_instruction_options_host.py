"""CPU: `MODEL.INSTRUCTION_ENCODER.rnn_type` GRU | LSTM and `bidirectional` True | False (instruction_encoder.py:27-32, 49)
- construction, widths, state-dict keys and strict loading for both policies - and the float64 GRU cell loop of
tests/instr_rnn_ref.py pinned to torch.nn.GRU (the GPU tests take d(loss)/d(W_hh h + b_hh) from it), and that file's
Latent-CMA torch oracle pinned to the reference's golden at the default combination."""
import pytest
import torch
import torch.nn as nn

from instr_rnn_ref import COMBOS, gru_cell_loop, make_case, make_policy, module_ref, options_config


def _torch_encoder_state(cell, bidirectional, cfg):
    rnn = getattr(nn, cell)(input_size=cfg.embedding_size, hidden_size=cfg.hidden_size, bidirectional=bidirectional)
    emb = nn.Embedding(cfg.vocab_size, cfg.embedding_size, padding_idx=0)
    sd = {"encoder_rnn." + k: v for k, v in rnn.state_dict().items()}
    sd.update({"embedding_layer." + k: v for k, v in emb.state_dict().items()})
    return sd


@pytest.mark.parametrize("cell,bidirectional", COMBOS)
def test_instruction_encoder_constructs_with_the_reference_keys(cell, bidirectional):
    from ivln_ce_amd.encoders import InstructionEncoder

    cfg = options_config(cell, bidirectional).MODEL.INSTRUCTION_ENCODER
    enc = InstructionEncoder(cfg)
    assert enc.output_size == (256 if bidirectional else 128)
    assert isinstance(enc.encoder_rnn, getattr(nn, cell)) and enc.encoder_rnn.bidirectional == bidirectional
    want = _torch_encoder_state(cell, bidirectional, cfg)
    got = enc.state_dict()
    assert list(got.keys()) == list(want.keys())
    assert {k: tuple(v.shape) for k, v in got.items()} == {k: tuple(v.shape) for k, v in want.items()}
    assert any(k.endswith("_reverse") for k in got) == bidirectional
    assert got["encoder_rnn.weight_hh_l0"].shape[0] == (3 if cell == "GRU" else 4) * 128
    # a state dict saved from the plain torch modules loads strictly, and its values arrive
    with torch.no_grad():
        want = {k: torch.full_like(v, 0.25) for k, v in want.items()}
    enc.load_state_dict(want, strict=True)
    assert all(bool((v == 0.25).all()) for v in enc.state_dict().values())


@pytest.mark.parametrize("policy_name", ["MapCMAPolicy", "LatentCMAPolicy"])
@pytest.mark.parametrize("cell,bidirectional", COMBOS)
def test_both_policies_construct_and_follow_the_text_width(cell, bidirectional, policy_name):
    pol = make_policy(cell, bidirectional, policy_name, fill=False)
    net = pol.net
    Ct = 256 if bidirectional else 128
    assert net.instruction_encoder.output_size == Ct
    assert net.text_k.in_channels == Ct and net.text_q.in_features == Ct
    assert net.model_config.INSTRUCTION_ENCODER.final_state_only is False
    default = make_policy("LSTM", True, policy_name, fill=False).net
    assert net.second_state_compress[0].in_features == default.second_state_compress[0].in_features - 256 + Ct
    cfg = net.model_config.INSTRUCTION_ENCODER
    want = {"net.instruction_encoder." + k: tuple(v.shape) for k, v in _torch_encoder_state(cell, bidirectional, cfg).items()}
    got = {k: tuple(v.shape) for k, v in pol.state_dict().items() if k.startswith("net.instruction_encoder.")}
    assert got == want
    pol.load_state_dict({k: v.clone() for k, v in pol.state_dict().items()}, strict=True)


def test_another_rnn_type_is_refused_by_name():
    from ivln_ce_amd.encoders import InstructionEncoder

    with pytest.raises(ValueError, match=r"MODEL\.INSTRUCTION_ENCODER\.rnn_type"):
        InstructionEncoder(options_config("RNN", True).MODEL.INSTRUCTION_ENCODER)
    with pytest.raises(ValueError, match=r"MODEL\.INSTRUCTION_ENCODER\.rnn_type"):
        make_policy("RNN", False, fill=False)


@pytest.mark.parametrize("ndir", [1, 2])
def test_gru_cell_loop_is_nn_gru(ndir):
    """the hand-written float64 cell loop against packed torch.nn.GRU: outputs, h_{t-1} and the input-side gradient at 1e-12;
    and dgh's own definition: equal to dgi in the r and z rows, dgi * r in the n rows (r recovered from the two)"""
    B, L, H, lens = 3, 5, 128, [5, 2, 1]
    c = make_case("GRU", ndir, B, L)
    m = module_ref("GRU", ndir, c["gx"], c["whh"], c["bhh"], lens, c["dout"], B, L, H, torch.float64)
    lp = gru_cell_loop(ndir, c["gx"], c["whh"], c["bhh"], lens, c["dout"], B, L, H, torch.float64)
    assert float((m["out"] - lp["out"]).abs().max()) < 1e-12
    for d in range(ndir):
        assert float((m["dgi"][d] - lp["dgi"][d]).abs().max()) < 1e-12
        assert float((m["hp"][d] - lp["hp"][d]).abs().max()) < 1e-12
        assert torch.equal(lp["dgh"][d][:, :2 * H], lp["dgi"][d][:, :2 * H])
        assert float(lp["dgh"][d][:, 2 * H:].abs().max()) > 0
        assert bool((lp["dgh"][d][:, 2 * H:].abs() <= lp["dgi"][d][:, 2 * H:].abs()).all())  # |r| <= 1
        pad = torch.tensor([[t >= n for t in range(L)] for n in lens]).view(B * L)
        assert float(lp["dgh"][d][pad].abs().max()) == 0.0 and float(lp["dgi"][d][pad].abs().max()) == 0.0


def test_latent_oracle_of_the_gpu_tests_is_the_reference_at_the_default_combination():
    """instr_rnn_ref.LatentCMAPolicyOptRef (the torch oracle the Latent-CMA GPU tests compare with) against the golden the
    reference's own LatentCMAPolicy produced for the default (LSTM, bidirectional) encoder - tests/golden/
    latent_update_plain.npz, episodic memory, T = 4, N = 3: logits and outgoing states at 1e-5, the action loss at 2e-5
    (the bounds tests/test_gpu_latent.py holds against the same file).  So the oracle does not owe its agreement with the
    HIP net to being written beside it."""
    import os

    import numpy as np
    import torch.nn.functional as F
    from gen_latent_update_features import features
    from instr_rnn_ref import LatentCMAPolicyOptRef

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "latent_update_plain.npz"))
    T, N = int(g["T"]), int(g["N"])
    rgb, dep = features(int(g["seed"]), T, N)
    pol = make_policy("LSTM", True, "LatentCMAPolicy", use_pm=True)  # (the golden's deterministic fill)
    ref = LatentCMAPolicyOptRef("LSTM", True).load_from(pol).train()
    obs = {"rgb_features": torch.from_numpy(rgb), "depth_features": torch.from_numpy(dep),
           "instruction": torch.from_numpy(g["instruction"])}
    with torch.no_grad():
        logits, states, _ = ref.logits(obs, torch.from_numpy(g["h0"]), torch.from_numpy(g["prev"]), torch.from_numpy(g["ep"]))
    logp = torch.log_softmax(logits, -1).view(T, N, -1)
    w = torch.from_numpy(g["weights"])
    ce = F.cross_entropy(logp.permute(0, 2, 1), torch.from_numpy(g["targets"]), reduction="none")
    action_loss = float(((w * ce).sum(0) / w.sum(0)).mean())
    e_l = float((logp - torch.from_numpy(g["logits"])).abs().max())
    e_s = float((states - torch.from_numpy(g["rnn_out"])).abs().max())
    print(f"latent oracle vs reference golden: logits {e_l:.3e} states {e_s:.3e} action loss {action_loss:.7f} ref {float(g['action_loss']):.7f}")
    assert e_l < 1e-5 and e_s < 1e-5 and abs(action_loss - float(g["action_loss"])) < 2e-5


def test_the_instruction_encoder_has_one_entry_point_per_kernel():
    """include/ivln_hip.h declares, of the instruction encoder (front end, recurrences, BPTT), exactly the five entry points
    below and ivln_embed_lengths, each once; no other name of those families - an entry point that forwards to one of them
    with arguments filled in - is declared or mentioned there, or anywhere in ops.py"""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    keep = ["ivln_embed_gates_dirs_f32", "ivln_embed_lengths", "ivln_gru_dirs_bwd_f32", "ivln_gru_dirs_fwd_f32",
            "ivln_lstm_dirs_bwd_f32", "ivln_lstm_dirs_fwd_f32"]
    family = r"\bivln_(?:embed_gates|embed_lengths|lstm_bidir|lstm_dirs|gru_dirs)\w*"
    header = open(os.path.join(root, "include", "ivln_hip.h")).read()
    declared = re.findall("(" + family + r")\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert sorted(declared) == keep, declared
    assert sorted(set(re.findall(family, header))) == keep
    ops_src = open(os.path.join(root, "ivln-ce_amd", "ops.py")).read()
    assert sorted(set(re.findall(family, ops_src))) == keep
