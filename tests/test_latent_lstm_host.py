"""CPU: Latent-CMA with LSTM state encoders (`MODEL.STATE_ENCODER.rnn_type: LSTM`), host side.  The policy builds in every
memory mode with the reference's state layout and state-dict keys; the torch oracle the GPU tests compare against
(tests/latent_lstm_ref.py) reproduces the reference's own numbers (tests/golden/latent_lstm_{plain,tour}.npz,
gen_latent_lstm_golden.py) at 1e-6 in float64; and the golden holds the record that the reference itself has no LSTM form
of the tour-memory variant."""
import os
import re

import numpy as np
import pytest
import torch

from latent_lstm_ref import MODES, LatentCMAPolicyLSTMRef, golden_inputs, make_policy

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
H = 512


def _golden(mode):
    return np.load(os.path.join(HERE, "golden", f"latent_lstm_{mode}.npz"))


@pytest.mark.parametrize("mode", MODES)
def test_policy_builds_with_lstm_encoders_in_every_memory_mode(mode):
    from ivln_ce_amd.encoders import LSTMStateEncoder

    pol = make_policy("LSTM", mode, fill=False)
    net = pol.net
    variant = mode == "variant"
    assert isinstance(net.state_encoder, LSTMStateEncoder) and isinstance(net.second_state_encoder, LSTMStateEncoder)
    assert net.num_recurrent_layers == (5 if variant else 4)
    assert tuple(net.state_encoder.rnn.weight_ih_l0.shape) == (4 * H, 416 + (H if variant else 0))
    assert tuple(net.second_state_encoder.rnn.weight_ih_l0.shape) == (4 * H, H)
    assert hasattr(net, "out_layer") == variant
    # the state as its users slice it (latent_cma_policy.py:392-399,427-431,470-477)
    st = torch.arange(2 * net.num_recurrent_layers * 3, dtype=torch.float32).view(2, net.num_recurrent_layers, 3)
    s1, s2, mem = net._state_slots(st)
    assert torch.equal(s1, st[:, 0:2]) and torch.equal(s2, st[:, 2:4])
    assert (mem is None) if not variant else torch.equal(mem, st[:, 4])
    # the GRU configuration beside it keeps its 2 / 3 slots
    gru = make_policy("GRU", mode, fill=False).net
    assert gru.num_recurrent_layers == (3 if variant else 2)
    g1, g2, gmem = gru._state_slots(st[:, :gru.num_recurrent_layers])
    assert torch.equal(g1, st[:, 0]) and torch.equal(g2, st[:, 1]) and ((gmem is None) if not variant else torch.equal(gmem, st[:, 2]))


@pytest.mark.parametrize("mode", MODES)
def test_lstm_is_opt_in_and_the_refusal_names_the_switch(mode):
    """a config that only sets rnn_type keeps its ValueError (tests/test_lstm_state_host.py pins it); the message says how
    to turn the option on"""
    from instr_rnn_ref import policy_space
    from latent_lstm_ref import mode_opts

    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.registry import baseline_registry
    from ivln_ce_amd.spaces import Discrete

    base = ["MODEL.policy_name", "LatentCMAPolicy", "MODEL.INSTRUCTION_ENCODER.use_pretrained_embeddings", False,
            "MODEL.DEPTH_ENCODER.ddppo_checkpoint", "NONE", "MODEL.STATE_ENCODER.rnn_type", "LSTM", *mode_opts(mode)]
    cls = baseline_registry.get_policy("LatentCMAPolicy")
    assert get_config(opts=base).MODEL.STATE_ENCODER.latent_lstm is False
    with pytest.raises(ValueError, match=r"rnn_type.*MODEL\.STATE_ENCODER\.latent_lstm True"):
        cls.from_config(get_config(opts=base), policy_space("LatentCMAPolicy"), Discrete(4))
    pol = cls.from_config(get_config(opts=base + ["MODEL.STATE_ENCODER.latent_lstm", True]), policy_space("LatentCMAPolicy"),
                          Discrete(4))
    assert pol.net.num_recurrent_layers == (5 if mode == "variant" else 4)
    # the switch means nothing to a GRU configuration
    gru = cls.from_config(get_config(opts=base[:6] + mode_opts(mode) + ["MODEL.STATE_ENCODER.latent_lstm", True]),
                          policy_space("LatentCMAPolicy"), Discrete(4))
    assert gru.net.num_recurrent_layers == (3 if mode == "variant" else 2)


@pytest.mark.parametrize("mode", ["plain", "tour"])
def test_state_dict_keys_are_the_references(mode):
    pol = make_policy("LSTM", mode, use_pm=mode == "plain", fill=False)
    assert sorted(pol.state_dict().keys()) == [str(k) for k in _golden(mode)["state_dict_keys"]]


def test_variant_state_dict_loads_into_the_oracle_strictly():
    """(the reference cannot run this mode, but it builds it: same keys, plus out_layer)"""
    pol = make_policy("LSTM", "variant")
    ref = LatentCMAPolicyLSTMRef("variant").load_from(pol)
    assert "net.out_layer.0.weight" in ref.state_dict()
    g = _golden("tour")
    assert int(g["variant_num_recurrent_layers"]) == pol.net.num_recurrent_layers == 5
    assert tuple(g["variant_weight_ih_shape"]) == tuple(pol.net.state_encoder.rnn.weight_ih_l0.shape)


def test_the_reference_raises_for_lstm_with_the_tour_memory_variant():
    """What DESIGN.md states about the variant is a recorded run of the reference, not a reading of its code."""
    g = _golden("tour")
    assert bool(g["variant_raises"]) and str(g["variant_error_type"]) == "RuntimeError"
    text = str(g["variant_error"])
    assert "[2, 1, 512]" in text and "[2, 2, 512]" in text, text  # (N, 1, H) slot <- (N, 2, H) [h | c]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"latent_lstm_tour\.npz", design), "DESIGN.md names the evidence"


@pytest.mark.parametrize("mode", ["plain", "tour"])
def test_oracle_reproduces_the_reference_goldens(mode):
    g = _golden(mode)
    a = golden_inputs(g)
    ref = LatentCMAPolicyLSTMRef(mode, use_pm=mode == "plain").load_from(make_policy("LSTM", mode, use_pm=mode == "plain")).double()
    loss, action_loss, aux, logits, states = ref.update_loss(a["obs"], a["h0"], a["prev"], a["ep"], a["tour"], a["targets"],
                                                             a["weights"])
    loss.backward()
    # (the golden holds Categorical(logits=...).logits: normalised log-probabilities)
    worst = {"logits": float(np.abs(torch.log_softmax(logits.detach(), -1).numpy() - g["logits"]).max()),
             "states": float(np.abs(states.detach().numpy() - g["rnn_out"]).max()),
             "loss": abs(float(loss.detach()) - float(g["loss"])),
             "action_loss": abs(float(action_loss.detach()) - float(g["action_loss"])),
             "aux_loss": abs(float(aux) - float(g["aux_loss"]))}
    params = dict(ref.named_parameters())
    seen = 0
    for k in g.files:
        if k.startswith("gradnorm/"):
            want, p = float(g[k]), params[k[9:]]
            worst[k] = abs(float(p.grad.norm()) - want) / max(1.0, abs(want))
            seen += 1
        elif k.startswith("grad/"):
            worst[k] = float(np.abs(params[k[5:]].grad.numpy() - g[k]).max())
    for k, v in worst.items():
        print(f"{mode:6s} {k:70s} {v:.3e}")
    assert seen >= 38
    bad = {k: v for k, v in worst.items() if not v <= 1e-6}
    assert not bad, bad


def test_oracle_variant_pools_the_memory_with_h_and_gives_it_no_gradient():
    """the definition of this project for LSTM + variant, on a tiny hand case through the oracle's net"""
    g = _golden("tour")
    a = golden_inputs(g)
    T, N = a["T"], a["N"]
    ref = LatentCMAPolicyLSTMRef("variant").load_from(make_policy("LSTM", "variant")).double()
    gen = torch.Generator().manual_seed(5)
    h0 = torch.zeros(N, 5, H, dtype=torch.float64)
    h0[:, 4] = 0.3 * torch.randn(N, H, generator=gen, dtype=torch.float64)
    h0.requires_grad_(True)
    sl = slice(0, N)
    obs = {k: v[sl] for k, v in a["obs"].items()}
    ones = torch.ones(N, 1, dtype=torch.uint8)
    tour = torch.tensor([[0], [1]], dtype=torch.uint8)
    feats, out = ref.net(obs, h0, a["prev"][sl], ones, ones, tour)
    assert torch.equal(out[0, 4], torch.max(torch.zeros(H, dtype=torch.float64), out[0, 0]))  # tour start: memory cleared
    assert torch.equal(out[1, 4], torch.max(h0[1, 4], out[1, 0])) and not torch.equal(out[1, 4], out[1, 0])
    feats.sum().backward()
    assert bool((h0.grad[0, 4] == 0).all())  # a cleared slot takes no gradient ...
    assert bool((h0.grad[1, 4] != 0).any())  # ... a kept one does, as an INPUT of this step only
    # the unrolled sequence runs, and what leaves it in the slot is the pooled memory of its last step
    logits, states, _ = ref.build_logits(a["obs"], h0.detach(), a["prev"], a["ep"], a["tour"])
    assert logits.shape == (T * N, 4) and bool((states[:, 4] >= states[:, 0]).all())


def test_the_new_entry_point_is_declared_in_a_header_of_its_own_and_bound_with_its_arity():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ivln_tour_state.h")).read(), flags=re.S)
    decls = re.findall(r"\bint\s+(ivln_\w+)\s*\(([^)]*)\)\s*;", src)
    assert [d[0] for d in decls] == ["ivln_lstm_seq_tour_fwd_f32"]
    params = [p.strip() for p in decls[0][1].split(",")]
    assert len(params) == 32 and params[-1] == "void* stream"
    assert "ivln_lstm_seq_tour" not in open(os.path.join(ROOT, "include", "ivln_hip.h")).read()  # (that header is pinned)
    assert '"ivln_tour_state.h"' in open(os.path.join(ROOT, "ivln-ce_amd", "build.py")).read()
    ops_src = open(os.path.join(ROOT, "ivln-ce_amd", "ops.py")).read()
    m = re.search(r"L\.ivln_lstm_seq_tour_fwd_f32\.argtypes = \((.*?)\)\n", ops_src, flags=re.S)
    from ivln_ce_amd._lib import i32, i64, vp

    argtypes = eval(" ".join(m.group(1).split()), {"vp": vp, "i32": i32, "i64": i64})  # noqa: S307  (a list expression of the three ctypes names)
    want = [i64 if p.startswith("int64_t ") else i32 if p.startswith("int ") else vp for p in params]
    assert argtypes == want
