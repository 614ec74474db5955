"""CPU: the structure of MapCMANet's rollout step (policy.py) - the geometry of its two row buffers, the per-form choice
of the fused head's scratch and entry point, and the signatures of the whole step and of the three stages that
graphed.GraphedRollout captures as separate graphs.  (What the step computes is tests/test_gpu_policy.py.)"""
import inspect

import pytest

from lstm_state_ref import make_policy


@pytest.mark.parametrize("rnn_type", ["GRU", "LSTM"])
def test_geometry_is_the_prefix_sums_of_the_column_blocks(rnn_type):
    net = make_policy(rnn_type).net
    geo = net.step_geometry
    H, Ct = net._hidden_size, net.instruction_encoder.output_size
    d_out, m_out = net.depth_linear[1].out_features, net.map_linear[1].out_features
    E = net.prev_action_embedding.embedding_dim
    assert (geo.d_out, geo.m_out, geo.E) == (d_out, m_out, E)
    assert geo.x2w == H + Ct + d_out + m_out + E
    assert (geo.o_txt, geo.o_dep, geo.o_map, geo.o_prev) == (H, H + Ct, H + Ct + d_out, H + Ct + d_out + m_out)
    assert geo.x2w == net.second_state_compress[0].in_features  # (x2 is what the compress layer reads)
    state_in, x2 = geo.buffers(3, "cpu")
    assert tuple(state_in.shape) == (3, d_out + m_out + E) == (3, net.state_encoder.rnn.input_size)
    assert tuple(x2.shape) == (3, geo.x2w)
    assert state_in.is_contiguous() and x2.is_contiguous()


def test_fused_head_ops_per_form():
    from ivln_ce_amd import ops
    from ivln_ce_amd.policy import MapCMANet

    assert MapCMANet._fused_head_ops("gru") == (ops.cma_step_ws, ops.cma_step)
    assert MapCMANet._fused_head_ops("lstm") == (ops.cma_step_lstm_ws, ops.cma_step_lstm)
    assert MapCMANet._fused_head_ops(None) is None


def test_step_and_stage_signatures():
    from ivln_ce_amd.policy import MapCMANet

    step = ["self", "observations", "rnn_states", "prev_actions", "action_masks"]
    sig = inspect.signature(MapCMANet.forward_hip)
    names = list(sig.parameters)
    assert names[:6] == step + ["save"] and sig.parameters["save"].default is None
    assert not any("stage" in n for n in names)
    # what a captured step adds is keyword-only: positional callers (train.py) see the five-argument forward
    extra = {n: p for n, p in sig.parameters.items() if n not in names[:6]}
    assert set(extra) == {"side_streams", "rnn_out"}
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None for p in extra.values())
    want = {
        "stage_depth": step + ["step"],
        "stage_pre": step + ["step", "txt3"],
        "stage_post": step + ["step", "dep2", "pre", "rnn_out"],
    }
    for name, params in want.items():
        assert list(inspect.signature(getattr(MapCMANet, name)).parameters) == params, name
    assert inspect.signature(MapCMANet.stage_pre).parameters["txt3"].default is None
    assert inspect.signature(MapCMANet.stage_post).parameters["rnn_out"].default is None


def test_split_capture_of_a_net_without_stages_is_refused_at_once():
    """`streams="split"` captures MapCMANet's stages; any other net is an error before anything runs, not a missing
    attribute in the middle of the warm-up."""
    import types

    import torch

    from ivln_ce_amd.graphed import GraphedRollout

    with pytest.raises(TypeError, match="split"):
        GraphedRollout(types.SimpleNamespace(net=torch.nn.Linear(1, 1)), [], {}, streams="split")
