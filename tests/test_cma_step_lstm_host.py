"""CPU: the host side of the fused recurrent head for LSTM state encoders (ivln_cma_step_lstm_fwd, csrc/cma_step.hip) -
the two C entry points and where the header declares them, their Python bindings, the form a policy reports, and the
descriptor both forms share.  (The arithmetic is tests/test_gpu_cma_step_lstm.py.)"""
import ctypes as C
import os
import re

import pytest

from lstm_state_ref import make_policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ivln_cma_step_lstm_ws_floats", "ivln_cma_step_lstm_fwd")


def _header():
    return open(os.path.join(ROOT, "include", "ivln_hip.h")).read()


def test_header_declares_both_entry_points_above_the_backward_section():
    src = _header()
    banner = src.index("Backward / loss / optimizer kernels")
    code = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), src, flags=re.S)  # (comments blanked, offsets kept)
    gru = code.index("ivln_cma_step_fwd(")
    for name in NEW:
        at = [m.start() for m in re.finditer(r"\b%s\s*\(" % name, code)]
        assert len(at) == 1, f"{name}: declared {len(at)} times"
        assert gru < at[0] < banner, f"{name} is not declared between ivln_cma_step_fwd and the backward banner"
    assert re.search(r"int64_t\s+ivln_cma_step_lstm_ws_floats\s*\(\s*int rows,\s*int L,\s*int P,\s*int H\s*\)\s*;", code)
    assert re.search(r"int\s+ivln_cma_step_lstm_fwd\s*\(\s*const ivln_cma_step_desc\*\s*d,\s*int mode,\s*void\*\s*stream\s*\)\s*;", code)


def test_library_exports_both_entry_points():
    import __graft_entry__ as ge

    L = C.CDLL(ge.build())
    for name in NEW + ("ivln_cma_step_fwd", "ivln_cma_step_ws_floats"):
        assert hasattr(L, name), name
    # host-only arithmetic: the LSTM scratch is the GRU form's plus the rows x 4H hidden half, in 128-byte lines
    for f in (L.ivln_cma_step_ws_floats, L.ivln_cma_step_lstm_ws_floats):
        f.restype, f.argtypes = C.c_int64, [C.c_int] * 4
    for rows, Ln, P, H in [(1, 1, 1, 64), (4, 80, 16, 512), (20, 12, 16, 64)]:
        extra = L.ivln_cma_step_lstm_ws_floats(rows, Ln, P, H) - L.ivln_cma_step_ws_floats(rows, Ln, P, H)
        assert extra >= rows * 4 * H and extra % 32 == 0, (rows, Ln, P, H, extra)


def test_bindings_exist_and_are_not_the_gru_ones():
    from ivln_ce_amd import ops

    assert callable(ops.cma_step_lstm) and callable(ops.cma_step_lstm_ws)
    assert ops.cma_step_lstm is not ops.cma_step and ops.cma_step_lstm_ws is not ops.cma_step_ws
    src = open(os.path.join(ROOT, "ivln-ce_amd", "ops.py")).read()
    gemm_banner = src.index("# ---- GEMM-shaped gradients")
    for name in ("def cma_step_lstm_ws(", "def cma_step_lstm("):
        assert 0 <= src.index(name) < gemm_banner, name
    body = src[src.index("def cma_step_lstm("):]
    body = body[:body.index("\n\n\n")]
    assert "ivln_cma_step_lstm_fwd" in body and "cma_step(" not in body  # (does not route through ops.cma_step)


@pytest.mark.parametrize("rnn_type,form", [("LSTM", "lstm"), ("GRU", "gru")])
def test_policy_names_the_fused_form_its_encoders_allow(rnn_type, form):
    net = make_policy(rnn_type).net
    assert net.fused_head_form == form
    assert net._gru_encoders == (form == "gru")


def test_mixed_encoders_allow_no_fused_form():
    from ivln_ce_amd.encoders import build_rnn_state_encoder

    net = make_policy("GRU").net
    g2 = net.second_state_encoder.rnn
    net.second_state_encoder = build_rnn_state_encoder(g2.input_size, g2.hidden_size, "LSTM")
    assert net.fused_head_form is None and not net._gru_encoders


def test_descriptor_mirror_is_unchanged():
    from ivln_ce_amd import ops

    # ivln_cma_step_desc: 10 ints, then pointers / int64 strides / one float on 8-byte slots - 264 bytes, 38 fields
    assert C.sizeof(ops.CmaStepDesc) == 264
    names = [f[0] for f in ops.CmaStepDesc._fields_]
    assert len(names) == 38 and names[:4] == ["rows", "L", "P", "H"] and names[-5:] == ["x2", "h_out", "ld_ho", "feats", "ws"]
    struct = re.search(r"typedef struct ivln_cma_step_desc \{(.*?)\} ivln_cma_step_desc;", _header(), flags=re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    # the header declares the mirror's fields, in the mirror's order (whatever form each declaration takes)
    at = [re.search(r"\b%s\b" % n, struct) for n in names]
    assert all(at), [n for n, m in zip(names, at) if not m]
    assert [m.start() for m in at] == sorted(m.start() for m in at)
