"""CPU: the recurrent state encoders live in one kernel file (csrc/state_rnn.hip, cell arithmetic in csrc/rnn_cell.h), the
files they came from are gone, and the consolidation did not move the C ABI: the code of include/ivln_hip.h - comments
stripped, whitespace collapsed - still hashes to the value it had before (comments may name other source files)."""
import hashlib
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ivln-ce_amd")

# sha256 of header_code() of the commit before the consolidation
HEADER_CODE_SHA256 = "c0a656a8e39d3fbe53844768aa1bee1bb890c307d4b4d45156a5c3a3d7da8b04"


def header_code():
    src = open(os.path.join(ROOT, "include", "ivln_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    return " ".join(src.split())


def test_state_encoders_are_one_kernel_file_and_the_abi_did_not_move():
    csrc = os.path.join(PKG, "csrc")
    for gone in ("lstm_state.hip", "gru_seq.hip", "gru_seq.h"):
        assert not os.path.exists(os.path.join(csrc, gone)), gone
    for there in ("state_rnn.hip", "rnn_cell.h"):
        assert os.path.exists(os.path.join(csrc, there)), there
    spec = importlib.util.spec_from_file_location("ivln_build_sources", os.path.join(PKG, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "state_rnn.hip" in build.SOURCES
    assert not {"lstm_state.hip", "gru_seq.hip"} & set(build.SOURCES)
    assert all(os.path.exists(os.path.join(csrc, f)) for f in build.SOURCES)
    code = header_code()
    assert "ivln_gru_step_f32" in code and "ivln_lstm_seq_bwd_f32" in code and "/*" not in code
    assert hashlib.sha256(code.encode()).hexdigest() == HEADER_CODE_SHA256
    # the pin itself: one changed argument type is noticed
    assert hashlib.sha256(code.replace("int64_t ldgi", "int ldgi", 1).encode()).hexdigest() != HEADER_CODE_SHA256
