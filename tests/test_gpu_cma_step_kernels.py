"""GPU: the fused recurrent head of the rollout step (csrc/cma_step.hip) alone, through the C ABI, in both forms -
ivln_cma_step_fwd (GRU state encoders, the default configuration and the benchmark) and ivln_cma_step_lstm_fwd - against the
head restated in float64 torch from UNFOLDED weights (tests/cma_step_ref.py).

  a. each form alone at the edges of its phase kernels: the lanes-per-row switches (rows 4 | 5, 8 | 9), one / two / three
     passes of the 16-lane form (rows 16, 17, 33), K tails of lpr_dot, odd L and P, phase 3's second softmax slot and its
     boundaries (L = 255 ... 512), a row of length 0, the Mq_img / TQb_img <= 0 defaults; sentinels behind every buffer
  b. the GRU form's envelope: every refusal happens before any launch

Bound of (a), per tensor:  max|fused - ref64| <= 2 * max|unfused - ref64| + 4 * 2^-24 * max|ref64|  - the bar of
tests/test_gpu_cma_step_lstm.py, no new constant.  "Unfused" is the project's op chain on the same device inputs
(ops.gru_step / ops.lstm_step, ops.linear, ops.attn, ops.attn_small2, ops.linear(relu=True), the step again), itself pinned
to float64 by tests/test_gpu_state_rnn_step.py, tests/test_gpu_lstm_state.py and tests/test_gpu_forward_kernels.py.  Every
comparison is written to cma_step_kernels.log in the suite's log directory before anything is asserted.
tests/test_cma_step_coverage.py (CPU) holds the reference's folded form to its unfolded one and shows that the cases below
reach the edges they are named for."""
import ctypes as C

import pytest
import torch

from cma_step_ref import EPS, FULL, SLOTS, SMALL, case_seed, make_case
from kernel_bar import _log, _same_bytes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOG = "cma_step_kernels.log"
E_INVALID, E_UNSUPPORTED = -1, -5
PAD = 8    # floats between two rows of a state view: ld = slots * H + 8
SENT = 64  # floats of sentinel behind the scratch

# per form: the op that runs it, the C entry point behind that op, the C function that sizes its scratch
FORMS = {"gru": ("cma_step", "ivln_cma_step_fwd", "ivln_cma_step_ws_floats"),
         "lstm": ("cma_step_lstm", "ivln_cma_step_lstm_fwd", "ivln_cma_step_lstm_ws_floats")}

# (rows, L, P, FULL widths?)
GRU_ONLY_CASES = [(1, 1, 1, False), (3, 17, 16, False), (4, 64, 4, False), (5, 33, 16, False), (8, 16, 9, False),
                  (9, 40, 16, False), (20, 12, 16, False), (8, 80, 16, True)]   # (the LSTM file's KERNEL_CASES)
PASS_CASES = [(16, 15, 16, False), (17, 31, 2, False), (33, 12, 16, False)]      # 1 / 2 / 3 passes of the 16-lane form
SLOT_CASES = [(2, 255, 16, False), (2, 256, 5, False), (2, 257, 16, False), (3, 511, 1, False), (2, 512, 16, False)]
WIDE_CASES = [(4, 200, 16, True)]
BOTH_CASES = PASS_CASES + SLOT_CASES + WIDE_CASES
KERNEL_CASES = [("gru",) + c for c in GRU_ONLY_CASES + BOTH_CASES] + [("lstm",) + c for c in BOTH_CASES]
EMPTY_ROW_CASE = (3, 17, 16, False, (17, 0, 1))   # (rows, L, P, wide, lengths)
SPLIT_FOLD_CASE = (5, 33, 16, False)              # Mq and TQb as two tensors, Mq_img = TQb_img = 0

_cases = {}


def _case(cell, rows, L, P, wide, mask0, lengths=None):
    key = (cell, rows, L, P, wide, mask0, lengths)
    if key not in _cases:
        _cases[key] = make_case(cell, rows, L, P, FULL if wide else SMALL, mask0, case_seed(rows, L, P, mask0), lengths)
    return _cases[key]


def _state_view(rows, slots, H, fill=None):
    """(rows, slots, H) view with row stride slots * H + PAD inside a wider buffer of sevens -> (view, buffer)"""
    wide = torch.full((rows, slots * H + PAD), 7.0, device=DEV)
    v = wide.as_strided((rows, slots, H), (slots * H + PAD, H, 1), 4)
    if fill is not None:
        v.copy_(fill.to(DEV))
    return v, wide


def _pads_intact(wide, slots, H):
    return float((wide[:, :4] - 7.0).abs().max()) == 0.0 and float((wide[:, 4 + slots * H:] - 7.0).abs().max()) == 0.0


class _Dev:
    """the case's operands on the device, shared by the fused and the unfused run"""

    def __init__(self, c):
        self.c = c
        self.slots = len(SLOTS[c["cell"]])
        for k in ("state_in", "mask", "lengths", "txt", "dkv", "mkv", "prev", "fold", "text_k", "w_q", "b_q", "w_tq", "b_tq",
                  "w_c", "b_c", "w_ih1", "w_hh1", "b_ih1", "b_hh1", "w_ih2", "w_hh2", "b_ih2", "b_hh2"):
            setattr(self, k, c[k].to(DEV).contiguous())
        self.h_in, self.h_in_wide = _state_view(c["rows"], self.slots, c["H"], c["state"])
        assert self.h_in.stride(0) == self.slots * c["H"] + PAD

    def x2(self):
        c = self.c
        x2 = torch.full((c["rows"], c["x2w"]), float("nan"), device=DEV)
        x2[:, c["x2w"] - c["E"]:] = self.prev  # the previous-action slice is the caller's
        return x2


def _desc(ops, dv, x2, h_out, feats, ws, split_fold=None):
    """the descriptor filled by hand; split_fold = (Mq, TQb): two contiguous tensors, the image strides left at 0"""
    c = dv.c
    d = ops.CmaStepDesc()
    d.rows, d.L, d.P, d.H, d.Hq, d.Ct, d.d_out, d.m_out, d.E, d.x2w = (c[k] for k in ("rows", "L", "P", "H", "Hq", "Ct", "d_out",
                                                                                     "m_out", "E", "x2w"))
    d.state_in, d.h_in, d.ld_h, d.mask = dv.state_in.data_ptr(), dv.h_in.data_ptr(), dv.h_in.stride(0), dv.mask.data_ptr()
    d.w_ih1, d.w_hh1, d.b_ih1, d.b_hh1 = (t.data_ptr() for t in (dv.w_ih1, dv.w_hh1, dv.b_ih1, dv.b_hh1))
    if split_fold is None:
        d.Mq, d.Mq_img = dv.fold.data_ptr(), dv.fold.stride(0)
        d.TQb, d.TQb_img = dv.fold[:, c["H"] + 1:].data_ptr(), dv.fold.stride(0)
    else:
        d.Mq, d.Mq_img, d.TQb, d.TQb_img = split_fold[0].data_ptr(), 0, split_fold[1].data_ptr(), 0
    d.lengths, d.txt, d.dkv, d.mkv, d.scale = dv.lengths.data_ptr(), dv.txt.data_ptr(), dv.dkv.data_ptr(), dv.mkv.data_ptr(), c["scale"]
    d.w_c, d.b_c = dv.w_c.data_ptr(), dv.b_c.data_ptr()
    d.w_ih2, d.w_hh2, d.b_ih2, d.b_hh2 = (t.data_ptr() for t in (dv.w_ih2, dv.w_hh2, dv.b_ih2, dv.b_hh2))
    d.x2, d.h_out, d.ld_ho, d.feats, d.ws = x2.data_ptr(), h_out.data_ptr(), h_out.stride(0), feats.data_ptr(), ws.data_ptr()
    return d


def _ws_floats(ops, c):
    f = getattr(ops._L(), FORMS[c["cell"]][2])
    f.restype, f.argtypes = C.c_int64, [C.c_int] * 4
    return int(f(c["rows"], c["L"], c["P"], c["H"]))


def _step_op(ops, cell):
    """the op that runs the form: ops.cma_step / ops.cma_step_lstm"""
    return getattr(ops, FORMS[cell][0])


def _outputs(cell, c, x2, feats, h_out):
    out = dict(x2=x2[:, :c["x2w"] - c["E"]], feats=feats)
    out.update((name, h_out[:, k]) for k, name in enumerate(SLOTS[cell]))
    return out


def _run_fused(ops, dv, split_fold=False):
    c = dv.c
    cell, rows, H = c["cell"], c["rows"], c["H"]
    n = _ws_floats(ops, c)
    ws = torch.full((n + SENT,), 3.0, device=DEV)   # exactly what the library asks for, then sentinels
    x2, feats = dv.x2(), torch.full((rows, H), float("nan"), device=DEV)
    h_out, h_out_wide = _state_view(rows, dv.slots, H)
    fold2 = None
    if split_fold:
        fold2 = (dv.fold[:, :H + 1].contiguous(), dv.fold[:, H + 1:].contiguous())
        assert fold2[0].stride(0) == (H + 1) * c["L"] and fold2[1].stride(0) == c["Hq"] * c["L"]
    _step_op(ops, cell)(_desc(ops, dv, x2, h_out, feats, ws, fold2))
    torch.cuda.synchronize()
    assert float((ws[n:] - 3.0).abs().max()) == 0.0, f"the kernel wrote behind {FORMS[cell][2]}() floats"
    assert _pads_intact(h_out_wide, dv.slots, H) and _pads_intact(dv.h_in_wide, dv.slots, H)
    assert _same_bytes(dv.h_in, c["state"].to(DEV)), "the incoming state was written"
    assert _same_bytes(x2[:, c["x2w"] - c["E"]:], dv.prev), "the caller's previous-action slice of x2 was written"
    return _outputs(cell, c, x2, feats, h_out)


def _run_unfused(ops, dv):
    """MapCMANet.forward_hip's unfused rollout chain on the same operands (text_k = the float64 projection, rounded once)"""
    c = dv.c
    cell, rows, H, Hq, Ct, d_out = (c[k] for k in ("cell", "rows", "H", "Hq", "Ct", "d_out"))
    x2, feats = dv.x2(), torch.empty((rows, H), device=DEV)
    out = torch.empty((rows, dv.slots, H), device=DEV)
    o_txt, o_dep, o_map = H, H + Ct, H + Ct + d_out
    state = x2[:, :H]

    def step(x, enc, w_ih, w_hh, b_ih, b_hh, h_new):
        if cell == "gru":
            ops.gru_step(x, None, dv.h_in[:, enc], dv.mask, w_ih, w_hh, b_ih, b_hh, h_new, out[:, enc])
        else:
            ops.lstm_step(x, None, dv.h_in[:, 2 * enc], dv.h_in[:, 2 * enc + 1], dv.mask, w_ih, w_hh, b_ih, b_hh, h_new,
                          out[:, 2 * enc + 1], out[:, 2 * enc])

    step(dv.state_in, 0, dv.w_ih1, dv.w_hh1, dv.b_ih1, dv.b_hh1, state)
    q1 = ops.linear(state, dv.w_q, dv.b_q)
    text = x2[:, o_txt:o_txt + Ct]
    ops.attn(q1, dv.text_k, dv.txt, dv.lengths, c["scale"], text)
    q2 = ops.linear(text, dv.w_tq, dv.b_tq)
    ops.attn_small2(q2, dv.dkv[:, :Hq], dv.dkv[:, Hq:], x2[:, o_dep:o_dep + d_out], dv.mkv[:, :Hq], dv.mkv[:, Hq:],
                    x2[:, o_map:o_map + c["m_out"]], c["scale"])
    c2 = ops.linear(x2, dv.w_c, dv.b_c, relu=True)
    step(c2, 1, dv.w_ih2, dv.w_hh2, dv.b_ih2, dv.b_hh2, feats)
    torch.cuda.synchronize()
    return _outputs(cell, c, x2, feats, out)


def _name(c, mask0):
    return f"{FORMS[c['cell']][0]} rows={c['rows']} L={c['L']} P={c['P']} H={c['H']} mask0={mask0}"


def _compare(case, c, fused, unfused, bad, row=None):
    """every tensor against float64 under the bar; logged before anything is asserted.  row: that row alone, under the bar
    of its own values"""
    for k, r64 in c["ref"].items():
        f, u = fused[k].cpu().double(), unfused[k].cpu().double()
        if row is not None:
            f, u, r64 = f[row], u[row], r64[row]
        ef, eu = float((f - r64).abs().max()), float((u - r64).abs().max())
        mx = float(r64.abs().max())
        bar = 2 * eu + 4 * EPS * mx
        ok = ef <= bar  # (False for NaN)
        line = f"{case:56s} {k:5s} fused {ef:.3e}  unfused {eu:.3e}  max|ref| {mx:.3e}  bar {bar:.3e}  {'ok' if ok else 'OVER'}"
        print(line)
        _log(line, LOG)
        if not ok:
            bad.append(line)


def _slots_feed_the_outputs(c, fused):
    """feats is the second encoder's h slot, x2[:, :H] the first's: the same bytes"""
    return _same_bytes(fused["h2"], fused["feats"]) and _same_bytes(fused["h1"], fused["x2"][:, :c["H"]])


def _check_case(ops, c, mask0, bad, tag=""):
    """one fused run against the unfused chain and float64, with everything (a) asks of a run -> both runs' outputs"""
    dv = _Dev(c)
    fused, unfused = _run_fused(ops, dv), _run_unfused(ops, dv)
    again = _run_fused(ops, dv)
    case = _name(c, mask0) + tag
    _compare(case, c, fused, unfused, bad)
    for k in c["ref"]:
        assert _same_bytes(fused[k], again[k]), f"{case} {k}: two runs on the same bytes differ"
    assert _slots_feed_the_outputs(c, fused), case
    if mask0 == 0:  # the masked row took nothing from its incoming state: the same bytes with that state replaced
        assert all(float(s.abs().max()) > 0 for s in c["state"][0])  # (every incoming slot of that row is non-zero)
        c0 = dict(c)
        c0["state"] = c["state"].clone()
        c0["state"][0] = 0.0
        z = _run_fused(ops, _Dev(c0))
        for k in c["ref"]:
            assert _same_bytes(z[k][0], fused[k][0]), f"{case} {k}: a masked row depends on its incoming state"
    return fused, unfused


# ------------------------------------------------------------------------------------------------------------------
# a. each form alone
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell,rows,L,P,wide", KERNEL_CASES)
def test_fused_head_matches_float64(cell, rows, L, P, wide):
    from ivln_ce_amd import ops

    bad = []
    for mask0 in ((0, 1) if rows == 1 else (0,)):
        c = _case(cell, rows, L, P, wide, mask0)
        assert c["sin_w"] == (288 + 128 if wide else 52) and c["x2w"] == (1184 if wide else 132)
        assert tuple(c["state"].shape) == (rows, len(SLOTS[cell]), c["H"]) and c["w_hh2"].shape[0] == (3 if cell == "gru" else 4) * c["H"]
        m, ln = c["mask"], c["lengths"]
        if rows > 1:
            assert int(m[0]) == 0 and int(m[1:].min()) == 1
        if L > 1:
            assert int(ln.max()) == L and (rows == 1 or int(ln.min()) == 1)
        if L >= 255:  # (asserted by the case maker in float64: the last position of the full row is live)
            assert c["last_pos_move"] >= 1000 * c["floor"]
            print(f"{_name(c, mask0)}: text moves {c['last_pos_move']:.3e} without position {L - 1} = "
                  f"{c['last_pos_move'] / c['floor']:.3g} floors of the bar")
        _check_case(ops, c, mask0, bad)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_fused_head_with_an_empty_row(cell):
    """lengths = 0: every text logit is masked, the weights are uniform and txt is all zero - text must be exactly 0.0, the
    row finite, and its other tensors under the same bar (float64 needs no special handling: txt = 0 makes the result
    independent of the attention weights)."""
    from ivln_ce_amd import ops

    rows, L, P, wide, lengths = EMPTY_ROW_CASE
    c = _case(cell, rows, L, P, wide, 0, lengths)
    empty = [r for r in range(rows) if int(c["lengths"][r]) == 0]
    assert empty == [1] and float(c["txt"][1].abs().max()) == 0.0 and int(c["mask"][1]) == 1
    bad = []
    tag = " lengths=" + ",".join(map(str, lengths))
    fused, unfused = _check_case(ops, c, 0, bad, tag=tag)
    _compare(_name(c, 0) + tag + " row=1", c, fused, unfused, bad, row=1)  # the empty row alone: the bar of its own values
    H, Ct = c["H"], c["Ct"]
    text = fused["x2"][1, H:H + Ct]
    assert float(text.abs().max()) == 0.0, "the empty row's text is not exactly 0.0"  # (False for NaN)
    for k, v in fused.items():
        assert bool(torch.isfinite(v[1]).all()), f"{k}: the empty row is not finite"
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_fused_head_default_fold_strides(cell):
    """Mq and TQb as two separate contiguous tensors with Mq_img = TQb_img = 0 (run_cma's defaults (H + 1) * L and Hq * L):
    the same bytes as the strided single-buffer run on the same values."""
    from ivln_ce_amd import ops

    rows, L, P, wide = SPLIT_FOLD_CASE
    c = _case(cell, rows, L, P, wide, 0)
    dv = _Dev(c)
    assert dv.fold.stride(0) == (c["H"] + 1 + c["Hq"]) * L  # (neither default is the single buffer's stride)
    one, two = _run_fused(ops, dv), _run_fused(ops, dv, split_fold=True)
    for k in c["ref"]:
        assert _same_bytes(one[k], two[k]), f"{_name(c, 0)} {k}: the default fold strides give other bytes"


# ------------------------------------------------------------------------------------------------------------------
# b. the GRU envelope
# ------------------------------------------------------------------------------------------------------------------
def test_fused_gru_head_refuses_before_it_launches():
    from ivln_ce_amd import ops
    from ivln_ce_amd._lib import IvlnError

    c = _case("gru", 3, 17, 16, False, 0)
    dv = _Dev(c)
    n, H, rows = _ws_floats(ops, c), c["H"], c["rows"]

    def attempt(code, **change):
        ws = torch.full((n + SENT,), 3.0, device=DEV)
        x2, feats = dv.x2(), torch.full((rows, H), float("nan"), device=DEV)
        before = x2.clone()
        h_out, h_out_wide = _state_view(rows, 2, H)
        d = _desc(ops, dv, x2, h_out, feats, ws)
        for k, v in change.items():
            setattr(d, k, v)
        with pytest.raises(IvlnError, match=r"\(%d\)" % code):
            _step_op(ops, "gru")(d)
        torch.cuda.synchronize()
        # nothing ran: every output and the scratch keep their sentinels, the incoming state its values
        assert _same_bytes(x2, before) and bool(torch.isnan(feats).all()), change
        assert float((h_out_wide - 7.0).abs().max()) == 0.0 and float((ws - 3.0).abs().max()) == 0.0, change
        assert _same_bytes(dv.h_in, c["state"].to(DEV)) and _pads_intact(dv.h_in_wide, 2, H), change

    ld = dv.h_in.stride(0)
    assert ld == 2 * H + PAD
    attempt(E_UNSUPPORTED, P=17)
    attempt(E_UNSUPPORTED, L=513)
    attempt(E_UNSUPPORTED, L=0)
    attempt(E_UNSUPPORTED, H=96)
    attempt(E_UNSUPPORTED, H=0)  # (x2w no longer fits H: the width rule refuses it, as it always did)
    # consistent apart from H, ld_h a multiple of 4: nothing but the H <= 0 rule stands between these and a launch
    attempt(E_UNSUPPORTED, H=0, x2w=c["x2w"] - H)
    attempt(E_UNSUPPORTED, H=-64, x2w=c["x2w"] - H - 64)
    attempt(E_UNSUPPORTED, x2w=c["x2w"] + 4)
    attempt(E_UNSUPPORTED, x2w=c["x2w"] - 4)
    attempt(E_UNSUPPORTED, ld_h=ld + 2)
    for name in ("ws", "x2", "feats", "h_in", "h_out"):
        attempt(E_INVALID, **{name: None})
    attempt(E_INVALID, ld_h=2 * H - 4)
    attempt(E_INVALID, ld_ho=2 * H - 4)
    attempt(E_INVALID, h_out=dv.h_in.data_ptr(), ld_ho=ld)
    attempt(E_INVALID, h_out=dv.h_in.data_ptr() + 4 * H, ld_ho=ld)  # (overlapping, not equal: h_out slot 0 on h_in slot 1)
