"""CPU companion of tests/test_gpu_cma_step_kernels.py (the fused recurrent head, csrc/cma_step.hip): what backs the GPU
tests' reference and makes their edge claims checkable without a GPU.

  - the fold: the head computed in float64 from the folded operands [Mq | TQb] is the unfolded head (tests/cma_step_ref.py)
  - the scratch layout, restated with al32, against the library's ivln_cma_step[_lstm]_ws_floats() for every GPU case
  - the lane partitions of side_S, phase 3's softmax and chunk -> dst mapping, rnn_unit's row passes and lpr_dot's K walk,
    restated in numpy: every element counted / written exactly once
  - the wiring: the GPU file's case lists hold the edges named here, and both C entry points are run there"""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import test_gpu_cma_step_kernels as K
from cma_step_ref import FULL, SMALL, case_seed, doubles, head64, make_case

CT = 256  # threads per workgroup (cma_step.hip)


# ----------------------------------------------------------------------------------------------------------------------
# the fold
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", ["gru", "lstm"])
@pytest.mark.parametrize("rows,L,P,lengths", [(3, 17, 16, (17, 0, 1)), (5, 33, 16, None), (3, 511, 1, None), (2, 257, 16, None)])
def test_folded_head_is_the_unfolded_head_in_float64(cell, rows, L, P, lengths):
    c = make_case(cell, rows, L, P, SMALL, 0, case_seed(rows, L, P, 0), lengths)
    if lengths is not None:
        assert 0 in c["lengths"].tolist() and float(c["txt"][c["lengths"] == 0].abs().max()) == 0.0
    d = doubles(c)
    unfolded, folded = head64(cell, d), head64(cell, d, folded=True)
    assert list(unfolded) == list(c["ref"]) and all(torch.equal(unfolded[k], c["ref"][k]) for k in unfolded)
    for k in unfolded:
        assert float(unfolded[k].abs().max()) > 0.1  # (nothing is compared at zero)
        assert float((folded[k] - unfolded[k]).abs().max()) <= 1e-12, k
    # and the operand the kernels get is that fold, rounded once
    H, Hq = c["H"], c["Hq"]
    assert c["fold"].dtype == torch.float32 and tuple(c["fold"].shape) == (rows, H + 1 + Hq, L)
    assert c["text_k"].dtype == torch.float32 and tuple(c["text_k"].shape) == (rows, Hq, L)


# ----------------------------------------------------------------------------------------------------------------------
# scratch layout
# ----------------------------------------------------------------------------------------------------------------------
def al32(n):
    return (n + 31) & ~31


def layout(cell, rows, L, P, H, gru_gates=3):
    """[name, first float, floats] of every scratch region the form's kernels address (ws_logits, ws_S, ws_gh2, ws_c2)"""
    s0 = al32(rows * L)
    g0 = s0 + al32(rows * L * 2 * P)
    c0 = g0 + al32(rows * 3 * H)
    regions = [("logits", 0, rows * L), ("S", s0, rows * L * 2 * P), ("c2", c0, rows * H)]
    if cell == "gru":
        regions.append(("gh2", g0, rows * gru_gates * H))
    else:
        regions.append(("gh2", c0 + al32(rows * H), rows * 4 * H))
    return regions


def layout_faults(regions, total):
    bad = [f"{n} ends at {a + k} > {total}" for n, a, k in regions if a + k > total or a < 0 or k <= 0 or a % 32]
    for i, (n0, a0, k0) in enumerate(regions):
        for n1, a1, k1 in regions[i + 1:]:
            if a0 < a1 + k1 and a1 < a0 + k0:
                bad.append(f"{n0} overlaps {n1}")
    return bad


def _gpu_shapes():
    """(cell, rows, L, P, H) of every case of the GPU file"""
    out = [(cell, rows, L, P, (FULL if wide else SMALL)["H"]) for cell, rows, L, P, wide in K.KERNEL_CASES]
    for cell in ("gru", "lstm"):
        out += [(cell,) + K.EMPTY_ROW_CASE[:3] + (SMALL["H"],), (cell,) + K.SPLIT_FOLD_CASE[:3] + (SMALL["H"],)]
    return out


def test_scratch_regions_are_disjoint_and_inside_what_the_library_asks_for():
    import __graft_entry__ as ge

    lib = C.CDLL(ge.build())
    size = {}
    for cell, (_, _, name) in K.FORMS.items():
        size[cell] = getattr(lib, name)
        size[cell].restype, size[cell].argtypes = C.c_int64, [C.c_int] * 4
    shapes = _gpu_shapes()
    assert len(shapes) == len(K.KERNEL_CASES) + 4
    for cell, rows, L, P, H in shapes:
        total = int(size[cell](rows, L, P, H))
        assert layout_faults(layout(cell, rows, L, P, H), total) == [], (cell, rows, L, P, H)
        # the GRU's hidden half lies INSIDE the layout, directly in front of c2: one gate too many lands in c2, not in a sentinel
        assert "c2 overlaps gh2" in layout_faults(layout("gru", rows, L, P, H, gru_gates=4), total)
        # and the LSTM form's scratch is the GRU form's plus its own hidden half
        assert int(size["lstm"](rows, L, P, H)) == int(size["gru"](rows, L, P, H)) + al32(rows * 4 * H)


# ----------------------------------------------------------------------------------------------------------------------
# lane partitions
# ----------------------------------------------------------------------------------------------------------------------
def _shfl_xor(v, o):
    """v[t] of a 256-thread workgroup after `v += __shfl_xor(v, o, 64)`: lanes pair inside their wave"""
    t = np.arange(CT)
    return v + v[(t & ~63) | ((t & 63) ^ o)]


@pytest.mark.parametrize("Hq", [32, 256])
@pytest.mark.parametrize("P", [1, 9, 16])
def test_side_S_counts_every_channel_once(Hq, P):
    t = np.arange(CT)
    p, cs, cper = t & 15, t >> 4, Hq // 16
    cnt = np.zeros((CT, Hq), dtype=np.int64)  # how often thread t's a0 holds channel c's product
    for th in range(CT):
        if p[th] < P:
            cnt[th, cs[th] * cper:(cs[th] + 1) * cper] += 1
    cnt = _shfl_xor(_shfl_xor(cnt, 16), 32)
    sp = np.zeros((4, 16, Hq), dtype=np.int64)
    for th in range(CT):
        if (th & 63) < 16:
            sp[th >> 6, p[th]] = cnt[th]
    stored = {}
    for th in range(32):
        q, sset = th & 15, th >> 4
        if q < P:
            assert (sset * P + q) not in stored
            stored[sset * P + q] = sp[0, q] + sp[1, q] + sp[2, q] + sp[3, q]
    assert sorted(stored) == list(range(2 * P))  # both sets' P columns of item (n, i), each stored once
    for v in stored.values():
        assert v.tolist() == [1] * Hq


@pytest.mark.parametrize("L", [1, 255, 256, 257, 511, 512])
def test_phase3_softmax_slots_cover_the_instruction_axis_once(L):
    def covered(slots):
        n = np.zeros(L, dtype=np.int64)
        for tid in range(CT):
            for s in range(slots):
                if tid + s * CT < L:
                    n[tid + s * CT] += 1
        return n

    assert L <= 512 and covered(2).tolist() == [1] * L
    assert (covered(1).tolist() == [1] * L) == (L <= CT), "a softmax without its second slot goes unnoticed"


@pytest.mark.parametrize("w", [SMALL, FULL], ids=["small", "full"])
def test_phase3_chunks_write_every_column_between_state_and_prev_once(w):
    H, Ct, d_out, m_out, E = (w[k] for k in ("H", "Ct", "d_out", "m_out", "E"))
    x2w = H + Ct + d_out + m_out + E
    n_txt, n_dep, chunks = Ct // 16, d_out // 16, (Ct + d_out + m_out) // 16
    hits = np.zeros(x2w, dtype=np.int64)
    for ch in range(chunks):
        for co in range(16):
            if ch < n_txt:
                dst = H + ch * 16 + co
            else:
                sset = 0 if ch < n_txt + n_dep else 1
                cch = ch - n_txt if sset == 0 else ch - n_txt - n_dep
                dst = H + Ct + (0 if sset == 0 else d_out) + cch * 16 + co
            hits[dst] += 1
    assert hits[:H].sum() == 0 and hits[x2w - E:].sum() == 0 and hits[H:x2w - E].tolist() == [1] * (Ct + d_out + m_out)


def lanes_per_row(rows):
    """run_cma's choice"""
    return 64 if rows <= 4 else 32 if rows <= 8 else 16


@pytest.mark.parametrize("rows,lpr,passes,last_live", [(4, 64, 1, 4), (5, 32, 1, 5), (8, 32, 1, 8), (9, 16, 1, 9), (16, 16, 1, 16),
                                                       (17, 16, 2, 1), (33, 16, 3, 1)])
def test_rnn_unit_serves_each_row_once(rows, lpr, passes, last_live):
    assert lanes_per_row(rows) == lpr
    rpb = CT // lpr
    served, live = np.zeros(rows, dtype=np.int64), []
    for r0 in range(0, rows, rpb):
        live.append(0)
        for tid in range(CT):
            l, row = tid % lpr, r0 + tid // lpr
            if l == 0 and row < rows:
                served[row] += 1
                live[-1] += 1
    assert served.tolist() == [1] * rows and len(live) == passes and live[-1] == last_live


@pytest.mark.parametrize("lpr", [64, 32, 16])
def test_lpr_dot_walks_K_once_with_a_tail(lpr):
    tails = 0
    for w in (SMALL, FULL):
        sin_w = w["d_out"] + w["m_out"] + w["E"]
        for Kd in (sin_w, w["H"], w["H"] + w["Ct"] + sin_w):
            hits = np.zeros(Kd, dtype=np.int64)
            for l in range(lpr):
                for k in range(l * 4, Kd, lpr * 4):
                    hits[k:k + 4] += 1
            assert Kd % 4 == 0 and hits.tolist() == [1] * Kd
            tails += Kd % (lpr * 4) != 0
    assert tails >= 2  # (some lanes make one step fewer than others: sin_w = 52 and x2w = 132 at the small widths)


# ----------------------------------------------------------------------------------------------------------------------
# the envelope's host side
# ----------------------------------------------------------------------------------------------------------------------
def _host_desc(ops, cell, buf, **change):
    """A descriptor of the small widths that is inside the envelope, every pointer into `buf` (host memory: a refusal
    reads no operand and touches no device, so these never reach a kernel); h_in and h_out rows do not overlap."""
    w, slots, rows = SMALL, len(K.SLOTS[cell]), 3
    H = w["H"]
    base, ld = C.addressof(buf), slots * H + 8
    d = ops.CmaStepDesc()
    d.rows, d.L, d.P, d.H, d.Hq, d.Ct, d.d_out, d.m_out, d.E = rows, 17, 16, H, w["Hq"], w["Ct"], w["d_out"], w["m_out"], w["E"]
    d.x2w = H + w["Ct"] + w["d_out"] + w["m_out"] + w["E"]
    for name, ctype in ops.CmaStepDesc._fields_:
        if ctype is C.c_void_p:
            setattr(d, name, base)
    d.h_in, d.ld_h, d.h_out, d.ld_ho, d.scale = base, ld, base + 4 * rows * ld, ld, 1.0
    for k, v in change.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_state_rules_refuse_on_the_host_for_both_forms(cell):
    """The rules both entries ask of the state views, each reached by a descriptor that breaks nothing else (H = 0 with
    x2w to match: only `H <= 0` refuses it).  Only refused descriptors are sent: they return before the first HIP call."""
    import __graft_entry__ as ge
    from ivln_ce_amd import ops

    lib = C.CDLL(ge.build())
    fwd = getattr(lib, K.FORMS[cell][1])
    fwd.restype, fwd.argtypes = C.c_int, [C.POINTER(ops.CmaStepDesc), C.c_int, C.c_void_p]
    slots, H = len(K.SLOTS[cell]), SMALL["H"]
    ld, x2w = slots * H + 8, H + SMALL["Ct"] + SMALL["d_out"] + SMALL["m_out"] + SMALL["E"]
    buf = (C.c_float * (8 * ld))()
    base = C.addressof(buf)

    def code(**change):
        return fwd(C.byref(_host_desc(ops, cell, buf, **change)), 0, None)

    assert code(H=0, x2w=x2w - H) == K.E_UNSUPPORTED and code(H=-64, x2w=x2w - H - 64) == K.E_UNSUPPORTED
    assert code(ld_h=slots * H - 4) == K.E_INVALID and code(ld_ho=slots * H - 4) == K.E_INVALID
    assert code(h_out=base) == K.E_INVALID                       # h_out == h_in
    assert code(h_out=base + 4 * H) == K.E_INVALID               # one slot further: overlapping, not equal
    assert code(h_out=base + 4 * (2 * ld + slots * H - 1)) == K.E_INVALID  # h_out's first float is h_in's last
    assert code(ld_h=ld + 2) == K.E_UNSUPPORTED and code(h_in=None) == K.E_INVALID and code(h_out=None) == K.E_INVALID


# ----------------------------------------------------------------------------------------------------------------------
# wiring
# ----------------------------------------------------------------------------------------------------------------------
def test_gpu_cases_hold_the_edges_and_run_both_entry_points():
    from ivln_ce_amd import ops

    by_cell = {cell: [c[1:] for c in K.KERNEL_CASES if c[0] == cell] for cell in ("gru", "lstm")}
    assert len(K.KERNEL_CASES) == len(set(K.KERNEL_CASES))
    assert by_cell["gru"] == K.GRU_ONLY_CASES + K.BOTH_CASES and by_cell["lstm"] == K.BOTH_CASES
    import test_gpu_cma_step_lstm as LSTM
    assert K.GRU_ONLY_CASES == LSTM.KERNEL_CASES  # what the LSTM form always had, now for the GRU form too
    for cell, cases in by_cell.items():
        both = cases + LSTM.KERNEL_CASES if cell == "lstm" else cases
        rows = {c[0] for c in both}
        assert {4, 5, 8, 9}.issubset(rows), cell  # both sides of each lanes-per-row switch
        assert {16, 17, 33}.issubset({c[0] for c in cases}), cell  # one, two, three passes of the 16-lane form
        assert {255, 256, 257, 511, 512}.issubset({c[1] for c in cases}), cell
        assert any(c[2] == 1 and c[1] > CT for c in cases), cell  # P = 1 beside the second softmax slot
        assert any(c[3] and c[1] >= 200 for c in cases), cell  # the model's widths at a long instruction
        assert {c[2] for c in both} >= {1, 2, 4, 5, 9, 16}, cell
    assert K.EMPTY_ROW_CASE == (3, 17, 16, False, (17, 0, 1))
    assert all(L <= 512 and 1 <= P <= 16 and rows >= 1 for _, rows, L, P, _ in K.KERNEL_CASES)
    # the two forms go through two ops, each of which calls its own C entry point
    assert set(K.FORMS) == {"gru", "lstm"}
    for cell, entry in (("gru", "ivln_cma_step_fwd"), ("lstm", "ivln_cma_step_lstm_fwd")):
        op, named, _ = K.FORMS[cell]
        assert named == entry and ("." + entry + "(") in inspect.getsource(getattr(ops, op))
    assert "ivln_cma_step_lstm_fwd" not in inspect.getsource(ops.cma_step)
    assert K._step_op(ops, "gru") is ops.cma_step and K._step_op(ops, "lstm") is ops.cma_step_lstm
