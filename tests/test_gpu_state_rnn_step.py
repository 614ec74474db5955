"""GPU: the step kernel that serves both recurrent state encoders (csrc/state_rnn.hip k_rnn_step<Cell, LPR, VEC>, entry
points ivln_gru_step_f32 / ivln_lstm_step_f32) alone, at the edges of its work split, against float64 on the CPU.

  rows 4 / 5    the switch from 64 to 32 lanes per row
  rows 9 / 17   a second pass with one live row of eight, and a third
  H = 8, I = 8      two of the 32 (64) lanes of a row hold a 16-byte piece of K, the others none
  H = 132, I = 20   33 pieces: the last stride over K is partial (one lane of 32)
  LSTM, rows 9: c_out aliasing c_in (the state advanced in place, as the sequence does), and the 4-byte-load form (h_in
  4 bytes off a 16-byte boundary; the GRU has no such form and refuses it, tests/test_gpu_forward_kernels.py)

Bar: tests/kernel_bar.py, 4 * e32 + 4 * 2^-24 * max|float64| with e32 = max|fp32 torch-CPU - float64| on the same inputs.
What the kernel only selects or copies is compared exactly: h_out2 against h_out, the LSTM's saved c_t against c_out, and a
masked row against the same row fed a zero state.  Every output is a column slice of a sentinel-filled matrix or lies
between sentinel bands; masks mix 0 and 1 in one batch; both input forms (x, precomputed gi) are run."""
import pytest
import torch
import torch.nn.functional as F

from kernel_bar import _Bar, _same_bytes, _twice
from test_gpu_forward_kernels import DEV, PAD, _band, _band_ok, _cols, _cols_ok, _gen, _gru_ref, _in_cols

pytestmark = pytest.mark.gpu
LOG = "state_rnn_step.log"
NG = {"GRU": 3, "LSTM": 4}


def _lstm_ref(x, gi_pre, h_in, c_in, mask, w_ih, w_hh, b_ih, b_hh, dt):
    H = w_hh.shape[1]
    m = mask.to(dt).view(-1, 1)
    gi = F.linear(x.to(dt), w_ih.to(dt), b_ih.to(dt)) if x is not None else gi_pre.to(dt)
    pre = gi + F.linear(h_in.to(dt) * m, w_hh.to(dt), b_hh.to(dt))
    i, f, g, o = (torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]),
                  torch.sigmoid(pre[:, 3 * H:]))
    ct = f * (c_in.to(dt) * m) + i * g
    return o * torch.tanh(ct), i, f, g, o, ct   # h_t, then the saves in the kernel's order


CASES = [(4, 64, 36, ""), (5, 64, 36, ""), (9, 64, 36, ""), (17, 64, 36, ""), (9, 8, 8, ""), (9, 132, 20, "")]
LSTM_ONLY = [(9, 64, 36, "c in place"), (9, 64, 36, "4-byte loads")]


@pytest.mark.parametrize("cell,rows,H,I,form", [("GRU",) + c for c in CASES] + [("LSTM",) + c for c in CASES + LSTM_ONLY])
def test_step_kernel_at_its_edges(cell, rows, H, I, form):
    from ivln_ce_amd import ops

    G = NG[cell] * H
    g = _gen(NG[cell], rows, H, I)
    x, h_in, c_in = torch.randn(rows, I, generator=g), torch.randn(rows, H, generator=g), torch.randn(rows, H, generator=g)
    w_ih, w_hh = torch.randn(G, I, generator=g) * I ** -0.5, torch.randn(G, H, generator=g) * H ** -0.5
    b_ih, b_hh = torch.randn(G, generator=g) * 0.1, torch.randn(G, generator=g) * 0.1
    mask = (torch.rand(rows, generator=g) < 0.6).to(torch.uint8)
    mask[0], mask[1], mask[-1] = 0, 1, 1   # 0 and 1 in the first pass, a live last row
    gi_pre = F.linear(x, w_ih, b_ih)
    off = form == "4-byte loads"
    x_d, gi_d, m_d = _in_cols(x), _in_cols(gi_pre), mask.to(DEV)
    h_d = _in_cols(h_in, 5, 7) if off else _in_cols(h_in, 4, 8)
    assert h_d.data_ptr() % 16 == (4 if off else 0) and x_d.data_ptr() % 16 == 0
    wd = [t.to(DEV) for t in (w_ih, w_hh, b_ih, b_hh)]
    nsave = NG[cell] + 1
    for use_x in (True, False):
        def run(h_src=h_d, c_src=c_in):
            o1, o1_w = _cols(rows, H, 4, 4)
            o2, o2_w = _cols(rows, H, 8, 4)
            sv = [_band(rows * H) for _ in range(nsave)]
            saves = tuple(s[0].view(rows, H) for s in sv)
            xa, ga = (x_d, None) if use_x else (None, gi_d)
            if cell == "GRU":
                ops.gru_step(xa, ga, h_src, m_d, *wd, o1, o2, saves=saves)
                return (o1_w, o2_w) + tuple(s[1] for s in sv)
            c_d = _in_cols(c_src, 4, 12)
            co, co_w = (c_d, c_d._base) if form == "c in place" else _cols(rows, H, 12, 4)
            ops.lstm_step(xa, ga, h_src, c_d, m_d, *wd, o1, co, o2, saves)
            return (o1_w, o2_w) + tuple(s[1] for s in sv) + (co_w,)

        got = _twice(run)
        case = f"{cell} rows={rows} H={H} I={I} {'x' if use_x else 'gi_pre'} {form}"
        bar = _Bar(case, LOG)
        _cols_ok(got[0], 4, H, case + " h_out")
        _cols_ok(got[1], 8, H, case + " h_out2")
        a = (x if use_x else None, None if use_x else gi_pre, h_in)
        if cell == "GRU":
            r64, r32 = (_gru_ref(*a, mask, w_ih, w_hh, b_ih, b_hh, dt) for dt in (torch.float64, torch.float32))
            names = ("h_out", "save_r", "save_z", "save_n", "save_ghn")
        else:
            r64, r32 = (_lstm_ref(*a, c_in, mask, w_ih, w_hh, b_ih, b_hh, dt) for dt in (torch.float64, torch.float32))
            names = ("h_out", "save_i", "save_f", "save_g", "save_o", "save_c")
        h_out = got[0][:, 4:4 + H].contiguous()
        bar.check("h_out", h_out, r64[0], r32[0])
        assert _same_bytes(h_out, got[1][:, 8:8 + H].contiguous()), "h_out2 != h_out"
        for k, name in enumerate(names[1:]):
            _band_ok(got[2 + k], rows * H, case + " " + name)
            bar.check(name, got[2 + k][PAD:PAD + rows * H].view(rows, H), r64[1 + k], r32[1 + k])
        if cell == "LSTM":
            left = 4 if form == "c in place" else 12
            _cols_ok(got[-1], left, H, case + " c_out")
            c_out = got[-1][:, left:left + H].contiguous()
            assert _same_bytes(c_out, got[2 + 4][PAD:PAD + rows * H].view(rows, H)), "saved c_t != c_out"
        # a masked row does not see its incoming state: the same bytes with that state zeroed on the host
        keep = mask.view(-1, 1).to(torch.float32)
        zeroed = run(_in_cols(h_in * keep, 5, 7) if off else _in_cols(h_in * keep, 4, 8), c_in * keep)
        for u, v in zip(got, zeroed):
            assert _same_bytes(u, v), "a masked row depends on the state it drops"
        bar.done()
