"""GPU: the fused recurrent head with LSTM state encoders (ivln_cma_step_lstm_fwd, csrc/cma_step.hip).

  e. a GRU policy beside an LSTM one in the same process (first in the file: its baseline step runs before any LSTM step
     of this module)
  a. the kernel alone, through the C ABI, against the head restated in float64 torch from UNFOLDED weights
  b. the envelope: every refusal happens before any launch
  c. the policy: fused against unfused against the torch-CPU oracle (lstm_state_ref.MapCMAPolicyLSTMRef)
  d. a rollout: hipGraph replay against eager, with an episode reset in the middle

Bound of (a), per tensor:  max|fused - ref64| <= 2 * max|unfused - ref64| + 4 * 2^-24 * max|ref64|.  "Unfused" is the
project's op chain on the same device inputs (ops.lstm_step, ops.linear, ops.attn, ops.attn_small2), itself pinned to
float64 by tests/test_gpu_lstm_state.py and tests/test_gpu_kernels.py; the factor 2 is the margin every re-associated
kernel form here gets against its fp32 sibling, the floor is four fp32 ulps of the tensor's largest value.  Both errors
are logged per tensor before anything is asserted.  Bounds of (c): tests/test_gpu_policy.py's
test_fused_head_matches_unfused_chain_and_oracle (2e-5 between the two forms; 2e-4 / 1e-4 to the oracle)."""
import os
import re

import pytest
import torch

from cma_step_ref import FULL, SMALL, make_case
from lstm_state_ref import MapCMAPolicyLSTMRef, make_policy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
E_INVALID, E_UNSUPPORTED = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_log_open = False


def _log_dir():
    if os.environ.get("IVLN_TEST_LOG_DIR"):
        return os.environ["IVLN_TEST_LOG_DIR"]
    for line in open(os.path.join(ROOT, ".gitignore")):
        if re.fullmatch(r"\w+_out/", line.strip()):
            return line.strip().rstrip("/")
    return "test_logs"


def _log(line):
    global _log_open
    print(line)
    os.makedirs(_log_dir(), exist_ok=True)
    with open(os.path.join(_log_dir(), "cma_step_lstm.log"), "a" if _log_open else "w") as f:
        f.write(line + "\n")
    _log_open = True


def _same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _dev_obs(obs):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in obs.items()}


class _Counted:
    """ops.<name> replaced by a wrapper that records every call: (workspace pointer, inside a stream capture?)"""

    def __init__(self, monkeypatch, name):
        from ivln_ce_amd import ops

        self.calls = []
        real = getattr(ops, name)

        def wrapper(d, mode=None):
            self.calls.append((int(d.ws or 0), bool(torch.cuda.is_current_stream_capturing())))
            return real(d, mode)

        monkeypatch.setattr(ops, name, wrapper)

    def __len__(self):
        return len(self.calls)


# ------------------------------------------------------------------------------------------------------------------
# e. GRU untouched
# ------------------------------------------------------------------------------------------------------------------
def test_gru_policy_is_untouched_by_an_lstm_policy_in_the_same_process(monkeypatch):
    """The same GRU step before and after an LSTM policy has stepped at the same shape (same rows / L / P / H: a shared
    workspace or fold cache would collide exactly here), and in a fresh GRU policy afterwards: the same bytes; the GRU
    workspaces are the tensors they were, and no LSTM workspace is one of them."""
    from ivln_ce_amd import ops
    from ivln_ce_amd.synthetic import SyntheticRollout

    B = 4
    g = torch.Generator().manual_seed(5)
    obs = SyntheticRollout(B=B, seed=411, n_tokens=64).step()
    obs["occupancy_map"] = (torch.rand(B, 64, 64, generator=g) < 0.4).to(torch.uint8)
    obs["semantic_map"] = (torch.randint(0, 13, (B, 64, 64), generator=g) * obs["occupancy_map"]).to(torch.uint8)
    obs = _dev_obs(obs)
    prev = torch.randint(0, 4, (B, 1), generator=g).to(DEV)
    masks = torch.tensor([[1], [0], [1], [1]], dtype=torch.uint8, device=DEV)
    rnn2, rnn4 = (0.2 * torch.randn(B, 2, 512, generator=g)).to(DEV), (0.2 * torch.randn(B, 4, 512, generator=g)).to(DEV)
    n_gru, n_lstm = _Counted(monkeypatch, "cma_step"), _Counted(monkeypatch, "cma_step_lstm")

    def step(pol, rnn):
        with torch.no_grad():
            f, s = pol.net(obs, rnn, prev, masks)
        return f.clone(), s.clone()

    gru = make_policy("GRU").to(DEV).eval()
    f0, s0 = step(gru, rnn2)
    assert len(n_gru) == 1 and len(n_lstm) == 0
    ws_before = {k: (v, v.data_ptr()) for k, v in ops._cma_ws.items()}
    assert ws_before
    lstm = make_policy("LSTM").to(DEV).eval()
    fl, sl = step(lstm, rnn4)
    assert len(n_gru) == 1 and len(n_lstm) == 1 and tuple(sl.shape) == (B, 4, 512)
    assert set(ops._cma_ws) == set(ws_before)
    assert all(ops._cma_ws[k] is v and v.data_ptr() == p for k, (v, p) in ws_before.items())
    assert ops._cma_lstm_ws and not ({v.data_ptr() for v in ops._cma_lstm_ws.values()} & {v.data_ptr() for v in ops._cma_ws.values()})
    assert getattr(gru.net, "_cma_fold")[0].data_ptr() != getattr(lstm.net, "_cma_fold")[0].data_ptr()
    f1, s1 = step(gru, rnn2)
    f2, s2 = step(make_policy("GRU").to(DEV).eval(), rnn2)
    assert len(n_gru) == 3 and len(n_lstm) == 1
    assert _same_bytes(f0, f1) and _same_bytes(s0, s1), "the GRU policy's step changed after an LSTM policy stepped"
    assert _same_bytes(f0, f2) and _same_bytes(s0, s2), "a fresh GRU policy steps differently after an LSTM policy stepped"


# ------------------------------------------------------------------------------------------------------------------
# a. the kernel alone
# ------------------------------------------------------------------------------------------------------------------
PAD = 8  # floats between two rows of a state view: ld = 4H + 8


def _make_case(rows, L, P, w, mask0, seed):
    """Inputs (fp32, CPU) and the float64 restatement of the head from unfolded weights (tests/cma_step_ref.py)"""
    return make_case("lstm", rows, L, P, w, mask0, seed)


_cases = {}


def _case(rows, L, P, wide, mask0):
    key = (rows, L, P, wide, mask0)
    if key not in _cases:
        _cases[key] = _make_case(rows, L, P, FULL if wide else SMALL, mask0, seed=rows * 10007 + L * 101 + P + mask0)
    return _cases[key]


def _state_view(rows, H, fill=None):
    """(rows, 4, H) view with row stride 4H + PAD inside a wider buffer of sevens -> (view, buffer)"""
    wide = torch.full((rows, 4 * H + PAD), 7.0, device=DEV)
    v = wide.as_strided((rows, 4, H), (4 * H + PAD, H, 1), 4)
    if fill is not None:
        v.copy_(fill.to(DEV))
    return v, wide


def _pads_intact(wide, H):
    return float((wide[:, :4] - 7.0).abs().max()) == 0.0 and float((wide[:, 4 + 4 * H:] - 7.0).abs().max()) == 0.0


class _Dev:
    """the case's operands on the device, shared by the fused and the unfused run"""

    def __init__(self, c):
        self.c = c
        for k in ("state_in", "mask", "lengths", "txt", "dkv", "mkv", "prev", "fold", "text_k", "w_q", "b_q", "w_tq", "b_tq",
                  "w_c", "b_c", "w_ih1", "w_hh1", "b_ih1", "b_hh1", "w_ih2", "w_hh2", "b_ih2", "b_hh2"):
            setattr(self, k, c[k].to(DEV).contiguous())
        self.h_in, self.h_in_wide = _state_view(c["rows"], c["H"], c["state"])

    def x2(self):
        c = self.c
        x2 = torch.full((c["rows"], c["x2w"]), float("nan"), device=DEV)
        x2[:, c["x2w"] - c["E"]:] = self.prev  # the previous-action slice is the caller's
        return x2


def _desc(ops, dv, x2, h_out, feats, ws):
    c = dv.c
    d = ops.CmaStepDesc()
    d.rows, d.L, d.P, d.H, d.Hq, d.Ct, d.d_out, d.m_out, d.E, d.x2w = (c[k] for k in ("rows", "L", "P", "H", "Hq", "Ct", "d_out",
                                                                                     "m_out", "E", "x2w"))
    d.state_in, d.h_in, d.ld_h, d.mask = dv.state_in.data_ptr(), dv.h_in.data_ptr(), dv.h_in.stride(0), dv.mask.data_ptr()
    d.w_ih1, d.w_hh1, d.b_ih1, d.b_hh1 = (t.data_ptr() for t in (dv.w_ih1, dv.w_hh1, dv.b_ih1, dv.b_hh1))
    d.Mq, d.Mq_img = dv.fold.data_ptr(), dv.fold.stride(0)
    d.TQb, d.TQb_img = dv.fold[:, c["H"] + 1:].data_ptr(), dv.fold.stride(0)
    d.lengths, d.txt, d.dkv, d.mkv, d.scale = dv.lengths.data_ptr(), dv.txt.data_ptr(), dv.dkv.data_ptr(), dv.mkv.data_ptr(), c["scale"]
    d.w_c, d.b_c = dv.w_c.data_ptr(), dv.b_c.data_ptr()
    d.w_ih2, d.w_hh2, d.b_ih2, d.b_hh2 = (t.data_ptr() for t in (dv.w_ih2, dv.w_hh2, dv.b_ih2, dv.b_hh2))
    d.x2, d.h_out, d.ld_ho, d.feats, d.ws = x2.data_ptr(), h_out.data_ptr(), h_out.stride(0), feats.data_ptr(), ws.data_ptr()
    return d


def _ws_floats(ops, c):
    import ctypes as C

    L_ = ops._L()
    L_.ivln_cma_step_lstm_ws_floats.restype = C.c_int64
    L_.ivln_cma_step_lstm_ws_floats.argtypes = [C.c_int] * 4
    return int(L_.ivln_cma_step_lstm_ws_floats(c["rows"], c["L"], c["P"], c["H"]))


SENT = 64  # floats of sentinel behind the scratch


def _run_fused(ops, dv):
    c = dv.c
    n = _ws_floats(ops, c)
    assert n >= c["rows"] * (c["L"] * (1 + 2 * c["P"]) + 5 * c["H"])  # logits, S tables, the 4H hidden half, c2
    ws = torch.full((n + SENT,), 3.0, device=DEV)
    x2, feats = dv.x2(), torch.full((c["rows"], c["H"]), float("nan"), device=DEV)
    h_out, h_out_wide = _state_view(c["rows"], c["H"])
    ops.cma_step_lstm(_desc(ops, dv, x2, h_out, feats, ws))
    torch.cuda.synchronize()
    assert float((ws[n:] - 3.0).abs().max()) == 0.0, "the kernel wrote behind ivln_cma_step_lstm_ws_floats() floats"
    assert _pads_intact(h_out_wide, c["H"]) and _pads_intact(dv.h_in_wide, c["H"])
    assert _same_bytes(dv.h_in, c["state"].to(DEV)), "the incoming state was written"
    assert _same_bytes(x2[:, c["x2w"] - c["E"]:], dv.prev), "the caller's previous-action slice of x2 was written"
    return dict(x2=x2[:, :c["x2w"] - c["E"]], feats=feats, h1=h_out[:, 0], c1=h_out[:, 1], h2=h_out[:, 2], c2=h_out[:, 3])


def _run_unfused(ops, dv):
    """MapCMANet.forward_hip's unfused rollout chain on the same operands (text_k = the float64 projection, rounded once)"""
    c = dv.c
    rows, H, Hq, Ct, d_out, m_out, L, P = (c[k] for k in ("rows", "H", "Hq", "Ct", "d_out", "m_out", "L", "P"))
    x2, feats = dv.x2(), torch.empty((rows, H), device=DEV)
    out = torch.empty((rows, 4, H), device=DEV)
    o_txt, o_dep, o_map = H, H + Ct, H + Ct + d_out
    state = x2[:, :H]
    ops.lstm_step(dv.state_in, None, dv.h_in[:, 0], dv.h_in[:, 1], dv.mask, dv.w_ih1, dv.w_hh1, dv.b_ih1, dv.b_hh1, state,
                  out[:, 1], out[:, 0])
    q1 = ops.linear(state, dv.w_q, dv.b_q)
    text = x2[:, o_txt:o_txt + Ct]
    ops.attn(q1, dv.text_k, dv.txt, dv.lengths, c["scale"], text)
    q2 = ops.linear(text, dv.w_tq, dv.b_tq)
    ops.attn_small2(q2, dv.dkv[:, :Hq], dv.dkv[:, Hq:], x2[:, o_dep:o_dep + d_out], dv.mkv[:, :Hq], dv.mkv[:, Hq:],
                    x2[:, o_map:o_map + m_out], c["scale"])
    c2 = ops.linear(x2, dv.w_c, dv.b_c, relu=True)
    ops.lstm_step(c2, None, dv.h_in[:, 2], dv.h_in[:, 3], dv.mask, dv.w_ih2, dv.w_hh2, dv.b_ih2, dv.b_hh2, feats, out[:, 3],
                  out[:, 2])
    torch.cuda.synchronize()
    return dict(x2=x2[:, :c["x2w"] - c["E"]], feats=feats, h1=out[:, 0], c1=out[:, 1], h2=out[:, 2], c2=out[:, 3])


KERNEL_CASES = [(1, 1, 1, False), (3, 17, 16, False), (4, 64, 4, False), (5, 33, 16, False), (8, 16, 9, False),
                (9, 40, 16, False), (20, 12, 16, False), (8, 80, 16, True)]


@pytest.mark.parametrize("rows,L,P,wide", KERNEL_CASES)
def test_fused_lstm_head_matches_float64(rows, L, P, wide):
    from ivln_ce_amd import ops

    bad = []
    for mask0 in ((0, 1) if rows == 1 else (0,)):
        c = _case(rows, L, P, wide, mask0)
        assert c["sin_w"] == (288 + 128 if wide else 52) and c["x2w"] == (1184 if wide else 132)
        m, ln, st = c["mask"], c["lengths"], c["state"]
        if rows > 1:
            assert int(m[0]) == 0 and int(m[1:].min()) == 1 and float(st[0, 0].abs().max()) > 0 and float(st[0, 1].abs().max()) > 0
            assert float(st[0, 2].abs().max()) > 0 and float(st[0, 3].abs().max()) > 0
        if L > 1:
            assert int(ln.max()) == L and (rows == 1 or int(ln.min()) == 1)
        dv = _Dev(c)
        assert dv.h_in.stride(0) == 4 * c["H"] + PAD > 4 * c["H"]
        fused, unfused = _run_fused(ops, dv), _run_unfused(ops, dv)
        again = _run_fused(ops, dv)
        case = f"cma_step_lstm rows={rows} L={L} P={P} H={c['H']} mask0={mask0}"
        for k, r64 in c["ref"].items():
            ef = float((fused[k].cpu().double() - r64).abs().max())
            eu = float((unfused[k].cpu().double() - r64).abs().max())
            mx = float(r64.abs().max())
            bar = 2 * eu + 4 * EPS * mx
            ok = ef <= bar  # (False for NaN)
            line = f"{case:52s} {k:5s} fused {ef:.3e}  unfused {eu:.3e}  max|ref| {mx:.3e}  bar {bar:.3e}  {'ok' if ok else 'OVER'}"
            _log(line)
            if not ok:
                bad.append(line)
            assert _same_bytes(fused[k], again[k]), f"{case} {k}: two runs on the same bytes differ"
        assert _same_bytes(fused["h2"], fused["feats"]) and _same_bytes(fused["h1"], fused["x2"][:, :c["H"]])
        if mask0 == 0:  # the masked row took nothing from its incoming state: the same bytes with that state replaced
            c0 = dict(c)
            c0["state"] = c["state"].clone()
            c0["state"][0] = 0.0
            z = _run_fused(ops, _Dev(c0))
            for k in c["ref"]:
                assert _same_bytes(z[k][0], fused[k][0]), f"{case} {k}: a masked row depends on its incoming state"
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------------
# b. the envelope
# ------------------------------------------------------------------------------------------------------------------
def test_fused_lstm_head_refuses_before_it_launches():
    from ivln_ce_amd import ops
    from ivln_ce_amd._lib import IvlnError

    c = _case(3, 17, 16, False, 0)
    dv = _Dev(c)
    n = _ws_floats(ops, c)

    def attempt(code, **change):
        ws = torch.full((n + SENT,), 3.0, device=DEV)
        x2, feats = dv.x2(), torch.full((c["rows"], c["H"]), float("nan"), device=DEV)
        before = x2.clone()
        h_out, h_out_wide = _state_view(c["rows"], c["H"])
        d = _desc(ops, dv, x2, h_out, feats, ws)
        for k, v in change.items():
            setattr(d, k, v)
        with pytest.raises(IvlnError, match=r"\(%d\)" % code):
            ops.cma_step_lstm(d)
        torch.cuda.synchronize()
        # nothing ran: every output and the scratch keep their sentinels, the incoming state its values
        assert _same_bytes(x2, before) and bool(torch.isnan(feats).all()), change
        assert float((h_out_wide - 7.0).abs().max()) == 0.0 and float((ws - 3.0).abs().max()) == 0.0, change
        assert _same_bytes(dv.h_in, c["state"].to(DEV)) and _pads_intact(dv.h_in_wide, c["H"]), change

    attempt(E_UNSUPPORTED, P=17)
    attempt(E_UNSUPPORTED, L=513)
    attempt(E_UNSUPPORTED, H=96)
    attempt(E_UNSUPPORTED, x2w=c["x2w"] + 4)
    attempt(E_UNSUPPORTED, x2w=c["x2w"] - 4)
    attempt(E_UNSUPPORTED, ld_ho=4 * c["H"] + PAD + 2)
    attempt(E_INVALID, ws=None)
    attempt(E_INVALID, h_out=dv.h_in.data_ptr(), ld_ho=dv.h_in.stride(0))
    attempt(E_INVALID, h_out=dv.h_in.data_ptr() + 4 * 2 * c["H"], ld_ho=dv.h_in.stride(0))  # (overlapping, not equal)


# ------------------------------------------------------------------------------------------------------------------
# c. the policy
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,lens", [(3, None), (8, None), (4, [1, 200, 17, 80]), (20, None)])
def test_fused_lstm_head_matches_unfused_chain_and_oracle(B, lens, monkeypatch):
    from ivln_ce_amd import ops
    from ivln_ce_amd.synthetic import SyntheticRollout

    torch.set_num_threads(8)
    pol = make_policy("LSTM").to(DEV).eval()
    ref = MapCMAPolicyLSTMRef().eval()
    ref.load_state_dict({k: v.cpu() for k, v in pol.state_dict().items()})
    g = torch.Generator().manual_seed(40 + B)
    obs = SyntheticRollout(B=B, seed=300 + B, n_tokens=64).step()
    if lens is not None:
        for b, n in enumerate(lens):
            obs["instruction"][b] = 0
            obs["instruction"][b, :n] = torch.randint(2, 2504, (n,), generator=g)
    obs["occupancy_map"] = (torch.rand(B, 64, 64, generator=g) < 0.4).to(torch.uint8)
    obs["semantic_map"] = (torch.randint(0, 13, (B, 64, 64), generator=g) * obs["occupancy_map"]).to(torch.uint8)
    rnn = 0.2 * torch.randn(B, 4, 512, generator=g)
    prev = torch.randint(0, 4, (B, 1), generator=g)
    masks = (torch.rand(B, 1, generator=g) < 0.7).to(torch.uint8)
    masks[0], masks[1] = 0, 1  # at least one of each
    dobs = _dev_obs(obs)
    n_lstm, n_gru = _Counted(monkeypatch, "cma_step_lstm"), _Counted(monkeypatch, "cma_step")
    out = {}
    saved = ops.CMA_STEP_MODE
    try:
        for mode in (-1, 0):
            ops.CMA_STEP_MODE = mode
            with torch.no_grad():
                f, s = pol.net(dobs, rnn.to(DEV), prev.to(DEV), masks.to(DEV))
                lg = pol.action_distribution.raw_logits(f)
            out[mode] = (f.cpu(), s.cpu(), lg.cpu())
            assert len(n_lstm) == (0 if mode < 0 else 1), f"mode {mode}: ivln_cma_step_lstm_fwd ran {len(n_lstm)} times"
    finally:
        ops.CMA_STEP_MODE = saved
    assert len(n_gru) == 0
    assert tuple(out[0][1].shape) == (B, 4, 512)
    with torch.no_grad():
        lr, sr, fr = ref.logits(obs, rnn, prev, masks)
    names = ("features", "state", "logits")
    for k in range(3):
        _log(f"policy B={B} lens={lens} {names[k]:8s} fused-unfused {float((out[0][k] - out[-1][k]).abs().max()):.3e}  "
             f"fused-oracle {float((out[0][k] - (fr, sr, lr)[k]).abs().max()):.3e}  "
             f"unfused-oracle {float((out[-1][k] - (fr, sr, lr)[k]).abs().max()):.3e}")
    for k in range(3):
        assert float((out[0][k] - out[-1][k]).abs().max()) < 2e-5, names[k]
    for mode in (-1, 0):
        assert float((out[mode][0] - fr).abs().max()) < 2e-4
        assert float((out[mode][1] - sr).abs().max()) < 2e-4
        assert float((out[mode][2] - lr).abs().max()) < 1e-4


# ------------------------------------------------------------------------------------------------------------------
# d. the rollout
# ------------------------------------------------------------------------------------------------------------------
def _rollout_obs(B, steps, seed, reset=None):
    """SyntheticRollout observations on the device; `reset` = (step, row): that row starts a new episode there"""
    from ivln_ce_amd.synthetic import SyntheticRollout

    roll = SyntheticRollout(B=B, seed=seed)
    obs = []
    for t in range(steps):
        o = roll.step()
        if reset is not None and t == reset[0]:
            o["not_done_masks"][reset[1]] = 0
        obs.append(_dev_obs(o))
    return obs


def test_graph_replay_of_the_fused_lstm_step_is_bit_identical_to_eager(same_depth_path, monkeypatch):
    same_depth_path(0)
    from ivln_ce_amd import ops
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.graphed import GraphedRollout
    from ivln_ce_amd.obs_transforms import GTSemanticsIterativeMapper

    assert ops.CMA_STEP_MODE >= 0
    B, steps = 2, 5
    pol = make_policy("LSTM").to(DEV).eval()
    cfg = get_config()
    obs = _rollout_obs(B, steps, seed=31, reset=(3, 0))
    n_lstm, n_gru = _Counted(monkeypatch, "cma_step_lstm"), _Counted(monkeypatch, "cma_step")
    tr_e = GTSemanticsIterativeMapper.from_config(cfg)
    rnn = torch.zeros(B, 4, 512, device=DEV)
    prev = torch.zeros(B, 1, dtype=torch.long, device=DEV)
    eager = []
    for o in obs:
        b = tr_e(dict(o))
        with torch.no_grad():
            a, rnn = pol.act(b, rnn, prev, b["not_done_masks"], deterministic=True)
        prev = a
        eager.append((a.clone(), rnn.clone()))
    assert len(n_lstm) == steps and not any(cap for _, cap in n_lstm.calls)
    assert float(eager[-1][1][:, 1].abs().max()) > 0 and float(eager[-1][1][:, 3].abs().max()) > 0  # both cell states live
    tr_g = GTSemanticsIterativeMapper.from_config(cfg)
    runner = GraphedRollout(pol, [tr_g], obs[0], deterministic=True)
    captured = [ws for ws, cap in n_lstm.calls[steps:] if cap]
    assert captured, "the fused LSTM head was not called inside the captured step"
    own = [v for k, v in ops._cma_lstm_ws.items() if k[-1] == id(runner)]
    assert len(own) == 1 and set(captured) == {own[0].data_ptr()}, "the captured step does not use the runner's own workspace"
    assert all(ws != own[0].data_ptr() for ws, _ in n_lstm.calls[:steps])  # (the eager steps used the eager workspace)
    n_built = len(n_lstm)
    tr_g.mapping_module.reset()
    runner.reset_state()
    for t, o in enumerate(obs):
        a = runner.step(o)
        torch.cuda.synchronize()
        assert tuple(runner.rnn_states.shape) == (B, 4, 512)
        assert torch.equal(a, eager[t][0]), f"actions step {t}"
        assert _same_bytes(runner.rnn_states, eager[t][1]), f"rnn step {t}"
    tr_g.mapping_module.check_status()
    assert len(n_lstm) == n_built, "a replayed step went through Python again"
    now = [v for k, v in ops._cma_lstm_ws.items() if k[-1] == id(runner)]
    assert len(now) == 1 and now[0] is own[0] and now[0].data_ptr() == captured[0]  # the pointer baked into the graph is alive
    assert float(runner.rnn_states[:, 1].abs().max()) > 0 and float(runner.rnn_states[:, 3].abs().max()) > 0
    assert len(n_gru) == 0
