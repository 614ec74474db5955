"""GPU: `MODEL.STATE_ENCODER.rnn_type: LSTM` - the masked LSTM step, its sequence form and its BPTT
(csrc/state_rnn.hip) alone against float64, then the MapCMA policy built with it: rollout steps, one update, and
hipGraph replay.

The reference of the kernel tests is `torch.nn.LSTM` in float64 driven step by step with h and c multiplied by the
mask before every step (lstm_state_ref.LSTMStateEncoderRef).  nn.LSTM does not expose the gate pre-activations, so the
quantities it cannot give (the activated gates, the masked h_{t-1} rows, d(loss)/d(pre-activations)) come from the same
loop written out cell by cell in float64, which is first pinned to nn.LSTM's outputs and gradients at 1e-12.

Bounds (none of them derived from what the kernels give):
  step      2e-5 absolute + 1e-4 relative: what tests/test_gpu_kernels.py::test_gru_step holds against torch
  sequence  1e-5 absolute + 1e-4 relative: what test_persistent_sequence_gru_matches_per_step_launches_and_torch holds
  backward  4 x (error of the torch-CPU fp32 run against its own float64 run, same inputs) + 4 * 2^-24 * max|ref|:
            tests/test_gpu_train_kernels.py::_Bar, the bar of test_gru_bptt_kernels
  policy    logits 1e-4, features / states 2e-4: tests/test_gpu_policy.py
  update    per tensor max|err| <= 1e-3 max|ref| + 2e-7 and direction cosine >= 1 - 1e-6:
            tests/test_gpu_train.py::test_benched_update_path_full_gradients_at_T64_N8
Every comparison is logged (error, the torch-CPU fp32 error on the same inputs, the bound) before anything is asserted.
"""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from lstm_state_ref import LSTMStateEncoderRef, MapCMAPolicyLSTMRef, make_policy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
E_INVALID = -1
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
    with open(os.path.join(_log_dir(), "lstm_state.log"), "a" if _log_open else "w") as f:
        f.write(line + "\n")
    _log_open = True


class _Check:
    """Collects the comparisons of one case: everything is logged before anything is asserted."""

    def __init__(self, case):
        self.case, self.bad = case, []

    def _note(self, name, err, e32, mx, bar):
        ok = err <= bar  # (False for NaN)
        line = f"{self.case:34s} {name:10s} hip {err:.3e}  e32 {e32:.3e}  max|ref| {mx:.3e}  bar {bar:.3e}  {'ok' if ok else 'OVER'}"
        _log(line)
        if not ok:
            self.bad.append(line)

    def close(self, name, got, ref64, ref32, atol, rtol=1e-4):
        """torch.allclose's form: |got - ref| <= atol + rtol |ref| elementwise; the log gives the worst element"""
        got, r64, r32 = (t.detach().cpu().double().reshape(-1) for t in (got, ref64, ref32))
        assert got.shape == r64.shape == r32.shape, (name, got.shape, r64.shape)
        d = (got - r64).abs()
        over = d - (atol + rtol * r64.abs())
        i = int(torch.nan_to_num(over, nan=float("inf")).argmax())
        self._note(name, float(d[i]), float((r32 - r64).abs().max()), float(r64.abs().max()), float(atol + rtol * r64[i].abs()))

    def bar(self, name, got, ref64, ref32, factor=4.0):
        """tensor-wide: max|got - ref| <= factor * max|fp32 torch - ref| + 4 * 2^-24 * max|ref|"""
        got, r64, r32 = (t.detach().cpu().double().reshape(-1) for t in (got, ref64, ref32))
        assert got.shape == r64.shape == r32.shape, (name, got.shape, r64.shape)
        e32, mx = float((r32 - r64).abs().max()), float(r64.abs().max())
        self._note(name, float((got - r64).abs().max()), e32, mx, factor * e32 + 4 * EPS * mx)

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def _same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------
# the reference: one case per (T, N, I, H), computed once and shared
# ------------------------------------------------------------------------------------------------------------------
def _leaf(t, dt):
    return t.detach().to(dt).clone().requires_grad_(True)


def _make_case(T, N, I, H, seed):
    g = torch.Generator().manual_seed(seed)
    c = dict(T=T, N=N, I=I, H=H, x=torch.randn(T, N, I, generator=g),
             w_ih=torch.randn(4 * H, I, generator=g) * (0.7 / I ** 0.5), b_ih=torch.randn(4 * H, generator=g) * 0.1,
             w_hh=torch.randn(4 * H, H, generator=g) * (0.8 / H ** 0.5), b_hh=torch.randn(4 * H, generator=g) * 0.1,
             h0=torch.randn(N, H, generator=g) * 0.5, c0=torch.randn(N, H, generator=g), d_out=torch.randn(T, N, H, generator=g))
    masks = torch.ones(T, N, dtype=torch.uint8)
    if N > 1:
        masks[0, 0] = 0  # an episode starts at t = 0: the incoming state of that row is dropped
    if T > 1:
        masks[T // 2, min(1, N - 1)] = 0  # ... and in the middle of the sequence
    c["masks"] = masks
    return c


def _cell_loop(c, dt):
    """the masked LSTM written out cell by cell, with autograd: gates i, f, g, o"""
    T, N, H = c["T"], c["N"], c["H"]
    x, w_ih, b_ih, w_hh, b_hh, h0, c0 = (_leaf(c[k], dt) for k in ("x", "w_ih", "b_ih", "w_hh", "b_hh", "h0", "c0"))
    h, cs, outs, pres, hps, sv = h0, c0, [], [], [], []
    for t in range(T):
        m = c["masks"][t].to(dt).view(N, 1)
        hp, cp = h * m, cs * m
        pre = x[t] @ w_ih.t() + b_ih + hp @ w_hh.t() + b_hh
        pre.retain_grad()
        i, f, gg, o = (torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]),
                       torch.sigmoid(pre[:, 3 * H:]))
        cs = f * cp + i * gg
        h = o * torch.tanh(cs)
        outs.append(h), pres.append(pre), hps.append(hp), sv.append((i, f, gg, o, cs))
    (torch.stack(outs) * c["d_out"].to(dt)).sum().backward()
    return dict(out=torch.stack(outs).detach(), hT=h.detach(), cT=cs.detach(),
                saves=[torch.stack([s[k] for s in sv]).detach() for k in range(5)], hp=torch.stack(hps).detach(),
                dgi=torch.stack([p.grad for p in pres]), dw_ih=w_ih.grad, dw_hh=w_hh.grad, db_ih=b_ih.grad, db_hh=b_hh.grad,
                dx=x.grad, dh0=h0.grad, dc0=c0.grad, gi=(x.detach() @ w_ih.detach().t() + b_ih.detach()))


def _nn_lstm(c, dt):
    """torch.nn.LSTM driven step by step with the masking (lstm_state_ref.LSTMStateEncoderRef), with autograd"""
    T, N, I, H = c["T"], c["N"], c["I"], c["H"]
    enc = LSTMStateEncoderRef(I, H).to(dt)
    with torch.no_grad():
        for k in ("w_ih", "w_hh", "b_ih", "b_hh"):
            getattr(enc.rnn, {"w": "weight", "b": "bias"}[k[0]] + k[1:] + "_l0").copy_(c[k].to(dt))
    x, h0, c0 = _leaf(c["x"], dt), _leaf(c["h0"], dt), _leaf(c["c0"], dt)
    out, state = enc(x.view(T * N, I), torch.stack([h0, c0], 1), c["masks"].view(T * N, 1))
    (out.view(T, N, H) * c["d_out"].to(dt)).sum().backward()
    r = enc.rnn
    return dict(out=out.view(T, N, H).detach(), hT=state[:, 0].detach(), cT=state[:, 1].detach(), dw_ih=r.weight_ih_l0.grad,
                dw_hh=r.weight_hh_l0.grad, db_ih=r.bias_ih_l0.grad, db_hh=r.bias_hh_l0.grad, dx=x.grad, dh0=h0.grad, dc0=c0.grad)


_cases = {}


def _case(T, N, I, H):
    key = (T, N, I, H)
    if key not in _cases:
        c = _make_case(T, N, I, H, seed=T * 1000 + N * 100 + H + I)
        r64, r32 = _cell_loop(c, torch.float64), _cell_loop(c, torch.float32)
        n64, n32 = _nn_lstm(c, torch.float64), _nn_lstm(c, torch.float32)
        for k, v in n64.items():  # the cell loop IS nn.LSTM's arithmetic
            assert float((v - r64[k]).abs().max()) <= 1e-12 * max(1.0, float(v.abs().max())), k
        r32.update(n32)  # fp32 figures: nn.LSTM's own wherever it has the quantity
        _cases[key] = (c, r64, r32)
    return _cases[key]


I_OF_H = {64: 20, 128: 96, 512: 416}


def _dev_weights(c):
    return {k: c[k].to(DEV) for k in ("w_ih", "w_hh", "b_ih", "b_hh")}


def _state_slices(c, slots):
    """h0 / c0 as the last two slots of a (N, slots, H) tensor: row stride slots * H, as the policy passes them"""
    wide = torch.full((c["N"], slots, c["H"]), 7.0, device=DEV)
    wide[:, slots - 2], wide[:, slots - 1] = c["h0"].to(DEV), c["c0"].to(DEV)
    return wide[:, slots - 2], wide[:, slots - 1]


def _strided_out(rows, H):
    wide = torch.full((rows, H + 8), 7.0, device=DEV)
    return wide[:, 4:4 + H], wide


# ------------------------------------------------------------------------------------------------------------------
# 1. one step
# ------------------------------------------------------------------------------------------------------------------
# (2, 22, 64): I % 4 != 0 - the 4-byte-load form of the kernel; the three other shapes take the 16-byte loads, with 64
# lanes per row up to 4 rows and 32 beyond
@pytest.mark.parametrize("rows,I,H", [(1, 20, 64), (3, 96, 128), (8, 416, 512), (2, 22, 64)])
def test_lstm_step_matches_float64(rows, I, H):
    from ivln_ce_amd import ops

    c, r64, r32 = _case(1, rows, I, H)
    assert rows == 1 or (int(c["masks"].min()) == 0 and int(c["masks"].max()) == 1)
    w = _dev_weights(c)
    masks = c["masks"].view(rows).to(DEV)
    x = c["x"][0].to(DEV)
    gi = F.linear(c["x"][0], c["w_ih"], c["b_ih"]).to(DEV)
    chk = _Check(f"lstm_step rows={rows} I={I} H={H}")
    for slots in (2, 4):  # row stride 2H and 4H
        for path in ("x", "gi_pre"):
            h_in, c_in = _state_slices(c, slots)
            out, wide = _strided_out(rows, H)
            state = torch.full((rows, 2, H), float("nan"), device=DEV)
            saves = tuple(torch.full((rows, H), float("nan"), device=DEV) for _ in range(5))
            ops.lstm_step(x if path == "x" else None, gi if path == "gi_pre" else None, h_in, c_in, masks, w["w_ih"], w["w_hh"],
                          w["b_ih"], w["b_hh"], out, state[:, 1], state[:, 0], saves)
            tag = f"{path}/{slots}H:"
            chk.close(tag + "h", out, r64["out"][0], r32["out"][0], 2e-5)
            chk.close(tag + "h2", state[:, 0], r64["hT"], r32["hT"], 2e-5)
            chk.close(tag + "c", state[:, 1], r64["cT"], r32["cT"], 2e-5)
            for k, nm in enumerate("ifgoc"):
                chk.close(tag + "s_" + nm, saves[k], r64["saves"][k][0], r32["saves"][k][0], 2e-5)
            assert _same_bytes(out, state[:, 0]), "the two output pointers hold different values"
            assert float((wide[:, :4] - 7.0).abs().max()) == 0.0 and float((wide[:, 4 + H:] - 7.0).abs().max()) == 0.0
    chk.done()


def test_lstm_entry_points_refuse_a_hidden_size_that_is_no_multiple_of_four():
    from ivln_ce_amd import ops
    from ivln_ce_amd._lib import IvlnError

    H, N, I = 6, 2, 8
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    m = torch.ones(N, dtype=torch.uint8, device=DEV)
    sv = tuple(z(N, H) for _ in range(5))
    with pytest.raises(IvlnError, match=r"\(%d\)" % E_INVALID):
        ops.lstm_step(z(N, I), None, z(N, H), z(N, H), m, z(4 * H, I), z(4 * H, H), z(4 * H), z(4 * H), z(N, H), z(N, H))
    with pytest.raises(IvlnError, match=r"\(%d\)" % E_INVALID):
        ops.lstm_seq(z(N, 4 * H), z(N, H), z(N, H), m, z(4 * H, H), z(4 * H), z(N, H), z(N, H), z(N, H), 1, N)
    with pytest.raises(IvlnError, match=r"\(%d\)" % E_INVALID):
        ops.lstm_seq_bwd(z(N, H), sv, z(N, H), z(N, H), z(N, H), m, z(H, 4 * H), 1, N, z(N, 4 * H), z(N, H), z(N, H), z(N, H))
    with pytest.raises(IvlnError, match=r"\(%d\)" % E_INVALID):  # both input forms at once
        ops.lstm_step(z(N, I), z(N, 32), z(N, 8), z(N, 8), m, z(32, I), z(32, 8), z(32), z(32), z(N, 8), z(N, 8))


# ------------------------------------------------------------------------------------------------------------------
# 2. / 3. the sequence and its BPTT
# ------------------------------------------------------------------------------------------------------------------
def _seq_forward(ops, c, w, saves=True):
    T, N, I, H = c["T"], c["N"], c["I"], c["H"]
    R = T * N
    gi = ops.linear_gemm(c["x"].reshape(R, I).to(DEV), w["w_ih"], w["b_ih"])  # the caller's GEMM (LSTMStateEncoder.forward)
    h0, c0 = _state_slices(c, 4)
    out, wide = _strided_out(R, H)
    state = torch.full((N, 2, H), float("nan"), device=DEV)
    sv = tuple(torch.full((R, H), float("nan"), device=DEV) for _ in range(5)) if saves else None
    masks = c["masks"].reshape(R).to(DEV)
    ops.lstm_seq(gi, h0, c0, masks, w["w_hh"], w["b_hh"], out, state[:, 0], state[:, 1], T, N, sv)
    return dict(gi=gi, h0=h0, c0=c0, out=out, wide=wide, state=state, saves=sv, masks=masks)


SEQ_SHAPES = [(1, 2, 64), (5, 3, 128), (4, 8, 512), (3, 9, 64)]   # (N = 9: a second pass of the step kernel, one live row)


@pytest.mark.parametrize("T,N,H", SEQ_SHAPES)
def test_lstm_sequence_matches_float64_and_the_step_kernel(T, N, H):
    from ivln_ce_amd import ops

    c, r64, r32 = _case(T, N, I_OF_H[H], H)
    m = c["masks"]
    assert int(m[0].min()) == 0 and int(m.max()) == 1 and (T == 1 or int(m[1:].min()) == 0)
    w = _dev_weights(c)
    f = _seq_forward(ops, c, w)
    chk = _Check(f"lstm_seq T={T} N={N} H={H}")
    chk.close("out", f["out"], r64["out"], r32["out"], 1e-5)
    chk.close("hT", f["state"][:, 0], r64["hT"], r32["hT"], 1e-5)
    chk.close("cT", f["state"][:, 1], r64["cT"], r32["cT"], 1e-5)
    for k, nm in enumerate("ifgoc"):
        chk.close("s_" + nm, f["saves"][k], r64["saves"][k], r32["saves"][k], 1e-5)
    assert float((f["wide"][:, :4] - 7.0).abs().max()) == 0.0 and float((f["wide"][:, 4 + H:] - 7.0).abs().max()) == 0.0
    # the same sequence as T calls of the step: the same kernel on the same operands, bit for bit
    out2, _ = _strided_out(T * N, H)
    state2 = torch.full((N, 2, H), float("nan"), device=DEV)
    sv2 = tuple(torch.full((T * N, H), float("nan"), device=DEV) for _ in range(5))
    for t in range(T):
        sl = slice(t * N, (t + 1) * N)
        h_in = f["h0"] if t == 0 else out2[(t - 1) * N:t * N]
        c_in = f["c0"] if t == 0 else state2[:, 1]
        ops.lstm_step(None, f["gi"][sl], h_in, c_in, f["masks"][sl], None, w["w_hh"], None, w["b_hh"], out2[sl], state2[:, 1],
                      state2[:, 0] if t == T - 1 else None, tuple(s[sl] for s in sv2))
    assert _same_bytes(out2, f["out"]) and _same_bytes(state2, f["state"])
    for a, b in zip(sv2, f["saves"]):
        assert _same_bytes(a, b)
    # without saves: the same outputs
    g = _seq_forward(ops, c, w, saves=False)
    assert _same_bytes(g["out"], f["out"]) and _same_bytes(g["state"], f["state"])
    chk.done()


@pytest.mark.parametrize("T,N,H", SEQ_SHAPES)
def test_lstm_sequence_backward_matches_float64_autograd(T, N, H):
    from ivln_ce_amd import ops

    I = I_OF_H[H]
    c, r64, r32 = _case(T, N, I, H)
    R = T * N
    w = _dev_weights(c)
    f = _seq_forward(ops, c, w)
    whh_t = ops.transpose(w["w_hh"])
    x2d = c["x"].reshape(R, I).to(DEV)

    def backward(d_out_cpu):
        d_out, _ = _strided_out(R, H)
        d_out.copy_(d_out_cpu.reshape(R, H).to(DEV))
        dgi = torch.full((R, 4 * H), float("nan"), device=DEV)
        hp = torch.full((R, H), float("nan"), device=DEV)
        d0 = torch.full((N, 2, H), float("nan"), device=DEV)
        ops.lstm_seq_bwd(d_out, f["saves"], f["out"], f["h0"], f["c0"], f["masks"], whh_t, T, N, dgi, hp, d0[:, 0], d0[:, 1])
        return dgi, hp, d0

    dgi, hp, d0 = backward(c["d_out"])
    chk = _Check(f"lstm_bptt T={T} N={N} H={H}")
    chk.bar("dgi", dgi, r64["dgi"], r32["dgi"])
    chk.bar("hp", hp, r64["hp"], r32["hp"])
    chk.bar("dh0", d0[:, 0], r64["dh0"], r32["dh0"])
    chk.bar("dc0", d0[:, 1], r64["dc0"], r32["dc0"])
    # the weight / bias / input gradients are the existing GEMM-shaped gradients and column sums over dgi (train._lstm_backward)
    db = ops.colsum(dgi)
    chk.bar("dW_ih", ops.linear_bwd_weight(dgi, x2d), r64["dw_ih"], r32["dw_ih"])
    chk.bar("dW_hh", ops.linear_bwd_weight(dgi, hp), r64["dw_hh"], r32["dw_hh"])
    chk.bar("db_ih", db, r64["db_ih"], r32["db_ih"])
    chk.bar("db_hh", db, r64["db_hh"], r32["db_hh"])
    chk.bar("dx", ops.linear_bwd_input(dgi, w["w_ih"]), r64["dx"], r32["dx"])
    # a step whose mask is 0 sends exactly zero into the previous state
    m = c["masks"]
    for n in range(N):
        zero = float(d0[n].abs().max()) == 0.0
        assert zero == (int(m[0, n]) == 0), f"row {n}: mask {int(m[0, n])} at t = 0, d(h0, c0) {'zero' if zero else 'not zero'}"
        assert float(r64["dh0"][n].abs().max()) == 0.0 if int(m[0, n]) == 0 else True
    if T > 1:
        # ... and in the middle: with upstream gradient only from the masked step on, nothing arrives in front of it
        t0, n0 = T // 2, min(1, N - 1)
        assert int(m[t0, n0]) == 0
        late = c["d_out"].clone()
        late[:t0, n0] = 0.0
        dgi2, _, d02 = backward(late)
        front = dgi2.view(T, N, 4 * H)[:t0, n0]
        assert float(front.abs().max()) == 0.0, "gradient crossed a masked step"
        assert float(d02[n0].abs().max()) == 0.0
        assert float(dgi2.view(T, N, 4 * H)[t0:, n0].abs().max()) > 0.0
        if N > 2:  # an unmasked row does pass it on
            assert float(dgi.view(T, N, 4 * H)[:t0, 2].abs().max()) > 0.0
    chk.done()


# ------------------------------------------------------------------------------------------------------------------
# 4. policy steps, 6. graph replay
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
        obs.append({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in o.items()})
    return obs


@pytest.mark.parametrize("rnn_type", ["LSTM", "GRU"])
def test_policy_steps_match_the_oracle_and_only_gru_takes_the_fused_head(rnn_type, monkeypatch):
    from det_init import det_fill

    from ivln_ce_amd import ops
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.obs_transforms import GTSemanticsIterativeMapper
    from oracle.policy_ref import MapCMAPolicyRef

    torch.set_num_threads(8)
    B, L = 2, 4 if rnn_type == "LSTM" else 2
    pol = make_policy(rnn_type).to(DEV).eval()
    assert pol.net.num_recurrent_layers == L
    if rnn_type == "LSTM":
        ref = MapCMAPolicyLSTMRef().eval()
        ref.load_state_dict({k: v.cpu() for k, v in pol.state_dict().items()})
    else:
        ref = det_fill(MapCMAPolicyRef(), seed=0).eval()
    fused = []
    real = ops.cma_step
    monkeypatch.setattr(ops, "cma_step", lambda d: (fused.append(1), real(d))[1])
    feats = {}
    pol.net.register_forward_hook(lambda mod, args, o: feats.__setitem__("f", o[0]))
    tr = GTSemanticsIterativeMapper.from_config(get_config())
    g = torch.Generator().manual_seed(3)
    rnn = 0.1 * torch.randn(B, L, 512, generator=g)  # (dropped by the first step's mask: every episode starts there)
    rnn_r, rnn_d = rnn.clone(), rnn.to(DEV)
    prev = torch.zeros(B, 1, dtype=torch.long)
    log = []
    for t, o in enumerate(_rollout_obs(B, 3, seed=77, reset=(1, 1))):
        b = tr(dict(o))
        masks = b["not_done_masks"]
        assert masks.view(-1).tolist() == [[0, 0], [1, 0], [1, 1]][t]
        with torch.no_grad():
            a, rnn_d = pol.act(b, rnn_d, prev.to(DEV), masks, deterministic=True)
            lg = pol.action_distribution.raw_logits(feats["f"])
            cpu = {k: b[k].cpu() for k in ("depth", "occupancy_map", "semantic_map", "instruction")}
            lr, rnn_r, fr = ref.logits(cpu, rnn_r, prev, masks.cpu())
        assert tuple(rnn_d.shape) == (B, L, 512)
        e_l, e_f = float((lg.cpu() - lr).abs().max()), float((feats["f"].cpu() - fr).abs().max())
        e_s = [float((rnn_d[:, k].cpu() - rnn_r[:, k]).abs().max()) for k in range(L)]
        log.append(f"{rnn_type} step {t}: logits {e_l:.3e} features {e_f:.3e} state slots " + " ".join(f"{e:.3e}" for e in e_s))
        _log(log[-1])
        assert e_l < 1e-4 and e_f < 2e-4 and max(e_s) < 2e-4, "\n".join(log)
        # (logits 1e-4 apart: the action taken is the oracle's arg-max up to a tie within twice that)
        assert float((lr.max(-1, keepdim=True).values - lr.gather(1, a.cpu())).max()) < 2e-4
        prev = a.cpu()
    assert len(fused) == (3 if rnn_type == "GRU" else 0), f"{rnn_type}: ivln_cma_step_fwd ran {len(fused)} times in 3 steps"


def test_graph_replay_of_the_lstm_policy_is_bit_identical_to_eager(same_depth_path):
    same_depth_path(0)
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.graphed import GraphedRollout
    from ivln_ce_amd.obs_transforms import GTSemanticsIterativeMapper

    B, steps = 2, 5
    pol = make_policy("LSTM").to(DEV).eval()
    cfg = get_config()
    obs = _rollout_obs(B, steps, seed=31, reset=(3, 0))
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
    assert float(eager[-1][1][:, 1].abs().max()) > 0 and float(eager[-1][1][:, 3].abs().max()) > 0  # both cell states live
    tr_g = GTSemanticsIterativeMapper.from_config(cfg)
    runner = GraphedRollout(pol, [tr_g], obs[0], deterministic=True)
    tr_g.mapping_module.reset()
    runner.reset_state()
    for t, o in enumerate(obs):
        a = runner.step(o)
        torch.cuda.synchronize()
        assert tuple(runner.rnn_states.shape) == (B, 4, 512)
        assert torch.equal(a, eager[t][0]), f"actions step {t}"
        assert torch.equal(runner.rnn_states, eager[t][1]), f"rnn step {t}"
    tr_g.mapping_module.check_status()


# ------------------------------------------------------------------------------------------------------------------
# 5. one update
# ------------------------------------------------------------------------------------------------------------------
def test_update_gradients_of_the_lstm_policy_match_float64_autograd():
    """`update_agent` at T = 4, N = 2 (one trajectory a step shorter, one episode restart in the middle) with
    STATE_ENCODER.rnn_type LSTM: the gradient of EVERY trainable tensor against float64 autograd of the oracle's loss.
    Per tensor: max |got - ref| <= 1e-3 * max |ref| + 2e-7, and the direction cosine >= 1 - 1e-6."""
    from ivln_ce_amd.aux_losses import AuxLosses
    from ivln_ce_amd.trainers import FlatAdam, update_agent
    from ivln_ce_amd.utils import dedupe_instructions, trim_instruction_padding

    torch.set_num_threads(8)
    T, N = 4, 2
    TN = T * N
    g = torch.Generator().manual_seed(42)
    lens = [4, 3]
    instr = torch.zeros(N, 200)
    for n in range(N):
        instr[n, :30 - 9 * n] = torch.randint(2, 2504, (30 - 9 * n,), generator=g).float()
    obs = {"depth_features": torch.randn(TN, 128, 4, 4, generator=g),
           "occupancy_map": (torch.rand(TN, 64, 64, generator=g) < 0.3).float(),
           "semantic_map": torch.randint(0, 13, (TN, 64, 64), generator=g).float(),
           "instruction": instr.repeat(T, 1), "progress": torch.rand(TN, 1, generator=g)}
    prev = torch.randint(0, 4, (TN, 1), generator=g)
    nd = torch.ones(T, N, dtype=torch.uint8)
    nd[0] = 0
    nd[2, 0] = 0
    nd = nd.view(-1, 1)
    tgt = torch.randint(0, 4, (T, N), generator=g)
    w = torch.where(torch.rand(T, N, generator=g) < 0.5, torch.tensor(3.2), torch.tensor(1.0))
    for n, Ln in enumerate(lens):  # collate_fn's padding of a finished trajectory (dagger_trainer.py:66-70)
        w[Ln:, n] = 0
        tgt[Ln:, n] = 0
        for k in obs:
            obs[k].view(T, N, *obs[k].shape[1:])[Ln:, n] = 1.0
        prev.view(T, N)[Ln:, n] = 0

    pol = make_policy("LSTM", use_pm=True).to(DEV).train()
    ref = MapCMAPolicyLSTMRef(use_pm=True)
    ref.load_state_dict({k: v.cpu() for k, v in pol.state_dict().items()})
    ref = ref.train().double()
    obs64 = {k: v.double() for k, v in obs.items()}
    torch.set_default_dtype(torch.float64)  # (tensors the oracle creates itself: initial state, one-hot maps)
    try:
        loss_r, act_r, aux_r, _ = ref.update_loss(obs64, prev, nd, tgt, w.double())
        loss_r.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    loss_r, aux_r = float(loss_r.detach()), float(aux_r.detach())
    grads = {k: p.grad.detach() for k, p in ref.named_parameters() if p.grad is not None}

    opt = FlatAdam(pol, lr=2.5e-4)
    dobs = dedupe_instructions(trim_instruction_padding(dict(obs), first_rows=N))
    dobs = {k: v.to(DEV) for k, v in dobs.items()}
    AuxLosses.activate()
    try:
        loss, act, aux = update_agent(pol, opt, dobs, prev.to(DEV), nd.to(DEV), tgt.to(DEV), w.to(DEV), hidden_size=512,
                                      step_grad=False)
    finally:
        AuxLosses.deactivate()
    _log(f"lstm update T={T} N={N}: loss {loss:.7f} ref {loss_r:.7f}  aux {aux:.7f} ref {aux_r:.7f}")
    assert abs(loss - loss_r) < 2e-5 and abs(aux - aux_r) < 2e-5, (loss, loss_r, aux, aux_r)
    params = dict(pol.named_parameters())
    must = [f"net.{e}.rnn.{p}_l0" for e in ("state_encoder", "second_state_encoder")
            for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    assert all(k in params and params[k].requires_grad and k in grads for k in must)
    zero_bias = lambda k: k.startswith("net.map_encoder.cnn.") and k.endswith(".conv.0.bias")  # noqa: E731
    log, bad = [], []
    for k, p in params.items():
        if not p.requires_grad or k not in grads:
            continue
        got, want = p.grad.detach().cpu().double().reshape(-1), grads[k].double().reshape(-1)
        if zero_bias(k):  # a conv bias in front of a train-mode BatchNorm: analytically zero, exact 0 here
            assert float(got.abs().max()) == 0.0, k
            continue
        scale = float(want.abs().max())
        err = float((got - want).abs().max())
        cos = float(torch.dot(got, want) / (got.norm() * want.norm()).clamp_min(1e-300)) if scale > 0 else 1.0
        log.append(f"{k}: max|ref| {scale:.3e} max|err| {err:.3e} cos-1 {cos - 1:.1e}")
        _log("lstm update " + log[-1])
        if not (err <= 1e-3 * scale + 2e-7 and (cos >= 1 - 1e-6 or scale < 1e-6)):
            bad.append(log[-1])
    assert not bad, "\n".join(bad)
    assert all(any(line.startswith(k + ":") for line in log) for k in must)
