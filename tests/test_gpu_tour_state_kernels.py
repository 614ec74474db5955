"""GPU: ivln_lstm_seq_tour_fwd_f32 alone (include/ivln_tour_state.h, csrc/state_rnn.hip k_rnn_step_tour): the masked LSTM
step with Latent-CMA's tour-long memory updated inside it, T dependent launches from one C call, against the same loop in
float64 torch on the CPU.

Cases (T, N, H, I0): (1, 1, 64, 32) a single row and step; (3, 3, 64, 32) 64 lanes per row; (2, 9, 64, 30) 32 lanes per
row, a second pass that is partly empty and the 4-byte load form (I0 = 30: neither the memory segment of W_ih nor the row
stride I0 + H allows 16-byte loads); (3, 5, 512, 416) the product's widths.  Masks: an episode reset inside a tour, a tour
reset mid-sequence, t = 0 with tour mask 0; memory and h of both signs; state views with the strides of (N, 5, H).

Bars: out, c, the final h and the saves  err <= 4 * e32 + 4 * 2^-24 * max|ref|  (tests/test_gpu_instruction_options._Bar:
e32 is the float32 torch loop's own error).  mem_in / mem_state_out involve no arithmetic: they equal, exactly, the mask /
max of the kernel's OWN out rows.  Every comparison is printed before anything is asserted."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
SENT = 1234.5
CASES = [(1, 1, 64, 32), (3, 3, 64, 32), (2, 9, 64, 30), (3, 5, 512, 416)]


class _Bar:
    """tests/test_gpu_instruction_options._Bar: everything is printed before anything is asserted."""

    def __init__(self, case):
        self.case, self.bad = case, []

    def check(self, name, got, ref64, ref32, factor=4.0):
        got = got.detach().cpu().double().reshape(-1)
        r64, r32 = ref64.detach().double().reshape(-1), ref32.detach().double().reshape(-1)
        assert got.shape == r64.shape == r32.shape, (name, got.shape, r64.shape, r32.shape)
        err, e32, mx = float((got - r64).abs().max()), float((r32 - r64).abs().max()), float(r64.abs().max())
        bar = factor * e32 + 4 * EPS * mx
        ok = err <= bar  # (False for NaN)
        line = f"{self.case:26s} {name:12s} hip {err:.3e}  e32 {e32:.3e}  max|ref| {mx:.3e}  bar {bar:.3e}  {'ok' if ok else 'OVER'}"
        print(line)
        if not ok:
            self.bad.append(line)

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def _masks(T, N):
    """(ep, tour) u8 (T, N).  Row 1 at t = 0 starts a tour (both 0), odd rows from 3 on start an episode inside their tour
    at t = 0; t = 1: row 0 starts an episode INSIDE its tour (ep 0, tour 1), row 1 starts a tour mid-sequence; t = 2: the
    last row starts an episode."""
    ep, tour = torch.ones(T, N, dtype=torch.uint8), torch.ones(T, N, dtype=torch.uint8)
    if N > 1:
        ep[0, 1] = tour[0, 1] = 0
        ep[0, 3::2] = 0
    if T > 1:
        ep[1, 0] = 0
        if N > 1:
            ep[1, 1] = tour[1, 1] = 0
    if T > 2:
        ep[2, N - 1] = 0
    return ep, tour


def _inputs(T, N, H, I0):
    g = torch.Generator().manual_seed(7000 + 100 * T + 10 * N + H + I0)
    r = lambda *s, k=1.0: torch.randn(*s, generator=g) * k  # noqa: E731
    ep, tour = _masks(T, N)
    return dict(gi=r(T * N, 4 * H, k=0.6), w_ih=r(4 * H, I0 + H, k=0.07), w_hh=r(4 * H, H, k=0.07), b_hh=r(4 * H, k=0.1),
                state=r(N, 5, H, k=0.5), ep=ep, tour=tour)


def _loop(inp, T, N, H, I0, dt):
    """the semantics of include/ivln_tour_state.h written out in torch on the CPU"""
    gi, wm, whh, bhh = inp["gi"].to(dt), inp["w_ih"][:, I0:].to(dt), inp["w_hh"].to(dt), inp["b_hh"].to(dt)
    st = inp["state"].to(dt)
    h, c, m = st[:, 0], st[:, 1], st[:, 4]
    res = {k: [] for k in ("out", "mem_in", "i", "f", "g", "o", "c")}
    for t in range(T):
        e, k = inp["ep"][t].to(dt).view(N, 1), inp["tour"][t].to(dt).view(N, 1)
        m = (m if t == 0 else torch.max(m, h)) * k
        gates = gi[t * N:(t + 1) * N] + m @ wm.T + (h * e) @ whh.T + bhh
        i, f, gg, o = torch.sigmoid(gates[:, :H]), torch.sigmoid(gates[:, H:2 * H]), torch.tanh(gates[:, 2 * H:3 * H]), \
            torch.sigmoid(gates[:, 3 * H:])
        c = f * (c * e) + i * gg
        h = o * torch.tanh(c)
        for name, v in (("out", h), ("mem_in", m), ("i", i), ("f", f), ("g", gg), ("o", o), ("c", c)):
            res[name].append(v)
    res = {k: torch.cat(v, 0) for k, v in res.items()}
    res["mem_state"] = torch.max(m, h)
    return res


_refs = {}


def _ref(case):
    if case not in _refs:
        inp = _inputs(*case)
        _refs[case] = (inp, _loop(inp, *case, torch.float64), _loop(inp, *case, torch.float32))
    return _refs[case]


class _Dev:
    """Device operands laid out as the policy lays them out: the incoming and the outgoing state are (N, 5, H) tensors
    [h1, c1, h2, c2, memory]; out is the first H columns of a wider row (x2), mem_in the LAST H columns of the encoder's
    (T*N, I0 + H) input; each save sits between two guard rows.  Every output buffer starts as a sentinel."""

    def __init__(self, inp, T, N, H, I0):
        self.T, self.N, self.H, self.I0 = T, N, H, I0
        d = lambda t: t.to(DEV).contiguous()  # noqa: E731
        self.gi, self.w_ih, self.w_hh, self.b_hh, self.state = (d(inp[k]) for k in ("gi", "w_ih", "w_hh", "b_hh", "state"))
        self.ep, self.tour = d(inp["ep"].view(-1)), d(inp["tour"].view(-1))
        full = lambda *s: torch.full(s, SENT, dtype=torch.float32, device=DEV)  # noqa: E731
        self.x2, self.state_in, self.state_out = full(T * N, H + 8), full(T * N, I0 + H), full(N, 5, H)
        self.sv = full(5, T * N + 2, H)
        self.out, self.mem_in = self.x2[:, :H], self.state_in[:, I0:]
        self.saves = tuple(self.sv[k, 1:-1] for k in range(5))

    def run(self):
        from ivln_ce_amd import ops

        so = self.state_out
        ops.lstm_seq_tour(self.gi, self.w_ih, self.w_hh, self.b_hh, self.state[:, 0], self.state[:, 1], self.state[:, 4],
                          self.ep, self.tour, self.out, self.mem_in, so[:, 0], so[:, 1], so[:, 4], self.T, self.N, self.saves)
        torch.cuda.synchronize()
        return self

    def raw(self, **over):
        """the C entry called directly with some arguments replaced -> its return code"""
        from ivln_ce_amd import ops

        so, st = self.state_out, self.state
        a = dict(gi_base=self.gi, w_ih=self.w_ih, I0=self.I0, w_hh=self.w_hh, b_hh=self.b_hh, h0=st[:, 0], ld_h0=None,
                 c0=st[:, 1], ld_c0=None, mem0=st[:, 4], ld_m0=None, ep=self.ep, tour=self.tour, out=self.out, ldo=None,
                 mem_in=self.mem_in, ld_mi=None, h_so=so[:, 0], ld_hs=None, c_so=so[:, 1], ld_cs=None, m_so=so[:, 4],
                 ld_ms=None, T=self.T, N=self.N, H=self.H, s0=self.saves[0], s1=self.saves[1], s2=self.saves[2],
                 s3=self.saves[3], s4=self.saves[4])
        a.update(over)
        for ld, of in (("ld_h0", "h0"), ("ld_c0", "c0"), ("ld_m0", "mem0"), ("ldo", "out"), ("ld_mi", "mem_in"),
                       ("ld_hs", "h_so"), ("ld_cs", "c_so"), ("ld_ms", "m_so")):
            if a[ld] is None:
                a[ld] = a[of].stride(0) if a[of] is not None else 0
        vals = [v.data_ptr() if torch.is_tensor(v) else v for v in a.values()]
        rc = ops._L().ivln_lstm_seq_tour_fwd_f32(*vals, None)
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        return [self.x2, self.state_in, self.state_out, self.sv]

    def untouched(self):
        return all(bool((t == SENT).all()) for t in self.outputs())


@pytest.mark.parametrize("case", CASES, ids=lambda c: "T%d-N%d-H%d-I%d" % c)
def test_tour_step_sequence_matches_float64(case):
    T, N, H, I0 = case
    inp, r64, r32 = _ref(case)
    dv = _Dev(inp, *case)
    assert dv.untouched()
    dv.run()
    out, mem_in, so = dv.out.cpu(), dv.mem_in.cpu(), dv.state_out.cpu()
    sv = [s.cpu() for s in dv.saves]
    bar = _Bar("T=%d N=%d H=%d I0=%d" % case)
    bar.check("out", out, r64["out"], r32["out"])
    for k, name in enumerate(("i", "f", "g", "o", "c")):
        bar.check("save_" + name, sv[k], r64[name], r32[name])
    bar.check("h_state", so[:, 0], r64["out"][-N:], r32["out"][-N:])
    bar.check("c_state", so[:, 1], r64["c"][-N:], r32["c"][-N:])
    # the memory: no arithmetic - exactly the mask / max of the kernel's own rows
    keep = inp["tour"].view(T, N, 1) != 0
    zero = torch.zeros(N, H)
    for t in range(T):
        src = inp["state"][:, 4] if t == 0 else torch.max(mem_in[(t - 1) * N:t * N], out[(t - 1) * N:t * N])
        want = torch.where(keep[t], src, zero)
        same = torch.equal(mem_in[t * N:(t + 1) * N], want)
        print(f"{bar.case:26s} mem_in[t={t}] exact: {same}")
        if not same:
            bar.bad.append(f"mem_in of step {t} is not the mask / max of the rows before it")
    exact = {"mem_state_out": torch.equal(so[:, 4], torch.max(mem_in[-N:], out[-N:])),
             "h_state_out == out[T-1]": torch.equal(so[:, 0], out[-N:]),
             "c_state_out == save_c[T-1]": torch.equal(so[:, 1], sv[4][-N:])}
    for name, same in exact.items():
        print(f"{bar.case:26s} {name} exact: {same}")
        if not same:
            bar.bad.append(name)
    # (the float64 memory agrees too, up to the error of the h it is pooled with)
    bar.check("mem_in", mem_in, r64["mem_in"], r32["mem_in"])
    bar.check("mem_state", so[:, 4], r64["mem_state"], r32["mem_state"])
    # untouched sentinels around every output
    guards = {"x2 beyond H": dv.x2[:, H:], "state_in before I0": dv.state_in[:, :I0], "state_out h2 / c2": dv.state_out[:, 2:4],
              "save guard rows": dv.sv[:, [0, -1]]}
    for name, gd in guards.items():
        if not bool((gd == SENT).all()):
            bar.bad.append(f"sentinel overwritten: {name}")
    # the masks decided something: both signs met in the max, and a reset row really is zero
    pooled = torch.max(mem_in[-N:], out[-N:])
    assert bool((pooled == mem_in[-N:]).any()) and bool((pooled == out[-N:]).any())
    if N > 1:
        assert bool((mem_in[1] == 0).all())
    bar.done()
    # two runs: identical bytes
    dv2 = _Dev(inp, *case).run()
    for a, b in zip(dv.outputs(), dv2.outputs()):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_tour_step_without_saves_and_final_h_gives_the_same_bytes():
    """saves and h_state_out are optional: without them the other outputs are the same bytes and nothing else is written"""
    from ivln_ce_amd import ops

    case = CASES[1]
    inp = _ref(case)[0]
    T, N = case[0], case[1]
    a, b = _Dev(inp, *case).run(), _Dev(inp, *case)
    ops.lstm_seq_tour(b.gi, b.w_ih, b.w_hh, b.b_hh, b.state[:, 0], b.state[:, 1], b.state[:, 4], b.ep, b.tour, b.out,
                      b.mem_in, None, b.state_out[:, 1], b.state_out[:, 4], T, N, None)
    torch.cuda.synchronize()
    assert torch.equal(a.x2, b.x2) and torch.equal(a.state_in, b.state_in)
    assert torch.equal(a.state_out[:, 1:], b.state_out[:, 1:])
    assert bool((b.state_out[:, 0] == SENT).all()) and bool((b.sv == SENT).all())


def test_tour_step_refuses_overlaps_and_bad_sizes():
    from ivln_ce_amd import ops
    from ivln_ce_amd._lib import IvlnError

    case = CASES[1]
    T, N, H, I0 = case
    dv = _Dev(_ref(case)[0], *case)
    so, st = dv.state_out, dv.state
    bad = {
        "h0 is a slot of the outgoing state": dict(h0=so[:, 0]),
        "mem0 is a slot of the outgoing state": dict(mem0=so[:, 4]),
        "h0 inside out": dict(h0=dv.out[:N]),
        "mem0 inside mem_in": dict(mem0=dv.mem_in[N:2 * N]),
        "h0 inside a save": dict(h0=dv.saves[2][:N]),
        "c0 inside the outgoing h slot": dict(c0=so[:, 0]),
        "T = 0": dict(T=0), "N = 0": dict(N=0), "H = 0": dict(H=0), "H not a multiple of 4": dict(H=H - 2),
        "I0 = 0": dict(I0=0), "row stride below H": dict(ldo=H - 4), "memory stride below H": dict(ld_mi=1),
        "NULL out": dict(out=None), "NULL mem0": dict(mem0=None), "NULL tour masks": dict(tour=None),
        "NULL c_state_out": dict(c_so=None), "NULL mem_state_out": dict(m_so=None), "partial saves": dict(s3=None),
    }
    failed = []
    for name, over in bad.items():
        rc = dv.raw(**over)
        print(f"{name:40s} rc {rc}  outputs untouched {dv.untouched()}")
        if rc != -1 or not dv.untouched():
            failed.append(name)
    assert not failed, failed
    # the Python binding checks shapes before the call
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    m = torch.ones(N, dtype=torch.uint8, device=DEV)
    good = dict(gi_base=z(N, 4 * H), w_ih=z(4 * H, I0 + H), w_hh=z(4 * H, H), b_hh=z(4 * H), h0=z(N, H), c0=z(N, H),
                mem0=z(N, H), ep_masks_u8=m, tour_masks_u8=m, out=z(N, H), mem_in=z(N, H), h_state_out=z(N, H),
                c_state_out=z(N, H), mem_state_out=z(N, H), T=1, N=N)
    ops.lstm_seq_tour(**good)
    for k, v in (("gi_base", z(N, 3 * H)), ("w_ih", z(4 * H, H)), ("mem0", z(N, H + 4)), ("out", z(N + 1, H)),
                 ("tour_masks_u8", m[:1]), ("ep_masks_u8", m.float()), ("saves", tuple(z(N + 1, H) for _ in range(5)))):
        with pytest.raises(IvlnError, match="lstm_seq_tour"):
            ops.lstm_seq_tour(**{**good, k: v})
    # c0 may BE c_state_out: the cell state advanced in place
    dv3 = _Dev(_ref(case)[0], *case)
    ref = _Dev(_ref(case)[0], *case).run()
    c = dv3.state[:, 1].clone()
    assert dv3.raw(c0=c, c_so=c) == 0
    assert torch.equal(dv3.x2, ref.x2) and torch.equal(c, ref.state_out[:, 1])
    assert torch.equal(dv3.state_out[:, [0, 4]], ref.state_out[:, [0, 4]]) and bool((dv3.state_out[:, 1] == SENT).all())
