"""GPU: the instruction encoder's options - `MODEL.INSTRUCTION_ENCODER.rnn_type` GRU | LSTM, `bidirectional` True | False
(instruction_encoder.py:27-32, 49).  The recurrences alone (csrc/instr_rnn.hip k_gru_dirs / k_gru_dirs_bwd, and
k_lstm_bidir / k_lstm_bidir_bwd with one direction) against float64 torch.nn.GRU / nn.LSTM on packed sequences, the
LSTM's launch forms (plain, ticket + spare, step cache) byte for byte against each other, then the MapCMA policy built
with every non-default combination, and Latent-CMA with (GRU, bidirectional) and (LSTM, unidirectional): rollout step,
distribution over T = 3, one update's gradients, hipGraph replay.

Bounds (none derived from what the kernels give):
  forward   2e-5 absolute + 1e-4 relative: tests/test_gpu_kernels.py::test_lstm_bidir_matches_packed_torch_lstm (values in [-1, 1])
  backward  err <= 4 * e32 + 4 * 2^-24 * max|ref|, e32 = the float32 torch run's error against its float64 run:
            tests/test_gpu_train_kernels.py::_Bar.check with factor 4
  policy    logits 1e-4, features / states 2e-4: tests/test_gpu_policy.py, tests/test_gpu_lstm_state.py
            (tests/test_gpu_latent.py holds the same two figures for Latent-CMA)
Every comparison is printed before anything is asserted.
"""
import functools
import types

import pytest
import torch

from instr_rnn_ref import (NON_DEFAULT, LatentCMAPolicyOptRef, gru_cell_loop, make_case, make_policy, mapcma_oracle,
                           module_ref)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
H = 128
CASES = [(1, 1, (1,)), (3, 5, (5, 7, 1)), (3, 5, (3, 0, 5)), (4, 37, (37, 5, 20, 1))]
KERNELS = [("GRU", 1), ("GRU", 2), ("LSTM", 1)]


class _Bar:
    """Collects the comparisons of one case: everything is printed before anything is asserted."""

    def __init__(self, case):
        self.case, self.bad = case, []

    def check(self, name, got, ref64, ref32, factor=4.0):
        got = got.detach().cpu().double().reshape(-1)
        r64 = ref64.detach().double().reshape(-1)
        r32 = ref32.detach().double().reshape(-1)
        assert got.shape == r64.shape == r32.shape, (name, got.shape, r64.shape, r32.shape)
        err = float((got - r64).abs().max())
        e32 = float((r32 - r64).abs().max())
        mx = float(r64.abs().max())
        bar = factor * e32 + 4 * EPS * mx
        ok = err <= bar  # (False for NaN)
        line = f"{self.case:44s} {name:34s} hip {err:.3e}  e32 {e32:.3e}  max|ref| {mx:.3e}  bar {bar:.3e}  {'ok' if ok else 'OVER'}"
        print(line)
        if not ok:
            self.bad.append(line)

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def _same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _twice(fn):
    """fn() -> tuple of fresh fp32 output tensors; run twice, identical bytes required (fixed reduction orders)."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(a, b)):
        assert _same_bytes(x, y), f"output {i} differs between two runs on the same inputs"
    return a


# ------------------------------------------------------------------------------------------------------------------
# the recurrences alone
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(cell, ndir, B, L, lens):
    """computed once per case and shared by the forward and backward tests; never modified.  Length 0, which
    pack_padded_sequence refuses: the reference runs that row with length 1 and the row is left out of the comparison"""
    c = make_case(cell, ndir, B, L)
    eff = [min(n, L) for n in lens]
    ref_lens = [max(n, 1) for n in eff]
    args = (ndir, c["gx"], c["whh"], c["bhh"], ref_lens, c["dout"], B, L, H)
    r = dict(case=c, eff=eff, m64=module_ref(cell, *args, torch.float64), m32=module_ref(cell, *args, torch.float32))
    if cell == "GRU":
        r["l64"], r["l32"] = gru_cell_loop(*args, torch.float64), gru_cell_loop(*args, torch.float32)
    return r


def _forward(cell, ndir, c, lengths, B, L, save=False, cache=None):
    from ivln_ce_amd import ops

    d = [[t.to(DEV) for t in c[k]] + [None] for k in ("gx", "whh", "bhh")]
    a = (d[0][0], d[0][1], d[1][0], d[1][1], d[2][0], d[2][1], lengths, B, L, H)
    if cell == "GRU":
        return ops.gru_dirs(*a, ndir=ndir, save=save, cache=cache)
    out, gates, cs = ops.lstm_bidir(*a, ndir=ndir, save=save, cache=cache)
    return out, (gates, cs)


@pytest.mark.parametrize("B,L,lens", CASES)
@pytest.mark.parametrize("cell,ndir", KERNELS)
def test_forward_matches_the_packed_torch_module(cell, ndir, B, L, lens):
    r = _reference(cell, ndir, B, L, lens)
    c, eff = r["case"], r["eff"]
    lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
    out, _ = _forward(cell, ndir, c, lengths, B, L)
    assert tuple(out.shape) == (B, ndir * H, L)
    o = out.cpu()
    for b, n in enumerate(eff):
        assert bool((o[b, :, n:] == 0).all()), f"row {b}: positions >= {n} are not exactly zero"
    keep = torch.tensor([n > 0 for n in eff])
    ref = r["m64"]["out"][keep]
    d = (o[keep].double() - ref).abs()
    over = d - (2e-5 + 1e-4 * ref.abs())
    print(f"{cell} ndir={ndir} B={B} L={L} lens={lens}: max|err| {float(d.max()):.3e}  torch-fp32 "
          f"{float((r['m32']['out'][keep].double() - ref).abs().max()):.3e}  worst over-bound {float(over.max()):.3e}")
    assert float(over.max()) <= 0
    # the per-row cache: clean rows keep their bytes, dirty rows equal the uncached result byte for byte
    dirty = torch.tensor([1 - (b % 2) for b in range(B)], dtype=torch.int32, device=DEV)
    cache = types.SimpleNamespace(out=torch.full((B, ndir * H, L), 7.0, device=DEV), dirty=dirty)
    got, _ = _forward(cell, ndir, c, lengths, B, L, cache=cache)
    assert got is cache.out
    for b in range(B):
        if b % 2:
            assert bool((got[b] == 7.0).all()), f"clean row {b} was written"
        else:
            assert _same_bytes(got[b], out[b]), f"dirty row {b} differs from the uncached run"


@pytest.mark.parametrize("B,L,lens", CASES)
@pytest.mark.parametrize("cell,ndir", KERNELS)
def test_bptt_matches_float64_autograd(cell, ndir, B, L, lens):
    from ivln_ce_amd import ops

    r = _reference(cell, ndir, B, L, lens)
    c, eff = r["case"], r["eff"]
    lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
    out, sv = _forward(cell, ndir, c, lengths, B, L, save=True)
    dout = c["dout"].to(DEV)  # (non-zero at padded positions, where it must be ignored)
    whh = [t.to(DEV) for t in c["whh"]] + [None]
    if cell == "GRU":
        got = _twice(lambda: tuple(t for trip in ops.gru_dirs_bwd(dout, out, sv, whh[0], whh[1], lengths, B, L, H, ndir=ndir)
                                   for t in trip))
        per_dir = [dict(dgi=got[3 * d], dgh=got[3 * d + 1], hp=got[3 * d + 2]) for d in range(ndir)]
    else:
        got = _twice(lambda: tuple(t for t in ops.lstm_bidir_bwd(dout, out, sv[0], sv[1], whh[0], whh[1], lengths, B, L, H,
                                                                 ndir=ndir) if t is not None))
        per_dir = [dict(dgi=got[0], hp=got[1])]
    keep = torch.tensor([n > 0 for n in eff]).view(B, 1).expand(B, L).reshape(B * L)
    pad = torch.tensor([[t >= n for t in range(L)] for n in eff]).view(B * L)
    bar = _Bar(f"{cell} ndir={ndir} B={B} L={L} lens={lens}")
    for d, res in enumerate(per_dir):
        for name, gv in res.items():
            gv = gv.cpu()
            assert bool((gv[pad] == 0).all()), f"{name}[{d}]: padded positions are not exactly zero"
            src64, src32 = (r["l64"], r["l32"]) if name == "dgh" else (r["m64"], r["m32"])
            bar.check(f"{name}[{d}]", gv[keep], src64[name][d][keep], src32[name][d][keep])
    bar.done()


def test_gru_refuses_other_hidden_sizes_and_direction_counts():
    from ivln_ce_amd import ops
    from ivln_ce_amd._lib import IvlnError

    z = torch.zeros(3 * 256 * 256, device=DEV)
    lengths = torch.ones(1, dtype=torch.int32, device=DEV)
    for Hx in (64, 256, 127):
        with pytest.raises(IvlnError, match=r"\(-5\)"):
            ops.gru_dirs(z, z, z, z, z, z, lengths, 1, 1, Hx)
    with pytest.raises(IvlnError, match=r"\(-1\)"):
        ops.gru_dirs(z, z, z, z, z, z, lengths, 1, 1, 128, ndir=3)
    # the folded front end: the direction count and gx_r must agree
    tok = torch.zeros(1, 4, dtype=torch.int64, device=DEV)
    nz = torch.ones(8, dtype=torch.uint8, device=DEV)
    ln = torch.zeros(1, dtype=torch.int32, device=DEV)
    Lb, G = ops._L(), 384
    tab, gx = torch.zeros(8, 2 * G, device=DEV), torch.zeros(4, G, device=DEV)
    ops.embed_gates(tok, tab, nz, ndir=2), ops.embed_gates(tok, tab[:, :G].contiguous(), nz, ndir=1)
    a = (tok.data_ptr(), tab.data_ptr(), nz.data_ptr(), 1, 4, G, 8)
    assert Lb.ivln_embed_gates_dirs_f32(*a, 2, gx.data_ptr(), None, ln.data_ptr(), None, None, None) == -1
    assert Lb.ivln_embed_gates_dirs_f32(*a, 1, gx.data_ptr(), gx.data_ptr(), ln.data_ptr(), None, None, None) == -1
    torch.cuda.synchronize()


def test_lstm_is_the_same_bytes_through_every_launch_form():
    """ivln_lstm_dirs_fwd_f32 launched plain, with a ticket and spare = 3, and with a fresh InstructionStepCache whose rows
    are all dirty, for two directions and for one: the same bytes (out; gates and cs too where the form saves them), and the
    BPTT on those saves against the float64 reference.  lens (37, 5, 20, 1): every tail of the four-deep prefetch loop, the
    reverse direction, and - with the ticket - blocks that leave without work."""
    for ndir in (2, 1):
        _lstm_launch_forms(ndir)


def _lstm_launch_forms(ndir):
    from ivln_ce_amd import ops

    B, L, lens = 4, 37, (37, 5, 20, 1)
    r = _reference("LSTM", ndir, B, L, lens)
    c, eff = r["case"], r["eff"]
    lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
    d = [t for k in ("gx", "whh", "bhh") for t in ([x.to(DEV) for x in c[k]] + [None])[:2]]
    plain = ops.lstm_bidir(*d, lengths, B, L, H, save=True, ndir=ndir)
    for name, a, b_ in zip(("out", "gates", "cs"), plain, ops.lstm_bidir(*d, lengths, B, L, H, save=True, ndir=ndir)):
        assert _same_bytes(a, b_), f"save=True twice: {name}"
    out, gates, cs = ops.lstm_bidir(*d, lengths, B, L, H, ndir=ndir)
    assert gates is None and cs is None and _same_bytes(out, plain[0]), "plain without saves"
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    for _ in range(2):  # (twice: the re-armed ticket serves the next launch)
        out, gates, cs = ops.lstm_bidir(*d, lengths, B, L, H, spare=3, ticket=ticket, ndir=ndir)
        assert gates is None and cs is None and _same_bytes(out, plain[0]), "ticket + spare=3"
        assert int(ticket.item()) == 0
    cache = ops.InstructionStepCache(B, L, 4 * H, H, DEV, key=None, ndir=ndir)
    assert cache.dirty.tolist() == [1] * B
    cache.out.fill_(7.0)
    out, gates, cs = ops.lstm_bidir(*d, lengths, B, L, H, cache=cache, ndir=ndir)
    assert out is cache.out and gates is None and cs is None and _same_bytes(out, plain[0]), "fresh cache, every row dirty"
    out, _, _ = ops.lstm_bidir(*d, lengths, B, L, H, spare=3, ticket=ticket, cache=cache, ndir=ndir)
    assert _same_bytes(out, plain[0]) and int(ticket.item()) == 0, "ticket + spare=3 + cache"
    # the BPTT on the saves of the plain form
    dout = c["dout"].to(DEV)
    got = _twice(lambda: tuple(t for t in ops.lstm_bidir_bwd(dout, plain[0], plain[1], plain[2], d[2], d[3], lengths, B, L, H,
                                                             ndir=ndir) if t is not None))
    per_dir = [dict(dgi=got[k], hp=got[ndir + k]) for k in range(ndir)]
    pad = torch.tensor([[t >= n for t in range(L)] for n in eff]).view(B * L)
    bar = _Bar(f"LSTM ndir={ndir} B={B} L={L} lens={lens}")
    for k, res in enumerate(per_dir):
        for name, gv in res.items():
            gv = gv.cpu()
            assert bool((gv[pad] == 0).all()), f"{name}[{k}]: padded positions are not exactly zero"
            bar.check(f"{name}[{k}]", gv, r["m64"][name][k], r["m32"][name][k])
    bar.done()


# ------------------------------------------------------------------------------------------------------------------
# MapCMA with every non-default combination
# ------------------------------------------------------------------------------------------------------------------
def _rollout_obs(B, steps, seed):
    """SyntheticRollout observations on the device; row 1's instruction is cut to 11 tokens (unequal lengths)"""
    from ivln_ce_amd.synthetic import SyntheticRollout

    roll = SyntheticRollout(B=B, seed=seed)
    obs = []
    for _ in range(steps):
        o = roll.step()
        o["instruction"][1, 11:] = 0
        obs.append({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in o.items()})
    return obs


def _oracle_for(pol, cell, bidirectional, use_pm=False):
    ref = mapcma_oracle(cell, bidirectional, use_pm=use_pm)
    ref.load_state_dict({k: v.cpu() for k, v in pol.state_dict().items()})  # strict: the reference's keys
    return ref


def _update_batch(T, N, seed=42):
    g = torch.Generator().manual_seed(seed)
    TN = T * N
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
    nd = nd.view(-1, 1)
    tgt = torch.randint(0, 4, (T, N), generator=g)
    w = torch.where(torch.rand(T, N, generator=g) < 0.5, torch.tensor(3.2), torch.tensor(1.0))
    return obs, prev, nd, tgt, w


@pytest.mark.parametrize("cell,bidirectional", NON_DEFAULT)
def test_mapcma_step_and_distribution_match_the_oracle(cell, bidirectional, monkeypatch):
    from ivln_ce_amd import ops
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.obs_transforms import GTSemanticsIterativeMapper

    torch.set_num_threads(8)
    B = 2
    pol = make_policy(cell, bidirectional).to(DEV).eval()
    ref = _oracle_for(pol, cell, bidirectional).eval()
    fused = []
    real = ops.cma_step
    monkeypatch.setattr(ops, "cma_step", lambda d: (fused.append(d.Ct), real(d))[1])
    feats = {}
    pol.net.register_forward_hook(lambda mod, args, o: feats.__setitem__("f", o[0]))
    tr = GTSemanticsIterativeMapper.from_config(get_config())
    b = tr(dict(_rollout_obs(B, 1, seed=77)[0]))
    masks = b["not_done_masks"]
    rnn = torch.zeros(B, 2, 512)
    prev = torch.zeros(B, 1, dtype=torch.long)
    with torch.no_grad():
        a, rnn_d = pol.act(b, rnn.to(DEV), prev.to(DEV), masks, deterministic=True)
        lg = pol.action_distribution.raw_logits(feats["f"])
        cpu = {k: b[k].cpu() for k in ("depth", "occupancy_map", "semantic_map", "instruction")}
        lr, rnn_r, fr = ref.logits(cpu, rnn, prev, masks.cpu())
    e_l, e_f = float((lg.cpu() - lr).abs().max()), float((feats["f"].cpu() - fr).abs().max())
    e_s = float((rnn_d.cpu() - rnn_r).abs().max())
    print(f"{cell} bidirectional={bidirectional} act: logits {e_l:.3e} features {e_f:.3e} states {e_s:.3e}")
    # the fused recurrent head is parameterised by the text width (CmaStepDesc.Ct): it runs for 128 as for 256
    assert fused == [pol.net.instruction_encoder.output_size], fused
    assert e_l < 1e-4 and e_f < 2e-4 and e_s < 2e-4
    assert float((lr.max(-1, keepdim=True).values - lr.gather(1, a.cpu())).max()) < 2e-4

    # build_distribution over T = 3 as the trainers call it: autograd on, the unfused chain with its saves
    T, N = 3, 2
    obs, prev, nd, _, _ = _update_batch(T, N)
    h0 = torch.zeros(N, 2, 512)
    dist, _ = pol.build_distribution({k: v.to(DEV) for k, v in obs.items()}, h0.to(DEV), prev.to(DEV), nd.to(DEV))
    assert dist.logits.requires_grad
    with torch.no_grad():
        lr, _, _ = ref.logits(obs, h0, prev, nd)
    e = float((dist.logits.detach().cpu() - torch.log_softmax(lr, -1)).abs().max())
    print(f"{cell} bidirectional={bidirectional} build_distribution T={T}: logits {e:.3e}")
    assert e < 1e-4


@pytest.mark.parametrize("cell,bidirectional", NON_DEFAULT)
def test_mapcma_update_gradients_of_the_instruction_branch(cell, bidirectional):
    """one `update_agent` at T = 3, N = 2: the gradients of the instruction encoder's parameters (the embedding table trains
    in this config) and of text_k / text_q against float64 autograd of the oracle's loss, under the _Bar rule with the
    oracle's own float32 run as e32"""
    from ivln_ce_amd.aux_losses import AuxLosses
    from ivln_ce_amd.trainers import FlatAdam, update_agent
    from ivln_ce_amd.utils import dedupe_instructions, trim_instruction_padding

    torch.set_num_threads(8)
    T, N = 3, 2
    obs, prev, nd, tgt, w = _update_batch(T, N)
    pol = make_policy(cell, bidirectional, use_pm=True).to(DEV).train()
    grads = {}
    for dt in (torch.float64, torch.float32):
        ref = _oracle_for(pol, cell, bidirectional, use_pm=True).train().to(dt)
        torch.set_default_dtype(dt)  # (tensors the oracle creates itself: initial state, one-hot maps)
        try:
            loss_r, _, _, _ = ref.update_loss({k: v.to(dt) for k, v in obs.items()}, prev, nd, tgt, w.to(dt))
            loss_r.backward()
        finally:
            torch.set_default_dtype(torch.float32)
        grads[dt] = {k: p.grad.detach() for k, p in ref.named_parameters() if p.grad is not None}
        if dt == torch.float64:
            loss64 = float(loss_r.detach())
    opt = FlatAdam(pol, lr=2.5e-4)
    dobs = dedupe_instructions(trim_instruction_padding(dict(obs), first_rows=N))
    dobs = {k: v.to(DEV) for k, v in dobs.items()}
    AuxLosses.activate()
    try:
        loss, _, _ = update_agent(pol, opt, dobs, prev.to(DEV), nd.to(DEV), tgt.to(DEV), w.to(DEV), hidden_size=512,
                                  step_grad=False)
    finally:
        AuxLosses.deactivate()
    print(f"{cell} bidirectional={bidirectional} update: loss {loss:.7f} ref {loss64:.7f}")
    assert abs(loss - loss64) < 2e-5
    params = dict(pol.named_parameters())
    names = [k for k in params if k.startswith("net.instruction_encoder.") or k.startswith(("net.text_k.", "net.text_q."))]
    stems = 4 * (2 if bidirectional else 1)
    assert len(names) == stems + 1 + 4 and all(params[k].requires_grad and k in grads[torch.float64] for k in names)
    bar = _Bar(f"{cell} bidirectional={bidirectional} update")
    for k in names:
        bar.check(k[4:], params[k].grad, grads[torch.float64][k], grads[torch.float32][k])
    bar.done()


@pytest.mark.parametrize("cell,bidirectional", NON_DEFAULT)
def test_mapcma_graph_replay_is_bit_identical_to_eager(cell, bidirectional, same_depth_path):
    same_depth_path(0)
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.graphed import GraphedRollout
    from ivln_ce_amd.obs_transforms import GTSemanticsIterativeMapper

    B, steps = 2, 3
    pol = make_policy(cell, bidirectional).to(DEV).eval()
    cfg = get_config()
    obs = _rollout_obs(B, steps, seed=31)
    obs[1]["instruction"][0, 3:9] = torch.arange(100, 106, device=DEV)  # one row's tokens change at step 1: that row alone is re-encoded
    obs[2]["instruction"] = obs[1]["instruction"].clone()
    tr_e = GTSemanticsIterativeMapper.from_config(cfg)
    rnn = torch.zeros(B, 2, 512, device=DEV)
    prev = torch.zeros(B, 1, dtype=torch.long, device=DEV)
    eager, dirty = [], []
    for o in obs:
        b = tr_e(dict(o))
        with torch.no_grad():
            a, rnn = pol.act(b, rnn, prev, b["not_done_masks"], deterministic=True)
        prev = a
        eager.append((a.clone(), rnn.clone()))
        cache = pol.net.instruction_encoder.last_cache
        dirty.append(None if cache is None else cache.dirty.tolist())
    assert dirty == [[1, 1], [1, 0], [0, 0]], dirty  # the cache's dirty path ran, row by row
    assert getattr(pol.net.instruction_encoder, "lstm_spare", 1) == 1
    tr_g = GTSemanticsIterativeMapper.from_config(cfg)
    runner = GraphedRollout(pol, [tr_g], obs[0], deterministic=True)
    if cell == "GRU":
        assert getattr(pol.net.instruction_encoder, "lstm_spare", 1) == 1  # (no ticket form of the GRU kernel)
    tr_g.mapping_module.reset()
    runner.reset_state()
    for t, o in enumerate(obs):
        a = runner.step(o)
        torch.cuda.synchronize()
        assert torch.equal(a, eager[t][0]), f"actions step {t}"
        assert torch.equal(runner.rnn_states, eager[t][1]), f"rnn step {t}"
    tr_g.mapping_module.check_status()


def test_default_policy_bytes_do_not_move_when_an_option_policy_runs():
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.obs_transforms import GTSemanticsIterativeMapper

    B = 2
    obs = _rollout_obs(B, 1, seed=5)[0]

    def step(cell, bidirectional):
        pol = make_policy(cell, bidirectional).to(DEV).eval()
        b = GTSemanticsIterativeMapper.from_config(get_config())(dict(obs))
        out = {}
        pol.net.register_forward_hook(lambda mod, args, o: out.__setitem__("f", o[0].clone()))
        with torch.no_grad():
            a, rnn = pol.act(b, torch.zeros(B, 2, 512, device=DEV), torch.zeros(B, 1, dtype=torch.long, device=DEV),
                             b["not_done_masks"], deterministic=True)
        return a.clone(), rnn.clone(), out["f"]

    before = step("LSTM", True)
    for cell, bidirectional in NON_DEFAULT:
        other = step(cell, bidirectional)
        assert not torch.equal(other[2], before[2])
    after = step("LSTM", True)
    assert torch.equal(before[0], after[0]) and _same_bytes(before[1], after[1]) and _same_bytes(before[2], after[2])


def test_unidirectional_lstm_over_subscribed_grid_is_the_plain_launch():
    """ivln_lstm_dirs_fwd_f32 with ndir = 1 and a ticket word: B * spare blocks draw the B items, the rest leave
    (`item >= ND * B`); same bytes as the plain launch, and the last block re-arms the ticket"""
    B, L, lens = 4, 37, (37, 5, 20, 1)
    c = make_case("LSTM", 1, B, L)
    lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
    plain, _ = _forward("LSTM", 1, c, lengths, B, L)
    from ivln_ce_amd import ops

    d = [c[k][0].to(DEV) for k in ("gx", "whh", "bhh")]
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    for spare in (2, 3):
        for _ in range(2):  # (twice: the re-armed ticket serves the next launch)
            got, _, _ = ops.lstm_bidir(d[0], None, d[1], None, d[2], None, lengths, B, L, H, spare=spare, ticket=ticket, ndir=1)
            assert _same_bytes(got, plain), f"spare {spare}"
            assert int(ticket.item()) == 0


def test_mapcma_no_grad_distribution_over_a_time_major_batch_takes_the_unfused_chain(monkeypatch):
    """rows = T * N over N states is not a step: without autograd it must not reach the fused recurrent head (one step of
    `rows` states, which would read and write T times the state buffers) but run the unfused chain - the logits are the
    oracle's and the grad-enabled call's within the policy bound"""
    from ivln_ce_amd import ops

    torch.set_num_threads(8)
    cell, bidirectional = "GRU", False
    pol = make_policy(cell, bidirectional).to(DEV).eval()
    ref = _oracle_for(pol, cell, bidirectional).eval()
    fused = []
    real = ops.cma_step
    monkeypatch.setattr(ops, "cma_step", lambda d: (fused.append(d.rows), real(d))[1])
    T, N = 3, 2
    obs, prev, nd, _, _ = _update_batch(T, N)
    h0 = torch.zeros(N, 2, 512)
    dobs = {k: v.to(DEV) for k, v in obs.items()}
    with torch.no_grad():
        dist, rnn = pol.build_distribution(dobs, h0.to(DEV), prev.to(DEV), nd.to(DEV))
        lr, rnn_r, _ = ref.logits(obs, h0, prev, nd)
    assert fused == [], f"the fused head ran with rows = {fused}"
    assert tuple(rnn.shape) == (N, 2, 512)
    dist_g, _ = pol.build_distribution(dobs, h0.to(DEV), prev.to(DEV), nd.to(DEV))
    e_o = float((dist.logits.cpu() - torch.log_softmax(lr, -1)).abs().max())
    e_g = float((dist.logits - dist_g.logits.detach()).abs().max())
    e_s = float((rnn.cpu() - rnn_r).abs().max())
    print(f"no-grad T={T}: logits vs oracle {e_o:.3e}, vs grad-enabled {e_g:.3e}, states {e_s:.3e}")
    assert e_o < 1e-4 and e_g < 1e-4 and e_s < 2e-4


# ------------------------------------------------------------------------------------------------------------------
# Latent-CMA with (GRU, bidirectional) and (LSTM, unidirectional)
# ------------------------------------------------------------------------------------------------------------------
LATENT = [("GRU", True), ("LSTM", False)]


def _latent_batch(T, N, seed=7):
    """cached image features (what the trainers feed an update), instructions of unequal length"""
    g = torch.Generator().manual_seed(seed)
    TN = T * N
    instr = torch.zeros(N, 200)
    for n in range(N):
        instr[n, :30 - 9 * n] = torch.randint(2, 2504, (30 - 9 * n,), generator=g).float()
    obs = {"rgb_features": torch.rand(TN, 2048, 4, 4, generator=g), "depth_features": torch.rand(TN, 128, 4, 4, generator=g),
           "instruction": instr.repeat(T, 1)}
    prev = torch.randint(0, 4, (TN, 1), generator=g)
    nd = torch.ones(T, N, dtype=torch.uint8)
    nd[0] = 0
    if T > 1:
        nd[1, 1] = 0
    tgt = torch.randint(0, 4, (T, N), generator=g)
    w = torch.where(torch.rand(T, N, generator=g) < 0.5, torch.tensor(3.2), torch.tensor(1.0))
    return obs, prev, nd.view(-1, 1), tgt, w


@pytest.mark.parametrize("cell,bidirectional", LATENT)
def test_latent_step_and_distribution_match_the_oracle(cell, bidirectional):
    torch.set_num_threads(8)
    pol = make_policy(cell, bidirectional, "LatentCMAPolicy").to(DEV).eval()
    ref = LatentCMAPolicyOptRef(cell, bidirectional).load_from(pol).eval()
    feats = {}
    pol.net.register_forward_hook(lambda mod, args, o: feats.__setitem__("f", o[0]))
    g = torch.Generator().manual_seed(3)
    for T, N in ((1, 3), (3, 2)):  # one act step of 3 envs with a carried state; a distribution over T = 3
        obs, prev, nd, _, _ = _latent_batch(T, N)
        if T == 1:
            nd = torch.tensor([[1], [0], [1]], dtype=torch.uint8)
        h0 = 0.1 * torch.randn(N, 2, 512, generator=g)
        dobs = {k: v.to(DEV) for k, v in obs.items()}
        if T == 1:
            with torch.no_grad():
                a, rnn = pol.act(dobs, h0.to(DEV), prev.to(DEV), nd.to(DEV), deterministic=True)
            lg = torch.log_softmax(pol.action_distribution.raw_logits(feats["f"]), -1).detach()
        else:
            dist, rnn = pol.build_distribution(dobs, h0.to(DEV), prev.to(DEV), nd.to(DEV))  # (autograd on: the trainers' call)
            assert dist.logits.requires_grad
            lg = dist.logits.detach()
        with torch.no_grad():
            lr, rnn_r, fr = ref.logits(obs, h0, prev, nd)
        e_l = float((lg.cpu() - torch.log_softmax(lr, -1)).abs().max())
        e_f = float((feats["f"].detach().cpu() - fr).abs().max())
        e_s = float((rnn.detach().cpu() - rnn_r).abs().max())
        print(f"latent {cell} bidirectional={bidirectional} T={T} N={N}: logits {e_l:.3e} features {e_f:.3e} states {e_s:.3e}")
        assert e_l < 1e-4 and e_f < 2e-4 and e_s < 2e-4
        if T == 1:
            assert float((lr.max(-1, keepdim=True).values - lr.gather(1, a.cpu())).max()) < 2e-4


@pytest.mark.parametrize("cell,bidirectional", LATENT)
def test_latent_update_gradients_of_the_instruction_branch(cell, bidirectional):
    """build_distribution + the weighted cross entropy + backward at T = 3, N = 2: the gradients of the instruction encoder's
    parameters (embedding included) and text_k / text_q against float64 autograd of the oracle, _Bar rule, e32 = the
    oracle's own float32 run"""
    import torch.nn.functional as F

    torch.set_num_threads(8)
    T, N = 3, 2
    obs, prev, nd, tgt, w = _latent_batch(T, N)
    pol = make_policy(cell, bidirectional, "LatentCMAPolicy").to(DEV).train()
    grads = {}
    for dt in (torch.float64, torch.float32):
        ref = LatentCMAPolicyOptRef(cell, bidirectional).load_from(pol).train().to(dt)
        loss_r = ref.update_loss({k: v.to(dt) for k, v in obs.items()}, prev, nd, tgt, w.to(dt))
        loss_r.backward()
        grads[dt] = {k: p.grad.detach() for k, p in ref.named_parameters() if p.grad is not None}
        if dt == torch.float64:
            loss64 = float(loss_r.detach())
    dist, _ = pol.build_distribution({k: v.to(DEV) for k, v in obs.items()}, torch.zeros(N, 2, 512, device=DEV), prev.to(DEV),
                                     nd.to(DEV))
    ce = F.cross_entropy(dist.logits.view(T, N, -1).permute(0, 2, 1), tgt.to(DEV), reduction="none")
    wd = w.to(DEV)
    loss = ((wd * ce).sum(0) / wd.sum(0)).mean()
    loss.backward()
    print(f"latent {cell} bidirectional={bidirectional} update: loss {float(loss.detach()):.7f} ref {loss64:.7f}")
    assert abs(float(loss.detach()) - loss64) < 2e-5
    params = dict(pol.named_parameters())
    names = [k for k in params if k.startswith("net.instruction_encoder.") or k.startswith(("net.text_k.", "net.text_q."))]
    assert len(names) == 4 * (2 if bidirectional else 1) + 1 + 4
    assert all(params[k].grad is not None and k in grads[torch.float64] for k in names)
    bar = _Bar(f"latent {cell} bidirectional={bidirectional} update")
    for k in names:
        bar.check(k[4:], params[k].grad, grads[torch.float64][k], grads[torch.float32][k])
    bar.done()


@pytest.mark.parametrize("cell,bidirectional", LATENT)
def test_latent_graph_replay_is_bit_identical_to_eager(cell, bidirectional, same_depth_path):
    same_depth_path(0)
    from ivln_ce_amd.graphed import GraphedRollout
    from ivln_ce_amd.synthetic import SyntheticRollout

    B, steps = 2, 3
    pol = make_policy(cell, bidirectional, "LatentCMAPolicy").to(DEV).eval()
    roll = SyntheticRollout(B=B, seed=11, with_rgb=True)
    obs = []
    for _ in range(steps):
        o = roll.step()
        o["instruction"][1, 11:] = 0
        obs.append({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in o.items()})
    obs[1]["instruction"][0, 3:9] = torch.arange(100, 106, device=DEV)  # one row's tokens change at step 1
    obs[2]["instruction"] = obs[1]["instruction"].clone()
    rnn = torch.zeros(B, 2, 512, device=DEV)
    prev = torch.zeros(B, 1, dtype=torch.long, device=DEV)
    eager, dirty = [], []
    for o in obs:
        with torch.no_grad():
            a, rnn = pol.act(o, rnn, prev, o["not_done_masks"], deterministic=True)
        prev = a
        eager.append((a.clone(), rnn.clone()))
        cache = pol.net.instruction_encoder.last_cache
        dirty.append(None if cache is None else cache.dirty.tolist())
    assert dirty == [[1, 1], [1, 0], [0, 0]], dirty  # the per-episode cache ran, row by row
    runner = GraphedRollout(pol, [], obs[0], deterministic=True)
    runner.reset_state()
    for t, o in enumerate(obs):
        a = runner.step(o)
        torch.cuda.synchronize()
        assert torch.equal(a, eager[t][0]), f"actions step {t}"
        assert torch.equal(runner.rnn_states, eager[t][1]), f"rnn step {t}"
