"""GPU: `encoders.InstructionEncoder` over pre-computed text features (`sensor_uuid = "rxr_instruction"`): outputs and the
gradients of W_ih, W_hh and both biases against the float64 restatement of tests/text_feat_ref.py (held to the reference's
module by tests/test_text_feat_host.py) under kernel_bar's rule, exact zeros past each length, and the per-episode step
cache byte for byte against the uncached chain."""
import functools

import pytest
import torch

from instr_rnn_ref import COMBOS
from kernel_bar import _Bar, _same_bytes
from text_feat_ref import KEY, encoder_ref, patterned_features, row_counts, rxr_config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOG = "text_feat_encoder.log"
FULL = list(range(6))
# row counts [6, 2, 1]; then the zero row at t = 1 between non-zero rows 0, 2, 3 (count 3, not last index 4)
PATTERNS = {"counts-6-2-1": ([FULL, [0, 1], [0]], 6, 8), "middle-zero": ([[0, 2, 3], FULL, [0, 1]], 6, 8)}
SMALL = [(c, b, p) for c, b in COMBOS for p in PATTERNS]
CASES = SMALL + [("LSTM", True, "rxr-512x768")]


def _shape(pattern):
    if pattern in PATTERNS:
        return PATTERNS[pattern]
    return [list(range(300)), [0] + list(range(2, 41))], 512, 768  # (counts 300 and 40, the second with a zero row at 1)


def _encoder(cell, bidirectional, E):
    from det_init import det_fill

    from ivln_ce_amd.encoders import InstructionEncoder

    enc = InstructionEncoder(rxr_config(cell, bidirectional, E=E).MODEL.INSTRUCTION_ENCODER)
    return det_fill(enc, seed=0).to(DEV)


@functools.lru_cache(maxsize=None)
def _reference(cell, bidirectional, pattern):
    """computed once per case, shared by the tests, never modified: float64 and float32 runs of the restatement with the
    gradients of sum(out * dout)"""
    rows, L, E = _shape(pattern)
    x = patterned_features(rows, L, E, seed=17)
    enc = _encoder(cell, bidirectional, E)
    g = torch.Generator().manual_seed(5)
    dout = torch.randn(len(rows), enc.output_size, L, generator=g)
    r = dict(x=x, dout=dout, lens=row_counts(x).tolist())
    for dt in (torch.float64, torch.float32):
        ref = encoder_ref(enc, dt)
        out = ref({KEY: x.to(dt)}, total_length=L)
        (out * dout.to(dt)).sum().backward()
        r[dt] = dict(out=out.detach(), grads={k: p.grad.detach() for k, p in ref.named_parameters()})
    return r


@pytest.mark.parametrize("cell,bidirectional,pattern", CASES)
def test_outputs_and_gradients_match_the_float64_restatement(cell, bidirectional, pattern):
    from ivln_ce_amd import train

    torch.set_num_threads(8)
    r = _reference(cell, bidirectional, pattern)
    x, lens = r["x"].to(DEV), r["lens"]
    B, L, E = x.shape
    enc = _encoder(cell, bidirectional, E)
    save = {}
    with torch.no_grad():
        out, lengths = enc({KEY: x}, save)
        plain, lengths2 = enc({KEY: x})
    assert lengths.tolist() == lens == lengths2.tolist()
    assert "tokens" not in save and save["emb"].data_ptr() == x.data_ptr() and tuple(save["emb"].shape) == (B * L, E)
    bar = _Bar(f"{cell} bidir={int(bidirectional)} {pattern}", LOG)
    for name, o in (("out-update", out), ("out-rollout", plain)):
        assert tuple(o.shape) == (B, enc.output_size, L)
        for b, n in enumerate(lens):
            assert bool((o[b, :, n:] == 0).all()), f"{name} row {b}: columns >= {n} are not exactly zero"
        bar.check(name, o, r[torch.float64]["out"], r[torch.float32]["out"])
    G = {}
    train.instruction_backward(enc, save, r["dout"].to(DEV), B, L, G)
    params = dict(enc.named_parameters())
    assert set(G) == set(params.values()) and len(params) == 4 * enc.ndir
    for k, p in params.items():
        bar.check(k[len("encoder_rnn."):], G[p], r[torch.float64]["grads"][k], r[torch.float32]["grads"][k])
    bar.done()


@pytest.mark.parametrize("cell,bidirectional,pattern", CASES)
def test_cached_call_equals_uncached_call_byte_for_byte(cell, bidirectional, pattern, monkeypatch):
    from ivln_ce_amd import ops

    x = _reference(cell, bidirectional, pattern)["x"].to(DEV)
    enc = _encoder(cell, bidirectional, x.shape[2])
    with torch.no_grad():
        cached, ln_c = enc({KEY: x})
        assert enc.last_cache is not None and enc.last_cache.dirty.tolist() == [1] * x.shape[0]
        again, _ = enc({KEY: x})
        assert enc.last_cache.dirty.tolist() == [0] * x.shape[0] and again.data_ptr() == cached.data_ptr()
        monkeypatch.setattr(ops, "CACHE_INSTRUCTION", False)  # (IVLN_CACHE_INSTRUCTION=0)
        plain, ln_p = enc({KEY: x})
        assert enc.last_cache is None
    assert _same_bytes(cached, plain) and ln_c.tolist() == ln_p.tolist()
    with torch.enable_grad():  # (a call that is neither an update pass nor a rollout step: the uncached chain)
        other, _ = enc({KEY: x})
    assert enc.last_cache is None and _same_bytes(other, plain)


@pytest.mark.parametrize("cell,bidirectional", COMBOS)
def test_three_steps_with_one_instruction_swapped(cell, bidirectional, monkeypatch):
    from ivln_ce_amd import ops

    rows, L, E = PATTERNS["counts-6-2-1"]
    x0 = patterned_features(rows, L, E, seed=17).to(DEV)
    x1 = x0.clone()
    x1[1] = patterned_features([[0, 2, 3]], L, E, seed=99)[0].to(DEV)  # env 1 starts another episode at step 2
    enc = _encoder(cell, bidirectional, E)
    steps, dirty = [], []
    with torch.no_grad():
        for x in (x0, x1, x1):
            out, ln = enc({KEY: x})
            steps.append((out.clone(), ln.clone()))
            dirty.append(enc.last_cache.dirty.tolist())
        assert dirty == [[1, 1, 1], [0, 1, 0], [0, 0, 0]], dirty
        monkeypatch.setattr(ops, "CACHE_INSTRUCTION", False)
        for (out, ln), x in zip(steps, (x0, x1, x1)):
            plain, ln_p = enc({KEY: x})
            assert _same_bytes(out, plain) and ln.tolist() == ln_p.tolist()
    assert steps[1][1].tolist() == [6, 3, 1]


def test_weight_change_invalidates_the_cache():
    """a parameter written in place (a version bump) or behind torch's back (ops.WEIGHT_EPOCH, FlatAdam.step) re-encodes
    every row at the next step"""
    from ivln_ce_amd import ops

    rows, L, E = PATTERNS["counts-6-2-1"]
    x = patterned_features(rows, L, E, seed=17).to(DEV)
    enc = _encoder("LSTM", True, E)
    with torch.no_grad():
        a = enc({KEY: x})[0].clone()
        enc.encoder_rnn.weight_ih_l0.mul_(0.5)
        b = enc({KEY: x})[0].clone()
        assert enc.last_cache.dirty.tolist() == [1, 1, 1] and not torch.equal(a, b)
        enc.encoder_rnn.weight_ih_l0.data.view(-1)[:].mul_(2.0)  # (no version bump through .data)
        ops.WEIGHT_EPOCH += 1
        ops.invalidate_step_caches()
        c = enc({KEY: x})[0]
        assert enc.last_cache.dirty.tolist() == [1, 1, 1] and _same_bytes(a, c)
