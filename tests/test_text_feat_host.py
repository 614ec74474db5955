"""CPU: the instruction encoder over pre-computed text features (`MODEL.INSTRUCTION_ENCODER.sensor_uuid = "rxr_instruction"`).
The float64 restatement the GPU tests compare against is held to the reference's own module (tests/golden/rxr_instruction.npz,
tests/golden/gen_rxr_instruction_golden.py); the policies construct from an RxR config with the reference's state-dict keys;
the library exports the header's entry points; the update batch's de-duplication and the store-once bookkeeping of the
loaders."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from det_init import det_fill  # noqa: E402
from instr_rnn_ref import COMBOS  # noqa: E402
from text_feat_ref import KEY, TextFeatEncoderRef, make_rxr_policy, row_counts  # noqa: E402

EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "rxr_instruction.npz")) as f:
        return {k: f[k] for k in f.files}


def test_row_counts_are_counts_not_last_indices(golden):
    x = torch.from_numpy(golden[KEY])
    assert row_counts(x).tolist() == [6, 2, 1, 3]  # (row 3: non-zero rows 0, 2, 3 - a last-index rule would say 4)
    assert bool((x[3, 1] == 0).all()) and bool((x[3, 3] != 0).any())


@pytest.mark.parametrize("cell,bidirectional", COMBOS)
def test_restatement_matches_the_reference_module(golden, cell, bidirectional):
    """bound: e32 = torch's own fp32 module against float64 on the same inputs, then kernel_bar's rule
    4 * e32 + 4 * 2^-24 * max|ref| - the golden file IS a float32 torch run, of the reference's module"""
    x = torch.from_numpy(golden[KEY])
    want = torch.from_numpy(golden[f"out/{cell}/{int(bidirectional)}"])
    B, L, E = x.shape
    runs = {}
    for dt in (torch.float64, torch.float32):
        enc = det_fill(TextFeatEncoderRef(cell, bidirectional, E), seed=0).to(dt)
        with torch.no_grad():
            runs[dt] = enc({KEY: x.to(dt)}, total_length=L)
    r64 = runs[torch.float64]
    assert tuple(want.shape) == tuple(r64.shape) == (B, 128 * (2 if bidirectional else 1), L)
    e32 = float((runs[torch.float32].double() - r64).abs().max())
    bar = 4 * e32 + 4 * EPS * float(r64.abs().max())
    err = float((want.double() - r64).abs().max())
    print(f"{cell} bidirectional={bidirectional}: golden vs float64 restatement {err:.3e}  e32 {e32:.3e}  bar {bar:.3e}")
    assert err <= bar
    # count semantics: row 3 (zero row at t = 1, count 3) runs over rows 0, 1, 2 - column 3, a NON-zero input row, is padding
    for b, n in enumerate([6, 2, 1, 3]):
        assert bool((want[b, :, n:] == 0).all()) and bool((r64[b, :, n:] == 0).all())
        assert bool((want[b, :, n - 1] != 0).any())


@pytest.mark.parametrize("policy_name", ["MapCMAPolicy", "LatentCMAPolicy"])
@pytest.mark.parametrize("cell,bidirectional", [("LSTM", True), ("GRU", False)])
def test_policies_construct_from_an_rxr_config(policy_name, cell, bidirectional):
    pol = make_rxr_policy(cell, bidirectional, policy_name)
    enc = pol.net.instruction_encoder
    assert enc.uses_features and enc.obs_key == KEY and not hasattr(enc, "embedding_layer")
    sd = enc.state_dict()
    assert not any("embedding_layer" in k for k in sd)
    gates = 3 if cell == "GRU" else 4
    assert tuple(enc.encoder_rnn.weight_ih_l0.shape) == (gates * 128, 768)
    twin = getattr(nn, cell)(input_size=768, hidden_size=128, bidirectional=bidirectional)
    want = {"encoder_rnn." + k: tuple(v.shape) for k, v in twin.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    other = make_rxr_policy(cell, bidirectional, policy_name)
    with torch.no_grad():
        for p in other.net.instruction_encoder.parameters():
            p.zero_()
    other.net.instruction_encoder.load_state_dict(sd)  # strict round trip
    assert all(torch.equal(v, other.net.instruction_encoder.state_dict()[k]) for k, v in sd.items())


def test_token_encoder_keeps_its_key_and_embedding():
    from instr_rnn_ref import make_policy

    enc = make_policy("LSTM", True, fill=False).net.instruction_encoder
    assert not enc.uses_features and enc.obs_key == "instruction" and hasattr(enc, "embedding_layer")


def test_library_exports_every_entry_of_the_text_feature_header():
    import __graft_entry__ as ge

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ivln_text_feat.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ivln_[a-z0-9_]+)\s*\(", src)))
    assert names == ["ivln_text_feat_front_f32", "ivln_text_feat_gates_f32", "ivln_text_feat_ws_words"]
    L = ctypes.CDLL(ge.build())
    assert all(hasattr(L, n) for n in names)
    ops_src = open(os.path.join(ROOT, "ivln-ce_amd", "ops.py")).read()
    assert all(f".{n}(" in ops_src for n in names)
    # refusals need no GPU: nothing is launched
    L.ivln_text_feat_ws_words.restype = ctypes.c_int64
    assert L.ivln_text_feat_ws_words(5) == 10
    one = ctypes.c_void_p(16)  # (never dereferenced: every call below is refused before a launch)
    assert L.ivln_text_feat_front_f32(None, 1, 1, 1, one, None, None, None, one, None) == -1
    assert L.ivln_text_feat_front_f32(one, 0, 1, 1, one, None, None, None, one, None) == -1
    assert L.ivln_text_feat_front_f32(one, 1, 1, 1, one, one, None, one, one, None) == -1  # a partial cache set
    assert L.ivln_text_feat_gates_f32(one, 1, 1, 1, None, None, 4, None, one, None) == -1


# ------------------------------------------------------------------------------------------------------------------
# update batches
# ------------------------------------------------------------------------------------------------------------------
def _batch(T=3, N=2, L=4, E=3):
    g = torch.Generator().manual_seed(9)
    first = torch.randn(N, L, E, generator=g)
    first[1, 2:] = 0
    return first.repeat(T, 1, 1).clone(), first


def test_dedupe_instruction_features_with_a_padded_tail():
    from ivln_ce_amd.utils import dedupe_instruction_features

    T, N = 3, 2
    x, first = _batch(T, N)
    x[2 * N + 1] = 1.0  # trajectory 1 ended after two steps: collate_fn's padding
    obs = {KEY: x, "other": torch.zeros(T * N)}
    out = dedupe_instruction_features(obs, first_rows=N)
    assert out is not obs and KEY + "_unique" not in obs
    u, idx = out[KEY + "_unique"], out[KEY + "_index"]
    assert tuple(u.shape) == (N + 1, 4, 3) and idx.dtype == torch.int32 and idx.tolist() == [0, 1, 0, 1, 0, 2]
    assert torch.equal(u[:N], first) and bool((u[N] == 1).all())
    assert torch.equal(u[idx.long()], x)  # the expanded result is the input


def test_dedupe_instruction_features_leaves_a_foreign_row_alone():
    from ivln_ce_amd.utils import dedupe_instruction_features

    T, N = 3, 2
    x, _ = _batch(T, N)
    x[N, 0, 0] += 1.0  # row (1, 0) is neither row (0, 0) nor padding
    obs = {KEY: x}
    assert dedupe_instruction_features(obs, first_rows=N) is obs
    assert dedupe_instruction_features({"instruction": torch.zeros(6, 5)}, first_rows=2).keys() == {"instruction"}


def test_bitwise_compare_tells_negative_zero():
    from ivln_ce_amd.utils import dedupe_instruction_features

    x, _ = _batch(3, 2)
    x[1, 3, 0] = 0.0
    x[3, 3, 0] = -0.0
    obs = {KEY: x}
    assert dedupe_instruction_features(obs, first_rows=2) is obs


def test_store_keeps_features_once_and_collate_repeats_them(tmp_path):
    """TrajectoryStore holds a trajectory's features as one (1, L, E) record; collate_fn then builds what the reference's
    collate_fn builds from per-timestep copies: the instruction repeated, padded timesteps 1.0"""
    from ivln_ce_amd.trainers import TrajectoryStore, collate_fn

    L, E = 4, 3
    g = np.random.RandomState(0)
    store = TrajectoryStore(str(tmp_path))
    feats = [g.randn(L, E).astype(np.float32) for _ in range(2)]
    lens = [3, 2]
    for i, (f, T) in enumerate(zip(feats, lens)):
        store.put(i, {KEY: np.repeat(f[None], T, 0), "progress": g.rand(T, 1)}, np.zeros(T), np.arange(T) % 4)
    items = []
    for i, T in enumerate(lens):
        obs, prev, oracle = store.get(i)
        assert obs[KEY].shape == (1, L, E) and obs["progress"].shape == (T, 1)
        items.append(({k: torch.from_numpy(np.copy(v)) for k, v in obs.items()}, torch.from_numpy(prev),
                      torch.from_numpy(oracle), torch.ones(T)))
    flat = collate_fn(items)[0]
    x = flat[KEY].view(3, 2, L, E)
    for n, (f, T) in enumerate(zip(feats, lens)):
        assert all(np.array_equal(x[t, n].numpy(), f) for t in range(T))
        assert bool((x[T:, n] == 1).all())
    # a trajectory whose features change is stored as it is
    moving = np.repeat(feats[0][None], 3, 0).copy()
    moving[2, 0, 0] += 1
    store.put(7, {KEY: moving}, np.zeros(3), np.zeros(3))
    assert store.get(7)[0][KEY].shape == (3, L, E)


def test_tour_collate_repeats_a_store_record_with_features(tmp_path):
    """the tour-ordered reader of the same store (tour_batches.TourTrajectoryDataset / tour_collate, IterativeDaggerTrainer):
    a 3-step and a 2-step trajectory keep their features at every one of their timesteps, padded timesteps are 1.0, and the
    batch de-duplicates like collate_fn's"""
    from ivln_ce_amd.tour_batches import TourTrajectoryDataset, tour_collate
    from ivln_ce_amd.trainers import TrajectoryStore
    from ivln_ce_amd.utils import dedupe_instruction_features

    L, E = 4, 3
    g = np.random.RandomState(1)
    store = TrajectoryStore(str(tmp_path))
    feats = [g.randn(L, E).astype(np.float32) for _ in range(2)]
    lens = [3, 2]
    for i, (f, T) in enumerate(zip(feats, lens)):
        store.put(i, {KEY: np.repeat(f[None], T, 0), "progress": g.rand(T, 1)}, np.zeros(T), np.arange(T) % 4)
        assert store.get(i)[0][KEY].shape == (1, L, E)
    ds = TourTrajectoryDataset(store, use_iw=True, inflection_weight_coef=3.2)
    ds.set_tour_done_idxs({0})
    batch = tour_collate([ds[0], ds[1]])
    x = batch[0][KEY]
    assert tuple(x.shape) == (3 * 2, L, E) and tuple(batch[0]["progress"].shape) == (6, 1)
    x = x.view(3, 2, L, E)
    for n, (f, T) in enumerate(zip(feats, lens)):
        assert all(np.array_equal(x[t, n].numpy(), f) for t in range(T)), f"trajectory {n} lost its features"
        assert bool((x[T:, n] == 1).all())
    dd = dedupe_instruction_features(batch[0], first_rows=2)
    assert dd[KEY + "_index"].tolist() == [0, 1, 0, 1, 0, 2]
    # a one-step trajectory beside a longer one: its single record is its only timestep
    store.put(2, {KEY: feats[1][None], "progress": g.rand(1, 1)}, np.zeros(1), np.zeros(1))
    x = tour_collate([ds[0], ds[2]])[0][KEY].view(3, 2, L, E)
    assert np.array_equal(x[0, 1].numpy(), feats[1]) and bool((x[1:, 1] == 1).all())


def test_bindings_refuse_operands_the_kernels_would_read_past():
    """ops.text_feat_front / text_feat_gates take every size from the shapes: another dtype, a strided view or operands
    that do not fit each other are refused before anything is launched (no GPU needed)"""
    from ivln_ce_amd import ops
    from ivln_ce_amd._lib import IvlnError

    x, w = torch.zeros(2, 3, 4), torch.zeros(8, 4)
    for bad in (x.double(), x[:, :, ::2], x[0], torch.zeros(0, 3, 4)):
        with pytest.raises(IvlnError):
            ops.text_feat_front(bad)
        with pytest.raises(IvlnError):
            ops.text_feat_gates(bad, w, None)
    for kw in (dict(w=torch.zeros(8, 5)), dict(w=w.t()), dict(w=w, bias=torch.zeros(7)), dict(w=w, out=torch.zeros(6, 7)),
               dict(w=w, out=torch.zeros(5, 8)), dict(w=w, out=torch.zeros(6, 16)[:, ::2]),
               dict(w=w, dirty=torch.zeros(3, dtype=torch.int32)), dict(w=w, dirty=torch.zeros(2, dtype=torch.int64))):
        with pytest.raises(IvlnError):
            ops.text_feat_gates(x, kw.pop("w"), kw.pop("bias", None), **kw)


def test_synthetic_env_emits_deterministic_features():
    from ivln_ce_amd.envs import construct_envs
    from ivln_ce_amd.synthetic import instruction_features
    from text_feat_ref import rxr_config

    cfg = rxr_config("LSTM", True, L=16, E=8)
    cfg.defrost()
    cfg.NUM_ENVIRONMENTS = 2
    cfg.freeze()
    envs = construct_envs(cfg)
    assert KEY in envs.observation_spaces[0].spaces and "instruction" not in envs.observation_spaces[0].spaces
    assert envs.observation_spaces[0].spaces[KEY].shape == (16, 8)
    obs = envs.reset()
    first = obs[0][0] if isinstance(obs[0], tuple) else obs[0]
    ep = envs.current_episodes()[0]
    f = first[KEY]
    assert f.shape == (16, 8) and f.dtype == np.float32 and "instruction" not in first
    n = min(int(np.count_nonzero(ep.tokens)), 16)
    assert np.array_equal(f, instruction_features(ep.tokens, 16, 8))
    assert bool((f[:n] != 0).any(1).all()) and bool((f[n:] == 0).all())
    # default observations and spaces do not move
    from ivln_ce_amd.config import get_config

    envs0 = construct_envs(get_config(opts=["NUM_ENVIRONMENTS", 1]))
    o0 = envs0.reset()[0]
    o0 = o0[0] if isinstance(o0, tuple) else o0
    assert "instruction" in o0 and KEY not in o0 and KEY not in envs0.observation_spaces[0].spaces
