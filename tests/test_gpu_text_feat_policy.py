"""GPU: MapCMA and Latent-CMA built from an RxR config (`MODEL.INSTRUCTION_ENCODER.sensor_uuid = "rxr_instruction"`, (512, 768)
pre-computed text features): rollout step against the torch oracles of tests/instr_rnn_ref.py with the instruction encoder
swapped (tests/text_feat_ref.py), the fused recurrent head at L = 512, one update's gradients with and without the
de-duplicated feature batch, hipGraph replay over an episode change, re-encoding after an optimizer step; MapCMA with LSTM state encoders (the other
fused head) against tests/lstm_state_ref.py's oracle.

Bounds (those tests/test_gpu_instruction_options.py holds for the same quantities):
  policy    logits 1e-4, features / states 2e-4 (its lines 12, 304, 533); argmax gap 2e-4 (305); the same figures for LSTM
            state encoders: tests/test_gpu_lstm_state.py
  update    loss 2e-5 (355); gradients err <= 4 * e32 + 4 * 2^-24 * max|ref|, e32 = the oracle's float32 run (10-11, 360-363)
  dedupe    loss 1e-6, gradients 1e-5 * max(1, max|g|): tests/test_gpu_train.py:563-567 (what the token path promises)
"""
import pytest
import torch

from kernel_bar import _Bar, _same_bytes
from text_feat_ref import KEY, LatentRxrRef, MapCMALSTMRxrRef, make_rxr_policy, mapcma_rxr_oracle, patterned_features

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOG = "text_feat_policy.log"
L_RXR, E_RXR = 512, 768
PAIRS = [("LSTM", True), ("GRU", False)]


def _rollout_obs(B, steps, seed, with_rgb=False):
    """SyntheticRollout observations with (512, 768) features on the device; row 1's features are cut to 11 rows"""
    from ivln_ce_amd.synthetic import SyntheticRollout

    roll = SyntheticRollout(B=B, seed=seed, with_rgb=with_rgb, text_features=(L_RXR, E_RXR))
    obs = []
    for _ in range(steps):
        o = roll.step()
        assert "instruction" not in o and tuple(o[KEY].shape) == (B, L_RXR, E_RXR)
        o[KEY][1, 11:] = 0
        obs.append({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in o.items()})
    return obs


def _mapcma_oracle_for(pol, cell, bidirectional, E, use_pm=False):
    ref = mapcma_rxr_oracle(cell, bidirectional, E, use_pm=use_pm)
    ref.load_state_dict({k: v.cpu() for k, v in pol.state_dict().items()})  # strict: the reference's keys, no embedding
    return ref


@pytest.mark.parametrize("cell,bidirectional", PAIRS)
def test_mapcma_step_matches_the_oracle_and_takes_the_fused_head(cell, bidirectional, monkeypatch):
    from ivln_ce_amd import ops
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.obs_transforms import GTSemanticsIterativeMapper

    torch.set_num_threads(8)
    B = 2
    pol = make_rxr_policy(cell, bidirectional).to(DEV).eval()
    assert pol.net.fused_head_form == "gru"
    ref = _mapcma_oracle_for(pol, cell, bidirectional, E_RXR).eval()
    fused = []
    real = ops.cma_step
    monkeypatch.setattr(ops, "cma_step", lambda d: (fused.append((d.Ct, d.L)), real(d))[1])
    feats = {}
    pol.net.register_forward_hook(lambda mod, args, o: feats.__setitem__("f", o[0]))
    b = GTSemanticsIterativeMapper.from_config(get_config())(dict(_rollout_obs(B, 1, seed=77)[0]))
    masks = b["not_done_masks"]
    rnn, prev = torch.zeros(B, 2, 512), torch.zeros(B, 1, dtype=torch.long)
    with torch.no_grad():
        a, rnn_d = pol.act(b, rnn.to(DEV), prev.to(DEV), masks, deterministic=True)
        lg = pol.action_distribution.raw_logits(feats["f"])
        cpu = {k: b[k].cpu() for k in ("depth", "occupancy_map", "semantic_map", KEY)}
        lr, rnn_r, fr = ref.logits(cpu, rnn, prev, masks.cpu())
    e_l, e_f = float((lg.cpu() - lr).abs().max()), float((feats["f"].cpu() - fr).abs().max())
    e_s = float((rnn_d.cpu() - rnn_r).abs().max())
    print(f"{cell} bidirectional={bidirectional} act: logits {e_l:.3e} features {e_f:.3e} states {e_s:.3e}")
    assert fused == [(pol.net.instruction_encoder.output_size, L_RXR)], fused  # the fused head, at L = 512
    assert pol.net.instruction_encoder.last_cache is not None
    assert e_l < 1e-4 and e_f < 2e-4 and e_s < 2e-4
    assert float((lr.max(-1, keepdim=True).values - lr.gather(1, a.cpu())).max()) < 2e-4


@pytest.mark.parametrize("cell,bidirectional", PAIRS)
def test_mapcma_with_lstm_state_encoders_takes_the_lstm_fused_head(cell, bidirectional, monkeypatch):
    """`MODEL.STATE_ENCODER.rnn_type: LSTM` with features: two steps (the second with a carried (h, c) state and env 1
    reset) against tests/lstm_state_ref.py's oracle with the instruction encoder swapped; the fused head is
    ivln_cma_step_lstm_fwd at (Ct, 512), the GRU form does not run"""
    from ivln_ce_amd import ops
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.obs_transforms import GTSemanticsIterativeMapper

    torch.set_num_threads(8)
    B = 2
    pol = make_rxr_policy(cell, bidirectional, state_rnn="LSTM").to(DEV).eval()
    assert pol.net.fused_head_form == "lstm" and pol.net.num_recurrent_layers == 4
    ref = MapCMALSTMRxrRef(cell, bidirectional, E_RXR)
    ref.load_state_dict({k: v.cpu() for k, v in pol.state_dict().items()})  # strict
    ref.eval()
    fused, gru = [], []
    real, real_gru = ops.cma_step_lstm, ops.cma_step
    monkeypatch.setattr(ops, "cma_step_lstm", lambda d, mode=None: (fused.append((d.Ct, d.L)), real(d, mode))[1])
    monkeypatch.setattr(ops, "cma_step", lambda d, mode=None: (gru.append(d.Ct), real_gru(d, mode))[1])
    feats = {}
    pol.net.register_forward_hook(lambda mod, args, o: feats.__setitem__("f", o[0]))
    tr = GTSemanticsIterativeMapper.from_config(get_config())
    rnn, prev = torch.zeros(B, 4, 512), torch.zeros(B, 1, dtype=torch.long)
    for t, o in enumerate(_rollout_obs(B, 2, seed=78)):
        if t == 1:
            o["not_done_masks"] = torch.tensor([[1], [0]], dtype=torch.uint8, device=DEV)
        b = tr(dict(o))
        masks = b["not_done_masks"]
        with torch.no_grad():
            a, rnn_d = pol.act(b, rnn.to(DEV), prev.to(DEV), masks, deterministic=True)
            lg = pol.action_distribution.raw_logits(feats["f"])
            cpu = {k: b[k].cpu() for k in ("depth", "occupancy_map", "semantic_map", KEY)}
            lr, rnn_r, fr = ref.logits(cpu, rnn, prev, masks.cpu())
        e_l, e_f = float((lg.cpu() - lr).abs().max()), float((feats["f"].cpu() - fr).abs().max())
        e_s = float((rnn_d.cpu() - rnn_r).abs().max())
        print(f"LSTM state, {cell} bidirectional={bidirectional} step {t}: logits {e_l:.3e} features {e_f:.3e} states {e_s:.3e}")
        assert e_l < 1e-4 and e_f < 2e-4 and e_s < 2e-4
        assert float((lr.max(-1, keepdim=True).values - lr.gather(1, a.cpu())).max()) < 2e-4
        rnn, prev = rnn_r, a.cpu()
    assert fused == [(pol.net.instruction_encoder.output_size, L_RXR)] * 2 and gru == [], (fused, gru)
    assert pol.net.instruction_encoder.last_cache.dirty.tolist() == [0, 0]  # (step 2 re-encoded nothing)


@pytest.mark.parametrize("cell,bidirectional", PAIRS)
def test_latent_step_matches_the_oracle(cell, bidirectional):
    torch.set_num_threads(8)
    N = 3
    pol = make_rxr_policy(cell, bidirectional, "LatentCMAPolicy").to(DEV).eval()
    ref = LatentRxrRef(cell, bidirectional, E_RXR).load_from(pol).eval()
    feats = {}
    pol.net.register_forward_hook(lambda mod, args, o: feats.__setitem__("f", o[0]))
    g = torch.Generator().manual_seed(3)
    obs = {"rgb_features": torch.rand(N, 2048, 4, 4, generator=g), "depth_features": torch.rand(N, 128, 4, 4, generator=g),
           KEY: patterned_features([range(40), range(7), [0] + list(range(2, 30))], L_RXR, E_RXR, seed=8)}
    prev = torch.randint(0, 4, (N, 1), generator=g)
    nd = torch.tensor([[1], [0], [1]], dtype=torch.uint8)
    h0 = 0.1 * torch.randn(N, 2, 512, generator=g)
    with torch.no_grad():
        a, rnn = pol.act({k: v.to(DEV) for k, v in obs.items()}, h0.to(DEV), prev.to(DEV), nd.to(DEV), deterministic=True)
        lg = torch.log_softmax(pol.action_distribution.raw_logits(feats["f"]), -1)
        lr, rnn_r, fr = ref.logits(obs, h0, prev, nd)
    e_l = float((lg.cpu() - torch.log_softmax(lr, -1)).abs().max())
    e_f, e_s = float((feats["f"].cpu() - fr).abs().max()), float((rnn.cpu() - rnn_r).abs().max())
    print(f"latent {cell} bidirectional={bidirectional}: logits {e_l:.3e} features {e_f:.3e} states {e_s:.3e}")
    assert pol.net.instruction_encoder.last_cache is not None
    assert e_l < 1e-4 and e_f < 2e-4 and e_s < 2e-4
    assert float((lr.max(-1, keepdim=True).values - lr.gather(1, a.cpu())).max()) < 2e-4


# ------------------------------------------------------------------------------------------------------------------
# updates (small features: L = 24, E = 16 - the update path has no shape-dependent branch in L or E)
# ------------------------------------------------------------------------------------------------------------------
L_UP, E_UP = 24, 16


def _update_batch(T, N, latent=False, seed=42):
    g = torch.Generator().manual_seed(seed)
    TN = T * N
    feat = patterned_features([range(20 - 7 * n) for n in range(N)], L_UP, E_UP, seed=seed + 1)
    obs = {"depth_features": torch.randn(TN, 128, 4, 4, generator=g), KEY: feat.repeat(T, 1, 1)}
    if latent:
        obs["rgb_features"] = torch.rand(TN, 2048, 4, 4, generator=g)
    else:
        obs.update(occupancy_map=(torch.rand(TN, 64, 64, generator=g) < 0.3).float(),
                   semantic_map=torch.randint(0, 13, (TN, 64, 64), generator=g).float(), progress=torch.rand(TN, 1, generator=g))
    prev = torch.randint(0, 4, (TN, 1), generator=g)
    nd = torch.ones(T, N, dtype=torch.uint8)
    nd[0] = 0
    tgt = torch.randint(0, 4, (T, N), generator=g)
    w = torch.where(torch.rand(T, N, generator=g) < 0.5, torch.tensor(3.2), torch.tensor(1.0))
    return obs, prev, nd.view(-1, 1), tgt, w


def _instruction_names(params):
    return [k for k in params if k.startswith("net.instruction_encoder.") or k.startswith(("net.text_k.", "net.text_q."))]


@pytest.mark.parametrize("cell,bidirectional", PAIRS)
def test_mapcma_update_gradients_with_and_without_the_deduplicated_batch(cell, bidirectional):
    """one `update_agent` at T = 3, N = 2 with the last timestep of trajectory 1 padded (all ones, zero weight): the
    gradients of the instruction encoder and of text_k / text_q (downstream of it) against float64 autograd of the
    oracle's loss; then the same update on the de-duplicated batch"""
    from ivln_ce_amd.aux_losses import AuxLosses
    from ivln_ce_amd.trainers import FlatAdam, update_agent
    from ivln_ce_amd.utils import dedupe_instruction_features

    torch.set_num_threads(8)
    T, N = 3, 2
    obs, prev, nd, tgt, w = _update_batch(T, N)
    w[2, 1] = 0
    for k in obs:
        obs[k].view(T, N, *obs[k].shape[1:])[2, 1] = 1.0
    pol = make_rxr_policy(cell, bidirectional, use_pm=True, L=L_UP, E=E_UP).to(DEV).train()
    grads = {}
    for dt in (torch.float64, torch.float32):
        ref = _mapcma_oracle_for(pol, cell, bidirectional, E_UP, use_pm=True).train().to(dt)
        torch.set_default_dtype(dt)  # (tensors the oracle creates itself: initial state, one-hot maps)
        try:
            loss_r, _, _, _ = ref.update_loss({k: v.to(dt) for k, v in obs.items()}, prev, nd, tgt, w.to(dt))
            loss_r.backward()
        finally:
            torch.set_default_dtype(torch.float32)
        grads[dt] = {k: p.grad.detach() for k, p in ref.named_parameters() if p.grad is not None}
        if dt == torch.float64:
            loss64 = float(loss_r.detach())
    dd = dedupe_instruction_features(dict(obs), first_rows=N)
    assert dd[KEY + "_index"].tolist() == [0, 1, 0, 1, 0, 2]
    res = []
    for host in (obs, dd):
        opt = FlatAdam(pol, lr=2.5e-4)
        AuxLosses.activate()
        try:
            loss, _, _ = update_agent(pol, opt, {k: v.float().to(DEV) for k, v in host.items()}, prev.to(DEV), nd.to(DEV),
                                      tgt.to(DEV), w.to(DEV), hidden_size=512, step_grad=False)
        finally:
            AuxLosses.deactivate()
        res.append((loss, {k: p.grad.detach().clone() for k, p in pol.named_parameters() if p.requires_grad}))
    (l0, g0), (l1, g1) = res
    print(f"{cell} bidirectional={bidirectional} update: loss {l0:.7f} deduplicated {l1:.7f} ref {loss64:.7f}")
    assert abs(l0 - loss64) < 2e-5 and abs(l0 - l1) < 1e-6
    names = _instruction_names(g0)
    assert len(names) == 4 * (2 if bidirectional else 1) + 4 and not any("embedding_layer" in k for k in g0)
    bar = _Bar(f"mapcma {cell} bidir={int(bidirectional)} update", LOG)
    for k in names:
        bar.check(k[4:], g0[k], grads[torch.float64][k], grads[torch.float32][k])
    bar.done()
    for k in g0:
        d, tol = float((g0[k] - g1[k]).abs().max()), 1e-5 * max(1.0, float(g0[k].abs().max()))
        assert d <= tol, (k, d, tol)


def test_latent_update_gradients_of_the_instruction_branch():
    import torch.nn.functional as F

    torch.set_num_threads(8)
    cell, bidirectional = "LSTM", True
    T, N = 3, 2
    obs, prev, nd, tgt, w = _update_batch(T, N, latent=True, seed=7)
    pol = make_rxr_policy(cell, bidirectional, "LatentCMAPolicy", L=L_UP, E=E_UP).to(DEV).train()
    grads = {}
    for dt in (torch.float64, torch.float32):
        ref = LatentRxrRef(cell, bidirectional, E_UP).load_from(pol).train().to(dt)
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
    print(f"latent update: loss {float(loss.detach()):.7f} ref {loss64:.7f}")
    assert abs(float(loss.detach()) - loss64) < 2e-5
    params = dict(pol.named_parameters())
    names = _instruction_names(params)
    assert len(names) == 8 + 4 and all(params[k].grad is not None and k in grads[torch.float64] for k in names)
    bar = _Bar("latent LSTM bidir=1 update", LOG)
    for k in names:
        bar.check(k[4:], params[k].grad, grads[torch.float64][k], grads[torch.float32][k])
    bar.done()


# ------------------------------------------------------------------------------------------------------------------
# graph replay, optimizer step
# ------------------------------------------------------------------------------------------------------------------
def _swap_episode(obs):
    """env 0 starts another episode at step 1: its features change, env 1's do not"""
    from ivln_ce_amd.synthetic import instruction_features

    new = torch.from_numpy(instruction_features(list(range(5, 45)), L_RXR, E_RXR)).to(DEV)
    obs[1][KEY] = obs[1][KEY].clone()
    obs[1][KEY][0] = new
    obs[2][KEY] = obs[1][KEY].clone()


def test_mapcma_graph_replay_over_an_episode_change_is_bit_identical_to_eager(same_depth_path):
    same_depth_path(0)
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.graphed import GraphedRollout
    from ivln_ce_amd.obs_transforms import GTSemanticsIterativeMapper

    B, steps = 2, 3
    pol = make_rxr_policy("LSTM", True).to(DEV).eval()
    cfg = get_config()
    obs = _rollout_obs(B, steps, seed=31)
    _swap_episode(obs)
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
    tr_g = GTSemanticsIterativeMapper.from_config(cfg)
    runner = GraphedRollout(pol, [tr_g], obs[0], deterministic=True)
    assert KEY in runner.static
    tr_g.mapping_module.reset()
    runner.reset_state()
    for t, o in enumerate(obs):
        a = runner.step(o)
        torch.cuda.synchronize()
        assert torch.equal(a, eager[t][0]), f"actions step {t}"
        assert torch.equal(runner.rnn_states, eager[t][1]), f"rnn step {t}"
    tr_g.mapping_module.check_status()


def test_latent_graph_replay_over_an_episode_change_is_bit_identical_to_eager(same_depth_path):
    same_depth_path(0)
    from ivln_ce_amd.graphed import GraphedRollout

    B, steps = 2, 3
    pol = make_rxr_policy("GRU", False, "LatentCMAPolicy").to(DEV).eval()
    obs = _rollout_obs(B, steps, seed=11, with_rgb=True)
    _swap_episode(obs)
    rnn = torch.zeros(B, 2, 512, device=DEV)
    prev = torch.zeros(B, 1, dtype=torch.long, device=DEV)
    eager, dirty = [], []
    for o in obs:
        with torch.no_grad():
            a, rnn = pol.act(o, rnn, prev, o["not_done_masks"], deterministic=True)
        prev = a
        eager.append((a.clone(), rnn.clone()))
        dirty.append(pol.net.instruction_encoder.last_cache.dirty.tolist())
    assert dirty == [[1, 1], [1, 0], [0, 0]], dirty
    runner = GraphedRollout(pol, [], obs[0], deterministic=True)
    runner.reset_state()
    for t, o in enumerate(obs):
        a = runner.step(o)
        torch.cuda.synchronize()
        assert torch.equal(a, eager[t][0]), f"actions step {t}"
        assert torch.equal(runner.rnn_states, eager[t][1]), f"rnn step {t}"


def test_an_optimizer_step_is_followed_by_a_re_encoding(monkeypatch):
    """FlatAdam.step writes the parameters through raw pointers: the step caches are invalidated, the next `act`
    re-encodes every row and sees the new weights - its features are the uncached chain's, byte for byte"""
    from ivln_ce_amd import ops
    from ivln_ce_amd.aux_losses import AuxLosses
    from ivln_ce_amd.trainers import FlatAdam, update_agent

    T, N = 3, 2
    pol = make_rxr_policy("LSTM", True, use_pm=True, L=L_UP, E=E_UP).to(DEV)
    opt = FlatAdam(pol, lr=1e-2)
    obs, prev, nd, tgt, w = _update_batch(T, N, seed=7)
    step = {k: v[:N].to(DEV) for k, v in obs.items()}
    h0, p0 = torch.zeros(N, 2, 512, device=DEV), torch.zeros(N, 1, dtype=torch.long, device=DEV)
    m0 = torch.zeros(N, 1, dtype=torch.uint8, device=DEV)
    feats = {}
    pol.net.register_forward_hook(lambda mod, args, o: feats.__setitem__("f", o[0].clone()))

    def act():
        pol.eval()
        with torch.no_grad():
            pol.act(step, h0, p0, m0, deterministic=True)
        return feats["f"]

    enc = pol.net.instruction_encoder
    f0 = act()
    assert enc.last_cache.dirty.tolist() == [1, 1]
    assert _same_bytes(act(), f0) and enc.last_cache.dirty.tolist() == [0, 0]
    pol.train()
    AuxLosses.activate()
    try:
        update_agent(pol, opt, {k: v.to(DEV) for k, v in obs.items()}, prev.to(DEV), nd.to(DEV), tgt.to(DEV), w.to(DEV),
                     hidden_size=512, step_grad=True)
    finally:
        AuxLosses.deactivate()
    f1 = act()
    assert enc.last_cache.dirty.tolist() == [1, 1] and not torch.equal(f1, f0)
    monkeypatch.setattr(ops, "CACHE_INSTRUCTION", False)
    assert _same_bytes(act(), f1) and enc.last_cache is None
