"""GPU: MODEL.DEPTH_ENCODER.trainable - the hand-written backward of the depth ResNet (ResNetEncoder.forward_train +
train.depth_encoder_backward) and its wiring into the update path.

Reference for the encoder's 162 gradients: the mask-frozen float64 twin (tests/depth_twin.py; tests/test_depth_twin.py pins
why free float64 autograd cannot serve), with the masks and pool indices taken from the HIP forward's saved tensors.
Bar: the project's gradient bar of tests/test_gpu_train.py, per tensor max|got - ref| <= 1e-3 max|ref| + 2e-7 and direction
cosine >= 1 - 1e-6.  Each comparison is written to the suite's log directory (kernel_bar._log_dir) before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "golden"))
import depth_twin as DT  # noqa: E402

DEV = torch.device("cuda:0")


def _write(name, lines):
    from kernel_bar import _log_dir

    os.makedirs(_log_dir(), exist_ok=True)
    open(os.path.join(_log_dir(), name), "w").write("\n".join(lines) + "\n")


def _encoder(seed=5):
    """tests/test_gpu_depth_net.py's encoder (GroupNorm affine randomised), trainable"""
    from ivln_ce_amd.encoders import ResNetEncoder

    torch.manual_seed(seed)
    enc = ResNetEncoder((256, 256, 1)).eval()
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.normal_(1.0, 0.2)
                m.bias.normal_(0.0, 0.2)
    return enc.to(DEV)


# ------------------------------------------------------------------------------------------------
# 3. the encoder alone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 1])
def test_encoder_backward_all_162_tensors_against_the_frozen_twin(B):
    from ivln_ce_amd import ops, train

    enc = _encoder()
    assert enc.trains and len(list(enc.parameters())) == 162
    g = torch.Generator().manual_seed(40 + B)
    depth = torch.rand(B, 256, 256, 1, generator=g)
    d_feats = torch.randn(B, 128, 4, 4, generator=g)
    d = depth.to(DEV)
    save = {}
    with torch.no_grad():
        feats = enc({"depth": d}, save=save).clone()
        old = ops.DEPTH_NET
        try:
            ops.DEPTH_NET = 0
            chain = enc({"depth": d}).clone()  # the launch chain the rollout takes for a trainable encoder
        finally:
            ops.DEPTH_NET = old
    e_chain = float((feats - chain).abs().max())
    assert sorted(save) == ["blocks", "comp", "stem"] and len(save["blocks"]) == 16
    masks, pool_idx = DT.masks_from_saves(save)
    G = {}
    with torch.no_grad():
        train.depth_encoder_backward(enc, save, d_feats.to(DEV), G)
    torch.cuda.synchronize()
    assert not save, "the saves are released as the backward walks them"
    names = {p: k for k, p in enc.named_parameters()}
    got = {names[p]: v for p, v in G.items()}
    assert len(got) == 162
    for k, p in enc.named_parameters():
        assert got[k].shape == p.shape, k
    ref, feats64 = DT.twin_gradients(enc.state_dict(), depth, masks, pool_idx, d_feats)
    e_fwd = float((feats.cpu().double() - feats64).abs().max())
    log, bad = DT.compare(got, ref)
    _write(f"depth_encoder_bwd_B{B}.log", [f"forward_train vs launch chain {e_chain:.3e}; vs the twin's float64 forward {e_fwd:.3e}"] + log)
    print(f"B={B}: forward_train vs chain {e_chain:.2e}, vs twin forward {e_fwd:.2e}; {len(bad)} of 162 over the bar")
    assert e_chain < 2e-4, e_chain
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------
# 4. / 5. the policies
# ------------------------------------------------------------------------------------------------
def _map_cma(trainable=True, **kw):
    from det_init import det_fill

    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.policy import MapCMAPolicy
    from ivln_ce_amd.spaces import Box, Dict, Discrete

    opts = ["MODEL.policy_name", "MapCMAPolicy", "MODEL.INSTRUCTION_ENCODER.use_pretrained_embeddings", False,
            "MODEL.DEPTH_ENCODER.ddppo_checkpoint", "NONE", "MODEL.PROGRESS_MONITOR.use", True,
            "MODEL.DEPTH_ENCODER.trainable", trainable] + [x for k, v in kw.items() for x in (k, v)]
    space = Dict({"depth": Box(0.0, 1.0, (256, 256, 1), np.float32), "occupancy_map": Box(0, 255, (64, 64), np.uint8),
                  "semantic_map": Box(0, 255, (64, 64), np.uint8), "instruction": Box(0, 2504, (200,), np.int64)})
    pol = MapCMAPolicy.from_config(get_config(opts=opts), space, Discrete(4))
    det_fill(pol, seed=0)
    return pol.to(DEV).train()


def _batch(T=2, N=2, seed=3):
    g = torch.Generator().manual_seed(seed)
    TN = T * N
    instr = torch.zeros(N, 200)
    for n in range(N):
        L = 30 - 13 * n
        instr[n, :L] = torch.randint(2, 2504, (L,), generator=g).float()
    obs = {"depth": torch.rand(TN, 256, 256, 1, generator=g),
           "occupancy_map": (torch.rand(TN, 64, 64, generator=g) < 0.3).float(),
           "semantic_map": torch.randint(0, 13, (TN, 64, 64), generator=g).float(),
           "instruction": instr.repeat(T, 1), "progress": torch.rand(TN, 1, generator=g)}
    prev = torch.randint(0, 4, (TN, 1), generator=g)
    nd = torch.ones(T, N, dtype=torch.uint8)
    nd[0] = 0
    tgt = torch.randint(0, 4, (T, N), generator=g)
    w = torch.where(torch.rand(T, N, generator=g) < 0.5, torch.tensor(3.2), torch.tensor(1.0))
    return dict(T=T, N=N, obs=obs, prev=prev, nd=nd.view(-1, 1), tgt=tgt, w=w)


class _Recorded:
    """train.depth_encoder_backward with its upstream gradient, and the masks of the saves it is about to release, kept"""

    def __init__(self, monkeypatch):
        from ivln_ce_amd import train

        self.calls, orig = [], train.depth_encoder_backward

        def wrapper(ve, save, d_feats, G):
            masks, pool_idx = DT.masks_from_saves(save)
            self.calls.append(dict(masks=masks, pool_idx=pool_idx, d_feats=d_feats.detach().cpu().clone()))
            return orig(ve, save, d_feats, G)

        monkeypatch.setattr(train, "depth_encoder_backward", wrapper)


def _update(pol, c, step_grad=False, opt=None):
    from ivln_ce_amd.aux_losses import AuxLosses
    from ivln_ce_amd.trainers import FlatAdam, update_agent

    opt = opt or FlatAdam(pol, lr=2.5e-4)
    dobs = {k: v.to(DEV) for k, v in c["obs"].items()}
    AuxLosses.activate()
    try:
        out = update_agent(pol, opt, dobs, c["prev"].to(DEV), c["nd"].to(DEV), c["tgt"].to(DEV), c["w"].to(DEV),
                           hidden_size=512, step_grad=step_grad)
    finally:
        AuxLosses.deactivate()
    torch.cuda.synchronize()
    return opt, out


def _encoder_grads_vs_twin(ve, rec, depth, logname):
    assert len(rec.calls) == 1, "depth_encoder_backward runs once per update"
    r = rec.calls[0]
    assert float(r["d_feats"].abs().max()) > 0
    ref, _ = DT.twin_gradients(ve.state_dict(), depth, r["masks"], r["pool_idx"], r["d_feats"])
    got = {k: p.grad for k, p in ve.named_parameters()}
    assert all(v is not None for v in got.values()) and len(got) == 162
    log, bad = DT.compare(got, ref)
    _write(logname, log)
    assert not bad, "\n".join(bad)


def test_map_cma_update_trains_the_depth_encoder(monkeypatch):
    """update_agent(step_grad=False) of MapCMAPolicy with DEPTH_ENCODER.trainable at T = 2, N = 2: every depth-encoder
    .grad against the twin under the upstream gradient that reached depth_encoder_backward (zero before this feature);
    every other parameter against the oracle's free fp32 autograd, its encoder un-frozen here, as the T64 x N8 test does."""
    from oracle.policy_ref import MapCMAPolicyRef

    c = _batch()
    pol = _map_cma(True)
    ve = pol.net.depth_encoder.visual_encoder
    assert all(p.requires_grad for p in ve.parameters())
    rec = _Recorded(monkeypatch)
    opt, (loss, act, aux) = _update(pol, c)
    assert sum(n.startswith("net.depth_encoder.visual_encoder.") for n in opt.names) == 162
    _encoder_grads_vs_twin(ve, rec, c["obs"]["depth"], "depth_trainable_mapcma_encoder.log")

    torch.set_num_threads(8)
    ref = MapCMAPolicyRef(use_pm=True).train()
    ref.load_state_dict({k: v.detach().cpu() for k, v in pol.state_dict().items()})
    for p in ref.net.depth_encoder.visual_encoder.parameters():
        p.requires_grad_(True)
    loss_r, _, aux_r, _ = ref.update_loss(c["obs"], c["prev"], c["nd"], c["tgt"], c["w"])
    loss_r.backward()
    assert abs(loss - float(loss_r)) < 2e-5 and abs(aux - float(aux_r)) < 2e-5, (loss, float(loss_r), aux, float(aux_r))
    rg = {k: p.grad for k, p in ref.named_parameters() if p.grad is not None}
    got, want = {}, {}
    for k, p in pol.named_parameters():
        if k.startswith("net.depth_encoder.visual_encoder.") or not p.requires_grad or k not in rg:
            continue
        if k.startswith("net.map_encoder.cnn.") and k.endswith(".conv.0.bias"):
            assert float(p.grad.abs().max()) == 0.0, k  # (analytically zero under train-mode BatchNorm)
            continue
        got[k], want[k] = p.grad, rg[k]
    assert len(got) >= 40
    log, bad = DT.compare(got, want)
    _write("depth_trainable_mapcma_others.log", log)
    assert not bad, "\n".join(bad)


def test_ablated_depth_branch_gives_exactly_zero_encoder_gradients(monkeypatch):
    c = _batch()
    pol = _map_cma(True, **{"MODEL.ablate_depth": True})
    rec = _Recorded(monkeypatch)
    _update(pol, c)
    assert not rec.calls, "the features are multiplied by 0: the encoder's backward is skipped"
    for k, p in pol.net.depth_encoder.visual_encoder.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) == 0.0, k


def test_latent_cma_update_trains_the_depth_encoder(monkeypatch):
    from det_init import det_fill
    from gen_latent_update_features import features

    from ivln_ce_amd import latent_policy  # noqa: F401
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.registry import baseline_registry
    from ivln_ce_amd.spaces import Box, Dict, Discrete
    from ivln_ce_amd.trainers import FlatAdam

    cfg = get_config(opts=["MODEL.policy_name", "LatentCMAPolicy", "MODEL.INSTRUCTION_ENCODER.use_pretrained_embeddings", False,
                           "MODEL.DEPTH_ENCODER.ddppo_checkpoint", "NONE", "MODEL.DEPTH_ENCODER.trainable", True])
    space = Dict({"depth": Box(0.0, 1.0, (256, 256, 1), np.float32), "rgb": Box(0, 255, (224, 224, 3), np.uint8),
                  "instruction": Box(0, 2504, (200,), np.int64)})
    pol = baseline_registry.get_policy("LatentCMAPolicy").from_config(cfg, space, Discrete(4))
    det_fill(pol, seed=0, conv_gain=1.0)
    pol = pol.to(DEV).train()
    ve = pol.net.depth_encoder.visual_encoder
    c = _batch()
    T, N = c["T"], c["N"]
    rgb_np, _ = features(7, T, N)
    obs = {"rgb_features": torch.from_numpy(rgb_np).to(DEV), "depth": c["obs"]["depth"].to(DEV),
           "instruction": c["obs"]["instruction"].to(DEV)}
    FlatAdam(pol, lr=2.5e-4)  # (every trainable parameter owns a .grad in the flat bucket)
    rec = _Recorded(monkeypatch)
    h0 = torch.zeros(N, pol.net.num_recurrent_layers, 512, device=DEV)
    ep = c["nd"].to(DEV)
    dist, _ = pol.build_distribution(obs, h0, c["prev"].to(DEV), ep, ep)
    logits = dist.logits.view(T, N, -1)
    ce = torch.nn.functional.cross_entropy(logits.permute(0, 2, 1), c["tgt"].to(DEV), reduction="none")
    w = c["w"].to(DEV)
    ((w * ce).sum(0) / w.sum(0)).mean().backward()
    torch.cuda.synchronize()
    _encoder_grads_vs_twin(ve, rec, c["obs"]["depth"], "depth_trainable_latent_encoder.log")


# ------------------------------------------------------------------------------------------------
# 5. the weights move, and every later forward sees them
# ------------------------------------------------------------------------------------------------
def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_two_adam_steps_move_the_encoder_and_the_next_forwards_see_the_new_weights():
    c = _batch()
    pol = _map_cma(True)
    ve = pol.net.depth_encoder.visual_encoder
    start = {k: v.detach().clone() for k, v in ve.state_dict().items()}
    dobs = {k: v.to(DEV) for k, v in c["obs"].items()}
    N = c["N"]
    step_obs = {k: v[:N] for k, v in dobs.items()}
    rnn = torch.zeros(N, 2, 512, device=DEV)
    prev, nd = c["prev"].to(DEV), c["nd"].to(DEV)
    with torch.no_grad():  # (fills every cache an act leaves behind - packed weights, the output buffer - with the OLD weights)
        pol.act(step_obs, rnn, prev[:N], nd[:N], deterministic=True)
    opt, _ = _update(pol, c, step_grad=True)
    _update(pol, c, step_grad=True, opt=opt)
    moved = [k for k, v in ve.state_dict().items() if not torch.equal(v, start[k])]
    assert len(moved) == 162, f"{162 - len(moved)} encoder tensors did not move"

    fresh = _map_cma(True)
    fresh.load_state_dict({k: v.detach().clone() for k, v in pol.state_dict().items()})
    with torch.no_grad():
        a_act, a_rnn = pol.act(step_obs, rnn, prev[:N], nd[:N], deterministic=True)
        b_act, b_rnn = fresh.act(step_obs, rnn, prev[:N], nd[:N], deterministic=True)
        a_dep = pol.net.depth_encoder(step_obs).clone()
        b_dep = fresh.net.depth_encoder(step_obs).clone()
    assert _same(a_dep, b_dep), "the rollout's depth features are those of the updated weights"
    assert torch.equal(a_act, b_act) and _same(a_rnn, b_rnn)
    h0 = torch.zeros(N, 2, 512, device=DEV)
    with torch.enable_grad():  # the next update's forward (MapCMAForwardFn -> forward_train)
        a_f, a_s = pol.build_features(dobs, h0, prev, nd)
        b_f, b_s = fresh.build_features(dobs, h0, prev, nd)
    assert _same(a_f.detach(), b_f.detach()) and _same(a_s, b_s)


def test_frozen_encoder_takes_no_saves_and_no_gradients(monkeypatch):
    """trainable False (the default): the update's forward takes the frozen path it always took - no per-layer saves, no
    encoder entry in G, depth_encoder_backward never called - and two updates from the same state return the same losses
    (the forward is bit-stable; the embedding gradient's float atomics are not, so the gradients are not compared)."""
    from ivln_ce_amd import train

    c = _batch()
    seen = {}
    orig = train._net_backward

    def spy(net, S, d_feats):
        G = orig(net, S, d_feats)
        enc = {id(p) for p in net.depth_encoder.visual_encoder.parameters()}
        seen.update(saves=S.get("depth_enc"), enc_in_G=sum(id(p) in enc for p in G), calls=seen.get("calls", 0) + 1)
        return G

    monkeypatch.setattr(train, "_net_backward", spy)
    rec = _Recorded(monkeypatch)
    grads = []
    for _ in range(2):
        pol = _map_cma(False)
        assert not pol.net.depth_encoder.visual_encoder.trains
        opt, out = _update(pol, c)
        assert all(p.grad is None for p in pol.net.depth_encoder.visual_encoder.parameters())
        grads.append(out)
    assert seen["calls"] == 2 and seen["saves"] is None and seen["enc_in_G"] == 0 and not rec.calls
    assert grads[0] == grads[1]
