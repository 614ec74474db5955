"""GPU: MODEL.RGB_ENCODER.trainable - the train-mode forward and the hand-written backward of the RGB ResNet-50
(_ResNet50Body.forward_train + train.rgb_encoder_backward) and its wiring into LatentCMANet's update path.

Reference for the encoder's gradients: the mask-frozen float64 twin (tests/rgb_twin.py; tests/test_rgb_twin.py pins why free
float64 autograd cannot serve), with the masks and pool indices taken from the HIP forward's saved tensors.
Bar per tensor: the project's gradient bar of tests/test_gpu_train.py (max|got - ref| <= 1e-3 max|ref| + 2e-7, direction
cosine >= 1 - 1e-6); where torch's own fp32 autograd on the CPU is near that bar against ITS twin on the same inputs
(BatchNorm over a handful of values amplifies rounding), 4 x that error instead (rgb_twin.compare_with_allowance).  The
forward and the running statistics: 4 x what torch's fp32 pass is away from its twin + 2e-5 max|ref|, the bar the frozen
path of this network is held to (tests/test_gpu_latent.py: 2e-4 at features up to 10).  Every figure is written to the
suite's log directory before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "golden"))
import rgb_twin as RT  # noqa: E402

DEV = torch.device("cuda:0")
FWD_REL = 2e-5  # (tests/test_gpu_latent.py: 2e-4 abs at features up to 10, the conv stack's own bar)


def _write(name, lines):
    from kernel_bar import _log_dir

    os.makedirs(_log_dir(), exist_ok=True)
    open(os.path.join(_log_dir(), name), "w").write("\n".join(lines) + "\n")


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _frames(B, H, seed):
    return torch.randint(0, 256, (B, H, H, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


# ------------------------------------------------------------------------------------------------
# the encoder alone
# ------------------------------------------------------------------------------------------------
# B = 3, 64 x 64: the final map is 2 x 2 (windows replicate), layer 4 normalises over 12 values;
# B = 2, 96 x 96: the final map is 3 x 3 with overlapping pool windows
@pytest.mark.parametrize("B,H", [(3, 64), (2, 96)])
def test_encoder_forward_statistics_and_every_gradient_against_the_frozen_twin(B, H):
    from ivln_ce_amd import ops, train
    from ivln_ce_amd.latent_policy import TorchVisionResNet50

    torch.set_num_threads(min(8, torch.get_num_threads()))
    state = {k: v.clone() for k, v in RT.oracle_cnn().state_dict().items()}
    enc = TorchVisionResNet50(256, trainable=True)
    enc.cnn.load_state_dict(state)
    cnn = enc.to(DEV).train().cnn
    n_par = len(list(cnn.parameters()))
    assert cnn.trains and n_par == len(dict(cnn.named_parameters())) == 159
    rgb = _frames(B, H, 40 + B)
    x = RT.to_input(rgb)
    d_feats = torch.randn(B, 2048, 4, 4, generator=torch.Generator().manual_seed(B))
    save = {}
    with torch.no_grad():
        feats = cnn.forward_train(rgb.to(DEV), save).clone()
    assert cnn._epoch != ops.WEIGHT_EPOCH, "the running statistics moved: the frozen path's folded cache is void"
    assert sorted(save) == ["blocks", "pool", "stem"] and len(save["blocks"]) == 16
    masks, pool_idx = RT.masks_from_saves(save)
    bufs = {k: v.detach().cpu().clone() for k, v in cnn.named_buffers()}
    G = {}
    with torch.no_grad():
        train.rgb_encoder_backward(cnn, save, d_feats.to(DEV), G)
    torch.cuda.synchronize()
    assert not save, "the saves are released as the backward walks them"
    names = {p: k for k, p in cnn.named_parameters()}
    got = {names[p]: v for p, v in G.items()}
    assert len(got) == n_par
    for k, p in cnn.named_parameters():
        assert got[k].shape == p.shape, k

    ref, feats64, bufs64 = RT.twin_gradients(state, x, masks, pool_idx, d_feats)
    cpu = RT.fp32_autograd_error(state, x, d_feats)  # torch's own fp32 pass against ITS twin: the arithmetic's noise
    lines, bad = [], []

    def within(what, g, r64, e32):
        err, mx = float((g.double() - r64).abs().max()), float(r64.abs().max())
        bar = 4 * e32 + FWD_REL * mx
        lines.append(f"{what}: max|ref| {mx:.3e} hip {err:.3e} torch-fp32 {e32:.3e} bar {bar:.3e} {'ok' if err <= bar else 'OVER'}")
        if not err <= bar:
            bad.append(lines[-1])

    within("features", feats.cpu(), feats64, float((cpu["feats32"].double() - cpu["feats64"]).abs().max()))
    for k, v in bufs64.items():
        if k.endswith("num_batches_tracked"):
            assert int(bufs[k]) == int(v) == 1, k
        else:
            within(k, bufs[k], v, float((cpu["bufs32"][k].double() - cpu["bufs64"][k]).abs().max()))
    log, over = RT.compare_with_allowance(got, ref, cpu["e32"])
    _write(f"rgb_encoder_bwd_B{B}_{H}.log", lines + log)
    print(f"B={B} {H}x{H}: {len(bad)} forward / statistics figures and {len(over)} of {n_par} gradients over the bar")
    assert not bad, "\n".join(bad)
    assert not over, "\n".join(over)


def test_an_eval_mode_encoder_that_trains_uses_the_running_statistics():
    """BatchNorm in eval mode with trainable parameters: forward_train gives the frozen path's features, leaves the
    running statistics alone and records train=False; the backward is dx = gamma * rstd * dz (the twin in eval mode)."""
    from ivln_ce_amd import train
    from ivln_ce_amd.latent_policy import TorchVisionResNet50

    torch.set_num_threads(min(8, torch.get_num_threads()))
    B, H = 2, 64
    ref_cnn = RT.oracle_cnn()
    with torch.no_grad():
        for m in ref_cnn.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0.0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    state = {k: v.clone() for k, v in ref_cnn.state_dict().items()}
    enc = TorchVisionResNet50(256, trainable=True)
    enc.cnn.load_state_dict(state)
    cnn = enc.to(DEV).eval().cnn
    rgb = _frames(B, H, 9)
    d_feats = torch.randn(B, 2048, 4, 4, generator=torch.Generator().manual_seed(2))
    save = {}
    with torch.no_grad():
        frozen = cnn(rgb.to(DEV)).clone()
        feats = cnn.forward_train(rgb.to(DEV), save).clone()
    assert all(torch.equal(v.cpu(), state[k]) for k, v in cnn.named_buffers())
    assert not save["stem"]["train"] and not any(s["l3"]["train"] for s in save["blocks"])
    masks, pool_idx = RT.masks_from_saves(save)
    G = {}
    with torch.no_grad():
        train.rgb_encoder_backward(cnn, save, d_feats.to(DEV), G)
    names = {p: k for k, p in cnn.named_parameters()}
    got = {names[p]: v for p, v in G.items()}

    def eval_twin(dtype, ms, idx):
        import itertools

        twin = RT.oracle_cnn(state).to(dtype).eval()
        it = itertools.count()
        hooks = [m.register_forward_hook(lambda _m, i, _o: i[0] * ms[next(it)].to(dtype)) for m in RT._relus(twin)]
        hooks.append(twin[3].register_forward_hook(lambda _m, i, o: i[0].flatten(2).gather(2, idx.flatten(2)).view_as(o)))
        f = RT.features(twin, RT.to_input(rgb).to(dtype))
        f.backward(d_feats.to(dtype))
        for h in hooks:
            h.remove()
        return {k: p.grad.detach() for k, p in twin.named_parameters()}, f.detach()

    ref, f64 = eval_twin(torch.float64, masks, pool_idx)
    # torch's fp32 eval pass against its own twin: the allowance's figure
    c32 = RT.oracle_cnn(state).eval()
    f32, m32, i32_ = RT.record_masks(c32, RT.to_input(rgb))
    f32.backward(d_feats)
    t32, t32f = eval_twin(torch.float64, m32, i32_)
    e32 = {k: float((p.grad.double() - t32[k]).abs().max()) for k, p in c32.named_parameters()}
    e_frozen = float((feats - frozen).abs().max())
    e_fwd, e_fwd32 = float((feats.cpu().double() - f64).abs().max()), float((f32.detach().double() - t32f).abs().max())
    log, over = RT.compare_with_allowance(got, ref, e32)
    _write("rgb_encoder_bwd_eval.log", [f"forward_train vs the folded path {e_frozen:.3e}; vs the twin {e_fwd:.3e} "
                                        f"(torch fp32: {e_fwd32:.3e})"] + log)
    assert e_fwd <= 4 * e_fwd32 + FWD_REL * float(f64.abs().max()), (e_fwd, e_fwd32)
    assert e_frozen <= 2 * (4 * e_fwd32 + FWD_REL * float(f64.abs().max())), (e_frozen, e_fwd32)  # (two passes, each within it)
    assert not over, "\n".join(over)


# ------------------------------------------------------------------------------------------------
# the policy
# ------------------------------------------------------------------------------------------------
def _latent(trainable=True, **kw):
    from det_init import det_fill

    from ivln_ce_amd import latent_policy  # noqa: F401
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.registry import baseline_registry
    from ivln_ce_amd.spaces import Box, Dict, Discrete

    cfg = get_config(opts=["MODEL.policy_name", "LatentCMAPolicy", "MODEL.INSTRUCTION_ENCODER.use_pretrained_embeddings", False,
                           "MODEL.DEPTH_ENCODER.ddppo_checkpoint", "NONE", "MODEL.RGB_ENCODER.trainable", trainable]
                    + [x for k, v in kw.items() for x in (k, v)])
    space = Dict({"depth": Box(0.0, 1.0, (256, 256, 1), np.float32), "rgb": Box(0, 255, (224, 224, 3), np.uint8),
                  "instruction": Box(0, 2504, (200,), np.int64)})
    pol = baseline_registry.get_policy("LatentCMAPolicy").from_config(cfg, space, Discrete(4))
    det_fill(pol, seed=0, conv_gain=1.0)
    return pol.to(DEV).train()


def _batch(T=2, N=2, seed=3, H=64, rgb_features=False):
    """T x N rows with 64 x 64 rgb frames (the network takes any even size; the twin on the CPU stays quick) and cached
    depth features (the depth encoder is not this test's subject)"""
    from gen_latent_update_features import features

    g = torch.Generator().manual_seed(seed)
    TN = T * N
    instr = torch.zeros(N, 200)
    for n in range(N):
        L = 30 - 13 * n
        instr[n, :L] = torch.randint(2, 2504, (L,), generator=g).float()
    rgb_np, dep_np = features(7, T, N)
    obs = {"depth_features": torch.from_numpy(dep_np), "instruction": instr.repeat(T, 1)}
    if rgb_features:
        obs["rgb_features"] = torch.from_numpy(rgb_np)
    else:
        obs["rgb"] = _frames(TN, H, seed + 1)
    prev = torch.randint(0, 4, (TN, 1), generator=g)
    nd = torch.ones(T, N, dtype=torch.uint8)
    nd[0] = 0
    tgt = torch.randint(0, 4, (T, N), generator=g)
    w = torch.where(torch.rand(T, N, generator=g) < 0.5, torch.tensor(3.2), torch.tensor(1.0))
    return dict(T=T, N=N, obs=obs, prev=prev, nd=nd.view(-1, 1), tgt=tgt, w=w)


def _update(pol, c, step_grad=False, opt=None):
    from ivln_ce_amd.trainers import FlatAdam, update_agent

    opt = opt or FlatAdam(pol, lr=2.5e-4)
    dobs = {k: v.to(DEV) for k, v in c["obs"].items()}
    out = update_agent(pol, opt, dobs, c["prev"].to(DEV), c["nd"].to(DEV), c["tgt"].to(DEV), c["w"].to(DEV),
                       hidden_size=512, step_grad=step_grad)
    torch.cuda.synchronize()
    return opt, out


class _Spy:
    """train.rgb_encoder_backward with its upstream gradient and the masks of the saves it is about to release kept, the
    update's saves as backward_hip sees them, and the number of encoder passes of either kind"""

    def __init__(self, monkeypatch, pol):
        from ivln_ce_amd import train

        self.calls, self.S, self.G, self.passes = [], [], [], dict(train=0, frozen=0)
        cnn, net = pol.net.rgb_encoder.cnn, pol.net
        orig = getattr(train, "rgb_encoder_backward", None)

        def wrapper(cnn_, save, d_feats, G):
            masks, pool_idx = RT.masks_from_saves(save)
            self.calls.append(dict(masks=masks, pool_idx=pool_idx, d_feats=d_feats.detach().cpu().clone()))
            return orig(cnn_, save, d_feats, G)

        monkeypatch.setattr(train, "rgb_encoder_backward", wrapper, raising=False)
        back = net.backward_hip

        def backward_hip(S, d):
            self.S.append(dict(S))
            G = back(S, d)
            self.G.append(G)
            return G

        monkeypatch.setattr(net, "backward_hip", backward_hip)
        for kind, name in (("train", "forward_train"), ("frozen", "forward")):
            fn = getattr(cnn, name, None)
            if fn is not None:
                def counted(*a, _fn=fn, _kind=kind, **k):
                    self.passes[_kind] += 1
                    return _fn(*a, **k)

                monkeypatch.setattr(cnn, name, counted)


def test_latent_cma_update_trains_the_rgb_encoder_and_the_rollout_follows(monkeypatch):
    """update_agent of LatentCMAPolicy with RGB_ENCODER.trainable at T = 2, N = 2 on rgb frames: every `cnn` .grad equals
    what the encoder alone gives (the twin) under the upstream d(rgb) that reached rgb_encoder_backward; one Adam step moves
    all of them; the rollout after it runs on the updated weights and running statistics."""
    from ivln_ce_amd import ops

    torch.set_num_threads(min(8, torch.get_num_threads()))
    c = _batch()
    pol = _latent(True)
    cnn = pol.net.rgb_encoder.cnn
    assert cnn.trains and all(p.requires_grad for p in cnn.parameters())
    n_par = len(list(cnn.parameters()))
    N = c["N"]
    dobs = {k: v.to(DEV) for k, v in c["obs"].items()}
    step_obs = {k: v[:N] for k, v in dobs.items()}
    with torch.no_grad():  # (fills the folded cache and the packed weights with the OLD weights)
        old_feats = pol.net.rgb_encoder(step_obs).clone()
    start = {k: v.detach().clone() for k, v in cnn.state_dict().items()}
    spy = _Spy(monkeypatch, pol)
    opt, _ = _update(pol, c, step_grad=False)
    assert sum(n.startswith("net.rgb_encoder.cnn.") for n in opt.names) == n_par
    assert len(spy.calls) == 1 and spy.passes == dict(train=1, frozen=0) and spy.S[0].get("rgb_enc") is not None
    r = spy.calls[0]
    assert tuple(r["d_feats"].shape) == (c["T"] * N, 2048, 4, 4) and float(r["d_feats"].abs().max()) > 0
    x = RT.to_input(c["obs"]["rgb"])
    ref, _, _ = RT.twin_gradients(start, x, r["masks"], r["pool_idx"], r["d_feats"])
    cpu = RT.fp32_autograd_error(start, x, r["d_feats"])
    got = {k: p.grad for k, p in cnn.named_parameters()}
    assert all(v is not None for v in got.values())
    log, over = RT.compare_with_allowance(got, ref, cpu["e32"])
    _write("rgb_trainable_latent_encoder.log", log)
    assert not over, "\n".join(over)

    epoch = ops.WEIGHT_EPOCH
    opt.step()
    torch.cuda.synchronize()
    assert ops.WEIGHT_EPOCH == epoch + 1
    moved = [k for k, v in cnn.state_dict().items() if not torch.equal(v, start[k])]
    assert len(moved) == len(start), f"{len(start) - len(moved)} tensors of the encoder did not move"
    fresh = _latent(True)
    fresh.load_state_dict({k: v.detach().clone() for k, v in pol.state_dict().items()})
    with torch.no_grad():
        a, b = pol.net.rgb_encoder(step_obs).clone(), fresh.net.rgb_encoder(step_obs).clone()
    assert cnn._epoch == ops.WEIGHT_EPOCH, "the folded BatchNorms were rebuilt for this weight epoch"
    assert spy.passes["frozen"] == 1
    assert _same(a, b), "the rollout's rgb features are those of the updated weights and running statistics"
    assert not _same(a, old_feats)


def test_ablated_rgb_branch_gives_exactly_zero_encoder_gradients_and_saves_nothing(monkeypatch):
    c = _batch()
    pol = _latent(True, **{"MODEL.ablate_rgb": True})
    spy = _Spy(monkeypatch, pol)
    _update(pol, c)
    assert not spy.calls and spy.passes["train"] == 0, "the features are multiplied by 0: no saving pass, no backward"
    assert "rgb_enc" in spy.S[0] and spy.S[0]["rgb_enc"] is None
    for k, p in pol.net.rgb_encoder.cnn.named_parameters():
        assert p in spy.G[0] and float(spy.G[0][p].abs().max()) == 0.0, k
        assert p.grad is not None and float(p.grad.abs().max()) == 0.0, k


def test_cached_rgb_features_take_no_encoder_pass_and_no_encoder_gradient(monkeypatch):
    c = _batch(rgb_features=True)
    pol = _latent(True)
    spy = _Spy(monkeypatch, pol)
    _update(pol, c)
    assert not spy.calls and spy.passes == dict(train=0, frozen=0)
    assert "rgb_enc" not in spy.S[0]
    assert not any(p in spy.G[0] for p in pol.net.rgb_encoder.cnn.parameters())


def test_frozen_rgb_encoder_takes_the_folded_path_no_saves_and_no_gradients(monkeypatch):
    """trainable False (the default): the update's forward takes the `_Folded` path it always took - no per-layer saves, no
    `rgb_enc` key, no `cnn` entry in G or FlatAdam, none of the train-mode kernels launched - and two updates from the same
    state return the same losses (the forward is bit-stable; the embedding gradient's float atomics are not)."""
    from ivln_ce_amd import ops

    def never(*a, **k):
        raise AssertionError("a kernel of the trainable encoder ran for a frozen one")

    for name in ("bn_apply", "bn_bwd", "adaptive_avgpool2d_bwd"):
        monkeypatch.setattr(ops, name, never, raising=False)
    c = _batch()
    outs = []
    for _ in range(2):
        pol = _latent(False)
        cnn = pol.net.rgb_encoder.cnn
        assert not any(p.requires_grad for p in cnn.parameters())
        spy = _Spy(monkeypatch, pol)
        opt, out = _update(pol, c)
        assert not any(n.startswith("net.rgb_encoder.cnn.") for n in opt.names)
        assert all(p.grad is None for p in cnn.parameters())
        assert not spy.calls and spy.passes == dict(train=0, frozen=1)
        assert "rgb_enc" not in spy.S[0] and not any(p in spy.G[0] for p in cnn.parameters())
        names = {p: k for k, p in pol.named_parameters()}
        outs.append((out, spy.S[0]["rgb"].clone(), spy.S[0]["feats"].clone(), {names[p]: g.clone() for p, g in spy.G[0].items()}))
    assert outs[0][0] == outs[1][0] and _same(outs[0][1], outs[1][1]) and _same(outs[0][2], outs[1][2])
    # the head's gradients, bit for bit (all but the instruction embedding's, the one sum with float atomics)
    assert sorted(outs[0][3]) == sorted(outs[1][3]) and len(outs[0][3]) >= 30
    differ = [k for k, g in outs[0][3].items() if "embedding_layer" not in k and not _same(g, outs[1][3][k])]
    assert not differ, differ
