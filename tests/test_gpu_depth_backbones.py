"""GPU: the depth encoder on the DD-PPO backbones beyond ResNet-50 (MODEL.DEPTH_ENCODER.backbone: resneXt50, se_resnet50,
se_resneXt50, se_resneXt101) - conv + GroupNorm pairs with the grouped 3x3 conv and the SE tail of csrc/group_conv.hip -
against the float64 restatement of tests/depth_backbones_ref.py, under the bar tests/test_gpu_depth_net.py applies to
ResNet-50 (max abs error of the (B, 128, 4, 4) features below 1e-4); the default backbone against features recorded on the
commit before these backbones existed; and one MapCMAPolicy step on se_resneXt50, eager and replayed."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import depth_backbones_ref as DR  # noqa: E402
from kernel_bar import _log  # noqa: E402

DEV = torch.device("cuda:0")
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _encoder(name, seed=5):
    """As tests/test_gpu_depth_net.py builds its encoder: seeded init, GroupNorm affine parameters randomised, frozen."""
    from ivln_ce_amd.encoders import ResNetEncoder

    torch.manual_seed(seed)
    enc = ResNetEncoder((256, 256, 1), backbone=name).eval() if name != "resnet50" else ResNetEncoder((256, 256, 1)).eval()
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.normal_(1.0, 0.2)
                m.bias.normal_(0.0, 0.2)
    for p in enc.parameters():
        p.requires_grad_(False)
    return enc.to(DEV)


def _restated(name, enc, depth):
    """-> (float64 features, fp32-CPU features) of the restatement with `enc`'s weights"""
    ref = DR.encoder(name)
    ref.load_state_dict({k: v.cpu() for k, v in enc.state_dict().items()}, strict=True)
    with torch.no_grad():
        r32 = ref({"depth": depth})
        r64 = ref.double()({"depth": depth.double()}).float()
    return r64, r32


def _pairs(enc, depth):
    """The encoder's conv + GroupNorm pair form: persistent launch and chain off."""
    from ivln_ce_amd import ops

    old = ops.DEPTH_NET, ops.CHAIN_GN_CONV
    try:
        ops.DEPTH_NET, ops.CHAIN_GN_CONV = 0, False
        with torch.no_grad():
            return enc({"depth": depth.to(DEV)}).cpu()
    finally:
        ops.DEPTH_NET, ops.CHAIN_GN_CONV = old


@functools.lru_cache(maxsize=None)
def _resnet50_pair_error():
    """The yardstick: the default backbone's pair-path error against ITS float64 restatement, same inputs (computed once)."""
    enc = _encoder("resnet50")
    depth = torch.rand(2, 256, 256, 1, generator=torch.Generator().manual_seed(2))
    r64, _ = _restated("resnet50", enc, depth)
    return float((_pairs(enc, depth) - r64).abs().max())


@pytest.mark.parametrize("name,B", [("resneXt50", 2), ("se_resnet50", 2), ("se_resneXt50", 2), ("se_resneXt101", 1)])
def test_backbone_matches_the_float64_restatement(name, B):
    from ivln_ce_amd import depth_net

    enc = _encoder(name)
    assert not depth_net.supported(enc) and depth_net.plan_for(enc, DEV) is None
    depth = torch.rand(B, 256, 256, 1, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():  # (default switches: the persistent launch and the chain decline, the pairs run)
        a = enc({"depth": depth.to(DEV)}).cpu()
        a2 = enc({"depth": depth.to(DEV)}).cpu()
    r64, r32 = _restated(name, enc, depth)
    err, e32 = float((a - r64).abs().max()), float((r32 - r64).abs().max())
    line = (f"{name} B={B}: HIP vs float64 restatement {err:.2e}  (fp32-CPU restatement's own error {e32:.2e}; resnet50 "
            f"pair path vs its restatement {_resnet50_pair_error():.2e}; max|ref| {float(r64.abs().max()):.2e})")
    print(line)
    _log(line, "depth_backbones_parity.log")  # (the suite's log directory, tests/kernel_bar.py)
    assert a.shape == (B, 128, 4, 4) and np.isfinite(a.numpy()).all()
    assert torch.equal(a, a2), "two runs give the same bytes"
    assert torch.equal(a, _pairs(enc, depth)), "only the pair form exists for this backbone, whatever the switches say"
    assert err < 1e-4, line  # tests/test_gpu_depth_net.py:67 - the bar ResNet-50 is held to


def test_default_backbone_is_bit_identical_to_the_commit_before():
    """tests/golden/depth_resnet50_paths.npz: the default encoder's features (seed 5, randomised GroupNorm affine, depth
    seed 2, batch 2) on the persistent launch, the gn_conv chain and the conv + GroupNorm pairs, recorded on an MI355X from
    the parent of the commit that added csrc/group_conv.hip.  The same bytes now: the new file, the generalised
    bottleneck class and the new ops changed nothing the default backbone computes.  (A later change that legitimately
    moves ResNet-50's bits re-records the file with the same recipe.)"""
    from ivln_ce_amd import ops

    want = np.load(os.path.join(G, "depth_resnet50_paths.npz"))
    enc = _encoder("resnet50")
    depth = torch.rand(2, 256, 256, 1, generator=torch.Generator().manual_seed(2)).to(DEV)
    old = ops.DEPTH_NET, ops.CHAIN_GN_CONV
    got = {}
    try:
        with torch.no_grad():
            ops.DEPTH_NET = 2
            got["persistent"] = enc({"depth": depth}).cpu().numpy()
            ops.DEPTH_NET, ops.CHAIN_GN_CONV = 0, True
            got["chain"] = enc({"depth": depth}).cpu().numpy()
            ops.CHAIN_GN_CONV = False
            got["pair"] = enc({"depth": depth}).cpu().numpy()
    finally:
        ops.DEPTH_NET, ops.CHAIN_GN_CONV = old
    for k in ("persistent", "chain", "pair"):
        assert got[k].tobytes() == want[k].tobytes(), f"{k}: max |diff| {np.abs(got[k] - want[k]).max():.3e}"


def _policy(backbone):
    from det_init import det_fill

    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.policy import MapCMAPolicy
    from ivln_ce_amd.spaces import Box, Dict, Discrete

    cfg = get_config(opts=["MODEL.policy_name", "MapCMAPolicy", "MODEL.INSTRUCTION_ENCODER.use_pretrained_embeddings", False,
                           "MODEL.DEPTH_ENCODER.ddppo_checkpoint", "NONE", "MODEL.DEPTH_ENCODER.backbone", backbone])
    space = Dict({"depth": Box(0.0, 1.0, (256, 256, 1), np.float32), "occupancy_map": Box(0, 255, (64, 64), np.uint8),
                  "semantic_map": Box(0, 255, (64, 64), np.uint8), "instruction": Box(0, 2504, (200,), np.int64)})
    pol = MapCMAPolicy.from_config(cfg, space, Discrete(4))
    det_fill(pol, seed=0)
    return pol.to(DEV).eval()


def test_policy_step_on_se_resnext50_replays_bit_identically_and_its_gates_are_live():
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.graphed import GraphedRollout
    from ivln_ce_amd.obs_transforms import GTSemanticsIterativeMapper
    from ivln_ce_amd.synthetic import SyntheticRollout

    pol = _policy("se_resneXt50")
    bb = pol.net.depth_encoder.visual_encoder.backbone
    assert not bb.plain and bb.layer1[0].convs[3].groups == 16 and bb.layer4[2].se is not None
    cfg = get_config()
    B = 2
    roll = SyntheticRollout(B=B, seed=31)
    obs = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in roll.step().items()}

    def eager():
        tr = GTSemanticsIterativeMapper.from_config(cfg)
        b = tr(dict(obs))
        rnn = torch.zeros(B, 2, 512, device=DEV)
        prev = torch.zeros(B, 1, dtype=torch.long, device=DEV)
        with torch.no_grad():
            a, rnn = pol.act(b, rnn, prev, b["not_done_masks"], deterministic=True)
        torch.cuda.synchronize()
        return a.clone(), rnn.clone()

    a_e, rnn_e = eager()
    tr_g = GTSemanticsIterativeMapper.from_config(cfg)
    runner = GraphedRollout(pol, [tr_g], obs, deterministic=True)
    tr_g.mapping_module.reset()
    runner.reset_state()
    a_g = runner.step(obs)
    torch.cuda.synchronize()
    assert torch.equal(a_g, a_e), "actions: replayed vs eager"
    assert torch.equal(runner.rnn_states, rnn_e), "recurrent state: replayed vs eager"
    tr_g.mapping_module.check_status()
    del runner
    # gates forced open (final excite bias + 40 -> sigmoid = 1): another network, so other features and another state
    with torch.no_grad():
        for layer in (bb.layer1, bb.layer2, bb.layer3, bb.layer4):
            for blk in layer:
                blk.se.excite[2].bias.fill_(40.0)
    _, rnn_open = eager()
    assert not torch.equal(rnn_open, rnn_e) and float((rnn_open - rnn_e).abs().max()) > 1e-4, "the SE branch is not live"
