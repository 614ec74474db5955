"""GPU: egocentric maps other than 64 x 64 cells (EGOCENTRIC_MAPPER.height_meters / width_meters / resolution_meters) from
the mapper to the action head, against what the reference's own code gave at those sizes (tests/golden/
gen_map_sizes_golden.py): the HIP mapper bit for bit, the policy's act steps and one update within the bars the 64 x 64 tests
use (tests/test_gpu_policy.py, tests/test_gpu_train.py), the head's two attention forms against each other, a 64 x 64
policy beside a 32 x 48 one, and the config surface end to end.  Every figure goes to map_sizes_parity.log in the suite's
log directory before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
sys.path.insert(0, os.path.dirname(__file__))
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = torch.device("cuda:0")
ATOL = 2e-4  # features and states (tests/test_gpu_policy.py); log-probabilities 1e-4
LOG = "map_sizes_parity.log"
SIZES = {"32x48": (32, 48), "96x112": (96, 112)}


def _log(line):
    from kernel_bar import _log as log

    log(line, LOG)


def _policy(rows, cols, rnn_type="GRU", use_pm=False, train=False):
    from det_init import det_fill

    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.policy import MapCMAPolicy
    from ivln_ce_amd.spaces import Box, Dict, Discrete

    cfg = get_config(opts=[
        "MODEL.policy_name", "MapCMAPolicy", "MODEL.INSTRUCTION_ENCODER.use_pretrained_embeddings", False,
        "MODEL.DEPTH_ENCODER.ddppo_checkpoint", "NONE", "MODEL.PROGRESS_MONITOR.use", use_pm,
        "MODEL.STATE_ENCODER.rnn_type", rnn_type,
    ])
    space = Dict({
        "depth": Box(0.0, 1.0, (256, 256, 1), np.float32), "occupancy_map": Box(0, 255, (rows, cols), np.uint8),
        "semantic_map": Box(0, 255, (rows, cols), np.uint8), "instruction": Box(0, 2504, (200,), np.int64),
    })
    pol = det_fill(MapCMAPolicy.from_config(cfg, space, Discrete(4)), seed=0).to(DEV)
    pol.train() if train else pol.eval()
    return pol


# ------------------------------------------------------------------------------------------------------------------
# mapper
# ------------------------------------------------------------------------------------------------------------------
def _mapper_obs(g, t):
    return {
        "depth": torch.from_numpy(g[f"depth_{t}"]).to(DEV), "semantic12": torch.from_numpy(g[f"semantic12_{t}"]).to(DEV),
        "world_robot_pose": torch.from_numpy(g[f"pose_{t}"]).to(DEV),
        "world_robot_orientation": torch.from_numpy(g[f"orientation_{t}"]).to(DEV),
        "not_done_masks": torch.from_numpy(g[f"not_done_{t}"]).to(DEV), "env_name": ["s"] * int(g["B"]),
    }


@pytest.mark.parametrize("entry", ["posed", "halves", "frames"])
@pytest.mark.parametrize("case", ["32x48", "96x112", "res02"])
def test_hip_mapper_matches_the_reference_at_other_map_sizes(case, entry):
    """The iterative gt-semantics mapper at 3.2 m x 4.8 m, 9.6 m x 11.2 m and 6.4 m x 6.4 m at 0.2 m: maps, world-cloud size
    and (last step) the world cloud itself, bit for bit, through the posed step, its begin / finish halves and the entry that
    takes the reference's transforms."""
    from ivln_ce_amd.mapping import CameraParameters, MapDimensions, create_gt_semantics_iterative_mapper

    g = np.load(os.path.join(G, f"map_sizes_mapper_{case}.npz"))
    H, W, steps = int(g["H"]), int(g["W"]), int(g["steps"])
    dims = MapDimensions(float(g["height_meters"]), float(g["width_meters"]), float(g["resolution_meters"]))
    assert (dims.num_rows, dims.num_cols) == (int(g["num_rows"]), int(g["num_cols"]))
    m = create_gt_semantics_iterative_mapper(DEV, CameraParameters(float(np.deg2rad(90.0 * H / W)), (H, W), 0.1), dims, b_max=2)
    for t in range(steps):
        obs = _mapper_obs(g, t)
        if entry == "posed":
            mem = m(obs)
        elif entry == "halves":
            m.begin(obs)
            mem = m.finish(obs)
        else:
            mem = m(obs, T=torch.from_numpy(g[f"T_{t}"]).to(DEV), rot=torch.from_numpy(g[f"rot_{t}"]).to(DEV))
        n = m.check_status()
        assert mem.occupancy.shape == (2, dims.num_rows, dims.num_cols)
        assert n == int(g[f"world_n_{t}"]), f"world size step {t}"
        assert np.array_equal(mem.occupancy.cpu().numpy(), g[f"occ_{t}"]), f"occupancy step {t}"
        assert np.array_equal(mem.semantic.cpu().numpy(), g[f"sem_{t}"]), f"semantic step {t}"
        if f"world_xyz_{t}" in g:
            xyz, b, s = m.world_cloud()
            assert np.array_equal(xyz.view(np.uint32), g[f"world_xyz_{t}"].view(np.uint32))
            assert np.array_equal(b, g[f"world_b_{t}"]) and np.array_equal(s, g[f"world_sem_{t}"])


@pytest.mark.parametrize("library", [True, False], ids=["library", "copy"])
def test_known_mapper_matches_the_reference_at_a_non_square_map(library, tmp_path):
    """create_known_mapper at 3.2 m x 4.8 m: the library step (ivln_mapper_known_step) and the copy path, bit for bit"""
    from ivln_ce_amd.mapping import MapDimensions, MappingModule

    g = np.load(os.path.join(G, "known_map_sizes.npz"))
    names = [str(x) for x in g["env_names"]]
    for n in set(names):
        np.savez(tmp_path / f"{n}.npz", xyz=g[f"scene_{n}_xyz"], semantics=g[f"scene_{n}_semantics"])
    dims = MapDimensions(float(g["height_meters"]), float(g["width_meters"]), float(g["resolution_meters"]))
    B = int(g["B"])
    m = MappingModule(DEV, None, dims, mode="known", maps_location=str(tmp_path), b_max=B, known_library=library)
    for t in range(int(g["steps"])):
        obs = {"depth": torch.zeros(B, 16, 16, 1, device=DEV), "world_robot_pose": torch.from_numpy(g[f"pose_{t}"]).to(DEV),
               "world_robot_orientation": torch.from_numpy(g[f"orientation_{t}"]).to(DEV),
               "not_done_masks": torch.from_numpy(g[f"not_done_{t}"]).to(DEV), "env_name": list(names)}
        mem = m(obs)
        m.check_status()
        assert np.array_equal(mem.occupancy.cpu().numpy(), g[f"occ_{t}"]), f"occupancy step {t}"
        assert np.array_equal(mem.semantic.cpu().numpy(), g[f"sem_{t}"]), f"semantic step {t}"


def test_known_library_step_at_another_resolution_matches_the_oracle(tmp_path):
    """the library step at 6.4 m x 4.8 m, 0.2 m cells (32 x 24) against the C oracle's known step: bit for bit"""
    from ivln_ce_amd.mapping import MapDimensions, MappingModule
    from oracle.mapper_ref import MapperRef

    g = np.load(os.path.join(G, "known_map_sizes.npz"))
    names = [str(x) for x in g["env_names"]]
    clouds = {}
    for n in set(names):
        np.savez(tmp_path / f"{n}.npz", xyz=g[f"scene_{n}_xyz"], semantics=g[f"scene_{n}_semantics"])
        clouds[n] = (np.ascontiguousarray(g[f"scene_{n}_xyz"]), g[f"scene_{n}_semantics"].astype(np.uint8))
    B = int(g["B"])
    m = MappingModule(DEV, None, MapDimensions(6.4, 4.8, 0.2), mode="known", maps_location=str(tmp_path), b_max=B,
                      known_library=True)
    ref = MapperRef(16, 16, height_m=6.4, width_m=4.8, res_m=0.2)
    for t in range(int(g["steps"])):
        pose, orient, nd = g[f"pose_{t}"], g[f"orientation_{t}"], g[f"not_done_{t}"]
        occ_r, sem_r = ref.known_step(clouds, names, pose, orient, nd)
        obs = {"depth": torch.zeros(B, 16, 16, 1, device=DEV), "world_robot_pose": torch.from_numpy(pose).to(DEV),
               "world_robot_orientation": torch.from_numpy(orient).to(DEV), "not_done_masks": torch.from_numpy(nd).to(DEV),
               "env_name": list(names)}
        mem = m(obs)
        m.check_status()
        assert occ_r.shape == (B, 32, 24) and int(occ_r.sum()) > 100
        assert np.array_equal(mem.occupancy.cpu().numpy(), occ_r), f"occupancy step {t}"
        assert np.array_equal(mem.semantic.cpu().numpy(), sem_r), f"semantic step {t}"


# ------------------------------------------------------------------------------------------------------------------
# policy: act
# ------------------------------------------------------------------------------------------------------------------
_GOLD = {}


def _gold():
    if "g" not in _GOLD:
        _GOLD["g"] = np.load(os.path.join(G, "policy_map_sizes.npz"))
    return _GOLD["g"]


def _act_obs(g, tag, t, dev=DEV):
    p = f"{tag}/act/"
    return {"depth_features": torch.from_numpy(g[p + f"depth_features_{t}"]).to(dev),
            "occupancy_map": torch.from_numpy(g[p + f"occ_{t}"]).to(dev), "semantic_map": torch.from_numpy(g[p + f"sem_{t}"]).to(dev),
            "instruction": torch.from_numpy(g[p + "instruction"]).to(dev)}


def _err(name, got, ref, log):
    e = float(np.abs(np.asarray(got) - np.asarray(ref)).max())
    log.append(f"{name}: max|err|={e:.3e} (ref max {float(np.abs(ref).max()):.3e})")
    _log(log[-1])
    return e


@pytest.mark.parametrize("tag", list(SIZES))
def test_act_matches_the_reference_at_other_map_sizes(tag):
    """Two act steps (a mask reset on the second) of the GRU policy from the reference's own run at 6 and at 42 map positions:
    map features, features, states within 2e-4, log-probabilities within 1e-4, the same arg-max - the bars of
    tests/test_gpu_policy.py::test_act_matches_reference_golden, none widened."""
    g, (rows, cols) = _gold(), SIZES[tag]
    pol = _policy(rows, cols)
    assert pol.net.map_linear[1].in_features == 128 * (rows // 16) * (cols // 16)
    p, log, worst = f"{tag}/act/", [], 0.0
    for t in range(2):
        obs = _act_obs(g, tag, t)
        with torch.no_grad():
            mp = pol.net.map_encoder(obs)
            f, rnn = pol.net(obs, torch.from_numpy(g[p + f"rnn_in_{t}"]).to(DEV), torch.from_numpy(g[p + f"prev_{t}"]).to(DEV),
                             torch.from_numpy(g[p + f"masks_{t}"]).to(DEV))
            logits = pol.action_distribution.raw_logits(f)
            act = pol._act(f, True)
        worst = max(worst, _err(f"{tag} map_feat_{t}", mp.cpu().numpy(), g[p + f"map_feat_{t}"], log))
        worst = max(worst, _err(f"{tag} features_{t}", f.cpu().numpy(), g[p + f"features_{t}"], log))
        worst = max(worst, _err(f"{tag} rnn_out_{t}", rnn.cpu().numpy(), g[p + f"rnn_out_{t}"], log))
        e = _err(f"{tag} logprobs_{t}", torch.log_softmax(logits, -1).cpu().numpy(), g[p + f"logits_{t}"], log)
        assert np.array_equal(act.cpu().numpy()[:, 0], g[p + f"logits_{t}"].argmax(-1)), "\n".join(log)
        assert e < 1e-4, "\n".join(log)
    assert worst < ATOL, "\n".join(log)


@pytest.mark.parametrize("tag", list(SIZES))
def test_lstm_act_matches_the_float64_oracle_at_other_map_sizes(tag):
    """STATE_ENCODER.rnn_type LSTM on the same inputs against the float64 torch oracle of tests/lstm_state_ref.py built for
    that map (it shares nothing with the GRU path): features and the four state slots within 2e-4, logits within 1e-4."""
    from lstm_state_ref import MapCMAPolicyLSTMRef

    torch.set_num_threads(8)
    g, (rows, cols) = _gold(), SIZES[tag]
    pol = _policy(rows, cols, rnn_type="LSTM")
    ref = MapCMAPolicyLSTMRef(map_hw=(rows, cols)).eval()
    ref.load_state_dict({k: v.cpu() for k, v in pol.state_dict().items()})
    ref = ref.double()
    p, log = f"{tag}/act/", []
    rnn_d = torch.zeros(2, 4, 512, device=DEV)
    rnn_r = torch.zeros(2, 4, 512, dtype=torch.float64)
    for t in range(2):
        obs = _act_obs(g, tag, t)
        prev, masks = torch.from_numpy(g[p + f"prev_{t}"]), torch.from_numpy(g[p + f"masks_{t}"])
        with torch.no_grad():
            f, rnn_d = pol.net(obs, rnn_d, prev.to(DEV), masks.to(DEV))
            lg = pol.action_distribution.raw_logits(f)
            cpu = {k: (v.cpu().double() if v.dtype.is_floating_point else v.cpu()) for k, v in obs.items()}
            keep = torch.get_default_dtype()
            torch.set_default_dtype(torch.float64)  # (the oracle's map features follow the default dtype)
            try:
                lr, rnn_r, fr = ref.logits(cpu, rnn_r, prev, masks.double())
            finally:
                torch.set_default_dtype(keep)
        e_f = _err(f"{tag} lstm features_{t}", f.cpu().double().numpy(), fr.numpy(), log)
        e_s = _err(f"{tag} lstm states_{t}", rnn_d.cpu().double().numpy(), rnn_r.numpy(), log)
        e_l = _err(f"{tag} lstm logits_{t}", lg.cpu().double().numpy(), lr.numpy(), log)
        assert e_f < ATOL and e_s < ATOL and e_l < 1e-4, "\n".join(log)


# ------------------------------------------------------------------------------------------------------------------
# policy: update
# ------------------------------------------------------------------------------------------------------------------
class _Sub:
    """the keys of one case's update in the fixture, under the names tests/test_gpu_train.py's helpers read"""

    def __init__(self, g, prefix):
        self.g, self.prefix = g, prefix
        self.files = [k[len(prefix):] for k in g.files if k.startswith(prefix)]

    def __getitem__(self, k):
        return self.g[self.prefix + k]


@pytest.mark.parametrize("tag", list(SIZES))
def test_update_matches_the_reference_at_other_map_sizes(tag):
    """The reference's own _update_agent body (torch loss + loss.backward()) on the HIP policy, T = 3, N = 2, progress monitor,
    train mode, against the reference's run: logits 1e-5, losses 2e-5, gradients by test_gpu_train._check_grads' rule (every
    gradient norm 5e-4 relative; the stored gradients rtol 1e-3 + atol 2e-6 - the two large ones on the rows the fixture
    keeps), BatchNorm buffers after the update."""
    from test_gpu_train import _batch, _check_grads

    from ivln_ce_amd.aux_losses import AuxLosses

    (rows, cols) = SIZES[tag]
    g = _Sub(_gold(), f"{tag}/update/")
    pol = _policy(rows, cols, use_pm=True, train=True)
    obs, prev, nd, tgt, w = _batch(g)
    T, N = tgt.shape
    AuxLosses.activate()
    AuxLosses.clear()
    try:
        dist, _ = pol.build_distribution(obs, torch.zeros(N, 2, 512, device=DEV), prev, nd)
        logits = dist.logits.view(T, N, -1)
        ce = F.cross_entropy(logits.permute(0, 2, 1), tgt, reduction="none")
        action_loss = ((w * ce).sum(0) / w.sum(0)).mean()
        aux = AuxLosses.reduce((w > 0).view(-1))
        loss = action_loss + aux
        loss.backward()
    finally:
        AuxLosses.deactivate()
    log = [f"{tag} loss {float(loss):.7f} ref {float(g['loss']):.7f}; action {float(action_loss):.7f} ref "
           f"{float(g['action_loss']):.7f}; aux {float(aux):.7f} ref {float(g['aux_loss']):.7f}",
           f"{tag} logits max|err| {float(np.abs(logits.detach().cpu().numpy() - g['logits']).max()):.3e}"]
    bad = _check_grads(pol, g, log)
    params = dict(pol.named_parameters())
    for k in g.files:
        if k.startswith("gradrows"):
            step, name = int(k.split("/")[0][8:]), k.split("/", 1)[1]
            got = params[name].grad.cpu().numpy()[::step]
            log.append(f"{name}[::{step}]: max|err|={np.abs(got - g[k]).max():.3e} (ref max {np.abs(g[k]).max():.3e})")
            if not np.allclose(got, g[k], atol=2e-6, rtol=1e-3):
                bad.append(k + f" maxerr={np.abs(got - g[k]).max():.3e}")
    for line in log:
        _log(line)
    assert np.allclose(logits.detach().cpu().numpy(), g["logits"], atol=1e-5), log[1]
    assert abs(float(loss) - float(g["loss"])) < 2e-5 and abs(float(action_loss) - float(g["action_loss"])) < 2e-5, log[0]
    assert abs(float(aux) - float(g["aux_loss"])) < 2e-5, log[0]
    assert not bad, "\n".join(bad + log)
    sd = pol.state_dict()
    for k in g.files:
        if k.startswith("post/"):
            assert np.allclose(sd[k[5:]].cpu().numpy(), g[k], atol=1e-6, rtol=1e-5), k


# ------------------------------------------------------------------------------------------------------------------
# head paths
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(SIZES))
def test_head_with_the_pair_kernel_against_the_generic_attentions(tag, monkeypatch):
    """ops.attn_pair (one launch) against the head forced onto two ops.attn launches: both within the reference bar of each
    other, and each form really ran"""
    from ivln_ce_amd import ops

    g, (rows, cols) = _gold(), SIZES[tag]
    pol = _policy(rows, cols)
    p = f"{tag}/act/"
    calls = {"pair": 0, "attn": 0}
    real_pair, real_attn = ops.attn_pair, ops.attn
    monkeypatch.setattr(ops, "attn_pair", lambda *a, **k: (calls.__setitem__("pair", calls["pair"] + 1), real_pair(*a, **k))[1])
    monkeypatch.setattr(ops, "attn", lambda *a, **k: (calls.__setitem__("attn", calls["attn"] + 1), real_attn(*a, **k))[1])
    out = {}
    for use in (True, False):
        monkeypatch.setattr(ops, "ATTN_PAIR", use)
        calls.update(pair=0, attn=0)
        with torch.no_grad():
            f, rnn = pol.net(_act_obs(g, tag, 1), torch.from_numpy(g[p + "rnn_in_1"]).to(DEV), torch.from_numpy(g[p + "prev_1"]).to(DEV),
                             torch.from_numpy(g[p + "masks_1"]).to(DEV))
        out[use] = (f.cpu().numpy(), rnn.cpu().numpy())
        assert (calls["pair"], calls["attn"]) == ((1, 1) if use else (0, 3)), calls  # (ops.attn: the text attention, + 2)
    log = []
    assert _err(f"{tag} pair vs generic features", out[True][0], out[False][0], log) < ATOL
    assert _err(f"{tag} pair vs generic states", out[True][1], out[False][1], log) < ATOL
    assert _err(f"{tag} generic features vs reference", out[False][0], g[p + "features_1"], log) < ATOL


def test_a_64x64_policy_keeps_the_fused_head_beside_a_32x48_one(monkeypatch):
    """One process, two policies: the 64 x 64 one takes ivln_cma_step_fwd before and after the 32 x 48 one exists and has
    run, and gives the same bytes; the 32 x 48 one never takes it."""
    from ivln_ce_amd import ops

    fused = []
    real = ops.cma_step
    monkeypatch.setattr(ops, "cma_step", lambda d: (fused.append(int(d.P)), real(d))[1])
    gen = torch.Generator().manual_seed(64)
    B = 2
    instr = torch.zeros(B, 200, dtype=torch.long)
    instr[:, :60] = torch.randint(2, 2504, (B, 60), generator=gen)

    def inputs(rows, cols):
        occ = (torch.rand(B, rows, cols, generator=gen) < 0.3).to(torch.uint8)
        return ({"depth_features": torch.randn(B, 128, 4, 4, generator=gen).to(DEV), "occupancy_map": occ.to(DEV),
                 "semantic_map": (torch.randint(0, 13, (B, rows, cols), generator=gen) * occ).to(torch.uint8).to(DEV),
                 "instruction": instr.to(DEV)},
                (0.1 * torch.randn(B, 2, 512, generator=gen)).to(DEV), torch.randint(0, 4, (B, 1), generator=gen).to(DEV),
                torch.ones(B, 1, dtype=torch.uint8, device=DEV))

    def step(pol, args):
        with torch.no_grad():
            f, r = pol.net(*args)
        torch.cuda.synchronize()
        return f.clone(), r.clone()

    pol64, in64 = _policy(64, 64), inputs(64, 64)
    before = step(pol64, in64)
    assert fused == [16]
    pol48, in48 = _policy(32, 48), inputs(32, 48)
    f48, _ = step(pol48, in48)
    assert fused == [16] and bool(torch.isfinite(f48).all())
    after = step(pol64, in64)
    assert fused == [16, 16]
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])


# ------------------------------------------------------------------------------------------------------------------
# end to end through the config surface
# ------------------------------------------------------------------------------------------------------------------
def test_config_to_graphed_rollout_and_update_at_32x48(same_depth_path):
    """EGOCENTRIC_MAPPER.height_meters 3.2 / width_meters 4.8 -> Mapper.from_config -> (32, 48) boxes -> MapCMAPolicy.from_config
    -> 6 replayed steps of 2 synthetic envs with 256 x 256 depth, bit-identical to the eager loop (actions, states, maps), as
    the 64 x 64 tests assert it; then one trainers.update_agent step that moves the map encoder's parameters."""
    same_depth_path(0)
    from det_init import det_fill

    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.graphed import GraphedRollout
    from ivln_ce_amd.obs_transforms import GTSemanticsIterativeMapper
    from ivln_ce_amd.policy import MapCMAPolicy
    from ivln_ce_amd.spaces import Box, Dict, Discrete
    from ivln_ce_amd.synthetic import SyntheticRollout
    from ivln_ce_amd.trainers import FlatAdam, update_agent

    cfg = get_config(opts=[
        "MODEL.policy_name", "MapCMAPolicy", "MODEL.INSTRUCTION_ENCODER.use_pretrained_embeddings", False,
        "MODEL.DEPTH_ENCODER.ddppo_checkpoint", "NONE",
        "RL.POLICY.OBS_TRANSFORMS.EGOCENTRIC_MAPPER.height_meters", 3.2,
        "RL.POLICY.OBS_TRANSFORMS.EGOCENTRIC_MAPPER.width_meters", 4.8,
    ])
    space = Dict({"depth": Box(0.0, 1.0, (256, 256, 1), np.float32), "instruction": Box(0, 2504, (200,), np.int64),
                  "semantic12": Box(0, 255, (256, 256, 1), np.uint8)})
    space = GTSemanticsIterativeMapper.from_config(cfg).transform_observation_space(space)
    assert space.spaces["occupancy_map"].shape == (32, 48) and space.spaces["semantic_map"].shape == (32, 48)
    assert "semantic12" not in space.spaces
    pol = det_fill(MapCMAPolicy.from_config(cfg, space, Discrete(4)), seed=0).to(DEV).eval()
    B, steps = 2, 6
    roll = SyntheticRollout(B=B, seed=48)
    obs = [{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in roll.step().items()} for _ in range(steps)]
    obs[3]["not_done_masks"][1] = 0
    tr_e = GTSemanticsIterativeMapper.from_config(cfg)
    rnn = torch.zeros(B, 2, 512, device=DEV)
    prev = torch.zeros(B, 1, dtype=torch.long, device=DEV)
    eager, batches = [], []
    for o in obs:
        b = tr_e(dict(o))
        with torch.no_grad():
            a, rnn = pol.act(b, rnn, prev, b["not_done_masks"], deterministic=True)
        prev = a
        assert b["occupancy_map"].shape == (B, 32, 48)
        eager.append((a.clone(), rnn.clone(), b["occupancy_map"].clone(), b["semantic_map"].clone()))
        batches.append({k: b[k].clone() for k in ("depth", "occupancy_map", "semantic_map", "instruction")})
    assert int(eager[-1][2].sum()) > 0, "the synthetic walls leave the 3.2 m map empty"
    tr_g = GTSemanticsIterativeMapper.from_config(cfg)
    runner = GraphedRollout(pol, [tr_g], obs[0], deterministic=True, streams="split")
    tr_g.mapping_module.reset()
    runner.reset_state()
    for t, o in enumerate(obs):
        a = runner.step(o)
        torch.cuda.synchronize()
        mem = tr_g.mapping_module.map_memory
        assert torch.equal(a, eager[t][0]), f"actions step {t}"
        assert torch.equal(runner.rnn_states, eager[t][1]), f"rnn step {t}"
        assert torch.equal(mem.occupancy, eager[t][2]) and torch.equal(mem.semantic, eager[t][3]), f"maps step {t}"
    tr_g.mapping_module.check_status()
    del runner

    # one update on the rollout's own batches (T = 6, N = 2)
    pol.train()
    T = steps
    batch = {k: torch.stack([b[k] for b in batches]).flatten(0, 1) for k in batches[0]}
    batch["instruction"] = batch["instruction"].float()
    batch["occupancy_map"], batch["semantic_map"] = batch["occupancy_map"].float(), batch["semantic_map"].float()
    gen = torch.Generator().manual_seed(7)
    prev_a = torch.randint(0, 4, (T * B, 1), generator=gen).to(DEV)
    nd = torch.ones(T, B, dtype=torch.uint8)
    nd[0] = 0
    tgt = torch.randint(0, 4, (T, B), generator=gen).to(DEV)
    w = torch.ones(T, B, device=DEV)
    enc = {k: v.detach().clone() for k, v in pol.net.map_encoder.named_parameters()}
    loss, action_loss, aux = update_agent(pol, FlatAdam(pol, lr=2.5e-4), batch, prev_a, nd.view(-1, 1).to(DEV), tgt, w, hidden_size=512)
    assert np.isfinite(loss) and np.isfinite(action_loss)
    moved = [k for k, v in pol.net.map_encoder.named_parameters() if float((v.detach() - enc[k]).abs().max()) > 0]
    # (conv biases in front of a train-mode BatchNorm have an exactly zero gradient: Adam leaves them where they are)
    assert len(moved) >= len(enc) - 4, sorted(set(enc) - set(moved))
