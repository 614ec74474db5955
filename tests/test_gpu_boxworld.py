"""GPU: the box-world renderer (csrc/boxworld.hip) against `boxworld.render_reference` bit for bit, the renderer and the HIP
mapper together against the C oracle and against the scene's geometry, and the evaluation / DAgger loops on
ENV_BACKEND "boxworld"."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

HFOV = math.pi / 2
DEV = torch.device("cuda:0")


def _cfg(*opts):
    from ivln_ce_amd.config import get_config

    return get_config(opts=list(opts) or None)


@pytest.fixture(scope="module")
def scenes():
    """Scenes of 0, 1 and 32 boxes (table entries 0, 1, 2)."""
    from ivln_ce_amd import boxworld as bw

    room = [-3.0, 0.0, -4.0, 3.5, 2.5, 2.0]
    full = bw.make_scene(5, _cfg("BOXWORLD.NUM_BOXES", 32))
    assert len(full.boxes) == 32
    return [bw.Scene(room, np.zeros((0, 6)), []), bw.Scene(room, [[-0.5, 0.0, -2.0, 0.75, 1.5, -1.5]], [7]), full]


POSES = np.array([[2.0, 1.25, 3.0], [0.0, 1.25, 0.0], [-1.0, 1.0, 0.5]], np.float32)
HEADINGS = [0.0, math.radians(15.0), 2.2173]  # 0, a turn of the agent's, and no multiple of 15 degrees
INDEX = [2, 0, 2]


def _renderer(scenes, depth_hw, rgb_hw, b_max=3):
    from ivln_ce_amd.boxworld import BoxWorldRenderer

    r = BoxWorldRenderer(DEV, b_max, depth_hw, HFOV, 0.0, 10.0, rgb_hw=rgb_hw, rgb_hfov_rad=HFOV, max_scenes=4)
    assert [r.add_scene(s) for s in scenes] == [0, 1, 2]
    return r


def _expect(scenes, index, poses, headings, hw, with_rgb):
    from ivln_ce_amd import boxworld as bw

    return [bw.render_reference(scenes[i], p, h, *hw, *bw.intrinsics(*hw, HFOV), 0.0, 10.0, with_rgb=with_rgb)
            for i, p, h in zip(index, poses, headings)]


@pytest.mark.parametrize("depth_hw,rgb_hw", [((24, 40), (20, 28)), ((17, 23), None), ((256, 256), (224, 224)),
                                             ((17, 23), (19, 21))])
def test_kernel_equals_the_float32_reference_bit_for_bit(scenes, depth_hw, rgb_hw):
    """Partial tiles, the W % 4 tail, an odd W (rows that start off a 16-byte boundary), one case without rgb (NULL)."""
    r = _renderer(scenes, depth_hw, rgb_hw)
    out = r.render(INDEX, POSES, HEADINGS)
    assert ("rgb" in out) == (rgb_hw is not None)
    assert out["depth"].shape == (3, *depth_hw, 1) and out["depth"].dtype == torch.float32 and out["depth"].is_cuda
    want = _expect(scenes, INDEX, POSES, HEADINGS, depth_hw, False)
    got_d, got_l = out["depth"].cpu().numpy()[..., 0], out["labels"].cpu().numpy()[..., 0]
    for b in range(3):
        assert np.array_equal(got_d[b].view(np.uint32), want[b]["depth"].view(np.uint32)), f"depth row {b}"
        assert np.array_equal(got_l[b], want[b]["labels"]), f"labels row {b}"
    assert len(np.unique(got_l[0])) >= 4 and not got_l[1].any()
    if rgb_hw is not None:
        want_c = _expect(scenes, INDEX, POSES, HEADINGS, rgb_hw, True)
        got_c = out["rgb"].cpu().numpy()
        assert got_c.shape == (3, *rgb_hw, 3)
        for b in range(3):
            assert np.array_equal(got_c[b], want_c[b]["rgb"]), f"rgb row {b}"
    r.check_status()
    # the next call writes the other buffer set: the views handed out above keep their values
    out2 = r.render([1, 1, 0], POSES[::-1].copy(), [0.5, 0.0, -1.0])
    assert out2["depth"].data_ptr() != out["depth"].data_ptr()
    assert np.array_equal(out["depth"].cpu().numpy()[..., 0], got_d)
    # one row between two steps (an episode reset) goes to that row's own buffers
    d2 = out2["depth"].cpu().numpy()
    row = r.render_row(1, 1, POSES[1], HEADINGS[0])
    w = _expect(scenes, [1], POSES[1:2], HEADINGS[:1], depth_hw, False)[0]
    assert np.array_equal(row["depth"].cpu().numpy()[..., 0], w["depth"]) and bool((row["labels"] == 7).any())
    assert np.array_equal(out2["depth"].cpu().numpy(), d2) and np.array_equal(out["depth"].cpu().numpy()[..., 0], got_d)
    r.check_status()


def test_bad_arguments_are_refused_and_nothing_is_written(scenes):
    from ivln_ce_amd._lib import stream_ptr

    r = _renderer(scenes, (8, 12), (6, 8))
    L, h = r._L, r._h
    idx = torch.zeros(3, dtype=torch.int32, device=DEV)
    pos = torch.tensor(POSES, device=DEV)
    sc = torch.tensor([[0.0, 1.0]] * 3, device=DEV)
    depth = torch.full((3, 8, 12), 7.0, device=DEV)
    lab = torch.full((3, 8, 12), 99, dtype=torch.uint8, device=DEV)
    rgb = torch.full((3, 6, 8, 3), 99, dtype=torch.uint8, device=DEV)

    def call(handle=h, B=3, H=8, W=12, Hr=6, Wr=8, rgb_p=rgb.data_ptr(), fx=6.0):
        return L.ivln_boxworld_render(handle, idx.data_ptr(), pos.data_ptr(), sc.data_ptr(), B, H, W, fx, 4.0, 0.0, 10.0,
                                      depth.data_ptr(), lab.data_ptr(), Hr, Wr, 4.0, 3.0, rgb_p, stream_ptr())

    INVALID = -1
    assert call(handle=None) == INVALID
    assert call(B=0) == INVALID
    assert call(H=0) == INVALID and call(W=0) == INVALID and call(W=-4) == INVALID
    assert call(rgb_p=None) == INVALID          # NULL rgb together with Hr > 0
    assert call(Hr=0, Wr=8) == INVALID and call(fx=0.0) == INVALID
    torch.cuda.synchronize()
    assert bool((depth == 7.0).all()) and bool((lab == 99).all()) and bool((rgb == 99).all())
    assert call(Hr=0, Wr=0, rgb_p=None) == 0    # no rgb asked for: NULL is fine
    torch.cuda.synchronize()
    assert bool((depth != 7.0).all()) and bool((rgb == 99).all())
    r.check_status()
    room = np.array([0, 0, 0, 1, 1, 1], np.float32)
    assert L.ivln_boxworld_add_scene(h, 0, room.ctypes.data, 0, None, None, stream_ptr()) == INVALID   # added before
    assert L.ivln_boxworld_add_scene(h, 9, room.ctypes.data, 0, None, None, stream_ptr()) == INVALID   # outside the table
    assert L.ivln_boxworld_add_scene(h, 3, room.ctypes.data, 33, room.ctypes.data, room.ctypes.data, stream_ptr()) == INVALID
    bad = np.array([0, 0, 0, 1, 0, 1], np.float32)                                                      # lo.y == hi.y
    assert L.ivln_boxworld_add_scene(h, 3, bad.ctypes.data, 0, None, None, stream_ptr()) == INVALID
    assert L.ivln_boxworld_size(h) == 3


def test_scene_index_without_a_table_entry_sets_the_sticky_status(scenes):
    from ivln_ce_amd._lib import IvlnError

    r = _renderer(scenes, (17, 23), (9, 10), b_max=4)
    out = r.render([2, 3, -1, 70000], np.repeat(POSES[:1], 4, 0), [0.3] * 4)   # absent entry, negative, outside the table
    d, l, c = (out[k].cpu().numpy() for k in ("depth", "labels", "rgb"))
    want = _expect(scenes, [2], POSES[:1], [0.3], (17, 23), False)[0]
    assert np.array_equal(d[0, ..., 0], want["depth"]) and np.array_equal(l[0, ..., 0], want["labels"])
    assert np.all(d[1:] == 1.0) and not l[1:].any() and not c[1:].any() and c[0].any()
    with pytest.raises(IvlnError):
        r.check_status()
    r.render([0, 1, 2, 0], np.repeat(POSES[:1], 4, 0), [0.3] * 4)
    with pytest.raises(IvlnError):   # sticky: a later clean call does not clear it
        r.check_status()
    from ivln_ce_amd._lib import stream_ptr

    assert r._L.ivln_boxworld_status(r._h, 1, stream_ptr()) == -1 and r._L.ivln_boxworld_status(r._h, 0, stream_ptr()) == 0


def test_renderer_and_hip_mapper_together_match_the_oracle_and_the_geometry():
    """Two envs, 64 x 64 frames, an 8-step walk in which row 0 sees the label-7 box from two headings and row 1's episode
    resets at step 4: the maps equal oracle/mapper_ref bit for bit (as the mapper tests do on noise), and every point of
    the world cloud lies within 2 mm of a surface of its label in its row's scene - in world coordinates, the frame
    `MappingModule.world_cloud` returns (2 mm: 20 x the float32 rounding of coordinates below 32 m)."""
    from ivln_ce_amd import boxworld as bw
    from ivln_ce_amd.boxworld import BoxWorldRenderer
    from ivln_ce_amd.obs_transforms import GTSemanticsIterativeMapper
    from oracle.mapper_ref import MapperRef

    H = W = 64
    cfg = _cfg("TASK_CONFIG.SIMULATOR.DEPTH_SENSOR.HEIGHT", H, "TASK_CONFIG.SIMULATOR.DEPTH_SENSOR.WIDTH", W)
    room = [-3.0, 0.0, -4.0, 3.5, 2.5, 2.0]
    sc = [bw.Scene(room, [[-0.5, 0.0, -2.0, 0.75, 1.5, -1.5], [1.5, 0.0, -1.0, 2.0, 1.0, 0.0]], [7, 3]),
          bw.Scene(room, [[-2.0, 0.0, -3.0, -1.0, 2.0, -2.5], [0.5, 0.0, -3.5, 1.5, 0.8, -3.0], [2.0, 0.0, 0.5, 3.0, 1.2, 1.5]],
                   [2, 11, 5])]
    r = BoxWorldRenderer(DEV, 2, (H, W), HFOV, 0.0, 10.0)
    for s in sc:
        r.add_scene(s)
    tr = GTSemanticsIterativeMapper.from_config(cfg)
    ref = MapperRef(H, W)
    # row 0: forward, then turns to the left and on; row 1: turns right, resets to a new start at step 4
    pose = np.array([[0.0, 1.25, 0.5], [0.5, 1.25, 0.0]], np.float32)
    heading = [0.0, 0.0]
    step, turn = 0.25, math.radians(15.0)
    seen7 = set()
    for t in range(8):
        not_done = np.ones((2, 1), np.uint8)
        if t == 0:
            not_done[:] = 0
        if t == 4:
            not_done[1] = 0
            pose[1], heading[1] = (-0.5, 1.25, 1.0), math.radians(30.0)
        fr = r.render([0, 1], pose, heading, with_rgb=False)
        orient = np.array([[0.0, heading[0]], [0.0, heading[1]]], np.float64)
        labels = fr["labels"].cpu().numpy()
        if (labels[0] == 7).any():
            seen7.add(round(heading[0], 6))
        T, rot = MapperRef.frames(pose, orient)
        occ_r, sem_r = ref.step(fr["depth"].cpu().numpy(), labels, pose.copy(), orient, not_done, T=T, rot=rot)
        obs = {"depth": fr["depth"], "semantic12": fr["labels"], "world_robot_pose": torch.from_numpy(pose.copy()).to(DEV),
               "world_robot_orientation": torch.from_numpy(orient).to(DEV), "not_done_masks": torch.from_numpy(not_done).to(DEV),
               "env_name": ["bw0", "bw1"]}
        out = tr(obs)
        tr.mapping_module.check_status()
        assert np.array_equal(out["occupancy_map"].cpu().numpy(), occ_r), f"occupancy step {t}"
        assert np.array_equal(out["semantic_map"].cpu().numpy(), sem_r), f"semantic step {t}"
        assert occ_r.any()
        # the walk: row 0 forward once, then left turns; row 1 right turns with a forward in between
        a0 = "F" if t == 0 else "L"
        a1 = "F" if t in (2, 5) else "R"
        for b, a in enumerate((a0, a1)):
            if a == "F":
                pose[b, 0] += np.float32(-step * math.sin(heading[b]))
                pose[b, 2] += np.float32(-step * math.cos(heading[b]))
            else:
                heading[b] += turn if a == "L" else -turn
    assert len(seen7) >= 2, seen7
    xyz, batch, sem = tr.mapping_module.world_cloud()
    xr, br, sr = ref.world()
    assert np.array_equal(xyz.view(np.uint32), xr.view(np.uint32)) and np.array_equal(batch, br) and np.array_equal(sem, sr)
    for b in range(2):
        m = batch == b
        assert m.sum() > 50   # (one point per map cell: the keep-highest of the mapper)
        dist = bw.surface_distance(sc[b], xyz[m], sem[m])
        assert dist.max() <= 2e-3, (b, float(dist.max()), int(sem[m][dist.argmax()]))
        assert (sem[m] > 0).any() and (sem[m] == 0).any()
    assert 7 in sem[batch == 0] and 7 not in sem[batch == 1]


def test_env_frames_are_device_views_and_batch_obs_stacks_them_on_the_device():
    from ivln_ce_amd import boxworld as bw
    from ivln_ce_amd.envs import BoxWorldVectorEnv, construct_envs
    from ivln_ce_amd.utils import batch_obs

    cfg = _cfg("NUM_ENVIRONMENTS", 2, "ENV_BACKEND", "boxworld")
    env = construct_envs(cfg, iterative=False, with_rgb=True, auto_reset_done=False)
    assert type(env) is BoxWorldVectorEnv
    obs = env.reset()
    for t in range(3):
        for o in obs:
            for k, dt in (("depth", torch.float32), ("semantic12", torch.uint8), ("rgb", torch.uint8)):
                assert torch.is_tensor(o[k]) and o[k].is_cuda and o[k].dtype == dt, k   # no host copy of a frame
        batch = batch_obs(obs, DEV)
        assert batch["depth"].shape == (2, 256, 256, 1) and batch["rgb"].shape == (2, 224, 224, 3) and batch["depth"].is_cuda
        e = env._envs[1]
        f = bw.render_reference(e.scene, obs[1]["world_robot_pose"], obs[1]["world_robot_orientation"][1], 256, 256,
                                *e.depth_f, 0.0, 10.0, with_rgb=False)
        assert np.array_equal(batch["depth"][1, ..., 0].cpu().numpy(), f["depth"])
        assert np.array_equal(batch["semantic12"][1, ..., 0].cpu().numpy(), f["labels"])
        held = obs[0]["depth"].clone()
        nxt = [x[0] for x in env.step([2, 1])]
        assert torch.equal(obs[0]["depth"], held)   # the views of step t are still valid after step t + 1
        obs = nxt
    held = obs[1]["depth"].clone()
    one = env.reset_at(0)[0]
    assert one["depth"].is_cuda and torch.equal(obs[1]["depth"], held)   # a reset of env 0 leaves env 1's frames alone
    env.check_status()
    env.close()


def _loop_cfg(tmp_path, *extra):
    return _cfg(
        "TRAINER_NAME", "dagger", "NUM_ENVIRONMENTS", 2, "ENV_BACKEND", "boxworld", "MODEL.policy_name", "MapCMAPolicy",
        "MODEL.INSTRUCTION_ENCODER.use_pretrained_embeddings", False, "MODEL.DEPTH_ENCODER.ddppo_checkpoint", "NONE",
        "RL.POLICY.OBS_TRANSFORMS.ENABLED_TRANSFORMS", ["GTSemanticsIterativeMapper"],
        "IL.DAGGER.iterations", 1, "IL.DAGGER.update_size", 4, "IL.DAGGER.p", 0.5, "IL.epochs", 1, "IL.batch_size", 2,
        "IL.DAGGER.lmdb_features_dir", str(tmp_path / "traj"), "CHECKPOINT_FOLDER", str(tmp_path / "ckpt"),
        "RESULTS_DIR", str(tmp_path / "res"), "EVAL_CKPT_PATH_DIR", str(tmp_path / "none.pth"), "EVAL.SAVE_RESULTS", False,
        *extra)


@pytest.fixture
def three_episodes(monkeypatch):
    from ivln_ce_amd import trainers

    real = trainers.construct_envs
    monkeypatch.setattr(trainers, "construct_envs", lambda *a, **k: real(*a, n_episodes=3, **k))
    monkeypatch.delenv("IVLN_ENV_BACKEND", raising=False)


def test_evaluation_on_boxworld_replayed_equals_eager(tmp_path, same_depth_path, three_episodes):
    import ivln_ce_amd  # noqa: F401
    from ivln_ce_amd import trainers  # noqa: F401
    from ivln_ce_amd.registry import baseline_registry

    same_depth_path(2)
    out = {}
    for mode in (True, False):
        torch.manual_seed(0)
        cfg = _loop_cfg(tmp_path, "EVAL.USE_HIP_GRAPH", mode)
        tr = baseline_registry.get_trainer("dagger")(cfg)
        res = tr._eval_checkpoint(str(tmp_path / "none.pth"))
        res.pop("eval_seconds")
        out[mode] = res
    assert out[True] == out[False], f"graph {out[True]} vs eager {out[False]}"
    assert out[True]["episodes"] == 6
    assert all(np.isfinite(v) for v in out[True].values() if isinstance(v, (int, float)))


def test_one_dagger_iteration_on_boxworld(tmp_path, three_episodes):
    import ivln_ce_amd  # noqa: F401
    from ivln_ce_amd import trainers  # noqa: F401
    from ivln_ce_amd.registry import baseline_registry

    torch.manual_seed(0)
    tr = baseline_registry.get_trainer("dagger")(_loop_cfg(tmp_path))
    log = tr.train()
    assert len(log) >= 1 and all(np.isfinite(l["loss"]) for l in log)
    assert len(tr.store) >= 4
