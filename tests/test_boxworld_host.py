"""CPU: the box-world backend (ivln_ce_amd/boxworld.py, envs.BoxWorldVectorEnv; ENV_BACKEND "boxworld").

`boxworld.render_reference` in float32 is the oracle of the device renderer (tests/test_gpu_boxworld.py) and the CPU path
of the backend, so it is held here to the same recipe in float64, to closed forms, and to the mapper's un-projection
convention; the vector env is held to `SyntheticVectorEnv`'s protocol, and its collision rules to the scene."""
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HFOV = math.pi / 2
CAM = (0.3, 1.25, -1.0)


def _cfg(*opts):
    from ivln_ce_amd.config import get_config

    return get_config(opts=list(opts) or None)


@pytest.fixture(scope="module")
def scene12():
    from ivln_ce_amd import boxworld as bw

    sc = bw.make_scene(11, _cfg())
    assert len(sc.boxes) == 12 and not sc.blocked(CAM, 0.2)  # (the camera stands clear of every box)
    return sc


def _render(sc, pos, heading, H, W, dtype=np.float32, dmax=10.0, **kw):
    from ivln_ce_amd import boxworld as bw

    return bw.render_reference(sc, pos, heading, H, W, *bw.intrinsics(H, W, HFOV), 0.0, dmax, dtype=dtype, **kw)


def test_float32_recipe_against_the_same_recipe_in_float64(scene12):
    """24 headings x two frame sizes of a seeded 12-box scene: label / face disagreement on at most 0.5 % of a frame's
    pixels and |depth32 - depth64| <= 1e-5 on the agreeing ones (30 x what a float32 restatement showed: 0 disagreeing
    pixels of 97 024, 3.0e-7; a half-pixel or focal-length mistake moves depth by 1e-3 or more)."""
    worst_bad, worst_err, total = 0.0, 0.0, 0
    for H, W in ((64, 64), (24, 40)):
        for k in range(24):
            h = math.radians(15.0 * k)
            a, b = _render(scene12, CAM, h, H, W), _render(scene12, CAM, h, H, W, dtype=np.float64)
            assert a["depth"].dtype == np.float32 and b["depth"].dtype == np.float64
            agree = (a["labels"] == b["labels"]) & (a["face"] == b["face"])
            bad = 1.0 - agree.mean()
            err = float(np.abs(a["depth"].astype(np.float64) - b["depth"])[agree].max())
            worst_bad, worst_err, total = max(worst_bad, bad), max(worst_err, err), total + H * W
            assert bad <= 0.005, (H, W, k, bad)
            assert err <= 1e-5, (H, W, k, err)
    print(f"float32 vs float64: worst disagreement {worst_bad:.4%}, worst depth error {worst_err:.2e} over {total} pixels")
    assert len(np.unique(_render(scene12, CAM, 0.0, 64, 64)["labels"])) >= 3  # (the frames are not one wall)


def test_empty_room_depth_is_the_analytic_wall_distance():
    from ivln_ce_amd import boxworld as bw

    sc = bw.Scene([-2.0, 0.0, -3.0, 2.5, 2.5, 1.0], np.zeros((0, 6)), [])
    o = np.array([0.25, 1.25, -0.5])
    for h in (0.0, math.radians(40.0), math.radians(-165.0)):
        H, W = 24, 40
        f = _render(sc, o, h, H, W)
        fx, fy = bw.intrinsics(H, W, HFOV)
        xs = (np.arange(W) + 0.5 - W / 2) / fx
        ys = (np.arange(H) + 0.5 - H / 2) / fy
        d = np.stack(np.broadcast_arrays((xs * math.cos(h) - math.sin(h))[None, :], (-ys)[:, None],
                                         (-xs * math.sin(h) - math.cos(h))[None, :]), -1)
        with np.errstate(divide="ignore"):
            t = np.where(d > 0, (sc.room[3:] - o) / d, np.where(d < 0, (sc.room[:3] - o) / d, np.inf)).min(-1)
        # float32 rounding of xs, d and t: a few ulp of values below 1 (6e-8 each)
        assert np.abs(f["depth"] - np.clip(t / 10.0, 0, 1)).max() <= 1e-6
        assert not f["labels"].any()
    # heading 0, the wall ahead: z-depth is the same for every pixel that sees it, whatever its ray's length
    f = _render(sc, o, 0.0, 24, 40)
    assert np.all(f["depth"][f["face"] == 4] == np.float32(2.5) / np.float32(10.0)) and (f["face"] == 4).sum() > 100


def test_odd_width_centre_column_takes_the_parallel_slab_branch():
    from ivln_ce_amd import boxworld as bw

    o = (0.0, 1.25, 0.0)
    ahead = [-0.5, 0.0, -2.0, 0.5, 2.5, -1.5]   # straddles x = 0: the centre column sees it
    aside = [0.75, 0.0, -1.0, 1.5, 2.5, -0.5]   # x = 0 is outside its slab: the centre column must not
    sc = bw.Scene([-3.0, 0.0, -4.0, 3.0, 2.5, 2.0], [aside, ahead], [5, 7])
    H, W = 17, 23
    f = _render(sc, o, 0.0, H, W)
    fx, _ = bw.intrinsics(H, W, HFOV)
    xs = ((np.arange(W, dtype=np.float32) + np.float32(0.5)) - np.float32(W / 2.0)) / np.float32(fx)
    assert xs[W // 2] == 0.0  # d.x == 0 exactly at heading 0
    mid = f["labels"][H // 2 - 2:H // 2 + 2, W // 2]
    assert np.all(mid == 7) and np.all(f["depth"][H // 2 - 2:H // 2 + 2, W // 2] == np.float32(1.5) / np.float32(10))
    assert not (f["labels"][:, W // 2] == 5).any() and (f["labels"] == 5).any()
    assert np.isfinite(f["depth"]).all()
    # a camera whose x lies on the slab boundary is inside that slab
    sc2 = bw.Scene(sc.room, [[0.0, 0.0, -2.0, 0.5, 2.5, -1.5]], [3])
    assert _render(sc2, o, 0.0, H, W)["labels"][H // 2, W // 2] == 3


def test_box_flush_with_a_wall_and_camera_inside_a_box():
    from ivln_ce_amd import boxworld as bw

    room = [-3.0, 0.0, -4.0, 3.0, 2.5, 2.0]
    flush_far = [-0.5, 0.0, -4.0, 0.5, 2.5, -3.0]   # its back face lies in the far wall
    flush_side = [2.0, 0.0, -3.5, 3.0, 2.5, -2.5]   # its side face lies in the +x wall
    sc = bw.Scene(room, [flush_far, flush_side], [2, 9])
    o = (0.0, 1.25, 0.0)
    f = _render(sc, o, 0.0, 32, 32)
    assert f["labels"][16, 16] == 2 and f["depth"][16, 16] == np.float32(3.0) / np.float32(10)
    assert (f["labels"] == 9).any() and np.isfinite(f["depth"]).all()
    g = _render(sc, (0.0, 1.25, -3.0), math.radians(-90.0), 32, 32)  # looking along +x: the side box's face at x = 2
    assert g["labels"][16, 16] == 9 and abs(float(g["depth"][16, 16]) - 0.2) <= 1e-6
    # a camera inside a box does not see that box: the frame is the frame without it
    around = [-0.4, 0.0, -0.4, 0.4, 2.0, 0.4]
    with_box = bw.Scene(room, [flush_far, around, flush_side], [2, 4, 9])
    for h in (0.0, 1.0, 2.5):
        a, b = _render(with_box, o, h, 32, 32), _render(sc, o, h, 32, 32)
        assert not (a["labels"] == 4).any()
        for k in ("depth", "labels", "face", "rgb"):
            assert np.array_equal(a[k], b[k]), k


def test_row_order_a_box_above_the_optical_axis_is_in_the_upper_rows():
    from ivln_ce_amd import boxworld as bw

    sc = bw.Scene([-3.0, 0.0, -4.0, 3.0, 2.5, 2.0], [[-0.5, 1.6, -2.5, 0.5, 2.0, -2.0]], [6])
    H = 32
    f = _render(sc, (0.0, 1.25, 0.0), 0.0, H, 32)
    rows = np.nonzero((f["labels"] == 6).any(axis=1))[0]
    assert len(rows) > 0 and rows.max() < H // 2
    # its +z face looks at the camera, and from below the camera also sees its underside (-y)
    assert set(np.unique(f["face"][f["labels"] == 6]).tolist()) == {2, 5}
    assert f["rgb"].dtype == np.uint8 and f["rgb"].shape == (H, 32, 3)
    px = tuple(np.argwhere((f["labels"] == 6) & (f["face"] == 5))[0])
    assert np.array_equal(f["rgb"][px], (bw.PALETTE[6].astype(np.int32) * bw.SHADE[5]) >> 8)
    floor = f["rgb"][(f["face"] == 2) & (f["labels"] == 0)]
    assert len(np.unique(floor.reshape(-1, 3), axis=0)) == 2  # the label-0 checker: two palette rows


def test_unprojected_pixels_lie_on_a_surface_of_their_label(scene12):
    """The mapper's convention without the mapper: every pixel with 0.1 < depth * 10 < 9, un-projected in float64 by the
    issue's formulas, lies within 2 mm of a surface carrying its label (20 x the float32 rounding of coordinates below
    32 m, 50 x below a map cell)."""
    from ivln_ce_amd import boxworld as bw

    seen = set()
    for H, W in ((64, 64), (24, 40)):
        fx, fy = bw.intrinsics(H, W, HFOV)
        for k in range(0, 24, 3):
            h = math.radians(15.0 * k + 4.0)
            f = _render(scene12, CAM, h, H, W)
            z = f["depth"].astype(np.float64) * 10.0
            keep = (z > 0.1) & (z < 9.0)
            pts = bw.unproject(f["depth"], CAM, h, fx, fy, 0.0, 10.0)[keep]
            dist = bw.surface_distance(scene12, pts, f["labels"][keep])
            assert keep.sum() > 0.5 * H * W and dist.max() <= 2e-3, (H, W, k, dist.max())
            seen |= set(np.unique(f["labels"][keep]).tolist())
    assert 0 in seen and len(seen) >= 4


# ---- the vector env -----------------------------------------------------------------------------------------------
SMALL = ("TASK_CONFIG.SIMULATOR.DEPTH_SENSOR.HEIGHT", 32, "TASK_CONFIG.SIMULATOR.DEPTH_SENSOR.WIDTH", 32,
         "TASK_CONFIG.SIMULATOR.RGB_SENSOR.HEIGHT", 28, "TASK_CONFIG.SIMULATOR.RGB_SENSOR.WIDTH", 28)


def _signature(o):
    return {k: (type(v).__name__,) if not hasattr(v, "shape") else (str(v.dtype), tuple(v.shape)) for k, v in o.items()}


@pytest.mark.parametrize("iterative", [False, True])
@pytest.mark.parametrize("with_rgb", [False, True])
@pytest.mark.parametrize("rxr", [False, True])
def test_env_protocol_equals_the_synthetic_envs(iterative, with_rgb, rxr):
    from ivln_ce_amd.envs import BoxWorldVectorEnv, SyntheticVectorEnv

    opts = SMALL + (("TASK_CONFIG.TASK.INSTRUCTION_SENSOR_UUID", "rxr_instruction") if rxr else ())
    cfg = _cfg("NUM_ENVIRONMENTS", 2, *opts)
    kw = dict(n_episodes=3, episodes_per_tour=2, min_len=4, max_len=6, with_rgb=with_rgb, with_semantic=True,
              iterative=iterative, seed=9, rank=0, world=1)
    a, b = SyntheticVectorEnv(cfg, **kw), BoxWorldVectorEnv(cfg, device="cpu", **kw)
    assert a.num_envs == b.num_envs == 2 and a.number_of_episodes == b.number_of_episodes

    def spaces(env):
        return [{k: (s.shape, np.dtype(s.dtype)) for k, s in sp.spaces.items()} for sp in env.observation_spaces]

    assert spaces(a) == spaces(b)
    ra, rb = a.reset(), b.reset()
    for t in range(12):
        for xa, xb in zip(ra, rb):
            assert len(xa) == len(xb) if iterative or t else True
            oa, ob = (xa[0], xb[0]) if (iterative or t) else (xa, xb)
            assert list(oa) == list(ob) and _signature(oa) == _signature(ob)
            assert ob["env_name"].startswith("bw") and ("rxr_instruction" in ob) == rxr and ("rgb" in ob) == with_rgb
            assert isinstance(ob["depth"], np.ndarray) and 0.0 <= ob["depth"].min() and ob["depth"].max() <= 1.0
            assert ob["semantic12"].max() <= 12
            sp = b.observation_spaces[0].spaces
            assert all(sp[k].shape == tuple(ob[k].shape) and sp[k].dtype == ob[k].dtype for k in sp)
        acts = [int(x[0]["shortest_path_sensor"][0]) if (iterative or t) else int(x["shortest_path_sensor"][0]) for x in rb]
        ra, rb = a.step(acts), b.step(acts)
    o = b.reset_at(1)[0]
    o = o[0] if iterative else o
    assert o["env_name"] == "bw1" and o["depth"].shape == (32, 32, 1) and o["semantic12"].dtype == np.uint8
    a.close()
    b.close()


def test_same_seed_same_frames_and_frames_follow_the_pose():
    from ivln_ce_amd.envs import BoxWorldVectorEnv

    cfg = _cfg("NUM_ENVIRONMENTS", 2, *SMALL)
    envs = [BoxWorldVectorEnv(cfg, device="cpu", seed=4, with_rgb=True, iterative=False) for _ in range(2)]
    obs = [e.reset() for e in envs]
    first = obs[0][0]["depth"].copy()
    for t in range(6):
        for oa, ob in zip(*obs):
            for k in ("depth", "semantic12", "rgb", "world_robot_pose"):
                assert np.array_equal(oa[k], ob[k]), (t, k)
        obs = [[x[0] for x in e.step([2, 1])] for e in envs]   # env 0 turns, env 1 walks
    assert not np.array_equal(obs[0][0]["depth"], first)        # the view changed with the heading
    e0 = envs[0]._envs[0]
    from ivln_ce_amd import boxworld as bw

    f = bw.render_reference(e0.scene, obs[0][0]["world_robot_pose"], obs[0][0]["world_robot_orientation"][1], 32, 32,
                            *bw.intrinsics(32, 32, HFOV), 0.0, 10.0)
    assert np.array_equal(obs[0][0]["depth"][..., 0], f["depth"]) and np.array_equal(obs[0][0]["semantic12"][..., 0], f["labels"])


def test_collisions_blocked_steps_keep_the_pose_and_expert_paths_are_free():
    from ivln_ce_amd.envs import FORWARD, BoxWorldVectorEnv, _advance

    cfg = _cfg("NUM_ENVIRONMENTS", 3, *SMALL)
    for iterative in (False, True):
        env = BoxWorldVectorEnv(cfg, device="cpu", seed=21, iterative=iterative, n_episodes=6, min_len=20, max_len=40,
                                with_semantic=False)
        for e in env._envs:
            r = e.radius
            for ep in e.episodes:
                pose, heading = ep.start.copy(), ep.start_heading
                for a in ep.script:      # the scripted expert never meets a wall or a box
                    before = pose.copy()
                    heading = _advance(pose, heading, a)
                    assert not e.scene.blocked(pose, r)
                    assert a == FORWARD or np.array_equal(before, pose)
                assert np.array_equal(np.float32(e._gt_positions(ep)[-1]), ep.goal)
            for tour in e.expert_path().values():
                for p in tour:
                    assert not e.scene.blocked(p["position"], r)
        # an agent that only walks forward ends up against something and stays there
        env.reset()
        blocked = 0
        for t in range(60):
            before = [(e.pose.copy(), e._forward_blocked(e.pose, e.heading), e.phase, e.ep_i) for e in env._envs]
            env.step([FORWARD] * env.num_envs)
            for e, (pose, was_blocked, phase, ep_i) in zip(env._envs, before):
                assert not e.scene.blocked(e.pose, e.radius)
                if was_blocked and phase == "agent" and e.phase == "agent" and e.ep_i == ep_i:
                    assert np.array_equal(e.pose, pose)
                    blocked += 1
        assert blocked > 0
        env.close()


def test_long_scripts_do_meet_obstacles_and_are_rewritten():
    """(the property above is not vacuous: with 40-step scripts in a 12-box room some FORWARDs were blocked and replaced)"""
    from ivln_ce_amd.envs import SyntheticVectorEnv, BoxWorldVectorEnv

    cfg = _cfg("NUM_ENVIRONMENTS", 3, *SMALL)
    kw = dict(seed=21, iterative=False, n_episodes=6, min_len=30, max_len=40)
    a, b = SyntheticVectorEnv(cfg, **kw), BoxWorldVectorEnv(cfg, device="cpu", **kw)
    scripts_a = [ep.script for e in a._envs for ep in e.episodes]
    scripts_b = [ep.script for e in b._envs for ep in e.episodes]
    assert [len(s) for s in scripts_a] == [len(s) for s in scripts_b]
    assert [ep.tokens.tolist() for e in a._envs for ep in e.episodes] == [ep.tokens.tolist() for e in b._envs for ep in e.episodes]
    assert scripts_a != scripts_b


def test_construct_envs_backends(monkeypatch):
    from ivln_ce_amd import envs

    monkeypatch.delenv("IVLN_ENV_BACKEND", raising=False)
    cfg = _cfg("NUM_ENVIRONMENTS", 2, "ENV_BACKEND", "boxworld", *SMALL)
    e = envs.construct_envs(cfg, device="cpu")
    assert type(e) is envs.BoxWorldVectorEnv
    assert sorted(e.scenes()) == ["bw0", "bw1"]
    e.close()
    cfg = _cfg("NUM_ENVIRONMENTS", 2)
    assert cfg.ENV_BACKEND == "synthetic"
    s = envs.construct_envs(cfg, with_rgb=True)
    assert type(s) is envs.SyntheticVectorEnv
    o = s.reset()[0]
    # the synthetic backend's first observation: values recorded before the box-world backend existed
    assert o["env_name"] == "scene0" and o["depth"].shape == (256, 256, 1)
    assert (float(o["depth"].astype(np.float64).sum()), int(o["semantic12"].astype(np.int64).sum()),
            int(o["rgb"].astype(np.int64).sum()), int(o["instruction"].sum())) == SYNTHETIC_FIRST_OBS
    s.close()
    monkeypatch.setenv("IVLN_ENV_BACKEND", "boxworld")
    e = envs.construct_envs(_cfg("NUM_ENVIRONMENTS", 1, *SMALL), device="cpu")
    assert type(e) is envs.BoxWorldVectorEnv
    e.close()
    monkeypatch.setenv("IVLN_ENV_BACKEND", "habitat")
    with pytest.raises(NotImplementedError):
        envs.construct_envs(cfg)


# (sum of depth in float64, of semantic12, of rgb, of the instruction tokens: env 0 of the default config, seed and sizes)
SYNTHETIC_FIRST_OBS = (32815.51239591837, 394536, 19189041, 33235)


def test_header_symbols_are_exported_and_the_source_is_built():
    import importlib.util

    import __graft_entry__ as ge

    ge.build()
    spec = importlib.util.spec_from_file_location("ivln_build_bw", os.path.join(ROOT, "ivln-ce_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.SOURCES["boxworld.hip"] == ["-ffp-contract=off"]
    from ivln_ce_amd._lib import lib

    header = open(os.path.join(ROOT, "include", "ivln_boxworld.h")).read()
    names = re.findall(r"^int (ivln_boxworld_\w+)\(", header, flags=re.M)
    assert set(names) >= {"ivln_boxworld_create", "ivln_boxworld_add_scene", "ivln_boxworld_destroy", "ivln_boxworld_render"}
    for n in names:
        assert hasattr(lib(), n), n
    assert int(re.search(r"#define IVLN_BW_MAX_BOXES (\d+)", header).group(1)) == 32
