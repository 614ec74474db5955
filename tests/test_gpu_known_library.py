"""GPU: known-map mode over the device-resident scene library (include/ivln_known_lib.h, mapping.KnownSceneLibrary,
MappingModule(known_library=True)).  Bit-exact occupancy / semantic maps and world counts at every step against the C
oracle (oracle.mapper_ref), the copy path (ivln_mapper_known_begin / _load_known / _known_raster) and the reference's own
golden; the step captured once and replayed with only `stage_host` on the host; argument checks; and the trainer's
evaluation loop and DAgger collection replayed against their eager runs."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _scene(rng, n, centre=(0.0, 0.0), span=4.0):
    """n points, x / z on a 5 cm lattice (many points per 10 cm cell: ties decide), labels 0..12 - as
    tests/test_gpu_mapper.py::test_known_map_mode_matches_oracle builds its scenes."""
    xyz = np.stack([rng.uniform(-span, span, n) + centre[0], rng.uniform(0.0, 2.5, n),
                    rng.uniform(-span, span, n) + centre[1]], 1).astype(np.float32)
    xyz[:, [0, 2]] = np.round(xyz[:, [0, 2]] / 0.05) * 0.05
    return xyz, rng.randint(0, 13, n).astype(np.int64)


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """Scene files + their clouds as the oracle takes them: 0 points, 1 point, 257 points (one past a workgroup's first
    pass), and 5000-point scenes with ties."""
    d = tmp_path_factory.mktemp("known_scenes")
    rng = np.random.RandomState(0)
    raw = {
        "empty": (np.zeros((0, 3), np.float32), np.zeros((0,), np.int64)),
        "one": (np.array([[0.1, 1.3, 0.2]], np.float32), np.array([7], np.int64)),
        "s257": _scene(rng, 257, span=2.0),
        "big": _scene(rng, 5000),
        "big2": _scene(rng, 5000),
    }
    clouds = {}
    for name, (xyz, sem) in raw.items():
        np.savez(d / f"{name}.npz", xyz=xyz, semantics=sem)
        clouds[name] = (xyz, sem.astype(np.uint8))
    return str(d), clouds


def _module(loc, b_max, library):
    from ivln_ce_amd.mapping import MapDimensions, MappingModule

    return MappingModule(torch.device(DEV), None, MapDimensions(6.4, 6.4, 0.1), mode="known", maps_location=loc,
                         b_max=b_max, known_library=library)


def _pose(t, B):
    pose = np.array([[0.3 * t, 1.25, -0.2 * t], [-0.5, 1.3, 0.4 * t], [0.2 * t - 0.6, 1.2, 0.1], [0.05 * t, 1.25, 0.1 * t]],
                    np.float32)[:B]
    orient = np.array([[0.0, 0.4 * t], [0.0, -0.7 * t], [0.0, 0.25 * t + 1.0], [0.0, 3.0 - 0.5 * t]], np.float64)[:B]
    return np.ascontiguousarray(pose), np.ascontiguousarray(orient)


def _obs(pose, orient, nd, names):
    B = len(names)
    return {"depth": torch.zeros(B, 16, 16, 1, device=DEV), "world_robot_pose": torch.from_numpy(pose).to(DEV),
            "world_robot_orientation": torch.from_numpy(orient).to(DEV),
            "not_done_masks": torch.from_numpy(np.asarray(nd, np.uint8).reshape(-1, 1)).to(DEV), "env_name": list(names)}


# (not_done per row, scene name per row): every row but the last resets at t = 0 - the last one has not_done = 1 there and
# was never loaded (empty maps) until it resets at t = 1; row 0 never resets again; row 1 resets every step to alternating
# scenes; rows 0 and 2 share a scene; at t = 3, 4 the batch is 2 rows; at t = 5 rows 2 and 3 are back WITHOUT a reset
# (paused rows were cleared: empty); they reset at t = 6
SCRIPT = [
    ([0, 0, 0, 1], ["big", "big2", "big", "one"]),
    ([1, 0, 1, 0], ["big", "s257", "big", "one"]),
    ([1, 0, 1, 1], ["big", "big2", "big", "one"]),
    ([1, 0], ["big", "s257"]),
    ([1, 0], ["big", "empty"]),
    ([1, 0, 1, 1], ["big", "big2", "s257", "empty"]),
    ([1, 0, 0, 0], ["big", "one", "s257", "empty"]),
    ([1, 0, 1, 1], ["big", "big2", "s257", "empty"]),
]


def test_library_steps_match_oracle_and_copy_path(scenes):
    from oracle.mapper_ref import MapperRef

    loc, clouds = scenes
    lib_m, copy_m, ref = _module(loc, 4, True), _module(loc, 4, False), MapperRef(16, 16)
    assert lib_m.known_library and not copy_m.known_library
    for t, (nd, names) in enumerate(SCRIPT):
        B = len(names)
        pose, orient = _pose(t, B)
        occ_r, sem_r = ref.known_step(clouds, names, pose, orient, np.asarray(nd, np.uint8))
        mem = lib_m(_obs(pose, orient, nd, names))
        n_lib = lib_m.check_status()
        occ, sem = mem.occupancy.cpu().numpy(), mem.semantic.cpu().numpy()
        mem_c = copy_m(_obs(pose, orient, nd, names))
        n_copy = copy_m.check_status()
        assert occ.shape == (B, 64, 64)
        assert np.array_equal(occ, occ_r), f"occupancy vs oracle, step {t}"
        assert np.array_equal(sem, sem_r), f"semantic vs oracle, step {t}"
        assert np.array_equal(occ, mem_c.occupancy.cpu().numpy()), f"occupancy vs copy path, step {t}"
        assert np.array_equal(sem, mem_c.semantic.cpu().numpy()), f"semantic vs copy path, step {t}"
        assert n_lib == n_copy == ref.world()[0].shape[0], f"world count step {t}: {n_lib} / {n_copy}"
        if t == 0:
            assert occ[3].sum() == 0 and sem[3].sum() == 0  # not_done = 1 and never loaded
            assert occ[0].sum() > 100 and len(np.unique(sem[0])) > 5
        if t == 5:
            assert occ[2].sum() == 0 and occ[3].sum() == 0  # back from a pause without a reset
        if t == 6:
            assert occ[2].sum() > 0
    assert len(lib_m.scene_library) == 5  # every scene once, whatever the number of rows and resets that used it


def test_rotation_bits_equal_ivln_mapper_frames(scenes):
    """The step derives the ego rotation itself; a map rastered with it equals the copy path's, which takes the
    rotation of ivln_mapper_frames, at headings where sin / cos round differently in float and double."""
    loc, _ = scenes
    lib_m, copy_m = _module(loc, 2, True), _module(loc, 2, False)
    for t, heading in enumerate([0.1, 1.0471975511965976, 2.2, -3.0, 5.5]):
        pose = np.array([[0.0, 1.25, 0.0], [0.3, 1.25, -0.3]], np.float32)
        orient = np.array([[0.0, heading], [0.2, -heading]], np.float64)
        nd = [0, 0] if t == 0 else [1, 1]
        a = lib_m(_obs(pose, orient, nd, ["big", "big2"]))
        b = copy_m(_obs(pose, orient, nd, ["big", "big2"]))
        assert torch.equal(a.occupancy, b.occupancy) and torch.equal(a.semantic, b.semantic), f"heading {heading}"


@pytest.mark.parametrize("plugin,sub", [("GTSemanticsKnownMapper", "gt_semantics"),
                                        ("PredictedSemanticsKnownMapper", "predicted_semantics")])
def test_plugins_in_library_mode_match_reference_golden(plugin, sub, tmp_path, monkeypatch):
    """tests/golden/known_map.npz (the reference's own `create_known_mapper` run) through both plugins as `from_config`
    builds them: library mode.  Maps equal occ_t / sem_t, the count equals world_n_t."""
    from ivln_ce_amd import obs_transforms  # noqa: F401
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.registry import baseline_registry

    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "known_map.npz"))
    names = [str(x) for x in g["env_names"]]
    d = tmp_path / "data" / "known_maps" / sub
    d.mkdir(parents=True)
    for n in set(names):
        np.savez(d / f"{n}.npz", xyz=g[f"scene_{n}_xyz"], semantics=g[f"scene_{n}_semantics"])
    monkeypatch.chdir(tmp_path)
    tr = baseline_registry.get_obs_transformer(plugin).from_config(get_config())
    B = int(g["B"])
    for t in range(int(g["steps"])):
        obs = {"depth": torch.zeros(B, 16, 16, 1, device=DEV),
               "world_robot_pose": torch.from_numpy(g[f"pose_{t}"]).to(DEV),
               "world_robot_orientation": torch.from_numpy(g[f"orientation_{t}"]).to(DEV),
               "not_done_masks": torch.from_numpy(g[f"not_done_{t}"]).to(DEV), "env_name": list(names)}
        out = tr(obs)
        assert tr.mapping_module.known_library and tr.mapping_module.mode == "known"
        n = tr.mapping_module.check_status()
        assert np.array_equal(out["occupancy_map"].cpu().numpy(), g[f"occ_{t}"]), f"occupancy step {t}"
        assert np.array_equal(out["semantic_map"].cpu().numpy(), g[f"sem_{t}"]), f"semantic step {t}"
        assert n == int(g[f"world_n_{t}"]), f"count step {t}"
    assert len(tr.mapping_module.scene_library) == len(set(names))


def test_captured_step_replays_with_only_stage_host_on_the_host(scenes, tmp_path):
    """One library step captured at B = 3 (a capture allows no synchronisation: it is the proof that nothing inside the step
    reads the device), replayed over a script in which scene indices and not_done change between replays; a scene whose file
    does not even exist at capture time is added between two replays and shows in the next one."""
    import shutil

    loc0, clouds = scenes
    loc = tmp_path / "maps"
    loc.mkdir()
    for name in ("big", "big2", "s257", "one"):
        shutil.copy(os.path.join(loc0, f"{name}.npz"), loc / f"{name}.npz")
    B = 3
    m, eager = _module(str(loc), 4, True), _module(str(loc), 4, True)
    pose, orient = _pose(0, B)
    static = _obs(pose, orient, [0, 0, 0], ["big", "big", "big"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up: the handle and the library exist before the capture
        m(static)
    torch.cuda.current_stream().wait_stream(side)
    m.reset()  # (what the trainers do after the first capture's warm-up: the latches are empty again)
    graph = torch.cuda.CUDAGraph()
    assert m.check_status() == 0  # no row holds a scene after the reset
    with torch.cuda.graph(graph):
        mem = m(static)
    script = [
        ([0, 0, 0], ["big", "s257", "big"]),
        ([1, 0, 1], ["big", "big2", "big"]),
        ([1, 1, 0], ["big", "big2", "late"]),  # "late" is written below, after the capture
        ([0, 1, 1], ["late", "one", "late"]),
        ([1, 0, 1], ["late", "one", "late"]),
    ]
    rng = np.random.RandomState(5)
    late = _scene(rng, 1000, span=3.0)
    for t, (nd, names) in enumerate(script):
        if t == 2:
            np.savez(loc / "late.npz", xyz=late[0], semantics=late[1])
            assert "late" not in m.scene_library
        pose, orient = _pose(t, B)
        obs = _obs(pose, orient, nd, names)
        for k in ("world_robot_pose", "world_robot_orientation", "not_done_masks"):
            static[k].copy_(obs[k])
        m.stage_host({"env_name": names})
        graph.replay()
        ref = eager(obs)
        assert torch.equal(mem.occupancy, ref.occupancy), f"occupancy step {t}"
        assert torch.equal(mem.semantic, ref.semantic), f"semantic step {t}"
        assert m.check_status() == eager.check_status()
        if t == 2:
            assert "late" in m.scene_library and int(mem.occupancy[2].sum()) > 50
    assert int(mem.occupancy.sum()) > 0


def test_argument_checks_and_a_scene_that_was_never_added(scenes):
    from ivln_ce_amd._lib import IvlnError, lib, stream_ptr
    from ivln_ce_amd.mapping import KnownSceneLibrary
    from oracle.mapper_ref import MapperRef

    loc, clouds = scenes
    L = lib()
    klib = KnownSceneLibrary(torch.device(DEV), loc, max_scenes=4)
    h = klib.handle()
    xyz = torch.zeros(8, 3, device=DEV)
    sem = torch.zeros(8, dtype=torch.uint8, device=DEV)
    rec = torch.zeros(9, 4, device=DEV)
    add = lambda scene, n, x=xyz, s=sem, r=rec.data_ptr(): L.ivln_known_lib_add(  # noqa: E731
        h, scene, x.data_ptr() if x is not None else None, s.data_ptr() if s is not None else None, n, r, stream_ptr())
    assert add(-1, 8) == -1 and add(4, 8) == -1  # scene index outside the table
    assert add(0, -1) == -1 and add(0, 1 << 31) == -1  # size
    assert add(0, 8, x=None) == -1 and add(0, 8, s=None) == -1 and add(0, 8, r=None) == -1  # NULL operands
    assert add(0, 8, r=rec.data_ptr() + 4) == -1  # records off a 16-byte boundary
    assert L.ivln_known_lib_size(h) == 0  # nothing was entered by a refused call
    assert add(0, 8) == 0 and L.ivln_known_lib_size(h) == 1
    assert add(0, 8) == -1  # an entry a captured step may be reading is not rewritten
    assert add(3, 0, x=None, s=None, r=None) == 0  # an empty scene needs no memory
    torch.cuda.synchronize()

    # a row latches an index with no entry (7: inside the table, 100000: outside it)
    m = _module(loc, 4, True)
    for name in ("big", "s257"):
        m.scene_library.index(name)
    m.scene_library._index["ghost"] = 7
    m.scene_library._index["far"] = 100000
    names = ["big", "ghost", "s257", "far"]
    pose, orient = _pose(1, 4)
    mem = m(_obs(pose, orient, [0, 0, 0, 0], names))
    with pytest.raises(IvlnError, match="invalid"):
        m.check_status()
    nothing = (np.zeros((0, 3), np.float32), np.zeros((0,), np.uint8))
    occ_r, sem_r = MapperRef(16, 16).known_step(dict(clouds, ghost=nothing, far=nothing), names, pose, orient,
                                                np.zeros(4, np.uint8))
    occ, sem = mem.occupancy.cpu().numpy(), mem.semantic.cpu().numpy()
    assert occ[1].sum() == 0 and sem[1].sum() == 0 and occ[3].sum() == 0 and sem[3].sum() == 0
    assert np.array_equal(occ, occ_r) and np.array_equal(sem, sem_r)
    assert occ[0].sum() > 100 and occ[2].sum() > 0


def test_known_mapper_eval_replayed_equals_eager(tmp_path, monkeypatch, same_depth_path):
    """`GTSemanticsKnownMapper` evaluation on the synthetic vector env, EVAL.USE_HIP_GRAPH on and off: the same actions and
    the same episode metrics.  Env i plays i + 1 episodes, so envs pause one after the other (eager map-before-pause step,
    capture again at the smaller batch); the replaying run must have built its runners."""
    import ivln_ce_amd  # noqa: F401
    from ivln_ce_amd import graphed, trainers
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.registry import baseline_registry

    same_depth_path(2)
    d = tmp_path / "data" / "known_maps" / "gt_semantics"
    d.mkdir(parents=True)
    rng = np.random.RandomState(11)
    for i in range(3):  # (_SynthEnv: env i is in "scene{i}" and starts near x = 3 i)
        xyz, sem = _scene(rng, 3000, centre=(3.0 * i, 0.0))
        np.savez(d / f"scene{i}.npz", xyz=xyz, semantics=sem)
    monkeypatch.chdir(tmp_path)

    actions_log = []
    real_envs = trainers.construct_envs

    def few_episodes(*a, **k):
        envs = real_envs(*a, **k)
        for i, e in enumerate(envs._envs):
            e.episodes = e.episodes[: i + 1]
        step = envs.step

        def logged(actions):
            actions_log.append(list(actions))
            return step(actions)

        envs.step = logged
        return envs

    monkeypatch.setattr(trainers, "construct_envs", few_episodes)
    built = []
    real_runner = graphed.GraphedRollout

    class Counted(real_runner):
        def __init__(self, policy, obs_transforms, example_obs, *a, **k):
            built.append(int(example_obs["depth"].shape[0]))
            super().__init__(policy, obs_transforms, example_obs, *a, **k)

    monkeypatch.setattr(graphed, "GraphedRollout", Counted)
    out, acts = {}, {}
    for mode in (True, False):
        torch.manual_seed(0)
        del actions_log[:]
        cfg = get_config(opts=[
            "TRAINER_NAME", "dagger", "NUM_ENVIRONMENTS", 3, "MODEL.policy_name", "MapCMAPolicy",
            "MODEL.INSTRUCTION_ENCODER.use_pretrained_embeddings", False, "MODEL.DEPTH_ENCODER.ddppo_checkpoint", "NONE",
            "RL.POLICY.OBS_TRANSFORMS.ENABLED_TRANSFORMS", ["GTSemanticsKnownMapper"],
            "TASK_CONFIG.ENVIRONMENT.MAX_EPISODE_STEPS", 12,
            "RESULTS_DIR", str(tmp_path / f"res{int(mode)}"), "EVAL_CKPT_PATH_DIR", str(tmp_path / "none.pth"),
            "EVAL.USE_HIP_GRAPH", mode, "EVAL.SAVE_RESULTS", False,
        ])
        tr = baseline_registry.get_trainer("dagger")(cfg)
        n_before = len(built)
        res = tr._eval_checkpoint(str(tmp_path / "none.pth"))
        res.pop("eval_seconds")
        out[mode], acts[mode] = res, [list(a) for a in actions_log]
        mm = tr.obs_transforms[0].mapping_module
        assert mm.known_library and len(mm.scene_library) == 3
        if mode:
            assert built[n_before:][0] == 3 and min(built[n_before:]) < 3, f"runners built at batch sizes {built[n_before:]}"
        else:
            assert len(built) == n_before
    assert acts[True] == acts[False] and len(acts[True]) > 10
    assert out[True] == out[False], f"graph {out[True]} vs eager {out[False]}"
    assert out[True]["episodes"] == 6


def test_known_mapper_dagger_collection_replayed_equals_eager(tmp_path, monkeypatch, same_depth_path):
    """DAgger collection with `GTSemanticsKnownMapper` (the reference's known_maps/{0_train_tf,1_ftune_dagger} configs): sampled
    steps replay as captured graphs (IL.DAGGER.USE_HIP_GRAPH) and every stored trajectory - maps, cached depth features,
    previous and expert actions - equals the eager collection's bit for bit, across the pauses of the beta == 1 pass."""
    import ivln_ce_amd  # noqa: F401
    from ivln_ce_amd import graphed, trainers
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.registry import baseline_registry

    same_depth_path(0)
    d = tmp_path / "data" / "known_maps" / "gt_semantics"
    d.mkdir(parents=True)
    rng = np.random.RandomState(12)
    for i in range(3):
        xyz, sem = _scene(rng, 3000, centre=(3.0 * i, 0.0))
        np.savez(d / f"scene{i}.npz", xyz=xyz, semantics=sem)
    monkeypatch.chdir(tmp_path)
    real_envs = trainers.construct_envs
    monkeypatch.setattr(trainers, "construct_envs", lambda *a, **k: real_envs(*a, n_episodes=2, episodes_per_tour=2, **k))
    built = []
    real_runner = graphed.GraphedRollout

    class Counted(real_runner):
        def __init__(self, *a, **k):
            built.append(1)
            super().__init__(*a, **k)

    monkeypatch.setattr(graphed, "GraphedRollout", Counted)
    stores = {}
    for mode in (True, False):
        cfg = get_config(opts=[
            "TRAINER_NAME", "dagger", "NUM_ENVIRONMENTS", 3, "MODEL.policy_name", "MapCMAPolicy",
            "MODEL.INSTRUCTION_ENCODER.use_pretrained_embeddings", False, "MODEL.DEPTH_ENCODER.ddppo_checkpoint", "NONE",
            "RL.POLICY.OBS_TRANSFORMS.ENABLED_TRANSFORMS", ["GTSemanticsKnownMapper"],
            "TASK_CONFIG.ENVIRONMENT.MAX_EPISODE_STEPS", 10,
            "IL.DAGGER.iterations", 1, "IL.DAGGER.update_size", 5, "IL.DAGGER.p", 1.0, "IL.DAGGER.USE_HIP_GRAPH", mode,
            "IL.DAGGER.lmdb_features_dir", str(tmp_path / f"traj{int(mode)}"), "CHECKPOINT_FOLDER", str(tmp_path / "ckpt"),
            "RESULTS_DIR", str(tmp_path / "res"), "EVAL_CKPT_PATH_DIR", str(tmp_path / "ckpt"),
        ])
        torch.manual_seed(0)
        tr = baseline_registry.get_trainer("dagger")(cfg)
        envs = trainers.construct_envs(cfg, None, iterative=False)
        observation_space, action_space = tr._get_spaces(cfg, envs=envs)
        envs.close()
        tr._initialize_policy(cfg, False, observation_space, action_space)
        torch.manual_seed(5)
        n_before = len(built)
        tr._update_dataset(0)
        assert len(tr.store) >= 5
        assert (len(built) > n_before) == mode
        stores[mode] = [tr.store.get(i) for i in range(len(tr.store))]
    assert len(stores[True]) == len(stores[False])
    for (oa, pa, ea), (ob, pb, eb) in zip(stores[True], stores[False]):
        assert sorted(oa) == sorted(ob)
        for k in oa:
            assert oa[k].dtype == ob[k].dtype and np.array_equal(oa[k], ob[k]), k
        assert np.array_equal(pa, pb) and np.array_equal(ea, eb)
    assert any(int(o["occupancy_map"].sum()) > 0 for o, _, _ in stores[True])
