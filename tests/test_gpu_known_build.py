"""GPU: the known-map builder (include/ivln_map_build.h; MappingModule.env_counts / export_scene,
KnownSceneLibrary.add_from_mapper, known_maps.build_known_maps).  Every comparison is bit-exact - this is integer and copy
work -: per-env clouds against the reference's own clouds (tests/golden/mapper_*.npz, known_build.npz) and against the
host-sorted `world_cloud()` at the edges of the scan, the mapper untouched by exports between its steps, promotion into a
scene library against the file paths and behind a captured step, the argument checks, and the builder loop."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
E_INVALID, E_CAPACITY, E_UNSUPPORTED = -1, -4, -5


def _mk(H, W, b_max=8, **kw):
    from ivln_ce_amd.mapping import CameraParameters, MapDimensions, create_gt_semantics_iterative_mapper

    cam = CameraParameters(float(np.deg2rad(90.0 * H / W)), (H, W), 0.1)
    return create_gt_semantics_iterative_mapper(torch.device(DEV), cam, MapDimensions(6.4, 6.4, 0.1), b_max=b_max, **kw)


def _obs(g, t):
    return {
        "depth": torch.from_numpy(g[f"depth_{t}"]).to(DEV),
        "semantic12": torch.from_numpy(g[f"semantic12_{t}"]).to(DEV),
        "world_robot_pose": torch.from_numpy(g[f"pose_{t}"]).to(DEV),
        "world_robot_orientation": torch.from_numpy(g[f"orientation_{t}"]).to(DEV),
        "not_done_masks": torch.from_numpy(g[f"not_done_{t}"]).to(DEV),
        "env_name": ["s"] * int(g["B"]),
    }


def _same(xyz, sem, xyz_ref, sem_ref, what):
    assert xyz.dtype == np.float32 and sem.dtype == np.uint8 and xyz.shape == (len(sem), 3), what
    assert xyz.shape == xyz_ref.shape, f"{what}: {xyz.shape[0]} points, expected {xyz_ref.shape[0]}"
    assert np.array_equal(np.ascontiguousarray(xyz).view(np.uint32), np.ascontiguousarray(xyz_ref).view(np.uint32)), what
    assert np.array_equal(sem, sem_ref), what


# ---- against the reference's clouds -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["planar_ties", "far_apart", "b2_64", "b4_32", "b1_256"])
def test_export_matches_reference_clouds(case):
    g = np.load(os.path.join(GOLDEN, f"mapper_{case}.npz"))
    B, steps = int(g["B"]), int(g["steps"])
    m = _mk(int(g["H"]), int(g["W"]))
    checked = 0
    for t in range(steps):
        m(_obs(g, t))
        m.check_status()
        if f"world_xyz_{t}" not in g:
            continue
        wb = g[f"world_b_{t}"]
        counts = m.env_counts()
        assert counts.dtype == np.int64 and counts.shape == (m.b_max,)
        assert np.array_equal(counts, np.bincount(wb, minlength=m.b_max)), f"counts step {t}"
        for b in range(B):
            xyz, sem = m.export_scene(b)
            _same(xyz, sem, g[f"world_xyz_{t}"][wb == b], g[f"world_sem_{t}"][wb == b], f"{case} step {t} env {b}")
        checked += 1
    assert checked >= 1


def test_exports_between_steps_leave_the_mapper_as_it_was():
    """mapper_b4_32 (with its reset steps), every env exported after every step: the maps and clouds of all later steps
    equal the golden as they do without the exports - the arg-max table the export borrows is all zero again."""
    g = np.load(os.path.join(GOLDEN, "mapper_b4_32.npz"))
    B, steps = int(g["B"]), int(g["steps"])
    m = _mk(int(g["H"]), int(g["W"]))
    for t in range(steps):
        mem = m(_obs(g, t))
        assert m.check_status() == int(g[f"world_n_{t}"]), f"world size step {t}"
        assert np.array_equal(mem.occupancy.cpu().numpy(), g[f"occ_{t}"]), f"occupancy step {t}"
        assert np.array_equal(mem.semantic.cpu().numpy(), g[f"sem_{t}"]), f"semantic step {t}"
        total = 0
        for b in range(B):
            total += len(m.export_scene(b)[1])
        assert total == int(g[f"world_n_{t}"])
        if f"world_xyz_{t}" in g:
            xyz, wb, s = m.world_cloud()
            assert np.array_equal(xyz.view(np.uint32), g[f"world_xyz_{t}"].view(np.uint32))
            assert np.array_equal(wb, g[f"world_b_{t}"]) and np.array_equal(s, g[f"world_sem_{t}"])


# ---- against the host-sorted path at the scan's edges ---------------------------------------------------------------------
def _grid_frame(H, k):
    """k valid pixels that each keep their own 5 cm cell: 16 image rows around the horizon (inside the height window at
    2 - 3 m), one depth per row 6 cm apart, 64 columns >= 6.25 cm apart at 2 m."""
    s = H // 64
    d = np.zeros((H, H), np.float32)
    n = 0
    for i in range(16):
        for j in range(64):
            if n < k:
                d[24 * s + s * i, s * j] = 0.2 + 0.006 * i
                n += 1
    return d


def _dense_frame(rng, H):
    """Every pixel inside the height window, depths spread over the frustum: ~8.5 k kept cells per 256 x 256 frame."""
    ys = (np.arange(H) + 0.5 - H / 2) / (H / 2)
    zmax = np.minimum(9.5, 0.45 / np.maximum(np.abs(ys), 1e-3))
    z = rng.uniform(0.3, 1.0, (H, H)) * zmax[:, None]
    return np.clip(z / 10.0, 0.02, 0.98).astype(np.float32)


# (H, frames of env 0, points of env 2) - env 1 never sees a valid pixel: an empty env between two non-empty ones
EDGE_CASES = {
    "1_0_255": (64, [("grid", 1)], 255),
    "256_0_257": (64, [("grid", 256)], 257),
    "big_0_256": (256, [("dense", None)] * 9, 256),
}


def _edge_mapper(name):
    H, frames0, k2 = EDGE_CASES[name]
    rng = np.random.RandomState(7)
    lab = np.random.RandomState(1)
    m = _mk(H, H, b_max=3)
    for t, (kind, k) in enumerate(frames0):
        depth = np.zeros((3, H, H, 1), np.float32)
        depth[0, :, :, 0] = _grid_frame(H, k) if kind == "grid" else _dense_frame(rng, H)
        if t == 0:
            depth[2, :, :, 0] = _grid_frame(H, k2)
        # env 0 looks along +z from z = 8 (it holds the LAST cell row of the world's bounding box: its keys run into the
        # key range of env 1, quirk Q2), env 2 along -z from z = -8 (the first row); env 0 moves 12 m per frame
        pose = np.array([[12.0 * t, 1.25, 8.0], [0.0, 1.25, 0.0], [3.0, 1.25, -8.0]], np.float32)
        orient = np.zeros((3, 2), np.float64)
        orient[0, 1] = np.pi
        m({"depth": torch.from_numpy(depth).to(DEV),
           "semantic12": torch.from_numpy(lab.randint(0, 13, (3, H, H, 1)).astype(np.uint8)).to(DEV),
           "world_robot_pose": torch.from_numpy(pose).to(DEV), "world_robot_orientation": torch.from_numpy(orient).to(DEV),
           "not_done_masks": torch.full((3, 1), 0 if t == 0 else 1, dtype=torch.uint8, device=DEV), "env_name": ["s"] * 3})
    m.check_status()
    return m


def _raw_export(m, b, n_alloc, max_n, pad=64):
    """ivln_mapper_env_export into buffers pre-filled with NaN / 0xFF, `pad` rows of sentinel band on either side."""
    from ivln_ce_amd._lib import lib, stream_ptr

    xyz = torch.full((n_alloc + 2 * pad, 3), float("nan"), dtype=torch.float32, device=DEV)
    sem = torch.full((n_alloc + 2 * pad,), 0xFF, dtype=torch.uint8, device=DEV)
    n_out = C.c_int64(-1)
    rc = lib().ivln_mapper_env_export(m._h, b, xyz.data_ptr() + 12 * pad, sem.data_ptr() + pad, max_n, C.byref(n_out),
                                      stream_ptr())
    torch.cuda.synchronize()
    return rc, n_out.value, xyz.cpu().numpy().view(np.uint32), sem.cpu().numpy()


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_export_at_the_scan_edges_matches_host_sorted_cloud(name):
    pad = 64
    nan_bits = np.float32("nan").view(np.uint32)
    m = _edge_mapper(name)
    wx, wb, ws = m.world_cloud()
    counts = np.bincount(wb, minlength=3)
    n0, _, n2 = name.split("_")
    if n0 == "big":  # several workgroups and two levels of tile sums above the marks (tiles of 256: > 65536 marks)
        assert counts[0] > 70000 and counts[1] == 0 and counts[2] == int(n2), counts
    else:
        assert counts.tolist() == [int(n0), 0, int(n2)], counts
    r = np.rint(wx[:, 2] / np.float32(0.05))
    assert r[wb == 0].max() == r.max() and r[wb == 2].min() == r.min()  # env 0 holds the last cell row, env 2 the first
    assert np.array_equal(m.env_counts(), counts)
    for b in range(3):
        n = int(counts[b])
        want_xyz, want_sem = wx[wb == b], ws[wb == b]
        xyz, sem = m.export_scene(b)
        _same(xyz, sem, want_xyz, want_sem, f"{name} env {b}")
        runs = [_raw_export(m, b, n, n, pad) for _ in range(2)]
        for rc, n_out, rx, rs in runs:
            assert rc == 0 and n_out == n
            assert np.array_equal(rx[pad:pad + n], np.ascontiguousarray(want_xyz).view(np.uint32).reshape(n, 3))
            assert np.array_equal(rs[pad:pad + n], want_sem)
            assert (rx[:pad] == nan_bits).all() and (rx[pad + n:] == nan_bits).all(), "xyz written outside [0, n)"
            assert (rs[:pad] == 0xFF).all() and (rs[pad + n:] == 0xFF).all(), "semantics written outside [0, n)"
        assert runs[0][2].tobytes() == runs[1][2].tobytes() and runs[0][3].tobytes() == runs[1][3].tobytes()
        if n > 0:  # one row short: refused, the needed count reported, nothing written
            rc, n_out, rx, rs = _raw_export(m, b, n, n - 1, pad)
            assert rc == E_CAPACITY and n_out == n
            assert (rx == nan_bits).all() and (rs == 0xFF).all()
    # the world is what it was: the host-sorted path returns the same cloud after all those exports
    wx2, wb2, ws2 = m.world_cloud()
    assert wx2.tobytes() == wx.tobytes() and np.array_equal(wb2, wb) and np.array_equal(ws2, ws)


# ---- promotion --------------------------------------------------------------------------------------------------------------
def _explore_two_rows(steps=4):
    from ivln_ce_amd.synthetic import SyntheticRollout

    m = _mk(64, 64, b_max=2)
    roll = SyntheticRollout(B=2, H=64, W=64, seed=21)
    for _ in range(steps):
        m({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in roll.step().items()})
    m.check_status()
    return m


def _known_obs(pose, orient, nd, names):
    B = len(names)
    return {"depth": torch.zeros(B, 16, 16, 1, device=DEV), "world_robot_pose": torch.from_numpy(pose).to(DEV),
            "world_robot_orientation": torch.from_numpy(orient).to(DEV),
            "not_done_masks": torch.from_numpy(np.asarray(nd, np.uint8).reshape(-1, 1)).to(DEV), "env_name": list(names)}


def _known_pose(t):
    pose = np.array([[0.2 * t, 1.25, -0.3 * t], [-0.4, 1.3, 0.25 * t - 1.0]], np.float32)
    orient = np.array([[0.0, 0.4 * t], [0.0, 3.0 - 0.7 * t]], np.float64)
    return pose, orient


KNOWN_SCRIPT = [([0, 0], ["p0", "p1"]), ([1, 1], ["p0", "p1"]), ([1, 0], ["p0", "p0"]), ([0, 1], ["p1", "p0"]),
                ([1, 1], ["p1", "p0"])]


def test_promoted_scenes_equal_the_file_paths(tmp_path, monkeypatch):
    from ivln_ce_amd import obs_transforms  # noqa: F401
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.mapping import KnownSceneLibrary, save_known_scene
    from ivln_ce_amd.registry import baseline_registry

    m = _explore_two_rows()
    counts = m.env_counts()
    assert counts[0] > 500 and counts[1] > 500
    library = KnownSceneLibrary(torch.device(DEV), None)
    assert library.add_from_mapper("p0", m, 0) == 0 and library.add_from_mapper("p1", m, 1) == 1
    assert library.points("p0") == counts[0] and library.points("p1") == counts[1]
    d = tmp_path / "data" / "known_maps" / "gt_semantics"
    for b, name in enumerate(["p0", "p1"]):
        save_known_scene(str(d), name, *m.export_scene(b))
    monkeypatch.chdir(tmp_path)  # (the plugins read data/known_maps/gt_semantics relative to the working directory)
    cls = baseline_registry.get_obs_transformer("GTSemanticsKnownMapper")
    promoted = cls.from_config(get_config())
    promoted.sizing.update(b_max=2, scene_library=library)
    files = cls.from_config(get_config())
    files.sizing.update(b_max=2)
    copy = cls.from_config(get_config(opts=["RL.POLICY.OBS_TRANSFORMS.EGOCENTRIC_MAPPER.known_library", False]))
    copy.sizing.update(b_max=2)
    seen = 0
    for t, (nd, names) in enumerate(KNOWN_SCRIPT):
        pose, orient = _known_pose(t)
        outs = [tr(_known_obs(pose, orient, nd, names)) for tr in (promoted, files, copy)]
        for tr in (promoted, files, copy):
            tr.mapping_module.check_status()
        for key in ("occupancy_map", "semantic_map"):
            a, b, c = (o[key].cpu().numpy() for o in outs)
            assert a.tobytes() == b.tobytes(), f"{key} step {t}: promoted library vs library fed the files"
            assert a.tobytes() == c.tobytes(), f"{key} step {t}: promoted library vs copy path"
        seen += int(outs[0]["occupancy_map"].sum())
    assert promoted.mapping_module.scene_library is library and promoted.mapping_module.known_library
    assert files.mapping_module.known_library and not copy.mapping_module.known_library
    assert len(library) == 2  # the promoted names were looked up, nothing was read from a file into this library
    assert seen > 200


def test_step_captured_before_a_promotion_sees_the_scene_on_replay(tmp_path):
    from ivln_ce_amd.mapping import KnownSceneLibrary, MapDimensions, MappingModule, save_known_scene

    explorer = _explore_two_rows()
    library = KnownSceneLibrary(torch.device(DEV), None)
    library.add_from_mapper("p0", explorer, 0)
    for b, name in enumerate(["p0", "p1"]):
        save_known_scene(str(tmp_path), name, *explorer.export_scene(b))
    dims = MapDimensions(6.4, 6.4, 0.1)
    m = MappingModule(torch.device(DEV), None, dims, mode="known", b_max=2, known_library=True, scene_library=library)
    eager = MappingModule(torch.device(DEV), None, dims, mode="known", maps_location=str(tmp_path), b_max=2,
                          known_library=True)
    pose, orient = _known_pose(0)
    static = _known_obs(pose, orient, [0, 0], ["p0", "p0"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up: the handle exists before the capture
        m(static)
    torch.cuda.current_stream().wait_stream(side)
    m.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mem = m(static)
    script = [([0, 0], ["p0", "p0"]), ([1, 1], ["p0", "p0"]), ([1, 0], ["p0", "p1"]), ([0, 1], ["p1", "p1"])]
    for t, (nd, names) in enumerate(script):
        if t == 2:
            assert "p1" not in library
            library.add_from_mapper("p1", explorer, 1)  # after the capture, between two replays
        pose, orient = _known_pose(t)
        obs = _known_obs(pose, orient, nd, names)
        for k in ("world_robot_pose", "world_robot_orientation", "not_done_masks"):
            static[k].copy_(obs[k])
        m.stage_host({"env_name": names})
        graph.replay()
        ref = eager(obs)
        assert torch.equal(mem.occupancy, ref.occupancy), f"occupancy step {t}"
        assert torch.equal(mem.semantic, ref.semantic), f"semantic step {t}"
        assert m.check_status() == eager.check_status()
        if t == 2:
            assert int(mem.occupancy[1].sum()) > 20
    assert len(library) == 2


# ---- argument checks ------------------------------------------------------------------------------------------------------
def test_argument_checks(tmp_path):
    from ivln_ce_amd._lib import IvlnError, lib, stream_ptr
    from ivln_ce_amd.mapping import KnownSceneLibrary, MapDimensions, MappingModule, save_known_scene

    L = lib()
    m = _explore_two_rows(steps=2)
    h, s = m._h, stream_ptr()
    n0 = int(m.env_counts()[0])
    assert n0 > 100
    nan_bits = np.float32("nan").view(np.uint32)
    xyz = torch.full((n0 + 8, 3), float("nan"), device=DEV)
    sem = torch.full((n0 + 8,), 0xFF, dtype=torch.uint8, device=DEV)
    cnt = (C.c_int64 * 2)(-7, -7)
    n_out = C.c_int64(-7)
    # ivln_mapper_env_counts
    assert L.ivln_mapper_env_counts(None, 2, cnt, s) == E_INVALID
    assert L.ivln_mapper_env_counts(h, 2, None, s) == E_INVALID
    assert L.ivln_mapper_env_counts(h, 0, cnt, s) == E_INVALID and L.ivln_mapper_env_counts(h, 3, cnt, s) == E_INVALID
    assert list(cnt) == [-7, -7]
    # ivln_mapper_env_export
    exp = lambda hh=h, b=0, x=xyz.data_ptr(), l=sem.data_ptr(), mx=n0, out=C.byref(n_out): L.ivln_mapper_env_export(  # noqa: E731
        hh, b, x, l, mx, out, s)
    assert exp(hh=None) == E_INVALID and exp(out=None) == E_INVALID
    assert exp(b=-1) == E_INVALID and exp(b=2) == E_INVALID  # b_max = 2
    assert exp(mx=-1) == E_INVALID
    assert exp(x=None) == E_INVALID and exp(l=None) == E_INVALID
    assert n_out.value == -7
    assert exp(mx=n0 - 1) == E_CAPACITY and n_out.value == n0
    torch.cuda.synchronize()
    assert (xyz.cpu().numpy().view(np.uint32) == nan_bits).all() and (sem.cpu().numpy() == 0xFF).all()
    assert exp() == 0 and n_out.value == n0
    # ivln_known_lib_add_from_mapper
    klib = KnownSceneLibrary(torch.device(DEV), None, max_scenes=4)
    kh = klib.handle()
    rec = torch.full((n0 + 1, 4), float("nan"), device=DEV)
    add = lambda kk=kh, scene=0, hh=h, b=0, r=rec.data_ptr(), mx=n0: L.ivln_known_lib_add_from_mapper(  # noqa: E731
        kk, scene, hh, b, r, mx, s)
    assert add(kk=None) == E_INVALID and add(hh=None) == E_INVALID
    assert add(scene=-1) == E_INVALID and add(scene=4) == E_INVALID
    assert add(b=-1) == E_INVALID and add(b=2) == E_INVALID
    assert add(mx=-1) == E_INVALID
    assert add(r=None) == E_INVALID and add(r=rec.data_ptr() + 4) == E_INVALID  # records off a 16-byte boundary
    assert add(mx=n0 - 1) == E_CAPACITY
    torch.cuda.synchronize()
    assert L.ivln_known_lib_size(kh) == 0 and (rec.cpu().numpy().view(np.uint32) == nan_bits).all()
    assert add() == 0 and L.ivln_known_lib_size(kh) == 1
    assert add() == E_INVALID  # an entry a captured step may be reading is not rewritten (as ivln_known_lib_add)
    torch.cuda.synchronize()
    got = rec.cpu().numpy()
    want_xyz, want_sem = m.export_scene(0)
    assert np.array_equal(got[:n0, :3].view(np.uint32), want_xyz.view(np.uint32))
    assert np.array_equal(np.ascontiguousarray(got[:n0, 3]).view(np.uint32), want_sem.astype(np.uint32))
    assert (got[n0:].view(np.uint32) == nan_bits).all()

    # a cloud loaded by ivln_mapper_load_known: its ranks are a host counter, not keys
    save_known_scene(str(tmp_path), "s", want_xyz, want_sem)
    known = MappingModule(torch.device(DEV), None, MapDimensions(6.4, 6.4, 0.1), mode="known", maps_location=str(tmp_path),
                          b_max=2)
    pose, orient = _known_pose(0)
    known(_known_obs(pose, orient, [0, 0], ["s", "s"]))
    assert known.check_status() == 2 * n0
    n_out.value = -7
    assert exp(hh=known._h) == E_UNSUPPORTED and n_out.value == -7
    assert add(scene=1, hh=known._h) == E_UNSUPPORTED and L.ivln_known_lib_size(kh) == 1
    with pytest.raises(IvlnError, match="iterative"):
        known.export_scene(0)
    with pytest.raises(IvlnError, match="iterative"):
        known.env_counts()

    # between `begin` and `finish` the cloud is not defined
    from ivln_ce_amd.synthetic import SyntheticRollout

    obs = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in SyntheticRollout(B=2, H=64, W=64, seed=22).step().items()}
    obs["not_done_masks"] = torch.ones(2, 1, dtype=torch.uint8, device=DEV)
    m.begin(obs)
    with pytest.raises(IvlnError, match="begin"):
        m.export_scene(0)
    with pytest.raises(IvlnError, match="begin"):
        klib.add_from_mapper("x", m, 0)
    assert "x" not in klib
    m.finish(obs)
    assert m.check_status() > 0 and len(m.export_scene(0)[1]) == m.env_counts()[0]
    with pytest.raises(IvlnError, match="row"):
        m.export_scene(2)
    with pytest.raises(IvlnError, match="no step"):
        _mk(64, 64, b_max=2).export_scene(0)


# ---- the builder ------------------------------------------------------------------------------------------------------------
def _gt_transformer(H, b_max=2):
    from ivln_ce_amd.mapping import CameraParameters, MapDimensions
    from ivln_ce_amd.obs_transforms import GTSemanticsIterativeMapper

    tr = GTSemanticsIterativeMapper(camera_parameters=CameraParameters(float(np.deg2rad(90.0)), (H, H), 0.1),
                                    map_dimensions=MapDimensions(6.4, 6.4, 0.1))
    tr.sizing = {"b_max": b_max}
    return tr


def test_builder_files_equal_a_hand_driven_mapper(tmp_path):
    from ivln_ce_amd.known_maps import build_known_maps
    from ivln_ce_amd.mapping import KnownSceneLibrary, load_known_scene
    from ivln_ce_amd.synthetic import SyntheticRollout

    # 12 batches, B = 2: row 0 stays in sA - across an "episode boundary" at t = 5, where the stream's own not_done is 0 -,
    # row 1 moves from sB to sC at t = 6
    roll = SyntheticRollout(B=2, H=64, W=64, seed=31)
    batches = []
    for t in range(12):
        o = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in roll.step().items()}
        o["env_name"] = ["sA", "sB" if t < 6 else "sC"]
        o["not_done_masks"] = torch.tensor([[0 if t in (0, 5) else 1], [0 if t == 0 else 1]], dtype=torch.uint8, device=DEV)
        batches.append(o)
    library = KnownSceneLibrary(torch.device(DEV), None)
    out = build_known_maps(iter(batches), _gt_transformer(64), out_dir=str(tmp_path), library=library)
    assert all("env_name" in o and int(o["not_done_masks"][0, 0]) == (0 if t in (0, 5) else 1) for t, o in enumerate(batches))
    assert sorted(os.listdir(tmp_path)) == ["sA.npz", "sB.npz", "sC.npz"] and list(out) == ["sB", "sA", "sC"]

    hand = _gt_transformer(64)
    want = {}
    for t, o in enumerate(batches):
        if t == 6:
            want["sB"] = hand.mapping_module.export_scene(1)  # before the step that clears the row
        o = dict(o)
        o["not_done_masks"] = torch.tensor([[0 if t == 0 else 1], [0 if t in (0, 6) else 1]], dtype=torch.uint8, device=DEV)
        hand(o)
    want["sA"], want["sC"] = hand.mapping_module.export_scene(0), hand.mapping_module.export_scene(1)
    hand.mapping_module.check_status()
    assert len(want["sA"][1]) > len(want["sC"][1]) > 500  # sA kept accumulating over the boundary
    for name, (xyz, sem) in want.items():
        fx, fs = load_known_scene(str(tmp_path), name)
        _same(fx, fs, xyz, sem, f"file of {name}")
        assert out[name] == len(sem) == library.points(name)
    assert library.names() == ["sB", "sA", "sC"]


def test_builder_with_predicted_semantics(tmp_path):
    sys.path.insert(0, GOLDEN)
    from det_init import det_fill

    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.known_maps import build_known_maps
    from ivln_ce_amd.mapping import load_known_scene
    from ivln_ce_amd.obs_transforms import PredictedSemanticsIterativeMapper
    from ivln_ce_amd.synthetic import SyntheticRollout

    roll = SyntheticRollout(B=2, seed=33, with_rgb=True)
    batches = []
    for t in range(2):
        o = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in roll.step().items()}
        o.pop("semantic12")
        o.pop("not_done_masks")
        o["env_name"] = ["rA", "rB"]
        batches.append(o)
    tr = PredictedSemanticsIterativeMapper.from_config(get_config())
    tr.sizing["b_max"] = 2
    tr.setup_mapping_module(batches[0])
    ps = tr.mapping_module.semantics_module  # deterministic RedNet weights (no checkpoint travels with the tests)
    ps.setup()
    det_fill(ps.model, seed=1, conv_gain=0.6)
    ps.model.invalidate_folded()
    out = build_known_maps(batches, tr, out_dir=str(tmp_path))
    counts = tr.mapping_module.env_counts()
    assert sorted(os.listdir(tmp_path)) == ["rA.npz", "rB.npz"]
    for b, name in enumerate(["rA", "rB"]):
        xyz, sem = load_known_scene(str(tmp_path), name)
        assert out[name] == len(sem) == counts[b] > 1000 and xyz.shape == (len(sem), 3)


# ---- the reference did every step: tests/golden/known_build.npz -----------------------------------------------------------
def test_builder_and_known_mapper_against_the_reference(tmp_path):
    from ivln_ce_amd.known_maps import build_known_maps
    from ivln_ce_amd.mapping import MapDimensions, MappingModule

    g = np.load(os.path.join(GOLDEN, "known_build.npz"))
    H = int(g["H"])
    batches = []
    for t in range(int(g["steps"])):
        o = _obs(g, t)
        del o["not_done_masks"]
        o["env_name"] = [str(x) for x in g[f"env_names_{t}"]]
        batches.append(o)
    out = build_known_maps(batches, _gt_transformer(H), out_dir=str(tmp_path))
    assert sorted(out) == ["gA", "gB", "gC"]
    for name in out:
        with np.load(tmp_path / f"{name}.npz") as f:  # array-identical to what the reference wrote with np.savez
            assert f["xyz"].dtype == g[f"scene_{name}_xyz"].dtype and f["semantics"].dtype == g[f"scene_{name}_semantics"].dtype
            assert np.array_equal(f["xyz"].view(np.uint32), g[f"scene_{name}_xyz"].view(np.uint32)), name
            assert np.array_equal(f["semantics"], g[f"scene_{name}_semantics"]), name
        assert out[name] == len(g[f"scene_{name}_semantics"]) > 100
    m = MappingModule(torch.device(DEV), None, MapDimensions(6.4, 6.4, 0.1), mode="known", maps_location=str(tmp_path),
                      b_max=2, known_library=True)
    for t in range(int(g["known_steps"])):
        mem = m(_known_obs(g[f"kpose_{t}"], g[f"korientation_{t}"], g[f"knot_done_{t}"],
                           [str(x) for x in g[f"kenv_names_{t}"]]))
        m.check_status()
        assert np.array_equal(mem.occupancy.cpu().numpy(), g[f"kocc_{t}"]), f"occupancy step {t}"
        assert np.array_equal(mem.semantic.cpu().numpy(), g[f"ksem_{t}"]), f"semantic step {t}"
        assert int(g[f"kocc_{t}"].sum()) > 50
