"""CPU: host side of the known-map builder (include/ivln_map_build.h, mapping.save_known_scene,
KnownSceneLibrary.add_from_mapper, known_maps.build_known_maps): the file format and its round trip, the builder's
not_done / flush logic against a mapping module that records its calls, the library's bookkeeping with the C call replaced,
and the exported symbols of the new header."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the file format ------------------------------------------------------------------------------------------------------
def test_save_load_round_trip_and_dtypes(tmp_path):
    from ivln_ce_amd.mapping import load_known_scene, save_known_scene

    rng = np.random.RandomState(4)
    xyz = rng.uniform(-5, 5, (37, 3)).astype(np.float32)
    sem = rng.randint(0, 13, 37).astype(np.uint8)
    loc = tmp_path / "maps" / "gt_semantics"  # (created on demand)
    path = save_known_scene(str(loc), "sceneX", xyz, sem)
    assert path == str(loc / "sceneX.npz")
    with np.load(path) as f:
        assert sorted(f.files) == ["semantics", "xyz"]
        assert f["xyz"].dtype == np.float32 and f["xyz"].shape == (37, 3)
        assert f["semantics"].dtype == np.int64 and f["semantics"].shape == (37,)
        # what the reference's loader does with the arrays (SemanticPointcloud.from_npz_file, mapper.py:283-294):
        # torch.LongTensor(ndarray) takes int64 and nothing else, torch.FloatTensor float32
        assert torch.equal(torch.LongTensor(f["semantics"]).to(torch.uint8), torch.from_numpy(sem))
        assert torch.equal(torch.FloatTensor(f["xyz"]), torch.from_numpy(xyz))
    x2, s2 = load_known_scene(str(loc), "sceneX")
    assert x2.dtype == np.float32 and s2.dtype == np.uint8
    assert np.array_equal(x2.view(np.uint32), xyz.view(np.uint32)) and np.array_equal(s2, sem)
    # an empty scene keeps its shapes
    save_known_scene(str(loc), "empty", np.zeros((0, 3), np.float32), np.zeros((0,), np.uint8))
    x0, s0 = load_known_scene(str(loc), "empty")
    assert x0.shape == (0, 3) and x0.dtype == np.float32 and s0.shape == (0,) and s0.dtype == np.uint8
    with np.load(loc / "empty.npz") as f:
        assert f["xyz"].shape == (0, 3) and f["semantics"].shape == (0,) and f["semantics"].dtype == np.int64
    with pytest.raises(ValueError, match="sceneY"):
        save_known_scene(str(loc), "sceneY", xyz, sem[:5])


def test_reference_loader_reads_the_file(tmp_path):
    """The reference's own `SemanticPointcloud.from_npz_file`, imported through tests/golden/_ref_shim.py in a process of
    its own (the shim registers stand-in modules that must not leak into this one)."""
    if not os.path.isdir("/root/reference/ivlnce_baselines"):
        pytest.skip("reference tree not mounted (GPU box)")
    from ivln_ce_amd.mapping import save_known_scene

    rng = np.random.RandomState(5)
    xyz = rng.uniform(-5, 5, (21, 3)).astype(np.float32)
    sem = rng.randint(0, 13, 21).astype(np.uint8)
    save_known_scene(str(tmp_path), "s", xyz, sem)
    save_known_scene(str(tmp_path), "e", xyz[:0], sem[:0])
    np.savez(tmp_path / "want.npz", xyz=xyz, sem=sem)
    code = (
        "import sys, numpy as np, torch\n"
        f"sys.path.insert(0, {os.path.join(ROOT, 'tests', 'golden')!r})\n"
        "import _ref_shim\n"
        "_ref_shim.install()\n"
        "from ivlnce_baselines.common.mapping_module import mapper as M\n"
        f"d = {str(tmp_path)!r}\n"
        "want = np.load(d + '/want.npz')\n"
        "pc = M.SemanticPointcloud.from_npz_file(d + '/s.npz', torch.device('cpu'), batch_ndx=3)\n"
        "assert pc.xyz.dtype == torch.float32 and pc.semantics.dtype == torch.uint8\n"
        "assert np.array_equal(pc.xyz.numpy(), want['xyz']) and np.array_equal(pc.semantics.numpy(), want['sem'])\n"
        "assert pc.batch_indices.tolist() == [3] * 21\n"
        "e = M.SemanticPointcloud.from_npz_file(d + '/e.npz', torch.device('cpu'))\n"
        "assert e.xyz.shape[0] == 0 and e.semantics.shape[0] == 0\n"
        "print('reference loader ok')\n"
    )
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "reference loader ok" in r.stdout, r.stderr[-2000:]


# ---- build_known_maps ---------------------------------------------------------------------------------------------------
class _FakeModule:
    """Stands in for MappingModule: row b's "cloud" is the list of frame tags the row has accumulated since its last
    not_done == 0; every call is recorded."""

    def __init__(self):
        self.rows, self.calls = {}, []

    def step(self, obs):
        nd = obs["not_done_masks"]
        assert nd.dtype == torch.uint8 and tuple(nd.shape) == (len(obs["env_name"]), 1)
        B = nd.shape[0]
        for b in list(self.rows):
            if b >= B:
                del self.rows[b]  # a row that left the batch is cleared (mapper.py:315-318)
        for b in range(B):
            if int(nd[b, 0]) == 0:
                self.rows[b] = []
            self.rows[b].append(int(obs["depth"][b, 0, 0, 0]))
        self.calls.append(("step", nd.reshape(-1).tolist(), list(obs["env_name"])))

    def check_status(self):
        self.calls.append(("check_status",))
        return 0

    def env_counts(self):
        self.calls.append(("env_counts",))
        return np.array([len(self.rows.get(b, [])) for b in range(4)], np.int64)

    def export_scene(self, b):
        self.calls.append(("export_scene", b))
        tags = self.rows.get(b, [])
        return np.repeat(np.asarray(tags, np.float32)[:, None], 3, 1), np.asarray(tags, np.uint8)


class _FakeTransformer:
    def __init__(self):
        self.mapping_module = _FakeModule()

    def __call__(self, obs):
        self.mapping_module.step(obs)
        for k in ("env_name", "world_robot_pose"):  # as Mapper.delete_extra_information does
            obs.pop(k, None)
        return obs


class _FakeLibrary:
    def __init__(self):
        self.added = {}

    def add_from_mapper(self, name, mm, b):
        assert name not in self.added
        self.added[name] = int(mm.env_counts()[b])
        return len(self.added) - 1

    def points(self, name):
        return self.added[name]


def _batches(script):
    for t, names in enumerate(script):
        yield {"depth": torch.full((len(names), 2, 2, 1), float(t + 1)), "env_name": list(names),
               "world_robot_pose": torch.zeros(len(names), 3)}


def test_builder_not_done_flush_and_return(tmp_path):
    from ivln_ce_amd.known_maps import build_known_maps
    from ivln_ce_amd.mapping import load_known_scene

    # row 0: A for five frames (an "episode boundary" in between changes nothing), then D; row 1: B, B, then C; at
    # t = 5 the batch shrinks to one row (C is flushed before the step that drops it)
    script = [["A", "B"], ["A", "B"], ["A", "C"], ["A", "C"], ["A", "C"], ["D"], ["D"]]
    tr, lib = _FakeTransformer(), _FakeLibrary()
    out = build_known_maps(_batches(script), tr, out_dir=str(tmp_path), library=lib)
    mm = tr.mapping_module
    steps = [c for c in mm.calls if c[0] == "step"]
    assert [c[1] for c in steps] == [[0, 0], [1, 1], [1, 0], [1, 1], [1, 1], [0], [1]]
    assert [c[2] for c in steps] == script  # the caller's dicts keep their env_name: the transformer got a copy
    assert out == {"B": 2, "A": 5, "C": 3, "D": 2} and list(out) == ["B", "A", "C", "D"]  # in flush order
    assert lib.added == out
    assert sorted(os.listdir(tmp_path)) == ["A.npz", "B.npz", "C.npz", "D.npz"]
    for name, tags in [("A", [1, 2, 3, 4, 5]), ("B", [1, 2]), ("C", [3, 4, 5]), ("D", [6, 7])]:
        xyz, sem = load_known_scene(str(tmp_path), name)
        assert sem.tolist() == tags and xyz[:, 0].tolist() == [float(x) for x in tags]
    # every flush happens BEFORE the step that clears the row, and checks the device status first
    kinds = [c[0] if c[0] != "step" else f"step{i}" for i, c in enumerate(mm.calls)]
    first_c = next(i for i, c in enumerate(mm.calls) if c[0] == "step" and c[2] == ["A", "C"])
    assert mm.calls[first_c - 1][0] == "env_counts" and ("export_scene", 1) in mm.calls[:first_c], kinds
    assert mm.calls.count(("check_status",)) == 4

    # no sink: counts only
    tr2 = _FakeTransformer()
    assert build_known_maps(_batches([["A"], ["A"], ["B"]]), tr2) == {"A": 2, "B": 1}
    assert not any(c[0] == "export_scene" for c in tr2.mapping_module.calls)
    assert build_known_maps(_batches([]), _FakeTransformer()) == {}


@pytest.mark.parametrize("script,scene", [
    ([["A", "B"], ["C", "B"], ["A", "B"]], "A"),  # back after it was flushed
    ([["A", "A"]], "A"),                          # two rows at once
    ([["A", "B"], ["A", "A"]], "A"),              # a row moves into a scene another row is still in
    ([["A", "B"], ["B", "C"]], "B"),              # ... or was in until this very step
])
def test_builder_refuses_a_scene_seen_twice(tmp_path, script, scene):
    from ivln_ce_amd.known_maps import build_known_maps

    with pytest.raises(ValueError, match=f"'{scene}'"):
        build_known_maps(_batches(script), _FakeTransformer(), out_dir=str(tmp_path))
    # the first cloud of the scene, if it was written, is what the file still holds
    if scene == "A" and len(script) == 3:
        with np.load(tmp_path / "A.npz") as f:
            assert f["semantics"].tolist() == [1]


# ---- KnownSceneLibrary.add_from_mapper ------------------------------------------------------------------------------------
def test_add_from_mapper_bookkeeping(tmp_path):
    from ivln_ce_amd._lib import IvlnError
    from ivln_ce_amd.mapping import KnownSceneLibrary

    class Stub(KnownSceneLibrary):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.calls = []

        def _add(self, scene, xyz, sem, records):
            self.calls.append(("file", scene, tuple(records.shape)))

        def _add_from_mapper(self, scene, mapping_module, b, records):
            self.calls.append(("mapper", scene, b, tuple(records.shape), records.dtype))

    class Counts:
        def env_counts(self):
            return np.array([7, 0, 3], np.int64)

    np.savez(tmp_path / "f.npz", xyz=np.zeros((2, 3)), semantics=np.zeros(2, np.int64))
    lib = Stub(torch.device("cpu"), str(tmp_path), max_scenes=3)
    assert lib.add_from_mapper("a", Counts(), 0) == 0
    assert lib.index("f") == 1  # file scenes and promoted scenes share the index space
    assert lib.add_from_mapper("e", Counts(), 1) == 2
    assert lib.calls == [("mapper", 0, 0, (7, 4), torch.float32), ("file", 1, (2, 4)), ("mapper", 2, 1, (0, 4), torch.float32)]
    assert lib.names() == ["a", "f", "e"] and [lib.points(n) for n in lib.names()] == [7, 2, 0]
    assert lib.index("a") == 0 and len(lib.calls) == 3  # a promoted name is looked up, never read from a file
    with pytest.raises(IvlnError, match="already"):
        lib.add_from_mapper("a", Counts(), 2)
    with pytest.raises(IvlnError, match="already"):
        lib.add_from_mapper("f", Counts(), 2)
    with pytest.raises(IvlnError, match="full"):
        lib.add_from_mapper("z", Counts(), 2)
    assert len(lib) == 3 and len(lib.calls) == 3 and "z" not in lib


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_library_exports_every_entry_of_the_map_build_header():
    import __graft_entry__ as ge

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ivln_map_build.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ivln_[a-z0-9_]+)\s*\(", src)))
    assert names == ["ivln_known_lib_add_from_mapper", "ivln_mapper_env_counts", "ivln_mapper_env_export"]
    L = ctypes.CDLL(ge.build())
    assert all(hasattr(L, n) for n in names)
    lib_src = open(os.path.join(ROOT, "ivln-ce_amd", "_lib.py")).read()
    assert all(f"L.{n}.argtypes" in lib_src for n in names)
    # refusals that need no GPU: NULL handles, nothing is launched or allocated
    one = ctypes.c_void_p(16)
    n = ctypes.c_int64(-7)
    assert L.ivln_mapper_env_counts(None, 1, ctypes.byref(n), None) == -1
    assert L.ivln_mapper_env_export(None, 0, one, one, ctypes.c_int64(1), ctypes.byref(n), None) == -1
    assert L.ivln_known_lib_add_from_mapper(None, 0, None, 0, one, ctypes.c_int64(1), None) == -1
    assert n.value == -7
