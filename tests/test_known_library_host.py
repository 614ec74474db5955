"""CPU: host side of the known-map scene library (include/ivln_known_lib.h, mapping.KnownSceneLibrary): the library exports
every entry point the header declares, the name -> index bookkeeping (exercised with a stub in place of the C call), the
config key and what the trainer's eligibility rule reads."""
import ctypes
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_entry_of_the_known_library_header():
    import __graft_entry__ as ge

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ivln_known_lib.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ivln_[a-z0-9_]+)\s*\(", src)))
    assert names == ["ivln_known_lib_add", "ivln_known_lib_create", "ivln_known_lib_destroy", "ivln_known_lib_size",
                     "ivln_mapper_known_attach", "ivln_mapper_known_count", "ivln_mapper_known_step"]
    L = ctypes.CDLL(ge.build())
    assert all(hasattr(L, n) for n in names)
    lib_src = open(os.path.join(ROOT, "ivln-ce_amd", "_lib.py")).read()
    assert all(f"L.{n}.argtypes" in lib_src for n in names)
    # refusals that need no GPU: NULL handles, nothing is launched or allocated
    one = ctypes.c_void_p(16)
    out = ctypes.c_void_p()
    assert L.ivln_known_lib_create(0, ctypes.byref(out)) == -1
    assert L.ivln_known_lib_create(4, None) == -1
    assert L.ivln_known_lib_add(None, 0, one, one, ctypes.c_int64(1), one, None) == -1
    assert L.ivln_known_lib_size(None) == -1
    assert L.ivln_mapper_known_attach(None, None) == -1
    assert L.ivln_mapper_known_step(None, one, one, one, one, 1, one, one, None) == -1
    n = ctypes.c_int64()
    assert L.ivln_mapper_known_count(None, 1, ctypes.byref(n), None) == -1
    assert L.ivln_known_lib_destroy(None) == 0


class _StubLibrary:
    """KnownSceneLibrary with the C call replaced: records what would have been added."""

    def __new__(cls, maps_location, max_scenes=1024):
        from ivln_ce_amd.mapping import KnownSceneLibrary

        class Stub(KnownSceneLibrary):
            def __init__(self, *a, **k):
                super().__init__(*a, **k)
                self.added = []

            def _add(self, scene, xyz, sem, records):
                self.added.append((scene, xyz.clone(), sem.clone(), tuple(records.shape), records.dtype))

        return Stub(torch.device("cpu"), str(maps_location), max_scenes=max_scenes)


def test_known_scene_library_bookkeeping(tmp_path):
    import pytest

    from ivln_ce_amd._lib import IvlnError

    rng = np.random.RandomState(3)
    files = {}
    for name, n in [("a", 5), ("b", 0), ("c", 3)]:
        xyz = rng.uniform(-1, 1, (n, 3))  # float64 on disk: the loader converts as MappingModule._load_known does
        sem = rng.randint(0, 300, n).astype(np.int64)  # (labels wrap to uint8 the way the copy path's do)
        np.savez(tmp_path / f"{name}.npz", xyz=xyz, semantics=sem)
        files[name] = (xyz.astype(np.float32), sem.astype(np.uint8))
    lib = _StubLibrary(tmp_path, max_scenes=3)
    assert len(lib) == 0 and "a" not in lib
    assert [lib.index(x) for x in ["b", "a", "b", "a", "b"]] == [0, 1, 0, 1, 0]  # first sight decides, lookups load nothing
    assert len(lib.added) == 2 and [x[0] for x in lib.added] == [0, 1]
    assert lib.names() == ["b", "a"] and lib.points("a") == 5 and lib.points("b") == 0
    scene, xyz, sem, rshape, rdtype = lib.added[1]
    assert xyz.dtype == torch.float32 and sem.dtype == torch.uint8 and xyz.is_contiguous()
    assert np.array_equal(xyz.numpy(), files["a"][0]) and np.array_equal(sem.numpy(), files["a"][1])
    assert rshape == (5, 4) and rdtype == torch.float32  # 16-byte records
    assert lib.added[0][3] == (0, 4)
    assert lib.index("c") == 2 and "c" in lib
    np.savez(tmp_path / "d.npz", xyz=np.zeros((1, 3)), semantics=np.zeros(1, np.int64))
    with pytest.raises(IvlnError, match="full"):
        lib.index("d")
    assert "d" not in lib and len(lib) == 3
    with pytest.raises(FileNotFoundError):
        _StubLibrary(tmp_path).index("missing")


def test_copy_path_loader_and_library_loader_convert_alike(tmp_path):
    from ivln_ce_amd.mapping import load_known_scene

    np.savez(tmp_path / "s.npz", xyz=np.arange(12, dtype=np.float64).reshape(4, 3) / 7, semantics=np.array([0, 255, 256, 12]))
    xyz, sem = load_known_scene(str(tmp_path), "s")
    assert xyz.dtype == np.float32 and xyz.shape == (4, 3) and xyz.flags.c_contiguous
    assert sem.dtype == np.uint8 and sem.tolist() == [0, 255, 0, 12]


def test_config_key_and_plugin_flag():
    from ivln_ce_amd import obs_transforms  # noqa: F401 (registers the plugins)
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.registry import baseline_registry

    cfg = get_config()
    assert cfg.RL.POLICY.OBS_TRANSFORMS.EGOCENTRIC_MAPPER.known_library is True
    for name in ["GTSemanticsKnownMapper", "PredictedSemanticsKnownMapper"]:
        cls = baseline_registry.get_obs_transformer(name)
        tr = cls.from_config(cfg)
        assert tr.known_library is True and hasattr(tr, "stage_host")
        off = cls.from_config(get_config(opts=["RL.POLICY.OBS_TRANSFORMS.EGOCENTRIC_MAPPER.known_library", False]))
        assert off.known_library is False
    it = baseline_registry.get_obs_transformer("GTSemanticsIterativeMapper").from_config(cfg)
    assert not hasattr(it, "stage_host")  # (the runner stages only what asks for it)


def test_graph_eligibility_of_known_mappers():
    """trainers._graph_eligible reads the transformers' class names and `known_library`; the rule is called on a stand-in
    for the trainer that carries the attributes it reads (a trainer of its own would need the GPU)."""
    import inspect

    from ivln_ce_amd import obs_transforms, trainers  # noqa: F401
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.registry import baseline_registry

    src = inspect.getsource(trainers.BaseVLNCETrainer._graph_eligible)
    assert "known_library" in src and "KnownMapper" in src

    class T:  # the attributes the rule reads
        def __init__(self, transforms, cfg):
            self.obs_transforms, self.config, self.device = transforms, cfg, torch.device("cuda", 0)

    cls = baseline_registry.get_obs_transformer("GTSemanticsKnownMapper")
    cfg = get_config(opts=["MODEL.policy_name", "MapCMAPolicy"])
    on = cls.from_config(cfg)
    off = cls.from_config(get_config(opts=["RL.POLICY.OBS_TRANSFORMS.EGOCENTRIC_MAPPER.known_library", False]))
    elig = trainers.BaseVLNCETrainer._graph_eligible
    assert elig(T([on], cfg)) is True
    assert elig(T([off], cfg)) is False
    assert elig(T([on, off], cfg)) is False
