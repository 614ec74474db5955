"""What leaving the mapper costs a cloud (include/ivln_map_build.h), at about 10^4, 10^5 and 10^6 points in one env:
  host_sorted      the yardstick of export: `MappingModule.world_cloud()` filtered to the env - three device-to-host copies
                   of the whole world and a numpy argsort
  export_scene     `MappingModule.export_scene(b)`: counts, ordered compaction on the device, one copy of the env's points
  via_files        the yardstick of promotion: export_scene -> save_known_scene -> KnownSceneLibrary.index (file read,
                   host-to-device copy, pack)
  add_from_mapper  `KnownSceneLibrary.add_from_mapper`: counts + ordered compaction straight into the library's records

    python tools/known_build_cost.py [--frames 1,12,118] [--rounds 5]

The cloud of env 0 is built once per size from `frames` 256 x 256 frames 12 m apart (~8 k kept cells each); env 1 holds one
frame, so the world is not a single env.  Host clock around each call ending in a synchronise, the settings alternating round
by round in one process after two warm-up rounds; median (min - max) in ms over `rounds`.  One JSON line per size."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SETTINGS = ("host_sorted", "export_scene", "via_files", "add_from_mapper")


def dense_frame(rng, H=256):
    """Every pixel inside the mapper's height window, depths spread over the frustum."""
    ys = (np.arange(H) + 0.5 - H / 2) / (H / 2)
    zmax = np.minimum(9.5, 0.45 / np.maximum(np.abs(ys), 1e-3))
    return np.clip(rng.uniform(0.3, 1.0, (H, H)) * zmax[:, None] / 10.0, 0.02, 0.98).astype(np.float32)


def explore(frames, dev):
    from ivln_ce_amd.mapping import CameraParameters, MapDimensions, create_gt_semantics_iterative_mapper

    H = 256
    side = int(np.ceil(np.sqrt(frames)))  # poses on a square lattice: the key space grows with the area, not its square
    cells = 3 * (side * 240 + 800) ** 2
    m = create_gt_semantics_iterative_mapper(dev, CameraParameters(float(np.deg2rad(90.0)), (H, H), 0.1),
                                             MapDimensions(6.4, 6.4, 0.1), b_max=2, world_capacity=frames * 12000 + 100000,
                                             table_cells=max(16 << 20, cells))
    rng = np.random.RandomState(3)
    for t in range(frames):
        depth = np.zeros((2, H, H, 1), np.float32)
        depth[0, :, :, 0] = dense_frame(rng)
        if t == 0:
            depth[1, :, :, 0] = dense_frame(rng)
        pose = np.array([[12.0 * (t % side), 1.25, 12.0 * (t // side)], [0.0, 1.25, 0.0]], np.float32)
        m({"depth": torch.from_numpy(depth).to(dev),
           "semantic12": torch.from_numpy(rng.randint(0, 13, (2, H, H, 1)).astype(np.uint8)).to(dev),
           "world_robot_pose": torch.from_numpy(pose).to(dev),
           "world_robot_orientation": torch.zeros(2, 2, dtype=torch.float64, device=dev),
           "not_done_masks": torch.full((2, 1), 0 if t == 0 else 1, dtype=torch.uint8, device=dev), "env_name": ["s", "s"]})
    m.check_status()
    return m


def _three(xs):
    return [round(statistics.median(xs), 3), round(min(xs), 3), round(max(xs), 3)]


def run(frames, rounds, dev):
    from ivln_ce_amd.mapping import KnownSceneLibrary, save_known_scene

    m = explore(frames, dev)
    n = int(m.env_counts()[0])
    times = {k: [] for k in SETTINGS}
    with tempfile.TemporaryDirectory() as tmp:
        def host_sorted():
            xyz, b, s = m.world_cloud()
            return xyz[b == 0], s[b == 0]

        def via_files(i):
            xyz, sem = m.export_scene(0)
            save_known_scene(tmp, f"f{i}", xyz, sem)
            KnownSceneLibrary(dev, tmp).index(f"f{i}")

        def add_from_mapper(i):
            KnownSceneLibrary(dev, None).add_from_mapper(f"p{i}", m, 0)

        calls = {"host_sorted": lambda i: host_sorted(), "export_scene": lambda i: m.export_scene(0), "via_files": via_files,
                 "add_from_mapper": add_from_mapper}
        a, b = host_sorted(), m.export_scene(0)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), "export_scene != host-sorted cloud"
        for rnd in range(2 + rounds):
            for k in SETTINGS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                calls[k](rnd)
                torch.cuda.synchronize()
                if rnd >= 2:
                    times[k].append((time.perf_counter() - t0) * 1e3)
    res = {"frames": frames, "env_points": n, "world_points": int(m.check_status()), "rounds": rounds}
    for k in SETTINGS:
        res[f"{k}_ms"] = _three(times[k])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="1,12,118")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("known_build_cost: needs the GPU (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    for frames in (int(f) for f in a.frames.split(",")):
        print(json.dumps(run(frames, a.rounds, dev)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
