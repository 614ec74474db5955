"""What seeding a row of an iterative mapper costs (include/ivln_map_seed.h), at 10^4, 10^5 and 10^6 points:
  load_known  the yardstick: the copy path's `ivln_mapper_load_known` of the same arrays into a known-mode handle (one
              launch + a one-thread commit, ranks from a host counter, no boxes, no capacity read-back)
  seed_row    `MappingModule.seed_row(0, xyz, sem)` with the arrays on the device already: the read-back of the count, the
              box partials, the append with its per-workgroup slot claims and the row's exact cell box

    python tools/map_seed_cost.py [--points 10000,100000,1000000] [--rounds 5]

Host clock around each call ending in a synchronise; the two alternate round by round in one process after two warm-up
rounds, each on a handle that was reset outside the clock; median (min - max) in ms over `rounds`.  No kernel is timed
alone.  One JSON line per size."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SETTINGS = ("load_known", "seed_row")


def _three(xs):
    return [round(statistics.median(xs), 3), round(min(xs), 3), round(max(xs), 3)]


def run(n, rounds, dev):
    from ivln_ce_amd._lib import check, lib, stream_ptr
    from ivln_ce_amd.mapping import CameraParameters, MapDimensions, MappingModule, create_gt_semantics_iterative_mapper

    dims = MapDimensions(6.4, 6.4, 0.1)
    kw = dict(b_max=2, world_capacity=n + 1024)
    it = create_gt_semantics_iterative_mapper(dev, CameraParameters(float(np.deg2rad(90.0)), (64, 64), 0.1), dims, **kw)
    it.ensure_handle(64, 64)
    known = MappingModule(dev, None, dims, mode="known", **kw)
    known._ensure_handle(64, 64)
    rng = np.random.RandomState(9)
    side = float(np.sqrt(n)) * 0.05  # about one point per 5 cm cell
    xyz = torch.from_numpy(np.stack([rng.uniform(0, side, n), rng.uniform(0.4, 1.7, n), rng.uniform(0, side, n)], 1)
                           .astype(np.float32)).to(dev)
    sem = torch.from_numpy(rng.randint(1, 13, n).astype(np.uint8)).to(dev)

    def load_known():
        check(lib().ivln_mapper_load_known(known._h, 0, xyz.data_ptr(), sem.data_ptr(), n, stream_ptr()), "load_known")

    calls = {"load_known": load_known, "seed_row": lambda: it.seed_row(0, xyz, sem)}
    times = {k: [] for k in SETTINGS}
    for rnd in range(2 + rounds):
        for k in SETTINGS:
            (it if k == "seed_row" else known).reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls[k]()
            torch.cuda.synchronize()
            if rnd >= 2:
                times[k].append((time.perf_counter() - t0) * 1e3)
        assert it.check_status() == n and known.status() == (0, n)
    res = {"points": n, "rounds": rounds}
    for k in SETTINGS:
        res[f"{k}_ms"] = _three(times[k])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="10000,100000,1000000")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("map_seed_cost: needs the GPU (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    for n in (int(p) for p in a.points.split(",")):
        print(json.dumps(run(n, a.rounds, dev)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
