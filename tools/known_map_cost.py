"""What the known-map rollout step costs: `GTSemanticsKnownMapper` + `MapCMAPolicy.act` at `--envs` envs, scene clouds of
`--points` points each (two envs per scene), one row reset every `--reset-every` steps, for
  copy_eager     the copy path (EGOCENTRIC_MAPPER.known_library False): ivln_mapper_known_begin compacts the whole world
                 every step, a reset copies the scene into the row, the step reads the device to find the finished rows
  library_eager  the scene library (mapping.KnownSceneLibrary, ivln_mapper_known_step), launched eagerly
  library_replay the same step captured and replayed (graphed.GraphedRollout, split mode as the trainers build it), the host's
                 part in `stage_host` in front of each replay

    python tools/known_map_cost.py [--envs 8] [--points 100000,1000000,3000000] [--rounds 5] [--steps 100]

Host clock around `steps` steps that end in a synchronise, the settings alternating round by round in one process after two
warm-up rounds; median / min / max over `rounds`.  The first setting is the yardstick of the others in the same call.
Prints one JSON line per cloud size."""
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
SETTINGS = ("copy_eager", "library_eager", "library_replay")


def _three(xs):
    return [round(statistics.median(xs), 4), round(min(xs), 4), round(max(xs), 4)]


def write_scenes(n_scenes, points):
    """scene{i}.npz under data/known_maps/gt_semantics of the working directory (where the plugins look)."""
    d = os.path.join("data", "known_maps", "gt_semantics")
    os.makedirs(d, exist_ok=True)
    rng = np.random.RandomState(points % 9973)
    for i in range(n_scenes):
        xyz = np.stack([rng.uniform(-8, 8, points), rng.uniform(0.0, 2.5, points), rng.uniform(-8, 8, points)], 1)
        np.savez(os.path.join(d, f"scene{i}.npz"), xyz=xyz.astype(np.float32), semantics=rng.randint(0, 13, points).astype(np.uint8))


def observations(B, n_scenes, reset_every, dev, n=4):
    """(obs per step of one period of 2 * reset_every steps): all rows reset at step 0 of the FIRST period only (see `run`),
    one row - rotating - at every reset_every-th step"""
    from ivln_ce_amd.synthetic import SyntheticRollout

    roll = SyntheticRollout(B=B, seed=1)
    base = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in roll.step().items()} for _ in range(n)]
    names = [f"scene{b % n_scenes}" for b in range(B)]
    for o in base:
        o["env_name"] = list(names)
        o["world_robot_pose"][:, 0] = torch.linspace(-2.0, 2.0, B, device=dev)
        o["world_robot_pose"][:, 2] = 0.5
    ones = torch.ones(B, 1, dtype=torch.uint8, device=dev)
    resets = []
    for b in range(B):
        m = ones.clone()
        m[b] = 0
        resets.append(m)
    return base, ones, resets, torch.zeros(B, 1, dtype=torch.uint8, device=dev)


class Setting:
    def __init__(self, kind, B, points, dev):
        from ivln_ce_amd.config import get_config
        from ivln_ce_amd.obs_transforms import GTSemanticsKnownMapper
        from ivln_ce_amd.policy import MapCMAPolicy
        from ivln_ce_amd.spaces import Box, Dict, Discrete

        self.kind, self.B = kind, B
        cfg = get_config(opts=["MODEL.policy_name", "MapCMAPolicy", "MODEL.INSTRUCTION_ENCODER.use_pretrained_embeddings", False,
                               "MODEL.DEPTH_ENCODER.ddppo_checkpoint", "NONE",
                               "RL.POLICY.OBS_TRANSFORMS.EGOCENTRIC_MAPPER.known_library", kind != "copy_eager"])
        sp = {"depth": Box(0.0, 1.0, (256, 256, 1), np.float32), "occupancy_map": Box(0, 255, (64, 64), np.uint8),
              "semantic_map": Box(0, 255, (64, 64), np.uint8), "instruction": Box(0, 2504, (200,), np.int64)}
        torch.manual_seed(0)
        self.policy = MapCMAPolicy.from_config(cfg, Dict(sp), Discrete(4)).to(dev).eval()
        self.tr = GTSemanticsKnownMapper.from_config(cfg)
        self.tr.sizing["b_max"] = B
        self.tr.sizing["world_capacity"] = B * points + 1024  # (the copy path holds every row's copy of its scene)
        self.rnn = torch.zeros(B, self.policy.net.num_recurrent_layers, cfg.MODEL.STATE_ENCODER.hidden_size, device=dev)
        self.prev = torch.zeros(B, 1, dtype=torch.long, device=dev)
        self.runner = None
        self.t = 0

    def step(self, obs):
        if self.kind == "library_replay":
            if self.runner is None:
                from ivln_ce_amd.graphed import GraphedRollout

                self.runner = GraphedRollout(self.policy, [self.tr], obs, deterministic=True, streams="split")
                self.tr.mapping_module.reset()
            return self.runner.step(obs)
        with torch.no_grad():
            batch = self.tr(dict(obs))
            actions, self.rnn = self.policy.act(batch, self.rnn, self.prev, obs["not_done_masks"], deterministic=True)
            self.prev.copy_(actions)
        return actions


def run(points, B, rounds, steps, reset_every, dev):
    n_scenes = max(1, B // 2)
    write_scenes(n_scenes, points)
    base, ones, resets, zeros = observations(B, n_scenes, reset_every, dev)
    runs = {k: Setting(k, B, points, dev) for k in SETTINGS}
    times = {k: [] for k in SETTINGS}
    for rnd in range(2 + rounds):
        for k, st in runs.items():
            if rnd == 0:  # every row loads its scene
                st.step(dict(base[0], not_done_masks=zeros))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                nd = resets[(st.t // reset_every) % B] if st.t % reset_every == reset_every - 1 else ones
                st.step(dict(base[i & 3], not_done_masks=nd))
                st.t += 1
            torch.cuda.synchronize()
            if rnd >= 2:
                times[k].append((time.perf_counter() - t0) * 1e3 / steps)
    res = {"envs": B, "points_per_scene": points, "scenes": n_scenes, "reset_every": reset_every, "steps": steps, "rounds": rounds}
    for k, st in runs.items():
        res[f"{k}_ms"] = _three(times[k])
        res[f"{k}_world_points"] = int(st.tr.mapping_module.check_status())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--points", default="100000,1000000,3000000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reset-every", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("known_map_cost: needs the GPU (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    for points in (int(p) for p in a.points.split(",")):
        with tempfile.TemporaryDirectory() as tmp:
            os.chdir(tmp)  # (the plugins read data/known_maps/... relative to the working directory)
            try:
                print(json.dumps(run(points, a.envs, a.rounds, a.steps, a.reset_every, dev)), flush=True)
            finally:
                os.chdir(ROOT)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
