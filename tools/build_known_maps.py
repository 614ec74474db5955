"""Builds the scene files of known-map mode by exploring: drives the project's vector env with the expert action of
`shortest_path_sensor`, feeds every step's observations to an iterative mapper transformer and writes each scene's cloud to
`{out}/{scene}.npz` (ivln_ce_amd.known_maps.build_known_maps) - the files `GTSemanticsKnownMapper` reads from
data/known_maps/gt_semantics, or with --predicted (RedNet labels from rgb + depth) the ones `PredictedSemanticsKnownMapper`
reads from data/known_maps/predicted_semantics.

    python tools/build_known_maps.py [--exp-config <yaml>] --out data/known_maps/gt_semantics --steps-per-scene 200 [--predicted]
                                     [KEY VALUE ...]   (trailing config overrides)

The vector env comes from ivln_ce_amd.envs.construct_envs, so the backend is chosen through the trailing overrides:
`ENV_BACKEND synthetic` (the default: env i stays in scene{i}, its frames are noise) or `ENV_BACKEND boxworld` (env i stays
in the room bw{i}; depth and labels are ray-cast from the pose on the device, so the files hold the room's surfaces: every
point of label L lies on a box of label L, `boxworld.surface_distance`).  An episode that ends is followed by the next one
of the same scene and the scene's cloud keeps growing across that boundary.  Prints one JSON line {scene: points}."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def explore(envs, steps, device):
    """`steps` batches from the vector env under the expert's actions (episodic protocol, finished episodes restart)."""
    from ivln_ce_amd.utils import batch_obs

    obs = envs.reset()
    for t in range(steps):
        yield batch_obs(obs, device)
        if t + 1 < steps:
            actions = [int(o["shortest_path_sensor"][0]) for o in obs]
            obs = [out[0] for out in envs.step(actions)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exp-config", default=None)
    ap.add_argument("--out", required=True)
    ap.add_argument("--steps-per-scene", type=int, required=True)
    ap.add_argument("--predicted", action="store_true", help="labels from RedNet (rgb + depth) instead of semantic12")
    ap.add_argument("opts", nargs=argparse.REMAINDER)
    a = ap.parse_args()
    if a.steps_per_scene <= 0:
        raise SystemExit("build_known_maps: --steps-per-scene must be positive")
    if not torch.cuda.is_available():
        raise SystemExit("build_known_maps: the mapper runs on the GPU (there is no CPU fallback)")
    from ivln_ce_amd import obs_transforms
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.envs import construct_envs
    from ivln_ce_amd.known_maps import build_known_maps

    cfg = get_config(a.exp_config, a.opts or None)
    device = torch.device("cuda", int(cfg.TORCH_GPU_ID))
    cls = obs_transforms.PredictedSemanticsIterativeMapper if a.predicted else obs_transforms.GTSemanticsIterativeMapper
    transformer = cls.from_config(cfg)
    envs = construct_envs(cfg, auto_reset_done=True, iterative=False, with_rgb=a.predicted)
    try:
        with torch.no_grad():
            result = build_known_maps(explore(envs, a.steps_per_scene, device), transformer, out_dir=a.out)
    finally:
        envs.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
