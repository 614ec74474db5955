"""Golden vectors for the known-map builder, every step done by the REFERENCE: its iterative `MappingModule`
(mapper.py:904-944, `create_gt_semantics_iterative_mapper`) runs over seeded 32x32 frames with B = 2 - row 0 stays in
scene gA, row 1 is in gB and moves to gC half-way (not_done 0 on a row's first frame of a scene, 1 otherwise: what
`known_maps.build_known_maps` supplies) -, each scene's cloud (`get_world_semantic_pointcloud()` restricted to the row,
taken before the row is cleared and at the end) is written with np.savez(xyz=..., semantics=...), and its known mapper
(`create_known_mapper`: `GetGTWorldSemanticPointcloud` :851-881 over `SemanticPointcloud.from_npz_file` :283-294) is
stepped over a pose list on those files.

Build container only:  python tests/golden/gen_known_build_golden.py  ->  tests/golden/known_build.npz
(frames, scene names per step, per-scene clouds, known-mode poses / masks / names and the expected maps; data only)."""
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_mapper_golden as G  # noqa: E402  (installs the import shim; seeded frames + the reference mapper's set-up)

M = G.M
OUT = os.path.dirname(os.path.abspath(__file__))
H = W = 32
B, STEPS, SWITCH = 2, 6, 3


def scene_names(t):
    return ["gA", "gB" if t < SWITCH else "gC"]


if __name__ == "__main__":
    frames = G.make_sequence(seed=21, B=B, H=H, W=W, steps=STEPS, resets=[(SWITCH, 1)])
    cam = M.CameraParameters(vertical_fov_radians=float(np.deg2rad(90.0 * (H / W))), features_spatial_dimensions=(H, W),
                             height_clip=0.1)
    dims = M.MapDimensions(height_meters=6.4, width_meters=6.4, resolution_meters=0.1)
    mm = M.create_gt_semantics_iterative_mapper(torch.device("cpu"), cam, dims)
    d = dict(B=B, H=H, W=W, steps=STEPS)
    clouds = {}

    def take(b, name):
        w = mm.get_world_semantic_pointcloud()
        keep = w.batch_indices == b
        clouds[name] = (w.xyz[keep].clone().numpy().astype(np.float32), w.semantics[keep].clone().numpy().astype(np.int64))

    for t, f in enumerate(frames):
        names = scene_names(t)
        if t == SWITCH:
            take(1, scene_names(t - 1)[1])  # before the step that clears the row
        ep = M.EpisodesInfo(f["not_done_masks"].clone(), list(names))
        obs = M.Observations(semantics=f["semantic12"].permute(0, 3, 1, 2), depth_normalized=f["depth"].permute(0, 3, 1, 2),
                             rgb=None)
        st = M.RobotCurrentState(pose=f["world_robot_pose"].clone(), elevation=f["world_robot_orientation"][:, 0].clone(),
                                 heading=f["world_robot_orientation"][:, 1].clone())
        mm(ep, obs, st)
        d[f"depth_{t}"], d[f"semantic12_{t}"] = f["depth"].numpy(), f["semantic12"].numpy()
        d[f"pose_{t}"], d[f"orientation_{t}"] = f["world_robot_pose"].numpy(), f["world_robot_orientation"].numpy()
        d[f"not_done_{t}"] = f["not_done_masks"].numpy()
        d[f"env_names_{t}"] = np.array(names)
    take(0, "gA")
    take(1, "gC")
    for name, (xyz, sem) in clouds.items():
        d[f"scene_{name}_xyz"], d[f"scene_{name}_semantics"] = xyz, sem

    # the reference's known mapper on the files of those clouds
    known = [  # (not_done per row, scene per row)
        ([0, 0], ["gA", "gB"]),
        ([1, 1], ["gA", "gB"]),
        ([0, 1], ["gC", "gB"]),
        ([1, 0], ["gC", "gA"]),
    ]
    d["known_steps"] = len(known)
    with tempfile.TemporaryDirectory() as tmp:
        for name, (xyz, sem) in clouds.items():
            np.savez(os.path.join(tmp, f"{name}.npz"), xyz=xyz, semantics=sem)
        km = M.create_known_mapper(torch.device("cpu"), dims, maps_location=tmp)
        for t, (nd, names) in enumerate(known):
            f = frames[min(t + 1, STEPS - 1)]
            pose = f["world_robot_pose"].clone()
            pose[:, 0] += 0.15 * t
            orient = f["world_robot_orientation"].clone()
            orient[:, 1] += 0.3 * t
            ndt = torch.tensor(nd, dtype=torch.uint8).reshape(B, 1)
            ep = M.EpisodesInfo(ndt.clone(), list(names))
            obs = M.Observations(semantics=None, depth_normalized=torch.zeros(B, 1, 8, 8), rgb=None)
            st = M.RobotCurrentState(pose=pose.clone(), elevation=orient[:, 0].clone(), heading=orient[:, 1].clone())
            mem = km(ep, obs, st)
            d[f"kpose_{t}"], d[f"korientation_{t}"], d[f"knot_done_{t}"] = pose.numpy().copy(), orient.numpy().copy(), ndt.numpy()
            d[f"kenv_names_{t}"] = np.array(names)
            d[f"kocc_{t}"], d[f"ksem_{t}"] = mem.occupancy.clone().numpy(), mem.semantic.clone().numpy()
    path = os.path.join(OUT, "known_build.npz")
    np.savez_compressed(path, **d)
    print("clouds", {k: int(v[1].shape[0]) for k, v in clouds.items()}, "occ cells",
          [int(d[f"kocc_{t}"].sum()) for t in range(len(known))], "sem cells",
          [int((d[f"ksem_{t}"] > 0).sum()) for t in range(len(known))], os.path.getsize(path) // 1024, "KiB")
