"""Golden vectors for egocentric maps other than 64 x 64 cells (EGOCENTRIC_MAPPER.height_meters / width_meters /
resolution_meters), by running the REFERENCE's own `MappingModule`, `create_known_mapper` and `MapCMAPolicy` with their own
`MapDimensions` / observation space.  Build container only:  python tests/golden/gen_map_sizes_golden.py

  map_sizes_mapper_{32x48,96x112,res02}.npz  iterative gt-semantics mapper, layout of mapper_b4_32.npz (+ the three map keys)
                                             (not mapper_*.npz: tests/test_gpu_mapper.py runs every file of that pattern at
                                             6.4 m / 6.4 m / 0.1 m)
  known_map_sizes.npz                        one known-map case at 3.2 m x 4.8 m, layout of known_map.npz
  policy_map_sizes.npz                       32x48 (6 map positions) and 96x112 (42): two act() steps on cached depth features
                                             and one update (T = 3, N = 2, progress monitor, train mode), keys "<case>/..."

Data only, every file under 1 MB.  The one listed gradient that is large (net.state_q.weight, 512 KB per case) is stored as
every 8th row ("gradrows8/..."), and map_linear's weight gradient - the one whose shape follows the map - as every 16th
("gradrows16/..."); their norms, like every parameter's, are stored in full.
torch.set_num_threads(1) for the mapper: the reference's duplicate-index map store is only deterministic single-threaded."""
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_mapper_golden import _ref_shim, make_sequence  # noqa: E402  (installs the shim, sets one thread; runs nothing)
from det_init import det_fill  # noqa: E402

from ivlnce_baselines.common.aux_losses import AuxLosses  # noqa: E402
from ivlnce_baselines.common.mapping_module import mapper as M  # noqa: E402
from ivlnce_baselines.common.mapping_module.projector import _transform3D  # noqa: E402
from ivlnce_baselines.models.map_cma_policy import MapCMAPolicy  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
LIMIT = 1_000_000


def _save(name, d):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    assert size < LIMIT, (name, size)
    return size // 1024


# ---- mapper --------------------------------------------------------------------------------------------------------
def mapper_case(name, dims3, depth_scale, seed):
    """make_sequence's walls stand 2 - 8 m away: outside a 3.2 m map.  Valid readings (not the sprinkled 0 / 1) are scaled
    so that the walls fall inside the map."""
    B, H, W, steps = 2, 32, 32, 4
    frames = make_sequence(seed, B, H, W, steps, resets=[(2, 1)])
    for f in frames:
        d = f["depth"]
        f["depth"] = torch.where((d > 0) & (d < 1), d * depth_scale, d)
    cam = M.CameraParameters(vertical_fov_radians=float(np.deg2rad(90.0 * (H / W))), features_spatial_dimensions=(H, W),
                             height_clip=0.1)
    dims = M.MapDimensions(height_meters=dims3[0], width_meters=dims3[1], resolution_meters=dims3[2])
    mm = M.create_gt_semantics_iterative_mapper(torch.device("cpu"), cam, dims)
    d = dict(B=B, H=H, W=W, steps=steps, seed=seed, height_meters=dims3[0], width_meters=dims3[1],
             resolution_meters=dims3[2], num_rows=int(dims.num_rows), num_cols=int(dims.num_cols))
    for t, f in enumerate(frames):
        ep = M.EpisodesInfo(f["not_done_masks"].clone(), ["s"] * B)
        obs = M.Observations(semantics=f["semantic12"].permute(0, 3, 1, 2), depth_normalized=f["depth"].permute(0, 3, 1, 2),
                             rgb=None)
        st = M.RobotCurrentState(pose=f["world_robot_pose"].clone(), elevation=f["world_robot_orientation"][:, 0].clone(),
                                 heading=f["world_robot_orientation"][:, 1].clone())
        T = _transform3D(st.pose, st.elevation + torch.pi, st.heading)
        rot = M.rotate_around_y_matrix(-st.heading)
        mem = mm(ep, obs, st)
        w = mm.get_world_semantic_pointcloud()
        occ, sem = mem.occupancy.clone().numpy(), mem.semantic.clone().numpy()
        assert occ.shape == (B, dims.num_rows, dims.num_cols), occ.shape
        if t > 0:  # an empty fixture proves nothing
            for b in range(B):
                assert int((occ[b] > 0).sum()) >= 40, (name, t, b, int((occ[b] > 0).sum()))
                assert len(set(np.unique(sem[b]).tolist()) - {0}) >= 3, (name, t, b, np.unique(sem[b]))
        d[f"depth_{t}"] = f["depth"].numpy()
        d[f"semantic12_{t}"] = f["semantic12"].numpy()
        d[f"pose_{t}"] = f["world_robot_pose"].numpy()
        d[f"orientation_{t}"] = f["world_robot_orientation"].numpy()
        d[f"not_done_{t}"] = f["not_done_masks"].numpy()
        d[f"occ_{t}"], d[f"sem_{t}"] = occ, sem
        d[f"T_{t}"], d[f"rot_{t}"] = T.numpy().copy(), rot.numpy().copy()
        d[f"world_n_{t}"] = np.int64(w.xyz.shape[0])
        if t == steps - 1:
            d[f"world_xyz_{t}"] = w.xyz.clone().numpy()
            d[f"world_b_{t}"] = w.batch_indices.clone().numpy().astype(np.int32)
            d[f"world_sem_{t}"] = w.semantics.clone().numpy()
    kib = _save(f"map_sizes_mapper_{name}.npz", d)
    print(name, (dims.num_rows, dims.num_cols), "occ cells", [int((d[f"occ_{t}"] > 0).sum()) for t in range(steps)], kib, "KiB")


# ---- known map -----------------------------------------------------------------------------------------------------
def known_case():
    from gen_known_map_golden import scene

    scenes = {"sceneA": scene(11, 1500), "sceneB": scene(12, 1100)}
    B, steps = 3, 4
    env_names = ["sceneA", "sceneB", "sceneA"]
    resets = {0: [0, 1, 2], 2: [1], 3: [0, 2]}
    dims3 = (3.2, 4.8, 0.1)
    d = dict(B=B, steps=steps, env_names=np.array(env_names), height_meters=dims3[0], width_meters=dims3[1],
             resolution_meters=dims3[2])
    for k, (xyz, sem) in scenes.items():
        d[f"scene_{k}_xyz"], d[f"scene_{k}_semantics"] = xyz, sem
    with tempfile.TemporaryDirectory() as tmp:
        for k, (xyz, sem) in scenes.items():
            np.savez(os.path.join(tmp, f"{k}.npz"), xyz=xyz, semantics=sem)
        dims = M.MapDimensions(height_meters=dims3[0], width_meters=dims3[1], resolution_meters=dims3[2])
        mm = M.create_known_mapper(torch.device("cpu"), dims, maps_location=tmp)
        g = torch.Generator().manual_seed(5)
        pose = torch.zeros(B, 3)
        pose[:, 1] = torch.tensor([1.25, 1.4, 0.9])
        pose[:, 0] = torch.tensor([0.0, -1.0, 1.5])
        heading = torch.rand(B, generator=g, dtype=torch.float64) * 6.28 - 3.14
        for t in range(steps):
            nd = torch.ones(B, 1, dtype=torch.uint8)
            for b in resets.get(t, []):
                nd[b, 0] = 0
            elev = (torch.rand(B, generator=g, dtype=torch.float64) - 0.5) * 0.02
            orient = torch.stack([elev, heading.clone()], 1)
            ep = M.EpisodesInfo(nd.clone(), list(env_names))
            obs = M.Observations(semantics=None, depth_normalized=torch.zeros(B, 1, 8, 8), rgb=None)
            st = M.RobotCurrentState(pose=pose.clone(), elevation=orient[:, 0].clone(), heading=orient[:, 1].clone())
            mem = mm(ep, obs, st)
            w = mm.get_world_semantic_pointcloud()
            d[f"pose_{t}"], d[f"orientation_{t}"], d[f"not_done_{t}"] = pose.numpy().copy(), orient.numpy().copy(), nd.numpy()
            d[f"occ_{t}"], d[f"sem_{t}"] = mem.occupancy.clone().numpy(), mem.semantic.clone().numpy()
            assert d[f"occ_{t}"].shape == (B, 32, 48)
            assert all(int((d[f"occ_{t}"][b] > 0).sum()) >= 40 for b in range(B))
            d[f"world_n_{t}"] = np.int64(w.xyz.shape[0])
            pose[:, 0] += (-0.25 * torch.sin(heading)).float()
            pose[:, 2] += (-0.25 * torch.cos(heading)).float()
            heading += np.deg2rad(15.0) * (1 if t % 2 == 0 else -2)
    kib = _save("known_map_sizes.npz", d)
    print("known 32x48 occ cells", [int(d[f"occ_{t}"].sum()) for t in range(steps)], kib, "KiB")


# ---- policy --------------------------------------------------------------------------------------------------------
def _space(rows, cols):
    sp = sys.modules["gym.spaces"]
    return sp.Dict({
        "depth": sp.Box(0.0, 1.0, (256, 256, 1), np.float32),
        "occupancy_map": sp.Box(0, 255, (rows, cols), np.uint8),
        "semantic_map": sp.Box(0, 255, (rows, cols), np.uint8),
        "instruction": sp.Box(0, 2504, (200,), np.int64),
    })


def _policy(rows, cols, use_pm):
    cfg = _ref_shim.default_model_config()
    cfg.MODEL.PROGRESS_MONITOR.use = use_pm
    pol = MapCMAPolicy.from_config(cfg, _space(rows, cols), sys.modules["gym.spaces"].Discrete(4))
    det_fill(pol, seed=0)
    return pol


def policy_act(d, tag, rows, cols, seed):
    B = 2
    g = torch.Generator().manual_seed(seed)
    pol = _policy(rows, cols, False)
    pol.eval()
    assert pol.net.map_linear[1].in_features == 128 * (rows // 16) * (cols // 16)
    feats = {}
    pol.net.map_encoder.register_forward_hook(lambda m, i, o: feats.__setitem__("map", o.detach().clone()))
    rnn = torch.zeros(B, 2, 512)
    prev = torch.zeros(B, 1, dtype=torch.long)
    instr = torch.zeros(B, 200, dtype=torch.long)
    for b, L in enumerate([57, 200]):
        instr[b, :L] = torch.randint(2, 2504, (L,), generator=g)
    d[f"{tag}/act/instruction"] = instr.numpy()
    for t in range(2):
        depth_features = torch.randn(B, 128, 4, 4, generator=g)
        occ = (torch.rand(B, rows, cols, generator=g) < 0.3).to(torch.uint8)
        sem = (torch.randint(0, 13, (B, rows, cols), generator=g) * occ).to(torch.uint8)
        masks = torch.ones(B, 1, dtype=torch.uint8)
        if t == 0:
            masks[:] = 0
        else:
            masks[1] = 0  # env 1 starts a new episode at step 1
        obs = {"depth_features": depth_features, "occupancy_map": occ, "semantic_map": sem, "instruction": instr}
        with torch.no_grad():
            f, rnn_out = pol.net(obs, rnn, prev, masks)
            logits = pol.action_distribution(f).logits
            action = logits.argmax(-1, keepdim=True)
        for k, v in [("depth_features", depth_features), ("occ", occ), ("sem", sem), ("masks", masks), ("prev", prev),
                     ("rnn_in", rnn), ("rnn_out", rnn_out), ("features", f), ("logits", logits), ("map_feat", feats["map"])]:
            d[f"{tag}/act/{k}_{t}"] = v.numpy().copy()
        rnn, prev = rnn_out, action
    print(tag, "act logits", d[f"{tag}/act/logits_1"].tolist())


def policy_update(d, tag, rows, cols, seed):
    T, N = 3, 2
    g = torch.Generator().manual_seed(seed)
    pol = _policy(rows, cols, True)
    pol.train()
    TN = T * N
    instr1 = torch.zeros(N, 200, dtype=torch.long)
    for b, L in enumerate([40, 131]):
        instr1[b, :L] = torch.randint(2, 2504, (L,), generator=g)
    instr = instr1.unsqueeze(0).expand(T, N, 200).reshape(TN, 200).float()
    occ_u8 = (torch.rand(TN, rows, cols, generator=g) < 0.3).to(torch.uint8)
    sem_u8 = (torch.randint(0, 13, (TN, rows, cols), generator=g).to(torch.uint8) * occ_u8)
    depth_features = torch.randn(TN, 128, 4, 4, generator=g)
    progress = torch.rand(TN, 1, generator=g)
    prev = torch.randint(0, 4, (TN, 1), generator=g)
    tgt = torch.randint(0, 4, (T, N), generator=g)
    w = torch.where(torch.rand(T, N, generator=g) < 0.3, torch.tensor(3.2), torch.tensor(1.0))
    w[2:, 1] = 0.0  # a padded (shorter) trajectory
    nd = torch.ones(T, N, dtype=torch.uint8)
    nd[0] = 0
    nd = nd.view(-1, 1)
    obs = {"depth_features": depth_features, "occupancy_map": occ_u8.float(), "semantic_map": sem_u8.float(),
           "instruction": instr, "progress": progress}
    AuxLosses.activate()
    AuxLosses.clear()
    dist, _ = pol.build_distribution(obs, torch.zeros(N, 2, 512), prev, nd)
    logits = dist.logits.view(T, N, -1)
    ce = F.cross_entropy(logits.permute(0, 2, 1), tgt, reduction="none")
    action_loss = ((w * ce).sum(0) / w.sum(0)).mean()
    aux = AuxLosses.reduce((w > 0).view(-1))
    loss = action_loss + aux
    loss.backward()
    AuxLosses.deactivate()
    p = f"{tag}/update/"
    d.update({p + "T": T, p + "N": N, p + "instruction": instr.numpy(), p + "occ": occ_u8.numpy(), p + "sem": sem_u8.numpy(),
              p + "depth_features": depth_features.numpy(), p + "progress": progress.numpy(), p + "prev": prev.numpy(),
              p + "targets": tgt.numpy(), p + "weights": w.numpy(), p + "not_done": nd.numpy(),
              p + "logits": logits.detach().numpy(), p + "loss": float(loss), p + "action_loss": float(action_loss),
              p + "aux_loss": float(aux)})
    params = dict(pol.named_parameters())
    for k, q in params.items():
        if q.grad is not None:
            d[p + "gradnorm/" + k] = float(q.grad.norm())
    for k in ["action_distribution.linear.weight", "net.map_encoder.cnn.0.conv.0.bias", "net.map_encoder.cnn.3.conv.1.weight",
              "net.prev_action_embedding.weight", "net.text_q.bias", "net.state_encoder.rnn.bias_hh_l0",
              "net.instruction_encoder.encoder_rnn.bias_ih_l0_reverse", "net.depth_encoder.spatial_embeddings.weight",
              "net.progress_monitor.weight", "net.map_kv.bias"]:
        d[p + "grad/" + k] = params[k].grad.numpy()
    d[p + "gradrows8/net.state_q.weight"] = params["net.state_q.weight"].grad.numpy()[::8].copy()
    # (map_linear's weight gradient is the tensor whose shape follows the map: 8 of its 128 rows)
    d[p + "gradrows16/net.map_linear.1.weight"] = params["net.map_linear.1.weight"].grad.numpy()[::16].copy()
    sd = pol.state_dict()
    for k in ["net.map_encoder.cnn.0.conv.1.running_mean", "net.map_encoder.cnn.3.conv.1.running_var"]:
        d[p + "post/" + k] = sd[k].numpy()
    print(tag, "update loss", float(loss), float(action_loss), float(aux))


if __name__ == "__main__":
    assert torch.get_num_threads() == 1
    mapper_case("32x48", (3.2, 4.8, 0.1), 0.2, seed=21)
    mapper_case("96x112", (9.6, 11.2, 0.1), 0.6, seed=22)
    mapper_case("res02", (6.4, 6.4, 0.2), 0.4, seed=29)
    known_case()
    d = {}
    for tag, rows, cols, seed in [("32x48", 32, 48, 501), ("96x112", 96, 112, 502)]:
        policy_act(d, tag, rows, cols, seed)
        policy_update(d, tag, rows, cols, seed + 10)
    print("policy_map_sizes.npz", _save("policy_map_sizes.npz", d), "KiB")
