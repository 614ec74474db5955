"""Host side of the egocentric mapper: owns the device state handle and mirrors the reference's
`MappingModule` objects (ivlnce_baselines/common/mapping_module/mapper.py:904-1028) and
`setup_mapping_module.py:13-89`.  All arithmetic is in csrc/mapper.hip.
"""
import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib
from ._lib import check, dptr, lib, stream_ptr

# ivln_mapper_step_posed: camera transforms derived inside the step's first kernel (6 launches per step instead of
# frames + 6); IVLN_MAPPER_POSED=0 keeps the separate ivln_mapper_frames launch (A/B, tests of the older entry points)
STEP_POSED = os.environ.get("IVLN_MAPPER_POSED", "1") != "0"


@dataclass
class CameraParameters:  # mapper.py:336-340
    vertical_fov_radians: float
    features_spatial_dimensions: tuple
    height_clip: float


@dataclass
class MapDimensions:  # mapper.py:89-99
    height_meters: float
    width_meters: float
    resolution_meters: float

    @property
    def num_rows(self):
        return math.ceil(self.height_meters / self.resolution_meters)

    @property
    def num_cols(self):
        return math.ceil(self.width_meters / self.resolution_meters)


def extract_camera_parameters(depth_sensor_params, map_sensor_params) -> CameraParameters:
    """setup_mapping_module.py:13-42: vfov = HFOV * H / W (degrees -> radians)."""
    vfov_deg = depth_sensor_params.HFOV * (depth_sensor_params.HEIGHT / depth_sensor_params.WIDTH)
    return CameraParameters(
        vertical_fov_radians=float(np.deg2rad(vfov_deg)),
        features_spatial_dimensions=(depth_sensor_params.HEIGHT, depth_sensor_params.WIDTH),
        height_clip=map_sensor_params.height_clip,
    )


def extract_egocentric_map_parameters(map_sensor_params) -> MapDimensions:
    """setup_mapping_module.py:45-54."""
    return MapDimensions(
        height_meters=map_sensor_params.height_meters,
        width_meters=map_sensor_params.width_meters,
        resolution_meters=map_sensor_params.resolution_meters,
    )


class OccupancySemanticMapMemory:
    """mapper.py:620-648: persistent (B,rows,cols) uint8 buffers returned by reference."""

    def __init__(self, b_max, rows, cols, device):
        self._occ = torch.zeros((b_max, rows, cols), dtype=torch.uint8, device=device)
        self._sem = torch.zeros((b_max, rows, cols), dtype=torch.uint8, device=device)
        self.batch_size = b_max

    @property
    def occupancy(self):
        return self._occ[: self.batch_size]

    @property
    def semantic(self):
        return self._sem[: self.batch_size]


def load_known_scene(maps_location, env_name):
    """{maps_location}/{env_name}.npz -> (xyz (n, 3) float32, semantics (n,) uint8), contiguous numpy arrays in file order
    (mapper.py:283-294)."""
    with np.load(os.path.join(maps_location, f"{env_name}.npz")) as f:
        xyz = np.ascontiguousarray(f["xyz"], dtype=np.float32).reshape(-1, 3)
        sem = np.ascontiguousarray(f["semantics"]).astype(np.int64).astype(np.uint8).reshape(-1)
    return xyz, sem


def save_known_scene(maps_location, env_name, xyz, semantics):
    """The inverse of `load_known_scene`: writes {maps_location}/{env_name}.npz with the keys known-map mode reads,
    `xyz` (n, 3) float32 and `semantics` (n,) int64 - the reference builds `torch.LongTensor(f["semantics"])`
    (mapper.py:283-294), which takes an int64 array and nothing narrower.  Row order is file order.  Returns the path."""
    xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32).reshape(-1, 3))
    sem = np.ascontiguousarray(np.asarray(semantics).reshape(-1).astype(np.int64))
    if xyz.shape[0] != sem.shape[0]:
        raise ValueError(f"scene {env_name}: {xyz.shape[0]} points but {sem.shape[0]} labels")
    os.makedirs(maps_location, exist_ok=True)
    path = os.path.join(maps_location, f"{env_name}.npz")
    np.savez(path, xyz=xyz, semantics=sem)
    return path


class KnownSceneLibrary:
    """Device-resident scene clouds of known-map mode, each held once (include/ivln_known_lib.h).  The host side is a
    dict name -> index; a scene is read from `{maps_location}/{name}.npz` the first time its name is seen, packed on the
    device into 16-byte records (x, y, z, label) and entered into the library's device table, whose address never changes -
    a captured step that is replayed behind an `index()` call sees the new scene.  The record tensors live as long as
    the library does."""

    def __init__(self, device, maps_location, max_scenes: int = 1024):
        self.device = device
        self.maps_location = maps_location
        self.max_scenes = int(max_scenes)
        self._index: Dict[str, int] = {}
        self._records: List[torch.Tensor] = []
        self._h = None

    def __len__(self):
        return len(self._index)

    def __contains__(self, name):
        return name in self._index

    def names(self):
        return list(self._index)

    def points(self, name) -> int:
        return int(self._records[self._index[name]].shape[0])

    def handle(self):
        """The C handle (created on first use, on the library's device)."""
        if self._h is None:
            h = C.c_void_p()
            with torch.cuda.device(self.device):
                check(lib().ivln_known_lib_create(self.max_scenes, C.byref(h)), "ivln_known_lib_create")
            self._h = h
        return self._h

    def __del__(self):
        try:
            if self._h is not None:
                lib().ivln_known_lib_destroy(self._h)
                self._h = None
        except Exception:  # noqa: BLE001
            pass

    def _load(self, name):
        xyz, sem = load_known_scene(self.maps_location, name)
        return torch.from_numpy(xyz).to(self.device), torch.from_numpy(sem).to(self.device)

    def _add(self, scene, xyz, sem, records):
        """The C call (tests replace it with a stub): pack + table entry, one launch on the current stream."""
        check(lib().ivln_known_lib_add(self.handle(), scene, xyz.data_ptr(), sem.data_ptr(), xyz.shape[0],
                                       records.data_ptr(), stream_ptr()), "ivln_known_lib_add")

    def index(self, name) -> int:
        """Index of scene `name`; loads and adds it on first sight (host file read + one launch on the current stream)."""
        i = self._index.get(name)
        if i is None:
            i = len(self._index)
            if i >= self.max_scenes:
                raise _lib.IvlnError(f"known-scene library is full ({self.max_scenes} scenes)")
            xyz, sem = self._load(name)
            records = torch.empty((xyz.shape[0], 4), dtype=torch.float32, device=self.device)
            # (xyz / sem are read by a launch on the current stream, which is also the stream their memory returns to)
            self._add(i, xyz.contiguous(), sem.contiguous(), records)
            self._records.append(records)
            self._index[name] = i
        return i

    def _add_from_mapper(self, scene, mapping_module, b, records):
        """The C call (tests replace it with a stub): ordered compaction of row b's cloud into `records` + table entry."""
        check(lib().ivln_known_lib_add_from_mapper(self.handle(), scene, mapping_module._h, int(b), records.data_ptr(),
                                                   records.shape[0], stream_ptr()), "ivln_known_lib_add_from_mapper")

    def add_from_mapper(self, name, mapping_module, b) -> int:
        """Promotes the cloud that row `b` of an iterative `MappingModule` has explored to scene `name`, in the reference's cloud
        order and without a host copy of the points (include/ivln_map_build.h): asks for the count, allocates the records,
        one C call on the current stream.  A captured step replayed behind this call sees the scene.  Returns its index; a
        name that is already present raises (an entry a captured step may be reading is never rewritten)."""
        if name in self._index:
            raise _lib.IvlnError(f"known-scene library already holds scene {name!r}")
        i = len(self._index)
        if i >= self.max_scenes:
            raise _lib.IvlnError(f"known-scene library is full ({self.max_scenes} scenes)")
        n = int(mapping_module.env_counts()[b])
        records = torch.empty((n, 4), dtype=torch.float32, device=self.device)
        self._add_from_mapper(i, mapping_module, b, records)
        self._records.append(records)
        self._index[name] = i
        return i


class MappingModule:
    """Drop-in for mapper.py:904-944 (`create_*_mapper` factories :950-1028).

    mode "iterative": labels come from `semantic12` (gt) or from `semantics_module(observations)`
    (predicted, e.g. RedNet) and the world cloud is built online.
    mode "known": the world cloud of each env is loaded from `{maps_location}/{env_name}.npz`
    when its episode resets (mapper.py:851-881).  With `known_library=True` the scenes live once in a
    `KnownSceneLibrary` and a row only latches the index of its scene (ivln_mapper_known_step): no per-step copy, no
    host read inside the step - `stage_host` does the host's part in front of it - so the step can be captured.  Every
    step of such a module goes through the library; without the flag the copy path (ivln_mapper_known_begin /
    _load_known / _known_raster) runs as before.
    """

    def __init__(
        self,
        device: torch.device,
        camera_parameters: Optional[CameraParameters],
        map_dimensions: MapDimensions,
        mode: str = "iterative",
        semantics_module=None,
        maps_location: Optional[str] = None,
        b_max: int = 64,
        world_capacity: int = 0,
        table_cells: int = 0,
        known_library: bool = False,
        scene_library: Optional[KnownSceneLibrary] = None,
    ):
        if device.type != "cuda":
            raise _lib.IvlnError("the HIP mapper needs a GPU device (no CPU fallback)")
        self.device = device
        self.mode = mode
        self.camera_parameters = camera_parameters
        self.map_dimensions = map_dimensions
        self.semantics_module = semantics_module
        self.maps_location = maps_location
        self.b_max = b_max
        self._world_capacity = world_capacity
        self._table_cells = table_cells
        self._h = None
        self._hw = None
        self.map_memory = OccupancySemanticMapMemory(
            b_max, map_dimensions.num_rows, map_dimensions.num_cols, device
        )
        self._T = torch.empty((b_max, 4, 4), dtype=torch.float32, device=device)
        self._rot = torch.empty((b_max, 3, 3), dtype=torch.float32, device=device)
        self._known_cache: Dict[str, tuple] = {}
        self._begin_open = False  # a `begin` whose `finish` has not run: the cloud cannot be exported (export_scene)
        self.known_library = bool(known_library) and mode == "known"
        if self.known_library:
            # (scene_library: one that exists already, e.g. filled by `add_from_mapper`; names it lacks are read from files)
            self.scene_library = scene_library if scene_library is not None else KnownSceneLibrary(device, maps_location)
            self._scene_dev = torch.full((b_max,), -1, dtype=torch.int32, device=device)  # the step's scene index per row
            # pinned staging rows, used in turn: a row is rewritten only after the copy that read it has run
            self._scene_pin = [torch.zeros((b_max,), dtype=torch.int32).pin_memory() for _ in range(4)]
            self._scene_ev = [None] * 4
            self._scene_turn = 0

    # -- handle management ---------------------------------------------------------------
    def _ensure_handle(self, H, W):
        if self._h is not None and self._hw == (H, W):
            return
        if self._h is not None:
            lib().ivln_mapper_destroy(self._h)
        h = C.c_void_p()
        vfov = self.camera_parameters.vertical_fov_radians if self.camera_parameters else math.pi / 2
        md = self.map_dimensions
        with torch.cuda.device(self.device):
            check(
                lib().ivln_mapper_create(
                    self.b_max, H, W, vfov, md.height_meters, md.width_meters, md.resolution_meters,
                    self._world_capacity, self._table_cells, C.byref(h),
                ),
                "ivln_mapper_create",
            )
        self._h, self._hw = h, (H, W)
        if self.known_library:
            check(lib().ivln_mapper_known_attach(self._h, self.scene_library.handle()), "ivln_mapper_known_attach")
        if getattr(self, "_width", (0, 0)) != (0, 0):
            check(lib().ivln_mapper_set_launch_width(self._h, *self._width), "ivln_mapper_set_launch_width")

    def __del__(self):
        try:
            if self._h is not None:
                lib().ivln_mapper_destroy(self._h)
                self._h = None
        except Exception:  # noqa: BLE001
            pass

    def reset(self):
        """Forgets the world cloud and an open `begin` with it (ivln_mapper_reset zeroes the arg-max table)."""
        if self._h is not None:
            check(lib().ivln_mapper_reset(self._h, stream_ptr()), "ivln_mapper_reset")
        self._begin_open = False

    def _refuse_open(self, what):
        if self._begin_open:
            raise _lib.IvlnError(f"MappingModule.{what}: `begin` is open - `finish` or `reset` it first (its arg-max entries "
                                 "are in the mapper's table)")

    # -- frames -----------------------------------------------------------------------------
    def frames(self, pose: torch.Tensor, orientation: torch.Tensor):
        """(B,3) f32 pose + (B,2) f64 [elevation, heading] -> T (B,4,4), rot (B,3,3) on device
        (core.py:6-37, mapper.py:38-48, 132-138)."""
        B = pose.shape[0]
        pose = pose.to(self.device, torch.float32).contiguous()
        orientation = orientation.to(self.device, torch.float64).contiguous()
        check(
            lib().ivln_mapper_frames(dptr(pose), dptr(orientation), B, dptr(self._T), dptr(self._rot), stream_ptr()),
            "ivln_mapper_frames",
        )
        return self._T[:B], self._rot[:B], pose

    # -- library-mode known maps: the host's part of a step ------------------------------------------
    def stage_host(self, observations):
        """Everything a library-mode step needs from the host, in front of the step (graphed.GraphedRollout calls it before
        each replay): scene names -> indices (an unseen scene is read and added to the library here) and ONE async copy of
        the indices from pinned memory into the persistent device buffer the step reads.  No device-to-host traffic."""
        if not self.known_library:
            return
        names = observations["env_name"]
        B = len(names)
        if B > self.b_max:
            raise _lib.IvlnError(f"batch {B} > b_max {self.b_max}")
        k = self._scene_turn
        self._scene_turn = (k + 1) % len(self._scene_pin)
        if self._scene_ev[k] is not None:
            self._scene_ev[k].synchronize()
        pin = self._scene_pin[k]
        index = self.scene_library.index
        pin.numpy()[:B] = [index(name) for name in names]
        self._scene_dev[:B].copy_(pin[:B], non_blocking=True)
        ev = self._scene_ev[k] or torch.cuda.Event()
        ev.record()
        self._scene_ev[k] = ev

    # -- one step -----------------------------------------------------------------------------
    def forward(self, observations: Dict[str, torch.Tensor], T=None, rot=None) -> OccupancySemanticMapMemory:
        """observations: the dict the reference's `Mapper.forward` receives
        (obs_transforms.py:79-103): depth (B,H,W,1) f32, semantic12 (B,H,W,1) u8 (gt) or rgb
        (pred), world_robot_pose (B,3), world_robot_orientation (B,2) f64, not_done_masks (B,1),
        env_name list[str]."""
        self._refuse_open("forward")
        depth = observations["depth"]
        B, H, W = depth.shape[0], depth.shape[1], depth.shape[2]
        if B > self.b_max:
            raise _lib.IvlnError(f"batch {B} > b_max {self.b_max}")
        self._ensure_handle(H, W)
        depth = depth.to(torch.float32).contiguous()
        not_done = observations["not_done_masks"].reshape(-1).to(torch.uint8).contiguous()
        posed = (T is None and self.mode == "iterative" and STEP_POSED) or self.known_library
        if posed:  # (library-mode known steps derive their rotation the same way: ivln_mapper_known_step)
            # the transforms are derived inside the step's first kernel (ivln_mapper_step_posed)
            pose = observations["world_robot_pose"].to(self.device, torch.float32).contiguous()
            orientation = observations["world_robot_orientation"].to(self.device, torch.float64).contiguous()
        elif T is None:
            T, rot, pose = self.frames(observations["world_robot_pose"], observations["world_robot_orientation"])
        else:
            pose = observations["world_robot_pose"].to(self.device, torch.float32).contiguous()
            T = T.to(self.device, torch.float32).contiguous()
            rot = rot.to(self.device, torch.float32).contiguous()
        mem = self.map_memory
        mem.batch_size = B
        s = stream_ptr()
        if self.mode == "iterative":
            if self.semantics_module is not None:
                labels = self.semantics_module(observations)  # (B,1,H,W) or (B,H,W) u8
            else:
                if "semantic12" not in observations or observations["semantic12"] is None:
                    raise Exception("Semantic Sensor not in use")  # mapper.py:660-661
                labels = observations["semantic12"]
            labels = labels.reshape(B, H, W).to(torch.uint8).contiguous()
            if getattr(self, "dry_run", False):
                # a capture's warm-up after the first one (graphed.GraphedRollout(warmup_mapper=False)): everything in front of
                # the mapper has run on this stream - RedNet's workspaces exist now - but the world cloud belongs to the
                # rollout in progress and is not stepped; the maps are whatever the last real step left
                return mem
            if posed:
                check(
                    lib().ivln_mapper_step_posed(
                        self._h, dptr(depth), dptr(labels), dptr(pose), dptr(orientation), dptr(not_done), B,
                        dptr(mem._occ), dptr(mem._sem), dptr(self._T), dptr(self._rot), s,
                    ),
                    "ivln_mapper_step_posed",
                )
            else:
                check(
                    lib().ivln_mapper_step(
                        self._h, dptr(depth), dptr(labels), dptr(T), dptr(pose), dptr(rot), dptr(not_done), B,
                        dptr(mem._occ), dptr(mem._sem), s,
                    ),
                    "ivln_mapper_step",
                )
        elif self.known_library:
            if not torch.cuda.is_current_stream_capturing():  # (a captured step: the runner staged in front of the replay)
                self.stage_host(observations)
            if getattr(self, "dry_run", False):
                return mem
            check(
                lib().ivln_mapper_known_step(self._h, dptr(self._scene_dev), dptr(pose), dptr(orientation), dptr(not_done),
                                             B, dptr(mem._occ), dptr(mem._sem), s),
                "ivln_mapper_known_step",
            )
        else:
            check(lib().ivln_mapper_known_begin(self._h, dptr(not_done), B, s), "ivln_mapper_known_begin")
            finished = (not_done == 0).nonzero().reshape(-1).tolist()
            for b in finished:  # mapper.py:871-879
                xyz, sem = self._load_known(observations["env_name"][b])
                check(
                    lib().ivln_mapper_load_known(self._h, int(b), dptr(xyz), dptr(sem), xyz.shape[0], s),
                    "ivln_mapper_load_known",
                )
            check(
                lib().ivln_mapper_known_raster(self._h, dptr(pose), dptr(rot), B, dptr(mem._occ), dptr(mem._sem), s),
                "ivln_mapper_known_raster",
            )
        return mem

    __call__ = forward

    # -- the same step in two halves (ivln_mapper_step_begin / _finish): `begin` needs depth and pose only, so with predicted
    #    semantics it can be enqueued on another stream beside the network whose labels `finish` waits for ------------------
    def begin(self, observations: Dict[str, torch.Tensor]):
        """Camera transforms, local min / max and the keep-highest arg-max of this step's depth frames (2 launches on the
        current stream).  Iterative mode with the posed entry only; `finish` must follow, ordered behind it."""
        if self.mode != "iterative" or not STEP_POSED:
            raise _lib.IvlnError("MappingModule.begin / finish: iterative mode with the posed step entry only")
        self._refuse_open("begin")
        depth = observations["depth"]
        B, H, W = depth.shape[0], depth.shape[1], depth.shape[2]
        if B > self.b_max:
            raise _lib.IvlnError(f"batch {B} > b_max {self.b_max}")
        self._ensure_handle(H, W)
        self.map_memory.batch_size = B
        if getattr(self, "dry_run", False):
            return
        depth = depth.to(torch.float32).contiguous()
        not_done = observations["not_done_masks"].reshape(-1).to(torch.uint8).contiguous()
        pose = observations["world_robot_pose"].to(self.device, torch.float32).contiguous()
        orientation = observations["world_robot_orientation"].to(self.device, torch.float64).contiguous()
        # (finish reads pose / T / rot through the pointers begin was given: they stay alive on the module)
        self._open = (depth, not_done, pose, orientation)
        check(lib().ivln_mapper_step_begin(self._h, dptr(depth), dptr(pose), dptr(orientation), dptr(not_done), B,
                                           dptr(self.map_memory._occ), dptr(self._T), dptr(self._rot), stream_ptr()),
              "ivln_mapper_step_begin")
        self._begin_open = True  # (behind the call: a begin the handle refused has opened nothing)

    def finish(self, observations: Dict[str, torch.Tensor]) -> OccupancySemanticMapMemory:
        """Labels (gt, or the semantics module's) -> world-cloud merge -> maps (4 launches behind the labels)."""
        mem = self.map_memory
        depth = observations["depth"]
        B, H, W = depth.shape[0], depth.shape[1], depth.shape[2]
        if self.semantics_module is not None:
            labels = self.semantics_module(observations)
        else:
            if "semantic12" not in observations or observations["semantic12"] is None:
                raise Exception("Semantic Sensor not in use")  # mapper.py:660-661
            labels = observations["semantic12"]
        labels = labels.reshape(B, H, W).to(torch.uint8).contiguous()
        from . import rednet as _rednet

        _rednet._stage_done("labels")  # (a capturing GraphedRollout cuts its graph here and waits for `begin`'s event)
        if getattr(self, "dry_run", False):
            return mem
        depth_c, not_done, pose, _ = self._open
        check(lib().ivln_mapper_step_finish(self._h, dptr(depth_c), dptr(labels), dptr(self._T), dptr(pose), dptr(self._rot),
                                            dptr(not_done), B, dptr(mem._occ), dptr(mem._sem), stream_ptr()),
              "ivln_mapper_step_finish")
        self._begin_open = False
        return mem

    def _load_known(self, env_name):
        if env_name not in self._known_cache:
            xyz, sem = load_known_scene(self.maps_location, env_name)
            self._known_cache[env_name] = (torch.from_numpy(xyz).to(self.device), torch.from_numpy(sem).to(self.device))
        return self._known_cache[env_name]

    # -- introspection (tests) -----------------------------------------------------------------
    def status(self):
        n = C.c_int64(0)
        code = lib().ivln_mapper_status(self._h, C.byref(n), stream_ptr())
        if self.known_library:  # the world size the copy path would report: the latched scenes of the current batch rows
            check(lib().ivln_mapper_known_count(self._h, self.map_memory.batch_size, C.byref(n), stream_ptr()),
                  "ivln_mapper_known_count")
        return code, n.value

    def set_launch_width(self, local_blocks: int = 0, world_blocks: int = 0):
        """Workgroups of the local- / world-cloud kernels (0 = full width).  Narrow when the mapper runs beside a
        latency-bound chain on another stream (graphed.py, split replay); results do not depend on it."""
        self._width = (int(local_blocks), int(world_blocks))
        if self._h is not None:
            check(lib().ivln_mapper_set_launch_width(self._h, *self._width), "ivln_mapper_set_launch_width")

    def check_status(self):
        code, n = self.status()
        check(code, "mapper device status")
        return n

    def world_cloud(self):
        """World cloud in the reference's order (ascending key of the last keep-highest):
        xyz (n,3) f32, batch (n,) i32, semantics (n,) u8 - numpy, for parity tests."""
        code, n = self.status()
        xyz = torch.empty((max(n, 1), 3), dtype=torch.float32, device=self.device)
        meta = torch.empty((max(n, 1),), dtype=torch.int32, device=self.device)
        rank = torch.empty((max(n, 1),), dtype=torch.int64, device=self.device)
        nn = C.c_int64(0)
        check(
            lib().ivln_mapper_world_export(self._h, dptr(xyz), dptr(meta), dptr(rank), n, C.byref(nn), stream_ptr()),
            "ivln_mapper_world_export",
        )
        xyz, meta, rank = xyz[:n].cpu().numpy(), meta[:n].cpu().numpy().view(np.uint32), rank[:n].cpu().numpy()
        order = np.argsort(rank, kind="stable")
        return xyz[order], (meta[order] >> 8).astype(np.int32), (meta[order] & 0xFF).astype(np.uint8)

    # -- known-map builder (include/ivln_map_build.h): the explored cloud per row, in the reference's order ---------------
    def _exportable(self, what):
        if self.mode != "iterative":
            raise _lib.IvlnError(f"MappingModule.{what}: iterative mode only (a known-mode cloud is not ordered by key)")
        if self._begin_open:
            raise _lib.IvlnError(f"MappingModule.{what}: `begin` is open - the cloud is defined between complete steps only")
        if self._h is None:
            raise _lib.IvlnError(f"MappingModule.{what}: no step has run yet")

    def env_counts(self) -> np.ndarray:
        """Points of every row's cloud: (b_max,) int64.  One launch + one read-back; synchronises."""
        self._exportable("env_counts")
        counts = (C.c_int64 * self.b_max)()
        check(lib().ivln_mapper_env_counts(self._h, self.b_max, counts, stream_ptr()), "ivln_mapper_env_counts")
        return np.array(counts[:], dtype=np.int64)

    def export_scene(self, b: int):
        """Row b's cloud in the reference's order, ordered and compacted on the device: xyz (n, 3) float32, semantics (n,)
        uint8 - the arrays of a known-map file (`save_known_scene`)."""
        self._exportable("export_scene")
        if not 0 <= int(b) < self.b_max:
            raise _lib.IvlnError(f"row {b} outside [0, {self.b_max})")
        n = int(self.env_counts()[b])
        xyz = torch.empty((max(n, 1), 3), dtype=torch.float32, device=self.device)
        sem = torch.empty((max(n, 1),), dtype=torch.uint8, device=self.device)
        nn = C.c_int64(0)
        check(lib().ivln_mapper_env_export(self._h, int(b), dptr(xyz), dptr(sem), n, C.byref(nn), stream_ptr()),
              "ivln_mapper_env_export")
        return xyz[:n].cpu().numpy(), sem[:n].cpu().numpy()

    # -- seeding (include/ivln_map_seed.h): rows dropped / pre-built points appended between steps; save and restore --------
    def ensure_handle(self, H: int, W: int):
        """Creates the C handle for H x W depth frames if the module has none for that size yet (a step does the same)."""
        self._ensure_handle(int(H), int(W))

    def _seedable(self, what):
        if self.mode != "iterative":
            raise _lib.IvlnError(f"MappingModule.{what}: iterative mode only")
        if self._begin_open:
            raise _lib.IvlnError(f"MappingModule.{what}: `begin` is open - the cloud is defined between complete steps only")
        if self._h is None:
            raise _lib.IvlnError(f"MappingModule.{what}: no handle yet - run a step or call ensure_handle(H, W) first")

    def _c_rows_clear(self, keep, B):
        """The C call (tests replace it with a stub)."""
        check(lib().ivln_mapper_rows_clear(self._h, dptr(keep), int(B), stream_ptr()), "ivln_mapper_rows_clear")

    def _c_append(self, b, xyz, sem):
        """The C call (tests replace it with a stub): xyz (n, 3) f32 and sem (n,) u8, contiguous on the device."""
        check(lib().ivln_mapper_env_append(self._h, int(b), xyz.data_ptr(), sem.data_ptr(), xyz.shape[0], stream_ptr()),
              "ivln_mapper_env_append")

    def _c_append_from_lib(self, b, library, scene):
        check(lib().ivln_mapper_env_append_from_lib(self._h, int(b), library.handle(), int(scene), stream_ptr()),
              "ivln_mapper_env_append_from_lib")

    def clear_rows(self, keep):
        """Drops the cloud of every row b with keep[b] == 0 and of every row >= len(keep) - what a step does with
        `not_done_masks` (mapper.py:310-326), on its own."""
        self._seedable("clear_rows")
        keep = torch.as_tensor(keep).reshape(-1).to(self.device, torch.uint8).contiguous()
        if not 1 <= keep.shape[0] <= self.b_max:
            raise _lib.IvlnError(f"clear_rows: {keep.shape[0]} rows outside [1, {self.b_max}]")
        self._c_rows_clear(keep, keep.shape[0])

    def _row_arrays(self, what, b, xyz, sem):
        if not 0 <= int(b) < self.b_max:
            raise _lib.IvlnError(f"{what}: row {b} outside [0, {self.b_max})")
        xyz = torch.as_tensor(xyz).to(self.device, torch.float32).reshape(-1, 3).contiguous()
        sem = torch.as_tensor(sem).reshape(-1).to(self.device, torch.uint8).contiguous()
        if xyz.shape[0] != sem.shape[0]:
            raise ValueError(f"{what}: {xyz.shape[0]} points but {sem.shape[0]} labels")
        return xyz, sem

    def seed_row(self, b: int, xyz, sem):
        """Appends a pre-built cloud - xyz (n, 3) float32, semantics (n,) uint8, the arrays of a known-map file - to row b:
        behind every point of the cloud, in the given order, in front of the next step's points (mapper.py:871-879)."""
        self._seedable("seed_row")
        xyz, sem = self._row_arrays("seed_row", b, xyz, sem)
        self._c_append(b, xyz, sem)

    def seed_row_from_library(self, b: int, library: KnownSceneLibrary, name: str):
        """`seed_row` with scene `name` of a device-resident library (read from its file on first sight): no host copy."""
        self._seedable("seed_row_from_library")
        if not 0 <= int(b) < self.b_max:
            raise _lib.IvlnError(f"seed_row_from_library: row {b} outside [0, {self.b_max})")
        self._c_append_from_lib(b, library, library.index(name))

    def _geometry(self):
        md = self.map_dimensions
        return {"rows": md.num_rows, "cols": md.num_cols, "resolution_meters": float(md.resolution_meters),
                "frame_size": list(self._hw) if self._hw is not None else None, "b_max": int(self.b_max)}

    def state_dict(self):
        """The mapper's state between two steps: the geometry it was taken with (rows, cols, resolution_meters, frame_size
        [H, W], b_max) and the world cloud in ascending rank - xyz (n, 3) float32, batch (n,) int32, semantics (n,) uint8,
        CPU tensors, so the dict goes through torch.save / torch.load.  Built from ivln_mapper_world_export."""
        self._exportable("state_dict")
        xyz, batch, sem = self.world_cloud()
        sd = self._geometry()
        sd.update(xyz=torch.from_numpy(np.ascontiguousarray(xyz)), batch=torch.from_numpy(np.ascontiguousarray(batch)),
                  semantics=torch.from_numpy(np.ascontiguousarray(sem)))
        return sd

    def load_state_dict(self, sd):
        """Resets the mapper and appends the saved cloud run by run - a run is a stretch of consecutive points of one row
        in rank order (one per row, more only where quirk Q2 interleaves rows).  Appends keep call order, so the restored
        cloud has the saved order exactly and every later step equals the uninterrupted mapper's.  A state taken with
        another map geometry or frame size raises ValueError naming both; nothing is touched then."""
        if self.mode != "iterative":
            raise _lib.IvlnError("MappingModule.load_state_dict: iterative mode only")
        if self._begin_open:
            raise _lib.IvlnError("MappingModule.load_state_dict: `begin` is open")
        mine = self._geometry()
        if mine["frame_size"] is None and self.camera_parameters is not None:
            mine["frame_size"] = [int(v) for v in self.camera_parameters.features_spatial_dimensions]
        theirs = {k: sd[k] for k in ("rows", "cols", "resolution_meters", "frame_size")}
        theirs["frame_size"] = [int(v) for v in theirs["frame_size"]]
        for k, v in theirs.items():
            if mine[k] is not None and mine[k] != v:
                raise ValueError(f"mapper state was taken with {k} = {v}, this mapper has {k} = {mine[k]}")
        xyz, batch, sem = sd["xyz"], torch.as_tensor(sd["batch"]).reshape(-1), sd["semantics"]
        n = int(batch.shape[0])
        if tuple(xyz.shape) != (n, 3) or tuple(sem.shape) != (n,):
            raise ValueError(f"mapper state: xyz {tuple(xyz.shape)}, batch ({n},), semantics {tuple(sem.shape)} do not match")
        if n and not (0 <= int(batch.min()) and int(batch.max()) < self.b_max):
            raise ValueError(f"mapper state holds rows up to {int(batch.max())}, this mapper has b_max = {self.b_max}")
        runs = cloud_runs(batch)
        self._ensure_handle(*theirs["frame_size"])
        self.reset()
        xyz = xyz.to(self.device, torch.float32).contiguous()
        sem = sem.to(self.device, torch.uint8).contiguous()
        for b, lo, hi in runs:
            self._c_append(b, xyz[lo:hi], sem[lo:hi])


def cloud_runs(batch):
    """Stretches of consecutive equal entries of `batch` (n,): [(row, start, stop)], in order."""
    batch = np.asarray(torch.as_tensor(batch).cpu()).reshape(-1)
    if batch.shape[0] == 0:
        return []
    cuts = np.flatnonzero(batch[1:] != batch[:-1]) + 1
    starts = np.concatenate(([0], cuts))
    stops = np.concatenate((cuts, [batch.shape[0]]))
    return [(int(batch[s]), int(s), int(e)) for s, e in zip(starts, stops)]


def create_gt_semantics_iterative_mapper(device, camera_parameters, map_dimensions, **kw) -> MappingModule:
    """mapper.py:991-998."""
    return MappingModule(device, camera_parameters, map_dimensions, mode="iterative", **kw)


def create_predicted_semantics_iterative_mapper(device, camera_parameters, map_dimensions, **kw) -> MappingModule:
    """mapper.py:1001-1008: labels = argmax of RedNet(rgb, depth)."""
    from .rednet import PredictSemantics

    return MappingModule(
        device, camera_parameters, map_dimensions, mode="iterative", semantics_module=PredictSemantics(device), **kw
    )


def create_gt_semantics_known_mapper(device, map_dimensions, **kw) -> MappingModule:
    """mapper.py:1011-1017."""
    return MappingModule(device, None, map_dimensions, mode="known", maps_location="data/known_maps/gt_semantics", **kw)


def create_predicted_semantics_known_mapper(device, map_dimensions, **kw) -> MappingModule:
    """mapper.py:1020-1028."""
    return MappingModule(
        device, None, map_dimensions, mode="known", maps_location="data/known_maps/predicted_semantics", **kw
    )
