"""Box-world: a room with axis-aligned boxes whose depth, labels and colour are ray-cast from the pose by the inverse of the
mapper's un-projection (include/ivln_boxworld.h defines the arithmetic; csrc/boxworld.hip is the device renderer).

  make_scene(seed, cfg, ...)   a seeded scene from the BOXWORLD config node
  render_reference(...)        the numpy restatement of the header, operation for operation: in float32 it equals the
                               kernel bit for bit (the oracle of its test) and is the CPU path of the backend; in float64
                               it is the reference the float32 recipe is judged against
  BoxWorldRenderer(device)     scene table + frame buffers on the device, one render call per env step

Conventions (the mapper's, core.py:70-171 with mapper.py:133-136): heading h about +y, at h = 0 the camera looks along -z;
right = (cos h, 0, -sin h), down = (0, -1, 0), forward = (-sin h, 0, -cos h); the ray parameter t is the z-depth."""
import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

MAX_BOXES = 32  # IVLN_BW_MAX_BOXES

# rows 0..12: the label colours; row 13: the second colour of the label-0 checker (csrc/boxworld.hip kPalette / kShade)
PALETTE = np.array([
    [200, 200, 200], [230, 25, 75], [60, 180, 75], [255, 225, 25], [0, 130, 200], [245, 130, 48], [145, 30, 180],
    [70, 240, 240], [240, 50, 230], [210, 245, 60], [250, 190, 190], [0, 128, 128], [170, 110, 40], [120, 120, 120],
], np.uint8)
SHADE = np.array([200, 232, 120, 255, 168, 216], np.int32)  # faces -x, +x, -y, +y, -z, +z
CHECKER_M = 0.5


@dataclass
class Scene:
    room: np.ndarray    # (6,) float32: lo xyz, hi xyz
    boxes: np.ndarray   # (n, 6) float32
    labels: np.ndarray  # (n,) uint8, 1..12

    def __post_init__(self):
        self.room = np.ascontiguousarray(self.room, np.float32).reshape(6)
        self.boxes = np.ascontiguousarray(self.boxes, np.float32).reshape(-1, 6)
        self.labels = np.ascontiguousarray(self.labels, np.uint8).reshape(-1)
        if len(self.boxes) != len(self.labels) or len(self.boxes) > MAX_BOXES:
            raise ValueError(f"a scene has one label per box and at most {MAX_BOXES} boxes")

    # -- collision: the agent is a disc of `radius` in the x-z plane ---------------------------------------------
    def blocked(self, pos, radius):
        """True when a disc centre `pos` (x, y, z) is outside the room or inside a box footprint grown by `radius`."""
        x, z = float(pos[0]), float(pos[2])
        lo, hi = self.room[:3], self.room[3:]
        if not (lo[0] <= x <= hi[0] and lo[2] <= z <= hi[2]):
            return True
        b = self.boxes
        if len(b) == 0:
            return False
        r = float(radius)
        return bool(np.any((x > b[:, 0] - r) & (x < b[:, 3] + r) & (z > b[:, 2] - r) & (z < b[:, 5] + r)))


def make_scene(seed, cfg, origin=(0.0, 0.0, 0.0), starts=()):
    """A seeded scene from `cfg.BOXWORLD`: a room of ROOM_SIZE (x, y, z) metres scaled per axis by up to +-ROOM_JITTER
    (x and z only; the floor is y = 0) around `origin`, which lies ROOM_ORIGIN_Z of the way from the room's +z wall (the
    agent starts looking along -z), and NUM_BOXES boxes on the floor with sizes between BOX_MIN_SIZE and BOX_MAX_SIZE and
    labels 1..12.  A box whose footprint, grown by START_CLEARANCE, covers one of `starts` is left out."""
    bw = cfg.BOXWORLD
    rng = np.random.RandomState(int(seed))
    size = np.array(bw.ROOM_SIZE, np.float64)
    jit = float(bw.ROOM_JITTER)
    ex, ez = size[0] * (1.0 + rng.uniform(-jit, jit)), size[2] * (1.0 + rng.uniform(-jit, jit))
    fz = float(bw.ROOM_ORIGIN_Z)
    ox, _, oz = (float(v) for v in origin)
    room = np.array([ox - ex / 2, 0.0, oz - (1.0 - fz) * ez, ox + ex / 2, size[1], oz + fz * ez], np.float32)
    n = int(bw.NUM_BOXES)
    if not 0 <= n <= MAX_BOXES:
        raise ValueError(f"BOXWORLD.NUM_BOXES must be in [0, {MAX_BOXES}]")
    smin, smax = np.array(bw.BOX_MIN_SIZE, np.float64), np.array(bw.BOX_MAX_SIZE, np.float64)
    smax = np.minimum(smax, [ex / 2, size[1], ez / 2])
    clear = float(bw.START_CLEARANCE)
    boxes, labels = [], []
    for _ in range(n):
        s = rng.uniform(smin, np.maximum(smin, smax))
        cx = rng.uniform(room[0], room[3] - s[0])
        cz = rng.uniform(room[2], room[5] - s[2])
        label = int(rng.randint(1, 13))
        box = np.array([cx, 0.0, cz, cx + s[0], s[1], cz + s[2]], np.float32)
        if any(box[0] - clear < p[0] < box[3] + clear and box[2] - clear < p[2] < box[5] + clear for p in starts):
            continue
        if not np.all(box[:3] < box[3:]):
            continue
        boxes.append(box)
        labels.append(label)
    return Scene(room, np.array(boxes, np.float32).reshape(-1, 6), np.array(labels, np.uint8))


def surface_distance(scene, points, labels):
    """Distance in metres (float64) of every world point to the nearest surface that carries its label: for a label
    L > 0 the surfaces of the scene's boxes of label L, for label 0 the room shell; inf where the scene has no such
    surface.  What a cloud built from this scene's frames is checked with (tests, tools/build_known_maps.py output)."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    labels = np.asarray(labels).reshape(-1)
    out = np.full(len(p), np.inf)

    def to_box_surface(q, lo, hi):
        outside = np.linalg.norm(np.maximum(np.maximum(lo - q, q - hi), 0.0), axis=1)
        inside = np.minimum(q - lo, hi - q).min(axis=1)  # (depth below the nearest face; only read where outside == 0)
        return np.where(outside > 0, outside, np.maximum(inside, 0.0))

    room = scene.room.astype(np.float64)
    m = labels == 0
    if m.any():
        out[m] = to_box_surface(p[m], room[:3], room[3:])
    for k in range(len(scene.boxes)):
        m = labels == scene.labels[k]
        if m.any():
            b = scene.boxes[k].astype(np.float64)
            out[m] = np.minimum(out[m], to_box_surface(p[m], b[:3], b[3:]))
    return out


def unproject(depth, cam_pos, heading, fx, fy, dmin, dmax):
    """World points (H, W, 3) float64 of a depth frame (H, W) by the camera model above, the mapper's convention:
    z = dmin + depth * (dmax - dmin), p = o + z * (xs * right + ys * down + forward)."""
    depth = np.asarray(depth, np.float64)
    H, W = depth.shape
    xs = (np.arange(W) + 0.5 - W / 2.0) / float(fx)
    ys = (np.arange(H) + 0.5 - H / 2.0) / float(fy)
    s, c = math.sin(float(heading)), math.cos(float(heading))
    z = float(dmin) + depth * (float(dmax) - float(dmin))
    o = np.asarray(cam_pos, np.float64).reshape(3)
    x, y = z * xs[None, :], z * ys[:, None]
    return np.stack([o[0] + x * c - z * s, o[1] - y, o[2] - x * s - z * c], axis=-1)


def intrinsics(H, W, hfov_rad):
    """(fx, fy) in double: vfov = hfov * H / W, fx = W / (2 tan(hfov / 2)), fy = H / (2 tan(vfov / 2))."""
    vfov = float(hfov_rad) * H / W
    return W / (2.0 * math.tan(float(hfov_rad) / 2.0)), H / (2.0 * math.tan(vfov / 2.0))


def render_reference(scene, cam_pos, heading, H, W, fx, fy, dmin, dmax, dtype=np.float32, with_rgb=True):
    """One frame by the recipe of include/ivln_boxworld.h in `dtype` arithmetic.  `heading` is the angle (its sine and
    cosine are taken in double and rounded once to `dtype`) or a (sin, cos) pair.  Returns a dict: depth (H, W) dtype,
    labels (H, W) uint8, face (H, W) uint8, t (H, W) dtype and, with_rgb, rgb (H, W, 3) uint8."""
    F = np.dtype(dtype).type
    if np.ndim(heading) == 0:
        s, c = F(math.sin(float(heading))), F(math.cos(float(heading)))
    else:
        s, c = F(heading[0]), F(heading[1])
    o = [F(v) for v in np.asarray(cam_pos, np.float32 if F is np.float32 else np.float64).reshape(3)]
    fx, fy, dmin, dmax = F(fx), F(fy), F(dmin), F(dmax)
    room = scene.room.astype(dtype)
    xs = ((np.arange(W).astype(dtype) + F(0.5)) - F(W / 2.0)) / fx
    ys = ((np.arange(H).astype(dtype) + F(0.5)) - F(H / 2.0)) / fy
    shape = (H, W)
    d = [np.broadcast_to((xs * c - s)[None, :], shape), np.broadcast_to((-ys)[:, None], shape),
         np.broadcast_to((-(xs * s) - c)[None, :], shape)]
    best = np.full(shape, np.inf, dtype)
    label = np.zeros(shape, np.uint8)
    face = np.zeros(shape, np.uint8)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for a in range(3):
            pos = d[a] > 0
            t = (np.where(pos, room[3 + a], room[a]) - o[a]) / d[a]
            upd = (d[a] != 0) & (t < best)
            best = np.where(upd, t, best)
            face = np.where(upd, (2 * a + pos).astype(np.uint8), face)
        for k in range(len(scene.boxes)):
            bx = scene.boxes[k].astype(dtype)
            tn = np.full(shape, -np.inf, dtype)
            tf = np.full(shape, np.inf, dtype)
            fk = np.zeros(shape, np.uint8)
            miss = np.zeros(shape, bool)
            for a in range(3):
                par = d[a] == 0
                if o[a] < bx[a] or o[a] > bx[3 + a]:
                    miss = miss | par
                t1 = (bx[a] - o[a]) / d[a]
                t2 = (bx[3 + a] - o[a]) / d[a]
                lt = t1 < t2
                ta, tb = np.where(lt, t1, t2), np.where(lt, t2, t1)
                up = ~par & (ta > tn)
                tn = np.where(up, ta, tn)
                fk = np.where(up, (2 * a + (d[a] < 0)).astype(np.uint8), fk)
                tf = np.where(~par & (tb < tf), tb, tf)
            hit = ~miss & (tn > 0) & (tn <= tf) & (tn < best)
            best = np.where(hit, tn, best)
            label = np.where(hit, scene.labels[k], label).astype(np.uint8)
            face = np.where(hit, fk, face)
        z = (best - dmin) / (dmax - dmin)
        z = np.where(z > 0, z, F(0))
        z = np.where(z < 1, z, F(1))
        out = {"depth": z.astype(dtype), "labels": label, "face": face, "t": best}
        if with_rgb:
            p = [o[a] + best * d[a] for a in range(3)]
            ax = face >> 1
            pi = np.where(ax == 0, p[1], p[0])
            pj = np.where(ax == 2, p[1], p[2])
            q = np.floor(pi / F(CHECKER_M)) + np.floor(pj / F(CHECKER_M))
            odd = (q - F(2) * np.floor(q * F(0.5))) != 0
            row = np.where(label != 0, label, np.where(odd, 13, 0)).astype(np.int64)
            out["rgb"] = ((PALETTE[row].astype(np.int32) * SHADE[face][..., None]) >> 8).astype(np.uint8)
    return out


class BoxWorldRenderer:
    """The device side of the backend: the scene table (a scene is uploaded once), two sets of frame buffers used in turn
    by `render` - the views handed out by one call stay valid through the next one - plus two sets of per-row buffers for
    `render_row` (an episode reset of one env between two steps), and a pinned staging block `scene_index | cam_pos |
    sincos` that reaches the device in ONE asynchronous copy per call.  Launches go to torch's current stream."""

    def __init__(self, device, b_max, depth_hw, hfov_rad, dmin, dmax, rgb_hw=None, rgb_hfov_rad=None, max_scenes=None):
        import torch

        from . import _lib

        if torch.device(device).type != "cuda":
            raise _lib.IvlnError("BoxWorldRenderer needs a GPU device (the CPU path is boxworld.render_reference)")
        self.torch, self._lib = torch, _lib
        self.device = torch.device(device)
        self.b_max = int(b_max)
        self.H, self.W = (int(v) for v in depth_hw)
        self.rgb_hw = tuple(int(v) for v in rgb_hw) if rgb_hw else None
        fx, fy = intrinsics(self.H, self.W, hfov_rad)
        self.fx, self.fy = np.float32(fx), np.float32(fy)
        self.fxr = self.fyr = np.float32(0)
        if self.rgb_hw:
            fxr, fyr = intrinsics(*self.rgb_hw, hfov_rad if rgb_hfov_rad is None else rgb_hfov_rad)
            self.fxr, self.fyr = np.float32(fxr), np.float32(fyr)
        self.dmin, self.dmax = np.float32(dmin), np.float32(dmax)
        L = _lib.lib()
        self._sig(L)
        self._L = L
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(L.ivln_boxworld_create(int(max_scenes or max(self.b_max, 1)), C.byref(self._h)), "ivln_boxworld_create")
        self._n_scenes = 0
        Bm = self.b_max

        def frames():
            f = {"depth": torch.empty((Bm, self.H, self.W, 1), dtype=torch.float32, device=self.device),
                 "labels": torch.empty((Bm, self.H, self.W, 1), dtype=torch.uint8, device=self.device)}
            if self.rgb_hw:
                f["rgb"] = torch.empty((Bm, *self.rgb_hw, 3), dtype=torch.uint8, device=self.device)
            return f

        self._sets = [frames(), frames()]      # whole-batch renders, used in turn
        self._row_sets = [frames(), frames()]  # single-row renders, used in turn per row
        self._turn = 0
        self._row_turn = [0] * Bm
        # staging: 6 words per row (index i32 | pos 3 x f32 | sin, cos f32); pinned blocks used in turn like
        # MappingModule.stage_host's - one is rewritten only after the copy that read it has run
        self._pin = [torch.zeros((6 * Bm,), dtype=torch.int32).pin_memory() for _ in range(4)]
        self._pin_ev = [None] * 4
        self._pin_turn = 0
        self._stage = [torch.zeros((6 * Bm,), dtype=torch.int32, device=self.device) for _ in range(2)]
        self._stage_turn = 0

    @staticmethod
    def _sig(L):
        vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
        L.ivln_boxworld_create.argtypes = [i32, C.POINTER(vp)]
        L.ivln_boxworld_destroy.argtypes = [vp]
        L.ivln_boxworld_add_scene.argtypes = [vp, i32, vp, i32, vp, vp, vp]
        L.ivln_boxworld_size.argtypes = [vp]
        L.ivln_boxworld_render.argtypes = [vp, vp, vp, vp, i32, i32, i32, f32, f32, f32, f32, vp, vp, i32, i32, f32, f32,
                                           vp, vp]
        L.ivln_boxworld_status.argtypes = [vp, i32, vp]

    def __del__(self):
        try:
            if self._h:
                self._L.ivln_boxworld_destroy(self._h)
                self._h = None
        except Exception:  # noqa: BLE001
            pass

    def add_scene(self, scene):
        """Uploads `scene`; returns its index in the table."""
        i = self._n_scenes
        boxes, labels = scene.boxes, scene.labels
        self._lib.check(
            self._L.ivln_boxworld_add_scene(self._h, i, scene.room.ctypes.data, len(boxes),
                                            boxes.ctypes.data if len(boxes) else None,
                                            labels.ctypes.data if len(boxes) else None, self._lib.stream_ptr()),
            "ivln_boxworld_add_scene")
        self._n_scenes += 1
        return i

    def _stage_rows(self, scene_index, cam_pos, headings):
        torch = self.torch
        B = len(scene_index)
        if not 1 <= B <= self.b_max:
            raise self._lib.IvlnError(f"batch {B} outside [1, {self.b_max}]")
        k = self._pin_turn
        self._pin_turn = (k + 1) % len(self._pin)
        if self._pin_ev[k] is not None:
            self._pin_ev[k].synchronize()
        words = self._pin[k].numpy()
        Bm = self.b_max
        words[:B] = scene_index
        fl = words.view(np.float32)
        fl[Bm:Bm + 3 * B] = np.asarray(cam_pos, np.float32).reshape(-1)
        h = np.asarray(headings, np.float64).reshape(-1)
        sc = fl[4 * Bm:4 * Bm + 2 * B].reshape(B, 2)
        sc[:, 0] = [math.sin(v) for v in h]  # (libm in double, as render_reference; rounded once to float32 here)
        sc[:, 1] = [math.cos(v) for v in h]
        dev = self._stage[self._stage_turn]
        self._stage_turn ^= 1
        dev.copy_(self._pin[k], non_blocking=True)
        ev = self._pin_ev[k] or torch.cuda.Event()
        ev.record()
        self._pin_ev[k] = ev
        return dev

    def _launch(self, dev, B, frames, row, with_rgb):
        Bm = self.b_max
        rgb = frames.get("rgb") if with_rgb else None
        Hr, Wr = self.rgb_hw if rgb is not None else (0, 0)
        p = dev.data_ptr()
        self._lib.check(
            self._L.ivln_boxworld_render(
                self._h, p, p + 4 * Bm, p + 16 * Bm, B, self.H, self.W, self.fx, self.fy, self.dmin, self.dmax,
                frames["depth"][row:].data_ptr(), frames["labels"][row:].data_ptr(), Hr, Wr, self.fxr, self.fyr,
                rgb[row:].data_ptr() if rgb is not None else None, self._lib.stream_ptr()),
            "ivln_boxworld_render")

    def render(self, scene_index, cam_pos, headings, with_rgb=True):
        """All rows in one call: scene_index (B,), cam_pos (B, 3), headings (B,) -> {depth (B, H, W, 1) f32, labels
        (B, H, W, 1) u8, rgb (B, Hr, Wr, 3) u8}: views of this turn's buffers, valid through the next `render`."""
        B = len(scene_index)
        dev = self._stage_rows(scene_index, cam_pos, headings)
        frames = self._sets[self._turn]
        self._turn ^= 1
        with_rgb = with_rgb and self.rgb_hw is not None
        self._launch(dev, B, frames, 0, with_rgb)
        return {k: v[:B] for k, v in frames.items() if k != "rgb" or with_rgb}

    def render_row(self, row, scene_index, cam_pos, heading, with_rgb=True):
        """One row (an episode reset between two steps) into that row's own buffers, so that the other rows' views of the
        last `render` stay what they are: {depth (H, W, 1), labels (H, W, 1), rgb (Hr, Wr, 3)}."""
        if not 0 <= row < self.b_max:
            raise self._lib.IvlnError(f"row {row} outside [0, {self.b_max})")
        dev = self._stage_rows([scene_index], [cam_pos], [heading])
        frames = self._row_sets[self._row_turn[row]]
        self._row_turn[row] ^= 1
        with_rgb = with_rgb and self.rgb_hw is not None
        self._launch(dev, 1, frames, row, with_rgb)
        return {k: v[row] for k, v in frames.items() if k != "rgb" or with_rgb}

    def check_status(self):
        """Synchronises; raises if a render met a scene index without a table entry."""
        self._lib.check(self._L.ivln_boxworld_status(self._h, 0, self._lib.stream_ptr()), "box-world device status")
