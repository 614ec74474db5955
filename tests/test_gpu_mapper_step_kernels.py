"""The iterative mapper's step kernels (csrc/mapper.hip: k_local_minmax<false|true>, k_local_argmax, k_local_select,
k_world_max, k_world_select, k_finalize, and k_frames) alone, through the C ABI, at the smallest shapes that reach their
edges, against the C oracle (oracle/mapper_ref.c through oracle.mapper_ref.MapperRef) stepped with the same T and rot.
Every comparison is bit-exact - occupancy, semantic map, world size, world xyz as uint32, env and label in cloud order,
after every step - and is written to mapper_step_kernels.log in the suite's log directory before anything is asserted.
The oracle is the only reference; the kernels' output is never compared with anything but the oracle's and with a second,
fresh mapper that is stepped through the same inputs and must give the same bytes.

The case tables are plain numpy and live here (CASES, built by case(tag)); tests/test_mapper_step_coverage.py (CPU)
imports them, steps the oracle and its own plain-Python restatement of make_key / table_slot / the launch partitions
through every case, and asserts that each case reaches the edge its tags name.  The table and capacity boundaries used
here (S, K, N) come from that restatement.

Buffers.  This file owns every buffer (ctypes, like tests/test_gpu_gemm_f32_kernels.py).  Every mapper is created with a
small explicit world capacity and table (a few thousand points and slots).  occ_out, sem_out, T_out and rot_out are B_max
rows long between two bands; rows >= B and the bands hold sentinels that must keep their bytes.  Depth, labels, T, pose,
rot, orientation and not_done sit between bands: NaN for the floats, 0xFF for the labels, 1 for not_done (a row read beyond B counts as alive and shows).

Sizes.  Each case runs 2 - 4 steps of at most 64 envs x 4 x 4 or 3 envs x 24 x 20 pixels; the launch-width cases alone use
5 envs of 64 x 64 grid frames, because a source buffer of 256 * 16 points needs that many valid pixels.

Hand-built transforms: rotation entries in {0, +-1} (+-0 in the tie frames) plus a translation, so the fmaf chain of the
unprojection equals the un-fused fp32 arithmetic numpy can restate; pose x / z = T's translation.  The entry-point tests
use transforms derived from (pose, orientation) instead - headings 0, +-pi, pi/2 and 1e-9 - by ivln_mapper_frames,
ivln_mapper_step_posed and ivln_mapper_step_begin / _finish, all held to MapperRef.frames and to the oracle.  The tie
frames of the height cases have no (pose, orientation) form (row 1 of T is zero) and run through ivln_mapper_step only.

Measured on an MI355X: 79 tests, 3612 comparisons (lines of the log), every one equal; the file takes 1.6 s (pytest's
total, mapper creation and both oracle runs included; no test above 0.3 s), tests/test_gpu_mapper.py (27 tests, the
workload's shapes) 1.5 s on the same machine at the parent commit.  No case failed: the step kernels reproduce the oracle
at every edge listed in the CPU companion, and no defect of csrc/mapper.hip was found.  Two things about the tables came
out of the scratch builds below.  not_done's guard bands are 1, not 0: a 0 hides a read beyond row B (a dead env changes
nothing), and the `ne` defect is only seen because of it.  And no case of the first version could tell the `C <= 0` branch
of table_slot from a division by C = 0, because with one column of cells every key is 0 and any function of it is a
bijection - deg-c0-tab1 (a table of ONE slot) was added and can.

Scratch builds with ONE value-only defect each (nothing of them is committed), tests of this file that fail:
  table_slot: `C <= 0` -> `C < 0`                                  0 of 78, then 1 of 79 (deg-c0-tab1, added for it)
  ord_f32: the -0 -> +0 fold dropped                               2 (hts-tie, hts-tie-twice)
  k_world_max: `~rank` -> `rank`                                   72 of 78 (every test whose world meets a second step)
  k_world_select: box init `i < B * 4` -> `i < B * 2`              9 (b64-4x4, both ras-borders, 6 entry-point cases)
  k_local_argmax: `ne` from sc->n_bbox_envs alone                  1 (rag-seq-323: B 3, 2, 3)
  working_blocks: `need < gridDim.x` -> `need <= gridDim.x`        0: the same value for every input, not a defect;
                  the clamp to the grid dropped instead            9 (wid-4096 / -4095 / -4097 at world width 1)
  k_world_select: iters for `blockIdx.x <= nbw`                    3 (width (1, 2): an idle block beside a working one)
  k_local_select: kLocalRankBit dropped from the new ranks         17
  k_local_argmax + _select: the LAST pixel wins a tie              5 (the four tie / ulp cases, deg-1x1)
  k_local_minmax: cmax one cell short                              18
  k_finalize: the last map cell not converted                      73
  k_finalize: n_bbox_envs one short                                5
  raster_point: `fr >= 0` -> `fr > 0` (-0.0 and row 0 refused)     40
  k_frames: sign of rot[2]                                         22 (every entry-point test)
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from kernel_bar import _log

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOG = "mapper_step_kernels.log"
PAD = 16               # elements of guard band on either side of every buffer
SENT_U8, SENT_F = 0xA5, -777.0
RC = {"ok": 0, "keyspace": -3, "capacity": -4}
f32 = np.float32

MAPS = {"m64": (6.4, 6.4, 0.1), "m48": (6.4, 4.8, 0.2)}   # (height_m, width_m, res_m): 64 x 64 and 32 x 24 cells
# camera-to-world rotation (core.py:20-36 at elevation pi, exact trigonometry) and the ego rotation for -heading
HEAD = {
    0: (np.array([[1, 0, 0], [0, -1, 0], [0, 0, -1]], f32), np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], f32)),
    90: (np.array([[0, 0, -1], [0, -1, 0], [-1, 0, 0]], f32), np.array([[0, 0, -1], [0, 1, 0], [1, 0, 0]], f32)),
    180: (np.array([[-1, 0, 0], [0, -1, 0], [0, 0, 1]], f32), np.array([[-1, 0, 0], [0, 1, 0], [0, 0, -1]], f32)),
    270: (np.array([[0, 0, 1], [0, -1, 0], [1, 0, 0]], f32), np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], f32)),
}
HEADINGS = [0.0, np.pi, -np.pi, np.pi / 2, 1e-9]   # of the entry-point tests, env b takes HEADINGS[(b + t) % 5]


# ----------------------------------------------------------------------------------------------------------------------
# case tables (numpy only: the CPU companion imports them)
# ----------------------------------------------------------------------------------------------------------------------
def _seed(tag):
    s = 29
    for ch in tag:
        s = (s * 131 + ord(ch)) % (2 ** 31)
    return s


def _T(head, t, row1=None):
    T = np.zeros((4, 4), f32)
    T[:3, :3] = HEAD[head][0]
    T[:3, 3] = t
    T[3, 3] = 1
    if row1 is not None:
        T[1] = row1
    return T


def _depth(rng, B, H, W, lo=0.05, hi=0.6, holes=True):
    d = rng.uniform(lo, hi, (B, H, W)).astype(f32)
    if holes and H * W >= 16:   # values the depth filter drops, each on its side of the cut, and a NaN
        k = rng.randint(0, H * W, (B, 4))
        for b in range(B):
            for j, v in enumerate([0.0, 0.995, 0.01, float("nan")]):
                d[b].reshape(-1)[k[b, j]] = v
    return d


def _step(depth, labels, trans, heads, pose_y=None, nd=None, t=0, row1=None, width=None):
    """one step of B = len(depth) envs: env b looks along heading heads[b] from trans[b]; pose = the translation (pose_y
    replaces its height: the filter windows move, the cloud does not)"""
    B = depth.shape[0]
    trans = np.asarray(trans, f32).reshape(B, 3)
    pose = trans.copy()
    if pose_y is not None:
        pose[:, 1] = pose_y
    T = np.stack([_T(heads[b], trans[b], None if row1 is None else row1[b]) for b in range(B)])
    rot = np.stack([HEAD[heads[b]][1] for b in range(B)])
    orient = np.zeros((B, 2), np.float64)
    for b in range(B):
        orient[b, 1] = HEADINGS[(b + t) % len(HEADINGS)]
    return dict(B=B, depth=np.ascontiguousarray(depth, f32), labels=np.ascontiguousarray(labels, np.uint8), T=T, pose=pose,
                rot=rot, not_done=np.ones(B, np.uint8) if nd is None else np.asarray(nd, np.uint8), orient=orient, width=width)


def _walk(tag, H, W, Bs, heads=None, y=1.25, spread=0.35, move=0.15, nds=None, lab0=False, widths=None):
    """len(Bs) steps of seeded frames: env b starts spread * b apart along x and z and moves `move` per step, so that
    every step's cloud overlaps the world the steps before left"""
    rng = np.random.RandomState(_seed(tag))
    steps = []
    for t, B in enumerate(Bs):
        d = _depth(rng, B, H, W)
        lab = np.zeros((B, H, W), np.uint8) if lab0 else rng.randint(0, 13, (B, H, W)).astype(np.uint8)
        tr = [(spread * b + move * t, y, -spread * b * 0.5 + move * 0.5 * t) for b in range(B)]
        hd = [(heads[b % len(heads)] if heads else 0) for b in range(B)]
        steps.append(_step(d, lab, tr, hd, nd=None if nds is None else nds[t], t=t, width=None if widths is None else widths[t]))
    return steps


def _deg_r0_1x20(tag):   # one image row: y = 0, every point of a constant-depth frame in ONE row of cells (R = 0)
    rng = np.random.RandomState(_seed(tag))
    lab = lambda B: rng.randint(1, 13, (B, 1, 20)).astype(np.uint8)   # noqa: E731
    s0 = _step(np.full((2, 1, 20), 0.2, f32), lab(2), [(0, 1.25, 0), (0.2, 1.35, 0)], [0, 0])
    s1 = _step(_depth(rng, 2, 1, 20), lab(2), [(0.1, 1.25, 0), (0.3, 1.35, 0.1)], [0, 0], t=1)
    s2 = _step(np.full((2, 1, 20), 0.2, f32), lab(2), [(0, 1.25, 0), (0.2, 1.35, 0)], [0, 0], t=2)
    return steps_case(1, 20, 2, 4.5, [s0, s1, s2], ("R0_local", "R0_world", "collide"))


def _deg_c0_tab1(tag):
    """every step one column of cells, in the local and in the world pass: every key is 0 and a table of ONE slot holds it
    (the slot of a one-column box is the key itself: nothing may be divided by C or rounded up to a tile)"""
    rng = np.random.RandomState(_seed(tag))
    d0 = np.linspace(0.1, 0.4, 16, dtype=f32).reshape(2, 8, 1)
    steps = [_step(d, rng.randint(1, 13, (2, 8, 1)).astype(np.uint8), [(0, 1.25, 0), (0, 1.25, 0)], [0, 0], t=t)
             for t, d in enumerate([d0, d0[::-1].copy(), d0 * f32(1.5)])]
    return steps_case(8, 1, 2, 60.0, steps, ("C0_always",), table=1)


def _deg_c0_8x1(tag):    # one image column: x = 0, every point in ONE column of cells (C = 0), every key 0
    rng = np.random.RandomState(_seed(tag))
    lab = lambda: rng.randint(1, 13, (2, 8, 1)).astype(np.uint8)   # noqa: E731
    d0 = np.linspace(0.1, 0.4, 16, dtype=f32).reshape(2, 8, 1)
    s0 = _step(d0, lab(), [(0, 1.25, 0), (0, 1.25, 0)], [0, 0])
    s1 = _step(_depth(rng, 2, 8, 1, holes=False), lab(), [(0, 1.25, 0.1), (0.1, 1.25, 0)], [0, 90], t=1)   # env 1 turns: 2-D
    s2 = _step(d0[::-1].copy(), lab(), [(0, 1.25, 0), (0, 1.25, 0)], [0, 0], t=2)   # one column again: the world pass has C = 0 too
    return steps_case(8, 1, 2, 60.0, [s0, s2, s1, s0], ("C0_local", "C0_world", "collide"))


def _deg_1x1(tag):       # one pixel per env: the limit case
    rng = np.random.RandomState(_seed(tag))
    lab = lambda: rng.randint(1, 13, (3, 1, 1)).astype(np.uint8)   # noqa: E731
    s0 = _step(np.array([0.2, 0.3, 0.4], f32).reshape(3, 1, 1), lab(), [(0, 1.25, 0)] * 3, [0, 0, 0])
    s1 = _step(np.array([0.25, 0.3, 0.35], f32).reshape(3, 1, 1), lab(), [(0, 1.25, 0), (0.4, 1.3, 0), (0.2, 1.2, 0.3)], [0, 90, 180], t=1)
    s2 = _step(np.array([0.2, 0.2, 0.2], f32).reshape(3, 1, 1), lab(), [(0, 1.25, 0)] * 3, [0, 0, 0], t=2)
    return steps_case(1, 1, 3, 60.0, [s0, s1, s2], ("C0_local", "R0_local", "collide"))


def _deg_r0_24x20(tag):  # constant depth: 24 image rows in one row of cells, the envs' keys collide
    rng = np.random.RandomState(_seed(tag))
    lab = lambda: rng.randint(0, 13, (3, 24, 20)).astype(np.uint8)   # noqa: E731
    tr = [(0, 1.25, 0), (0.2, 1.3, 0), (-0.15, 1.2, 0)]
    s0 = _step(np.full((3, 24, 20), 0.2, f32), lab(), tr, [0, 0, 0])
    s1 = _step(_depth(rng, 3, 24, 20), lab(), tr, [0, 0, 0], t=1)
    s2 = _step(np.full((3, 24, 20), 0.2, f32), lab(), tr, [0, 0, 0], t=2)
    return steps_case(24, 20, 3, 90.0, [s0, s1, s2], ("R0_local", "R0_world", "collide"))


def _hts_tie(tag, twice):
    """row 1 of T zeroed: every height is exactly zero, +0 in env 0; in env 1 (row 1 = (0, 0, -0, -0)) -0 where x and y
    are negative and +0 elsewhere.  Depth constant within each column: all 8 image rows of a column share one cell, so
    every cell is an 8-way exact tie (in env 1's left half between -0 and +0) that the first pixel must win."""
    rng = np.random.RandomState(_seed(tag))
    H, W = 8, 12
    d = np.broadcast_to(f32(0.1) + f32(0.03) * np.arange(W, dtype=f32), (2, H, W)).copy()
    row1 = [np.array([0, 0, 0, 0], f32), np.array([0, 0, -0.0, -0.0], f32)]
    tr = [(0, 0, 0), (0.5, 0, 0.2)]
    mk = lambda t: _step(d, rng.randint(1, 13, (2, H, W)).astype(np.uint8), tr, [0, 0], pose_y=0.0, t=t, row1=row1)   # noqa: E731
    steps = [mk(0), mk(1), mk(2)] if twice else [mk(0), _step(_depth(rng, 2, H, W), rng.randint(1, 13, (2, H, W)).astype(np.uint8),
                                                              tr, [0, 0], pose_y=0.0, t=1)]
    return steps_case(H, W, 2, 60.0, steps, ("tie_local", "neg_zero") + (("tie_world",) if twice else ()), posed=False)


def _hts_ulp(tag, up):
    """every height of a step is one constant (row 1 of T = (0, 0, 0, c)): -0.25, then its fp32 neighbour above (every new
    point wins its cell) or below (every old point keeps it), then -0.25 again"""
    rng = np.random.RandomState(_seed(tag))
    H, W = 6, 10
    d = np.broadcast_to(f32(0.1) + f32(0.04) * np.arange(W, dtype=f32), (2, H, W)).copy()
    c0 = f32(-0.25)
    c1 = np.nextafter(c0, f32(0.0 if up else -1.0))
    tr = [(0, 0, 0), (0.5, 0, 0.2)]
    steps = []
    for t, c in enumerate([c0, c1, c0]):
        row1 = [np.array([0, 0, 0, c], f32)] * 2
        steps.append(_step(d, rng.randint(1, 13, (2, H, W)).astype(np.uint8), tr, [0, 0], pose_y=0.0, t=t, row1=row1))
    return steps_case(H, W, 2, 60.0, steps, ("negative", "tie_local", "ulp_up" if up else "ulp_down"), posed=False)


def grid_frame(k):
    """a 64 x 64 frame whose first k pixels of a 16 x 64 grid are valid: 16 image rows around the horizon, one depth per
    row 6 cm apart, 64 columns >= 6.25 cm apart at 2 m - each keeps its own 5 cm cell (the frame of
    tests/test_gpu_known_build.py::_grid_frame, restated so that importing this file needs no other GPU test file)"""
    d = np.zeros((64, 64), f32)
    n = 0
    for i in range(16):
        for j in range(64):
            if n < k:
                d[24 + i, j] = 0.2 + 0.006 * i
                n += 1
    return d


def _wid(tag, n0, n1=None):
    """world-cloud kernels at a source-buffer size of exactly n0 points (and n0 + n1 in the second step): grid frames, the
    envs 8 m apart along z so that no two share a key"""
    rng = np.random.RandomState(_seed(tag))
    B = 5
    per = [min(1024, max(0, n0 - 1024 * b)) for b in range(B)]
    tr = [(0, 1.25, 8.0 * b) for b in range(B)]
    lab = lambda: rng.randint(1, 13, (B, 64, 64)).astype(np.uint8)   # noqa: E731
    d0 = np.stack([grid_frame(k) for k in per])
    steps = [_step(d0, lab(), tr, [0] * B)]
    d1 = d0 if n1 is None else np.stack([grid_frame(k) for k in [min(1024, max(0, n1 - 1024 * b)) for b in range(B)]])
    steps.append(_step(d1, lab(), tr, [0] * B, t=1))
    return steps_case(64, 64, B, 90.0, steps, ("n_src",), posed=False, cap=3 * 4096)


def _ras_borders(tag, mp):
    """one pixel per env (x = y = 0 in the image, z = 0.5 m), placed by its translation; pose x = z = 0 and the ego rotation
    is the identity, so the raster sees the world coordinates themselves.  Rows / columns: the last fp32 value that still
    rounds inside and the first that rounds outside, at both borders (the CPU companion derives them: raster_border).
    Then a point at exactly -half (cell 0) and +half (one past the last cell) of either axis.
    Heights: step 0 puts a point at y = 0.5 in each of 7 envs; step 1 has no valid pixel and moves pose y so that the point
    sits at h - 1.25, h + 0.75 and their fp32 neighbours."""
    import test_mapper_step_coverage as P

    hm, wm, res = MAPS[mp]
    rng = np.random.RandomState(_seed(tag))
    pts = []   # (x, z) of the raster-border envs; every env has its own row AND column of cells
    for i, (zin, zout) in enumerate([P.raster_border(hm, res, False), P.raster_border(hm, res, True)]):
        pts += [(f32(-1.0 + 0.5 * i), zin), (f32(-0.7 + 0.5 * i), zout)]
    for i, (xin, xout) in enumerate([P.raster_border(wm, res, False), P.raster_border(wm, res, True)]):
        pts += [(xin, f32(-1.1 + 0.6 * i)), (xout, f32(-0.8 + 0.6 * i))]
    half = [(f32(1.3), f32(-hm / 2)), (f32(1.6), f32(hm / 2)), (f32(-wm / 2), f32(1.7)), (f32(wm / 2), f32(2.0))]   # exactly +-half
    pts += half
    hts = [(f32(0.3 * j - 0.9), f32(0.37 * j - 1.3)) for j in range(7)]
    B = len(pts) + len(hts)
    tr = [(x, 1.25, f32(z) + f32(0.5)) for x, z in pts] + [(x, 0.5, f32(z) + f32(0.5)) for x, z in hts]   # (exact sums)
    pose_y0 = np.array([1.25] * len(pts) + [0.5] * len(hts), f32)
    lab = lambda: rng.randint(1, 13, (B, 1, 1)).astype(np.uint8)   # noqa: E731
    s0 = _step(np.full((B, 1, 1), 0.05, f32), lab(), tr, [0] * B, pose_y=pose_y0)
    s0["pose"][:, [0, 2]] = 0
    h_lo, h_hi = f32(1.75), f32(-0.25)   # 1.75 - 1.25 = 0.5 = -0.25 + 0.75
    h_in = h_hi                          # the first h above -0.25 whose fp32 sum h + 0.75 exceeds 0.5 (the sum is coarser than h:
    while h_in + f32(0.75) <= f32(0.5):  # the neighbours in between still round to 0.5 and keep the point out)
        h_in = np.nextafter(h_in, f32(9))
    pose_y1 = np.array([1.25] * len(pts) + [h_lo, np.nextafter(h_lo, f32(0)), np.nextafter(h_lo, f32(9)),
                                            h_hi, np.nextafter(h_hi, f32(0)), h_in, np.nextafter(h_hi, f32(-9))], f32)
    s1 = _step(np.zeros((B, 1, 1), f32), lab(), tr, [0] * B, pose_y=pose_y1, t=1)
    s1["pose"][:, [0, 2]] = 0
    return steps_case(1, 1, B, 60.0, [s0, s1], ("raster_border", "height_window"), posed=False, mp=mp)


def steps_case(H, W, B_max, vfov_deg, steps, edges, posed=True, mp="m64", cap=4096, table=1 << 19):
    hfov_deg = vfov_deg * W / H                          # the oracle derives vfov as hfov * H / W:
    vfov_rad = float(np.deg2rad(hfov_deg * (H / W)))     # the mapper is given that very double
    return types.SimpleNamespace(H=H, W=W, B_max=B_max, hfov_deg=hfov_deg, vfov_rad=vfov_rad, map=MAPS[mp], steps=steps,
                                 edges=tuple(edges), posed=posed, cap=cap, table=table,
                                 rows=int(np.ceil(MAPS[mp][0] / MAPS[mp][2])), cols=int(np.ceil(MAPS[mp][1] / MAPS[mp][2])))


def _b_many(tag, B, B_max):   # 4 x 4 frames, one env per 0.1 m: k_world_select's box[] and the 64 transforms in LDS
    rng = np.random.RandomState(_seed(tag))
    steps = []
    for t in range(2):
        tr = [(0.1 * (b % 8) + 0.05 * t, 1.25, 0.1 * (b // 8)) for b in range(B)]
        steps.append(_step(_depth(rng, B, 4, 4, 0.05, 0.15), rng.randint(0, 13, (B, 4, 4)).astype(np.uint8), tr,
                           [(0, 90, 180, 270)[b % 4] for b in range(B)], t=t))
    return steps_case(4, 4, B_max, 90.0, steps, ("all_envs",) + (("rows_ge_B",) if B < B_max else ()))


def _tab(tag, k):   # the far env one more 5 cm cell to the right per k: C of the world pass takes every residue mod 4
    rng = np.random.RandomState(_seed("tab"))
    steps = []
    for t in range(3):
        tr = [(0.1 * t, 1.25, 0), (0.6, 1.25, 0.3 + 0.1 * t), (1.2 + 0.05 * k, 1.25, -0.25)]
        steps.append(_step(_depth(rng, 3, 24, 20), rng.randint(0, 13, (3, 24, 20)).astype(np.uint8), tr, [0, 90, 0], t=t))
    return steps_case(24, 20, 3, 90.0, steps, ("S_gt_K",))


CASES = {
    # 1. degenerate boxes, each followed by a step with ordinary depth
    "deg-r0-1x20": _deg_r0_1x20,
    "deg-c0-8x1": _deg_c0_8x1,
    "deg-c0-tab1": _deg_c0_tab1,
    "deg-1x1": _deg_1x1,
    "deg-r0-24x20": _deg_r0_24x20,
    # 2. ragged pixel counts, B against B_max
    "rag-24x20-b3of5": lambda tag: steps_case(24, 20, 5, 90.0, _walk(tag, 24, 20, [3, 3, 3], heads=[0, 90, 180]), ("ragged", "rows_ge_B")),
    "rag-5x13-b3of5": lambda tag: steps_case(5, 13, 5, 40.0, _walk(tag, 5, 13, [3, 3, 3], heads=[0, 270]), ("rows_ge_B",)),
    "rag-seq-323": lambda tag: steps_case(24, 20, 3, 90.0, _walk(tag, 24, 20, [3, 2, 3, 3], heads=[0, 0, 90]), ("ragged", "rows_ge_B", "paused")),
    "rag-seq-15": lambda tag: steps_case(5, 13, 5, 40.0, _walk(tag, 5, 13, [1, 5, 5], heads=[0, 90]), ("rows_ge_B",)),
    "b64-4x4": lambda tag: _b_many(tag, 64, 64),
    "b33-4x4": lambda tag: _b_many(tag, 33, 40),
    # 3. heights
    "hts-signs": lambda tag: steps_case(24, 20, 3, 90.0, _walk(tag, 24, 20, [3, 3, 3], heads=[0, 180, 90], y=0.0), ("both_signs", "negative")),
    "hts-tie": lambda tag: _hts_tie(tag, False),
    "hts-tie-twice": lambda tag: _hts_tie(tag, True),
    "hts-ulp-up": lambda tag: _hts_ulp(tag, True),
    "hts-ulp-down": lambda tag: _hts_ulp(tag, False),
    # 4. table boundaries
    "tab-0": lambda tag: _tab(tag, 0), "tab-1": lambda tag: _tab(tag, 1), "tab-2": lambda tag: _tab(tag, 2), "tab-3": lambda tag: _tab(tag, 3),
    # 5. capacity (no env resets or pauses: the source buffer holds what the oracle's cloud holds)
    "cap": lambda tag: steps_case(24, 20, 3, 90.0, _walk(tag, 24, 20, [3, 3, 3], heads=[0, 90, 0]), ("capacity",)),
    # 6. launch widths: source-buffer sizes around 256 * 16
    "wid-0": lambda tag: _wid(tag, 0, 0), "wid-4096": lambda tag: _wid(tag, 4096),
    "wid-4095": lambda tag: _wid(tag, 4095, 2), "wid-4097": lambda tag: _wid(tag, 4097, 4095),
    "wid-switch": lambda tag: steps_case(24, 20, 3, 90.0, _walk(tag, 24, 20, [3, 3, 3, 3], heads=[0, 90], widths=[(0, 0), (0, 0), (1, 1), (1, 1)]),
                                         ("ragged", "width_switch")),
    # 7. raster edges
    "ras-borders-m48": lambda tag: _ras_borders(tag, "m48"),
    "ras-borders-m64": lambda tag: _ras_borders(tag, "m64"),
    "ras-label0": lambda tag: steps_case(24, 20, 3, 90.0, _walk(tag, 24, 20, [3, 3], lab0=True), ("label0",), mp="m48"),
    "ras-two-labels": lambda tag: steps_case(24, 20, 3, 90.0, _walk(tag, 24, 20, [3, 3, 3, 3], heads=[0, 90, 180],
                                                                    nds=[[1, 1, 1], [1, 1, 1], [1, 0, 1], [1, 1, 1]]),
                                             ("two_labels", "reset"), mp="m48"),
}
WIDTHS = [(1, 1), (2, 1), (0, 1), (1, 0), (1, 2)]     # (local_blocks, world_blocks); (1, 2): an idle block beside a narrow launch
WIDTH_CASES = ["wid-0", "wid-4096", "wid-4095", "wid-4097", "rag-24x20-b3of5"]
ENTRY_CASES = [t for t in CASES if t.startswith(("rag-", "b64", "b33", "hts-signs"))]   # cases 2 and 3 with a (pose, orientation) form
ENTRIES = ["frames", "posed", "split"]
TAB_CASES = ["tab-0", "tab-1", "tab-2", "tab-3"]


@functools.lru_cache(maxsize=None)
def case(tag):
    c = CASES[tag](tag)
    c.tag = tag
    return c


# ----------------------------------------------------------------------------------------------------------------------
# the oracle, stepped once per (case, transforms) and shared
# ----------------------------------------------------------------------------------------------------------------------
def step_transforms(s, posed):
    """(T, rot) of a step: hand-built, or derived from (pose, orientation) by the oracle's frames"""
    from oracle.mapper_ref import MapperRef

    return MapperRef.frames(s["pose"], s["orient"]) if posed else (s["T"], s["rot"])


@functools.lru_cache(maxsize=None)
def oracle_run(tag, posed=False, first=0):
    """per step from `first` on, on a fresh oracle: occupancy, semantic map, world (xyz, env, label), T, rot.  Read-only."""
    from oracle.mapper_ref import MapperRef

    c = case(tag)
    ref = MapperRef(c.H, c.W, c.hfov_deg, *c.map)
    out = []
    for s in c.steps[first:]:
        T, rot = step_transforms(s, posed)
        occ, sem = ref.step(s["depth"], s["labels"], s["pose"], None, s["not_done"], T=T, rot=rot)
        xyz, b, lab = ref.world()
        r = dict(occ=occ, sem=sem, xyz=xyz, b=b, lab=lab, T=np.ascontiguousarray(T, f32), rot=np.ascontiguousarray(rot, f32))
        for v in r.values():
            v.setflags(write=False)
        out.append(r)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the mapper through its C ABI
# ----------------------------------------------------------------------------------------------------------------------
def _banded(a, fill):
    """a (numpy) on the device between two bands of PAD elements of `fill` -> (tensor, pointer to the payload)"""
    a = np.ascontiguousarray(a).reshape(-1)
    t = torch.full((a.size + 2 * PAD,), fill, dtype=torch.from_numpy(a[:0].copy()).dtype, device=DEV)
    t[PAD:PAD + a.size] = torch.from_numpy(a.copy()).to(DEV)
    return t, t.data_ptr() + PAD * t.element_size()


def _out(n, fill, dtype):
    t = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=DEV)
    return t, t.data_ptr() + PAD * t.element_size()


class _Hip:
    def __init__(self, c, cap=None, table=None, width=None):
        from ivln_ce_amd._lib import lib, stream_ptr

        self.c, self.L, self.s = c, lib(), stream_ptr()
        self.h = C.c_void_p()
        rc = self.L.ivln_mapper_create(c.B_max, c.H, c.W, c.vfov_rad, *c.map, cap or c.cap, table or c.table, C.byref(self.h))
        assert rc == 0, f"ivln_mapper_create: {rc}"
        self.width = None
        if width is not None:
            self.set_width(width)

    def set_width(self, width):
        if width != self.width:
            assert self.L.ivln_mapper_set_launch_width(self.h, *width) == 0
            self.width = width

    def close(self):
        if self.h:
            torch.cuda.synchronize()
            self.L.ivln_mapper_destroy(self.h)
            self.h = None

    def reset(self):
        assert self.L.ivln_mapper_reset(self.h, self.s) == 0

    def status(self):
        n = C.c_int64(-1)
        return self.L.ivln_mapper_status(self.h, C.byref(n), self.s), n.value

    def world(self, n):
        """the cloud in ascending rank (the reference's order): xyz as uint32 (n, 3), env, label"""
        xyz, px = _out(3 * max(n, 1), float("nan"), torch.float32)
        meta, pm = _out(max(n, 1), -1, torch.int32)
        rank, pr = _out(max(n, 1), -1, torch.int64)
        nn = C.c_int64(-1)
        assert self.L.ivln_mapper_world_export(self.h, px, pm, pr, n, C.byref(nn), self.s) == 0 and nn.value == n
        torch.cuda.synchronize()
        xyz = xyz[PAD:PAD + 3 * n].cpu().numpy().view(np.uint32).reshape(n, 3)
        meta = meta[PAD:PAD + n].cpu().numpy().view(np.uint32)
        order = np.argsort(rank[PAD:PAD + n].cpu().numpy(), kind="stable")
        return xyz[order], (meta[order] >> 8).astype(np.int32), (meta[order] & 0xFF).astype(np.uint8)

    def buffers(self, s):
        """the step's inputs between their bands and B_max rows of sentinel-filled outputs (alive as long as the result is)"""
        c = self.c
        cells = c.rows * c.cols
        keep = [_banded(s["depth"], float("nan")), _banded(s["labels"], 0xFF), _banded(s["pose"], float("nan")),
                _banded(s["not_done"], 1), _banded(s["T"], float("nan")), _banded(s["rot"], float("nan")),
                _banded(s["orient"], float("nan"))]
        (_, dep), (_, lab), (_, pose), (_, nd), (_, T), (_, rot), (_, ori) = keep
        occ, pocc = _out(c.B_max * cells, SENT_U8, torch.uint8)
        sem, psem = _out(c.B_max * cells, SENT_U8, torch.uint8)
        To, pT = _out(c.B_max * 16, SENT_F, torch.float32)
        ro, pr = _out(c.B_max * 9, SENT_F, torch.float32)
        return types.SimpleNamespace(keep=keep, B=s["B"], dep=dep, lab=lab, pose=pose, nd=nd, T=T, rot=rot, ori=ori, occ=occ,
                                     pocc=pocc, sem=sem, psem=psem, To=To, pT=pT, ro=ro, pr=pr)

    def begin(self, q):
        return self.L.ivln_mapper_step_begin(self.h, q.dep, q.pose, q.ori, q.nd, q.B, q.pocc, q.pT, q.pr, self.s)

    def finish(self, q):
        return self.L.ivln_mapper_step_finish(self.h, q.dep, q.lab, q.pT, q.pose, q.pr, q.nd, q.B, q.pocc, q.psem, self.s)

    def call(self, q, entry):
        """the return code of one step on the buffers q through `entry`"""
        L, B = self.L, q.B
        if entry == "step":
            return L.ivln_mapper_step(self.h, q.dep, q.lab, q.T, q.pose, q.rot, q.nd, B, q.pocc, q.psem, self.s)
        if entry == "frames":
            rc = L.ivln_mapper_frames(q.pose, q.ori, B, q.pT, q.pr, self.s)
            return rc or L.ivln_mapper_step(self.h, q.dep, q.lab, q.pT, q.pose, q.pr, q.nd, B, q.pocc, q.psem, self.s)
        if entry == "posed":
            return L.ivln_mapper_step_posed(self.h, q.dep, q.lab, q.pose, q.ori, q.nd, B, q.pocc, q.psem, q.pT, q.pr, self.s)
        return self.begin(q) or self.finish(q)

    def result(self, q, entry, rows=None):
        """the bytes a step left in q: occ, sem (B rows), T_out, rot_out (posed entries), the guard check.  rows: the rows
        that may have been written (default B; 0: every output must be sentinels still)"""
        c, B = self.c, q.B if rows is None else rows
        cells = c.rows * c.cols
        torch.cuda.synchronize()
        occ, sem, To, ro = q.occ.cpu().numpy(), q.sem.cpu().numpy(), q.To.cpu().numpy(), q.ro.cpu().numpy()
        guards = True
        for a, n, sent in [(occ, B * cells, SENT_U8), (sem, B * cells, SENT_U8),
                           (To, B * 16 if entry != "step" else 0, f32(SENT_F)), (ro, B * 9 if entry != "step" else 0, f32(SENT_F))]:
            guards &= bool((a[:PAD] == sent).all() and (a[PAD + n:] == sent).all())   # the bands and the rows >= B
        return dict(occ=occ[PAD:PAD + B * cells].reshape(B, c.rows, c.cols), sem=sem[PAD:PAD + B * cells].reshape(B, c.rows, c.cols),
                    T=To[PAD:PAD + B * 16].view(np.uint32), rot=ro[PAD:PAD + B * 9].view(np.uint32), guards=guards)

    def step(self, s, entry="step"):
        """one step through `entry` -> the bytes it left: occ, sem (B rows), T_out, rot_out (posed entries), the guard check"""
        if s["width"] is not None:
            self.set_width(s["width"])
        q = self.buffers(s)
        rc = self.call(q, entry)
        assert rc == 0, f"{entry}: return code {rc}"
        return self.result(q, entry)


class _Cmp:
    """every comparison is a line of the log before it is an assertion"""
    count = 0

    def __init__(self, what):
        self.what, self.bad = what, []

    def eq(self, t, name, got, ref):
        got, ref = np.asarray(got), np.asarray(ref)
        same = got.shape == ref.shape and got.dtype == ref.dtype and bool(np.array_equal(got, ref))
        nd = "shape" if got.shape != ref.shape else int((got != ref).sum())
        line = f"{self.what:44s} step {t} {name:10s} {'equal' if same else 'DIFF'} ({nd} of {ref.size} differ)"
        _log(line, LOG)
        _Cmp.count += 1
        if not same:
            self.bad.append(line)

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def _run(tag, entry="step", width=None, cap=None, table=None, first=0, mappers=None):
    """the case's steps on two fresh mappers; after every step both are held to the oracle and to each other"""
    c = case(tag)
    posed = entry != "step"
    ref = oracle_run(tag, posed, first)
    own = mappers is None
    ms = mappers or [_Hip(c, cap, table, width), _Hip(c, cap, table, width)]
    cmp = _Cmp(f"{tag} {entry} w{width} cap{cap} tab{table}")
    try:
        for t, s in enumerate(c.steps[first:]):
            outs = []
            for m in ms:
                o = m.step(s, entry)
                code, n = m.status()
                o["n"], o["code"] = n, code
                o["xyz"], o["b"], o["lab"] = m.world(n) if code == 0 and 0 <= n <= (cap or c.cap) else (None, None, None)
                outs.append(o)
            r, o = ref[t], outs[0]
            cmp.eq(t, "status", o["code"], 0)
            cmp.eq(t, "guards", o["guards"], True)
            cmp.eq(t, "world_n", o["n"], r["xyz"].shape[0])
            cmp.eq(t, "occ", o["occ"], r["occ"])
            cmp.eq(t, "sem", o["sem"], r["sem"])
            if o["xyz"] is not None:
                cmp.eq(t, "world_xyz", o["xyz"], r["xyz"].view(np.uint32))
                cmp.eq(t, "world_env", o["b"], r["b"])
                cmp.eq(t, "world_label", o["lab"], r["lab"])
            if posed:
                cmp.eq(t, "T_out", o["T"], r["T"].reshape(-1).view(np.uint32))
                cmp.eq(t, "rot_out", o["rot"], r["rot"].reshape(-1).view(np.uint32))
            for k in ["code", "guards", "n", "occ", "sem", "xyz", "b", "lab", "T", "rot"]:
                if o[k] is not None and outs[1][k] is not None:
                    cmp.eq(t, "2nd:" + k, outs[1][k], o[k])
            cmp.done()
    finally:
        if own:
            for m in ms:
                m.close()


# ----------------------------------------------------------------------------------------------------------------------
# tests
# ----------------------------------------------------------------------------------------------------------------------
def test_return_codes_are_the_headers():
    import os
    import re

    import test_mapper_step_coverage as P

    hdr = open(os.path.join(P.ROOT, "include", "ivln_hip.h")).read()
    for name, code in RC.items():
        assert int(re.search(r"#define IVLN_(?:E_)?%s\s+(-?\d+)" % name.upper(), hdr).group(1)) == code


@pytest.mark.parametrize("tag", [t for t in CASES if t.startswith("deg-")])
def test_degenerate_boxes(tag):
    _run(tag)


@pytest.mark.parametrize("tag", [t for t in CASES if t.startswith(("rag-", "b64", "b33"))])
def test_ragged_pixels_and_batch_against_b_max(tag):
    _run(tag)


@pytest.mark.parametrize("tag", [t for t in CASES if t.startswith("hts-")])
def test_heights_signs_and_ties(tag):
    _run(tag)


@pytest.mark.parametrize("tag", TAB_CASES)
def test_table_of_exactly_the_highest_slot(tag):
    import test_mapper_step_coverage as P

    S, K = P.table_bounds(tag)
    assert S > K
    _run(tag, table=S + 1)


@pytest.mark.parametrize("tag", TAB_CASES)
def test_table_one_slot_short_is_keyspace(tag):
    """every KEY fits a table of S cells (S > K), the highest SLOT does not: the launcher's status is IVLN_E_KEYSPACE"""
    import test_mapper_step_coverage as P

    S, K = P.table_bounds(tag)
    c = case(tag)
    for _ in range(2):
        m = _Hip(c, table=S)
        try:
            for s in c.steps:
                m.step(s)
            code, _n = m.status()
            _log(f"{tag:44s} table {S} (highest slot {S}, highest key {K}) status {code}", LOG)
            assert code == RC["keyspace"]
        finally:
            m.close()


def test_capacity_of_exactly_the_peak():
    import test_mapper_step_coverage as P

    N, _t = P.capacity_peak("cap")
    _run("cap", cap=N)


def test_capacity_one_short_is_reported_and_reset_recovers():
    """capacity N - 1: the step of the peak returns, the status is IVLN_E_CAPACITY with the count clamped to the capacity;
    after ivln_mapper_reset the same mapper steps the case's first frame again and equals a fresh oracle"""
    import test_mapper_step_coverage as P

    N, t_peak = P.capacity_peak("cap")
    c = case("cap")
    ms = [_Hip(c, cap=N - 1), _Hip(c, cap=N - 1)]
    try:
        for m in ms:
            for t, s in enumerate(c.steps[:t_peak + 1]):
                m.step(s)
                code, n = m.status()
                _log(f"{'cap':44s} capacity {N - 1} step {t} status {code} world_n {n}", LOG)
                assert code == (RC["capacity"] if t == t_peak else 0) and 0 <= n <= N - 1
            m.reset()
            assert m.status() == (0, 0)
        cmp = _Cmp("cap after reset")
        r, s = oracle_run("cap")[0], c.steps[0]
        for i, m in enumerate(ms):
            o = m.step(s)
            code, n = m.status()
            cmp.eq(0, f"{i}:status", code, 0)
            cmp.eq(0, f"{i}:world_n", n, r["xyz"].shape[0])
            cmp.eq(0, f"{i}:occ", o["occ"], r["occ"])
            cmp.eq(0, f"{i}:sem", o["sem"], r["sem"])
            cmp.eq(0, f"{i}:guards", o["guards"], True)
            if code == 0 and n == r["xyz"].shape[0]:
                xyz, b, lab = m.world(n)
                cmp.eq(0, f"{i}:world_xyz", xyz, r["xyz"].view(np.uint32))
                cmp.eq(0, f"{i}:world_env", b, r["b"])
                cmp.eq(0, f"{i}:world_label", lab, r["lab"])
        cmp.done()
    finally:
        for m in ms:
            m.close()


@pytest.mark.parametrize("width", WIDTHS, ids=lambda w: f"{w[0]}x{w[1]}")
@pytest.mark.parametrize("tag", WIDTH_CASES)
def test_launch_widths(tag, width):
    _run(tag, width=width)


def test_launch_width_changed_between_steps():
    _run("wid-switch")


@pytest.mark.parametrize("tag", [t for t in CASES if t.startswith("ras-")])
def test_raster_edges(tag):
    _run(tag)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("tag", ENTRY_CASES)
def test_entry_points(tag, entry):
    """transforms from (pose, orientation): ivln_mapper_frames + ivln_mapper_step, ivln_mapper_step_posed,
    ivln_mapper_step_begin + _finish - each equals the oracle stepped with MapperRef.frames (T_out and rot_out equal
    those frames), so the three equal each other bit for bit"""
    _run(tag, entry=entry)


def test_entry_points_interleaved_on_one_mapper():
    """one mapper, another entry point every step: nothing but the kernels' own state links two steps"""
    c = case("rag-seq-323")
    ref = oracle_run("rag-seq-323", True)
    cmp = _Cmp("rag-seq-323 interleaved")
    m = _Hip(c)
    try:
        for t, s in enumerate(c.steps):
            o = m.step(s, ENTRIES[t % 3])
            code, n = m.status()
            cmp.eq(t, "status", code, 0)
            cmp.eq(t, "world_n", n, ref[t]["xyz"].shape[0])
            cmp.eq(t, "occ", o["occ"], ref[t]["occ"])
            cmp.eq(t, "sem", o["sem"], ref[t]["sem"])
            cmp.eq(t, "T_out", o["T"], ref[t]["T"].reshape(-1).view(np.uint32))
            cmp.eq(t, "rot_out", o["rot"], ref[t]["rot"].reshape(-1).view(np.uint32))
            cmp.done()
    finally:
        m.close()


# kernel of csrc/mapper.hip's step (and k_frames) -> a test of this file that runs it against the oracle
KERNEL_COVERED = {
    "k_local_minmax": "test_entry_points",                 # <false>: every other test; <true>: the posed and split entries
    "k_local_argmax": "test_degenerate_boxes",
    "k_local_select": "test_heights_signs_and_ties",
    "k_world_max": "test_heights_signs_and_ties",
    "k_world_select": "test_ragged_pixels_and_batch_against_b_max",
    "k_finalize": "test_raster_edges",
    "k_frames": "test_entry_points",
}
