"""CPU companion of tests/test_gpu_mapper_step_kernels.py: the index arithmetic of the mapper's step (csrc/mapper.hip) restated
in plain Python / numpy - make_key, table_slot, the chunk and grid partition of the local-cloud kernels, working_blocks and
k_world_select's iters, the cell of a point under the hand-built {0, +-1} transforms - and a model of one step built from
them.  The model is first held to the C oracle (same world cloud, to the bit, after every step of every case); then every
case of the GPU file's tables is asserted to reach the edge its tags name, and not to be degenerate by accident.  The GPU
file takes S, K (highest slot, highest key) and N (peak source-buffer size) from here."""
import functools
import os
import re

import numpy as np
import pytest

import test_gpu_mapper_step_kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
THREADS, PPT, WORLD_BLOCKS = 256, 4, 1024   # kThreads, kPPT, kWorldBlocks


# ----------------------------------------------------------------------------------------------------------------------
# restatements
# ----------------------------------------------------------------------------------------------------------------------
def make_key(b, r, c, mm):
    """mm = (rmin, cmin, rmax, cmax); the multipliers are max - min, not + 1 (mapper.py:469)"""
    R, Cc = mm[2] - mm[0], mm[3] - mm[1]
    return b * (R * Cc) + (r - mm[0]) * Cc + (c - mm[1])


def table_slot(key, Cc, table_cells):
    """slot of a key: the (key / C, key % C) plane tiled 4 x 4; -1 outside the table"""
    if key < 0 or key >= table_cells:
        return -1
    if Cc <= 0:
        return key
    q, kc = key // Cc, key % Cc
    Ct = (Cc + 3) >> 2
    slot = ((((q >> 2) * Ct) + (kc >> 2)) << 4) | ((q & 3) << 2) | (kc & 3)
    return slot if slot < table_cells else -1


def local_grid(npix, local_blocks):
    """(blocks, chunks each block walks): chunks of 256 * 4 pixels, block i takes chunks i, i + blocks, ..."""
    nchunks = (npix + THREADS * PPT - 1) // (THREADS * PPT)
    lb = local_blocks if 0 < local_blocks < nchunks else nchunks
    return lb, [len(range(i, nchunks, lb)) for i in range(lb)], nchunks * THREADS * PPT - npix


def world_grid(world_blocks):
    """(grid, points per thread) of the world-cloud kernels"""
    return (world_blocks if 0 < world_blocks < WORLD_BLOCKS else WORLD_BLOCKS), (16 if world_blocks > 0 else 1)


def working_blocks(n, wpt, grid):
    per = THREADS * (wpt if wpt > 0 else 1)
    need = (n + per - 1) // per
    return 1 if need < 1 else min(need, grid)


def iters(n, nbw, blk):
    return (n + nbw * THREADS - 1) // (nbw * THREADS) if blk < nbw else 0


def scales(H, W, vfov_rad):
    """x_scale[W], y_scale[H] (core.py:70-115): intrinsics in doubles -> fp32, (u + 0.5 - cx) / fx in fp32"""
    hfov = W / H * vfov_rad
    fx, fy = f32(W / (2.0 * np.tan(hfov / 2.0))), f32(H / (2.0 * np.tan(vfov_rad / 2.0)))
    cx, cy = f32(W / 2.0), f32(H / 2.0)
    return ((np.arange(W, dtype=f32) + f32(0.5)) - cx) / fx, ((np.arange(H, dtype=f32) + f32(0.5)) - cy) / fy


def cells(v, half_res):
    return np.rint(v / f32(half_res)).astype(np.int64)


def local_points(c, s):
    """the filtered local cloud of a step in pixel order: (b, x, y, z, label) - rotation entries in {0, +-1}, so every product
    of the fmaf chain is exact and ((t0 * x + t1 * y) + t2 * z) + t3 rounds where the chain rounds"""
    xs, ys = scales(c.H, c.W, c.vfov_rad)
    d = s["depth"]
    B = s["B"]
    ok = (d > f32(0.01)) & (d < f32(0.99))
    with np.errstate(invalid="ignore"):
        z = d * f32(10.0)
        x, y = z * xs[None, None, :], z * ys[None, :, None]
        T = s["T"]
        w = []
        for r in range(3):
            t = [T[:, r, k].reshape(B, 1, 1) for k in range(4)]
            assert set(np.unique(np.abs(T[:, r, :3]))) <= {0.0, 1.0}
            w.append((((t[0] * x + t[1] * y) + t[2] * z) + t[3]) - f32(0.0))
        h = s["pose"][:, 1].reshape(B, 1, 1)
        ok &= (w[1] > h - f32(1.0)) & (w[1] < h + f32(0.5))
    b = np.broadcast_to(np.arange(B).reshape(B, 1, 1), d.shape)
    return b[ok].astype(np.int64), w[0][ok], w[1][ok], w[2][ok], s["labels"][ok]


def keep_highest(b, x, y, z, half_res):
    """mapper.py:428-474 on a cloud in order -> (indices kept, in ascending key; what the pass saw)"""
    n = len(b)
    if n == 0:
        return np.zeros(0, np.int64), dict(n=0, R=None, C=None, K=-1, keys=np.zeros(0, np.int64), ties=0, pairs=0, mm=None)
    r, cc = cells(z, half_res), cells(x, half_res)
    mm = (int(r.min()), int(cc.min()), int(r.max()), int(cc.max()))
    keys = make_key(b, r, cc, mm)
    order = np.lexsort((np.arange(n), keys))       # by key, then by place in the cloud
    ks, ys = keys[order], y[order]
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    gid = np.cumsum(np.r_[True, ks[1:] != ks[:-1]]) - 1
    ismax = ys == np.maximum.reduceat(ys, starts)[gid]          # (-0 == +0, like the reference's `>`)
    first = np.minimum.reduceat(np.where(ismax, np.arange(n), n), starts)   # the first maximum wins
    keep, ties = order[first], int((np.add.reduceat(ismax.astype(np.int64), starts) > 1).sum())
    pairs = len(set(zip(b.tolist(), r.tolist(), cc.tolist())))
    return keep.astype(np.int64), dict(n=n, R=mm[2] - mm[0], C=mm[3] - mm[1], K=int(keys.max()), keys=keys, ties=ties,
                                          pairs=pairs, mm=mm)


@functools.lru_cache(maxsize=None)
def model_run(tag):
    """every step of the case through the model -> per step: the two passes' diagnostics, the world, n_src (points in the
    kernels' source buffer in front of the world pass: the whole old cloud, dead envs included, + the local survivors)"""
    c = K.case(tag)
    half_res = f32(c.map[2] / 2)
    W = [np.zeros(0, np.int64)] + [np.zeros(0, f32)] * 3 + [np.zeros(0, np.uint8)]
    out = []
    for s in c.steps:
        n_old_all = len(W[0])
        alive = (W[0] < s["B"]) & (s["not_done"][np.minimum(W[0], s["B"] - 1)] != 0)
        W = [a[alive] for a in W]
        P = local_points(c, s)
        kl, dl = keep_highest(P[0], P[1], P[2], P[3], half_res)
        P = [a[kl] for a in P]
        n_old = len(W[0])
        W = [np.concatenate([a, p]) for a, p in zip(W, P)]
        kw, dw = keep_highest(W[0], W[1], W[2], W[3], half_res)
        dw["n_old"], dw["kept_old"] = n_old, int((kw < n_old).sum())
        W = [a[kw] for a in W]
        out.append(dict(local=dl, world=dw, W=[a.copy() for a in W], n_src=n_old_all + len(kl), nl=len(kl), n_alive=n_old))
    return out


def table_slots(keys, Cc, table_cells):
    """table_slot over an array of keys"""
    keys = np.asarray(keys, np.int64)
    if Cc <= 0:
        slot = keys.copy()
    else:
        q, kc = keys // Cc, keys % Cc
        slot = ((((q >> 2) * ((Cc + 3) >> 2)) + (kc >> 2)) << 4) | ((q & 3) << 2) | (kc & 3)
    return np.where((keys < 0) | (keys >= table_cells) | (slot >= table_cells), -1, slot)


def slots_of(d, table_cells=1 << 40):
    return table_slots(d["keys"], d["C"], table_cells)


def table_bounds(tag):
    """(S, K): the highest slot and the highest key over the local and world passes of every step"""
    S = Kmax = -1
    for st in model_run(tag):
        for d in (st["local"], st["world"]):
            if d["n"]:
                S, Kmax = max(S, int(slots_of(d).max())), max(Kmax, d["K"])
    return S, Kmax


def capacity_peak(tag):
    """(N, step): the most points the source buffer holds in one step in front of the world keep-highest (the oracle's
    nworld + nl), and the first step that reaches it"""
    ns = [st["n_src"] for st in model_run(tag)]
    return max(ns), ns.index(max(ns))


def raster_cell(v, half, res):
    """rintf((v + half) / res) as a float (-0.0 passes the kernels' >= 0 test)"""
    return np.rint((f32(v) + f32(half)) / f32(res))


def raster_border(size_m, res_m, far):
    """(last fp32 coordinate that rounds inside the map, first that rounds outside) at the near / far border of an axis of
    size_m metres: adjacent fp32 values around the .5-cell position"""
    half, res = f32(size_m / 2), f32(res_m)
    n = int(np.ceil(size_m / res_m))
    edge, inside, step_out = ((n - 0.5) * res_m - size_m / 2, n - 1, f32(9)) if far else (-0.5 * res_m - size_m / 2, 0, f32(-9))
    v = f32(edge)
    for _ in range(64):   # walk to the inside of the border, then out again
        if raster_cell(v, half, res) == inside:
            break
        v = np.nextafter(v, -step_out)
    for _ in range(256):
        nxt = np.nextafter(v, step_out)
        if raster_cell(nxt, half, res) != inside:
            return v, nxt
        v = nxt
    raise AssertionError("no border found")


# ----------------------------------------------------------------------------------------------------------------------
# the model is the oracle, to the bit
# ----------------------------------------------------------------------------------------------------------------------
ALL = list(K.CASES)


@pytest.mark.parametrize("tag", ALL)
def test_model_equals_oracle_and_case_is_not_degenerate(tag):
    c = K.case(tag)
    ref, mod = K.oracle_run(tag), model_run(tag)
    assert len(ref) == len(mod) == len(c.steps) and 2 <= len(c.steps) <= 4
    assert max(s["B"] for s in c.steps) * c.H * c.W <= max(64 * 4 * 4, 3 * 24 * 20) or tag.startswith("wid-")   # (grid frames: 64 x 64)
    for t, (r, m) in enumerate(zip(ref, mod)):
        assert np.array_equal(m["W"][1].view(np.uint32), r["xyz"][:, 0].view(np.uint32)), (tag, t)
        assert np.array_equal(m["W"][2].view(np.uint32), r["xyz"][:, 1].view(np.uint32)), (tag, t)
        assert np.array_equal(m["W"][3].view(np.uint32), r["xyz"][:, 2].view(np.uint32)), (tag, t)
        assert np.array_equal(m["W"][0], r["b"]) and np.array_equal(m["W"][4], r["lab"]), (tag, t)
    if tag != "wid-0":
        assert ref[-1]["xyz"].shape[0] > 0 and max(int(r["occ"].sum()) for r in ref) > 0, tag
    else:
        assert all(r["xyz"].shape[0] == 0 and int(r["occ"].sum()) == 0 for r in ref)
    # the defaults of the case fit: no key or point is refused
    S, Kmax = table_bounds(tag)
    assert max(S, Kmax) < c.table and capacity_peak(tag)[0] <= c.cap


@pytest.mark.parametrize("tag", ALL)
def test_slot_is_a_bijection_of_the_keys_on_every_box(tag):
    c = K.case(tag)
    for st in model_run(tag):
        for d in (st["local"], st["world"]):
            if not d["n"]:
                continue
            R, Cc = d["R"], d["C"]
            top = (max(s["B"] for s in c.steps) - 1) * R * Cc + R * Cc + Cc   # the highest key the box allows
            sl = table_slots(np.arange(top + 1), Cc, 1 << 40)
            assert len(np.unique(sl)) == top + 1 and sl.min() >= 0
            assert sl.max() >= top   # (slots only ever spread the keys out)
            cut = table_slots(np.arange(top + 1), Cc, top + 1)
            assert ((cut == -1) | (cut == sl)).all() and ((cut == -1) == (sl > top)).all()
            for k in {0, 1, Cc, top // 2, top - 1, top} & set(range(top + 1)):   # the array form is the scalar restatement
                assert table_slot(k, Cc, 1 << 40) == sl[k] and table_slot(k, Cc, top + 1) == cut[k]


# ----------------------------------------------------------------------------------------------------------------------
# each case reaches the edge its tag names
# ----------------------------------------------------------------------------------------------------------------------
def _with(edge):
    return [t for t in ALL if edge in K.case(t).edges]


EDGES = sorted({e for t in ALL for e in K.case(t).edges})


def test_every_edge_has_a_check_here():
    known = {"R0_local", "R0_world", "C0_local", "C0_world", "collide", "ragged", "rows_ge_B", "paused", "all_envs", "both_signs",
             "negative", "tie_local", "tie_world", "neg_zero", "ulp_up", "ulp_down", "S_gt_K", "capacity", "n_src", "width_switch",
             "raster_border", "height_window", "label0", "two_labels", "reset", "C0_always"}
    assert set(EDGES) == known


@pytest.mark.parametrize("tag", _with("collide"))
def test_degenerate_box_in_the_named_pass_and_the_collision_removes_points(tag):
    c, mod = K.case(tag), model_run(tag)
    for edge, ps, dim in [("R0_local", "local", "R"), ("R0_world", "world", "R"), ("C0_local", "local", "C"), ("C0_world", "world", "C")]:
        if edge in c.edges:
            assert any(st[ps]["n"] > 1 and st[ps][dim] == 0 for st in mod), (tag, edge)
    assert mod[0]["nl"] < mod[0]["local"]["pairs"]         # fewer survivors than distinct (env, cell) pairs
    assert any(st["local"]["n"] and st["local"]["R"] > 0 and st["local"]["C"] > 0 for st in mod[1:])   # ... then a 2-D cloud
    assert any(st["world"]["R"] > 0 and st["world"]["C"] > 0 and st["n_alive"] > 0 for st in mod[1:])
    if tag == "deg-c0-8x1":
        assert len(mod[0]["W"][0]) == 1 and mod[0]["local"]["K"] == 0   # 16 depths, two envs: one world point
    if tag == "deg-r0-1x20":   # only env 0's row survives where the envs' columns overlap
        assert mod[0]["local"]["n"] == 40 and len(mod[0]["W"][0]) < 40
    # the C <= 0 branch of the slot and q >= 1 (key >= C) are both taken somewhere in the section
    if "C0_local" in c.edges:
        assert table_slot(0, 0, 8) == 0 and table_slot(7, 0, 8) == 7 and table_slot(8, 0, 8) == -1
    if "R0_local" in c.edges and tag != "deg-1x1":
        d = next(st["local"] for st in mod if st["local"]["R"] == 0 and st["local"]["n"] > 1)
        assert d["K"] == d["C"] and d["K"] // d["C"] == 1


def test_one_column_boxes_fit_a_table_of_one_slot():
    for tag in _with("C0_always"):
        c, mod = K.case(tag), model_run(tag)
        assert c.table == 1 and table_bounds(tag) == (0, 0)
        for st in mod:
            for d in (st["local"], st["world"]):
                assert d["n"] >= 1 and d["C"] == 0 and d["K"] == 0 and (slots_of(d, 1) == 0).all()
            assert st["local"]["n"] > 1 and st["local"]["R"] > 0
            assert len(st["W"][0]) == 1
        assert mod[1]["world"]["n"] == 2   # an old and a new point meet under key 0


def test_ragged_chunks_and_rows_beyond_the_batch():
    for tag in _with("ragged"):
        c = K.case(tag)
        assert all((s["B"] * c.H * c.W) % (THREADS * PPT) for s in c.steps) and max(s["B"] for s in c.steps) * c.H * c.W > THREADS * PPT
    for tag in _with("rows_ge_B"):
        c = K.case(tag)
        assert any(s["B"] < c.B_max for s in c.steps)
    for tag in _with("paused"):   # B shrinks and grows again: the paused env's points drop out, its row comes back empty
        c, mod = K.case(tag), model_run(tag)
        Bs = [s["B"] for s in c.steps]
        assert Bs[:3] == [3, 2, 3]
        assert (mod[0]["W"][0] == 2).any() and not (mod[1]["W"][0] == 2).any() and mod[2]["n_alive"] == len(mod[1]["W"][0])
    assert [s["B"] for s in K.case("rag-seq-15").steps][:2] == [1, 5]
    for tag in _with("all_envs"):
        c, mod = K.case(tag), model_run(tag)
        B = c.steps[0]["B"]
        assert B in (33, 64) and all(set(st["W"][0].tolist()) == set(range(B)) for st in mod)
        assert B * 4 == THREADS if B == 64 else B * 4 < THREADS   # k_world_select's box init: one pass of the block at B = 64


def test_heights_reach_both_signs_and_every_kind_of_tie():
    for tag in _with("both_signs"):
        y = model_run(tag)[0]["W"][2]
        assert (y < 0).sum() > 20 and (y > 0).sum() > 20
    for tag in _with("negative"):
        assert all((st["W"][2] < 0).any() for st in model_run(tag))
    for tag in _with("tie_local"):
        st = model_run(tag)[0]
        assert st["local"]["ties"] == st["nl"] > 0 and st["local"]["n"] == st["nl"] * K.case(tag).H   # every cell: all image rows tie
    for tag in _with("tie_world"):   # the same frame again: every cell an old-versus-new tie, the old point stays
        mod = model_run(tag)
        assert mod[1]["world"]["ties"] > 0 and mod[1]["world"]["kept_old"] == mod[1]["world"]["n_old"] == len(mod[1]["W"][0])
    for tag in _with("neg_zero"):    # -0 wins a tie against +0 where it comes first: the fold in front of the ordering
        c, mod = K.case(tag), model_run(tag)
        b, x, y, z, lab = local_points(c, c.steps[0])
        assert (y == 0).all() and np.signbit(y[b == 1]).any() and not np.signbit(y[b == 1]).all() and not np.signbit(y[b == 0]).any()
        W = mod[0]["W"]
        assert np.signbit(W[2]).any()    # a -0 point survived: it was first among +0 points of its cell
        rr, cc = cells(z, f32(c.map[2] / 2)), cells(x, f32(c.map[2] / 2))
        mixed = [np.signbit(y[(b == 1) & (rr == r0) & (cc == c0)]) for r0, c0 in set(zip(rr[b == 1].tolist(), cc[b == 1].tolist()))]
        assert any(m[0] and not m.all() for m in mixed)
    up, down = model_run("hts-ulp-up"), model_run("hts-ulp-down")
    assert up[1]["world"]["kept_old"] == 0 and up[1]["world"]["n_old"] > 0           # one ulp higher: every new point wins
    assert down[1]["world"]["kept_old"] == down[1]["world"]["n_old"] > 0              # one ulp lower: every old point stays
    assert up[2]["world"]["kept_old"] == up[2]["world"]["n_old"] and down[2]["world"]["kept_old"] == down[2]["world"]["n_old"]


def test_table_boundaries():
    res = set()
    for tag in _with("S_gt_K"):
        S, Kmax = table_bounds(tag)
        assert S > Kmax > 0
        mod = model_run(tag)
        hit = [(t, ps) for t, st in enumerate(mod) for ps in ("local", "world") if st[ps]["n"] and int(slots_of(st[ps]).max()) == S]
        assert hit
        # with S + 1 cells nothing is refused, with S cells exactly the slot S is - and no KEY is (every key < S)
        for st in mod:
            for d in (st["local"], st["world"]):
                assert (slots_of(d, S + 1) >= 0).all() and (d["keys"] < S).all()
        t, ps = hit[0]
        assert (slots_of(mod[t][ps], S) < 0).sum() >= 1
        res |= {mod[t][ps]["C"] % 4 for t, ps in hit}
        res |= {st["world"]["C"] % 4 for st in mod}
    assert res == {0, 1, 2, 3}


def test_capacity_peak_is_the_oracles_count():
    N, t = capacity_peak("cap")
    mod = model_run("cap")
    assert all((s["not_done"] != 0).all() and s["B"] == K.case("cap").B_max for s in K.case("cap").steps)   # no dead points
    assert N == mod[t]["n_alive"] + mod[t]["nl"] and t >= 1 and N > len(mod[t]["W"][0])
    assert mod[0]["n_src"] <= N - 1   # the frame stepped after the reset fits the smaller capacity


def test_launch_width_partitions():
    want = {"wid-0": (0, 0), "wid-4096": (4096, 8192), "wid-4095": (4095, None), "wid-4097": (4097, None)}
    seen = set()
    for tag, (n0, n1) in want.items():
        mod = model_run(tag)
        assert mod[0]["n_src"] == n0 and (n1 is None or mod[1]["n_src"] == n1), (tag, [st["n_src"] for st in mod])
        seen |= {st["n_src"] % (THREADS * 16) for st in mod if st["n_src"] or tag == "wid-0"}
    assert {0, 1, THREADS * 16 - 1} <= seen
    idle = narrow = False
    for tag in K.WIDTH_CASES:
        c = K.case(tag)
        for lbw, wbw in K.WIDTHS:
            for s, st in zip(c.steps, model_run(tag)):
                lb, walk, ragged = local_grid(s["B"] * c.H * c.W, lbw)
                assert sum(walk) * THREADS * PPT - ragged == s["B"] * c.H * c.W and lb <= max(1, c.B_max * c.H * c.W // 1024 + 1)
                narrow |= lb == 1 and walk[0] > 1
                grid, wpt = world_grid(wbw)
                nbw = working_blocks(st["n_src"], wpt, grid)
                assert 1 <= nbw <= grid
                covered = sum(iters(st["n_src"], nbw, blk) for blk in range(grid)) * THREADS
                assert st["n_src"] <= covered < st["n_src"] + nbw * THREADS
                idle |= nbw < grid and iters(st["n_src"], nbw, grid - 1) == 0
    assert idle and narrow
    assert working_blocks(0, 16, 2) == 1 and working_blocks(4096, 16, 2) == 1 and working_blocks(4097, 16, 2) == 2
    assert working_blocks(4095, 16, 2) == 1 and working_blocks(8192, 16, 1) == 1 and working_blocks(8193, 16, 2) == 2
    sw = K.case("wid-switch")
    assert [s["width"] for s in sw.steps] == [(0, 0), (0, 0), (1, 1), (1, 1)]   # step 2 reads the boxes of a 1024-block grid


def test_raster_edges():
    for tag in _with("raster_border"):
        c = K.case(tag)
        hm, wm, res = c.map
        ref = K.oracle_run(tag)
        assert ref[0]["xyz"].shape[0] == c.B_max   # no two envs collided
        occ = ref[0]["occ"]
        for far in (False, True):
            zin, zout = raster_border(hm, res, far)
            xin, xout = raster_border(wm, res, far)
            assert np.nextafter(zin, zout) == zout and np.nextafter(xin, xout) == xout
            assert raster_cell(zin, hm / 2, res) == (c.rows - 1 if far else 0) and raster_cell(zout, hm / 2, res) == (c.rows if far else -1)
            assert raster_cell(xin, wm / 2, res) == (c.cols - 1 if far else 0) and raster_cell(xout, wm / 2, res) == (c.cols if far else -1)
            if not far:   # rintf of a value in (-0.5, 0) is -0.0 and is inside
                assert np.signbit(raster_cell(zin, hm / 2, res)) and np.signbit(raster_cell(xin, wm / 2, res))
        # envs 0..3: rows near in / out, far in / out; envs 4..7: columns
        assert [int(occ[b].sum()) for b in range(8)] == [1, 0, 1, 0, 1, 0, 1, 0]
        assert occ[0, 0].sum() == 1 and occ[2, c.rows - 1].sum() == 1 and occ[4, :, 0].sum() == 1 and occ[6, :, c.cols - 1].sum() == 1
        xyz = ref[0]["xyz"]
        assert np.array_equal(xyz[:4, 2], np.array([*raster_border(hm, res, False), *raster_border(hm, res, True)], f32))
        # heights: at h - 1.25 and h + 0.75 out, the fp32 neighbour inside the window in, the one outside out
        # (and h = -0.25 + 1 ulp: h + 0.75 still rounds to 0.5 in fp32, out)
        assert [int(ref[1]["occ"][b].sum()) for b in range(12, 19)] == [0, 1, 0, 0, 0, 1, 0]
        assert ref[1]["xyz"].shape[0] == c.B_max and (ref[1]["xyz"][12:, 1] == f32(0.5)).all()
        # envs 8..11: exactly -half (row / column 0) and +half (one past the last) of either axis
        assert [int(occ[b].sum()) for b in range(8, 12)] == [1, 0, 1, 0] and occ[8, 0].sum() == 1 and occ[10, :, 0].sum() == 1
        assert xyz[8, 2] == f32(-hm / 2) and xyz[9, 2] == f32(hm / 2) and xyz[10, 0] == f32(-wm / 2) and xyz[11, 0] == f32(wm / 2)
    for tag in _with("label0"):
        ref = K.oracle_run(tag)
        assert all(int(r["occ"].sum()) > 50 and int(r["sem"].sum()) == 0 for r in ref)
    for tag in _with("two_labels"):
        c, ref = K.case(tag), K.oracle_run(tag)
        hm, wm, res = c.map
        found = False
        for r, s in zip(ref, c.steps):   # two world points with different labels in one map cell: the later in the cloud wins
            for b in range(s["B"]):
                sel = r["b"] == b
                zr = (r["xyz"][sel] + (-s["pose"][b]))
                rot = s["rot"][b]
                xr = (rot[0, 0] * zr[:, 0] + rot[0, 1] * zr[:, 1]) + rot[0, 2] * zr[:, 2]
                zz = (rot[2, 0] * zr[:, 0] + rot[2, 1] * zr[:, 1]) + rot[2, 2] * zr[:, 2]
                row, col = np.rint((zz + f32(hm / 2)) / f32(res)), np.rint((xr + f32(wm / 2)) / f32(res))
                lab = r["lab"][sel]
                cellmap = {}
                for rr, cc2, lb in zip(row, col, lab):
                    if 0 <= rr < c.rows and 0 <= cc2 < c.cols and lb:
                        cellmap.setdefault((rr, cc2), []).append(int(lb))
                for (rr, cc2), labs in cellmap.items():
                    if len(set(labs)) > 1:
                        found = True
                        h = s["pose"][b, 1]
                        ys = r["xyz"][sel][:, 1]
                        if ((ys > h - f32(1.25)) & (ys < h + f32(0.75))).all():
                            assert r["sem"][b, int(rr), int(cc2)] == labs[-1]
        assert found
    for tag in _with("reset"):
        c, mod = K.case(tag), model_run(tag)
        t = next(i for i, s in enumerate(c.steps) if (s["not_done"] == 0).any())
        b = int(np.where(c.steps[t]["not_done"] == 0)[0][0])
        assert t >= 1 and (mod[t - 1]["W"][0] == b).any() and mod[t]["n_alive"] < len(mod[t - 1]["W"][0])
        assert mod[t]["n_src"] > mod[t]["n_alive"] + mod[t]["nl"]    # the dead env's points still sit in the source buffer


def test_entry_cases_step_on_derived_transforms():
    for tag in K.ENTRY_CASES:
        c = K.case(tag)
        assert c.posed
        ref = K.oracle_run(tag, True)
        assert ref[-1]["xyz"].shape[0] > 0 and int(ref[-1]["occ"].sum()) > 0
    heads = {float(s["orient"][b, 1]) for tag in K.ENTRY_CASES for s in K.case(tag).steps for b in range(s["B"])}
    assert heads == {0.0, np.pi, -np.pi, np.pi / 2, 1e-9}
    assert not K.case("hts-tie").posed and "hts-tie" not in K.ENTRY_CASES


# ----------------------------------------------------------------------------------------------------------------------
# every kernel of the step has a test
# ----------------------------------------------------------------------------------------------------------------------
def _step_kernels():
    src = open(os.path.join(ROOT, "ivln-ce_amd", "csrc", "mapper.hip")).read()
    head = src[:src.index("// ---- known-map mode ----")]
    pat = r"__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\("
    names = re.findall(pat, head)
    return sorted(set(names) | ({"k_frames"} if "k_frames" in re.findall(pat, src) else set()))


def _uncovered(names, table):
    no_entry = [n for n in names if n not in table]
    no_test = [n for n, t in table.items() if not callable(getattr(K, t, None)) or not t.startswith("test_")]
    return no_entry, no_test


def test_every_step_kernel_names_a_test():
    names = _step_kernels()
    assert names == sorted(["k_local_minmax", "k_local_argmax", "k_local_select", "k_world_max", "k_world_select", "k_finalize", "k_frames"])
    assert _uncovered(names, K.KERNEL_COVERED) == ([], [])
    assert not [n for n in K.KERNEL_COVERED if n not in names]
    short = dict(K.KERNEL_COVERED)
    short.pop("k_world_max")
    assert _uncovered(names, short)[0] == ["k_world_max"]      # removing a key is noticed
    assert _uncovered(names, dict(K.KERNEL_COVERED, k_finalize="test_that_is_not_there"))[1] == ["k_finalize"]
    assert K.pytestmark.name == "gpu"
