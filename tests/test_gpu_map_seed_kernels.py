"""GPU: the C calls of include/ivln_map_seed.h (ivln_mapper_rows_clear, ivln_mapper_env_append,
ivln_mapper_env_append_from_lib) against the C oracle driven as clear_done / load_known / step.  Every comparison is bit
for bit: occupancy map, semantic map, and the cloud in order (`world_cloud()` against `MapperRef.world()`).  Small frames
(16 x 16 depth, up to 4 envs, 64 x 64 maps); the oracle-only assertions say that a case really holds the tie or the key
collision it is there for."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H = W = 16
E_INVALID, E_KEYSPACE, E_CAPACITY, E_UNSUPPORTED = -1, -3, -4, -5
HALF_RES = np.float32(0.05)


TABLE = 1 << 20  # keys of 3 envs within ~6 m of the origin stay far below it


def _mk(b_max=4, table_cells=TABLE, world_capacity=0):
    from ivln_ce_amd.mapping import CameraParameters, MapDimensions, create_gt_semantics_iterative_mapper

    cam = CameraParameters(float(np.deg2rad(90.0)), (H, W), 0.1)
    m = create_gt_semantics_iterative_mapper(torch.device(DEV), cam, MapDimensions(6.4, 6.4, 0.1), b_max=b_max,
                                             table_cells=table_cells, world_capacity=world_capacity)
    m.ensure_handle(H, W)
    return m


def _frame(rng, B, not_done=None, headings=None, empty_rows=()):
    """One step's inputs: depths inside 5 m, labels 1..6 (seeds use 7..12), poses within a metre of the origin."""
    depth = rng.uniform(0.05, 0.5, (B, H, W)).astype(np.float32)
    for b in empty_rows:
        depth[b] = 0.0
    pose = np.stack([rng.uniform(-1, 1, B), np.full(B, 1.25), rng.uniform(-1, 1, B)], 1).astype(np.float32)
    head = rng.uniform(-np.pi, np.pi, B) if headings is None else np.asarray(headings, np.float64)
    return {"depth": depth, "labels": rng.randint(1, 7, (B, H, W)).astype(np.uint8), "pose": pose,
            "orient": np.stack([np.zeros(B), head], 1).astype(np.float64),
            "not_done": np.ones(B, np.uint8) if not_done is None else np.asarray(not_done, np.uint8)}


def _seed_points(rng, n, lo=7):
    xyz = np.stack([rng.uniform(-3, 3, n), rng.uniform(0.4, 1.7, n), rng.uniform(-3, 3, n)], 1).astype(np.float32)
    return xyz, rng.randint(lo, 13, n).astype(np.uint8)


class Pair:
    """A HIP mapper handle and the C oracle, driven in lockstep; every step compares maps, world size and cloud."""

    def __init__(self, **kw):
        from oracle import mapper_ref

        self.m = _mk(**kw)
        self.ref = mapper_ref.MapperRef(H, W)
        self.R = mapper_ref
        self.maps = []

    def raw_append(self, b, xyz, sem, n=None):
        from ivln_ce_amd._lib import lib, stream_ptr

        xyz_d = torch.from_numpy(np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)).to(DEV)
        sem_d = torch.from_numpy(np.ascontiguousarray(sem, np.uint8)).to(DEV)
        rc = lib().ivln_mapper_env_append(self.m._h, b, xyz_d.data_ptr(), sem_d.data_ptr(),
                                          len(sem) if n is None else n, stream_ptr())
        torch.cuda.synchronize()
        return rc

    def ref_append(self, b, xyz, sem):
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        sem = np.ascontiguousarray(sem, np.uint8)
        self.R.lib().mapper_ref_load_known(self.ref.h, b, self.R._p(xyz), self.R._p(sem), len(sem))

    def append(self, b, xyz, sem):
        assert self.raw_append(b, xyz, sem) == 0
        self.ref_append(b, xyz, sem)

    def clear(self, keep):
        from ivln_ce_amd._lib import lib, stream_ptr

        keep = np.ascontiguousarray(keep, np.uint8)
        keep_d = torch.from_numpy(keep).to(DEV)
        assert lib().ivln_mapper_rows_clear(self.m._h, keep_d.data_ptr(), len(keep), stream_ptr()) == 0
        torch.cuda.synchronize()
        self.R.lib().mapper_ref_clear_done(self.ref.h, len(keep), self.R._p(keep))

    def reset(self):
        self.m.reset()
        self.R.lib().mapper_ref_reset(self.ref.h)

    def obs(self, f):
        B = f["depth"].shape[0]
        return {"depth": torch.from_numpy(f["depth"]).to(DEV).reshape(B, H, W, 1),
                "semantic12": torch.from_numpy(f["labels"]).to(DEV).reshape(B, H, W, 1),
                "world_robot_pose": torch.from_numpy(f["pose"]).to(DEV),
                "world_robot_orientation": torch.from_numpy(f["orient"]).to(DEV),
                "not_done_masks": torch.from_numpy(f["not_done"]).to(DEV).reshape(B, 1), "env_name": ["s"] * B}

    def same_cloud(self, what):
        xr, br, sr = self.ref.world()
        xyz, b, s = self.m.world_cloud()
        assert xyz.shape[0] == xr.shape[0], f"{what}: {xyz.shape[0]} points, oracle {xr.shape[0]}"
        assert np.array_equal(np.ascontiguousarray(xyz).view(np.uint32), xr.view(np.uint32)), f"{what}: cloud xyz / order"
        assert np.array_equal(b, br) and np.array_equal(s, sr), f"{what}: cloud rows / labels"

    def step(self, f, what="step", split=False):
        T, rot = self.R.MapperRef.frames(f["pose"], f["orient"])
        occ_r, sem_r = self.ref.step(f["depth"], f["labels"], f["pose"], f["orient"], f["not_done"], T=T, rot=rot)
        o = self.obs(f)
        if split:
            self.m.begin(o)
            mem = self.m.finish(o)
        else:
            mem = self.m(o, T=torch.from_numpy(T).to(DEV), rot=torch.from_numpy(rot).to(DEV))
        assert self.m.check_status() == self.ref.world()[0].shape[0], f"{what}: world size"
        occ, sem = mem.occupancy.cpu().numpy(), mem.semantic.cpu().numpy()
        assert np.array_equal(occ, occ_r), f"{what}: occupancy"
        assert np.array_equal(sem, sem_r), f"{what}: semantic map"
        self.same_cloud(what)
        self.maps.append((occ.tobytes(), sem.tobytes()))

    def raw_world(self):
        """(xyz, meta, rank) bytes of ivln_mapper_world_export in ascending rank."""
        from ivln_ce_amd._lib import lib, stream_ptr

        _, n = self.m.status()
        xyz = torch.zeros((max(n, 1), 3), dtype=torch.float32, device=DEV)
        meta = torch.zeros((max(n, 1),), dtype=torch.int32, device=DEV)
        rank = torch.zeros((max(n, 1),), dtype=torch.int64, device=DEV)
        nn = C.c_int64(0)
        assert lib().ivln_mapper_world_export(self.m._h, xyz.data_ptr(), meta.data_ptr(), rank.data_ptr(), n, C.byref(nn),
                                              stream_ptr()) == 0
        assert nn.value == n
        r = rank[:n].cpu().numpy()
        order = np.argsort(r, kind="stable")
        return xyz[:n].cpu().numpy()[order].tobytes(), meta[:n].cpu().numpy()[order].tobytes(), r[order].tobytes()


def _cells(xyz):
    return np.rint(xyz[:, 2] / HALF_RES).astype(np.int64), np.rint(xyz[:, 0] / HALF_RES).astype(np.int64)


# ---- append into a handle without box partials ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
@pytest.mark.parametrize("start", ["fresh", "reset"])
def test_append_into_a_never_stepped_or_just_reset_handle(n, start):
    rng = np.random.RandomState(100 + n)
    p = Pair()
    if start == "reset":
        p.step(_frame(rng, 3), "step before the reset")
        p.append(1, *_seed_points(rng, 40))
        p.reset()
    xyz, sem = _seed_points(rng, n)
    p.append(1, xyz, sem)
    assert p.m.check_status() == n
    p.same_cloud("behind the append")
    assert np.array_equal(p.m.env_counts(), [0, n, 0, 0])
    p.step(_frame(rng, 3), "first step")
    p.step(_frame(rng, 3), "second step")


# ---- ordering ---------------------------------------------------------------------------------------------------------------
def test_order_old_before_seed_before_later_seed_before_local():
    from oracle.mapper_ref import MapperRef

    rng = np.random.RandomState(7)
    p = Pair()
    p.step(_frame(rng, 3), "step 0")
    p.step(_frame(rng, 3), "step 1")
    nxt = _frame(rng, 3, empty_rows=(2,))  # (row 2 sees nothing in the next frame: its resident stays the highest of its cell)
    # the next frame's own survivors, exact to the bit: a scratch oracle steps that frame alone
    scratch = MapperRef(H, W)
    scratch.step(nxt["depth"], nxt["labels"], nxt["pose"], nxt["orient"], nxt["not_done"])
    lx, lb, ls = scratch.world()
    q = int(np.flatnonzero(lb == 0)[np.argmax(lx[lb == 0, 1])])  # row 0's highest local point
    wx, wb, ws = p.ref.world()
    r_ = int(np.flatnonzero(wb == 2)[np.argmax(wx[wb == 2, 1])])  # row 2's highest resident point
    P, Q, S = wx[r_].copy(), lx[q].copy(), np.array([2.5, 1.74, -2.5], np.float32)
    assert 1 <= ws[r_] <= 6 and 1 <= ls[q] <= 6
    fill2, fill0a, fill0b = _seed_points(rng, 30, lo=11), _seed_points(rng, 30, lo=11), _seed_points(rng, 30, lo=11)
    # row 2 first, then two calls to row 0: non-ascending rows
    p.append(2, np.vstack([fill2[0][:10], P[None], fill2[0][10:]]), np.concatenate([fill2[1][:10], [7], fill2[1][10:]]))
    p.append(0, np.vstack([fill0a[0], S[None], Q[None]]), np.concatenate([fill0a[1], [8, 10]]))
    p.append(0, np.vstack([S[None], fill0b[0]]), np.concatenate([[9], fill0b[1]]))
    p.same_cloud("behind the appends")
    p.step(nxt, "the step behind the seeds")
    xr, br, sr = p.ref.world()

    def label_at(b, pt):
        hit = np.flatnonzero((br == b) & (xr.view(np.uint32) == pt.view(np.uint32)).all(1))
        assert len(hit) == 1, (b, pt, hit)
        return int(sr[hit[0]])

    assert label_at(2, P) == ws[r_]  # old beats seed (label 7)
    assert label_at(0, S) == 8       # the earlier seed beats the later one (label 9)
    assert label_at(0, Q) == 10      # seed beats the next frame's local point (label ls[q])
    p.step(_frame(rng, 3), "one more step")


# ---- rows_clear -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [[1, 1, 1], [1, 0, 1], [0, 0, 0], [1, 1]], ids=["all-ones", "one-of-three", "all", "B-smaller"])
def test_rows_clear(keep):
    rng = np.random.RandomState(11)
    p = Pair()
    p.step(_frame(rng, 3), "step 0")
    p.step(_frame(rng, 3), "step 1")
    before = p.raw_world()
    counts = p.m.env_counts()
    p.clear(keep)
    kept = [b for b in range(3) if b < len(keep) and keep[b]]
    want = np.array([counts[b] if b in kept else 0 for b in range(4)])
    assert np.array_equal(p.m.env_counts(), want)
    p.same_cloud("behind the clear")
    if all(keep) and len(keep) == 3:
        assert p.raw_world() == before  # a no-op: same points, same ranks
    p.append(1, *_seed_points(rng, 50))
    p.step(_frame(rng, 3), "step behind the clear")
    p.step(_frame(rng, 3), "second step behind the clear")


def test_rows_clear_keeps_the_boxes_exact():
    """Row 1 alone holds the extreme cell row and column of the world's box.  With it gone the box is row 0's 10 x 10 block
    of cells, whose column multiplier is 9 (quirk Q1): cell (r, 9) and cell (r + 1, 0) share a key (Q2) and the next step
    loses points to that.  A box that still covered row 1's corners would keep them all."""
    p = Pair()
    rr, cc = np.meshgrid(np.arange(10), np.arange(10), indexing="ij")
    grid = np.stack([cc.ravel() * 0.05, 0.5 + 0.01 * np.arange(100), rr.ravel() * 0.05], 1).astype(np.float32)
    far = np.array([[-5.0, 1.0, -5.0], [5.0, 1.0, 5.0]], np.float32)
    p.append(0, grid, np.full(100, 7, np.uint8))
    p.append(1, far, np.array([8, 9], np.uint8))
    blank = _frame(np.random.RandomState(3), 3, empty_rows=(0, 1, 2))
    p.step(blank, "step with the wide box")
    assert p.ref.world()[0].shape[0] == 102  # nothing collides while row 1 spans the box
    p.clear([1, 0, 1])
    p.step(blank, "step with row 0's own box")
    xr, br, _ = p.ref.world()
    r, c = _cells(xr)
    assert len(set(zip(br.tolist(), r.tolist(), c.tolist()))) == xr.shape[0] < 100  # the oracle lost points to shared keys
    p.step(_frame(np.random.RandomState(4), 3), "a real step behind it")


# ---- a seed longer than one pass of the import grid -----------------------------------------------------------------------
def test_long_seed_on_distinct_cells():
    side = 520  # 270400 points > 1024 workgroups x 256 threads
    rr, cc = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    rng = np.random.RandomState(5)
    xyz = np.stack([(cc.ravel() - side // 2) * 0.05, rng.uniform(0.4, 1.7, side * side), (rr.ravel() - side // 2) * 0.05],
                   1).astype(np.float32)
    sem = rng.randint(7, 13, side * side).astype(np.uint8)
    r, c = _cells(xyz)
    assert len(set(zip(r.tolist(), c.tolist()))) == side * side > 1024 * 256
    p = Pair(b_max=2, table_cells=0)
    p.append(0, xyz, sem)
    assert np.array_equal(p.m.env_counts(), [side * side, 0])
    p.step(_frame(rng, 2), "first step")
    p.step(_frame(rng, 2), "second step")


# ---- from a scene library -------------------------------------------------------------------------------------------------
def test_append_from_lib_equals_append_of_the_same_arrays():
    from ivln_ce_amd._lib import lib, stream_ptr
    from ivln_ce_amd.mapping import KnownSceneLibrary

    rng = np.random.RandomState(21)
    frames = [_frame(rng, 3) for _ in range(3)]
    scene_a, scene_b = _seed_points(rng, 700), _seed_points(rng, 257)
    klib = KnownSceneLibrary(torch.device(DEV), None, max_scenes=4)
    keep = []

    def add(i, xyz, sem):
        x, s = torch.from_numpy(xyz).to(DEV), torch.from_numpy(sem).to(DEV)
        rec = torch.empty((len(sem), 4), dtype=torch.float32, device=DEV)
        klib._add(i, x, s, rec)
        keep.append(rec)

    add(0, *scene_a)
    arrays, fromlib = Pair(), Pair()
    add(1, *scene_b)  # a scene added after the mappers were created
    for p in (arrays, fromlib):
        p.step(frames[0], "step 0")
    arrays.append(2, *scene_a)
    arrays.append(0, *scene_b)
    for b, i, sc in [(2, 0, scene_a), (0, 1, scene_b)]:
        assert lib().ivln_mapper_env_append_from_lib(fromlib.m._h, b, klib.handle(), i, stream_ptr()) == 0
        fromlib.ref_append(b, *sc)
    torch.cuda.synchronize()
    assert arrays.raw_world() == fromlib.raw_world()
    for p in (arrays, fromlib):
        p.step(frames[1], "step 1")
        p.step(frames[2], "step 2")
    assert arrays.raw_world() == fromlib.raw_world() and arrays.maps == fromlib.maps


# ---- between the append and the next step ---------------------------------------------------------------------------------
def test_counts_and_exports_around_an_append():
    from ivln_ce_amd._lib import lib, stream_ptr

    rng = np.random.RandomState(31)
    p = Pair()
    p.step(_frame(rng, 3), "step 0")
    counts = p.m.env_counts()
    p.append(1, *_seed_points(rng, 300))
    assert np.array_equal(p.m.env_counts(), counts + np.array([0, 300, 0, 0]))
    n1 = int(counts[1]) + 300
    xyz = torch.full((n1, 3), float("nan"), device=DEV)
    sem = torch.full((n1,), 0xFF, dtype=torch.uint8, device=DEV)
    n_out = C.c_int64(-7)
    # the appended ranks are not keys: the ordered export declines row 1, and still serves a row without such points
    assert lib().ivln_mapper_env_export(p.m._h, 1, xyz.data_ptr(), sem.data_ptr(), n1, C.byref(n_out), stream_ptr()) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(xyz).all() and (sem == 0xFF).all()
    xr, br, sr = p.ref.world()
    x0, s0 = p.m.export_scene(0)
    assert np.array_equal(x0.view(np.uint32), xr[br == 0].view(np.uint32)) and np.array_equal(s0, sr[br == 0])
    p.same_cloud("the table is clean behind the declined export")
    p.step(_frame(rng, 3), "step 1")
    xr, br, sr = p.ref.world()
    for b in range(3):
        xb, sb = p.m.export_scene(b)
        assert np.array_equal(xb.view(np.uint32), xr[br == b].view(np.uint32)) and np.array_equal(sb, sr[br == b]), b


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_by_return_code_leave_the_cloud_unchanged(tmp_path):
    from ivln_ce_amd._lib import lib, stream_ptr
    from ivln_ce_amd.mapping import KnownSceneLibrary, MapDimensions, MappingModule, save_known_scene

    L, s = lib(), stream_ptr()
    rng = np.random.RandomState(41)
    p = Pair()
    p.step(_frame(rng, 3), "step 0")
    p.append(0, *_seed_points(rng, 20))
    before = p.raw_world()
    h = p.m._h
    xyz, sem = _seed_points(rng, 64)
    xd, sd = torch.from_numpy(xyz).to(DEV), torch.from_numpy(sem).to(DEV)
    keep = torch.ones(4, dtype=torch.uint8, device=DEV)
    keep[1] = 0
    klib = KnownSceneLibrary(torch.device(DEV), None, max_scenes=4)
    rec = torch.empty((64, 4), dtype=torch.float32, device=DEV)
    klib._add(0, xd, sd, rec)
    app = lambda hh=h, b=0, x=xd.data_ptr(), l=sd.data_ptr(), n=64: L.ivln_mapper_env_append(hh, b, x, l, n, s)  # noqa: E731
    clr = lambda hh=h, k=keep.data_ptr(), B=3: L.ivln_mapper_rows_clear(hh, k, B, s)  # noqa: E731
    frm = lambda hh=h, b=0, kk=klib.handle(), i=0: L.ivln_mapper_env_append_from_lib(hh, b, kk, i, s)  # noqa: E731
    assert app(hh=None) == E_INVALID and app(b=-1) == E_INVALID and app(b=4) == E_INVALID and app(n=-1) == E_INVALID
    assert app(x=None) == E_INVALID and app(l=None) == E_INVALID
    assert clr(hh=None) == E_INVALID and clr(B=0) == E_INVALID and clr(B=5) == E_INVALID and clr(k=None) == E_INVALID
    assert frm(hh=None) == E_INVALID and frm(b=-1) == E_INVALID and frm(b=4) == E_INVALID and frm(kk=None) == E_INVALID
    assert frm(i=1) == E_INVALID and frm(i=-1) == E_INVALID and frm(i=4) == E_INVALID  # never added / outside the library
    # the rank band [table_cells, 2^31) cannot hold that many points: refused before anything is read
    assert app(n=(1 << 31) - TABLE) == E_KEYSPACE
    torch.cuda.synchronize()
    assert p.raw_world() == before
    assert app(n=0) == 0 and app(x=None, l=None, n=0) == 0
    assert p.raw_world() == before

    # a mapper with a library attached, and one that holds ivln_mapper_load_known points
    dims = MapDimensions(6.4, 6.4, 0.1)
    save_known_scene(str(tmp_path), "s", xyz, sem)
    pose = torch.tensor([[0.0, 1.25, 0.0]] * 2, device=DEV)
    o = {"depth": torch.zeros((2, H, W, 1), device=DEV), "world_robot_pose": pose, "env_name": ["s", "s"],
         "world_robot_orientation": torch.zeros((2, 2), dtype=torch.float64, device=DEV),
         "not_done_masks": torch.zeros((2, 1), dtype=torch.uint8, device=DEV)}
    for kw in (dict(known_library=True), dict()):
        known = MappingModule(torch.device(DEV), None, dims, mode="known", maps_location=str(tmp_path), b_max=4, **kw)
        known(dict(o))
        assert known.check_status() == 128
        assert app(hh=known._h) == E_UNSUPPORTED and clr(hh=known._h) == E_UNSUPPORTED and frm(hh=known._h) == E_UNSUPPORTED
        assert known.check_status() == 128

    # capacity: refused whole, before anything is written
    small = Pair(world_capacity=300)
    small.append(2, *_seed_points(rng, 200))
    at200 = small.raw_world()
    x101, s101 = _seed_points(rng, 101)
    assert small.raw_append(2, x101, s101) == E_CAPACITY
    assert small.m.check_status() == 200 and small.raw_world() == at200
    small.append(2, x101[:100], s101[:100])
    assert small.m.check_status() == 300
    small.same_cloud("a full cloud")


# ---- the split step, determinism -------------------------------------------------------------------------------------------
def _scenario(split):
    rng = np.random.RandomState(51)
    quarter = [0.0, np.pi / 2, np.pi]
    p = Pair()
    p.step(_frame(rng, 3, headings=quarter), "step 0", split=split)
    p.append(2, *_seed_points(rng, 300))
    p.append(0, *_seed_points(rng, 257))
    p.step(_frame(rng, 3, headings=quarter[::-1]), "step 1", split=split)
    p.clear([1, 1, 0])
    p.append(2, *_seed_points(rng, 100))
    p.step(_frame(rng, 3, headings=quarter), "step 2", split=split)
    return p.maps, p.raw_world()


def test_split_step_behind_a_seed_equals_the_whole_step_and_runs_repeat():
    whole, again, split = _scenario(False), _scenario(False), _scenario(True)
    assert whole == again  # two runs, the same bytes: maps, points, ranks
    assert whole == split
