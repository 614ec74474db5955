"""The iterative mapper's state that outlives a call (csrc/mapper.hip): the keep-highest arg-max table and the per-cell
raster words are all zero between complete calls, and an ivln_mapper_step_begin that is never finished must not cost a
later step a single point.  ivln_mapper_debug_nonzero (include/ivln_mapper_debug.h) reads the invariant itself; everything
else is held bit for bit to the C oracle, which is fed the COMPLETED steps only - occupancy, semantic map, world size,
world xyz as uint32, env and label in rank order.  Every comparison is a line of the step-kernel file's log before it is an
assertion (its _Cmp), and after every call of every test the probe must read [0, 0] except where a test says otherwise.

Buffers, cases and the oracle are the step-kernel file's (tests/test_gpu_mapper_step_kernels.py: _Hip and its sentinel
bands, case, oracle_run, ENTRY_CASES - frames of a few hundred pixels, B_max <= 64, tables of 2^19 cells).  The sequences:

  clean walk         every entry form, every ENTRY_CASE; the capacity-one-short and table-one-slot-short cases too
  dangling + reset   begin(A), no finish: probe > 0; reset: [0, 0]; then the walk W equals the oracle stepped with W
  dangling + refused begin(A), then every call the open state refuses: IVLN_E_INVALID, sentinels, probe and status untouched;
                     finish(A) completes A and the walk goes on.  A closed twin takes the same calls with IVLN_OK.
  dangling mid-walk  steps 0, 1, begin(2): world_export = the oracle after step 1; finish: step 2 and env_export = oracle;
                     or reset and a fresh walk - behind begin(2) itself, and behind the begin of step 0's frame 1 cm higher
  other consumers    env_export one short, env_export, add_from_mapper: [0, 0], and the next two steps equal the oracle
  two streams        begin on a side stream, finish on the main one behind an event

DANGLING names the step A whose begin is abandoned and the first step of the walk behind the reset; the CPU
companion (tests/test_mapper_protocol_host.py) runs a model of the table through exactly these pairs WITHOUT the reset and
asserts that points are lost - so a reset that does not clear the table cannot pass here.  Two clean steps follow every
interruption: a slot poisoned in the world pass loses its point on every later step.

Measured on an MI355X: 69 tests, 3196 comparisons (lines of the log), none above 0.2 s, the file under 2 s.  On the commit
before the fix (its library with only the probe added) every dangling + reset and mid-walk reset sequence fails - the table
still holds A's 38 - 592 entries behind the reset, and the walk is short of the oracle by exactly the points the CPU
companion's model predicts: 0 - 7 for the pairs of unrelated frames (reset-step2 included: where the model predicts 0 only
the probe fails), every survivor of B - 38 to 580 points - for the lifted ones -, and so do both refused-call sequences
(every call returns IVLN_OK) and both MappingModule tests."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_mapper_step_kernels as K
from kernel_bar import _log
from test_gpu_mapper_step_kernels import ENTRY_CASES, PAD, _Cmp, _Hip, _out, case, oracle_run

pytestmark = pytest.mark.gpu
DEV = K.DEV
LOG = K.LOG
E_INVALID, E_CAPACITY = -1, K.RC["capacity"]

LIFT = 0.01   # metres
# (case, index of the abandoned step A, first step of the walk behind the reset, lift of A's camera).  Two kinds:
#  - A and the walk's first step B are different steps of the case.  Their frames are unrelated, a few hundred survivors in
#    a key space of tens of thousands of slots: a forgotten arg-max meets B in a handful of slots or in none (the CPU
#    companion models every ordered pair of every case).  Listed: the pairs whose walk loses points in B's local pass and
#    is still short behind its last step.
#  - A = B's own frame seen from a camera 1 cm higher - what a capture's example frame is to the first frame stepped: the
#    same cells, the same box, so the same slots, every entry 1 cm above B's candidate.  B loses every survivor it has.
DANGLING = [("rag-seq-323", 2, 0, 0.0), ("rag-seq-323", 0, 1, 0.0), ("b33-4x4", 1, 0, 0.0)] + [(tag, 0, 0, LIFT) for tag in ENTRY_CASES]
MID_CASES = [t for t in ENTRY_CASES if len(case(t).steps) >= 3]   # steps 0, 1 complete, step 2 interrupted
MID_RESET = (0, LIFT)   # (A, lift) of the mid-walk begin that a reset and a fresh walk from step 0 follow
REFUSED_CASES = ["rag-seq-323", "hts-signs"]


def step_a(tag, a, lift):
    """the step whose begin is abandoned: step `a` of the case, its camera (pose y) `lift` metres higher"""
    s = dict(case(tag).steps[a])
    s["pose"] = s["pose"].copy()
    s["pose"][:, 1] += K.f32(lift)
    return s


class _P(_Hip):
    """_Hip + the probe, the calls of the builder / seeding headers, and a begin that can be left open"""

    def probe(self):
        out = (C.c_int64 * 2)(-1, -1)
        rc = self.L.ivln_mapper_debug_nonzero(self.h, out, self.s)
        assert rc == 0, f"ivln_mapper_debug_nonzero: {rc}"
        return [int(out[0]), int(out[1])]

    def env_export(self, b, max_n):
        """-> (rc, n_out, xyz uint32 (max_n, 3), sem, sentinels intact) through banded buffers"""
        xyz, px = _out(3 * max(max_n, 1), float("nan"), torch.float32)
        sem, ps = _out(max(max_n, 1), K.SENT_U8, torch.uint8)
        n_out = C.c_int64(-7)
        rc = self.L.ivln_mapper_env_export(self.h, b, px, ps, max_n, C.byref(n_out), self.s)
        torch.cuda.synchronize()
        x, l = xyz.cpu().numpy().view(np.uint32), sem.cpu().numpy()
        nan = np.float32("nan").view(np.uint32)
        n = n_out.value if rc == 0 else 0
        clean = bool((x[:PAD] == nan).all() and (x[PAD + 3 * n:] == nan).all() and (l[:PAD] == K.SENT_U8).all()
                     and (l[PAD + n:] == K.SENT_U8).all())
        return rc, n_out.value, x[PAD:PAD + 3 * n].reshape(n, 3), l[PAD:PAD + n], clean


class _Lib:
    """a scene library through the C ABI with one scene (index 0) of `n` points added from host arrays"""

    def __init__(self, m, n=5):
        self.L, self.s = m.L, m.s
        self.h = C.c_void_p()
        assert self.L.ivln_known_lib_create(4, C.byref(self.h)) == 0
        self.xyz = torch.linspace(0.1, 0.9, 3 * n, device=DEV).reshape(n, 3).contiguous()
        self.sem = torch.arange(1, n + 1, dtype=torch.uint8, device=DEV)
        self.rec0 = torch.zeros((n, 4), device=DEV)
        assert self.L.ivln_known_lib_add(self.h, 0, self.xyz.data_ptr(), self.sem.data_ptr(), n, self.rec0.data_ptr(), self.s) == 0
        self.n = n

    def size(self):
        return self.L.ivln_known_lib_size(self.h)

    def close(self):
        torch.cuda.synchronize()
        self.L.ivln_known_lib_destroy(self.h)


def _hold(cmp, m, t, o, r, posed=True):
    """the state a complete step left against the oracle's record r, and the probe at [0, 0]"""
    code, n = m.status()
    cmp.eq(t, "status", code, 0)
    cmp.eq(t, "guards", o["guards"], True)
    cmp.eq(t, "world_n", n, r["xyz"].shape[0])
    cmp.eq(t, "occ", o["occ"], r["occ"])
    cmp.eq(t, "sem", o["sem"], r["sem"])
    if code == 0 and 0 <= n <= m.c.cap:
        xyz, b, lab = m.world(n)
        cmp.eq(t, "world_xyz", xyz, r["xyz"].view(np.uint32))
        cmp.eq(t, "world_env", b, r["b"])
        cmp.eq(t, "world_label", lab, r["lab"])
    if posed:
        cmp.eq(t, "T_out", o["T"], r["T"].reshape(-1).view(np.uint32))
        cmp.eq(t, "rot_out", o["rot"], r["rot"].reshape(-1).view(np.uint32))
    cmp.eq(t, "probe", m.probe(), [0, 0])


def _lost(cmp, m, t, r):
    """a line of the log: how many world points the mapper is short of the oracle (the parent-commit evidence)"""
    _code, n = m.status()
    _log(f"{cmp.what:44s} step {t} world points: oracle {r['xyz'].shape[0]}, mapper {n}, short {r['xyz'].shape[0] - n}", LOG)


def _walk(cmp, m, c, ref, first, entries=("posed",), t0=0):
    """the case's steps from `first` on, as many as `ref` has records, each held to its record"""
    for t, (s, _r) in enumerate(zip(c.steps[first:], ref)):
        entry = entries[t % len(entries)]
        o = m.step(s, entry)
        _lost(cmp, m, t0 + t, ref[t])
        _hold(cmp, m, t0 + t, o, ref[t], posed=entry != "step")


def _export_equals_oracle(cmp, m, t, r, envs):
    for b in envs:
        sel = r["b"] == b
        n = int(sel.sum())
        rc, n_out, xyz, sem, clean = m.env_export(b, n)
        cmp.eq(t, f"exp{b}:rc", rc, 0)
        cmp.eq(t, f"exp{b}:n", n_out, n)
        cmp.eq(t, f"exp{b}:xyz", xyz, r["xyz"].view(np.uint32)[sel])
        cmp.eq(t, f"exp{b}:sem", sem, r["lab"][sel])
        cmp.eq(t, f"exp{b}:bands", clean, True)
        cmp.eq(t, f"exp{b}:probe", m.probe(), [0, 0])


# ----------------------------------------------------------------------------------------------------------------------
# clean walks
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["step"] + K.ENTRIES)
@pytest.mark.parametrize("tag", ENTRY_CASES)
def test_clean_walk_leaves_the_table_zero(tag, entry):
    c = case(tag)
    ref = oracle_run(tag, entry != "step")
    cmp = _Cmp(f"protocol clean {tag} {entry}")
    m = _P(c)
    try:
        cmp.eq(-1, "probe", m.probe(), [0, 0])
        _walk(cmp, m, c, ref, 0, (entry,))
        cmp.done()
    finally:
        m.close()


def test_capacity_one_short_leaves_the_table_zero_before_and_after_reset():
    import test_mapper_step_coverage as P

    N, t_peak = P.capacity_peak("cap")
    c = case("cap")
    cmp = _Cmp("protocol cap one short")
    m = _P(c, cap=N - 1)
    try:
        for t, s in enumerate(c.steps[:t_peak + 1]):
            m.step(s)
            cmp.eq(t, "status", m.status()[0], E_CAPACITY if t == t_peak else 0)
            cmp.eq(t, "probe", m.probe(), [0, 0])
        m.reset()
        cmp.eq(9, "status", m.status(), (0, 0))
        cmp.eq(9, "probe", m.probe(), [0, 0])
        o = m.step(c.steps[0])
        _hold(cmp, m, 10, o, oracle_run("cap")[0], posed=False)
        cmp.done()
    finally:
        m.close()


@pytest.mark.parametrize("tag", K.TAB_CASES)
def test_table_one_slot_short_leaves_the_table_zero_before_and_after_reset(tag):
    import test_mapper_step_coverage as P

    S, _K = P.table_bounds(tag)
    c = case(tag)
    cmp = _Cmp(f"protocol {tag} table {S}")
    m = _P(c, table=S)
    try:
        for t, s in enumerate(c.steps):
            m.step(s)
            cmp.eq(t, "probe", m.probe(), [0, 0])
        cmp.eq(9, "status", m.status()[0], K.RC["keyspace"])
        m.reset()
        cmp.eq(9, "status", m.status(), (0, 0))
        cmp.eq(9, "probe", m.probe(), [0, 0])
        cmp.done()
    finally:
        m.close()


# ----------------------------------------------------------------------------------------------------------------------
# a begin that is never finished
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,a,first,lift", DANGLING, ids=lambda v: str(v))
def test_dangling_begin_then_reset(tag, a, first, lift):
    """begin(A), no finish: the table holds A's arg-max (probe > 0: the probe sees what it is there to see); reset empties
    it; the walk behind it equals the oracle stepped with that walk alone"""
    c = case(tag)
    ref = oracle_run(tag, True, first)
    cmp = _Cmp(f"protocol dangling+reset {tag} A{a}+{lift} from {first}")
    m = _P(c)
    try:
        qa = m.buffers(step_a(tag, a, lift))
        cmp.eq(-2, "begin:rc", m.begin(qa), 0)
        dirty = m.probe()
        _log(f"{cmp.what:44s} probe behind begin(A): {dirty}", LOG)
        cmp.eq(-2, "dirty>0", dirty[0] > 0, True)
        cmp.eq(-2, "cells", dirty[1], 0)
        m.reset()
        cmp.eq(-1, "probe", m.probe(), [0, 0])
        cmp.eq(-1, "status", m.status(), (0, 0))
        _walk(cmp, m, c, ref, first)
        cmp.done()
    finally:
        m.close()


@pytest.mark.parametrize("tag", REFUSED_CASES)
def test_dangling_begin_then_every_refused_call(tag):
    """step 0, begin(1), then each call the open state refuses - IVLN_E_INVALID, nothing launched, nothing written: output
    sentinels, the probe's counts, ivln_mapper_status and the library as they were - then finish(1) and the walk goes on.
    A closed twin mapper (steps 0 and 1 complete) takes the data calls with IVLN_OK: the arguments are good, it is the
    open begin that is refused."""
    c = case(tag)
    ref = oracle_run(tag, True)
    cmp = _Cmp(f"protocol refused {tag}")
    m, twin = _P(c), _P(c)
    lib = _Lib(m)
    try:
        _walk(cmp, m, c, ref[:1], 0)
        for s in c.steps[:2]:
            twin.step(s, "posed")
        q1 = m.buffers(c.steps[1])
        cmp.eq(1, "begin:rc", m.begin(q1), 0)
        before, status = m.probe(), m.status()
        cmp.eq(1, "dirty>0", before[0] > 0, True)
        B = c.steps[1]["B"]
        keep = torch.ones(B, dtype=torch.uint8, device=DEV)
        n0 = int((ref[1]["b"] == 0).sum())
        rec, prec = _out(4 * (n0 + 1), float("nan"), torch.float32)
        prec += (-prec) % 16   # (16-byte records)
        nan = np.float32("nan").view(np.uint32)

        def steps(mm, entry):
            q = mm.buffers(c.steps[2])
            rc = mm.begin(q) if entry == "begin" else mm.call(q, entry)
            return rc, mm.result(q, "posed", rows=0)["guards"]

        def export(mm):
            rc, n_out, _x, _l, clean = mm.env_export(0, n0)
            return rc, clean and (rc == 0 or n_out == -7)

        def add(mm):
            rc = mm.L.ivln_known_lib_add_from_mapper(lib.h, 1 if mm is m else 2, mm.h, 0, prec, n0, mm.s)
            torch.cuda.synchronize()
            return rc, rc == 0 or bool((rec.cpu().numpy().view(np.uint32) == nan).all())

        calls = {
            "ivln_mapper_step_begin": lambda mm: steps(mm, "begin"),
            "ivln_mapper_step": lambda mm: steps(mm, "step"),
            "ivln_mapper_step_posed": lambda mm: steps(mm, "posed"),
            "ivln_mapper_env_export": export,
            "ivln_known_lib_add_from_mapper": add,
            "ivln_mapper_env_append": lambda mm: (mm.L.ivln_mapper_env_append(mm.h, 0, lib.xyz.data_ptr(), lib.sem.data_ptr(), lib.n, mm.s), True),
            "ivln_mapper_env_append_from_lib": lambda mm: (mm.L.ivln_mapper_env_append_from_lib(mm.h, 0, lib.h, 0, mm.s), True),
            "ivln_mapper_rows_clear": lambda mm: (mm.L.ivln_mapper_rows_clear(mm.h, keep.data_ptr(), B, mm.s), True),
        }
        assert set(calls) == set(REFUSED)
        size = lib.size()
        for name, fn in calls.items():
            rc, untouched = fn(m)
            cmp.eq(1, name[5:25], rc, E_INVALID)
            cmp.eq(1, "  outputs", untouched, True)
            cmp.eq(1, "  probe", m.probe(), before)
            cmp.eq(1, "  status", m.status(), status)
            cmp.eq(1, "  library", lib.size(), size)
        # the closed twin: the same data calls, same arguments (the step entries are every other test's subject)
        for name in ["ivln_mapper_env_export", "ivln_known_lib_add_from_mapper", "ivln_mapper_env_append",
                     "ivln_mapper_env_append_from_lib", "ivln_mapper_rows_clear"]:
            cmp.eq(1, "twin:" + name[12:25], calls[name](twin)[0], 0)
        cmp.eq(1, "finish:rc", m.finish(q1), 0)
        o = m.result(q1, "posed")
        _hold(cmp, m, 1, o, ref[1])
        for t, s in enumerate(c.steps[2:], 2):
            o = m.step(s, "split" if t % 2 else "posed")
            _hold(cmp, m, t, o, ref[t])
        cmp.done()
    finally:
        m.close()
        twin.close()
        lib.close()


@pytest.mark.parametrize("how", ["finish", "reset", "reset-step2"])
@pytest.mark.parametrize("tag", MID_CASES)
def test_dangling_begin_in_the_middle_of_a_walk(tag, how):
    """steps 0 and 1, then a begin that is left open.  finish: begin(step 2), world_export equals the oracle behind step 1,
    finish completes step 2, env_export equals the oracle, the walk goes on.  reset-step2: the same begin(step 2), abandoned
    by a reset, then a fresh walk from step 0 - the sequence as it is usually met; step 2 and step 0 are unrelated frames, so
    an uncleared table costs the fresh walk a handful of points or none (the CPU companion prints the model's count for each
    case).  reset: what is abandoned is instead step 0's own frame from 1 cm higher (MID_RESET), which costs the fresh walk
    every survivor of its first step - the variant a reset that does not clear the table cannot pass."""
    c = case(tag)
    ref = oracle_run(tag, True)
    cmp = _Cmp(f"protocol mid-walk {how} {tag}")
    m = _P(c)
    try:
        _walk(cmp, m, c, ref[:2], 0)
        q2 = m.buffers(step_a(tag, *MID_RESET) if how == "reset" else c.steps[2])
        cmp.eq(2, "begin:rc", m.begin(q2), 0)
        cmp.eq(2, "dirty>0", m.probe()[0] > 0, True)
        code, n = m.status()   # the cloud is what step 1 left: begin touches the table alone
        cmp.eq(2, "status", (code, n), (0, ref[1]["xyz"].shape[0]))
        if n == ref[1]["xyz"].shape[0]:
            xyz, b, lab = m.world(n)
            cmp.eq(2, "world_xyz", xyz, ref[1]["xyz"].view(np.uint32))
            cmp.eq(2, "world_env", b, ref[1]["b"])
            cmp.eq(2, "world_label", lab, ref[1]["lab"])
        if how == "finish":
            cmp.eq(2, "finish:rc", m.finish(q2), 0)
            _hold(cmp, m, 2, m.result(q2, "posed"), ref[2])
            _export_equals_oracle(cmp, m, 2, ref[2], range(c.steps[2]["B"]))
            for t, s in enumerate(c.steps[3:], 3):
                _hold(cmp, m, t, m.step(s, "posed"), ref[t])
        else:
            m.reset()
            cmp.eq(3, "probe", m.probe(), [0, 0])
            cmp.eq(3, "status", m.status(), (0, 0))
            _walk(cmp, m, c, ref, 0, t0=10)
            _export_equals_oracle(cmp, m, 19, ref[-1], range(c.steps[-1]["B"]))
        cmp.done()
    finally:
        m.close()


# ----------------------------------------------------------------------------------------------------------------------
# the table's other users
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", MID_CASES)
def test_export_and_library_promotion_leave_the_table_zero(tag):
    c = case(tag)
    ref = oracle_run(tag, True)
    cmp = _Cmp(f"protocol consumers {tag}")
    m = _P(c)
    lib = _Lib(m)
    try:
        _walk(cmp, m, c, ref[:1], 0)
        B = c.steps[0]["B"]
        b = int(np.bincount(ref[0]["b"], minlength=B).argmax())   # the row with the most points
        n = int((ref[0]["b"] == b).sum())
        assert n > 1
        rc, n_out, _x, _l, clean = m.env_export(b, n - 1)
        cmp.eq(0, "short:rc", rc, E_CAPACITY)
        cmp.eq(0, "short:n", n_out, n)
        cmp.eq(0, "short:bands", clean, True)
        cmp.eq(0, "short:probe", m.probe(), [0, 0])
        _export_equals_oracle(cmp, m, 0, ref[0], range(B))
        rec, prec = _out(4 * (n + 1), float("nan"), torch.float32)
        prec += (-prec) % 16
        cmp.eq(0, "add:rc", m.L.ivln_known_lib_add_from_mapper(lib.h, 1, m.h, b, prec, n, m.s), 0)
        cmp.eq(0, "add:probe", m.probe(), [0, 0])
        off = (prec - rec.data_ptr()) // 4
        got = rec.cpu().numpy()[off:off + 4 * n].reshape(n, 4)
        sel = ref[0]["b"] == b
        cmp.eq(0, "add:xyz", got[:, :3].view(np.uint32), ref[0]["xyz"].view(np.uint32)[sel])
        cmp.eq(0, "add:label", np.ascontiguousarray(got[:, 3]).view(np.uint32), ref[0]["lab"][sel].astype(np.uint32))
        for t, s in enumerate(c.steps[1:3], 1):
            _hold(cmp, m, t, m.step(s, "split" if t == 1 else "posed"), ref[t])
        cmp.done()
    finally:
        m.close()
        lib.close()


@pytest.mark.parametrize("tag", REFUSED_CASES)
def test_begin_on_a_side_stream_finish_on_the_main_one(tag):
    """what a predicted-semantics step does beside RedNet: begin on a side stream, finish on the caller's behind an event"""
    c = case(tag)
    ref = oracle_run(tag, True)
    cmp = _Cmp(f"protocol two streams {tag}")
    m = _P(c)
    side, main = torch.cuda.Stream(), torch.cuda.current_stream()
    try:
        for t, s in enumerate(c.steps):
            q = m.buffers(s)
            ev = torch.cuda.Event()
            side.wait_stream(main)   # (the buffers were filled on the main stream)
            rc = m.L.ivln_mapper_step_begin(m.h, q.dep, q.pose, q.ori, q.nd, q.B, q.pocc, q.pT, q.pr, side.cuda_stream)
            ev.record(side)
            main.wait_event(ev)
            cmp.eq(t, "begin:rc", rc, 0)
            cmp.eq(t, "finish:rc", m.finish(q), 0)
            _hold(cmp, m, t, m.result(q, "posed"), ref[t])
        cmp.done()
    finally:
        m.close()


# ----------------------------------------------------------------------------------------------------------------------
# MappingModule
# ----------------------------------------------------------------------------------------------------------------------
def _module(b_max=2):
    from ivln_ce_amd.mapping import CameraParameters, MapDimensions, create_gt_semantics_iterative_mapper

    cam = CameraParameters(float(np.deg2rad(90.0)), (64, 64), 0.1)
    return create_gt_semantics_iterative_mapper(torch.device(DEV), cam, MapDimensions(6.4, 6.4, 0.1), b_max=b_max)


def _frames(n, seed=22):
    from ivln_ce_amd.synthetic import SyntheticRollout

    roll = SyntheticRollout(B=2, H=64, W=64, seed=seed)
    out = []
    for _ in range(n):
        obs = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in roll.step().items()}
        obs["not_done_masks"] = torch.ones(2, 1, dtype=torch.uint8, device=DEV)
        out.append(obs)
    return out


def _module_probe(m):
    from test_gpu_policy import mapper_table_nonzero   # (the one wrapper of ivln_mapper_debug_nonzero for a MappingModule)

    return mapper_table_nonzero(m)


def test_module_refuses_begin_and_forward_while_a_begin_is_open():
    from ivln_ce_amd._lib import IvlnError

    obs = _frames(2)
    m = _module()
    m.begin(obs[0])
    dirty = _module_probe(m)
    assert dirty[0] > 0
    with pytest.raises(IvlnError, match="begin"):
        m.begin(obs[1])
    with pytest.raises(IvlnError, match="begin"):
        m.forward(obs[1])
    with pytest.raises(IvlnError, match="begin"):
        m(obs[1])
    assert _module_probe(m) == dirty
    m.finish(obs[0])
    assert _module_probe(m) == [0, 0] and m.check_status() > 0
    m(obs[1])
    assert _module_probe(m) == [0, 0]


def test_module_reset_closes_an_open_begin():
    """begin, reset: export_scene, seed_row and forward work again, and the stepped maps and cloud equal a fresh module's"""
    obs = _frames(4)
    seed_xyz = np.array([[0.3, 0.2, 0.4], [0.5, 0.1, -0.2], [-0.4, 0.3, 0.6]], np.float32)
    seed_sem = np.array([3, 5, 7], np.uint8)
    m, fresh = _module(), _module()
    m(obs[0])
    m.begin(obs[3])
    assert _module_probe(m)[0] > 0
    m.reset()
    assert _module_probe(m) == [0, 0] and m.check_status() == 0
    xyz, sem = m.export_scene(0)
    assert xyz.shape == (0, 3) and sem.shape == (0,)
    fresh.ensure_handle(64, 64)
    cmp = _Cmp("protocol module reset")
    for mm in (m, fresh):
        mm.seed_row(1, seed_xyz, seed_sem)
    for t in (1, 2):
        got, want = m(obs[t]), fresh(obs[t])
        cmp.eq(t, "occ", got.occupancy.cpu().numpy(), want.occupancy.cpu().numpy())
        cmp.eq(t, "sem", got.semantic.cpu().numpy(), want.semantic.cpu().numpy())
        cmp.eq(t, "status", m.check_status(), fresh.check_status())
        for k, (a, b) in enumerate(zip(m.world_cloud(), fresh.world_cloud())):
            cmp.eq(t, f"cloud{k}", a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
        cmp.eq(t, "probe", _module_probe(m), [0, 0])
    assert fresh.check_status() > 100
    cmp.done()


# entry point the open state refuses (include/ivln_hip.h, ivln_mapper_step_begin) -> a test of this file that makes the call
# on an open mapper and holds it to IVLN_E_INVALID with nothing written
REFUSED = {
    "ivln_mapper_step_begin": "test_dangling_begin_then_every_refused_call",
    "ivln_mapper_step": "test_dangling_begin_then_every_refused_call",
    "ivln_mapper_step_posed": "test_dangling_begin_then_every_refused_call",
    "ivln_mapper_env_export": "test_dangling_begin_then_every_refused_call",
    "ivln_known_lib_add_from_mapper": "test_dangling_begin_then_every_refused_call",
    "ivln_mapper_env_append": "test_dangling_begin_then_every_refused_call",
    "ivln_mapper_env_append_from_lib": "test_dangling_begin_then_every_refused_call",
    "ivln_mapper_rows_clear": "test_dangling_begin_then_every_refused_call",
}
# function of csrc/mapper.hip that hands the table to a launch or a memset -> a test of this file whose sequence runs it
TABLE_USERS = {
    "ivln_mapper_create": "test_clean_walk_leaves_the_table_zero",
    "ivln_mapper_reset": "test_dangling_begin_then_reset",
    "mapper_begin": "test_dangling_begin_then_reset",
    "mapper_finish": "test_dangling_begin_in_the_middle_of_a_walk",
    "env_compact": "test_export_and_library_promotion_leave_the_table_zero",
    "ivln_mapper_debug_nonzero": "test_dangling_begin_then_reset",
}
