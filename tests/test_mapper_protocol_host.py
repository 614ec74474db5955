"""CPU companion of tests/test_gpu_mapper_protocol.py: a model of the mapper's arg-max table ITSELF - slot -> packed value,
atomicMax, the winner clears its slot - built from the restated arithmetic of tests/test_mapper_step_coverage.py (make_key,
table_slots, the local cloud extended by the pixel index) plus ord_f32 and the two packed forms of csrc/mapper.hip:

  local pass   packed = ord_f32(height) << 32 | (0xFFFFFFFF - pixel)        (k_local_argmax / k_local_select)
  world pass   packed = ord_f32(height) << 32 | ~rank                       (k_world_max / k_world_select)
               rank = 2^31 | local key for a point appended this step, = its world key of the last step otherwise

The model is validated first: with a table that starts all zero it keeps, after every step, exactly the points of
model_run(tag) (hand-built transforms) and of the C oracle (the transforms derived from pose and orientation, which the GPU
sequences step on - their fmaf chain is restated in float64, exact for a product of two fp32 values).  Then the GPU file's
sequences are proven not to be vacuous: step A's local arg-max is entered and NOT cleared - a begin that is never finished,
behind a reset that leaves the table alone - and the walk behind it must lose points against the clean model, in its
first step's local pass and still after its last step.

Figures.  Two steps of a case are unrelated frames - 100 to 600 survivors in a key space of tens of thousands of slots -,
so a forgotten arg-max meets a later frame in a handful of slots or in none: 6 of the 27 ordered pairs of the cases' own
steps lose anything in B's local pass, 1 to 3 points.  The GPU file lists three of those and, for every case, the pair that
is not marginal: A = B's own frame from a camera 1 cm higher (what a capture's example frame is to the first frame stepped),
which costs B every survivor it has.  PARENT_LOST holds what the commit before the fix lost on an MI355X (its library with
only the probe added) in test_dangling_begin_then_reset and in the mid-walk variant: the model predicts every figure."""
import functools
import os
import re

import numpy as np
import pytest

import test_gpu_mapper_protocol as G
import test_gpu_mapper_step_kernels as K
import test_mapper_step_coverage as P

f32 = np.float32
u64 = np.uint64
LOCAL_RANK_BIT = 1 << 31


# ----------------------------------------------------------------------------------------------------------------------
# restatements
# ----------------------------------------------------------------------------------------------------------------------
def ord_f32(h):
    """orderable bits of a height: -0 folds to +0, negatives are complemented, the rest get the top bit"""
    u = (np.asarray(h, f32) + f32(0.0)).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000).astype(u64)


def packed_local(y, pix):
    return (ord_f32(y) << u64(32)) | (0xFFFFFFFF - np.asarray(pix, np.int64)).astype(u64)


def packed_world(y, rank):
    return (ord_f32(y) << u64(32)) | (~np.asarray(rank, np.int64) & 0xFFFFFFFF).astype(u64)


def _fma(a, b, acc):
    """fmaf(a, b, acc) for fp32 operands: the product is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + acc.astype(np.float64)).astype(f32)


def local_cloud(c, s, T):
    """P.local_points for ANY transform, extended by the pixel index: (pix, b, x, y, z, label) of the filtered local cloud
    in pixel order (unproject of csrc/mapper.hip: a product, three fmaf, the origin shift, the height window)"""
    xs, ys = P.scales(c.H, c.W, c.vfov_rad)
    d, B = s["depth"], s["B"]
    ok = (d > f32(0.01)) & (d < f32(0.99))
    with np.errstate(invalid="ignore"):
        z = d * f32(10.0)
        x, y = z * xs[None, None, :], z * ys[None, :, None]
        x, y = np.broadcast_to(x, d.shape).astype(f32), np.broadcast_to(y, d.shape).astype(f32)
        T = np.asarray(T, f32)
        w = []
        for r in range(3):
            t = [np.broadcast_to(T[:, r, k].reshape(B, 1, 1), d.shape) for k in range(4)]
            acc = t[0] * x
            acc = _fma(t[1], y, acc)
            acc = _fma(t[2], z, acc)
            acc = _fma(t[3], np.ones_like(z), acc)
            w.append(acc - f32(0.0))
        h = s["pose"][:, 1].reshape(B, 1, 1)
        ok &= (w[1] > h - f32(1.0)) & (w[1] < h + f32(0.5))
    b = np.broadcast_to(np.arange(B).reshape(B, 1, 1), d.shape)
    pix = np.arange(d.size).reshape(d.shape)
    return pix[ok].astype(np.int64), b[ok].astype(np.int64), w[0][ok], w[1][ok], w[2][ok], s["labels"][ok]


class Table:
    """the mapper's state between calls: the table and the world cloud (b, x, y, z, label, rank)"""

    def __init__(self, c):
        self.c, self.half_res = c, f32(c.map[2] / 2)
        self.tab = np.zeros(c.table, u64)
        self.W = [np.zeros(0, np.int64)] + [np.zeros(0, f32)] * 3 + [np.zeros(0, np.uint8), np.zeros(0, np.int64)]

    def _slots(self, b, x, z):
        r, cc = P.cells(z, self.half_res), P.cells(x, self.half_res)
        mm = (int(r.min()), int(cc.min()), int(r.max()), int(cc.max()))
        keys = P.make_key(b, r, cc, mm)
        return keys, P.table_slots(keys, mm[3] - mm[1], self.c.table)

    def _select(self, slots, packed):
        """atomicMax of every candidate, then the candidates that find their own value win and clear the slot"""
        assert (slots >= 0).all()
        np.maximum.at(self.tab, slots, packed)
        win = self.tab[slots] == packed
        self.tab[slots[win]] = 0
        return win

    def begin(self, s, T):
        """k_local_argmax alone: the entries stay"""
        pix, b, x, y, z, _lab = local_cloud(self.c, s, T)
        if len(pix):
            _keys, slots = self._slots(b, x, z)
            np.maximum.at(self.tab, slots, packed_local(y, pix))

    def reset(self, clear_table):
        self.W = [a[:0] for a in self.W]
        if clear_table:
            self.tab[:] = 0

    def step(self, s, T):
        """one complete step -> (local survivors as a set of pixels, the world in rank order)"""
        B = s["B"]
        pix, b, x, y, z, lab = local_cloud(self.c, s, T)
        alive = (self.W[0] < B) & (s["not_done"][np.minimum(self.W[0], B - 1)] != 0)
        W = [a[alive] for a in self.W]
        kept = np.zeros(0, np.int64)
        if len(pix):
            keys, slots = self._slots(b, x, z)
            win = self._select(slots, packed_local(y, pix))
            kept = pix[win]
            new = [b[win], x[win], y[win], z[win], lab[win], keys[win] | LOCAL_RANK_BIT]
            W = [np.concatenate([a, n]) for a, n in zip(W, new)]
        if len(W[0]):
            keys, slots = self._slots(W[0], W[1], W[3])
            win = self._select(slots, packed_world(W[2], W[5]))
            W = [a[win] for a in W[:5]] + [keys[win]]
            order = np.argsort(W[5], kind="stable")
            W = [a[order] for a in W]
        self.W = W
        return set(kept.tolist()), W

    def dirty(self):
        return int((self.tab != 0).sum())


def transforms(s, posed):
    return K.step_transforms(s, posed)


def _same_world(W, xyz, b, lab):
    return (np.array_equal(W[1].view(np.uint32), xyz[:, 0].view(np.uint32)) and np.array_equal(W[2].view(np.uint32), xyz[:, 1].view(np.uint32))
            and np.array_equal(W[3].view(np.uint32), xyz[:, 2].view(np.uint32)) and np.array_equal(W[0], b) and np.array_equal(W[4], lab))


# ----------------------------------------------------------------------------------------------------------------------
# the model of the table is the step, to the bit
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", K.ENTRY_CASES)
def test_table_model_equals_the_step_model_and_the_oracle(tag):
    c = K.case(tag)
    mod = P.model_run(tag)
    for posed, ref in ((False, K.oracle_run(tag, False)), (True, K.oracle_run(tag, True))):
        tb = Table(c)
        for t, s in enumerate(c.steps):
            kept, W = tb.step(s, transforms(s, posed)[0])
            assert tb.dirty() == 0, (tag, posed, t)                      # the winners leave the table clean
            assert _same_world(W, ref[t]["xyz"], ref[t]["b"], ref[t]["lab"]), (tag, posed, t)
            if not posed:                                                # ... and the survivors are model_run's
                m = mod[t]
                assert len(kept) == m["nl"] and _same_world(W, np.stack(m["W"][1:4], 1), m["W"][0], m["W"][4]), (tag, t)


# ----------------------------------------------------------------------------------------------------------------------
# the GPU sequences are not vacuous
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def poisoned_walk(tag, a, first, lift=0.0):
    """begin(A) that is never finished, a reset that leaves the table alone, then the walk from `first` ->
    (stale entries, local survivors of the walk's first step: all and suppressed, world points missing behind every step)"""
    c = K.case(tag)
    clean, bad = Table(c), Table(c)
    sa = G.step_a(tag, a, lift)
    bad.begin(sa, transforms(sa, True)[0])
    entries = bad.dirty()
    bad.reset(clear_table=False)
    suppressed, missing = None, []
    for s in c.steps[first:]:
        T = transforms(s, True)[0]
        k0, W0 = clean.step(s, T)
        k1, W1 = bad.step(s, T)
        if suppressed is None:
            suppressed, nl = len(k0 - k1), len(k0)
            assert k1 <= k0
        missing.append(len(W0[0]) - len(W1[0]))
    return entries, nl, suppressed, missing


# what the parent commit's library (+ the probe alone) lost on an MI355X in test_dangling_begin_then_reset, per pair of
# G.DANGLING: world points short of the oracle behind every step of the walk.  The model must predict exactly these.
PARENT_LOST = {
    ("rag-seq-323", 2, 0, 0.0): [3, 4, 4, 4], ("rag-seq-323", 0, 1, 0.0): [1, 3, 4], ("b33-4x4", 1, 0, 0.0): [3, 3],
    ("rag-24x20-b3of5", 0, 0, 0.01): [436, 430, 429], ("rag-5x13-b3of5", 0, 0, 0.01): [118, 118, 118],
    ("rag-seq-323", 0, 0, 0.01): [455, 298, 300, 301], ("rag-seq-15", 0, 0, 0.01): [38, 38, 38], ("b64-4x4", 0, 0, 0.01): [580, 579],
    ("b33-4x4", 0, 0, 0.01): [297, 299], ("hts-signs", 0, 0, 0.01): [453, 450, 452],
    # the mid-walk reset behind begin(step 2) (steps 0 and 1 complete in front of it)
    ("rag-24x20-b3of5", 2, 0, 0.0): [0, 7, 7], ("rag-5x13-b3of5", 2, 0, 0.0): [0, 0, 0], ("rag-seq-15", 2, 0, 0.0): [0, 0, 0],
    ("hts-signs", 2, 0, 0.0): [0, 3, 2],
}


def test_every_dangling_pair_of_the_gpu_file_loses_points_in_the_model():
    pairs = list(G.DANGLING) + [(tag, G.MID_RESET[0], 0, G.MID_RESET[1]) for tag in G.MID_CASES]
    assert {p[0] for p in pairs} == set(K.ENTRY_CASES)
    for tag, a, first, lift in pairs:
        c = K.case(tag)
        assert (a != first or lift != 0.0) and len(c.steps) - first >= 2        # A and B differ; two complete steps follow
        entries, nl, suppressed, missing = poisoned_walk(tag, a, first, lift)
        print(f"{tag:18s} A = step {a} + {lift} m, walk from step {first}: {entries} stale entries, {suppressed} of {nl} local "
              f"survivors of B suppressed, world points missing per step {missing}")
        assert entries > 0 and suppressed >= 1 and missing[-1] >= 1, (tag, a, first, lift)
        if lift:   # the same slots, every stale entry above B's candidate: B keeps nothing, and the walk never recovers it
            assert suppressed == nl and missing[0] == nl and min(missing) >= nl // 4, (tag, suppressed, nl, missing)
        assert missing == PARENT_LOST[(tag, a, first, lift)], (tag, missing)


def test_the_mid_walk_reset_behind_step_2_is_modelled():
    """steps 0 and 1 complete, begin(step 2) abandoned, a reset that leaves the table alone, a fresh walk from step 0 (the GPU
    file's `reset-step2`): the table holds what begin(2) entered, whatever steps 0 and 1 did before - they left it clean.
    Unrelated frames: the model's losses are printed, and are the figures PARENT_LOST holds where the pair is listed."""
    for tag in G.MID_CASES:
        entries, nl, suppressed, missing = poisoned_walk(tag, 2, 0)
        print(f"{tag:18s} begin(step 2), fresh walk from step 0: {entries} stale entries, {suppressed} of {nl} local survivors "
              f"suppressed, world points missing per step {missing}")
        assert entries > 0 and all(0 <= k <= 8 for k in missing)
        assert missing == PARENT_LOST[(tag, 2, 0, 0.0)]


def test_unrelated_frames_rarely_collide():
    """every ordered pair (A, first) of every case's own steps: most lose nothing - why DANGLING lists the pairs it does"""
    hit = total = 0
    for tag in K.ENTRY_CASES:
        n = len(K.case(tag).steps)
        for a in range(n):
            for first in range(n - 1):
                if a != first:
                    _e, _nl, suppressed, missing = poisoned_walk(tag, a, first)
                    total += 1
                    hit += suppressed >= 1 and missing[-1] >= 1
    print(f"{hit} of {total} ordered pairs of the cases' own steps lose points in B's local pass and stay short")
    assert 3 <= hit < total


def test_a_cleared_table_loses_nothing():
    """the same sequences with the reset the header promises: every step equals the clean model"""
    for tag, a, first, lift in G.DANGLING:
        c = K.case(tag)
        tb = Table(c)
        sa = G.step_a(tag, a, lift)
        tb.begin(sa, transforms(sa, True)[0])
        assert tb.dirty() > 0
        tb.reset(clear_table=True)
        ref = K.oracle_run(tag, True, first)
        for t, s in enumerate(c.steps[first:]):
            _kept, W = tb.step(s, transforms(s, True)[0])
            assert _same_world(W, ref[t]["xyz"], ref[t]["b"], ref[t]["lab"]) and tb.dirty() == 0, (tag, t)


# ----------------------------------------------------------------------------------------------------------------------
# who touches the table, and who is refused
# ----------------------------------------------------------------------------------------------------------------------
def _mapper_src():
    return open(os.path.join(P.ROOT, "ivln-ce_amd", "csrc", "mapper.hip")).read()


def table_users(src):
    """host functions of mapper.hip whose body hands m->tab64 to a launch or a memset (hipFree is neither)"""
    host = src[src.index("struct ivln_mapper {"):]
    users = set()
    heads = list(re.finditer(r"^(?:static\s+)?int\s+(\w+)\s*\(", host, flags=re.M))
    for i, h in enumerate(heads):
        body = host[h.start():heads[i + 1].start() if i + 1 < len(heads) else len(host)]
        body = re.sub(r"//[^\n]*", "", body)
        calls = re.findall(r"(hipLaunchKernelGGL|hipMemset(?:Async)?)\s*\(((?:[^()]|\([^()]*\))*)\)", body)
        handed = any("m->tab64" in args for _f, args in calls) or bool(re.search(r"=\s*\{[^}]*m->tab64", body))
        if handed:
            users.add(h.group(1))
    return users


def _uncovered(names, table):
    no_entry = sorted(n for n in names if n not in table)
    no_test = sorted(n for n, t in table.items() if not callable(getattr(G, t, None)) or not t.startswith("test_"))
    return no_entry, no_test


def test_the_tables_users_are_pinned_and_each_has_a_sequence():
    users = table_users(_mapper_src())
    assert users == {"ivln_mapper_create", "ivln_mapper_reset", "mapper_begin", "mapper_finish", "env_compact",
                     "ivln_mapper_debug_nonzero"}
    assert _uncovered(users, G.TABLE_USERS) == ([], []) and set(G.TABLE_USERS) == users
    # the scan itself: a new user is noticed, a comment is not
    more = _mapper_src() + "\nint ivln_new_thing(ivln_mapper* m) {\n    hipMemsetAsync(m->tab64, 0, 8, 0);\n    return 0;\n}\n"
    assert table_users(more) == users | {"ivln_new_thing"}
    assert table_users(_mapper_src() + "\nint ivln_quiet(ivln_mapper* m) {\n    // hipMemset(m->tab64, 0, 8);\n    return 0;\n}\n") == users
    # the probe's kernel sits behind the marker that pins the step's kernel list
    src = _mapper_src()
    assert src.index("void k_debug_nonzero") > src.index("// ---- known-map mode ----")


def refused_in_header():
    """the entry points the contract of ivln_mapper_step_begin (include/ivln_hip.h) names as refused while open"""
    hdr = open(os.path.join(P.ROOT, "include", "ivln_hip.h")).read()
    text = hdr[hdr.index("Open state."):]
    text = " ".join(text[:text.index("*/")].replace("*", " ").split())
    sentence = text[text.index("launches nothing and writes nothing:"):]
    sentence = sentence[:sentence.index(".")]
    names = set()
    for m in re.finditer(r"(ivln_\w+)((?:\s*/\s*_\w+)*)", sentence):
        names.add(m.group(1))
        for alt in re.findall(r"_\w+", m.group(2)):
            names.add(m.group(1)[:m.group(1).rindex("_")] + alt)
    if "a second _begin" in sentence:
        names.add("ivln_mapper_step_begin")
    return names


def test_every_refused_entry_point_names_a_test():
    names = refused_in_header()
    assert names == {"ivln_mapper_step_begin", "ivln_mapper_step", "ivln_mapper_step_posed", "ivln_mapper_env_export",
                     "ivln_known_lib_add_from_mapper", "ivln_mapper_env_append", "ivln_mapper_env_append_from_lib",
                     "ivln_mapper_rows_clear"}
    assert _uncovered(names, G.REFUSED) == ([], []) and set(G.REFUSED) == names
    short = dict(G.REFUSED)
    short.pop("ivln_mapper_rows_clear")
    assert _uncovered(names, short)[0] == ["ivln_mapper_rows_clear"]      # removing a key is noticed
    assert _uncovered(names, dict(G.REFUSED, ivln_mapper_step="test_that_is_not_there"))[1] == ["ivln_mapper_step"]
    # each of them tests the open flag in front of its first launch
    src = _mapper_src()
    for n in names - {"ivln_mapper_env_append", "ivln_mapper_env_append_from_lib", "ivln_mapper_rows_clear"}:
        body = src[src.index(f"int {n}("):]
        body = body[body.index("{"):body.index("\n}\n")]
        work = [body.index(w) for w in ("mapper_begin(", "mapper_step(", "env_stats(", "hipLaunchKernelGGL") if w in body]
        assert "m->open" in body and work and body.index("m->open") < min(work), n
    seed = src[src.index("static int seed_refused"):]
    assert "m->open" in seed[:seed.index("\n}\n")]
    assert G.pytestmark.name == "gpu"


def test_the_probes_header_declares_one_symbol_and_the_library_exports_it():
    import ctypes

    import __graft_entry__ as ge

    src = open(os.path.join(P.ROOT, "include", "ivln_mapper_debug.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(ivln_[a-z0-9_]+)\s*\(", src))) == ["ivln_mapper_debug_nonzero"]
    L = ctypes.CDLL(ge.build())
    assert hasattr(L, "ivln_mapper_debug_nonzero")
    out = (ctypes.c_int64 * 2)(-7, -7)
    L.ivln_mapper_debug_nonzero.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]
    assert L.ivln_mapper_debug_nonzero(None, out, None) == -1 and list(out) == [-7, -7]      # IVLN_E_INVALID, nothing written
    # the product path does not call it
    pkg = os.path.join(P.ROOT, "ivln-ce_amd")
    users = [f for f in os.listdir(pkg) if f.endswith(".py") and "ivln_mapper_debug_nonzero" in open(os.path.join(pkg, f)).read()]
    assert users == ["_lib.py"]
