"""CPU: the plan arithmetic of csrc/gn_conv.hip's two launchers and of partial_conv's tile / waves-per-tile choice, restated
in plain Python, and what it says about the cases of tests/test_gpu_gn_conv_kernels.py (which imports gn_plan / nconv_plan
from here to hold the real launchers to them: accepted or refused, and the number of strips).

Restated (ivln-ce_amd/csrc/gn_conv.hip):
  partial_conv      lines 253-275   pixel tiles, rows per weight chunk, T, the waves-per-tile ladder, items = T * KS
  ivln_gn_conv_f32  lines 766-881   refusals, S, part_floats, fixed LDS, prestage or streamed, wave roles, per_a / per_b
  k_gn_conv         lines 373-381, 393-398   a block's channel slice and load roles (t1, vector or scalar tile loads)
  ivln_nconv_f32    lines 883-955   refusals, RS / strips / Hs, mz, part_floats, the loader-side weight waves
  k_nconv           lines 549-554, 637   a strip's rows, conv B's rows, DPP-row or looped statistics merge

The defect this file records: with fewer than 8 output tiles (T) per block, KS = 8, 4, 4, 2 waves shared a tile for
T = 1, 2, 3, 4..7 and wrote T * KS partial tiles of 1024 floats into `part`, which both launchers size at 8 * 1024 floats.
T in {3, 5, 6, 7} gave 12, 10, 12, 14 items: items 8 and up landed in the staged weights behind `part`.  `ladder_parent`
keeps that choice; `ladder` is the one the kernel has now (T << ksl <= 8).  Every shape of the depth encoder has a
power-of-two T, for which the two ladders agree - no production plan and no timing moved.

Two launcher branches that no layer of the encoder takes were found by a search over small shapes with these plans and have
cases of their own: "spare waves go to the larger slab role" (the rounded shares of the load roles sum to 7 of the 8 waves:
spare-front, spare-tile) and `part` dropped WITHOUT a front stage (nofront-nopart: a 1 x 32 map with 256 channels in one
group, second operand, residual and pooled tile together - the only way the fixed LDS without a front stage exceeds
kLdsFloats - 8192 - 2048; also cpg = GT / 2, the largest the launcher takes).
Unreached by any accepted shape:
  * k_nconv's empty partial of conv B (npx <= 0): conv B needs a stride-1 conv A and RS is a multiple of conv B's stride,
    so a strip's first row r0 < H gives r0 / sb <= (H - 1) / sb < Ho_b - every strip has at least one row of conv B.  (The
    consumer side of an empty partial is tested: the zero-part sub-cases.)"""
import types

import pytest

GT, NW, TILE_MAX, LDS, NC_E4, PART = 512, 8, 8192, 38 * 1024, 6, 8 * 1024


def r4(v):
    return (v + 3) & ~3


def padded_row(kb):
    return r4(kb) + 4


def ladder(T, hc, part):
    """waves per tile (KS) of partial_conv as it is now"""
    ksl = 0 if (T >= 8 or not part) else (1 if T >= 4 else (2 if T >= 2 else 3))
    while (1 << ksl) > hc:
        ksl -= 1
    while ksl > 0 and (T << ksl) > 8:
        ksl -= 1
    return 1 << ksl


def ladder_parent(T, hc, part):
    """THE PARENT'S ladder (before T << ksl <= 8 was enforced): kept as the record of the defect, used by no plan"""
    ksl = 0 if (T >= 8 or not part) else (1 if T >= 4 else (2 if T >= 2 else 3))
    while (1 << ksl) > hc:
        ksl -= 1
    return 1 << ksl


def conv_chunks(co_beg, co_end, HWo, Kbp, wl_floats, prestaged, hc, part, lad=ladder):
    """partial_conv's weight chunks of one block: [(rows, T, KS)]"""
    ptl = (HWo + 31) >> 5
    rows_max = co_end - co_beg
    if not prestaged:
        rows_max = wl_floats // Kbp
        if rows_max > 32:
            rows_max &= ~31
    out = []
    if rows_max <= 0:
        return out
    for cb0 in range(co_beg, co_end, rows_max):
        nrow = min(rows_max, co_end - cb0)
        T = ((nrow + 31) >> 5) * ptl
        out.append((nrow, T, lad(T, hc, part)))
    return out


def _refuse(code, why):
    return types.SimpleNamespace(ok=False, code=code, why=why)


def gn_plan(c, lad=ladder):
    """ivln_gn_conv_f32 on a case dict of tests/test_gpu_gn_conv_kernels.py (N C H W groups, a = (Cout, k, stride, pad),
    b = (Cout, stride), pool, x2 = splits2, residual, act_out, front = (C0, groups0, splits0), splits)"""
    N, C, H, W, groups = c["N"], c["C"], c["H"], c["W"], c["groups"]
    a, b, front = c.get("a"), c.get("b"), c.get("front")
    x2, res, pool = c.get("x2"), bool(c.get("residual")), bool(c.get("pool"))
    if C % groups or (not a and not b and not c.get("act_out")):
        return _refuse("invalid", "arguments")
    if front and (pool or front[0] % front[1] or front[0] & 1):
        return _refuse("invalid", "front stage")
    if a and a[1] not in (1, 3):
        return _refuse("unsupported", "kernel size")
    cpg, HW = C // groups, H * W
    nel = cpg * HW
    if nel > TILE_MAX or cpg > GT // 2:
        return _refuse("unsupported", "cpg * H * W > 8192")
    Hc, Wc = ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if pool else (H, W)
    Ho_a = Wo_a = Ho_b = Wo_b = HWo_a = HWo_b = 0
    if a:
        Ho_a, Wo_a = (Hc + 2 * a[3] - a[1]) // a[2] + 1, (Wc + 2 * a[3] - a[1]) // a[2] + 1
        if Ho_a <= 0 or Wo_a <= 0:
            return _refuse("invalid", "empty output")
        HWo_a = Ho_a * Wo_a
    if b:
        Ho_b, Wo_b = (Hc - 1) // b[1] + 1, (Wc - 1) // b[1] + 1
        HWo_b = Ho_b * Wo_b
    if (a or b) and cpg & 1:
        return _refuse("unsupported", "odd channels per group with a conv")
    S, blocks = 1, N * groups
    cmin = (b[0] if b and b[0] < a[0] else a[0]) if a else (b[0] if b else 1)
    while S < 4 and blocks * S * 2 <= 256 and cmin // (S * 2) >= 16:
        S *= 2
    per_a, per_b = (-(-a[0] // S) if a else 0), (-(-b[0] // S) if b else 0)
    nel4 = r4(nel)
    tiles_a = ((per_a + 31) // 32) * ((HWo_a + 31) // 32) if a else 8
    tiles_b = ((per_b + 31) // 32) * ((HWo_b + 31) // 32) if b else 8
    part = PART if (tiles_a < 8 or tiles_b < 8) else 0
    fixed = 64 + 4 * r4(cpg) + nel4 * (1 + (1 if x2 else 0) + (1 if res else 0)) + (r4(cpg * Hc * Wc) if pool else 0)
    if front:
        C0 = front[0]
        fixed += r4(C0 * HW) + r4(2 * C0) + cpg * (r4(C0) + 4)
        if ((cpg + 31) // 32) * ((HW + 31) // 32) < 8:
            part = PART
    wanted_part = part
    if fixed + part + 2048 > LDS:
        part = 0
    fixed += part
    if fixed + 64 > LDS:
        return _refuse("unsupported", "152 KB of LDS")
    kbp_a, kbp_b = (padded_row(cpg * a[1] * a[1]) if a else 0), (padded_row(cpg) if b else 0)
    need_a, need_b = per_a * kbp_a, per_b * kbp_b
    cap = LDS - fixed
    prestage = need_a + need_b <= cap
    wl = need_a + need_b if prestage else cap
    if wl < kbp_a or wl < kbp_b:
        return _refuse("unsupported", "152 KB of LDS")
    tb = float(nel) * ((0 if front else c["splits"]) + (x2 or 0) + (1 if res else 0))
    fb = float(front[0]) * HW * front[2] if front else 0.0
    w0b = float(cpg) * front[0] + 2.0 * front[0] if front else 0.0
    wb_ = float(need_a + need_b) if prestage else 0.0
    by, tot = [tb, fb, w0b, wb_], tb + fb + w0b + wb_
    nw = [0] * 4
    for i in range(4):
        nw[i] = int(NW * by[i] / tot + 0.5) if by[i] > 0 else 0
        if by[i] > 0 and nw[i] < 1:
            nw[i] = 1
    used = sum(nw)
    while used > NW:
        m = 0
        for i in range(1, 4):
            if nw[i] > nw[m]:
                m = i
        nw[m] -= 1
        used -= 1
    big = 0 if tb >= fb else 1
    if by[big] <= 0:
        big = 3
    spare = NW - used
    nw[big] += spare
    if by[big] <= 0:
        return _refuse("invalid", "no load role")
    if N > 65535:
        return _refuse("unsupported", "N")
    convs = {}
    if front:  # the front conv: this group's cpg rows over K = C0, prestaged, one chunk
        convs["front"] = [conv_chunks(0, cpg, HW, padded_row(front[0]), 0, True, front[0] >> 1, part, lad)]
    if a:
        convs["a"] = [conv_chunks(s * per_a, min(a[0], (s + 1) * per_a), HWo_a, kbp_a, wl, prestage, cpg >> 1, part, lad) for s in range(S)]
    if b:
        convs["b"] = [conv_chunks(s * per_b, min(b[0], (s + 1) * per_b), HWo_b, kbp_b, wl, prestage, cpg >> 1, part, lad) for s in range(S)]
    return types.SimpleNamespace(ok=True, S=S, per_a=per_a, per_b=per_b, part_floats=part, part_dropped=bool(wanted_part and not part),
                                 prestage=prestage, wl_floats=wl, lds_floats=fixed + wl, roles=tuple(nw), spare=spare,
                                 t1=GT - 64 * (nw[1] + nw[2] + nw[3]), vec=(HW & 3) == 0, cpg=cpg, Hc=Hc, Wc=Wc,
                                 out_a=(Ho_a, Wo_a), out_b=(Ho_b, Wo_b), convs=convs)


def nconv_plan(c, lad=ladder):
    """ivln_nconv_f32 on a case dict (N C H W, groups / parts or None for a plain input, a = (Cout, k, groups_a, stride),
    b = (Cout, groups_b, stride), x2 = parts2, residual, act_out, rows_per_block)"""
    N, C, H, W = c["N"], c["C"], c["H"], c["W"]
    groups, parts, x2 = c.get("groups") or 0, c.get("parts") or 0, c.get("x2") or 0
    a, b, res, rpb = c["a"], c.get("b"), bool(c.get("residual")), c.get("rows_per_block", 0)
    stats = groups > 0
    if stats and C % groups:
        return _refuse("invalid", "arguments")
    if a[0] % a[2] or (b and b[0] % b[1]):
        return _refuse("invalid", "arguments")
    ka, sa, sb = a[1], a[3], (b[2] if b else 1)
    if ka not in (1, 3) or W & 3 or C & 1 or groups > 32 or N > 65535 or sa > 2 or sb > 2:
        return _refuse("unsupported", "k, W % 4, odd C or groups > 32")
    if c.get("act_out") and sa != 1:
        return _refuse("unsupported", "act_out beside a stride-2 conv A")
    if b and sa != 1:
        return _refuse("unsupported", "conv B beside a stride-2 conv A")
    ph = ka // 2
    Ho_a, Wo_a = (H + 2 * ph - ka) // sa + 1, (W + 2 * ph - ka) // sa + 1
    Ho_b, Wo_b = ((H - 1) // sb + 1, (W - 1) // sb + 1) if b else (0, 0)
    if Wo_a & 3 or (b and Wo_b & 3):
        return _refuse("unsupported", "Wo % 4")
    Cp, cpo_a, cpo_b = r4(C), a[0] // a[2], (b[0] // b[1] if b else 1)
    pfl = (r4(parts * groups * 3) if stats else 0) + (r4(x2 * groups * 3) if x2 else 0)
    kbp_a, kbp_b = r4(C * ka * ka) + 4, (r4(C) + 4 if b else 0)
    rs = rpb if rpb > 0 else (1 if Wo_a >= 64 else 64 // Wo_a)
    halvings, fl, part, mz, per_a, per_b = 0, 0, 0, 1, 0, 0
    while True:
        if rs < 1:
            return _refuse("unsupported", "152 KB of LDS")
        RS = min(rs, Ho_a)
        if b and RS % sb:
            RS = (RS + sb - 1) // sb * sb
        RSb = RS // sb if b else 0
        strips = (Ho_a + RS - 1) // RS
        Hs = (RS - 1) * sa + ka
        strip = C * Hs * W
        base = 64 + pfl + 4 * r4(groups) + 8 * Cp + r4(strip)
        ok, mz = False, 1
        while True:
            per_a, per_b = -(-a[0] // mz), (-(-b[0] // mz) if b else 0)
            whole = mz == 1 or (per_a % cpo_a == 0 and per_a % 32 == 0 and a[0] % per_a == 0 and
                                (not b or (per_b % cpo_b == 0 and per_b % 32 == 0 and b[0] % per_b == 0)))
            if not whole:
                break
            tiles_a = ((per_a + 31) // 32) * ((RS * Wo_a + 31) // 32)
            tiles_b = ((per_b + 31) // 32) * ((RSb * Wo_b + 31) // 32) if b else NW
            part = PART if (tiles_a < NW or tiles_b < NW) else 0
            fl = base + r4(per_a * RS * Wo_a) + (r4(per_b * RSb * Wo_b) if b else 0) + per_a * kbp_a + (per_b * kbp_b if b else 0)
            wanted_part = part
            if fl + part > LDS and fl <= LDS:
                part = 0
            fits = fl + part <= LDS
            more = strips * N * mz * 2 <= 256 and per_a >= 64 and per_a % 64 == 0 and (not b or per_b % 64 == 0)
            if fits and not more:
                ok = True
                break
            if mz >= 16:
                ok = fits
                break
            mz *= 2
        if ok and (GT - 64) * NC_E4 * 4 < strip:
            ok = False
        if ok:
            break
        if rpb > 0:
            return _refuse("unsupported", "rows_per_block does not fit")
        rs //= 2
        halvings += 1
    wfl = per_a * kbp_a + (per_b * kbp_b if b else 0)
    nw0 = int(NW * wfl / float(wfl + strip * (1 + (1 if x2 else 0) + (1 if res else 0))) + 0.5)
    nw0 = 1 if nw0 < 1 else min(nw0, NW - 2)
    nw = nw0
    while nw > 1 and (GT - 64 * nw) * NC_E4 * 4 < strip:
        nw -= 1
    if (GT - 64 * nw) * NC_E4 * 4 < strip:
        return _refuse("unsupported", "152 KB of LDS")
    convs = {"a": [], "b": []}
    for s in range(strips):
        rows = min(RS, Ho_a - s * RS)
        rows_b = min(RSb, Ho_b - s * RS * sa // sb) if b else 0
        for z in range(mz):
            if min(a[0], (z + 1) * per_a) > z * per_a:
                convs["a"].append(conv_chunks(z * per_a, min(a[0], (z + 1) * per_a), rows * Wo_a, kbp_a, 0, True, C >> 1, part, lad))
            if b and min(b[0], (z + 1) * per_b) > z * per_b and rows_b > 0:
                convs["b"].append(conv_chunks(z * per_b, min(b[0], (z + 1) * per_b), rows_b * Wo_b, kbp_b, 0, True, C >> 1, part, lad))
    if not b:
        del convs["b"]
    merge = lambda p: "dpp" if (p <= 16 and groups <= 16) else "loop"  # noqa: E731
    return types.SimpleNamespace(ok=True, RS=RS, RSb=RSb, strips=strips, Hs=Hs, mz=mz, per_a=per_a, per_b=per_b, part_floats=part,
                                 part_dropped=bool(wanted_part and not part), halvings=halvings, nw0=nw0, nw=nw,
                                 lds_floats=fl + part, out_a=(Ho_a, Wo_a), out_b=(Ho_b, Wo_b), convs=convs,
                                 merge=(merge(parts) if stats else None), merge2=(merge(x2) if x2 else None))


def _items(plan):
    """(largest T * KS of a block that shares tiles, all (T, KS) met) over every conv, slice and chunk of a plan"""
    worst, seen = 0, set()
    for name, blocks in plan.convs.items():
        for chunks in blocks:
            for _, T, KS in chunks:
                seen.add((name, T, KS))
                if KS > 1:
                    worst = max(worst, T * KS)
    return worst, seen


def _T(plan, name):
    return sorted({T for n, T, _ in _items(plan)[1] if n == name})


def _cases():
    import test_gpu_gn_conv_kernels as K

    return K


# what each tag names (the issue's table): attribute -> value of the plan, or a callable on (plan, parent's items)
GN_EDGES = {
    "t3": lambda p: p.S == 2 and _T(p, "a") == [3] and not p.vec,
    "t5": lambda p: _T(p, "a") == [5] and p.cpg == 4 and p.vec,
    "t7": lambda p: p.S == 1 and _T(p, "a") == [7] and p.per_a == 20,
    "b3": lambda p: _T(p, "a") == [16] and _T(p, "b") == [3] and ("a", 16, 1) in _items(p)[1] and ("b", 3, 2) in _items(p)[1],
    "stream": lambda p: (not p.prestage and p.S == 4 and p.per_a == 50 and p.per_b == 18 and [r for r, _, _ in p.convs["a"][0]] == [32, 18]
                         and p.lds_floats == LDS),
    "ragged-S": lambda p: (p.S == 4 and p.per_a == 17 and [sum(r for r, _, _ in ch) for ch in p.convs["a"]] == [17, 17, 17, 15]
                           and _items(p)[1] == {("a", 1, 1)} and p.cpg == 2 and p.part_floats == PART),
    "pool": lambda p: (p.Hc, p.Wc) == (7, 6) and not p.vec and "a" in p.convs and "b" in p.convs,
    "act-only": lambda p: p.cpg == 3 and not p.convs,
    "front3": lambda p: _T(p, "front") == [3] and _T(p, "a") == [3] and p.t1 == 0 and p.roles[0] == 0,
    "front-nopart": lambda p: p.part_dropped and p.part_floats == 0 and max(_T(p, "front") + _T(p, "a")) < 8 and _items(p)[0] == 0,
    "front-x2": lambda p: "a" not in p.convs and "b" in p.convs and "front" in p.convs and p.roles[0] > 0,
    "spare-front": lambda p: p.spare == 1 and p.roles == (0, 6, 1, 1),
    "spare-tile": lambda p: p.spare == 1 and p.roles == (3, 2, 1, 2),
    "nofront-nopart": lambda p: p.part_dropped and "front" not in p.convs and p.cpg == GT // 2 and _items(p)[1] == {("a", 1, 1)},
}
NCONV_EDGES = {
    "n-t6": lambda p: p.strips == 1 and _T(p, "a") == [6] and p.merge == "dpp",
    "n-t5": lambda p: _T(p, "a") == [5],
    "n-t3": lambda p: _T(p, "a") == [3] and p.RS == 7 and (p.RS * p.out_a[1]) % 32 != 0,
    "n-loop17": lambda p: p.merge == "loop" and p.RS == 16 and p.strips == 2,
    "n-dpp16": lambda p: p.merge == "dpp" and p.RS == 16 and p.strips == 2,
    "n-g32": lambda p: p.merge == "loop" and p.mz == 2,
    "n-b-odd": lambda p: p.RS == 8 and p.RS > p.out_a[0] and p.RSb == 4 and p.strips == 1,
    "n-s2-odd": lambda p: p.out_a == (5, 4),
    "n-w64": lambda p: p.RS == 1 and p.strips == 8 and (p.nw0, p.nw) == (5, 2),
    "n-halved": lambda p: p.halvings == 1 and p.part_dropped and p.mz == 2 and p.nw == 1,
    "n-plain": lambda p: p.merge is None and "b" in p.convs,
    "n-x2-res": lambda p: p.merge == "dpp" and p.merge2 == "dpp",
}
# T * KS of the parent's ladder at the tagged cases (conv -> items): the defect
PARENT_ITEMS = {"t3": 12, "t5": 10, "t7": 14, "b3": 12, "front3": 12, "n-t6": 12, "n-t5": 10, "n-t3": 12}


def test_every_case_reaches_the_edge_its_tag_names():
    K = _cases()
    assert sorted(c["tag"] for c in K.GN_CASES) == sorted(GN_EDGES) and sorted(c["tag"] for c in K.NCONV_CASES) == sorted(NCONV_EDGES)
    for c in K.GN_CASES:
        p = gn_plan(c)
        assert p.ok and GN_EDGES[c["tag"]](p), (c["tag"], vars(p))
    for c in K.NCONV_CASES:
        p = nconv_plan(c)
        assert p.ok and NCONV_EDGES[c["tag"]](p), (c["tag"], vars(p))
    # input slab counts (slab_sum): the unrolled 16, the first slab + one group of four (5), that + a tail (6), the tail
    # only (3), a single slab
    splits = {c["splits"] for c in K.GN_CASES if not c.get("front")} | {c["front"][2] for c in K.GN_CASES if c.get("front")}
    assert {1, 3, 5, 6, 16} <= splits
    assert all(c["x2"] != c.get("splits") for c in K.GN_CASES if c.get("x2"))


def test_refusal_shapes_sit_on_either_side_of_each_reason():
    K = _cases()
    for c in K.GN_REFUSALS:
        p = gn_plan(c)
        assert p.ok == (c["why"] is None), (c["tag"], vars(p))
        if not p.ok:
            assert p.code == "unsupported" and p.why == c["why"], (c["tag"], p.why)
    for c in K.NCONV_REFUSALS:
        p = nconv_plan(c)
        assert p.ok == (c["why"] is None), (c["tag"], vars(p))
        if not p.ok:
            assert p.code == "unsupported" and p.why == c["why"], (c["tag"], p.why)
    whys = {c["why"] for c in K.GN_REFUSALS + K.NCONV_REFUSALS}
    assert whys >= {None, "cpg * H * W > 8192", "odd channels per group with a conv", "152 KB of LDS", "k, W % 4, odd C or groups > 32",
                    "Wo % 4", "act_out beside a stride-2 conv A", "conv B beside a stride-2 conv A", "rows_per_block does not fit"}


def _encoder_shapes():
    """the layer shapes tests/test_gpu_gn_conv.py runs, as case dicts: (gn cases, nconv cases)"""
    import test_gpu_gn_conv as E

    gn = [dict(N=N, C=C, H=H, W=W, groups=16, splits=s, a=ca, b=cb, x2=(4 if tail == "second" else None), residual=tail == "residual",
               act_out=True) for N, C, H, W, s, ca, cb, tail in E._SHAPES]
    gn.append(dict(N=3, C=32, H=64, W=64, groups=16, splits=2, a=(32, 1, 1, 0), b=(128, 1), pool=True, act_out=True))
    mark = [m for m in E.test_two_conv_layers_per_launch_front_stage.pytestmark if m.name == "parametrize"][0]
    for N, C0, H, W, C, ca, cb, tail in mark.args[1]:
        gn.append(dict(N=N, C=C, H=H, W=W, groups=16, splits=0, a=ca, b=cb, x2=(16 if tail == "second" else None),
                       residual=tail == "residual", act_out=True, front=(C0, 16, 16)))
    mark = [m for m in E.test_conv_with_groupnorm_on_load_and_statistics_out.pytestmark if m.name == "parametrize"][0]
    nc = []
    for N, C, H, W, ca, cb, mode in mark.args[1]:
        groups = 16 if C % 32 == 0 else 8
        rs = 5 if H == 8 else 0
        rows_in = min(max(1, 64 // W) if rs == 0 else rs, H)
        parts = (H + rows_in - 1) // rows_in
        ga = 16 if ca[0] % 32 == 0 else (2 if ca[0] % 2 == 0 else 1)
        sa = ca[2] if len(ca) > 2 else 1
        # (ops.nconv hands the launcher an explicit rows_per_block: 64 output pixels unless the test asks)
        Wo = (W - 1) // sa + 1
        rpb = rs if rs else min(1 if Wo >= 64 else 64 // Wo, (H - 1) // sa + 1)
        b = None if cb is None else (cb[0], 16 if cb[0] % 32 == 0 else 2, cb[2] if len(cb) > 2 else 1)
        if b and rpb % b[2]:
            rpb = (rpb + b[2] - 1) // b[2] * b[2]
        plain = mode == "plain_in"
        case = dict(N=N, C=C, H=H, W=W, groups=None if plain else groups, parts=None if plain else parts, a=(ca[0], ca[1], ga, sa), b=b,
                    x2=(parts if mode == "gn_second" else None), residual=mode == "gn_residual", act_out=not plain and sa == 1,
                    rows_per_block=rpb)
        while rs == 0 and not nconv_plan(case).ok and case["rows_per_block"] > (b[2] if b else 1):   # (and halves it while refused)
            case["rows_per_block"] //= 2
        nc.append(case)
    return gn, nc


def test_partial_tiles_fit_their_scratch_everywhere_and_the_parents_did_not():
    K = _cases()
    enc_gn, enc_nc = _encoder_shapes()
    assert len(enc_gn) == 24 and len(enc_nc) == 10
    every = [(c, gn_plan) for c in K.GN_CASES + enc_gn + [c for c in K.GN_REFUSALS if c["why"] is None]]
    every += [(c, nconv_plan) for c in K.NCONV_CASES + enc_nc + [c for c in K.NCONV_REFUSALS if c["why"] is None]]
    shared = 0
    for c, plan in every:
        p = plan(c)
        assert p.ok, c
        worst, seen = _items(p)
        assert worst * 1024 <= p.part_floats, (c, worst, p.part_floats)   # T * KS * 1024 <= part_floats whenever KS > 1
        assert all(KS == 1 for _, _, KS in seen) or p.part_floats == PART
        shared += worst > 0
    assert shared >= 20
    # the parent's ladder: the tagged cases overran `part` (12, 10, 14, ... partial tiles for 8 places) ...
    got = {}
    for c, plan in [(c, gn_plan) for c in K.GN_CASES] + [(c, nconv_plan) for c in K.NCONV_CASES]:
        worst = _items(plan(c, ladder_parent))[0]
        if worst > 8:
            got[c["tag"]] = worst
    assert got == PARENT_ITEMS
    # ... and the encoder's own shapes never did, which is why no rollout met it: same plans under both ladders
    for c, plan in [(c, gn_plan) for c in enc_gn] + [(c, nconv_plan) for c in enc_nc]:
        old, new = plan(c, ladder_parent), plan(c)
        assert _items(old)[0] <= 8
        if not (c["C"] == 64 and c["H"] == 7) and not (c["C"] == 96 and c.get("front")):   # (that file's two odd-size shapes)
            assert _items(old)[1] == _items(new)[1], c


@pytest.mark.parametrize("hc", [1, 2, 4, 8, 64])
def test_new_ladder_equals_the_parents_at_power_of_two_tile_counts(hc):
    for part in (0, PART):
        for T in (1, 2, 4, 8, 16, 32):
            assert ladder(T, hc, part) == ladder_parent(T, hc, part)
        for T in range(1, 40):
            KS = ladder(T, hc, part)
            assert KS <= max(1, hc) and (KS == 1 or (part and T * KS <= 8)) and KS <= ladder_parent(T, hc, part)
    assert [ladder(T, 64, PART) for T in range(1, 9)] == [8, 4, 2, 2, 1, 1, 1, 1]
    assert [ladder_parent(T, 64, PART) * T for T in range(1, 9)] == [8, 8, 12, 8, 10, 12, 14, 8]
