"""Which launches of the two K-split kernels of csrc/conv_bf3.hip take four waves per workgroup (two co-resident workgroups per
CU) instead of eight: the rule of bf3_ks_four_waves restated in plain Python and held, at 256 CUs, to the measured table
committed as profiles/coresident_ks_sweep.txt - the shapes recorded there as winners of the four-wave form, and only those,
take it; one-round grids stay on eight waves.  And the LDS of every four-wave instantiation, read from the source as
tests/test_conv_bf3_plan_coverage.py reads its tables: two such workgroups fit a CU's 160 KB.  No GPU."""
import os
import re

import test_conv_bf3_plan_coverage as P

CUS = 256
LDS_CU = 160 * 1024
SWEEP = os.path.join(P.ROOT, "profiles", "coresident_ks_sweep.txt")


def four_waves(wgs, nch, cus, nw_pin=0):
    """bf3_ks_four_waves: a pinned wave count (tile_override 16 / 17, 18 / 19), else more workgroups than CUs, at most twice as
    many, and two chunks for each of the four waves"""
    if nw_pin:
        return nw_pin == 4
    return cus < wgs <= 2 * cus and nch >= 2 * 4


def grid(form, M, N, K):
    """(workgroups of the eight-wave grid, 16-channel chunks) of a K-split launch: 32 channels x 64 pixels (3x3, stacked 2x2)
    or x 128 pixels (1x1) per workgroup"""
    KS = {"3x3": 3, "2x2": 2, "1x1": 1}[form]
    assert K % (KS * KS * P.CB) == 0
    px = 128 if KS == 1 else 64
    return P.cdiv(N, px) * P.cdiv(M, 32), K // (KS * KS * P.CB)


def sweep_rows():
    rows = []
    for line in open(SWEEP):
        m = re.match(r"shape: (3x3|2x2|1x1) (\d+) x (\d+) x (\d+) \|.*\| workgroups +(\d+) chunks +(\d+) \| 8 waves +([\d.]+) \| 4 waves +([\d.]+) \|"
                     r".*\| winner (4|8)$", line.rstrip())
        if m:
            rows.append(dict(form=m[1], M=int(m[2]), N=int(m[3]), K=int(m[4]), wgs=int(m[5]), nch=int(m[6]), us8=float(m[7]), us4=float(m[8]),
                             winner=int(m[9])))
    return rows


def test_rule_source_is_the_restated_one():
    """the C rule, as text: the bounds and the chunk count this file restates"""
    body = re.search(r"static bool bf3_ks_four_waves\(int64_t wgs, int nch, int nw_pin\) \{(.*?)\n\}", P._BF3, re.S).group(1)
    assert "if (nw_pin) return nw_pin == 4;" in body
    assert "return wgs > cus && wgs <= 2 * cus && nch >= 2 * 4;" in body
    # both launchers ask it with their eight-wave grid and their chunk count
    assert "bf3_ks_four_waves(wgs2, d.Cin / CB, nw_pin)" in P._BF3 and "bf3_ks_four_waves(wgs, d.Cin / CB, nw_pin)" in P._BF3
    assert "bf3_ks_four_waves(wgs, nch, nw_pin)" in P._BF3


def test_sweep_table_is_consistent():
    rows = sweep_rows()
    assert len(rows) >= 9
    for r in rows:
        assert grid(r["form"], r["M"], r["N"], r["K"]) == (r["wgs"], r["nch"]), r
        # a winner of the four-wave form was measured faster there
        assert (r["winner"] == 4) <= (r["us4"] < r["us8"]), r


def test_winners_of_the_sweep_and_only_those_take_four_waves():
    rows = sweep_rows()
    took = {(r["form"], r["M"], r["N"], r["K"]) for r in rows if four_waves(r["wgs"], r["nch"], CUS)}
    won = {(r["form"], r["M"], r["N"], r["K"]) for r in rows if r["winner"] == 4}
    assert took == won and won
    # the launches of one replayed step between one and two rounds (M x N x K) are among them
    for shape in (("3x3", 256, 4096, 2304), ("3x3", 128, 8192, 1152), ("2x2", 512, 2048, 1024), ("1x1", 512, 4096, 1024),
                  ("1x1", 2048, 1024, 1536), ("1x1", 2048, 1024, 512)):
        assert shape in won, shape


def test_one_round_shapes_stay_on_eight_waves():
    for form, M, N, K in (("1x1", 256, 4096, 1024), ("3x3", 512, 512, 4608), ("3x3", 256, 2048, 2304)):
        wgs, nch = grid(form, M, N, K)
        assert wgs <= CUS and not four_waves(wgs, nch, CUS), (form, M, N, K)
    # ... and so does a grid past two rounds, and one whose waves would get fewer than two chunks
    assert not four_waves(2 * CUS + 1, 64, CUS) and four_waves(2 * CUS, 64, CUS) and four_waves(CUS + 1, 8, CUS)
    assert not four_waves(2 * CUS, 7, CUS)
    # a pin overrides the grid
    assert four_waves(1, 5, CUS, nw_pin=4) and not four_waves(2 * CUS, 64, CUS, nw_pin=8)


def test_two_four_wave_workgroups_fit_a_cu():
    """LDS of every NW = 4 instantiation: launch_bf3_ks_tile's max(NW patch regions, NW partial tiles) for the tiles
    launch_bf3_ks_px64 instantiates with KS = 2 and 3, and the 1x1 launcher's four partial tiles"""
    m = re.search(r"constexpr int NPIX = \(PTH \+ KS - 1\) \* \(PTW \+ KS - 1\), WREG = \(NPIX \* PIXB \+ 15\) & ~15, "
                  r"RED = NW \* 32 \* \(32 \* TN \+ 4\) \* 4;\s*constexpr size_t lds = \(size_t\)\(NW \* WREG > RED \? NW \* WREG : RED\);", P._BF3)
    assert m, "launch_bf3_ks_tile's LDS formula"
    tiles = re.findall(r"launch_bf3_ks_tile<(\d+), (\d+), (\d+), KS, 4>", P._BF3)
    assert sorted((int(a), int(b), int(c)) for a, b, c in tiles) == [(2, 32, 2), (4, 16, 2), (8, 8, 2)]
    calls = sorted(int(k) for k in re.findall(r"launch_bf3_ks_px64<(\d)>\(d, s", P._BF3))
    assert calls == [2, 3]
    sizes = {}
    for pth, ptw, tn in ((int(a), int(b), int(c)) for a, b, c in tiles):
        for KS in calls:
            wreg = ((pth + KS - 1) * (ptw + KS - 1) * P.PIXB + 15) & ~15
            sizes[(KS, pth, ptw)] = max(4 * wreg, 4 * 32 * (32 * tn + 4) * 4)
    m1 = re.search(r"constexpr size_t lds = \(size_t\)4 \* 32 \* \((\d+) \+ (\d+)\) \* 4;\s*static_assert\(lds <= 80 \* 1024", P._BF3)
    assert m1, "the 1x1 launcher's four-wave LDS"
    sizes["1x1"] = 4 * 32 * (int(m1[1]) + int(m1[2])) * 4
    assert len(sizes) == 7
    for key, lds in sizes.items():
        assert 2 * lds <= LDS_CU, (key, lds)
    assert sizes[(3, 2, 32)] == 60928 and sizes["1x1"] == 67584   # the largest of each kernel
