"""CPU-only: the pairwise sample moments (csrc/mdk_moments_core.h), driven through tools/moments_emu -- the host build of the header: its
matrices against the restatement in Python ints (tests/moments_rule.py), the level formula exhaustively, the centring at the limits of
what it accepts, the refusals, and the additivity of the sums."""
import random
import subprocess

import numpy as np
import pytest

import moments_rule as rule
from conftest import REPO
from moments_tables import check_mix, expected, limit_matrices, table

EMU = REPO / "tools" / "_build" / "moments_emu"


def table_text(m, u, min_depth):
    S, n = len(m), len(m[0]) if len(m) else 0
    lines = ["T %d %d %d" % (S, n, min_depth)]
    for s in range(S):
        lines += ["%d %d" % e for e in zip(m[s], u[s])]
    return "\n".join(lines) + "\n"


def sums_text(n, sx, sxx, sxy):
    S = len(n)
    return "\n".join(["C %d" % S] + [" ".join(str(v) for v in row) for mat in (n, sx, sxx, sxy) for row in mat]) + "\n"


def run(text, jobs):
    """the emulator's results for the jobs of `text`, `jobs` their (kind, S): (err, at) for a refused one, otherwise for a table (n, sx,
    sxx, sxy, cxy, vxx) and for sums (cxy, vxx) -- integers as lists of lists, doubles as lists of lists of 64-bit patterns"""
    r = subprocess.run([str(EMU)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = iter(r.stdout.splitlines())
    out = []
    for kind, S in jobs:
        err, at = (int(v) for v in next(lines).split("\t"))
        if err:
            out.append((err, at))
            continue
        mats = []
        for q in range(6 if kind == "T" else 2):
            base = 10 if kind == "T" and q < 4 else 16
            mats.append([[int(v, base) for v in next(lines).split("\t")] for _ in range(S)])
        out.append(tuple(mats))
    assert next(lines, None) is None
    return out


def emu_table(m, u, min_depth):
    return run(table_text(m, u, min_depth), [("T", len(m))])[0]


def emu_center(n, sx, sxx, sxy):
    return run(sums_text(n, sx, sxx, sxy), [("C", len(n))])[0]


def rule_table(m, u, min_depth):
    sums = rule.moments(m, u, min_depth)
    cxy, vxx = rule.center(*sums)
    return tuple(sums) + (rule.pattern(cxy), rule.pattern(vxx))


@pytest.mark.parametrize("S,n", [(1, 1), (2, 65), (3, 257), (12, 65), (12, 300), (17, 63)])
def test_emulator_is_the_rule(S, n):
    """seeded tables at both depths: the four sums exactly, the centred ones bit for bit -- and the int64 matrix products the larger
    tests use are the loop over pairs and sites"""
    m, u = table(S, n)
    for min_depth in (1, 5):
        check_mix(m, u, min_depth)
        want = rule_table(m.tolist(), u.tolist(), min_depth)
        assert emu_table(m.tolist(), u.tolist(), min_depth) == want
        assert expected(S, n, min_depth) == want


def test_no_sites_and_no_cover():
    assert emu_table([[], []], [[], []], 1) == rule_table([[], []], [[], []], 1)
    got = emu_table([[0, 1, 2], [3, 0, 0]], [[0, 2, 1], [0, 0, 0]], 4)
    assert got == rule_table([[0, 1, 2], [3, 0, 0]], [[0, 2, 1], [0, 0, 0]], 4)
    assert got[0] == [[0, 0], [0, 0]] and got[4] == [[0, 0], [0, 0]]


def test_level_formula_exhaustively():
    """every m + u <= 64 and the largest depths: the level is round-half-up of m / d * 65536, and the emulator's diagonal holds it"""
    cells = [(a, d - a) for d in range(1, 65) for a in range(d + 1)]
    top = rule.LIMIT - 1
    cells += [(top, 0), (0, top), (top, top), (top, 1), (1, top), (top - 1, top), (top // 2, top // 2 + 1), (1, 2), (12345678, 54321)]
    # ... and seeded cells of every magnitude, among them quotients next to an integer and next to a half: d = 2^k +- 1, m = d / 2 +- 1
    rnd = random.Random(20240613)
    for _ in range(1500):
        a, b = rnd.randrange(1 << rnd.randrange(1, 27)), rnd.randrange(1 << rnd.randrange(1, 27))
        cells.append((a, b) if a + b else (1, 0))
    for k in range(2, 27):
        for d in ((1 << k) - 1, (1 << k) + 1, (1 << k) + 3):
            for a in (d // 2 - 1, d // 2, d // 2 + 1, d // 3, d - 1, 1):
                if 0 <= a <= min(d, top) and d - a <= top:
                    cells.append((a, d - a))
    for a, b in cells:
        x = rule.level(a, b)
        d = a + b
        assert 0 <= x <= rule.ONE and 2 * d * x <= 2 * a * rule.ONE + d < 2 * d * (x + 1)
        assert abs(x * d - a * rule.ONE) * 2 <= d                   # within half a unit of the exact level
    assert rule.level(top, 0) == rule.ONE and rule.level(0, top) == 0 and rule.level(1, 1) == 32768 and rule.level(1, 2) == 21845
    # a sample per cell, one site: the diagonal of sx is the cell's level
    for at in range(0, len(cells), 128):
        some = cells[at:at + 128]
        got = emu_table([[a] for a, _ in some], [[b] for _, b in some], 1)
        assert [got[1][i][i] for i in range(len(some))] == [rule.level(a, b) for a, b in some]
        assert [got[2][i][i] for i in range(len(some))] == [rule.level(a, b) ** 2 for a, b in some]


def test_all_methylated_at_the_largest_count():
    """every x^2 is 2^32: the sums carry past 32 bits at the second site"""
    top = rule.LIMIT - 1
    m, u = [[top] * 4100] * 2, [[0] * 4100] * 2
    got = emu_table(m, u, 5)
    assert got == rule_table(m, u, 5)
    assert got[2] == [[4100 << 32] * 2] * 2 and got[3] == [[4100 << 32] * 2] * 2 and got[4] == [[0, 0], [0, 0]]


def test_centring_at_the_limits():
    for sums in limit_matrices():
        assert rule.sums_refusal(*sums) is None, sums
        cxy, vxx = rule.center(*sums)
        assert emu_center(*sums) == (rule.pattern(cxy), rule.pattern(vxx)), sums
    # the cancellations, as numbers
    cxy, vxx = rule.center(*limit_matrices()[0])
    assert cxy == [[0.0, 0.0], [0.0, 0.0]] and vxx == [[0.0, 0.0], [0.0, 0.0]]
    assert rule.center(*limit_matrices()[4])[0][0][1] == -1.0 and rule.center(*limit_matrices()[6])[0][0][1] == 1.0
    assert rule.center(*limit_matrices()[2])[0][0][1] == 2.0 ** 92


def test_rounding_of_the_conversion():
    """mom_to_double against float(int) where the conversion rounds.  cxy = 2^92 - 2^38 c: 39 bits go, and for an odd c what goes is
    exactly a half -- a tie, to the even neighbour: upward at c = 1 (into the exponent: 2^92) and 5, downward at 3 and 7.  Then a
    seeded sweep of 32 x 32 cells within the bounds, of both signs"""
    import random
    for c in range(1, 9):
        sums = ([[1 << 30] * 2] * 2, [[1 << 38, 1 << 38], [c, c]], [[1 << 62] * 2] * 2, [[1 << 62] * 2] * 2)
        exact = (1 << 92) - (c << 38)
        kept, rest = exact >> 39, exact & ((1 << 39) - 1)
        assert (rest == 1 << 38) == (c % 2 == 1)                    # a tie
        want = float(exact)
        assert want == float((kept + (1 if c % 2 and kept % 2 else 0)) << 39)
        assert rule.sums_refusal(*sums) is None
        got = emu_center(*sums)
        assert got[0][0][1] == rule.bits(want) == got[0][1][0]
    assert float((1 << 92) - (1 << 38)) == 2.0 ** 92
    rnd = random.Random(20240611)
    S = 32
    n = [[rnd.randrange(0, (1 << 30) + 1) if rnd.random() < 0.7 else rnd.randrange(0, 40) for _ in range(S)] for _ in range(S)]
    sx = [[rnd.randrange(0, v * 65536 + 1) for v in row] for row in n]
    sxx = [[rnd.randrange(0, (v << 32) + 1) >> rnd.choice((0, 0, 20, 40)) for v in row] for row in n]
    sxy = [[rnd.randrange(0, (v << 32) + 1) >> rnd.choice((0, 0, 20, 40)) for v in row] for row in n]
    assert rule.sums_refusal(n, sx, sxx, sxy) is None
    cxy, vxx = rule.center(n, sx, sxx, sxy)
    assert any(v < 0 for row in cxy for v in row) and any(v > 2.0 ** 80 for row in cxy for v in row) and any(v < 0 for row in vxx for v in row)
    assert emu_center(n, sx, sxx, sxy) == (rule.pattern(cxy), rule.pattern(vxx))


def test_sums_refusals():
    ok = ([[4, 4], [4, 4]], [[9, 9], [9, 9]], [[30, 30], [30, 30]], [[30, 20], [20, 30]])
    assert rule.sums_refusal(*ok) is None and len(emu_center(*ok)) == 2
    cases = []
    for q, (i, j, value) in enumerate(((0, 1, -1), (1, 0, -5), (1, 1, -1), (0, 1, -2))):          # a negative sum in each matrix
        sums = [[list(r) for r in mat] for mat in ok]
        sums[q][i][j] = value
        cases.append((sums, (rule.E_SUM_NEGATIVE, 2 * i + j)))
    big = [[list(r) for r in mat] for mat in ok]
    big[0][1][1] = (1 << 30) + 1
    cases.append((big, (rule.E_SUM_N, 3)))
    sx = [[list(r) for r in mat] for mat in ok]
    sx[1][0][1] = 4 * 65536 + 1
    cases.append((sx, (rule.E_SUM_SX, 1)))
    for q in (2, 3):
        sq = [[list(r) for r in mat] for mat in ok]
        sq[q][1][0] = (4 << 32) + 1
        cases.append((sq, (rule.E_SUM_SQ, 2)))
    two = [[list(r) for r in mat] for mat in ok]                    # two refused cells: the first is reported
    two[1][1][1] = -1
    two[0][0][1] = (1 << 30) + 1
    cases.append((two, (rule.E_SUM_N, 1)))
    for sums, want in cases:
        assert rule.sums_refusal(*sums) == want
        assert emu_center(*sums) == want


def test_entry_refusals():
    m, u = table(3, 65)
    m, u = m.tolist(), u.tolist()
    for (s, k, which, value), want in (((1, 40, 0, -1), (rule.E_NEGATIVE, 40)), ((2, 7, 1, rule.LIMIT), (rule.E_ENTRY, 7)), ((0, 64, 1, -3), (rule.E_NEGATIVE, 64))):
        mm, uu = [list(r) for r in m], [list(r) for r in u]
        (mm, uu)[which][s][k] = value
        assert rule.refusal(mm, uu) == want and emu_table(mm, uu, 1) == want
    mm, uu = [list(r) for r in m], [list(r) for r in u]
    mm[2][9], uu[0][9], mm[1][30] = rule.LIMIT, -1, -1              # at one site the negative entry is named, and the smallest site
    assert rule.refusal(mm, uu) == (rule.E_NEGATIVE, 9) and emu_table(mm, uu, 1) == (rule.E_NEGATIVE, 9)
    mm, uu = [list(r) for r in m], [list(r) for r in u]
    mm[0][5] = rule.LIMIT - 1                                       # the largest entry is taken
    assert rule.refusal(mm, uu) is None and len(emu_table(mm, uu, 1)) == 6


def test_two_halves_add_to_the_whole():
    m, u = table(12, 300)
    for min_depth in (1, 5):
        whole = expected(12, 300, min_depth)
        for cut in (1, 150, 299):
            a = rule.moments_np(m[:, :cut], u[:, :cut], min_depth)
            b = rule.moments_np(m[:, cut:], u[:, cut:], min_depth)
            sums = [(x + y).tolist() for x, y in zip(a, b)]
            assert tuple(sums) == whole[:4]
            cxy, vxx = rule.center(*sums)
            assert (rule.pattern(cxy), rule.pattern(vxx)) == whole[4:]
            assert emu_center(*sums) == whole[4:]
    assert np.array_equal(np.array(whole[0]), np.array(whole[0]).T) and np.array_equal(np.array(whole[3]), np.array(whole[3]).T)


def test_the_header_declares_what_lib_moments_binds():
    import re
    import methyldackel_amd as mdk
    header = (REPO / "include" / "mdk_moments.h").read_text()
    assert '#include "mdk_moments.h"' in (REPO / "include" / "mdk_stats.h").read_text()
    declared = set(re.findall(r"\b(md_stats_\w+)\s*\(", header))
    assert declared == {"md_stats_moments", "md_stats_center", "md_stats_moments_limits"}
    L = mdk.lib_moments()                                           # (loading it needs no device)
    assert L is mdk.lib_stats()
    bound = {name for name in vars(L) if name.startswith("md_stats_")}
    assert declared <= bound
    for name, count in (("md_stats_moments", 11), ("md_stats_center", 8), ("md_stats_moments_limits", 5)):
        decl = re.search(r"int %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(decl.split(",")) == count == len(getattr(L, name).argtypes), name


def test_refused_without_a_device():
    import torch
    import methyldackel_amd as mdk
    m, u = torch.ones((3, 5), dtype=torch.int32), torch.ones((3, 5), dtype=torch.int32)
    with pytest.raises(mdk.MdkError, match="there is no CPU path"):
        mdk.sample_moments(m, u)
    with pytest.raises(mdk.MdkError, match="one dtype and one shape"):
        mdk.sample_moments(m, u.long())
    with pytest.raises(mdk.MdkError, match="min_depth"):
        mdk.sample_moments(m, u, 0)
    with pytest.raises(mdk.MdkError, match="1 to 1024 samples"):
        mdk.sample_moments(m[:0], u[:0])
    assert callable(mdk.Cohort.moments) and callable(mdk.CohortRegions.moments) and callable(mdk.moments_limits)
    assert mdk.MOMENTS_WHAT == ("correlation", "covariance", "n")
