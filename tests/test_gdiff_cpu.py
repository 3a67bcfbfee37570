"""CPU-only: the quasi-binomial F test of three or more groups of replicates per site (csrc/mdk_gdiff_core.h), driven through
tools/gdiff_emu: its results against the restatement in Python floats (tests/gdiff_rule.py) bit for bit, against the two-group rule
(tests/qdiff_rule.py) bit for bit where two groups are covered, and against exact arithmetic -- the statistic in rationals, the tail of
F(q, nu) from mpmath's betainc at 70 digits --; and what the test is for, its calibration on over-dispersed replicates without a
difference."""
import struct
import subprocess
from fractions import Fraction

import pytest

from conftest import REPO
from diff_rule import bits
import gdiff_rule
import qdiff_rule
from gdiff_rule import ACCEPTED, C_CONST, C_NU, C_STEPS, HAND, NAMES, REFUSED, exact_statistic, null_sites, refusal, seeded, site, tail, two

EMU = REPO / "tools" / "_build" / "gdiff_emu"
U = Fraction(1, 2 ** 53)
GRID_NU = (1, 2, 3, 4, 5, 10, 31, 62, 63, 500, 1021)
GRID_Q = (1, 2, 3, 4, 5, 8, 15, 64, 255)


def pattern(x):
    return "%016x" % (bits(x) & (2 ** 64 - 1))


def number(digits):
    return struct.unpack("<d", struct.pack("<Q", int(digits, 16)))[0]


def run(text):
    r = subprocess.run([str(EMU)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return [l.split("\t") for l in r.stdout.splitlines()]


def emu(sites, min_dispersion=1.0):
    """the emulator's lines for sites (lists of groups (ms, us))"""
    return run("".join("s %s %d %s %s\n" % (pattern(min_dispersion), len(s), " ".join(str(len(ms)) for ms, _ in s),
                                           " ".join("%d %d" % e for ms, us in s for e in zip(ms, us))) for s in sites))


def emu_tail(points):
    """(p, steps) of every (W, nu, q) as the host build of the header gives them"""
    return [(number(g[0]), int(g[1])) for g in run("".join("t %s %d %d\n" % (pattern(W), nu, q) for W, nu, q in points))]


def rule(s, min_dispersion=1.0):
    """what the emulator prints for an accepted site"""
    gm, gu, row, steps = site(s, min_dispersion)
    return ["0", pattern(row[0]), str(row[1]), str(row[2]), pattern(row[3]), str(row[4]), str(row[5]), pattern(row[6]), pattern(row[7]), str(steps)] + \
        [str(v) for pair in zip(gm, gu) for v in pair]


def exact_tail(W, nu, q):
    """P(F(q, nu) > W / q) for an exact W (a Fraction), to 70 digits"""
    import mpmath as mp
    with mp.workdps(70):
        w = mp.mpf(W.numerator) / mp.mpf(W.denominator)
        return mp.betainc(mp.mpf(nu) / 2, mp.mpf(q) / 2, 0, mp.mpf(nu) / (mp.mpf(nu) + w), regularized=True)


def ratio(p, want, steps, nu, q):
    """the relative error of p against the exact p-value `want` (mpmath), over its bound"""
    import mpmath as mp
    with mp.workdps(70):
        return float(abs(mp.mpf(p) - want) / want * 2 ** 53) / (C_STEPS * steps + C_NU * (nu + q) + C_CONST)


def wide(G, size, count, seed):
    """sites of G groups of `size` samples each, all covered"""
    import random
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        groups = []
        for _ in range(G):
            f = rng.uniform(0.3, 0.7)
            ms, us = [], []
            for _ in range(size):
                n = rng.randint(5, 40)
                k = sum(1 for _ in range(n) if rng.random() < f)
                ms.append(k); us.append(n - k)
            groups.append((ms, us))
        out.append(groups)
    return out


@pytest.fixture(scope="module")
def sites():
    return seeded() + wide(3, 22, 8, 66) + wide(256, 4, 2, 1024) + wide(512, 2, 1, 512) + [h[1] for h in HAND] + ACCEPTED


def test_the_constants_are_the_headers():
    import re
    header = (REPO / "methyldackel_amd" / "csrc" / "mdk_gdiff_core.h").read_text()
    got = re.search(r"enum \{ GDIFF_C_STEPS = (\d+), GDIFF_C_NU = (\d+), GDIFF_C_CONST = (\d+) \};", header)
    assert got and tuple(map(int, got.groups())) == (C_STEPS, C_NU, C_CONST)
    assert (gdiff_rule.TINY, gdiff_rule.HUGE, gdiff_rule.NEGLIGIBLE) == (qdiff_rule.TINY, qdiff_rule.HUGE, qdiff_rule.NEGLIGIBLE)


def test_emulator_equals_the_rule_bit_for_bit(sites):
    assert len(sites) > 900
    for floor in (1.0, 0.25):
        got = emu(sites, floor)
        assert len(got) == len(sites)
        for s, g in zip(sites, got):
            assert g == rule(s, floor), (s, floor)
    assert {2, 3, 4, 5, 8, 17, 256, 512} <= {len(s) for s in sites}
    assert {1, 2, 3, 4, 5, 6} <= {len(ms) for s in sites for ms, _ in s}
    entries = [m + u for s in seeded() for ms, us in s for m, u in zip(ms, us)]
    assert 0.08 < sum(1 for e in entries if e == 0) / len(entries) < 0.25                        # a tenth uncovered, and the groups that are gone
    assert any(sum(us) == 0 and sum(ms) > 0 for s in sites for ms, us in s)                      # a group all methylated
    assert any(sum(us) + sum(ms) == 0 for s in sites for ms, us in s)                            # a whole group uncovered
    dfg = {site(s)[2][5] for s in sites}
    assert {0, 1, 2, 3, 4, 7, 16, 255, 511} <= dfg


def test_two_groups_are_the_two_group_rule_bit_for_bit():
    """every site of qdiff_rule run as two groups: pvalue, df, dispersion, statistic and steps are qdiff_rule.site's, the pooled counts
    too, and meth_diff is the absolute value of its meth_diff"""
    theirs = qdiff_rule.seeded() + [h[1] for h in qdiff_rule.HAND] + qdiff_rule.ACCEPTED
    assert len(theirs) > 2000
    for floor in (1.0, 0.25):
        for s, g in zip(theirs, emu([two(s) for s in theirs], floor)):
            row, steps = qdiff_rule.site(*s, floor)
            assert g[0] == "0"
            assert [g[4], g[5], g[7], g[8], g[9]] == [pattern(row[5]), str(row[6]), pattern(row[7]), pattern(row[8]), str(steps)], s
            assert g[1] == pattern(abs(row[4])) and g[10:] == [str(v) for v in row[:4]], s
            both = row[0] + row[1] > 0 and row[2] + row[3] > 0
            assert g[6] == ("1" if both else "0")
            if both:
                assert (g[2], g[3]) == (("0", "1") if row[4] > 0 else ("1", "0") if row[4] < 0 else ("0", "0")), s


def test_tail_with_one_numerator_degree_is_qdiff_tail():
    points = [(10.0 ** (k / 4.0), nu) for nu in (1, 2, 3, 4, 5, 10, 31, 62, 63, 1021, 1022) for k in range(-24, 401)] + \
             [(10.0 ** (k / 50.0), nu) for nu in (1, 2, 3, 4, 5, 10, 31, 62, 63) for k in range(-15, 51)] + [(0.0, 3), (2.0 ** -941, 3), (2.0 ** 1000, 3), (float("inf"), 2)]
    got = emu_tail([(W, nu, 1) for W, nu in points])
    theirs = subprocess.run([str(REPO / "tools" / "_build" / "qdiff_emu")], input="".join("t %s %d\n" % (pattern(W), nu) for W, nu in points), capture_output=True, text=True)
    assert theirs.returncode == 0
    assert [(number(l.split("\t")[0]), int(l.split("\t")[1])) for l in theirs.stdout.splitlines()] == got
    assert len(got) > 4664


def test_an_uncovered_middle_group_leaves_the_two_group_site():
    pairs = [two(s) for s in qdiff_rule.seeded(per_shape=60)]
    threes = [[a, ([0] * gone, [0] * gone), b] for a, b in pairs for gone in (1, 2, 3)]
    alone = [h for h in emu(pairs) for _ in range(3)]
    got = emu(threes)
    assert len(got) == len(alone) == 900
    for g, h in zip(got, alone):
        assert g[:2] == h[:2] and g[4:10] == h[4:10]
        assert g[10:] == h[10:12] + ["0", "0"] + h[12:]
        assert (g[2], g[3]) == tuple({"0": "0", "1": "2", "-1": "-1"}[v] for v in (h[2], h[3]))
    assert any(r[6] == "1" and number(r[4]) < 1.0 for r in got)


def test_tail_grid_against_mpmath():
    """The tail alone, W a double handed to the header as it is: nu of GRID_NU, q of GRID_Q, W = 10^(k / 4) from 1e-6 to 1e100, and W =
    10^(k / 50) from 0.1 to 1000 times q where the two branches meet.  Wherever the exact p is at least 1e-280 the header's is not 0.0
    and within (4 steps + 12 (nu + q) + 32) 2^-53 of it, relatively; at every point the host build gives the bits of the restatement in
    Python floats.  Measured over this grid (28,270 points at or above 1e-280): the worst error is 0.3070 of its bound (nu = 1021, q = 2, W =
    3.9905, 25 terms; 0.1618 on the coarse grid alone, at nu = 63, q = 4, W = 5.623); the longest series has 12,025 terms; the trap of cutting on x^(nu / 2) alone, nu = 62, q = 15, W = 1e11, has p = 2.0146e-279."""
    points = [(10.0 ** (k / 4.0), nu, q) for nu in GRID_NU for q in GRID_Q for k in range(-24, 401)]
    fine = [(q * 10.0 ** (k / 50.0), nu, q) for nu in GRID_NU for q in GRID_Q for k in range(-50, 151, 5)]
    got = emu_tail(points + fine)
    worst, at, checked, longest = 0.0, None, 0, 0
    for (W, nu, q), (p, steps) in zip(points + fine, got):
        assert 0.0 <= p <= 1.0
        assert (p, steps) == tail(W, nu, q), (W, nu, q)
        want = exact_tail(Fraction(W), nu, q)
        longest = max(longest, steps)
        if want >= 1e-280:
            assert p != 0.0, (nu, q, W)
            r = ratio(p, want, steps, nu, q)
            if r > worst:
                worst, at = r, (nu, q, W, steps)
            assert r <= 1.0, (nu, q, W, p, r)
            checked += 1
        else:
            assert p < 1e-279, (nu, q, W, p)
    (trap,) = emu_tail([(1e11, 62, 15)])
    assert 1.9e-279 < trap[0] < 2.1e-279
    print(f"worst error / bound {worst:.4f} at (nu, q, W, steps) {at}; {checked} points checked; the longest series {longest} terms")
    assert worst <= 0.5                                                              # the constants: no less than twice the measured worst
    assert checked > 20000


def test_a_larger_statistic_never_has_a_larger_pvalue():
    for nu in GRID_NU:
        for q in GRID_Q:
            ws = sorted({10.0 ** (k / 4.0) for k in range(-24, 401)} | {q * 10.0 ** (k / 50.0) for k in range(-50, 151)})
            ps = [p for p, _ in emu_tail([(W, nu, q) for W in ws])]
            assert ps[0] <= 1.0 and all(b <= a for a, b in zip(ps, ps[1:])), (nu, q)
            assert ps[0] > 0.99 and ps[-1] < 1e-40


def test_header_against_exact_arithmetic(sites):
    """Whole sites: X, phi and W in rationals, the tail of the exact W from mpmath; the header's p, from tools/gdiff_emu, within
    (4 steps + 12 (nu + q) + 32) 2^-53 of it wherever the exact p is at least 1e-280.  W is some g + nu / 2 + 8 roundings from exact
    and p moves by at most (nu + q) / 2 times that, relatively, which the bound's 12 (nu + q) holds.  Measured over 935 sites: the
    worst error is 0.1202 of its bound."""
    worst, at, checked = 0.0, None, 0
    for s, g in zip(sites, emu(sites)):
        assert g[0] == "0"
        p, df, dfg, steps = number(g[4]), int(g[5]), int(g[6]), int(g[9])
        if number(g[8]) == 0.0 and number(g[7]) == 1.0 and p == 1.0 and steps == 0:
            continue                                                                 # degenerate, or no difference at all
        X, phi, W, nu, q = exact_statistic(s)
        assert (nu, q) == (df, dfg) and phi >= 1
        assert abs(Fraction(number(g[7])) - phi) <= phi * (nu + len(s) + 8) * U
        assert abs(Fraction(number(g[8])) - W / q) <= W / q * (nu + 2 * len(s) + 16) * U
        want = exact_tail(W, nu, q)
        if want >= 1e-280:
            r = ratio(p, want, steps, nu, q)
            if r > worst:
                worst, at = r, (s, steps)
            assert p != 0.0 and r <= 1.0, (s, p, r)
            checked += 1
        else:
            assert p < 1e-279
    print(f"worst error / bound {worst:.4f} at {at}; {checked} sites checked")
    assert checked > 800 and worst <= 0.5


@pytest.mark.parametrize("name,s,known", HAND, ids=[h[0] for h in HAND])
def test_by_hand(name, s, known):
    (got,) = emu([s])
    assert got == rule(s)
    gm, gu, row, steps = site(s)
    for column, value in known.items():
        assert row[NAMES.index(column)] == value, column
    assert row[0] >= 0.0
    if name == "identical replicates":
        # no residual at all: phi is at its floor, and p is the plain F(2, 3) tail of the pooled table's chi-square, (160^2 + 200^2 + 40^2) / (20 x 28 x 32)
        X, phi, W, nu, q = exact_statistic(s)
        assert (X, phi, nu, q) == (Fraction(15, 4), 1, 3, 2)
        assert ratio(row[3], exact_tail(W, nu, q), steps, nu, q) <= 1.0 and row[7] == 1.875
        assert site(s, 0.25)[2][6] == 0.25
    if name.startswith("parity"):
        X, phi, W, nu, q = exact_statistic(s)
        assert (nu, q) == (known["df"], known["df_groups"]) and ratio(row[3], exact_tail(W, nu, q), steps, nu, q) <= 1.0 and 0.0 < row[3] < 1.0
    if name == "the middle group uncovered":
        theirs, their_steps = qdiff_rule.site(s[0][0], s[0][1], s[2][0], s[2][1])
        assert (row[3], row[4], row[6], row[7], steps) == (theirs[5], theirs[6], theirs[7], theirs[8], their_steps) and row[0] == -theirs[4]
    if name == "huge W":
        X, phi, W, nu, q = exact_statistic(s)
        assert exact_tail(W, nu, q) < 1e-280 and steps == 0


def test_refused_and_accepted_at_the_limits():
    for (name, s, bit), g in zip(REFUSED, emu([r[1] for r in REFUSED])):
        assert refusal(s) == bit and g[0] == str(bit), name
        assert g[1:10] == [pattern(0.0), "-1", "-1", pattern(1.0), "0", "0", pattern(1.0), pattern(0.0), "0"] and set(g[10:]) == {"0"} and len(g) == 10 + 2 * len(s), name
    for s, g in zip(ACCEPTED, emu(ACCEPTED)):
        assert refusal(s) == 0 and g == rule(s)
    # with two groups the margins are diff_rule's
    for name, s, bit in qdiff_rule.REFUSED:
        assert refusal(two(s)) == bit == qdiff_rule.refusal(*s), name
        (g,) = emu([two(s)])
        assert g[0] == str(bit)


def test_calibration_on_overdispersed_replicates():
    """The reason for the test: 4,000 sites without a difference, three groups of three replicates, depth 20 to 40, every replicate's
    fraction a beta draw around 0.6 with intra-class correlation 0.2.  The header rejects between 2 % and 8 % of them at 0.05 -- the
    band is a condition around the nominal 5 % --; the chi-square test of the pooled 3 x 2 tables, which takes every read for an
    independent draw, rejects many times as many.  Measured: 4.725 % against 65.5 %."""
    import mpmath as mp
    null = null_sites()
    assert len(null) == 4000 and all(len(s) == 3 and all(len(ms) == 3 for ms, _ in s) for s in null)
    got = emu(null)
    p = [number(g[4]) for g in got]
    assert all(g[5] == "6" and g[6] == "2" for g in got)
    rate = sum(1 for x in p if x < 0.05) / len(p)
    pooled = sum(1 for s in null[:1000] if mp.exp(-mp.mpf(float(exact_statistic(s)[0])) / 2) < 0.05) / 1000.0           # chi-square, 2 df: exp(-X / 2)
    print(f"rejected at 0.05: {100 * rate:.3f} % (the quasi-binomial F test), {100 * pooled:.2f} % (the chi-square test of the pooled table, the first 1,000 sites)")
    assert 0.02 <= rate <= 0.08
    assert pooled > 0.25
