"""CPU-only: the quasi-binomial F test of two groups of replicates per site (csrc/mdk_qdiff_core.h), driven through tools/qdiff_emu: its
results against the restatement in Python floats (tests/qdiff_rule.py) bit for bit, and against exact arithmetic -- the statistic in
rationals, the tail of F(1, nu) from mpmath at 70 digits --; and what the test is for, its calibration on over-dispersed replicates
without a difference."""
import struct
import subprocess
from fractions import Fraction

import pytest

from conftest import REPO
from diff_rule import bits
from diff_rule import pvalue as fisher
from qdiff_rule import (ACCEPTED, C_CONST, C_NU, C_STEPS, HAND, NAMES, REFUSED, exact_statistic, null_sites, refusal, score, seeded, site, tail)

EMU = REPO / "tools" / "_build" / "qdiff_emu"
U = Fraction(1, 2 ** 53)
GRID_NU = (1, 2, 3, 4, 5, 10, 31, 62, 63, 1021, 1022)


def pattern(x):
    return "%016x" % (bits(x) & (2 ** 64 - 1))


def number(digits):
    return struct.unpack("<d", struct.pack("<Q", int(digits, 16)))[0]


def run(text):
    r = subprocess.run([str(EMU)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return [l.split("\t") for l in r.stdout.splitlines()]


def emu(sites, min_dispersion=1.0):
    """the emulator's lines for sites (ma, ua, mb, ub)"""
    return run("".join("s %s %d %d %s\n" % (pattern(min_dispersion), len(s[0]), len(s[2]), " ".join("%d %d" % e for e in zip(s[0] + s[2], s[1] + s[3]))) for s in sites))


def emu_tail(points):
    """(p, steps) of every (F, nu) as the host build of the header gives them"""
    return [(number(g[0]), int(g[1])) for g in run("".join("t %s %d\n" % (pattern(F), nu) for F, nu in points))]


def rule(s, min_dispersion=1.0):
    """what the emulator prints for an accepted site"""
    row, steps = site(*s, min_dispersion)
    return ["0"] + [str(v) for v in row[:4]] + [pattern(row[4]), pattern(row[5]), str(row[6]), pattern(row[7]), pattern(row[8]), str(steps)]


def exact_tail(F, nu):
    """P(F(1, nu) > F) for an exact F (a Fraction), to 70 digits"""
    import mpmath as mp
    with mp.workdps(70):
        f = mp.mpf(F.numerator) / mp.mpf(F.denominator)
        return mp.betainc(mp.mpf(nu) / 2, mp.mpf(1) / 2, 0, mp.mpf(nu) / (mp.mpf(nu) + f), regularized=True)


def ratio(p, want, steps, nu):
    """the relative error of p against the exact p-value `want` (mpmath), over its bound"""
    import mpmath as mp
    with mp.workdps(70):
        return float(abs(mp.mpf(p) - want) / want * 2 ** 53) / (C_STEPS * steps + C_NU * nu + C_CONST)


def wide(S, count, seed):
    """sites of S samples, all covered, half of them a group"""
    import random
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        fa, fb = rng.uniform(0.3, 0.7), rng.uniform(0.3, 0.7)
        m, u = [], []
        for s in range(S):
            n = rng.randint(5, 40)
            k = sum(1 for _ in range(n) if rng.random() < (fa if s < S // 2 else fb))
            m.append(k); u.append(n - k)
        out.append((m[:S // 2], u[:S // 2], m[S // 2:], u[S // 2:]))
    return out


@pytest.fixture(scope="module")
def sites():
    return seeded() + wide(66, 12, 66) + wide(1024, 2, 1024) + [h[1] for h in HAND] + ACCEPTED


def test_emulator_equals_the_rule_bit_for_bit(sites):
    assert len(sites) > 2000
    for floor in (1.0, 0.25):
        got = emu(sites, floor)
        assert len(got) == len(sites)
        for s, g in zip(sites, got):
            assert g == rule(s, floor), (s, floor)
    shapes = {len(s[0]) + len(s[2]) for s in sites}
    assert {3, 4, 5, 7, 12} <= shapes
    assert any(0 < sum(1 for m, u in zip(s[0] + s[2], s[1] + s[3]) if m + u == 0) for s in sites)
    assert any(sum(s[1]) == 0 and sum(s[0]) > 0 for s in sites)                     # group A all methylated


def test_tail_grid_against_mpmath():
    """The tail alone, F a double handed to the header as it is: nu of GRID_NU, F = 10^(k / 4) from 1e-6 to 1e100 and 10^(k / 50) from
    0.5 to 10, where the two branches meet and the complement's cancellation is at its worst.  Wherever the exact p is at least
    1e-280 the header's is within (4 steps + 12 nu + 32) 2^-53 of it, relatively.  Measured over this grid (3,417 points at or above
    1e-280): the worst error is 0.3225 of its bound (nu = 63, F = 2.754, 25 terms); a finer scan by hand found 0.41 (nu = 1022, F =
    2.92, 23 terms: 5,115 units of 2^-53 -- the power's nu / 2 multiplications carried into 1 - q where q is 10.5 times p); for nu <=
    4 the worst is 0.06 of the bound.  The longest series has 12,582 terms (nu = 1022)."""
    points = [(10.0 ** (k / 4.0), nu) for nu in GRID_NU for k in range(-24, 401)] + [(10.0 ** (k / 50.0), nu) for nu in GRID_NU for k in range(-15, 51)]
    got = emu_tail(points)
    worst, at, checked, longest = 0.0, None, 0, 0
    for (F, nu), (p, steps) in zip(points, got):
        assert 0.0 <= p <= 1.0
        if nu <= 62 or 0.3 < F < 30.0:
            assert (p, steps) == tail(F, nu), (F, nu)                                # (the restatement is slow where nu is large)
        want = exact_tail(Fraction(F), nu)
        longest = max(longest, steps)
        if want >= 1e-280:
            r = ratio(p, want, steps, nu)
            if r > worst:
                worst, at = r, (nu, F, steps)
            assert r <= 1.0, (nu, F, p, r)
            checked += 1
        else:
            assert p < 1e-279, (nu, F, p)
        if p == 0.0:
            assert want < 1e-280, (nu, F)
    print(f"worst error / bound {worst:.4f} at (nu, F, steps) {at}; {checked} points checked; the longest series {longest} terms")
    assert worst <= 0.5                                                              # the constants: no less than twice the measured worst
    assert checked > 3000


def test_header_against_exact_arithmetic(sites):
    """Whole sites: X, phi and F in rationals, the tail of the exact F from mpmath; the header's p, from tools/qdiff_emu, within
    (4 steps + 12 nu + 32) 2^-53 of it wherever the exact p is at least 1e-280.  F itself is some nu / 2 + 6 roundings from exact and p
    moves by at most nu / 2 times that, relatively: for the sites here but the two of 1,024 samples it is a small part of the bound,
    and those two are held to the bound as well.  Measured over 1,854 sites: the worst error is 0.145 of its bound."""
    worst, at, checked = 0.0, None, 0
    for s, g in zip(sites, emu(sites)):
        assert g[0] == "0"
        df, p, steps = int(g[7]), number(g[6]), int(g[10])
        if number(g[9]) == 0.0 and number(g[8]) == 1.0 and p == 1.0 and steps == 0:
            continue                                                                 # degenerate, or no difference at all
        X, phi, F, nu = exact_statistic(*s)
        assert nu == df and phi >= 1
        assert abs(Fraction(number(g[8])) - phi) <= phi * (nu + 8) * U
        assert abs(Fraction(number(g[9])) - F) <= F * (nu + 16) * U
        want = exact_tail(F, nu)
        if want >= 1e-280:
            r = ratio(p, want, steps, nu)
            if r > worst:
                worst, at = r, (s, steps)
            assert r <= 1.0, (s, p, r)
            checked += 1
        else:
            assert p < 1e-279
    print(f"worst error / bound {worst:.4f} at {at}; {checked} sites checked")
    assert checked > 1500 and worst <= 0.5


@pytest.mark.parametrize("name,s,known", HAND, ids=[h[0] for h in HAND])
def test_by_hand(name, s, known):
    (got,) = emu([s])
    assert got == rule(s)
    row, steps = site(*s)
    for column, value in known.items():
        assert row[NAMES.index(column)] == value, column
    if name == "identical replicates":
        # no residual at all: phi is at its floor, and p is the plain F(1, 4) tail of the pooled chi-square
        X = score(*row[:4])
        assert row[8] == X and row[5] == tail(X, 4)[0]
        assert exact_statistic(*s)[:2] == (Fraction(60 * 270 ** 2, 30 * 30 * 27 * 33), 1)
        want = exact_tail(exact_statistic(*s)[0], 4)
        assert ratio(row[5], want, steps, 4) <= 1.0 and 0.07 < row[5] < 0.09
        assert site(*s, 0.25)[0][8] == X / 0.25 and site(*s, 0.25)[0][7] == 0.25
    if name.startswith("parity"):
        # the same counts but for one sample: nu = 4 starts the constant at 2.0, nu = 3 at pi
        X, phi, F, nu = exact_statistic(*s)
        assert nu == known["df"] and ratio(row[5], exact_tail(F, nu), steps, nu) <= 1.0 and 0.0 < row[5] < 1.0
    if name == "huge F":
        assert exact_tail(exact_statistic(*s)[2], 118) < 1e-280 and steps == 0


def test_refused_and_accepted_at_the_limits():
    for (name, s, bit), g in zip(REFUSED, emu([r[1] for r in REFUSED])):
        assert refusal(*s) == bit and g[0] == str(bit) and set(g[1:5] + [g[7], g[10]]) == {"0"}, name
    for s, g in zip(ACCEPTED, emu(ACCEPTED)):
        assert refusal(*s) == 0 and g == rule(s)


def test_calibration_on_overdispersed_replicates():
    """The reason for the test: 4,000 sites without a difference, three replicates against three, depth 20 to 40, every replicate's
    fraction a beta draw around 0.6 with intra-class correlation 0.2.  The header rejects between 2 % and 8 % of them at 0.05 -- the
    band is a condition around the nominal 5 % --; Fisher's exact test of the pooled tables rejects several times as many.  Measured:
    4.50 % against 43.2 %."""
    null = null_sites()
    assert len(null) == 4000
    p = [number(g[6]) for g in emu(null)]
    rate = sum(1 for x in p if x < 0.05) / len(p)
    pooled = sum(1 for s in null[:1000] if fisher(sum(s[0]), sum(s[1]), sum(s[2]), sum(s[3]))[0] < 0.05) / 1000.0
    print(f"rejected at 0.05: {100 * rate:.2f} % (the quasi-binomial F test), {100 * pooled:.2f} % (Fisher's test of the pooled table, the first 1,000 sites)")
    assert 0.02 <= rate <= 0.08
    assert pooled > 0.25
