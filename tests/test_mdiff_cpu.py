"""CPU-only: the quasi-binomial F test of a design's tested columns per site (csrc/mdk_mdiff_core.h), driven through tools/mdiff_emu:
its results against the restatement in Python floats (tests/mdiff_rule.py) bit for bit, against the same estimator at 50 digits in
mpmath, against the test of several groups (tests/gdiff_rule.py) where the design is an intercept and group dummies; and what the
test is for, its calibration on a paired design with a patient effect."""
import struct
import subprocess

import pytest

from conftest import REPO
from diff_rule import bits
import gdiff_rule
import mdiff_rule
from mdiff_rule import ACCEPTED, FULL, HAND, NAMES, NUMERIC, PLAIN, RANK, REDUCED, REFUSED, bound, dummies, exact, independent, paired_null_sites, refusal, seeded, site

EMU = REPO / "tools" / "_build" / "mdiff_emu"


def pattern(x):
    return "%016x" % (bits(x) & (2 ** 64 - 1))


def number(digits):
    return struct.unpack("<d", struct.pack("<Q", int(digits, 16)))[0]


def run(text):
    r = subprocess.run([str(EMU)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return [l.split("\t") for l in r.stdout.splitlines()]


def emu(sites, min_dispersion=1.0):
    """the emulator's lines for sites (ms, us, X, q)"""
    return run("".join("s %s %d %d %d %s %s\n" % (pattern(min_dispersion), len(ms), len(X[0]), q, " ".join("%d %d" % e for e in zip(ms, us)),
                                                " ".join(pattern(v) for x in X for v in x)) for ms, us, X, q in sites))


def rule(s, min_dispersion=1.0):
    """what the emulator prints for an accepted site"""
    K, M, coef, row, steps = site(*s, min_dispersion)
    return ["0", pattern(row[0]), str(row[1]), pattern(row[2]), pattern(row[3]), str(row[4]), str(row[5]), str(steps), str(K), str(M)] + [pattern(c) for c in coef]


@pytest.fixture(scope="module")
def sites():
    return seeded() + [h[1] for h in HAND] + ACCEPTED


def test_the_constants_are_the_headers():
    import re
    header = (REPO / "methyldackel_amd" / "csrc" / "mdk_mdiff_core.h").read_text()
    got = re.search(r"enum \{ MDIFF_C_STEPS = (\d+), MDIFF_C_NU = (\d+), MDIFF_C_FIT = (\d+), MDIFF_C_CONST = (\d+), MDIFF_C_TOL = (\d+) \};", header)
    assert got and tuple(map(int, got.groups())) == (mdiff_rule.C_STEPS, mdiff_rule.C_NU, mdiff_rule.C_FIT, mdiff_rule.C_CONST, mdiff_rule.C_TOL)
    assert re.search(r"enum \{ MDIFF_MAX_COLUMNS = 8, MDIFF_MAX_PASSES = 40 \};", header) and (mdiff_rule.MAX_COLUMNS, mdiff_rule.MAX_PASSES) == (8, 40)
    assert re.search(r"enum \{ MDIFF_RANK = 1, MDIFF_NUMERIC = 2, MDIFF_REDUCED = 4, MDIFF_FULL = 8 \};", header) and (RANK, NUMERIC, REDUCED, FULL) == (1, 2, 4, 8)
    for name, value in (("ETA_MAX", "40.0"), ("STEP_MAX", "4.0"), ("CONVERGED", "0x1p-40"), ("RANK_PIVOT", "0x1p-26"), ("INV_LN2", "0x1.71547652b82fep+0"),
                        ("LN2_HI", "0x1.62e42fee00000p-1"), ("LN2_LO", "0x1.a39ef35793c76p-33")):
        assert re.search(rf"#define MDIFF_{name} {re.escape(value)}\s", header), name
        assert getattr(mdiff_rule, name) == float.fromhex(value) if value.startswith("0x") else float(value)
    assert len(mdiff_rule.EXP_C) == 14 and all(c.hex() in header for c in mdiff_rule.EXP_C)


def test_the_exponential_against_mpmath():
    """mdiff_exp at 20,001 arguments over [-40, 0] and at the ends of its reduction's intervals: the host build gives the restatement's
    bits, and the worst error against mpmath is below two units of 2^-53 of the exact value: a correctly rounded one has up to one, and
    Horner's last steps and the reduced argument's rounding add less than another.  Measured: 1.5159 units, at t = -4.498."""
    import mpmath as mp
    ln2 = 0.6931471805599453
    ts = [-40.0 * k / 20000.0 for k in range(20001)] + [-(j + 0.5) * ln2 * (1.0 + d) for j in range(57) for d in (-1e-15, 0.0, 1e-15)] + [-0.0]
    got = run("".join("e %s\n" % pattern(t) for t in ts))
    worst, at = 0.0, None
    with mp.workdps(40):
        for t, g in zip(ts, got):
            v = number(g[0])
            assert v == mdiff_rule.exp(t), t
            want = mp.exp(mp.mpf(t))
            err = float(abs(mp.mpf(v) - want) / want * 2 ** 53)
            if err > worst:
                worst, at = err, t
    print(f"mdiff_exp: the worst error {worst:.4f} units of 2^-53 at t = {at!r}; {len(ts)} arguments")
    assert worst < 2.0 and number(got[0][0]) == 1.0 and number(got[-1][0]) == 1.0


def test_emulator_equals_the_rule_bit_for_bit(sites):
    assert len(sites) > 600
    for floor in (1.0, 0.25):
        got = emu(sites, floor)
        assert len(got) == len(sites)
        for s, g in zip(sites, got):
            assert g == rule(s, floor), (s, floor)
    own = seeded()
    assert {len(s[0]) for s in own} == set(range(5, 13)) and {len(s[2][0]) for s in own} == set(range(2, 9))
    assert {(len(s[2][0]), s[3]) for s in own} >= {(2, 1), (8, 1), (8, 7), (5, 3)}
    entries = [m + u for ms, us, _, _ in own for m, u in zip(ms, us)]
    assert 0.07 < sum(1 for e in entries if e == 0) / len(entries) < 0.13 and max(entries) == 40
    rows = [site(*s)[3] for s in sites]
    flags = {r[4] for r in rows}
    assert {0, RANK, NUMERIC, FULL, REDUCED | FULL} <= flags
    assert sum(1 for r in rows if r[4] == 0 and r[0] < 1.0) > 450 and max(r[5] for r in rows if r[4] == 0) > 30           # separated fits among them


@pytest.mark.parametrize("name,s,known", HAND, ids=[h[0] for h in HAND])
def test_by_hand(name, s, known):
    (got,) = emu([s])
    assert got == rule(s)
    K, M, coef, row, steps = site(*s)
    for column, value in known.items():
        assert row[NAMES.index(column)] == value, column
    assert (K, M) == (sum(s[0]), sum(s[1]))
    if row[4] & (RANK | NUMERIC) or row[2:4] == (1.0, 0.0) and row[5] == 0:
        assert coef == [0.0] * len(s[2][0]) and steps == 0
    if name == "two groups":
        # an intercept and one dummy: the two-group test of mdk_qdiff_core.h, and the coefficients are the logits of the pooled fractions
        import math
        import qdiff_rule
        theirs, _ = qdiff_rule.site(s[0][:3], s[1][:3], s[0][3:], s[1][3:])
        for ours, its in ((row[0], theirs[5]), (row[2], theirs[7]), (row[3], theirs[8])):
            assert abs(ours - its) <= 1e-12 * its
        assert row[1] == theirs[6]
        assert abs(coef[0] - math.log(18 / 14)) < 1e-12 and abs(coef[0] + coef[1] - math.log(9 / 21)) < 1e-12
    if name == "the reduced fit cannot converge":
        assert coef[1] < -75.0 and abs(coef[2] - site(*HAND[9][1])[2][2]) < 1e-9          # the group's coefficient is the covered batch site's all the same
    if name == "a batch whose only sample is uncovered":
        assert independent(s[2])                                                         # over all samples the design has its rank


def test_refused_and_accepted_at_the_limits():
    for (name, (ms, us), bit), g in zip(REFUSED, emu([(ms, us, PLAIN, 1) for _, (ms, us), _ in REFUSED])):
        assert refusal(ms, us) == bit and g[0] == str(bit), name
        assert g[1:] == [pattern(1.0), "0", pattern(1.0), pattern(0.0), "0", "0", "0", "0", "0", pattern(0.0), pattern(0.0)], name
    for s, g in zip(ACCEPTED, emu(ACCEPTED)):
        assert refusal(s[0], s[1]) == 0 and g == rule(s)


def test_the_design_s_rank_test():
    designs = [s[2] for s in seeded(per_shape=2)]
    dependent = [[[1.0, 0.0, 1.0], [1.0, 1.0, 0.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0]],           # the two dummies add up to the intercept
                 [[1.0, 0.0], [1.0, 0.0], [1.0, 0.0]],                                          # an empty column
                 [[1.0, a, b, 1.0 + 2.0 * a + b] for a, b in ((2.0, 3.0), (5.0, 1.0), (0.5, 0.5), (1.0, 1.0), (9.0, 2.0))],          # the last: the intercept, twice the second and the third
                 [[1.0, 1.0 + 2.0 ** -30], [1.0, 1.0], [1.0, 1.0 - 2.0 ** -30]],                # nearly the intercept: a pivot of 2^-60 of its diagonal
                 [[1e-170, 1.0], [1e-170, 2.0], [1e-170, 3.0]]]                                 # its square is no normal double
    near = [[[1.0, 1.0 + 2.0 ** -10], [1.0, 1.0], [1.0, 1.0 - 2.0 ** -10]]]                       # a pivot of 2^-20: independent
    every = designs + dependent + near
    got = run("".join("d %d %d %s\n" % (len(X), len(X[0]), " ".join(pattern(v) for x in X for v in x)) for X in every))
    assert [g[0] for g in got] == ["1" if independent(X) else "0" for X in every]
    assert all(independent(X) for X in designs + near) and not any(independent(X) for X in dependent)


def ratio(got, want, allowed):
    import mpmath as mp
    return float(abs(mp.mpf(got) - want) / want) / allowed


def test_header_against_the_same_estimator_in_mpmath():
    """Sites of designs with a continuous column, every fourth of mdiff_rule.seeded(): p, the dispersion and the statistic against a
    50-digit Newton fit of the same estimator with betainc for the tail.  Wherever the flags are 0 and the exact p is at least 1e-280
    each is within the header's bound of its exact value.  Measured over 130 such sites: the worst error is 0.1125 of the bound, 1,322
    units of 2^-53, at a site of nine covered samples and six columns whose fits took 8 passes."""
    own = [s for k, s in enumerate(seeded()) if k % 4 == 0]
    assert all(any(v not in (0.0, 1.0) for x in s[2] for v in x) for s in own)
    worst, at, checked, plain, units = 0.0, None, 0, 0.0, 0.0
    for s, g in zip(own, emu(own)):
        ms, us, X, q = s
        p, df, phi, stat, flags, its, steps = number(g[1]), int(g[2]), number(g[3]), number(g[4]), int(g[5]), int(g[6]), int(g[7])
        if flags or its == 0:
            continue
        k = sum(1 for m, u in zip(ms, us) if m + u > 0)
        allowed = bound(steps, df, q, k, len(X[0]))
        want_p, want_phi, want_stat = exact(ms, us, X, q)
        if want_p < 1e-280:
            continue
        pairs = [(phi, want_phi)] + ([(p, want_p), (stat, want_stat)] if want_stat > 1e-25 else [])           # (a statistic that is 0 exactly has no relative error)
        r = max(ratio(a, b, allowed) for a, b in pairs)
        if want_stat <= 1e-25:
            assert stat < 1e-20 and p > 1.0 - 1e-9
        if r > worst:
            worst, at = r, (s, its)
        if its < 20:
            plain = max(plain, r)
            units = max(units, r * allowed * 2 ** 53)
        assert r <= 1.0, (s, r)
        checked += 1
    print(f"worst error / bound {worst:.4f} at {at}; {checked} sites checked; among the fits of fewer than 20 passes {plain:.4f}, {units:.1f} units of 2^-53")
    assert checked > 120 and worst <= 0.5


def test_group_dummies_are_the_groups_test():
    """gdiff_rule's own sites of 2 to 8 groups with every group covered, as an intercept and a dummy for every group but the first, the
    dummies tested: df is gdiff_rule.site's, and p, the dispersion and the statistic are within the SUM of the two headers' bounds of
    it -- both are within their own bound of the same exact value.  Groups all methylated or all unmethylated are among them: their
    fits are separated and converge within the 40 passes.  Measured over 547 sites, 235 of them with a separated group: the worst
    difference is 0.3464 of the sum, the most passes of a site's two fits together 39."""
    theirs = [s for s in gdiff_rule.seeded() if len(s) <= 8 and all(any(m + u > 0 for m, u in zip(ms, us)) for ms, us in s)]
    theirs += [h[1] for h in gdiff_rule.HAND if len(h[1]) <= 8 and len(h[1][0][0]) < 10 and all(any(m + u > 0 for m, u in zip(ms, us)) for ms, us in h[1])]
    assert len(theirs) > 500 and {len(s) for s in theirs} >= {2, 3, 4, 5, 8}
    ours = [dummies(s) for s in theirs]
    worst, longest, separated, tested = 0.0, 0, 0, 0
    for s, d, g in zip(theirs, ours, emu(ours)):
        assert g == rule(d)
        p, df, phi, stat, flags, its, steps = number(g[1]), int(g[2]), number(g[3]), number(g[4]), int(g[5]), int(g[6]), int(g[7])
        gm, gu, row, their_steps = gdiff_rule.site(s)
        assert flags == 0, s                                                             # both fits converged within the cap
        assert df == row[4], s
        if row[3] == 1.0 and row[7] == 0.0 and their_steps == 0:
            assert (p, phi, stat) == (1.0, 1.0, 0.0) or stat < 1e-20, s                    # degenerate, or no difference at all
            continue
        k = sum(1 for m, u in zip(d[0], d[1]) if m + u > 0)
        q = d[3]
        assert row[5] == q
        allowed = bound(steps, df, q, k, q + 1) + (gdiff_rule.C_STEPS * their_steps + gdiff_rule.C_NU * (df + q) + gdiff_rule.C_CONST) * 2.0 ** -53
        longest = max(longest, its)
        separated += any(a == 0 or b == 0 for a, b in zip(gm, gu))
        tested += 1
        for ours_v, its_v in ((phi, row[6]), (stat, row[7])) + (((p, row[3]),) if row[3] >= 1e-280 else ()):
            r = abs(ours_v - its_v) / its_v / allowed
            worst = max(worst, r)
            assert r <= 1.0, (s, ours_v, its_v, r)
    print(f"worst difference / the sum of the bounds {worst:.4f}; {tested} sites tested, {separated} of them with a separated group; the longest fit {longest} passes")
    assert tested > 450 and separated > 40 and longest <= mdiff_rule.MAX_PASSES


def test_calibration_on_a_paired_design():
    """The reason for the test: 4,000 sites without a group effect, six patients with a sample in either group, depth 20 to 40, a patient
    effect of standard deviation 1 on the logit scale and every sample's fraction a beta draw with intra-class correlation 0.2.  With a
    dummy per patient beside the group the header rejects between 2 % and 8 % of them at 0.05, the band of the two other F tests.
    Measured: 5.775 %; mdk_qdiff_core.h's test of the two groups, which cannot see the pairs, rejects 1.200 %.  At 21 of the sites the
    first patient's two samples are all methylated: the intercept runs off, the full fit goes on from where the reduced one ended, and
    after some 37 passes a pivot is lost among the roundings (MDIFF_NUMERIC: p = 1.0, no rejection).  A dummy for EVERY patient and no
    intercept has no such reference level to lose: 5.850 % and no site flagged."""
    import qdiff_rule
    null = paired_null_sites()
    assert len(null) == 4000 and all(len(s[0]) == 12 and len(s[2][0]) == 7 and s[3] == 1 for s in null)
    got = emu(null)
    for s, g in zip(null[:150], got):
        assert g == rule(s)
    assert all(g[0] == "0" and g[2] == "5" and int(g[5]) in (0, NUMERIC) for g in got)
    lost = sum(1 for g in got if int(g[5]))
    rate = sum(1 for g in got if number(g[1]) < 0.05) / len(got)
    unpaired = sum(1 for ms, us, _, _ in null if qdiff_rule.site(ms[0::2], us[0::2], ms[1::2], us[1::2])[0][5] < 0.05) / len(null)
    print(f"rejected at 0.05: {100 * rate:.3f} % (the model with a dummy per patient), {100 * unpaired:.3f} % (the two-group F test without them); {lost} sites lost a pivot")
    assert 0.02 <= rate <= 0.08
