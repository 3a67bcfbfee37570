"""CPU-only: the test of two groups per site (csrc/mdk_diff_core.h, the functions the kernel of csrc/mdk_diff.hip runs), driven through
tools/diff_emu: its p-values against the restatement in Python floats (tests/diff_rule.py) bit for bit, and against exact rational
arithmetic; and what mdk.diff_counts and Cohort.diff refuse without a device."""
import struct
import subprocess
from fractions import Fraction
from math import comb

import pytest

import methyldackel_amd as mdk
from conftest import REPO
from diff_rule import ACCEPTED, HAND, LIMIT, REFUSED, bits, entry_check, exact, margin_check, meth_diff, pvalue, seeded

EMU = REPO / "tools" / "_build" / "diff_emu"
U = Fraction(1, 2 ** 53)


def emu(tables):
    r = subprocess.run([str(EMU)], input="".join("%d\t%d\t%d\t%d\n" % t for t in tables), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return [tuple(int(x, 16) if k in (1, 2) else int(x) for k, x in enumerate(l.split("\t"))) for l in r.stdout.splitlines()]


def emu_pvalue(tables):
    """(p, steps) of every table as the host build of the header gives them"""
    return [(struct.unpack("<d", struct.pack("<Q", g[1]))[0], g[3]) for g in emu(tables)]


def rule(t):
    """what the emulator prints for an accepted table"""
    p, steps = pvalue(*t)
    return (0, bits(p) & (2 ** 64 - 1), bits(meth_diff(*t)) & (2 ** 64 - 1), steps)


@pytest.fixture(scope="module")
def tables():
    return seeded() + [t for _, t, _ in HAND] + ACCEPTED


def test_emulator_equals_the_rule_bit_for_bit(tables):
    got = emu(tables)
    assert len(got) == len(tables)
    for t, g in zip(tables, got):
        assert g == rule(t), t


def test_header_against_exact_rationals(tables):
    """The p-values and `steps` are the header's, from tools/diff_emu.  For every table whose exact p is at least 1e-280 the p is within (4 steps + 8) 2^-53 of it, relatively: two roundings a
    term, carried into two sums.  Measured over these tables (1669 of them at or above 1e-280): the worst error is 0.1393 of its bound (table (2, 6, 3, 0),
    4 terms); the largest relative error is 3.57e-15.  Where the observed table's exact weight is below 2^-961 of the mode's the
    rule gives 0.0, and it gives 0.0 only where the exact p is below 1e-280."""
    worst, worst_err, cut, checked, zeros = Fraction(0), Fraction(0), Fraction(1, 2 ** 961), 0, 0
    at = None
    for t, (p, steps) in zip(tables, emu_pvalue(tables)):
        want, ratio = exact(*t)
        assert 0.0 <= p <= 1.0
        if want >= Fraction(1, 10 ** 280):
            err = abs(Fraction(p) - want) / want
            bound = (4 * steps + 8) * U
            if err / bound > worst:
                worst, at = err / bound, (t, steps)
            worst_err = max(worst_err, err)
            assert err <= bound, (t, p, float(err), float(bound))
            checked += 1
        if ratio < cut:
            assert p == 0.0, t
        if p == 0.0:
            assert want < Fraction(1, 10 ** 280), t
            zeros += 1
    print(f"worst error / bound {float(worst):.4f} at {at}; worst relative error {float(worst_err):.3e}; {checked} tables checked, {zeros} give 0.0")
    assert checked > 1000 and zeros > 50


@pytest.mark.parametrize("name,t,p", HAND, ids=[h[0] for h in HAND])
def test_by_hand(name, t, p):
    (got,) = emu([t])
    assert got == rule(t)
    if p is not None:
        assert pvalue(*t)[0] == p
    if name == "symmetric tie":
        # (7, 2, 2, 7) and (2, 7, 7, 2) weigh the same: both tails count, exactly twice the one from 7 up
        a, b, c, d = t
        upper = Fraction(sum(comb(a + c, k) * comb(b + d, a + b - k) for k in range(a, a + b + 1)), comb(a + b + c + d, a + b))
        assert exact(*t)[0] == 2 * upper
        assert abs(Fraction(pvalue(*t)[0]) - 2 * upper) / (2 * upper) <= (4 * pvalue(*t)[1] + 8) * U and pvalue(*t)[0] == pvalue(b, a, d, c)[0]
    if name.startswith("no coverage") or name.startswith("lo == hi"):
        assert pvalue(*t) == (1.0, 0)
    if name.startswith("no coverage"):
        assert meth_diff(*t) == 0.0 and got[2] == 0
    if name == "apart":
        assert got[1] == 0 and meth_diff(*t) == -100.0
    if name == "largest margins":
        assert margin_check(*t) == 0 and max(t[0] + t[2], t[2] + t[3]) == LIMIT - 2 and 0.0 < pvalue(*t)[0] < 1e-30


def test_symmetric_tables_count_both_tails():
    """the far tail's term comes down another side of the mode than the observed one: other roundings, the same weight -- the bar's
    1e-7 takes it in.  The header's p-values, from tools/diff_emu"""
    pairs = ((9, 1), (30, 12), (250, 180), (3, 3), (700, 650))
    got = emu_pvalue([(x, y, y, x) for x, y in pairs] + [(y, x, x, y) for x, y in pairs])
    for k, (x, y) in enumerate(pairs):
        want = exact(x, y, y, x)[0]
        p, steps = got[k]
        assert abs(Fraction(p) - want) / want <= (4 * steps + 8) * U
        if x != y:
            # one tail alone is half of it
            upper = Fraction(sum(comb(x + y, k) * comb(x + y, x + y - k) for k in range(x, x + y + 1)), comb(2 * (x + y), x + y))
            assert want == 2 * upper and p == got[len(pairs) + k][0]


@pytest.mark.parametrize("name,t,bit", REFUSED, ids=[f"{r[0]}{i}" for i, r in enumerate(REFUSED)])
def test_refused_just_outside(name, t, bit):
    (got,) = emu([t])
    err = 0
    for v in t:
        err |= entry_check(v)
    assert got == (err or margin_check(*t), 0, 0, 0) and got[0] == bit


def test_accepted_just_inside():
    for t, g in zip(ACCEPTED, emu(ACCEPTED)):
        assert g == rule(t) and g[0] == 0


def matrices(rows=((3, 1, 5), (1, 3, 0), (2, 2, 2)), dtype=None):
    import torch
    m = torch.tensor(rows, dtype=dtype or torch.int32)
    return m, m.clone()


def test_refused_without_a_device():
    import torch
    m, u = matrices()
    with pytest.raises(mdk.MdkError, match="compared on the device.*no CPU path"):
        mdk.diff_counts(m, u, [0], [1, 2])
    with pytest.raises(mdk.MdkError, match="one dtype and one shape"):
        mdk.diff_counts(m, u.to(torch.int64), [0], [1])
    with pytest.raises(mdk.MdkError, match="one dtype and one shape"):
        mdk.diff_counts(m, u[:, :2], [0], [1])
    with pytest.raises(mdk.MdkError, match="int32 or int64"):
        mdk.diff_counts(m.to(torch.int16), u.to(torch.int16), [0], [1])
    with pytest.raises(mdk.MdkError, match=r"\[samples, sites\]"):
        mdk.diff_counts(m[0], u[0], [0], [1])
    for a, b in (([3], [1]), ([0], [-1]), ([0], [1, 1.5]), ([True], [1])):
        with pytest.raises(mdk.MdkError, match="samples 0 to 2"):
            mdk.diff_counts(m, u, a, b)
    with pytest.raises(mdk.MdkError, match="sample 1 is in both groups"):
        mdk.diff_counts(m, u, [0, 1], [1, 2])
    with pytest.raises(mdk.MdkError, match="group a is empty"):
        mdk.diff_counts(m, u, [], [1])
    with pytest.raises(mdk.MdkError, match="group b is empty"):
        mdk.diff_counts(m, u, [0], [])
    with pytest.raises(mdk.MdkError, match="1 to 1024 samples"):
        mdk.diff_counts(torch.zeros((1025, 1), dtype=torch.int32), torch.zeros((1025, 1), dtype=torch.int32), [0], [1])
    # strided and transposed matrices: the kernel would read other entries
    wide = torch.zeros((3, 6), dtype=torch.int32)
    for bad in (wide[:, ::2], torch.zeros((3, 3), dtype=torch.int32).t()):
        with pytest.raises(mdk.MdkError, match="nmeth must be contiguous"):
            mdk.diff_counts(bad, bad.contiguous(), [0], [1])
        with pytest.raises(mdk.MdkError, match="nunmeth must be contiguous"):
            mdk.diff_counts(bad.contiguous(), bad, [0], [1])
    cols = {n: torch.zeros(3, dtype=getattr(torch, dt)) for n, dt in mdk.SITE_COLUMNS}
    cohort = mdk.Cohort(["a"], cols, m, u)
    with pytest.raises(mdk.MdkError, match="no CPU path"):
        cohort.diff([0], [1, 2])
    with pytest.raises(mdk.MdkError, match="both groups"):
        cohort.diff([0, 2], [2])
    assert "md_text_diff" in mdk.HIP_SYMBOLS


def test_diff_columns_and_file_format(tmp_path):
    """Diff without a device: select, rows and the file, whose doubles read back to the same bits"""
    import torch
    vals = {"contig": [0, 0, 1], "start": [5, 9, 2], "end": [6, 10, 3], "context": [0, 0, 2], "strand": [1, -1, 0], "nmeth_a": [3, 0, 5000], "nunmeth_a": [1, 0, 0],
            "nmeth_b": [1, 12, 0], "nunmeth_b": [3, 30, 5000], "meth_diff": [meth_diff(3, 1, 1, 3), 0.0, -100.0], "pvalue": [pvalue(3, 1, 1, 3)[0], 1.0, 2.0 ** -700 / 3]}
    d = mdk.Diff(["chr1", "chrM"], {n: torch.tensor(vals[n], dtype=getattr(torch, dt)) for n, dt in mdk.Diff.COLUMNS}, merged=True)
    assert len(d) == 3 and d.merged
    rows = d.rows()
    assert rows[0] == ("chr1", 5, 6, 0, 1, 3, 1, 1, 3, -50.0, 0.48571428571428577) and rows[2][0] == "chrM"
    path = d.write(str(tmp_path / "d.tsv"))
    back = [l.rstrip("\n").split("\t") for l in open(path)]
    assert [tuple([r[0]] + [int(x) for x in r[1:9]] + [float(x) for x in r[9:]]) for r in back] == rows
    s = d.select(torch.tensor([True, False, True]))
    assert s.rows() == [rows[0], rows[2]] and s.merged and s.contigs == d.contigs
    q = d.qvalue().tolist()
    from diff_rule import bh
    assert q == bh(vals["pvalue"])
