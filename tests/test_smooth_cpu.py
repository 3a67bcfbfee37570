"""CPU-only: kernel-weighted methylation levels (csrc/mdk_smooth_core.h), driven through tools/smooth_emu -- the host build of the header in
the kernels' blocking: its results against the restatement in Python floats (tests/smooth_rule.py) bit for bit and under several
blockings, hand cases, the two facts the kernels rely on, the sums against exact rationals, the weight against the exact tricube, and
the refusals."""
import random
import subprocess
from fractions import Fraction

import pytest

import smooth_rule as rule
from conftest import REPO
from smooth_tables import PARAMS, expected, shared_table

EMU = REPO / "tools" / "_build" / "smooth_emu"
U = Fraction(1, 2 ** 53)
BLOCKINGS = ((256, 384, 8), (64, 64, 2), (1, 1, 1), (7, 5, 3), (300, 1000, 16))
SIZES = (1, 2, 65, 300)


def table_text(contig, start, m, u, half_bases, min_sites, kernel, blocking=BLOCKINGS[0]):
    S, n = len(m), len(start)
    lines = ["%d %d %d %d %d %d %d %d" % ((half_bases, min_sites, kernel, S, n) + tuple(blocking))]
    lines += ["%d %d" % cx for cx in zip(contig, start)]
    for s in range(S):
        lines += ["%d %d" % e for e in zip(m[s], u[s])]
    return "\n".join(lines) + "\n"


def run(text, shapes):
    """the emulator's results for the tables of `text`, `shapes` their (S, n): per table (err, site) for a refused one, otherwise
    (level, depth, nsites, half, lo) -- level and depth lists per sample of 64-bit patterns"""
    r = subprocess.run([str(EMU)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = iter(r.stdout.splitlines())
    out = []
    for S, n in shapes:
        err, site = (int(v) for v in next(lines).split("\t"))
        if err:
            out.append((err, site))
            continue
        rows = [[int(v) for v in next(lines).split("\t")] for _ in range(n)]
        vals = [[[int(v, 16) for v in next(lines).split("\t")] for _ in range(n)] for _ in range(S)]
        out.append(([[v[0] for v in s] for s in vals], [[v[1] for v in s] for s in vals], [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]))
    assert next(lines, None) is None
    return out


def emu(contig, start, m, u, half_bases, min_sites, kernel, blocking=BLOCKINGS[0]):
    return run(table_text(contig, start, m, u, half_bases, min_sites, kernel, blocking), [(len(m), len(start))])[0]


def one(x, m, u, half_bases, min_sites, kernel, contig=None):
    """a one-sample table through the emulator AND the rule, which must agree: (level as floats, depth as floats, nsites, half)"""
    contig = [0] * len(x) if contig is None else contig
    got = emu(contig, x, [m], [u], half_bases, min_sites, kernel)
    want = rule.smooth(contig, x, [m], [u], half_bases, min_sites, kernel)
    assert got[:4] == want
    return [rule.from_bits(b) for b in got[0][0]], [rule.from_bits(b) for b in got[1][0]], got[2], got[3]


@pytest.mark.parametrize("n", SIZES)
def test_emulator_is_the_rule(n):
    """seeded tables, every parameter pair, both kernels, S of 1 and 3: all four outputs bit for bit"""
    for S in (1, 3):
        contig, start, m, u = shared_table(n, S, 7 * n + S)
        for hb, ms in PARAMS:
            for kernel in (rule.TRICUBE, rule.FLAT):
                got = emu(contig, start, m, u, hb, ms, kernel)
                assert got[:4] == expected(n, S, 7 * n + S, hb, ms, kernel), (n, S, hb, ms, kernel)


def test_blockings_agree():
    """(tile, chunk, batch) of the defaults, of the GPU test's limits, of one row each, odd ones, and larger than the table: identical output"""
    n, S = 300, 5
    contig, start, m, u = shared_table(n, S, 11)
    for hb, ms in ((50, 7), (500, 70), (3, 200)):
        for kernel in (rule.TRICUBE, rule.FLAT):
            outs = run("".join(table_text(contig, start, m, u, hb, ms, kernel, b) for b in BLOCKINGS), [(S, n)] * len(BLOCKINGS))
            assert outs[0][:4] == expected(n, S, 11, hb, ms, kernel)
            assert all(o == outs[0] for o in outs[1:])


def test_hand_cases():
    """Worked by hand.
    x = [0, 10, 20], (m, u) = (1, 1), (2, 0), (3, 3), half_bases 10, min_sites 1: k = 1, d_k = 0, half = 10 everywhere; site 1's window
      is [0, 20], all three rows; sites 0 and 2 see two.  Tricube: a neighbour at d = 10 = half weighs 0, so every site keeps its own
      level and depth: 1/2, 2/2, 3/6.  Flat: site 1 gets the sums of all three, 6 / 10; site 0 gets 3 / 4, site 2 gets 5 / 8.
    A one-site contig (between two others): k = 1 whatever min_sites is, half = half_bases, one row.
    A contig of 3 sites x = [0, 100, 1000] with min_sites 5: k = 3, d_k = 1000, 900, 1000: the window is the whole contig.
    x = [0, 10, 20, 30, 40], half_bases 0, min_sites 2: d_k = 10 everywhere; the inner sites have BOTH neighbours at d_k and hold 3 rows.
    half_bases 0, min_sites 1: the site alone: level m / (m + u), depth m + u, and the quiet NaN 0x7ff8000000000000 without coverage."""
    x, m, u = [0, 10, 20], [1, 2, 3], [1, 0, 3]
    assert one(x, m, u, 10, 1, rule.TRICUBE) == ([0.5, 1.0, 0.5], [2.0, 2.0, 6.0], [2, 3, 2], [10, 10, 10])
    assert one(x, m, u, 10, 1, rule.FLAT) == ([0.75, 0.6, 0.625], [4.0, 10.0, 8.0], [2, 3, 2], [10, 10, 10])
    for kernel in (rule.TRICUBE, rule.FLAT):
        level, depth, nsites, half = one([5, 7, 9], [4, 1, 4], [4, 3, 4], 100, 5, kernel, contig=[0, 2, 3])
        assert (level, depth, nsites, half) == ([0.5, 0.25, 0.5], [8.0, 4.0, 8.0], [1, 1, 1], [100, 100, 100])
    level, depth, nsites, half = one([0, 100, 1000], [1, 1, 1], [0, 0, 0], 10, 5, rule.FLAT)
    assert (level, depth, nsites, half) == ([1.0, 1.0, 1.0], [3.0, 3.0, 3.0], [3, 3, 3], [1000, 900, 1000])
    level, depth, nsites, half = one([0, 100, 1000], [1, 1, 1], [0, 0, 0], 10, 5, rule.TRICUBE)
    assert (nsites, half) == ([3, 3, 3], [1000, 900, 1000])
    w100, w900 = rule.weight(rule.TRICUBE, 100, 1000), rule.weight(rule.TRICUBE, 900, 1000)
    assert depth == [1.0 + w100, rule.weight(rule.TRICUBE, 100, 900) + 1.0, w900 + 1.0] and 0.0 < w900 < 0.02 < 0.99 < w100 < 1.0         # (a row at d = half weighs 0)
    level, depth, nsites, half = one([0, 10, 20, 30, 40], [1] * 5, [1] * 5, 0, 2, rule.FLAT)
    assert (nsites, half, depth) == ([2, 3, 3, 3, 2], [10] * 5, [4.0, 6.0, 6.0, 6.0, 4.0])
    for kernel in (rule.TRICUBE, rule.FLAT):
        got = emu([0] * 4, [3, 4, 5, 9], [[1, 0, 3, 0]], [[2, 0, 0, 7]], 0, 1, kernel)
        assert got[0][0] == [rule.bits(1 / 3), 0x7FF8000000000000, rule.bits(1.0), rule.bits(0.0)]
        assert got[1][0] == [rule.bits(3.0), rule.bits(0.0), rule.bits(3.0), rule.bits(7.0)]
        assert got[2:4] == ([1] * 4, [0] * 4)


def brute_windows(contig, start, half_bases, min_sites):
    """every site's (lo, hi, half) with nothing assumed: the k-th smallest distance, then every row of the contig tried"""
    out = []
    for i in range(len(start)):
        rows = [j for j in range(len(start)) if contig[j] == contig[i]]
        half = max(half_bases, sorted(abs(start[j] - start[i]) for j in rows)[min(min_sites, len(rows)) - 1])
        inside = [j for j in rows if abs(start[j] - start[i]) <= half]
        assert inside == list(range(inside[0], inside[-1] + 1))
        out.append((inside[0], inside[-1] + 1, half))
    return out


def test_windows_are_monotone_and_capped():
    """the two facts the kernels rely on, by brute force on random tables: lo and hi never fall from a site to the next, and a window
    holds at most max(2 half_bases + 1, 2 min_sites - 1) sites; the emulator's windows are the brute-force ones"""
    rng = random.Random(5)
    texts, shapes, wants = [], [], []
    for _ in range(600):
        n = rng.randint(1, 40)
        contig, start, c, x = [], [], 0, rng.randint(0, 50)
        for _ in range(n):
            contig.append(c); start.append(x)
            if rng.random() < 0.1:
                c += 1; x = rng.randint(0, 50)
            else:
                x += rng.choice((1, 1, 1, 2, 3, 10, 100, rng.randint(1, 3000)))
        hb, ms = rng.choice((0, 1, 2, 5, 20, 100, 1000)), rng.choice((1, 2, 3, 4, 7, 20, 70))
        win = brute_windows(contig, start, hb, ms)
        assert win == rule.windows(contig, start, hb, ms)
        cap = max(2 * hb + 1, 2 * ms - 1)
        for i, (lo, hi, _) in enumerate(win):
            assert lo <= i < hi and hi - lo <= cap
            assert i == 0 or (win[i - 1][0] <= lo and win[i - 1][1] <= hi), (contig, start, hb, ms, i)
        texts.append(table_text(contig, start, [[1] * n], [[0] * n], hb, ms, rule.FLAT)); shapes.append((1, n)); wants.append(win)
    for got, win in zip(run("".join(texts), shapes), wants):
        assert (got[4], got[2], got[3]) == ([w[0] for w in win], [w[1] - w[0] for w in win], [w[2] for w in win])


def test_sums_against_exact_rationals():
    """flat: level is the correctly rounded quotient of the integer sums.  Tricube: within (2 nsites + 2) 2^-53, relative, of rational
    arithmetic over the rule's own double weights -- a product and a sum round once per row and sum, the quotient once"""
    n, S = 300, 3
    contig, start, m, u = shared_table(n, S, 11)
    worst = Fraction(0)
    for hb, ms in ((50, 7), (500, 70)):
        win = rule.windows(contig, start, hb, ms)
        flat, cube = emu(contig, start, m, u, hb, ms, rule.FLAT), emu(contig, start, m, u, hb, ms, rule.TRICUBE)
        for s in range(S):
            for i, (lo, hi, half) in enumerate(win):
                M, D = sum(m[s][lo:hi]), sum(m[s][lo:hi]) + sum(u[s][lo:hi])
                assert flat[0][s][i] == (rule.bits(float(Fraction(M, D))) if D else rule.NAN_BITS) and flat[1][s][i] == rule.bits(float(D))
                w = [Fraction(rule.weight(rule.TRICUBE, abs(start[j] - start[i]), half)) for j in range(lo, hi)]
                M = sum(wj * m[s][j] for wj, j in zip(w, range(lo, hi)))
                D = sum(wj * (m[s][j] + u[s][j]) for wj, j in zip(w, range(lo, hi)))
                if not D:
                    assert cube[0][s][i] == rule.NAN_BITS and cube[1][s][i] == 0
                    continue
                level, depth = Fraction(rule.from_bits(cube[0][s][i])), Fraction(rule.from_bits(cube[1][s][i]))
                assert abs(depth - D) <= (hi - lo) * U * D
                if not M:
                    assert level == 0
                    continue
                err = abs(level - M / D) / (M / D) / ((2 * (hi - lo) + 2) * U)
                worst = max(worst, err)
                assert err <= 1, (s, i, float(err))
    print("worst share of the bound: %.3f" % float(worst))


def test_weight_against_the_exact_tricube():
    """|w - (1 - (d / half)^3)^3| <= 32 * 2^-53 on a grid of half <= 2^20, for the Python restatement and, through a two-row table
    whose second row alone has depth 1 -- the first site's depth is then that row's weight --, for the host build of the header"""
    rng = random.Random(9)
    grid = []
    for half in (1, 2, 3, 7, 10, 999, 1000, 1 << 10, 65537, (1 << 20) - 1, 1 << 20):
        ds = range(half + 1) if half <= 10 else sorted({0, 1, 2, half // 2, half - 2, half - 1, half} | {rng.randint(0, half) for _ in range(150)})
        grid += [(half, d) for d in ds]
    outs = run("".join(table_text([0, 0], [0, max(d, 1)], [[0, 0]], [[0, 1]], half, 1, rule.TRICUBE) for half, d in grid if d), [(1, 2)] * sum(1 for _, d in grid if d))
    outs = iter(outs)
    worst = Fraction(0)
    for half, d in grid:
        w = rule.weight(rule.TRICUBE, d, half)
        if d:
            assert next(outs)[1][0][0] == rule.bits(w), (half, d)
        err = abs(Fraction(w) - (1 - Fraction(d, half) ** 3) ** 3) / U
        worst = max(worst, err)
        assert err <= 32 and (w > 0.0) == (d < half)
    assert rule.weight(rule.TRICUBE, 0, 0) == 1.0 and rule.weight(rule.FLAT, 5, 5) == 1.0
    print("worst: %.2f * 2^-53" % float(worst))


def test_refusals():
    """every refusal gives its bit and names the smallest refused site, under any blocking; the largest accepted entry is accepted"""
    n, S = 65, 3
    contig, start, m, u = (list(v) if i < 2 else [list(r) for r in v] for i, v in enumerate(shared_table(n, S, 7 * n + S)))
    inner = next(i for i in range(2, n) if contig[i - 1] == contig[i])

    def changed(edit):
        c, x, mm, uu = list(contig), list(start), [list(r) for r in m], [list(r) for r in u]
        edit(c, x, mm, uu)
        return c, x, mm, uu

    def equal_start(c, x, mm, uu): x[inner] = x[inner - 1]
    def descending(c, x, mm, uu): x[inner] = x[inner - 1] - 1
    def contig_back(c, x, mm, uu): c[n - 1] = c[0] if c[n - 1] != c[0] else -5
    def negative_contig(c, x, mm, uu): c[0] = -1
    def negative_start(c, x, mm, uu): x[0] = -1
    def negative_count(c, x, mm, uu): uu[2][40] = -1
    def large_count(c, x, mm, uu): mm[1][64] = 1 << 26
    def both(c, x, mm, uu): x[inner] = x[inner - 1]; mm[0][inner - 1] = -3; uu[1][inner - 1] = 1 << 30
    def later_entry(c, x, mm, uu): x[inner] = x[inner - 1]; mm[0][n - 1] = -3

    cases = [(equal_start, (rule.E_ORDER, inner)), (descending, (rule.E_ORDER, inner)), (negative_contig, (rule.E_POSITION, 0)),
             (negative_start, (rule.E_POSITION, 0)), (negative_count, (rule.E_NEGATIVE, 40)), (large_count, (rule.E_ENTRY, 64)),
             (both, (rule.E_NEGATIVE, inner - 1)), (later_entry, (rule.E_ORDER, inner))]
    for edit, want in cases:
        t = changed(edit)
        assert rule.refusal(*t) == want, edit.__name__
        for b in BLOCKINGS:
            for kernel in (rule.TRICUBE, rule.FLAT):
                assert emu(*t, 50, 7, kernel, b) == want, (edit.__name__, b)
    t = changed(contig_back)
    assert rule.refusal(*t)[0] == rule.E_ORDER and emu(*t, 50, 7, rule.TRICUBE) == rule.refusal(*t)
    t = changed(lambda c, x, mm, uu: mm[1].__setitem__(64, (1 << 26) - 1))
    assert rule.refusal(*t) is None and emu(*t, 50, 7, rule.FLAT)[:4] == rule.smooth(*t, 50, 7, rule.FLAT)


def test_arguments_are_refused_without_a_device():
    """smooth_counts checks its arguments before the library is touched: parameters out of range, an unknown kernel, dtypes and shapes,
    and CPU tensors -- there is no CPU path"""
    import torch
    import methyldackel_amd as mdk
    c, x = torch.zeros(4, dtype=torch.int32), torch.arange(4, dtype=torch.int32)
    m = torch.ones((2, 4), dtype=torch.int32)
    for kw, text in ((dict(half_bases=-1), "half_bases"), (dict(half_bases=(1 << 20) + 1), "half_bases"), (dict(min_sites=0), "min_sites"),
                     (dict(min_sites=(1 << 16) + 1), "min_sites"), (dict(min_sites=7.0), "min_sites"), (dict(kernel="gauss"), "unknown kernel 'gauss'")):
        with pytest.raises(mdk.MdkError, match=text):
            mdk.smooth_counts(c, x, m, m, **kw)
    for args, text in (((c, x, m, m[:1]), "one dtype and one shape"), ((c, x, m, m.long()), "one dtype and one shape"), ((c, x[:3], m, m), "sites"),
                       ((c.long(), x, m, m), "int32"), ((c, x, m[0], m[0]), r"\[samples, sites\]"), ((c, x, m, m), "no CPU path")):
        with pytest.raises(mdk.MdkError, match=text):
            mdk.smooth_counts(*args)
    cols = {"contig": c, "start": x, "end": x + 1, "context": torch.zeros(4, dtype=torch.uint8), "strand": torch.zeros(4, dtype=torch.int8), "nsamples": c + 2}
    with pytest.raises(mdk.MdkError, match="no CPU path"):
        mdk.Cohort(["chr1"], cols, m, m).smooth()
    with pytest.raises(mdk.MdkError, match="no CPU path"):
        mdk.Cohort(["chr1"], cols, m, m).sample(0).smooth(half_bases=5, min_sites=1, kernel="flat")
