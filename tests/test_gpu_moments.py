"""GPU: the pairwise sample moments on the device (csrc/mdk_moments.hip in libmdk_stats.so) -- mdk.sample_moments, mdk.moments_limits,
Cohort.moments, CohortRegions.moments and their SampleMoments.  Every comparison of integers is exact and the doubles cxy and vxx are
compared as bit patterns, against the restatement in Python ints (tests/moments_rule.py); mean() is the correctly rounded quotient, and
correlation() and covariance() are held to 8 and 4 units of 2^-53 in exact rationals."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import moments_rule as rule
from moments_tables import check_mix, expected, limit_matrices, table

pytestmark = pytest.mark.gpu
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 4100)
SAMPLES = (1, 2, 3, 12, 17, 65)
U = Fraction(1, 2 ** 53)
MASK = (1 << 64) - 1


def device(a, dtype="int64"):
    import torch
    return torch.from_numpy(np.array(a)).to(getattr(torch, dtype)).cuda().contiguous()      # (a copy: the shared tables are read-only)


def patterns(t):
    import torch
    return [[v & MASK for v in row] for row in t.view(torch.int64).cpu().tolist()]


def results(mo):
    """a SampleMoments as tests/moments_tables.expected gives one"""
    return tuple(t.cpu().tolist() for t in (mo.n, mo.sx, mo.sxx, mo.sxy)) + (patterns(mo.cxy), patterns(mo.vxx))


@pytest.fixture(autouse=True)
def default_limits():
    import methyldackel_amd as mdk
    yield
    mdk.moments_limits()


@pytest.mark.parametrize("n", SIZES)
def test_tables_against_the_rule(n):
    """every S at this n, int32 and int64 taking turns, min_depth 1 and 5: the default shape and, up to 17 samples, each shape forced --
    all six matrices; the inputs as they were; a second run the same bits"""
    import torch
    import methyldackel_amd as mdk
    for turn, S in enumerate(SAMPLES):
        m, u = table(S, n)
        dtype = ("int32", "int64")[(turn + SIZES.index(n)) % 2]
        dm, du = device(m, dtype), device(u, dtype)
        for min_depth in (1, 5):
            check_mix(m, u, min_depth)
            want = expected(S, n, min_depth)
            for shape in ("auto", "lanes", "staged") if S <= 17 else ("auto",):
                mdk.moments_limits(shape=shape)
                mo = mdk.sample_moments(dm, du, min_depth)
                assert results(mo) == want, (S, n, dtype, min_depth, shape)
                assert (mo.n_samples, mo.min_depth, mo.names) == (S, min_depth, None)
                assert all(t.dtype == torch.int64 and tuple(t.shape) == (S, S) and t.is_cuda for t in (mo.n, mo.sx, mo.sxx, mo.sxy))
                assert all(t.dtype == torch.float64 and tuple(t.shape) == (S, S) for t in (mo.cxy, mo.vxx))
            assert results(mdk.sample_moments(dm, du, min_depth)) == want                  # once more
        assert np.array_equal(dm.cpu().numpy(), m) and np.array_equal(du.cpu().numpy(), u)


def test_1024_samples():
    import torch
    import methyldackel_amd as mdk
    S, n = 1024, 65
    m, u = table(S, n)
    check_mix(m, u, 1)
    sums = rule.moments_np(m, u, 1)
    mo = mdk.sample_moments(device(m, "int32"), device(u, "int32"), 1)
    for got, want in zip((mo.n, mo.sx, mo.sxx, mo.sxy), sums):
        assert np.array_equal(got.cpu().numpy(), want)
    cxy, vxx = patterns(mo.cxy), patterns(mo.vxx)
    N, SX, SXX, SXY = (a.tolist() for a in sums)
    cells = [(i, i) for i in range(0, S, 37)] + [(i, j) for i in range(0, S, 61) for j in range(0, S, 53)] + [(S - 1, S - 1), (S - 1, 0), (2, 3), (4, 5), (5, 4), (0, 7)]
    for i, j in cells:
        assert cxy[i][j] == rule.bits(float(N[i][j] * SXY[i][j] - SX[i][j] * SX[j][i])), (i, j)
        assert vxx[i][j] == rule.bits(float(N[i][j] * SXX[i][j] - SX[i][j] ** 2)), (i, j)
    assert torch.equal(mo.cxy, mo.cxy.t())


@pytest.mark.parametrize("shape", ["lanes", "staged"])
def test_levels_of_every_magnitude(shape):
    """1024 samples of one site each, seeded counts of 1 to 26 bits and depths next to powers of two: the diagonal of sx is the cell's
    level, whose division is an estimate in floats put right in integers"""
    import random
    import torch
    import methyldackel_amd as mdk
    rnd = random.Random(20240614)
    top = rule.LIMIT - 1
    cells = [(top, 0), (0, top), (top, top), (top, 1), (1, top), (top - 1, top), (1, 2), (1, 1)]
    for k in range(2, 27):
        for d in ((1 << k) - 1, (1 << k) + 1):
            cells += [(a, d - a) for a in (d // 2 - 1, d // 2, d // 2 + 1, d // 3) if 0 <= a <= min(d, top) and d - a <= top]
    while len(cells) < 1024:
        a, b = rnd.randrange(1 << rnd.randrange(1, 27)), rnd.randrange(1 << rnd.randrange(1, 27))
        cells.append((a, b) if a + b else (1, 0))
    cells = cells[:1024]
    m, u = np.array([[a] for a, _ in cells], dtype=np.int64), np.array([[b] for _, b in cells], dtype=np.int64)
    mdk.moments_limits(shape=shape)
    mo = mdk.sample_moments(device(m, "int32"), device(u, "int32"))
    assert torch.diagonal(mo.sx).cpu().tolist() == [rule.level(a, b) for a, b in cells]
    assert torch.diagonal(mo.n).cpu().tolist() == [1] * 1024


@pytest.mark.parametrize("S,n,dtype", [(3, 257, "int64"), (12, 4100, "int32"), (17, 4100, "int64"), (65, 4100, "int32"), (65, 65, "int64")])
def test_small_blocking_gives_the_same(S, n, dtype):
    """chunks of 64 sites, the smallest pair tile and 3 workgroups, in either shape: the matrices of the defaults"""
    import methyldackel_amd as mdk
    m, u = table(S, n)
    dm, du = device(m, dtype), device(u, dtype)
    for min_depth in (1, 5):
        want = expected(S, n, min_depth)
        assert results(mdk.sample_moments(dm, du, min_depth)) == want
        for limits in (dict(shape="lanes", chunk_sites=64, pair_tile=1, max_workgroups=3), dict(shape="staged", chunk_sites=64, pair_tile=1, max_workgroups=3),
                       dict(shape="staged", chunk_sites=192, pair_tile=2, max_workgroups=5), dict(shape="lanes", pair_tile=2), dict(shape="staged", pair_tile=4, max_workgroups=1)):
            mdk.moments_limits(**limits)
            assert results(mdk.sample_moments(dm, du, min_depth)) == want, limits
        mdk.moments_limits()


def test_limits_refusals():
    import methyldackel_amd as mdk
    for bad in (dict(shape=3), dict(shape=-1), dict(chunk_sites=32), dict(chunk_sites=100), dict(chunk_sites=320), dict(chunk_sites=128), dict(chunk_sites=256, pair_tile=2),
                dict(pair_tile=3), dict(pair_tile=8), dict(max_workgroups=-1)):
        with pytest.raises(mdk.MdkError, match="md_stats_moments_limits"):
            mdk.moments_limits(**bad)


def test_the_largest_count_everywhere():
    """every nmeth 2^26 - 1, nunmeth 0, 4100 sites: every x^2 is 2^32, the sums carry past 32 bits from the second site on"""
    import torch
    import methyldackel_amd as mdk
    top, n, S = rule.LIMIT - 1, 4100, 3
    dm = torch.full((S, n), top, dtype=torch.int32, device="cuda")
    du = torch.zeros((S, n), dtype=torch.int32, device="cuda")
    for shape in ("lanes", "staged"):
        mdk.moments_limits(shape=shape)
        mo = mdk.sample_moments(dm, du, 5)
        assert mo.n.cpu().tolist() == [[n] * S] * S and mo.sx.cpu().tolist() == [[n * 65536] * S] * S
        assert mo.sxx.cpu().tolist() == [[n << 32] * S] * S and mo.sxy.cpu().tolist() == [[n << 32] * S] * S
        assert not mo.cxy.any() and not mo.vxx.any()
        assert torch.isnan(mo.correlation()).all() and mo.mean().cpu().tolist() == [[1.0] * S] * S


@pytest.mark.parametrize("shape", ["lanes", "staged"])
def test_entry_refusals_name_the_smallest_site(shape):
    import torch
    import methyldackel_amd as mdk
    mdk.moments_limits(shape=shape, chunk_sites=64, max_workgroups=7)
    S, n = 12, 4100
    m, u = table(S, n)
    for dtype in ("int32", "int64"):
        for changes, want in ((((1, 3000, 0, -1),), (rule.E_NEGATIVE, 3000)), (((11, 77, 1, rule.LIMIT),), (rule.E_ENTRY, 77)),
                              (((2, 4099, 1, -7), (9, 4099, 0, rule.LIMIT)), (rule.E_NEGATIVE, 4099)),
                              (((5, 2000, 0, -1), (6, 130, 1, rule.LIMIT), (7, 131, 1, -1)), (rule.E_ENTRY, 130))):
            mm, uu = m.copy(), u.copy()
            for s, k, which, value in changes:
                (mm, uu)[which][s, k] = value
            assert rule.refusal(mm.tolist(), uu.tolist()) == want
            text = ("a count is negative" if want[0] == rule.E_NEGATIVE else r"a count is 2\^26 or more") + rf" \(site {want[1]}\)"
            with pytest.raises(mdk.MdkError, match="md_stats_moments.*" + text):
                mdk.sample_moments(device(mm, dtype), device(uu, dtype))
        mm = m.copy()
        mm[4, 100] = rule.LIMIT - 1                                 # the largest entry is taken
        assert np.array_equal(mdk.sample_moments(device(mm, dtype), device(u, dtype)).n.cpu().numpy(), rule.moments_np(mm, u, 1)[0])
    big = torch.zeros((2, 70), dtype=torch.int64, device="cuda")
    big[1, 66] = 1 << 40                                            # (no 32 bits hold it)
    with pytest.raises(mdk.MdkError, match=r"a count is 2\^26 or more \(site 66\)"):
        mdk.sample_moments(big, big.clone())


def test_api_refusals():
    import torch
    import methyldackel_amd as mdk
    m = torch.ones((3, 10), dtype=torch.int32, device="cuda")
    u = torch.ones((3, 10), dtype=torch.int32, device="cuda")
    before = dict(mdk._side_handles)
    for args, text in (((m.cpu(), u), "there is no CPU path"), ((m, u.cpu()), "there is no CPU path"), ((m, u.long()), "one dtype and one shape"),
                       ((m, u[:, :9].contiguous()), "one dtype and one shape"), ((m.float(), u.float()), "int32 or int64"), ((m[0], u[0]), r"\[samples, sites\]"),
                       ((m.tolist(), u), r"\[samples, sites\]"), ((m.t(), u.t()), "contiguous"), ((m[:, ::2], u[:, ::2]), "contiguous"),
                       ((m[:0], u[:0]), "1 to 1024 samples"), ((m[:1].expand(1025, 10), u[:1].expand(1025, 10)), "1 to 1024 samples"),
                       ((m[:1, :1].expand(1, (1 << 30) + 1), u[:1, :1].expand(1, (1 << 30) + 1)), "more than 2\\^30")):
        with pytest.raises(mdk.MdkError, match=text):
            mdk.sample_moments(*args)
    for bad in (0, -1, 1 << 26, 1.0, True, None):
        with pytest.raises(mdk.MdkError, match="min_depth"):
            mdk.sample_moments(m, u, bad)
    with pytest.raises(mdk.MdkError):
        mdk.sample_moments(m, u, names=["a", "b"])
    assert dict(mdk._side_handles) == before                        # refused before the library was touched
    assert mdk.sample_moments(m, u, (1 << 26) - 1).n.cpu().tolist() == [[0] * 3] * 3


def center_on_device(sums):
    import methyldackel_amd as mdk
    return mdk._moments_center([device(np.array(a, dtype=np.int64)) for a in sums])


def test_centring_of_hand_written_sums():
    """md_stats_center at the limits of what it accepts, bit for bit, ties among them; and its refusals with the first cell"""
    import methyldackel_amd as mdk
    cases = limit_matrices() + [([[1 << 30] * 2] * 2, [[1 << 38, 1 << 38], [c, c]], [[1 << 62] * 2] * 2, [[1 << 62] * 2] * 2) for c in range(1, 9)]
    for sums in cases:
        assert rule.sums_refusal(*sums) is None
        cxy, vxx = rule.center(*sums)
        got = center_on_device(sums)
        assert (patterns(got[0]), patterns(got[1])) == (rule.pattern(cxy), rule.pattern(vxx)), sums
    ok = ([[4, 4], [4, 4]], [[9, 9], [9, 9]], [[30, 30], [30, 30]], [[30, 20], [20, 30]])
    for q, i, j, value, text in ((0, 0, 1, -1, r"a sum is negative \(cell 0, 1\)"), (3, 1, 0, -2, r"a sum is negative \(cell 1, 0\)"), (0, 1, 1, (1 << 30) + 1, r"n is more than 2\^30 \(cell 1, 1\)"),
                                 (1, 0, 0, 4 * 65536 + 1, r"sx is more than n \* 65536 \(cell 0, 0\)"), (2, 1, 0, (4 << 32) + 1, r"sxx or sxy is more than n \* 2\^32 \(cell 1, 0\)"),
                                 (3, 0, 1, (4 << 32) + 1, r"sxx or sxy is more than n \* 2\^32 \(cell 0, 1\)")):
        sums = [[list(r) for r in mat] for mat in ok]
        sums[q][i][j] = value
        assert rule.sums_refusal(*sums) is not None
        with pytest.raises(mdk.MdkError, match="md_stats_center.*" + text):
            center_on_device(sums)
    two = [[list(r) for r in mat] for mat in ok]
    two[1][1][1], two[0][0][1] = -1, (1 << 30) + 1                  # two refused cells: the first is named
    with pytest.raises(mdk.MdkError, match=r"n is more than 2\^30 \(cell 0, 1\)"):
        center_on_device(two)
    sums = limit_matrices()[0]
    got = center_on_device(sums)
    assert not got[0].any() and not got[1].any()


def test_sum_of_two_parts_is_the_whole():
    import torch
    import methyldackel_amd as mdk
    S, n = 12, 4100
    m, u = table(S, n)
    names = [f"lib{i}" for i in range(S)]
    for min_depth, cut in ((1, 1), (5, 2049), (1, 4099)):
        want = expected(S, n, min_depth)
        a = mdk.sample_moments(device(m[:, :cut], "int32"), device(u[:, :cut], "int32"), min_depth, names=names)
        b = mdk.sample_moments(device(m[:, cut:], "int32"), device(u[:, cut:], "int32"), min_depth, names=names)
        both = a + b
        assert results(both) == want and both.names == tuple(names) and both.min_depth == min_depth
        assert results(a) != want
    other = mdk.sample_moments(device(m[:, :cut], "int32"), device(u[:, :cut], "int32"), 5, names=names)
    with pytest.raises(mdk.MdkError, match="same samples and min_depth"):
        a + other
    with pytest.raises(mdk.MdkError, match="same samples and min_depth"):
        a + mdk.sample_moments(device(m[:, :cut], "int32"), device(u[:, :cut], "int32"), 1)           # no names
    with pytest.raises(mdk.MdkError, match="same samples and min_depth"):
        a + mdk.sample_moments(device(m[:5, :cut], "int32"), device(u[:5, :cut], "int32"), 1)
    with pytest.raises(TypeError):
        a + 1
    full = mdk.SampleMoments(*[torch.full((2, 2), v, dtype=torch.int64, device="cuda") for v in (1 << 30, 1 << 46, 1 << 62, 1 << 62)], *[torch.zeros((2, 2), dtype=torch.float64, device="cuda")] * 2)
    one = mdk.SampleMoments(*[torch.full((2, 2), v, dtype=torch.int64, device="cuda") for v in (1, 3, 9, 9)], *[torch.zeros((2, 2), dtype=torch.float64, device="cuda")] * 2)
    with pytest.raises(mdk.MdkError, match=r"more than 2\^30"):
        full + one


@functools.lru_cache(maxsize=None)
def statistics_case(min_depth):
    import methyldackel_amd as mdk
    S, n = 17, 4100
    m, u = table(S, n)
    mo = mdk.sample_moments(device(m, "int32"), device(u, "int32"), min_depth)
    sums = [a.tolist() for a in rule.moments_np(m, u, min_depth)]
    assert results(mo)[:4] == tuple(sums)
    return mo, sums


@pytest.mark.parametrize("min_depth", [1, 5])
def test_mean_is_the_correctly_rounded_quotient(min_depth):
    mo, (N, SX, SXX, SXY) = statistics_case(min_depth)
    got = mo.mean().cpu().tolist()
    S = len(N)
    undefined = 0
    for i in range(S):
        for j in range(S):
            if N[i][j] == 0:
                assert math.isnan(got[i][j])
                undefined += 1
            else:
                assert rule.bits(got[i][j]) == rule.bits(SX[i][j] / N[i][j] / 65536.0), (i, j)         # (int / int is correctly rounded)
    assert 0 < undefined < S * S


@pytest.mark.parametrize("min_depth", [1, 5])
def test_correlation_and_covariance_within_their_bounds(min_depth):
    """correlation() within 8 * 2^-53 and covariance() within 4 * 2^-53 of exact arithmetic, in rationals and without a square root: with
    c = cxy, v = vxx[i][j] vxx[j][i] as exact integers, (r (1 -+ t))^2 v brackets c^2.  The bounds: one rounding each in cxy and the two
    vxx, then the product, the square root and the division -- 4.5 units for the correlation; cxy, the product n (n - 1) and the
    division -- 3 for the covariance"""
    mo, (N, SX, SXX, SXY) = statistics_case(min_depth)
    S = len(N)
    r_got, c_got, d_got = mo.correlation().cpu().tolist(), mo.covariance().cpu().tolist(), mo.distance().cpu().tolist()
    defined = undefined = 0
    worst_r = worst_c = Fraction(0)
    for i in range(S):
        for j in range(S):
            n = N[i][j]
            c = n * SXY[i][j] - SX[i][j] * SX[j][i]
            vi, vj = n * SXX[i][j] - SX[i][j] ** 2, n * SXX[j][i] - SX[j][i] ** 2
            if n < 2:
                assert math.isnan(c_got[i][j])
            else:
                exact = Fraction(c, n * (n - 1) << 32)
                err = abs(Fraction(c_got[i][j]) - exact)
                assert err <= 4 * U * abs(exact), (i, j)
                worst_c = max(worst_c, err / abs(exact) / U) if exact else worst_c
            if n < 2 or vi == 0 or vj == 0:
                assert math.isnan(r_got[i][j]) and math.isnan(d_got[i][j]), (i, j)
                undefined += 1
                continue
            defined += 1
            r = Fraction(r_got[i][j])
            assert -1 <= r <= 1 and d_got[i][j] == 1.0 - r_got[i][j]
            if i == j:
                assert r_got[i][j] == 1.0
                continue
            assert (r > 0) == (c > 0) and (r < 0) == (c < 0), (i, j)
            lo, hi = (abs(r) * (1 - 8 * U)) ** 2 * vi * vj, (abs(r) * (1 + 8 * U)) ** 2 * vi * vj
            if abs(r) == 1:                                         # clamped: the exact value may lie beyond
                hi = max(hi, Fraction(c * c))
            assert lo <= c * c <= hi, (i, j)
            if c:
                # |r| / rho - 1 in units of 2^-53, to first order half of r^2 v / c^2 - 1
                worst_r = max(worst_r, abs(r * r * vi * vj / (c * c) - 1) / 2 / U)
    print(f"min_depth {min_depth}: {defined} defined cells, {undefined} undefined; largest error: correlation {float(worst_r):.2f} u, covariance {float(worst_c):.2f} u")
    assert defined > S * S // 2 and undefined >= 2 * S - 1
    assert r_got[2][3] == 1.0 and r_got[3][2] == 1.0                # the two identical samples


def test_cohort_and_regions_carry_names_and_write(tmp_path):
    import torch
    import methyldackel_amd as mdk
    S, n = 12, 257
    m, u = table(S, n)
    names = tuple(f"lib{i}" for i in range(S))
    i = torch.arange(n, dtype=torch.int32)
    cols = {"contig": torch.zeros(n, dtype=torch.int32), "start": 10 * i, "end": 10 * i + 1, "context": torch.zeros(n, dtype=torch.uint8),
            "strand": torch.ones(n, dtype=torch.int8), "nsamples": torch.full((n,), S, dtype=torch.int32)}
    co = mdk.Cohort(["chr1"], {k: v.cuda() for k, v in cols.items()}, device(m, "int32"), device(u, "int32"), names=names)
    mo = co.moments(min_depth=5)
    assert results(mo) == expected(S, n, 5) and mo.names == names and mo.min_depth == 5
    assert results(mdk.Cohort(["chr1"], {k: v.cuda() for k, v in cols.items()}, device(m, "int32"), device(u, "int32")).moments()) == expected(S, n, 1)
    # per-interval sums are int64
    reg = mdk.CohortRegions(["chr1"], *[cols[k].cuda() for k in ("contig", "start", "end")], torch.ones((S, n), dtype=torch.int32, device="cuda"), device(m), device(u), names=names)
    rm = reg.moments()
    assert results(rm) == expected(S, n, 1) and rm.names == names
    big = device(m)
    big[3, 200] = 1 << 26
    with pytest.raises(mdk.MdkError, match=r"a count is 2\^26 or more \(site 200\)"):
        mdk.CohortRegions(["chr1"], *[cols[k].cuda() for k in ("contig", "start", "end")], torch.ones((S, n), dtype=torch.int32, device="cuda"), big, device(u)).moments()
    # the square tables
    for what, matrix in (("correlation", mo.correlation()), ("covariance", mo.covariance()), ("n", mo.n)):
        rows = mo.rows(what)
        assert [r[0] for r in rows] == list(names) and all(len(r) == S + 1 for r in rows)
        lines = open(mo.write(tmp_path / f"{what}.tsv", what)).read().split("\n")
        assert lines[0].split("\t") == ["#sample"] + list(names) and lines[-1] == "" and len(lines) == S + 2
        host = matrix.cpu().tolist()
        for s, line in enumerate(lines[1:-1]):
            cells = line.split("\t")
            assert cells[0] == names[s] and len(cells) == S + 1
            for text, v in zip(cells[1:], host[s]):
                if what == "n":
                    assert text == str(v)
                elif math.isnan(v):
                    assert text == "nan"
                else:
                    assert text == "%.17g" % v and float(text) == v
    assert [r[0] for r in mdk.sample_moments(device(m, "int32"), device(u, "int32")).rows("n")] == [f"s{i}" for i in range(S)]
    with pytest.raises(mdk.MdkError, match="unknown matrix"):
        mo.rows("spearman")
