"""GPU: kernel-weighted methylation levels on the device (k_smooth_window and k_smooth_sum of csrc/mdk_smooth.hip, libmdk_smooth.so) --
mdk.smooth_counts, mdk.smooth_limits, Cohort.smooth, Calls.smooth and their Smoothed.  Every comparison is exact, the integers equal and
the doubles as their 64-bit patterns: against the Python restatement of the rule (tests/smooth_rule.py), which tests/test_smooth_cpu.py
holds against the host build of the same header, against brute force and against exact rationals.  No Session and no BAM: the tables
are hand-made (tests/smooth_tables.py), and an expected result is computed once and shared."""
import re

import pytest

import smooth_rule as rule
from smooth_tables import PARAMS, expected, shared_table

pytestmark = pytest.mark.gpu
# both sides of a wavefront's 64 sites and of a tile's 256, several tiles, and a short last one
SIZES = (1, 63, 64, 65, 255, 256, 257, 513, 4100)
SAMPLES = (1, 3, 12)
KERNELS = ("tricube", "flat")
MESSAGES = {rule.E_ORDER: "not strictly ascending", rule.E_POSITION: "a contig or a start is negative", rule.E_NEGATIVE: "a count is negative",
            rule.E_ENTRY: "a count is 2^26 or more"}


def samples_of(n, k):
    """the S of combination k at size n: all three come up at every size; at 4100 the reference of 12 samples would take the longest, and 3
    stand in for them"""
    S = SAMPLES[(k + n) % 3]
    return 3 if n > 513 and S == 12 else S


def on_device(table, dtype):
    import torch
    contig, start, m, u = table
    return (torch.tensor(contig, dtype=torch.int32).cuda(), torch.tensor(start, dtype=torch.int32).cuda(),
            torch.tensor(m, dtype=dtype).reshape(len(m), len(start)).cuda(), torch.tensor(u, dtype=dtype).reshape(len(u), len(start)).cuda())


def same(got, want):
    """(level, depth, nsites, half) tensors against the rule's lists: the dtypes and shapes the stated ones, the integers equal, the doubles
    bit for bit"""
    import torch
    S, n = len(want[0]), len(want[2])
    for g, w in zip(got[:2], want[:2]):
        if g.dtype != torch.float64 or g.shape != (S, n) or not torch.equal(g.view(torch.int64).cpu(), torch.tensor(w, dtype=torch.int64).reshape(S, n)):
            return False
    for g, w in zip(got[2:], want[2:]):
        if g.dtype != torch.int32 or g.shape != (n,) or not torch.equal(g.cpu(), torch.tensor(w, dtype=torch.int32)):
            return False
    return True


# first in the file: the kernels' first execution
@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_parameters_and_kernels(n, params):
    """all four outputs for every size, every parameter pair and both kernels; S and the element width take turns so that every S and both
    widths meet every size; the inputs as they were after the call; a second run gives the same bits"""
    import torch
    import methyldackel_amd as mdk
    hb, ms = params
    for kn, kernel in enumerate(KERNELS):
        k = 2 * PARAMS.index(params) + kn
        S = samples_of(n, k)
        dtype = torch.int32 if (k // 3 + n) % 2 else torch.int64
        args = on_device(shared_table(n, S, n), dtype)
        before = [t.clone() for t in args]
        got = mdk.smooth_counts(*args, half_bases=hb, min_sites=ms, kernel=kernel)
        assert same(got, expected(n, S, n, hb, ms, rule.KERNELS[kernel])), (n, S, hb, ms, kernel, dtype)
        assert all(torch.equal(a, b) for a, b in zip(args, before))
        again = mdk.smooth_counts(*args, half_bases=hb, min_sites=ms, kernel=kernel)
        assert all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b) for a, b in zip(got, again))


def test_the_table_mixes_what_it_should():
    """the shared tables hold what the cases above are meant to meet: consecutive starts, gaps of thousands, one-site contigs, a contig
    change off every multiple of 64, uncovered entries, and levels without depth"""
    for n in (257, 4100):
        contig, start, m, u = shared_table(n, 3, n)
        steps = [b - a for a, b, c, d in zip(start, start[1:], contig, contig[1:]) if c == d]
        changes = [i for i in range(1, n) if contig[i] != contig[i - 1]]
        assert 1 in steps and max(steps) >= 1000 and any(i % 64 for i in changes) and any(i % 256 for i in changes)
        assert any(a + 1 == b for a, b in zip([0] + changes, changes + [n]))
        assert 0.05 < sum(1 for a, b in zip(m[0], u[0]) if a + b == 0) / n < 0.2
        assert rule.NAN_BITS in expected(n, 3, n, 50, 7, rule.TRICUBE)[0][2]


def test_limits_do_not_change_the_results():
    """tiles of 64 sites, chunks of 64 rows, batches of 2 samples and 3 workgroups: windows of 70 and of 200 sites and more are wider than
    a tile and span several chunks, S = 3 and S = 12 cross a batch boundary, every workgroup takes many items -- and the results are
    those under the defaults, which are the rule's"""
    import torch
    import methyldackel_amd as mdk
    try:
        mdk.smooth_limits(tile_sites=64, chunk_sites=64, sample_batch=2, max_workgroups=3)
        for n, S in ((4100, 3), (513, 12), (65, 3)):
            for hb, ms in ((500, 70), (3, 200), (0, 1)):
                for kernel in KERNELS:
                    k = 2 * PARAMS.index((hb, ms)) + KERNELS.index(kernel)
                    if samples_of(n, k) != S and n > 65:
                        continue                                # (the combinations whose expected results the sizes' test has made)
                    args = on_device(shared_table(n, S, n), torch.int32)
                    want = expected(n, S, n, hb, ms, rule.KERNELS[kernel])
                    assert (ms < 70 or max(want[2]) > 64) and same(mdk.smooth_counts(*args, half_bases=hb, min_sites=ms, kernel=kernel), want), (n, S, hb, ms, kernel)
        for bad in (dict(tile_sites=100), dict(tile_sites=512), dict(chunk_sites=8), dict(sample_batch=9), dict(chunk_sites=4096, sample_batch=8), dict(max_workgroups=-1)):
            with pytest.raises(mdk.MdkError, match="md_smooth_limits"):
                mdk.smooth_limits(**bad)
    finally:
        mdk.smooth_limits()
    args = on_device(shared_table(513, 12, 513), torch.int64)
    assert same(mdk.smooth_counts(*args, half_bases=500, min_sites=70), expected(513, 12, 513, 500, 70, rule.TRICUBE))


def cohort_of(table, names=None):
    import torch
    import methyldackel_amd as mdk
    contig, start, m, u = on_device(table, torch.int32)
    n = len(table[1])
    cols = {"contig": contig, "start": start, "end": start + 1, "context": torch.zeros(n, dtype=torch.uint8).cuda(), "strand": torch.ones(n, dtype=torch.int8).cuda(),
            "nsamples": torch.full((n,), len(table[2]), dtype=torch.int32).cuda()}
    return mdk.Cohort(names or ["c%d" % i for i in range(max(table[0]) + 1)], cols, m, u), cols


def test_cohort_and_calls_smooth():
    """Cohort.smooth and Calls.smooth on hand-built objects: the site columns come back as the same tensors, the parameters are kept, and
    select and rows() give what the tensors hold"""
    import torch
    import methyldackel_amd as mdk
    n, S = 257, 3
    table = shared_table(n, S, n)
    co, cols = cohort_of(table)
    sm = co.smooth(half_bases=50, min_sites=7)
    want = expected(n, S, n, 50, 7, rule.TRICUBE)
    assert isinstance(sm, mdk.Smoothed) and same((sm.level, sm.depth, sm.nsites, sm.half), want)
    assert all(getattr(sm, name) is t for name, t in cols.items()) and sm.contigs is co.contigs
    assert (sm.half_bases, sm.min_sites, sm.kernel, sm.n_samples, len(sm)) == (50, 7, "tricube", S, n)
    flat = co.smooth(half_bases=50, min_sites=7, kernel="flat")
    assert flat.kernel == "flat" and same((flat.level, flat.depth, flat.nsites, flat.half), expected(n, S, n, 50, 7, rule.FLAT))
    # the defaults are BSmooth's window
    dflt = co.smooth()
    assert (dflt.half_bases, dflt.min_sites, dflt.kernel) == (1000, 70, "tricube")
    assert same((dflt.level, dflt.depth, dflt.nsites, dflt.half), rule.smooth(*table, 1000, 70, rule.TRICUBE))
    # select: along the site axis, by a mask, an index tensor and a slice
    mask = sm.nsites > 8
    for index in (mask, torch.nonzero(mask).flatten(), slice(3, 200, 7)):
        part = sm.select(index)
        assert len(part) == int(part.level.shape[1]) == int(sm.start[index].shape[0]) and part.n_samples == S
        assert torch.equal(part.level.view(torch.int64), sm.level[:, index].view(torch.int64)) and torch.equal(part.depth, sm.depth[:, index])
        assert all(torch.equal(getattr(part, name), getattr(sm, name)[index]) for name in list(cols) + ["nsites", "half"])
        assert (part.half_bases, part.min_sites, part.kernel) == (50, 7, "tricube") and part.level.is_contiguous()
    rows = sm.select(slice(0, 5)).rows()
    contig, start = table[0], table[1]
    for i, row in enumerate(rows):
        assert row[:5] == ("c%d" % contig[i], start[i], start[i] + 1, want[2][i], want[3][i]) and len(row) == 5 + S
        for s in range(S):
            lv, dp = row[5 + s]
            assert rule.bits(dp) == want[1][s][i] and (rule.bits(lv) == want[0][s][i] or (lv != lv and want[0][s][i] == rule.NAN_BITS))
    # Calls.smooth: a sample of the cohort is a Calls over the same sites
    calls = co.sample(1)
    one = calls.smooth(half_bases=50, min_sites=7, kernel="flat")
    w = expected(n, S, n, 50, 7, rule.FLAT)
    assert one.n_samples == 1 and same((one.level, one.depth, one.nsites, one.half), ([w[0][1]], [w[1][1]], w[2], w[3]))
    assert one.start is calls.start and one.contig is calls.contig and one.end is calls.end and not hasattr(one, "nsamples")
    assert len(one.rows()) == n and len(one.rows()[0]) == 6


def test_refusals_name_the_first_site():
    """rows out of order, an equal start, a negative position, a negative count and a count of 2^26: MdkError with rc -3, the refusal in
    words and the first (smallest) refused site, under the defaults and under small tiles; the call after a refused one is as any other"""
    import torch
    import methyldackel_amd as mdk
    n, S = 513, 3
    contig, start, m, u = shared_table(n, S, n)
    inner = [i for i in range(1, n) if contig[i - 1] == contig[i]]
    a, b = inner[len(inner) // 2], inner[-1]

    def edited(**edits):
        c, x, mm, uu = list(contig), list(start), [list(r) for r in m], [list(r) for r in u]
        for what, (at, v) in edits.items():
            if what == "x":
                x[at] = v
            elif what == "c":
                c[at] = v
            elif what == "m":
                mm[at[0]][at[1]] = v
            else:
                uu[at[0]][at[1]] = v
        return c, x, mm, uu

    assert contig[n - 2] > 0
    cases = [edited(x=(a, start[a - 1])), edited(x=(a, start[a - 1] - 1)), edited(c=(n - 1, contig[n - 2] - 1)), edited(c=(0, -1)), edited(x=(0, -1)), edited(u=((2, 300), -1)), edited(m=((1, 256), 1 << 26)), edited(m=((0, 511), 1 << 26), u=((1, 77), -9)),
             edited(x=(b, start[b - 1]), m=((2, a), -1)), edited(x=(a, start[a - 1]), m=((2, b), 1 << 40))]
    try:
        for limits in (dict(), dict(tile_sites=64, chunk_sites=64, sample_batch=2, max_workgroups=5)):
            mdk.smooth_limits(**limits)
            for k, t in enumerate(cases):
                bit, site = rule.refusal(*t)
                dtype = torch.int64 if k % 2 or max(max(r) for r in t[2]) >= 1 << 31 else torch.int32
                with pytest.raises(mdk.MdkError, match=re.escape(MESSAGES[bit]) + rf".*\(site {site}\)") as e:
                    mdk.smooth_counts(*on_device(t, dtype), half_bases=50, min_sites=7, kernel=KERNELS[k % 2])
                assert e.value.rc == -3 and "md_smooth_run" in str(e.value)
    finally:
        mdk.smooth_limits()
    assert [rule.refusal(*t) for t in cases[:3]] == [(rule.E_ORDER, a)] * 2 + [(rule.E_ORDER, n - 1)] and rule.refusal(*cases[7]) == (rule.E_NEGATIVE, 77)
    assert rule.refusal(*cases[8]) == (rule.E_NEGATIVE, a) and rule.refusal(*cases[9]) == (rule.E_ORDER, a)
    # the largest entry that is accepted, and the call after refused ones
    t = edited(m=((1, 256), (1 << 26) - 1))
    assert same(mdk.smooth_counts(*on_device(t, torch.int32), half_bases=50, min_sites=7), rule.smooth(*t, 50, 7, rule.TRICUBE))


def test_argument_errors_and_the_empty_table():
    """parameters out of range, a CPU tensor, mismatched shapes, dtypes and an unknown kernel raise before the library is touched; n = 0
    returns empty tensors"""
    import torch
    import methyldackel_amd as mdk
    contig, start, m, u = on_device(shared_table(65, 3, 65), torch.int32)
    for kw, text in ((dict(half_bases=-1), "half_bases"), (dict(half_bases=(1 << 20) + 1), "half_bases"), (dict(half_bases=2.5), "half_bases"),
                     (dict(min_sites=0), "min_sites"), (dict(min_sites=(1 << 16) + 1), "min_sites"), (dict(min_sites=True), "min_sites"),
                     (dict(kernel="gauss"), "unknown kernel 'gauss'"), (dict(kernel=0), "unknown kernel")):
        with pytest.raises(mdk.MdkError, match=text):
            mdk.smooth_counts(contig, start, m, u, **kw)
    for args, text in (((contig.cpu(), start, m, u), "no CPU path"), ((contig, start, m.cpu(), u), "no CPU path"), ((contig, start[:-1], m, u), "sites"),
                       ((contig, start, m, u[:2]), "one dtype and one shape"), ((contig, start, m, u.long()), "one dtype and one shape"),
                       ((contig.long(), start, m, u), "int32"), ((contig, start, m[0], u[0]), r"\[samples, sites\]"), ((contig, start, m.t(), u.t()), "sites"),
                       ((contig, start, m[:, ::2], u[:, ::2]), "sites"), ((contig[::2], start[::2], m[:, ::2], u[:, ::2]), "contiguous"),
                       ((contig, start, m.double(), u.double()), "int32 or int64")):
        with pytest.raises(mdk.MdkError, match=text):
            mdk.smooth_counts(*args)
    with pytest.raises(mdk.MdkError, match="unknown kernel"):
        cohort_of(shared_table(65, 3, 65))[0].smooth(kernel="epanechnikov")
    # the ends of the ranges are inside them
    t = shared_table(65, 3, 65)
    assert same(mdk.smooth_counts(contig, start, m, u, half_bases=1 << 20, min_sites=1 << 16, kernel="flat"), rule.smooth(*t, 1 << 20, 1 << 16, rule.FLAT))
    # no site: empty tensors of the stated kinds, for a cohort too
    for S in (1, 3):
        empty = (torch.zeros(0, dtype=torch.int32).cuda(), torch.zeros(0, dtype=torch.int32).cuda(), torch.zeros((S, 0), dtype=torch.int64).cuda(), torch.zeros((S, 0), dtype=torch.int64).cuda())
        level, depth, nsites, half = mdk.smooth_counts(*empty)
        assert level.shape == depth.shape == (S, 0) and nsites.shape == half.shape == (0,) and level.is_cuda
        assert (level.dtype, depth.dtype, nsites.dtype, half.dtype) == (torch.float64, torch.float64, torch.int32, torch.int32)
