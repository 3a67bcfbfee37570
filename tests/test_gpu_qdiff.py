"""GPU: two groups of replicate samples compared site by site on the device (k_qdiff of csrc/mdk_qdiff.hip, libmdk_stats.so) --
mdk.diff_replicates, Cohort.diff_replicates and its ReplicateDiff.  Every comparison is exact, the integers equal and the doubles as
their 64-bit patterns: against the Python restatement of the rule (tests/qdiff_rule.py), which tests/test_qdiff_cpu.py holds against the
host build of the same header, against exact rationals and against mpmath.  No Session and no BAM: the cohorts are hand-made."""
import random
import re

import pytest

from diff_rule import LIMIT, MESSAGES, bh, bits
from qdiff_rule import ACCEPTED, HAND, NAMES, REFUSED, null_sites, seeded, site

pytestmark = pytest.mark.gpu
DTYPES = ("int64", "int64", "int64", "int64", "float64", "float64", "int32", "float64", "float64")
# both sides of a wavefront's 64 sites and of a workgroup's 256, several workgroups, and a short last one
SIZES = (1, 63, 64, 65, 255, 256, 257, 513, 4100)
# S of 3, 4, 5, 7 and 12; the groups unsorted; samples 2 (of 5) and 8 (of 12) in neither
CASES = [(3, [0], [1, 2]), (3, [2, 0], [1]), (4, [3, 1], [2, 0]), (5, [4, 0], [3, 1]), (7, [5, 0, 3], [6, 1]), (7, [2], [4, 6, 0, 1]),
         (12, [11, 3, 7, 0, 5], [2, 9, 1, 10, 6, 4])]


def matrices(n, S, seed, uncovered=0.1, shifted=()):
    """two lists of S rows of n counts: depths 1 to 40 around a fraction per site, every second site with a shift in the samples
    `shifted`, a tenth of the entries without coverage; now and then a site all methylated or all unmethylated"""
    rng = random.Random(seed)
    m, u = [[0] * n for _ in range(S)], [[0] * n for _ in range(S)]
    for i in range(n):
        f = rng.choice((0.0, 1.0)) if rng.random() < 0.05 else rng.uniform(0.1, 0.9)
        shift = rng.uniform(-0.5, 0.5) if i & 1 and 0.0 < f < 1.0 else 0.0
        for s in range(S):
            if rng.random() < uncovered:
                continue
            depth = rng.randint(1, 40)
            g = f + (shift if s in shifted else 0.0) + (rng.uniform(-0.06, 0.06) if 0.0 < f < 1.0 else 0.0)
            k = int(round(depth * min(1.0, max(0.0, g))))
            m[s][i], u[s][i] = k, depth - k
    return m, u


def expected(m, u, ga, gb, floor=1.0):
    """what mdk.diff_replicates gives for count matrices (lists of rows) and two lists of sample indices: nine lists in NAMES' order and
    the term counts.  The groups are visited ascending, however they were given"""
    ga, gb = sorted(ga), sorted(gb)
    cols, steps = [[] for _ in NAMES], []
    for i in range(len(m[0])):
        row, st = site([m[s][i] for s in ga], [u[s][i] for s in ga], [m[s][i] for s in gb], [u[s][i] for s in gb], floor)
        for c, v in zip(cols, row):
            c.append(v)
        steps.append(st)
    return cols, steps


def columns(sites, floor=1.0):
    """the same for a list of sites (ma, ua, mb, ub) of one shape: the matrices' rows (A's samples, then B's), the nine lists, the steps"""
    m = [list(r) for r in zip(*[s[0] + s[2] for s in sites])]
    u = [list(r) for r in zip(*[s[1] + s[3] for s in sites])]
    na = len(sites[0][0])
    return m, u, list(range(na)), list(range(na, len(m))), expected(m, u, range(na), range(na, len(m)), floor)


def on_device(rows, dtype):
    import torch
    return torch.tensor(rows, dtype=dtype).cuda()


def same(got, want):
    """nine tensors against nine lists: the dtypes the stated ones, the integers equal, the doubles bit for bit"""
    import torch
    for name, dt, g, w in zip(NAMES, DTYPES, got, want):
        if g.dtype != getattr(torch, dt) or g.shape != (len(w),):
            return False
        if dt == "float64":
            if not torch.equal(g.view(torch.int64).cpu(), torch.tensor([bits(x) for x in w], dtype=torch.int64)):
                return False
        elif not torch.equal(g.cpu(), torch.tensor(w, dtype=g.dtype)):
            return False
    return True


# first in the file: the kernel's first execution
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_dtypes(n):
    """all nine outputs and the term counts for every size and every S, unused samples, the groups unsorted, both element widths; the
    inputs as they were after the call"""
    import torch
    import methyldackel_amd as mdk
    for k, (S, ga, gb) in enumerate(CASES if n <= 513 else CASES[4:7:2]):
        m, u = matrices(n, S, seed=1000 * n + k, shifted=gb)
        want, steps = expected(m, u, ga, gb)
        for dtype in (torch.int32, torch.int64):
            dm, du = on_device(m, dtype), on_device(u, dtype)
            keep = dm.clone(), du.clone()
            got = mdk.diff_replicates(dm, du, ga, gb, steps=True)
            assert len(got) == 10 and same(got[:9], want), (n, S, ga, gb, dtype)
            assert got[9].dtype == torch.uint32 and got[9].cpu().tolist() == steps
            assert torch.equal(dm, keep[0]) and torch.equal(du, keep[1])
            for t in got:
                assert t.shape == (n,) and t.device == dm.device and t.is_contiguous()
            again = mdk.diff_replicates(dm, du, sorted(ga), sorted(gb))
            assert len(again) == 9 and all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)
                                           for x, y in zip(again, got))
        if n >= 255:
            uncovered = sum(1 for s in ga + gb for i in range(n) if m[s][i] + u[s][i] == 0) / (n * len(ga + gb))
            assert 0.05 < uncovered < 0.16 and max(steps) > 5
            if S >= 7:
                assert 0 < sum(1 for p in want[5] if p == 1.0) < n and any(p < 0.05 for p in want[5])


@pytest.mark.parametrize("floor", [1.0, 0.25])
def test_the_rule_s_own_sites_on_the_device(floor):
    """qdiff_rule.seeded(), HAND and ACCEPTED, a call per shape (samples of A, samples of B); at the default floor what is known by
    hand of HAND"""
    import torch
    import methyldackel_amd as mdk
    named = [(None, s, None) for s in seeded()] + list(HAND) + [(None, s, None) for s in ACCEPTED]
    shapes = {}
    for entry in named:
        shapes.setdefault((len(entry[1][0]), len(entry[1][2])), []).append(entry)
    assert len(named) > 2000 and {sum(k) for k in shapes} >= {3, 4, 5, 7, 12, 120}
    for k, (shape, entries) in enumerate(sorted(shapes.items())):
        m, u, ga, gb, (want, steps) = columns([e[1] for e in entries], floor)
        dtype = (torch.int32, torch.int64)[k & 1]
        got = mdk.diff_replicates(on_device(m, dtype), on_device(u, dtype), ga, gb, min_dispersion=floor, steps=True)
        assert same(got[:9], want), (shape, floor)
        assert got[9].cpu().tolist() == steps
        host = [t.cpu().tolist() for t in got[:9]]
        for i, (name, _, known) in enumerate(entries):
            for col, v in (known or {} if floor == 1.0 else {}).items():             # (what is known by hand is known at the default floor)
                assert host[NAMES.index(col)][i] == v, (name, col)


def wide(S, count, seed):
    """sites of S samples, all covered, half of them a group (as tests/test_qdiff_cpu.py makes them)"""
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


@pytest.mark.parametrize("S,count", [(66, 12), (1024, 2)])
def test_wide_groups(S, count):
    """66 samples, and the most the call takes: 1,024 samples, nu = 1022, the order's buffer full"""
    import torch
    import methyldackel_amd as mdk
    m, u, ga, gb, (want, steps) = columns(wide(S, count, S))
    assert want[6] == [S - 2] * count
    got = mdk.diff_replicates(on_device(m, torch.int32), on_device(u, torch.int32), ga[::-1], gb[::-1], steps=True)
    assert same(got[:9], want) and got[9].cpu().tolist() == steps
    got = mdk.diff_replicates(on_device(m, torch.int64), on_device(u, torch.int64), ga, gb, min_dispersion=0.25)
    assert same(got, columns(wide(S, count, S), 0.25)[4][0])


def long_site():
    """24 samples, twelve a group, F just above 3 nu / (nu + 2), where the tail's series is longest"""
    rng = random.Random(629)
    fa = rng.uniform(0.3, 0.7); fb = fa + rng.choice((-1, 1)) * rng.uniform(0.05, 0.12)
    m, u = [], []
    for s in range(24):
        n = rng.randint(15, 40)
        f = (fa if s < 12 else fb) + rng.uniform(-0.1, 0.1)
        k = sum(1 for _ in range(n) if rng.random() < f)
        m.append(k); u.append(n - k)
    return m, u


@pytest.mark.parametrize("at", [0, 63, 64, 300])
def test_a_long_series_does_not_disturb_its_neighbours(at):
    """513 sites of three samples against three -- the other eighteen rows without coverage there -- and one site of all 24 with some
    hundreds of terms, wherever it stands in its wavefront"""
    import torch
    import methyldackel_amd as mdk
    ga, gb = list(range(12)), list(range(12, 24))
    few = [0, 1, 2, 12, 13, 14]
    sm, su = matrices(514, 6, seed=77, uncovered=0.0, shifted=(3, 4, 5))
    m, u = [[0] * 514 for _ in range(24)], [[0] * 514 for _ in range(24)]
    for r, s in enumerate(few):
        m[s], u[s] = sm[r], su[r]
    lm, lu = long_site()
    for s in range(24):
        m[s][at], u[s][at] = lm[s], lu[s]
    want, steps = expected(m, u, ga, gb)
    assert steps[at] > 200 and want[6][at] == 22 and 2.5 < want[8][at] < 3.5
    assert 2 * max(st for i, st in enumerate(steps) if i != at) < steps[at]
    got = mdk.diff_replicates(on_device(m, torch.int32), on_device(u, torch.int32), ga, gb, steps=True)
    assert same(got[:9], want) and got[9].cpu().tolist() == steps
    # the neighbours' bits are those of the call without the long site
    for s in range(24):
        m[s][at], u[s][at] = (sm[few.index(s)][at], su[few.index(s)][at]) if s in few else (0, 0)
    plain = mdk.diff_replicates(on_device(m, torch.int32), on_device(u, torch.int32), ga, gb)
    keep = torch.arange(514, device="cuda") != at
    for x, y in zip(plain, got[:9]):
        assert torch.equal(x[keep].view(torch.int64) if x.dtype == torch.float64 else x[keep], y[keep].view(torch.int64) if y.dtype == torch.float64 else y[keep])


def refused_matrices(placed):
    """513 accepted sites of two samples against two, and the given sites at the given places"""
    m, u = matrices(513, 4, seed=5)
    for at, (ma, ua, mb, ub) in placed:
        for s, (mm, uu) in enumerate(zip(ma + mb, ua + ub)):
            m[s][at], u[s][at] = mm, uu
    return m, u


@pytest.mark.parametrize("name,t,bit", REFUSED, ids=[f"{r[0]}{i}" for i, r in enumerate(REFUSED)])
def test_refusals_name_the_first_site(name, t, bit):
    """each refused condition among accepted sites, at site 300 and again behind it: rc -3, diff_counts's words, the first such site"""
    import torch
    import methyldackel_amd as mdk
    m, u = refused_matrices([(300, t), (301, t), (512, t)])
    for dtype in (torch.int32, torch.int64):
        with pytest.raises(mdk.MdkError, match=re.escape(MESSAGES[bit]) + r".*\(site 300\)") as e:
            mdk.diff_replicates(on_device(m, dtype), on_device(u, dtype), [1, 0], [3, 2])
        assert e.value.rc == -3 and "md_stats_qdiff" in str(e.value)
    # the call after a refused one is as any other
    m, u = matrices(257, 4, seed=6)
    assert same(mdk.diff_replicates(on_device(m, torch.int32), on_device(u, torch.int32), [0, 1], [2, 3]), expected(m, u, [0, 1], [2, 3])[0])


def test_of_two_refused_sites_the_smaller_index_is_named():
    """in whatever workgroup they stand, and whichever of them has the lower bit"""
    import torch
    import methyldackel_amd as mdk
    negative, entry, margin = REFUSED[0][1], REFUSED[2][1], REFUSED[4][1]
    for (lo, first), (hi, second), text in (((40, margin), (300, negative), MESSAGES[4]), ((299, negative), (300, entry), MESSAGES[1]),
                                            ((7, entry), (8, negative), MESSAGES[2]), ((0, margin), (512, margin), MESSAGES[4])):
        m, u = refused_matrices([(hi, second), (lo, first)])
        with pytest.raises(mdk.MdkError, match=re.escape(text) + rf".*\(site {lo}\)"):
            mdk.diff_replicates(on_device(m, torch.int32), on_device(u, torch.int32), [0, 1], [2, 3])
    # a margin pooled over samples whose entries are all accepted, and a sample that is not used is not read
    half = LIMIT // 2
    m, u = [[1, half], [2, half], [3, 5], [2, 2]], [[1, 0], [1, 0], [1, 1], [3, 1]]
    with pytest.raises(mdk.MdkError, match=r"pooled margin.*\(site 1\)"):
        mdk.diff_replicates(on_device(m, torch.int32), on_device(u, torch.int32), [0, 1], [2, 3])
    m[1][0] = -5
    assert same(mdk.diff_replicates(on_device(m, torch.int32), on_device(u, torch.int32), [0], [2, 3]), expected(m, u, [0], [2, 3])[0])


def test_arguments_refused_before_the_library_is_touched():
    import torch
    import methyldackel_amd as mdk
    m, u = matrices(6, 4, seed=9)
    dm, du = on_device(m, torch.int32), on_device(u, torch.int32)
    cases = [((dm.cpu(), du.cpu(), [0, 1], [2, 3]), {}, "no CPU path"), ((dm, du.cpu(), [0, 1], [2, 3]), {}, "no CPU path"),
             ((dm[:, ::2], du[:, ::2].contiguous(), [0], [1]), {}, "nmeth must be contiguous"), ((dm[::2], du[::2].t().contiguous().t(), [0], [1]), {}, "must be contiguous"),
             ((dm, du.to(torch.int64), [0], [1]), {}, "one dtype and one shape"), ((dm, du, [], [1]), {}, "group a is empty"), ((dm, du, [0], []), {}, "group b is empty"),
             ((dm, du, [0, 1], [1, 2]), {}, "sample 1 is in both groups"), ((dm, du, [0], [4]), {}, "names sample 4"), ((dm, du, [-1], [2]), {}, "names sample -1")]
    cases += [((dm, du, [0, 1], [2, 3]), {"min_dispersion": v}, "min_dispersion") for v in (float("nan"), 0.0, 2.0 ** -56, 2.0 ** 801)]
    calls = []
    real = mdk.lib_stats
    mdk.lib_stats = lambda: calls.append(1) or real()
    try:
        for args, kw, text in cases:
            with pytest.raises(mdk.MdkError, match=re.escape(text)):
                mdk.diff_replicates(*args, **kw)
        assert not calls
        # the ends of the floor's range are inside it
        for floor in (2.0 ** -55, 2.0 ** 800):
            assert same(mdk.diff_replicates(dm, du, [0, 1], [2, 3], min_dispersion=floor), expected(m, u, [0, 1], [2, 3], floor)[0])
        assert len(calls) == 2
    finally:
        mdk.lib_stats = real


def cohort():
    """three samples over one universe of sites, united: hand-made Calls, no BAM"""
    import torch
    import methyldackel_amd as mdk
    from merge_rule import COLUMNS
    from unite_rule import CONTIGS, sample
    samples = [mdk.Calls(list(CONTIGS), {n: torch.from_numpy(c.copy()).cuda() for n, c in zip(COLUMNS, sample(513, s))}) for s in range(3)]
    return mdk.unite(samples, min_samples=2), mdk


def test_cohort_diff_replicates(tmp_path):
    import torch
    co, mdk = cohort()
    assert len(co) > 100
    d = co.diff_replicates([0], [2, 1])
    assert type(d) is mdk.ReplicateDiff and isinstance(d, mdk.Diff) and len(d) == len(co) and d.contigs == co.contigs and d.merged == co.merged
    for name in ("contig", "start", "end", "context", "strand"):
        assert getattr(d, name) is getattr(co, name), name
    want, _ = expected(co.nmeth.cpu().tolist(), co.nunmeth.cpu().tolist(), [0], [1, 2])
    assert same([getattr(d, n) for n in NAMES], want)
    direct = mdk.diff_replicates(co.nmeth, co.nunmeth, [0], [1, 2])
    assert same(direct, want)
    assert 0 < sum(1 for p in want[5] if p < 1.0) and set(want[6]) == {0, 1}
    # rows, select, write and the file read back
    rows = d.rows()
    assert len(rows[0]) == 14 and [r[5:] for r in rows] == list(zip(*want)) and rows[0][0] == co.contigs[int(co.contig[0])]
    mask = d.pvalue < 0.5
    s = d.select(mask)
    assert type(s) is mdk.ReplicateDiff and 0 < len(s) < len(d) and s.rows() == [r for r, k in zip(rows, mask.cpu().tolist()) if k] and s.merged == d.merged
    path = d.write(str(tmp_path / "qdiff.tsv"))
    back = [l.rstrip("\n").split("\t") for l in open(path)]
    assert all(len(r) == 14 for r in back)
    assert [tuple([r[0]] + [int(x) for x in r[1:9]] + [bits(float(r[9])), bits(float(r[10])), int(r[11]), bits(float(r[12])), bits(float(r[13]))]) for r in back] == \
           [r[:9] + (bits(r[9]), bits(r[10]), r[11], bits(r[12]), bits(r[13])) for r in rows]
    # qvalue: Benjamini and Hochberg of the F test's p-values
    q = d.qvalue()
    assert q.dtype == torch.float64 and q.device == d.pvalue.device and [bits(x) for x in q.cpu().tolist()] == [bits(x) for x in bh(want[5])]
    # the pooled counts and meth_diff are Cohort.diff's
    f = co.diff([0], [2, 1])
    for name in NAMES[:5]:
        assert torch.equal(getattr(f, name).view(torch.int64), getattr(d, name).view(torch.int64)), name
    with pytest.raises(mdk.MdkError, match="both groups"):
        co.diff_replicates([0, 1], [1])


def test_dmrs_are_the_pooled_counts_own_and_a_region_has_its_replicate_test():
    """the same joining on the same counts as Cohort.diff's, in every column; then the docstring's replicate test of the regions"""
    import torch
    import methyldackel_amd as mdk
    from merge_rule import COLUMNS
    starts = list(range(100, 100 + 4 * 40, 4))
    def calls(fraction, depth):
        n = len(starts)
        m = [round(depth * fraction(i)) for i in range(n)]
        cols = {"contig": [0] * n, "start": starts, "end": [s + 2 for s in starts], "nmeth": m, "nunmeth": [depth - x for x in m], "context": [0] * n, "strand": [0] * n}
        types = dict(mdk.CALL_COLUMNS)
        return mdk.Calls(["chr1", "chrM"], {k: torch.tensor(cols[k], dtype=getattr(torch, types[k])).cuda() for k in COLUMNS}, merged=True)
    hyper = lambda i: 0.9 if 5 <= i < 15 else 0.1 if 25 <= i < 32 else 0.5          # group b: up over sites 5 .. 14, down over 25 .. 31
    co = mdk.unite([calls(lambda i: 0.5, 30), calls(lambda i: 0.45, 20), calls(hyper, 40), calls(hyper, 25)])
    a, b = [1, 0], [3, 2]
    d, f = co.diff_replicates(a, b), co.diff(a, b)
    mask = f.qvalue() < 0.05
    params = dict(max_gap=8, max_skip=1, min_sites=3, min_diff=20.0)
    ours, theirs = d.dmrs(mask, **params), f.dmrs(mask, **params)
    assert type(ours) is mdk.Dmrs and ours.direction.cpu().tolist() == [1, -1] and ours.merged and ours.rows() == theirs.rows()
    for name, dt in mdk.DMR_COLUMNS:
        x, y = getattr(ours, name), getattr(theirs, name)
        assert x.dtype == getattr(torch, dt) and torch.equal(x.view(torch.int64) if dt == "float64" else x, y.view(torch.int64) if dt == "float64" else y), name
    per = [co.sample(i).regions(ours.intervals()) for i in range(co.n_samples)]
    m, u = torch.stack([p.nmeth for p in per]), torch.stack([p.nunmeth for p in per])
    assert m.dtype == torch.int64 and m.shape == (4, 2)
    test = mdk.diff_replicates(m, u, a, b)
    assert same(test, expected(m.cpu().tolist(), u.cpu().tolist(), a, b)[0])
    assert torch.equal(test[0], ours.nmeth_a) and torch.equal(test[3], ours.nunmeth_b) and test[6].cpu().tolist() == [2, 2]


def test_cohort_without_sites_and_with_one_sample_a_group():
    import torch
    co, mdk = cohort()
    empty = co.select(slice(0, 0)).diff_replicates([0, 1], [2])
    assert type(empty) is mdk.ReplicateDiff and len(empty) == 0 and empty.rows() == [] and len(empty.qvalue()) == 0
    for (name, dt), t in zip(mdk.ReplicateDiff.COLUMNS, (getattr(empty, n) for n, _ in mdk.ReplicateDiff.COLUMNS)):
        assert t.shape == (0,) and t.dtype == getattr(torch, dt) and t.device.type == "cuda", name
    assert len(empty.dmrs(torch.zeros(0, dtype=torch.bool, device="cuda"))) == 0
    assert all(t.shape == (0,) for t in mdk.diff_replicates(co.nmeth[:, :0].contiguous(), co.nunmeth[:, :0].contiguous(), [0], [1, 2], steps=True))
    # one sample a group: nothing to estimate a dispersion from
    d = co.diff_replicates([2], [0])
    assert torch.all(d.pvalue == 1.0) and torch.all(d.df == 0) and torch.all(d.dispersion == 1.0) and torch.all(d.statistic == 0.0)
    f = co.diff([2], [0])
    assert torch.equal(d.nmeth_a, f.nmeth_a) and torch.equal(d.nunmeth_b, f.nunmeth_b) and torch.equal(d.meth_diff.view(torch.int64), f.meth_diff.view(torch.int64))
    assert bool((f.pvalue < 1.0).any())


def test_calibration_on_the_device():
    """4,000 sites without a difference, three over-dispersed replicates against three (rho = 0.2): the F test rejects about one in
    twenty at 0.05 -- the CPU test's band, the rule gives 4.50 % --, Fisher's test of the pooled tables more than one in four"""
    import torch
    import methyldackel_amd as mdk
    sites = null_sites()
    assert len(sites) == 4000
    m, u, ga, gb, (want, steps) = columns(sites)
    n = len(sites)
    cols = {"contig": torch.zeros(n, dtype=torch.int32), "start": torch.arange(n, dtype=torch.int32) * 100, "end": torch.arange(n, dtype=torch.int32) * 100 + 1,
            "context": torch.zeros(n, dtype=torch.uint8), "strand": torch.ones(n, dtype=torch.int8), "nsamples": torch.full((n,), 6, dtype=torch.int32)}
    co = mdk.Cohort(["chr1"], {k: v.cuda() for k, v in cols.items()}, on_device(m, torch.int32), on_device(u, torch.int32))
    d = co.diff_replicates(ga, gb)
    assert same([getattr(d, name) for name in NAMES], want)
    rate = float((d.pvalue < 0.05).sum()) / n
    pooled = float((co.diff(ga, gb).pvalue < 0.05).sum()) / n
    print(f"rejected at 0.05: F test {rate:.4f}, pooled Fisher {pooled:.4f}")
    assert 0.02 <= rate <= 0.08
    assert pooled > 0.25
