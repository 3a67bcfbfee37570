"""GPU: three or more groups of replicate samples compared site by site on the device (k_gdiff of csrc/mdk_gdiff.hip, libmdk_stats.so) --
mdk.diff_groups, Cohort.diff_groups and its GroupDiff.  Every comparison is exact, the integers equal and the doubles as their 64-bit
patterns: against the Python restatement of the rule (tests/gdiff_rule.py), which tests/test_gdiff_cpu.py holds against the host build of
the same header, against exact rationals and against mpmath; and, for two groups, against mdk.diff_replicates on the same matrices.  No
Session and no BAM: the cohorts are hand-made."""
import random
import re

import pytest

import qdiff_rule
from diff_rule import LIMIT, MESSAGES, bh, bits
from gdiff_rule import ACCEPTED, HAND, NAMES, REFUSED, null_sites, seeded, site, two

pytestmark = pytest.mark.gpu
DTYPES = ("float64", "int32", "int32", "float64", "int32", "int32", "float64", "float64")
# both sides of a wavefront's 64 sites and of a workgroup's 256, several workgroups, and a short last one
SIZES = (1, 63, 64, 65, 255, 256, 257, 513, 4100)
# S of 3 to 12; the groups unsorted; samples 2 (of 5), 3 and 8 (of 12) in none
CASES = [(3, [[0], [1], [2]]), (4, [[3, 1], [2, 0]]), (5, [[4, 0], [3], [1]]), (7, [[5, 0, 3], [6, 1], [4, 2]]), (9, [[2, 0, 1], [5, 4, 3], [8, 6, 7]]),
         (12, [[11, 7, 0], [2, 9, 1, 10], [6, 4], [5]])]


def matrices(n, S, seed, uncovered=0.1, groups=()):
    """two lists of S rows of n counts: depths 1 to 40 around a fraction per site, every second site with a shift of its own in every
    group of `groups` but the first, a tenth of the entries without coverage; now and then a site all methylated or all unmethylated,
    now and then a group without coverage at a site"""
    rng = random.Random(seed)
    m, u = [[0] * n for _ in range(S)], [[0] * n for _ in range(S)]
    of = {s: g for g, group in enumerate(groups) for s in group}
    for i in range(n):
        f = rng.choice((0.0, 1.0)) if rng.random() < 0.05 else rng.uniform(0.1, 0.9)
        shift = [0.0] + [rng.uniform(-0.5, 0.5) if i & 1 and 0.0 < f < 1.0 else 0.0 for _ in groups[1:]]
        gone = rng.randrange(len(groups)) if groups and rng.random() < 0.06 else -1
        for s in range(S):
            if rng.random() < uncovered or of.get(s, -2) == gone:
                continue
            depth = rng.randint(1, 40)
            g = f + shift[of.get(s, 0)] + (rng.uniform(-0.06, 0.06) if 0.0 < f < 1.0 else 0.0)
            k = int(round(depth * min(1.0, max(0.0, g))))
            m[s][i], u[s][i] = k, depth - k
    return m, u


def expected(m, u, groups, floor=1.0):
    """what mdk.diff_groups gives for count matrices (lists of rows) and lists of sample indices: the two [G, n] matrices as lists of
    rows, eight lists in NAMES' order and the term counts.  A group is visited ascending, however it was given"""
    groups = [sorted(g) for g in groups]
    gm, gu = [[] for _ in groups], [[] for _ in groups]
    cols, steps = [[] for _ in NAMES], []
    for i in range(len(m[0])):
        a, b, row, st = site([([m[s][i] for s in g], [u[s][i] for s in g]) for g in groups], floor)
        for g in range(len(groups)):
            gm[g].append(a[g]); gu[g].append(b[g])
        for c, v in zip(cols, row):
            c.append(v)
        steps.append(st)
    return gm, gu, cols, steps


def columns(sites, floor=1.0):
    """the same for a list of sites of one shape (the groups' sizes): the matrices' rows (group 0's samples, then group 1's, ...), the
    groups, and what is expected"""
    m = [list(r) for r in zip(*[[v for ms, _ in s for v in ms] for s in sites])]
    u = [list(r) for r in zip(*[[v for _, us in s for v in us] for s in sites])]
    groups, at = [], 0
    for ms, _ in sites[0]:
        groups.append(list(range(at, at + len(ms))))
        at += len(ms)
    return m, u, groups, expected(m, u, groups, floor)


def on_device(rows, dtype):
    import torch
    return torch.tensor(rows, dtype=dtype).cuda()


def equal_bits(x, y):
    import torch
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)


def same(got, want):
    """the ten tensors of a call against (gm, gu, the eight lists): the dtypes the stated ones, the integers equal, the doubles bit for bit"""
    import torch
    gm, gu, cols = want[:3]
    for g, w in ((got[0], gm), (got[1], gu)):
        if g.dtype != torch.int64 or g.shape != (len(w), len(w[0])) or not g.is_contiguous() or not torch.equal(g.cpu(), torch.tensor(w, dtype=torch.int64).reshape(g.shape)):
            return False
    for name, dt, g, w in zip(NAMES, DTYPES, got[2:10], cols):
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
    """all ten outputs and the term counts for every size and every S, unused samples, the groups unsorted, both element widths; the
    inputs as they were after the call; sorted groups give the same bits"""
    import torch
    import methyldackel_amd as mdk
    for k, (S, groups) in enumerate(CASES if n <= 513 else CASES[3::2]):
        m, u = matrices(n, S, seed=1000 * n + k, groups=groups)
        want = expected(m, u, groups)
        for dtype in (torch.int32, torch.int64):
            dm, du = on_device(m, dtype), on_device(u, dtype)
            keep = dm.clone(), du.clone()
            got = mdk.diff_groups(dm, du, groups, steps=True)
            assert len(got) == 11 and same(got, want), (n, S, groups, dtype)
            assert got[10].dtype == torch.uint32 and got[10].cpu().tolist() == want[3]
            assert torch.equal(dm, keep[0]) and torch.equal(du, keep[1])
            for t in got:
                assert t.shape[-1] == n and t.device == dm.device and t.is_contiguous()
            again = mdk.diff_groups(dm, du, [sorted(g) for g in groups])
            assert len(again) == 10 and all(equal_bits(x, y) for x, y in zip(again, got))
        if n >= 255 and S >= 4:                                                   # (S = 3: one sample a group, nothing to test anywhere)
            cols, steps = want[2], want[3]
            assert max(steps) > 5 and any(d > 0.0 for d in cols[0]) and min(cols[0]) >= 0.0
            if len(groups) >= 3 and S >= 7:
                assert 0 < sum(1 for p in cols[3] if p == 1.0) < n and any(p < 0.05 for p in cols[3])
                assert len(set(cols[5])) > 1                                          # a group without coverage here and there


@pytest.mark.parametrize("floor", [1.0, 0.25])
def test_the_rule_s_own_sites_on_the_device(floor):
    """gdiff_rule.seeded(), HAND and ACCEPTED, a call per shape (the groups' sizes); at the default floor what is known by hand of HAND"""
    import torch
    import methyldackel_amd as mdk
    named = [(None, s, None) for s in seeded()] + list(HAND) + [(None, s, None) for s in ACCEPTED]
    shapes = {}
    for entry in named:
        shapes.setdefault(tuple(len(ms) for ms, _ in entry[1]), []).append(entry)
    assert len(named) > 900 and {len(k) for k in shapes} >= {2, 3, 4, 5, 8, 17}
    # (few sites share a shape: the calls are many and small, so every eighth shape of the seeded ones runs at the second floor)
    for k, (shape, entries) in enumerate(sorted(shapes.items())):
        if floor != 1.0 and k % 8:
            continue
        m, u, groups, want = columns([e[1] for e in entries], floor)
        dtype = (torch.int32, torch.int64)[k & 1]
        got = mdk.diff_groups(on_device(m, dtype), on_device(u, dtype), groups, min_dispersion=floor, steps=True)
        assert same(got, want), (shape, floor)
        assert got[10].cpu().tolist() == want[3]
        host = [t.cpu().tolist() for t in got[2:10]]
        for i, (name, _, known) in enumerate(entries):
            for col, v in (known or {} if floor == 1.0 else {}).items():             # (what is known by hand is known at the default floor)
                assert host[NAMES.index(col)][i] == v, (name, col)


def test_two_groups_are_diff_replicates_bit_for_bit():
    """every output of a call with two groups against mdk.diff_replicates on the same matrices: the pooled rows are its four count
    columns, pvalue, df, dispersion, statistic and steps its own, meth_diff its absolute value; also qdiff_rule's own sites"""
    import torch
    import methyldackel_amd as mdk
    runs = []
    for k, (S, ga, gb) in enumerate([(3, [0], [1, 2]), (4, [3, 1], [2, 0]), (7, [5, 0, 3], [6, 1]), (12, [11, 3, 7, 0, 5], [2, 9, 1, 10, 6, 4])]):
        m, u = matrices(513, S, seed=40 + k, groups=[ga, gb])
        runs.append((m, u, ga, gb))
    theirs = qdiff_rule.seeded(per_shape=120) + [h[1] for h in qdiff_rule.HAND] + qdiff_rule.ACCEPTED
    shapes = {}
    for s in theirs:
        shapes.setdefault((len(s[0]), len(s[2])), []).append(s)
    for (na, nb), group in sorted(shapes.items()):
        m, u, groups, _ = columns([two(s) for s in group])
        runs.append((m, u, groups[0], groups[1]))
    assert len(runs) > 20
    for k, (m, u, ga, gb) in enumerate(runs):
        dtype = (torch.int32, torch.int64)[k & 1]
        dm, du = on_device(m, dtype), on_device(u, dtype)
        for floor in (1.0, 0.25):
            g = mdk.diff_groups(dm, du, [ga, gb], min_dispersion=floor, steps=True)
            r = mdk.diff_replicates(dm, du, ga, gb, min_dispersion=floor, steps=True)
            assert torch.equal(g[0][0], r[0]) and torch.equal(g[1][0], r[1]) and torch.equal(g[0][1], r[2]) and torch.equal(g[1][1], r[3])
            assert equal_bits(g[2], r[4].abs())
            for ours, its in ((5, 5), (6, 6), (8, 7), (9, 8), (10, 9)):              # pvalue, df, dispersion, statistic, steps
                assert equal_bits(g[ours], r[its]), (k, floor, ours)
            both = (r[0] + r[1] > 0) & (r[2] + r[3] > 0)
            assert torch.equal(g[7], both.to(torch.int32))
            lo = torch.where(r[4] < 0, 1, 0).to(torch.int32)
            assert torch.equal(g[3][both], lo[both]) and torch.equal(g[4][both], torch.where(r[4] > 0, 1, 0).to(torch.int32)[both])


def wide(G, size, count, seed):
    """sites of G groups of `size` samples each, all covered (as tests/test_gdiff_cpu.py makes them)"""
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


@pytest.mark.parametrize("G,size", [(2, 512), (512, 2), (1024, 1)])
def test_the_most_samples(G, size):
    """1,024 samples, the buffers of the order and of the groups' ends full: two groups of 512 (nu = 1022), 512 groups of two (q = 511, nu =
    512) and 1,024 groups of one, a design without replicates, where every site has p 1.0 and df 0"""
    import torch
    import methyldackel_amd as mdk
    m, u, groups, want = columns(wide(G, size, 3, G))
    assert want[2][4] == [1024 - G] * 3 and want[2][5] == [G - 1] * 3
    got = mdk.diff_groups(on_device(m, torch.int32), on_device(u, torch.int32), [g[::-1] for g in groups], steps=True)
    assert same(got, want) and got[10].cpu().tolist() == want[3]
    if size == 1:
        assert want[2][3] == [1.0] * 3 and want[2][6] == [1.0] * 3 and want[3] == [0] * 3
    got = mdk.diff_groups(on_device(m, torch.int64), on_device(u, torch.int64), groups, min_dispersion=0.25)
    assert same(got, columns(wide(G, size, 3, G), 0.25)[3])


def long_site():
    """24 samples in four groups of six whose statistic stands where the tail's two series meet and are longest"""
    rng = random.Random(619)
    m, u = [], []
    for s in range(24):
        n = rng.randint(15, 40)
        f = (0.5, 0.58, 0.44, 0.53)[s // 6] + rng.uniform(-0.1, 0.1)
        k = sum(1 for _ in range(n) if rng.random() < f)
        m.append(k); u.append(n - k)
    return m, u


@pytest.mark.parametrize("at", [0, 63, 64, 300])
def test_a_long_series_does_not_disturb_its_neighbours(at):
    """513 sites of four groups of two samples -- the other sixteen rows without coverage there -- and one site of all 24 with a series
    several times as long as any other's, wherever it stands in its wavefront"""
    import torch
    import methyldackel_amd as mdk
    groups = [list(range(6 * g, 6 * g + 6)) for g in range(4)]
    few = [0, 1, 6, 7, 12, 13, 18, 19]
    sm, su = matrices(514, 8, seed=77, uncovered=0.0, groups=[[0, 1], [2, 3], [4, 5], [6, 7]])
    m, u = [[0] * 514 for _ in range(24)], [[0] * 514 for _ in range(24)]
    for r, s in enumerate(few):
        m[s], u[s] = sm[r], su[r]
    lm, lu = long_site()
    for s in range(24):
        m[s][at], u[s][at] = lm[s], lu[s]
    want = expected(m, u, groups)
    steps = want[3]
    assert steps[at] > 200 and want[2][4][at] == 20 and want[2][5][at] == 3 and 1.4 < want[2][7][at] < 1.6
    assert 2 * max(st for i, st in enumerate(steps) if i != at) < steps[at]
    got = mdk.diff_groups(on_device(m, torch.int32), on_device(u, torch.int32), groups, steps=True)
    assert same(got, want) and got[10].cpu().tolist() == steps
    # the neighbours' bits are those of the call without the long site
    for s in range(24):
        m[s][at], u[s][at] = (sm[few.index(s)][at], su[few.index(s)][at]) if s in few else (0, 0)
    plain = mdk.diff_groups(on_device(m, torch.int32), on_device(u, torch.int32), groups)
    keep = torch.arange(514, device="cuda") != at
    for x, y in zip(plain, got[:10]):
        assert equal_bits(x[..., keep], y[..., keep])


GROUPS3 = [[1, 0], [3, 2], [4]]


def refused_matrices(placed):
    """513 accepted sites of five samples in three groups (2, 2, 1), and the given sites at the given places"""
    m, u = matrices(513, 5, seed=5, groups=GROUPS3)
    for at, s in placed:
        flat = [(mm, uu) for ms, us in s for mm, uu in zip(ms, us)]
        assert len(flat) == 5
        for r, (mm, uu) in enumerate(flat):
            m[r][at], u[r][at] = mm, uu
    return m, u


@pytest.mark.parametrize("name,t,bit", REFUSED, ids=[f"{r[0].replace(' ', '_')}{i}" for i, r in enumerate(REFUSED)])
def test_refusals_name_the_first_site(name, t, bit):
    """each refused condition among accepted sites, at site 300 and again behind it: rc -3, diff_counts's words, the first such site; the
    refused sites have the outputs of a site without anything to test, the others their own"""
    import torch
    import methyldackel_amd as mdk
    lowest = bit & -bit
    m, u = refused_matrices([(300, t), (301, t), (512, t)])
    for dtype in (torch.int32, torch.int64):
        with pytest.raises(mdk.MdkError, match=re.escape(MESSAGES[lowest]) + r".*\(site 300\)") as e:
            mdk.diff_groups(on_device(m, dtype), on_device(u, dtype), GROUPS3)
        assert e.value.rc == -3 and "md_stats_gdiff" in str(e.value)
    # the call after a refused one is as any other
    m, u = matrices(257, 5, seed=6, groups=GROUPS3)
    assert same(mdk.diff_groups(on_device(m, torch.int32), on_device(u, torch.int32), GROUPS3), expected(m, u, GROUPS3))


def test_of_two_refused_sites_the_smaller_index_is_named():
    """in whatever workgroup they stand, and whichever of them has the lower bit"""
    import torch
    import methyldackel_amd as mdk
    negative, entry, margin = REFUSED[0][1], REFUSED[2][1], REFUSED[4][1]
    for (lo, first), (hi, second), text in (((40, margin), (300, negative), MESSAGES[4]), ((299, negative), (300, entry), MESSAGES[1]),
                                            ((7, entry), (8, negative), MESSAGES[2]), ((0, margin), (512, margin), MESSAGES[4])):
        m, u = refused_matrices([(hi, second), (lo, first)])
        with pytest.raises(mdk.MdkError, match=re.escape(text) + rf".*\(site {lo}\)"):
            mdk.diff_groups(on_device(m, torch.int32), on_device(u, torch.int32), [[0, 1], [2, 3], [4]])
    # the methylated of ALL groups, pooled over groups whose own depths are accepted; and a sample that is not used is not read
    third = LIMIT // 3 + 1
    m, u = [[1, third], [2, third], [3, third], [2, 2]], [[1, 0], [1, 0], [1, 1], [3, 1]]
    with pytest.raises(mdk.MdkError, match=r"pooled margin.*\(site 1\)"):
        mdk.diff_groups(on_device(m, torch.int32), on_device(u, torch.int32), [[0], [1], [2, 3]])
    m[1][0] = -5
    assert same(mdk.diff_groups(on_device(m, torch.int32), on_device(u, torch.int32), [[0], [2, 3]]), expected(m, u, [[0], [2, 3]]))


def cohort_of(sites):
    """a hand-made Cohort of sites of one shape on one contig: its groups and what is expected of it"""
    import torch
    import methyldackel_amd as mdk
    m, u, groups, want = columns(sites)
    n = len(sites)
    cols = {"contig": torch.zeros(n, dtype=torch.int32), "start": torch.arange(n, dtype=torch.int32) * 100, "end": torch.arange(n, dtype=torch.int32) * 100 + 1,
            "context": torch.zeros(n, dtype=torch.uint8), "strand": torch.ones(n, dtype=torch.int8), "nsamples": torch.full((n,), len(m), dtype=torch.int32)}
    return mdk.Cohort(["chr1"], {k: v.cuda() for k, v in cols.items()}, on_device(m, torch.int32), on_device(u, torch.int32)), groups, want, mdk


def united():
    """four samples over one universe of sites, united: hand-made Calls, no BAM"""
    import torch
    import methyldackel_amd as mdk
    from merge_rule import COLUMNS
    from unite_rule import CONTIGS, sample
    samples = [mdk.Calls(list(CONTIGS), {n: torch.from_numpy(c.copy()).cuda() for n, c in zip(COLUMNS, sample(513, s))}) for s in range(4)]
    return mdk.unite(samples, min_samples=2), mdk


def test_cohort_diff_groups(tmp_path):
    import torch
    co, mdk = united()
    assert len(co) > 100
    groups = [[3, 0], [1], [2]]
    d = co.diff_groups(groups, names=["ctl", "het", "hom"])
    assert type(d) is mdk.GroupDiff and not isinstance(d, mdk.Diff) and len(d) == len(co) and d.contigs == co.contigs and d.merged == co.merged
    assert d.n_groups == 3 and d.names == ("ctl", "het", "hom") and co.diff_groups(groups).names == ("g0", "g1", "g2")
    for name in ("contig", "start", "end", "context", "strand"):
        assert getattr(d, name) is getattr(co, name), name
    want = expected(co.nmeth.cpu().tolist(), co.nunmeth.cpu().tolist(), groups)
    assert same([d.nmeth, d.nunmeth] + [getattr(d, n) for n in NAMES], want)
    assert same(mdk.diff_groups(co.nmeth, co.nunmeth, groups), want)
    assert 0 < sum(1 for p in want[2][3] if p < 1.0) and set(want[2][4]) <= {0, 1}
    # rows, select, write and the file read back
    rows = d.rows()
    assert len(rows[0]) == 5 + 3 + 8 and rows[0][0] == co.contigs[int(co.contig[0])]
    assert [r[5:8] for r in rows] == [tuple(zip(a, b)) for a, b in zip(zip(*want[0]), zip(*want[1]))] and [r[8:] for r in rows] == list(zip(*want[2]))
    mask = d.pvalue < 0.9
    s = d.select(mask)
    assert type(s) is mdk.GroupDiff and 0 < len(s) < len(d) and s.rows() == [r for r, k in zip(rows, mask.cpu().tolist()) if k] and s.merged == d.merged and s.names == d.names
    path = d.write(str(tmp_path / "gdiff.tsv"))
    lines = [l.rstrip("\n").split("\t") for l in open(path)]
    assert lines[0] == ["#chrom", "start", "end", "context", "strand", "ctl.nmeth", "ctl.nunmeth", "het.nmeth", "het.nunmeth", "hom.nmeth", "hom.nunmeth"] + list(NAMES)
    back = lines[1:]
    assert len(back) == len(rows) and all(len(r) == 19 for r in back)
    flat = [r[:5] + tuple(v for pair in r[5:8] for v in pair) + r[8:] for r in rows]
    doubles = (11, 14, 17, 18)
    assert [tuple([r[0]] + [bits(float(x)) if i in doubles else int(x) for i, x in enumerate(r) if i]) for r in back] == \
           [tuple([r[0]] + [bits(x) if i in doubles else x for i, x in enumerate(r) if i]) for r in flat]
    # qvalue: Benjamini and Hochberg of the omnibus p-values
    q = d.qvalue()
    assert q.dtype == torch.float64 and q.device == d.pvalue.device and [bits(x) for x in q.cpu().tolist()] == [bits(x) for x in bh(want[2][3])]
    # a pair of groups: Cohort.diff of them, column for column
    for i, j in ((0, 2), (2, 1), (1, 0)):
        c, f = d.contrast(i, j), co.diff(groups[i], groups[j])
        assert type(c) is mdk.Diff and len(c) == len(d)
        for name, _ in mdk.Diff.COLUMNS:
            assert equal_bits(getattr(c, name), getattr(f, name)), (i, j, name)
        assert c.start is co.start
    with pytest.raises(mdk.MdkError, match="both groups"):
        co.diff_groups([[0, 1], [1], [2]])


def test_cohort_without_sites_and_region_sums():
    import torch
    co, mdk = united()
    empty = co.select(slice(0, 0)).diff_groups([[0, 1], [2], [3]])
    assert type(empty) is mdk.GroupDiff and len(empty) == 0 and empty.rows() == [] and len(empty.qvalue()) == 0 and empty.n_groups == 3
    assert empty.nmeth.shape == (3, 0) and empty.nmeth.dtype == torch.int64
    for name, dt in mdk.GroupDiff.COLUMNS:
        t = getattr(empty, name)
        assert t.shape == (0,) and t.dtype == getattr(torch, dt) and t.device.type == "cuda", name
    assert len(empty.contrast(0, 1)) == 0
    # on the sums of a CohortRegions
    starts, ends = co.start.cpu().tolist(), co.end.cpu().tolist()
    first = [i for i, c in enumerate(co.contig.cpu().tolist()) if c == 0]
    tiles = mdk.Intervals(co.contigs, torch.zeros(4, dtype=torch.int32).cuda(), torch.tensor([starts[first[k * len(first) // 4]] for k in range(4)], dtype=torch.int32).cuda(),
                          torch.tensor([starts[first[(k + 1) * len(first) // 4 - 1]] + 1 for k in range(4)], dtype=torch.int32).cuda())
    per = co.regions(tiles)
    got = mdk.diff_groups(per.nmeth, per.nunmeth, [[0, 1], [2], [3]])
    assert same(got, expected(per.nmeth.cpu().tolist(), per.nunmeth.cpu().tolist(), [[0, 1], [2], [3]])) and int(per.nmeth.sum()) > 0


def test_calibration_on_the_device():
    """4,000 sites without a difference, three groups of three over-dispersed replicates (rho = 0.2): the rule's p-values bit for bit,
    and the F test rejects about one in twenty at 0.05 -- the CPU test's band; the rule gives 4.725 %"""
    sites = null_sites()
    assert len(sites) == 4000
    co, groups, want, mdk = cohort_of(sites)
    d = co.diff_groups(groups)
    assert same([d.nmeth, d.nunmeth] + [getattr(d, name) for name in NAMES], want)
    rate = float((d.pvalue < 0.05).sum()) / len(sites)
    print(f"rejected at 0.05: F test of three groups {rate:.5f}")
    assert 0.02 <= rate <= 0.08 and rate == sum(1 for p in want[2][3] if p < 0.05) / 4000.0
