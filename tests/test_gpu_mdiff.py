"""GPU: a site's counts regressed on a design matrix on the device (k_mdiff of csrc/mdk_mdiff.hip, libmdk_stats.so) -- mdk.diff_model,
Cohort.diff_model and its ModelDiff.  Every comparison is exact, the integers equal and the doubles as their 64-bit patterns: against the
Python restatement of the rule (tests/mdiff_rule.py) and, where the sites are many, against the host build of the same header
(tools/mdiff_emu), which tests/test_mdiff_cpu.py holds against the restatement bit for bit, against mpmath and against the test of
several groups.  No Session and no BAM: the cohorts are hand-made."""
import random
import re
import struct
import subprocess

import pytest

from conftest import REPO
from diff_rule import MESSAGES, bh, bits
from mdiff_rule import ACCEPTED, FULL, HAND, NAMES, NUMERIC, PLAIN, RANK, REDUCED, REFUSED, paired_null_sites, seeded, site

pytestmark = pytest.mark.gpu
EMU = REPO / "tools" / "_build" / "mdiff_emu"
DTYPES = ("float64", "int32", "float64", "float64", "uint8", "int32")
# both sides of a wavefront's 64 sites and of a workgroup's 256, several workgroups, and a short last one
SIZES = (1, 63, 64, 65, 255, 256, 257, 513, 4100)
# (S, the used samples in the design's row order -- unsorted, some samples in none --, the design's columns beside the intercept, the tested columns)
CASES = [(5, [3, 0, 4, 1], ("group",), [1]), (6, [5, 1, 0, 4, 2, 3], ("dose", "group"), [1]), (8, [7, 2, 0, 5, 6, 1, 3], ("group", "batch", "dose"), [3, 1]),
         (12, [11, 7, 0, 2, 9, 1, 10, 6, 4, 5], ("batch", "dose", "group", "age", "pair"), [3]),
         (12, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], ("batch", "dose", "group", "age", "pair", "sex", "lot"), [0, 7])]


def pattern(x):
    return "%016x" % (bits(x) & (2 ** 64 - 1))


def number(digits):
    return struct.unpack("<d", struct.pack("<Q", int(digits, 16)))[0]


def design_for(columns, rows, seed):
    """a design of `rows` rows: an intercept, then a column of every named kind"""
    rng = random.Random(seed)
    out = [[1.0] for _ in range(rows)]
    for c, kind in enumerate(columns):
        for k in range(rows):
            out[k].append({"group": float(k % 2), "batch": float(k >= rows // 2), "pair": float(k // 2 == 1), "sex": float(k % 3 == 0), "lot": float(k % 4 == 1)}.get(kind, round(rng.uniform(-2.0, 2.0), 2)))
    return out


def matrices(n, S, seed, uncovered=0.1):
    """two lists of S rows of n counts: depths 1 to 40 around a fraction per site, every second site with a shift in the odd samples, a
    tenth of the entries without coverage; now and then a site all methylated or all unmethylated, now and then the odd samples all
    methylated: a separated fit"""
    rng = random.Random(seed)
    m, u = [[0] * n for _ in range(S)], [[0] * n for _ in range(S)]
    for i in range(n):
        f = rng.choice((0.0, 1.0)) if rng.random() < 0.04 else rng.uniform(0.1, 0.9)
        shift = rng.uniform(-0.4, 0.4) if i & 1 and 0.0 < f < 1.0 else 0.0
        full = rng.random() < 0.04
        for s in range(S):
            if rng.random() < uncovered:
                continue
            depth = rng.randint(1, 40)
            g = f + (shift if s & 1 else 0.0) + (rng.uniform(-0.1, 0.1) if 0.0 < f < 1.0 else 0.0)
            k = depth if full and s & 1 else int(round(depth * min(1.0, max(0.0, g))))
            m[s][i], u[s][i] = k, depth - k
    return m, u


def expected(m, u, samples, design, test, floor=1.0):
    """what mdk.diff_model gives for count matrices (lists of rows): (coef as p lists, K, M, the six lists of NAMES, steps), from the host
    build of the header.  The used samples are visited ascending, however they were given, and the tested columns are the last"""
    p, tested = len(design[0]), [test] if isinstance(test, int) else list(test)
    columns = [j for j in range(p) if j not in tested] + tested
    by_sample = sorted(range(len(samples)), key=lambda k: samples[k])
    rows = " ".join(pattern(design[k][j]) for k in by_sample for j in columns)
    used = [samples[k] for k in by_sample]
    head = "s %s %d %d %d " % (pattern(floor), len(used), p, len(tested))
    text = "".join(head + " ".join("%d %d" % (m[s][i], u[s][i]) for s in used) + " " + rows + "\n" for i in range(len(m[0])))
    r = subprocess.run([str(EMU)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [l.split("\t") for l in r.stdout.splitlines()]
    assert all(g[0] == "0" for g in got)
    coef = [[number(g[10 + columns.index(j)]) for g in got] for j in range(p)]
    cols = [[number(g[1]) for g in got], [int(g[2]) for g in got], [number(g[3]) for g in got], [number(g[4]) for g in got], [int(g[5]) for g in got], [int(g[6]) for g in got]]
    return coef, [int(g[8]) for g in got], [int(g[9]) for g in got], cols, [int(g[7]) for g in got]


def by_the_rule(sites, floor=1.0):
    """the same for sites of mdiff_rule that share a design, from the restatement in Python floats: the matrices' rows, and what is expected"""
    m = [list(r) for r in zip(*[s[0] for s in sites])]
    u = [list(r) for r in zip(*[s[1] for s in sites])]
    out = [site(*s, floor) for s in sites]
    p = len(sites[0][2][0])
    return m, u, ([[o[2][j] for o in out] for j in range(p)], [o[0] for o in out], [o[1] for o in out], [[o[3][c] for o in out] for c in range(6)], [o[4] for o in out])


def on_device(rows, dtype):
    import torch
    return torch.tensor(rows, dtype=dtype).cuda()


def equal_bits(x, y):
    import torch
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)


def same(got, want):
    """the nine tensors of a call against (coef, K, M, the six lists): the dtypes the stated ones, the integers equal, the doubles bit for bit"""
    import torch
    coef, K, M, cols = want[:4]
    g = got[0]
    if g.dtype != torch.float64 or g.shape != (len(coef), len(K)) or not g.is_contiguous():
        return False
    if not torch.equal(g.view(torch.int64).cpu(), torch.tensor([[bits(x) for x in row] for row in coef], dtype=torch.int64).reshape(g.shape)):
        return False
    for g, w in ((got[1], K), (got[2], M)):
        if g.dtype != torch.int64 or not torch.equal(g.cpu(), torch.tensor(w, dtype=torch.int64)):
            return False
    for name, dt, g, w in zip(NAMES, DTYPES, got[3:9], cols):
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
    """all nine outputs and the term counts for every size, designs of 2 to 8 columns, unused samples, the samples unsorted, the tested
    columns anywhere, both element widths; the inputs as they were after the call; sorted samples give the same bits"""
    import torch
    import methyldackel_amd as mdk
    seen, terms = [[] for _ in NAMES], []
    for k, (S, samples, columns, test) in enumerate(CASES if n <= 513 else CASES[2:4]):
        design = design_for(columns, len(samples), seed=k)
        m, u = matrices(n, S, seed=1000 * n + k)
        want = expected(m, u, samples, design, test)
        for dtype in (torch.int32, torch.int64):
            dm, du = on_device(m, dtype), on_device(u, dtype)
            keep = dm.clone(), du.clone()
            got = mdk.diff_model(dm, du, design, test, samples=samples, steps=True)
            assert len(got) == 10 and same(got, want), (n, S, columns, dtype)
            assert got[9].dtype == torch.uint32 and got[9].cpu().tolist() == want[4]
            assert torch.equal(dm, keep[0]) and torch.equal(du, keep[1])
            for t in got:
                assert t.shape[-1] == n and t.device == dm.device and t.is_contiguous()
            by_sample = sorted(range(len(samples)), key=lambda j: samples[j])
            again = mdk.diff_model(dm, du, torch.tensor([design[j] for j in by_sample], dtype=torch.float64), test, samples=[samples[j] for j in by_sample])
            assert len(again) == 9 and all(equal_bits(x, y) for x, y in zip(again, got))
        for c, column in enumerate(want[3]):
            seen[c].extend(column)
        terms.extend(want[4])
    if n >= 255:                                                                        # what the sites of a size hold, all cases together
        assert max(terms) > 5 and any(p < 0.05 for p in seen[0]) and 0 < sum(1 for p in seen[0] if p == 1.0) < len(seen[0])
        assert len(set(seen[1])) > 3 and max(seen[5]) > 25 and min(seen[5]) == 0         # uncovered samples here and there; separated fits; degenerate sites
        assert any(f & RANK for f in seen[4]) and any(f & NUMERIC for f in seen[4])     # the pair's two samples without coverage; a pivot lost


@pytest.mark.parametrize("floor", [1.0, 0.25])
def test_the_rule_s_own_sites_on_the_device(floor):
    """mdiff_rule.seeded(), HAND and ACCEPTED, every site with the design it has -- a call a site --; at the default floor what is known
    by hand of HAND.  Every flag is among them"""
    import torch
    import methyldackel_amd as mdk
    named = [(None, s, None) for s in seeded()] + list(HAND) + [(None, s, None) for s in ACCEPTED]
    assert len(named) > 600
    flags = set()
    for k, (name, s, known) in enumerate(named):
        if floor != 1.0 and k % 8 and name is None:
            continue
        m, u, want = by_the_rule([s], floor)
        p, q = len(s[2][0]), s[3]
        dtype = (torch.int32, torch.int64)[k & 1]
        got = mdk.diff_model(on_device(m, dtype), on_device(u, dtype), s[2], list(range(p - q, p)), min_dispersion=floor, steps=True)
        assert same(got, want), (s, floor)
        assert got[9].cpu().tolist() == want[4]
        flags.add(want[3][4][0])
        for col, v in (known or {} if floor == 1.0 else {}).items():                     # (what is known by hand is known at the default floor)
            assert got[3 + NAMES.index(col)].cpu().tolist()[0] == v, (name, col)
    assert {0, RANK, NUMERIC, FULL, REDUCED | FULL} <= flags


def wide_sites(count, seed):
    """sites of 1,024 samples and a design of eight columns"""
    rng = random.Random(seed)
    X = [[1.0, float(s % 2), float(s % 3 == 0), float(s >= 512), round(rng.uniform(-2.0, 2.0), 3), round(rng.uniform(0.0, 1.0), 3), float(s % 5 == 1), float(s % 7 < 3)] for s in range(1024)]
    out = []
    for _ in range(count):
        ms, us = [], []
        for s in range(1024):
            n = 0 if rng.random() < 0.05 else rng.randint(5, 40)
            f = min(0.95, max(0.05, 0.5 + 0.08 * X[s][1] - 0.05 * X[s][4] + rng.uniform(-0.15, 0.15)))
            k = sum(1 for _ in range(n) if rng.random() < f)
            ms.append(k); us.append(n - k)
        out.append((ms, us, X, 2))
    return out


def test_the_most_samples_and_columns():
    """1,024 samples and eight columns, the buffers of the order and of the design full: three sites"""
    import torch
    import methyldackel_amd as mdk
    sites = wide_sites(3, 1024)
    m, u, want = by_the_rule(sites)
    assert all(900 < df < 1017 for df in want[3][1]) and want[3][4] == [0, 0, 0] and all(0.0 < p < 1.0 for p in want[3][0])
    order = list(range(1023, -1, -1))
    got = mdk.diff_model(on_device(m, torch.int32), on_device(u, torch.int32), [sites[0][2][s] for s in order], [6, 7], samples=order, steps=True)
    assert same(got, want) and got[9].cpu().tolist() == want[4]
    got = mdk.diff_model(on_device(m, torch.int64), on_device(u, torch.int64), sites[0][2], [6, 7], min_dispersion=0.25)
    assert same(got, by_the_rule(sites, 0.25)[2])


@pytest.mark.parametrize("at", [0, 63, 64, 300])
def test_a_long_fit_does_not_disturb_its_neighbours(at):
    """514 sites of two groups of three whose fits take a few passes, and one site with a group all methylated -- a separated fit of
    some thirty passes --, wherever it stands in its wavefront"""
    import torch
    import methyldackel_amd as mdk
    rng = random.Random(77)
    m, u = [[0] * 514 for _ in range(6)], [[0] * 514 for _ in range(6)]
    for i in range(514):
        f = rng.uniform(0.3, 0.7)
        for s in range(6):
            depth = rng.randint(10, 40)
            k = int(round(depth * min(0.9, max(0.1, f + (0.1 if s >= 3 else 0.0) + rng.uniform(-0.08, 0.08)))))
            m[s][i], u[s][i] = k, depth - k
    plain_m, plain_u = [r[at] for r in m], [r[at] for r in u]
    for s in range(6):
        m[s][at], u[s][at] = (20 + s, 17 - s) if s < 3 else (30 + s, 0)
    want = expected(m, u, list(range(6)), PLAIN, 1)
    its = want[3][5]
    assert its[at] >= 28 and want[3][4][at] == 0 and 3 * max(v for i, v in enumerate(its) if i != at) < its[at]
    got = mdk.diff_model(on_device(m, torch.int32), on_device(u, torch.int32), PLAIN, 1, steps=True)
    assert same(got, want) and got[9].cpu().tolist() == want[4]
    # the neighbours' bits are those of the call without the long site
    for s in range(6):
        m[s][at], u[s][at] = plain_m[s], plain_u[s]
    plain = mdk.diff_model(on_device(m, torch.int32), on_device(u, torch.int32), PLAIN, 1)
    keep = torch.arange(514, device="cuda") != at
    for x, y in zip(plain, got[:9]):
        assert equal_bits(x[..., keep], y[..., keep])


def refused_matrices(placed):
    """513 accepted sites of six samples, and the given sites at the given places"""
    m, u = matrices(513, 6, seed=5)
    for at, (ms, us) in placed:
        for r in range(6):
            m[r][at], u[r][at] = ms[r], us[r]
    return m, u


@pytest.mark.parametrize("name,t,bit", REFUSED, ids=[f"{r[0].replace(' ', '_')}{i}" for i, r in enumerate(REFUSED)])
def test_refusals_name_the_first_site(name, t, bit):
    """each refused condition among accepted sites, at site 300 and again behind it: rc -3, diff_counts's words, the first such site; the
    call after a refused one is as any other"""
    import torch
    import methyldackel_amd as mdk
    lowest = bit & -bit
    m, u = refused_matrices([(300, t), (301, t), (512, t)])
    for dtype in (torch.int32, torch.int64):
        with pytest.raises(mdk.MdkError, match=re.escape(MESSAGES[lowest]) + r".*\(site 300\)") as e:
            mdk.diff_model(on_device(m, dtype), on_device(u, dtype), PLAIN, 1)
        assert e.value.rc == -3 and "md_stats_mdiff" in str(e.value)
    m, u = matrices(257, 6, seed=6)
    assert same(mdk.diff_model(on_device(m, torch.int32), on_device(u, torch.int32), PLAIN, 1), expected(m, u, list(range(6)), PLAIN, 1))


def test_of_two_refused_sites_the_smaller_index_is_named_and_the_design_is_checked():
    """in whatever workgroup they stand, and whichever of them has the lower bit; a sample that is not used is not read; and what the
    library refuses of a design before it launches"""
    import torch
    import methyldackel_amd as mdk
    negative, entry, margin = REFUSED[0][1], REFUSED[2][1], REFUSED[4][1]
    for (lo, first), (hi, second), text in (((40, margin), (300, negative), MESSAGES[4]), ((299, negative), (300, entry), MESSAGES[1]),
                                            ((7, entry), (8, negative), MESSAGES[2]), ((0, margin), (512, margin), MESSAGES[4])):
        m, u = refused_matrices([(hi, second), (lo, first)])
        with pytest.raises(mdk.MdkError, match=re.escape(text) + rf".*\(site {lo}\)"):
            mdk.diff_model(on_device(m, torch.int32), on_device(u, torch.int32), PLAIN, 1)
    m, u = matrices(65, 6, seed=8)
    m[2][10] = -5
    with pytest.raises(mdk.MdkError, match=r"negative.*\(site 10\)"):
        mdk.diff_model(on_device(m, torch.int32), on_device(u, torch.int32), PLAIN, 1)
    five = [0, 1, 3, 4, 5]
    rows = [PLAIN[s] for s in five]
    assert same(mdk.diff_model(on_device(m, torch.int32), on_device(u, torch.int32), rows, 1, samples=five), expected(m, u, five, rows, 1))
    m[2][10] = 5
    dm, du = on_device(m, torch.int32), on_device(u, torch.int32)
    for design, text in (([[1.0, 0.0, 1.0], [1.0, 1.0, 0.0]] * 3, "columns are dependent"), ([[1.0, 0.0]] * 6, "columns are dependent"),
                         ([[1.0, 1.0 + 2.0 ** -30 * s] for s in range(6)], "columns are dependent")):
        with pytest.raises(mdk.MdkError, match=text) as e:
            mdk.diff_model(dm, du, design, 1)
        assert e.value.rc == -3 and "md_stats_mdiff" in str(e.value)
    assert same(mdk.diff_model(dm, du, PLAIN, 1), expected(m, u, list(range(6)), PLAIN, 1))          # the call after a refused one is as any other


def united():
    """four samples over one universe of sites, united: hand-made Calls, no BAM"""
    import torch
    import methyldackel_amd as mdk
    from merge_rule import COLUMNS
    from unite_rule import CONTIGS, sample
    samples = [mdk.Calls(list(CONTIGS), {n: torch.from_numpy(c.copy()).cuda() for n, c in zip(COLUMNS, sample(513, s))}) for s in range(4)]
    return mdk.unite(samples, min_samples=2), mdk


PAIRS = [[1.0, 0.0], [1.0, 1.0], [1.0, 1.0], [1.0, 0.0]]                          # four samples: an intercept and the group


def test_cohort_diff_model(tmp_path):
    import torch
    co, mdk = united()
    assert len(co) > 100
    d = co.diff_model(PAIRS, 1, names=["intercept", "group"])
    assert type(d) is mdk.ModelDiff and not isinstance(d, mdk.Diff) and len(d) == len(co) and d.contigs == co.contigs and d.merged == co.merged
    assert d.n_columns == 2 and d.tested == (1,) and d.names == ("intercept", "group") and co.diff_model(PAIRS, [1]).names == ("x0", "x1")
    for name in ("contig", "start", "end", "context", "strand"):
        assert getattr(d, name) is getattr(co, name), name
    want = expected(co.nmeth.cpu().tolist(), co.nunmeth.cpu().tolist(), [0, 1, 2, 3], PAIRS, 1)
    assert same([d.coef, d.nmeth, d.nunmeth] + [getattr(d, n) for n in NAMES], want)
    assert same(mdk.diff_model(co.nmeth, co.nunmeth, PAIRS, 1), want)
    assert 0 < sum(1 for p in want[3][0] if p < 1.0) and set(want[3][1]) <= {0, 1, 2}
    # the tested column first: the coefficients come back in the caller's order
    swapped = co.diff_model([[row[1], row[0]] for row in PAIRS], 0)
    assert swapped.tested == (0,) and equal_bits(swapped.coef, d.coef.flip(0).contiguous()) and equal_bits(swapped.pvalue, d.pvalue)
    # rows, select, write and the file read back
    rows = d.rows()
    assert len(rows[0]) == 5 + 2 + 1 + 6 and rows[0][0] == co.contigs[int(co.contig[0])]
    assert [r[5:7] for r in rows] == list(zip(want[1], want[2])) and [r[7] for r in rows] == list(zip(*want[0])) and [r[8:] for r in rows] == list(zip(*want[3]))
    mask = d.pvalue < 0.9
    s = d.select(mask)
    assert type(s) is mdk.ModelDiff and 0 < len(s) < len(d) and s.rows() == [r for r, k in zip(rows, mask.cpu().tolist()) if k] and s.merged == d.merged and s.names == d.names
    path = d.write(str(tmp_path / "mdiff.tsv"))
    lines = [l.rstrip("\n").split("\t") for l in open(path)]
    assert lines[0] == ["#chrom", "start", "end", "context", "strand", "nmeth", "nunmeth", "coef.intercept", "coef.group"] + list(NAMES)
    back = lines[1:]
    assert len(back) == len(rows) and all(len(r) == 15 for r in back)
    flat = [r[:7] + r[7] + r[8:] for r in rows]
    doubles = (7, 8, 9, 11, 12)
    assert [tuple([r[0]] + [bits(float(x)) if i in doubles else int(x) for i, x in enumerate(r) if i]) for r in back] == \
           [tuple([r[0]] + [bits(x) if i in doubles else x for i, x in enumerate(r) if i]) for r in flat]
    # qvalue: Benjamini and Hochberg of the p-values; and regions joined on a pair's direction
    q = d.qvalue()
    assert q.dtype == torch.float64 and q.device == d.pvalue.device and [bits(x) for x in q.cpu().tolist()] == [bits(x) for x in bh(want[3][0])]
    regions = co.diff([0, 3], [1, 2]).dmrs(q < 0.9)
    assert type(regions) is mdk.Dmrs
    with pytest.raises(mdk.MdkError, match="named twice"):
        co.diff_model(PAIRS, 1, samples=[0, 1, 1, 2])


def test_cohort_without_sites_and_region_sums():
    import torch
    co, mdk = united()
    empty = co.select(slice(0, 0)).diff_model(PAIRS, 1)
    assert type(empty) is mdk.ModelDiff and len(empty) == 0 and empty.rows() == [] and len(empty.qvalue()) == 0 and empty.n_columns == 2
    assert empty.coef.shape == (2, 0) and empty.coef.dtype == torch.float64
    for name, dt in mdk.ModelDiff.COLUMNS:
        t = getattr(empty, name)
        assert t.shape == (0,) and t.dtype == getattr(torch, dt) and t.device.type == "cuda", name
    # on the sums of a CohortRegions
    starts = co.start.cpu().tolist()
    first = [i for i, c in enumerate(co.contig.cpu().tolist()) if c == 0]
    tiles = mdk.Intervals(co.contigs, torch.zeros(4, dtype=torch.int32).cuda(), torch.tensor([starts[first[k * len(first) // 4]] for k in range(4)], dtype=torch.int32).cuda(),
                          torch.tensor([starts[first[(k + 1) * len(first) // 4 - 1]] + 1 for k in range(4)], dtype=torch.int32).cuda())
    per = co.regions(tiles)
    got = mdk.diff_model(per.nmeth, per.nunmeth, PAIRS, 1)
    assert same(got, expected(per.nmeth.cpu().tolist(), per.nunmeth.cpu().tolist(), [0, 1, 2, 3], PAIRS, 1)) and int(per.nmeth.sum()) > 0


def test_calibration_on_the_device():
    """4,000 sites without a group effect, six patients with a sample in either group, a patient effect and intra-class correlation 0.2,
    a dummy per patient beside the group: the rule's outputs bit for bit, and its rejection rate at 0.05 exactly -- the CPU test's
    band; the rule gives 5.775 %"""
    import torch
    import methyldackel_amd as mdk
    sites = paired_null_sites()
    assert len(sites) == 4000
    m = [list(r) for r in zip(*[s[0] for s in sites])]
    u = [list(r) for r in zip(*[s[1] for s in sites])]
    X = sites[0][2]
    want = expected(m, u, list(range(12)), X, 6)
    n = len(sites)
    cols = {"contig": torch.zeros(n, dtype=torch.int32), "start": torch.arange(n, dtype=torch.int32) * 100, "end": torch.arange(n, dtype=torch.int32) * 100 + 1,
            "context": torch.zeros(n, dtype=torch.uint8), "strand": torch.ones(n, dtype=torch.int8), "nsamples": torch.full((n,), 12, dtype=torch.int32)}
    co = mdk.Cohort(["chr1"], {k: v.cuda() for k, v in cols.items()}, on_device(m, torch.int32), on_device(u, torch.int32))
    d = co.diff_model(X, 6)
    assert same([d.coef, d.nmeth, d.nunmeth] + [getattr(d, name) for name in NAMES], want)
    rate = float((d.pvalue < 0.05).sum()) / n
    print(f"rejected at 0.05: the model with a dummy per patient {rate:.5f}")
    assert 0.02 <= rate <= 0.08 and rate == sum(1 for p in want[3][0] if p < 0.05) / 4000.0
