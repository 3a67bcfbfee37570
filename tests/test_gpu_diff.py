"""GPU: two groups of samples compared site by site on the device (k_diff of csrc/mdk_diff.hip) -- mdk.diff_counts, Cohort.diff and its
Diff.  Every comparison is exact, the doubles as their 64-bit patterns: against the Python restatement of the rule (tests/diff_rule.py),
which tests/test_diff_cpu.py holds against the host build of the same header and against exact rationals."""
import random
import re

import pytest

from diff_rule import ACCEPTED, HAND, LIMIT, MESSAGES, REFUSED, bh, bits, expected, pvalue

pytestmark = pytest.mark.gpu
NAMES = ("nmeth_a", "nunmeth_a", "nmeth_b", "nunmeth_b", "meth_diff", "pvalue")
# 1 .. 513: the issue's -- both sides of a wavefront's and of a workgroup's 256 sites; 2049 and 4100: many workgroups and a short last one
SIZES = (1, 255, 256, 257, 513, 2049, 4100)


def matrices(n, S, seed, top=12, zero=0.1):
    """two lists of S rows of n counts: shallow sites, a tenth of the entries without coverage"""
    rng = random.Random(seed)
    return tuple([[0 if rng.random() < zero else rng.randint(0, top) for _ in range(n)] for _ in range(S)] for _ in range(2))


def on_device(rows, dtype):
    import torch
    return torch.tensor(rows, dtype=dtype).cuda()


def same(got, want):
    """the six tensors against six lists: the integers equal, the doubles bit for bit"""
    import torch
    for name, g, w in zip(NAMES, got, want):
        if g.dtype == torch.float64:
            if not torch.equal(g.view(torch.int64).cpu(), torch.tensor([bits(x) for x in w], dtype=torch.int64)):
                return False
        elif g.dtype != torch.int64 or not torch.equal(g.cpu(), torch.tensor(w, dtype=torch.int64)):
            return False
    return True


# first in the file: the kernel's first execution
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_dtypes(n):
    """all six outputs for every size, S = 2, 3 and 7, unused samples, the groups in any order, both element widths; the inputs as they
    were after the call"""
    import torch
    import methyldackel_amd as mdk
    cases = [(2, [0], [1]), (2, [1], [0]), (3, [2], [0]), (3, [1, 0], [2]), (7, [5, 0, 3], [6, 1]), (7, [2], [4, 6, 0, 1])]
    for k, (S, ga, gb) in enumerate(cases if n <= 513 else cases[3:5]):
        m, u = matrices(n, S, seed=1000 * n + k)
        want = expected(m, u, ga, gb)
        for dtype in (torch.int32, torch.int64):
            dm, du = on_device(m, dtype), on_device(u, dtype)
            keep = dm.clone(), du.clone()
            got = mdk.diff_counts(dm, du, ga, gb)
            assert same(got, want), (n, S, ga, gb, dtype)
            assert torch.equal(dm, keep[0]) and torch.equal(du, keep[1])
            for t in got:
                assert t.shape == (n,) and t.device == dm.device and t.is_contiguous()
        if n >= 255:
            assert 0 < sum(1 for p in want[5] if p == 1.0) < n and any(p < 0.05 for p in want[5])


@pytest.mark.parametrize("at", [0, 63, 64, 300])
def test_a_deep_site_does_not_disturb_its_neighbours(at):
    """513 sites of depth at most 20 and one of 3,000 a cell: some 490 terms among sites of ten, wherever it stands in its wavefront"""
    import torch
    import methyldackel_amd as mdk
    m, u = matrices(513, 2, seed=77, top=5, zero=0.0)
    rng = random.Random(at)
    for s in range(2):
        m[s][at], u[s][at] = rng.randint(2900, 3000), rng.randint(2900, 3000)
    want = expected(m, u, [0], [1])
    assert pvalue(m[0][at], u[0][at], m[1][at], u[1][at])[1] > 400
    got = mdk.diff_counts(on_device(m, torch.int32), on_device(u, torch.int32), [0], [1])
    assert same(got, want)


def test_hand_tables_on_the_device():
    """a table a site: group A is sample 0, group B sample 1"""
    import torch
    import methyldackel_amd as mdk
    tables = [t for _, t, _ in HAND] + ACCEPTED
    m, u = [[t[0] for t in tables], [t[2] for t in tables]], [[t[1] for t in tables], [t[3] for t in tables]]
    got = mdk.diff_counts(on_device(m, torch.int64), on_device(u, torch.int64), [0], [1])
    assert same(got, expected(m, u, [0], [1]))
    p, diff = got[5].cpu().tolist(), got[4].cpu().tolist()
    for k, (name, t, want) in enumerate(HAND):
        if want is not None:
            assert p[k] == want, name
        if name.startswith("no coverage"):
            assert diff[k] == 0.0
    # every margin as a sum over several samples: the entries are small, the pooled counts are what is checked
    assert same(mdk.diff_counts(on_device([[LIMIT // 2 - 1], [LIMIT // 2], [0]], torch.int32), on_device([[0], [0], [7]], torch.int32), [0, 1], [2]),
                expected([[LIMIT // 2 - 1], [LIMIT // 2], [0]], [[0], [0], [7]], [0, 1], [2]))


@pytest.mark.parametrize("name,t,bit", REFUSED, ids=[f"{r[0]}{i}" for i, r in enumerate(REFUSED)])
def test_refusals_name_the_first_site(name, t, bit):
    """each refused condition alone, at site 300 of 513 and again behind it: rc -3, the message, the first site that has it"""
    import torch
    import methyldackel_amd as mdk
    m, u = matrices(513, 2, seed=5)
    for at in (300, 301, 512):
        m[0][at], u[0][at], m[1][at], u[1][at] = t
    dtype = torch.int64 if max(t) >= 2 ** 31 else torch.int32
    with pytest.raises(mdk.MdkError, match=re.escape(MESSAGES[bit]) + r".*\(site 300\)") as e:
        mdk.diff_counts(on_device(m, dtype), on_device(u, dtype), [0], [1])
    assert e.value.rc == -3
    # the call after a refused one is as any other
    m, u = matrices(257, 2, seed=6)
    assert same(mdk.diff_counts(on_device(m, dtype), on_device(u, dtype), [0], [1]), expected(m, u, [0], [1]))


def test_a_margin_pooled_over_samples_is_refused_and_an_unused_sample_is_not_read():
    import torch
    import methyldackel_amd as mdk
    half = LIMIT // 2
    m, u = [[1, half], [2, half], [3, 5]], [[1, 0], [1, 0], [1, 1]]
    with pytest.raises(mdk.MdkError, match=r"pooled margin.*\(site 1\)"):
        mdk.diff_counts(on_device(m, torch.int32), on_device(u, torch.int32), [0, 1], [2])
    # sample 1 not used: its entries -- a negative one among them -- are not looked at
    m[1][0] = -5
    got = mdk.diff_counts(on_device(m, torch.int32), on_device(u, torch.int32), [0], [2])
    assert same(got, expected(m, u, [0], [2]))


def test_strided_and_transposed_matrices_are_refused():
    """the kernel reads [S, n] sample-major: any other layout would give other entries"""
    import torch
    import methyldackel_amd as mdk
    m, u = matrices(6, 3, seed=9)
    dm, du = on_device(m, torch.int32), on_device(u, torch.int32)
    square = on_device(matrices(3, 3, seed=9)[0], torch.int32)
    for bad, good in ((dm[:, ::2], du[:, ::2].contiguous()), (square.t(), square.clone()), (dm[::2], du[::2].contiguous())):
        assert not bad.is_contiguous()
        with pytest.raises(mdk.MdkError, match="nmeth must be contiguous"):
            mdk.diff_counts(bad, good, [0], [1])
        with pytest.raises(mdk.MdkError, match="nunmeth must be contiguous"):
            mdk.diff_counts(good, bad, [0], [1])
        assert same(mdk.diff_counts(bad.contiguous(), good, [0], [1]), expected(bad.cpu().tolist(), good.cpu().tolist(), [0], [1]))


def cohort():
    """three samples over one universe of sites, united: hand-made Calls, no BAM"""
    import torch
    import methyldackel_amd as mdk
    from merge_rule import COLUMNS
    from unite_rule import CONTIGS, sample
    samples = [mdk.Calls(list(CONTIGS), {n: torch.from_numpy(c.copy()).cuda() for n, c in zip(COLUMNS, sample(513, s))}) for s in range(3)]
    return mdk.unite(samples, min_samples=2), mdk


def test_cohort_diff_select_rows_write(tmp_path):
    import torch
    co, mdk = cohort()
    assert len(co) > 100
    d = co.diff([0], [2, 1])
    assert isinstance(d, mdk.Diff) and len(d) == len(co) and d.contigs == co.contigs and d.merged == co.merged
    for name in ("contig", "start", "end", "context", "strand"):
        assert getattr(d, name) is getattr(co, name), name
    want = expected(co.nmeth.cpu().tolist(), co.nunmeth.cpu().tolist(), [0], [1, 2])
    assert same([getattr(d, n) for n in NAMES], want)
    rows = d.rows()
    assert [r[5:] for r in rows] == list(zip(*want)) and rows[0][0] == co.contigs[int(co.contig[0])]
    mask = d.pvalue < 0.5
    s = d.select(mask)
    assert 0 < len(s) < len(d) and s.rows() == [r for r, k in zip(rows, mask.cpu().tolist()) if k] and s.merged == d.merged
    path = d.write(str(tmp_path / "diff.tsv"))
    back = [l.rstrip("\n").split("\t") for l in open(path)]
    assert [tuple([r[0]] + [int(x) for x in r[1:9]] + [bits(float(x)) for x in r[9:]]) for r in back] == [r[:9] + (bits(r[9]), bits(r[10])) for r in rows]
    with pytest.raises(mdk.MdkError, match="both groups"):
        co.diff([0, 1], [1])


def test_qvalue_is_benjamini_hochberg():
    import torch
    co, mdk = cohort()
    d = co.diff([0, 1], [2])
    p = d.pvalue.cpu().tolist()
    assert len(set(p)) < len(p)                                    # ties: sites without a choice have p = 1.0
    q = d.qvalue()
    assert q.dtype == torch.float64 and q.device == d.pvalue.device and q.shape == d.pvalue.shape
    assert [bits(x) for x in q.cpu().tolist()] == [bits(x) for x in bh(p)]
    one = d.select(slice(0, 1))
    assert one.qvalue().cpu().tolist() == one.pvalue.cpu().tolist()
    assert len(d.select(slice(0, 0)).qvalue()) == 0


def test_regions_sums_stacked():
    """the tile form: per-sample Regions sums stacked into int64 matrices"""
    import torch
    co, mdk = cohort()
    lengths = [int(co.end[co.contig == c].max()) if bool((co.contig == c).any()) else 0 for c in range(len(co.contigs))]
    tiles = mdk.Intervals.windows(lengths, 50, contigs=co.contigs)
    per = [co.sample(i).regions(tiles) for i in range(co.n_samples)]
    m, u = torch.stack([r.nmeth for r in per]), torch.stack([r.nunmeth for r in per])
    assert m.dtype == torch.int64 and m.shape == (3, len(tiles))
    assert same(mdk.diff_counts(m, u, [1], [0, 2]), expected(m.cpu().tolist(), u.cpu().tolist(), [1], [0, 2]))
