"""GPU: significant neighbouring sites joined into regions on the device (k_dmr_* of csrc/mdk_dmr.hip) -- Diff.dmrs and its Dmrs.  Every
comparison is exact, the doubles as their 64-bit patterns: against the Python restatement of the rule (tests/dmr_rule.py), which
tests/test_dmr_cpu.py holds against the host build of the same header.  The Diffs are hand-built from lists: nothing here depends on
unite or diff but the last test."""
import re

import pytest

from diff_rule import LIMIT, bh, bits
from dmr_rule import CONTIGS, HAND, MESSAGES, PARAMS, SIMPSON, SIZES, census, dmrs, refusal_tables, site, table, UP, DOWN

pytestmark = pytest.mark.gpu
ROW_NAMES = ("contig", "start", "end", "nmeth_a", "nunmeth_a", "nmeth_b", "nunmeth_b")


def diff_of(rows, contigs=CONTIGS):
    """a Diff on the device from (contig, start, end, a, b, c, d) tuples; its two doubles are NaN: the rule reads neither"""
    import torch
    import methyldackel_amd as mdk
    types = dict(mdk.Diff.COLUMNS)
    cols = {n: torch.tensor([r[k] for r in rows], dtype=getattr(torch, types[n])).cuda() for k, n in enumerate(ROW_NAMES)}
    for n, dt in mdk.Diff.COLUMNS:
        if n not in cols:
            cols[n] = torch.full((len(rows),), float("nan") if dt == "float64" else 0, dtype=getattr(torch, dt)).cuda()
    return mdk.Diff(list(contigs), cols)


def mask_of(sig):
    import torch
    return torch.tensor([bool(s) for s in sig], dtype=torch.bool).cuda()


def exact(r):
    """a region with its doubles as patterns"""
    return tuple(r[:10]) + (bits(r[10]), bits(r[11]))


def on_device(rows, sig, contigs=CONTIGS, **params):
    """Diff.dmrs of the table: the Dmrs, and its regions as exact tuples with the contig as an index"""
    import torch
    import methyldackel_amd as mdk
    d = diff_of(rows, contigs)
    r = d.dmrs(mask_of(sig), **params)
    assert isinstance(r, mdk.Dmrs) and r.contigs == list(contigs)
    for name, dt in mdk.DMR_COLUMNS:
        t = getattr(r, name)
        assert t.dtype == getattr(torch, dt) and t.shape == (len(r),) and t.is_contiguous() and t.device == d.start.device, name
    return r, [exact((list(contigs).index(x[0]),) + x[1:]) for x in r.rows()]


def check(rows, sig, contigs=CONTIGS, **params):
    """the device against the rule; returns the rule's regions"""
    want = dmrs(rows, sig, len(contigs), **params)
    assert on_device(rows, sig, contigs, **params)[1] == [exact(w) for w in want]
    return want


def line(n, step=10, counts=UP):
    """n rows on one contig, `step` bases apart, all of one kind"""
    return [site(0, 5 + step * i, *counts) for i in range(n)]


# first in the file: the kernels' first execution
@pytest.mark.parametrize("n", SIZES)
def test_sizes(n):
    """the seeded tables test_dmr_cpu.py checks against the host build, under four sets of parameters; the inputs as they were after
    the call"""
    import torch
    rows, sig = table(n)
    if n > 1:
        got = census(rows, sig, len(CONTIGS), **PARAMS)
        assert got["kept2"] >= 2 and got["by_min_sites"] >= 1 and got["by_min_diff"] >= 1, got
    d, mask = diff_of(rows), mask_of(sig)
    keep = {name: getattr(d, name).clone() for name, _ in d.COLUMNS}
    keep_mask = mask.clone()
    for params in (PARAMS, dict(PARAMS, min_sites=1), dict(PARAMS, max_skip=0, min_diff=0.0), dict(max_gap=40, max_skip=3, min_sites=3, min_diff=35.0)):
        r = d.dmrs(mask, **params)
        want = dmrs(rows, sig, len(CONTIGS), **params)
        assert [exact((CONTIGS.index(x[0]),) + x[1:]) for x in r.rows()] == [exact(w) for w in want], params
        for name, _ in r.COLUMNS:
            t = getattr(r, name)
            assert t.is_contiguous() and t.device == mask.device and t.shape == (len(want),)
    assert torch.equal(mask, keep_mask)
    for name, t in keep.items():
        assert torch.equal(getattr(d, name).view(torch.uint8 if t.dtype == torch.float64 else t.dtype), t.view(torch.uint8 if t.dtype == torch.float64 else t.dtype)), name


@pytest.mark.parametrize("n,at", [(130, 63), (300, 255)], ids=["63|64", "255|256"])
def test_a_chain_across_a_wavefront_and_a_workgroup(n, at):
    rows = line(n)
    sig = [i in (at, at + 1) for i in range(n)]
    want = check(rows, sig, max_gap=10, max_skip=0, min_sites=2, min_diff=0.0)
    assert [w[:6] for w in want] == [(0, rows[at][1], rows[at + 1][2], 2, 2, 1)]


@pytest.mark.parametrize("n,p,i", [(600, 511, 512), (600, 500, 530), (1100, 100, 1000)], ids=["511|512", "500..530", "100..1000"])
def test_a_chain_across_workgroups_over_skipped_rows(n, p, i):
    """the previous candidate comes from the block table: the block before, and past whole blocks without a candidate"""
    rows = line(n, step=1)
    sig = [k in (p, i) for k in range(n)]
    want = check(rows, sig, max_gap=5000, max_skip=2000, min_sites=2, min_diff=0.0)
    assert [w[:6] for w in want] == [(0, rows[p][1], rows[i][2], i - p + 1, 2, 1)]
    if i > p + 1:                                           # one skipped row fewer allowed: two regions
        assert [w[3] for w in check(rows, sig, max_gap=5000, max_skip=i - p - 2, min_sites=1, min_diff=0.0)] == [1, 1]


def test_a_region_over_more_than_three_whole_blocks():
    """rows 100 .. 1198, a candidate every third row: blocks 1, 2 and 3 come as prefix differences, rows 100 .. 255 and 1024 .. 1198 are
    read; the rows alternate in depth so that a wrong row shows in the sums"""
    n = 1300
    rows = [site(0, 5 + 2 * i, (2 + i % 5, 8), (8 + i % 3, 2)) for i in range(n)]
    sig = [100 <= i <= 1198 and (i - 100) % 3 == 0 for i in range(n)]
    want = check(rows, sig, max_gap=6, max_skip=2, min_sites=3, min_diff=0.0)
    assert [w[:6] for w in want] == [(0, rows[100][1], rows[1198][2], 1099, 367, 1)]
    assert want[0][6] == sum(r[3] for r in rows[100:1199]) and want[0][9] == sum(r[6] for r in rows[100:1199])
    # and from a block's first row to a block's last: no partial end at all
    sig = [256 <= i <= 1023 for i in range(n)]
    assert [w[3:5] for w in check(rows, sig, max_gap=6, max_skip=0, min_sites=3, min_diff=0.0)] == [(768, 768)]


def test_regions_at_row_0_and_at_the_last_row():
    for n in (70, 256, 257):
        rows = line(n)
        sig = [i < 3 or i >= n - 3 for i in range(n)]
        want = check(rows, sig, max_gap=10, max_skip=0, min_sites=3, min_diff=0.0)
        assert [w[1:5] for w in want] == [(rows[0][1], rows[2][2], 3, 3), (rows[n - 3][1], rows[n - 1][2], 3, 3)]


def test_no_candidate_at_all():
    import torch
    rows = line(300)
    for sig in ([False] * 300, None):
        if sig is None:                                     # every row significant, none a candidate: equal fractions
            rows, sig = line(300, counts=((5, 5), (5, 5))), [True] * 300
        r, got = on_device(rows, sig, max_gap=10, max_skip=0, min_sites=1, min_diff=0.0)
        assert got == [] and len(r) == 0 and r.pvalue.dtype == torch.float64 and r.pvalue.device.type == "cuda"
    # no row at all: no launch
    r, got = on_device([], [], max_gap=10, max_skip=0, min_sites=1, min_diff=0.0)
    assert got == [] and len(r) == 0 and r.direction.dtype == torch.int8 and r.direction.device.type == "cuda"


def test_every_row_a_candidate_in_one_region_and_every_row_its_own():
    rows = line(600, counts=DOWN)
    sig = [True] * 600
    want = check(rows, sig, max_gap=10, max_skip=0, min_sites=600, min_diff=0.0)
    assert [w[:6] for w in want] == [(0, rows[0][1], rows[-1][2], 600, 600, -1)]
    want = check(rows, sig, max_gap=0, max_skip=0, min_sites=1, min_diff=0.0)
    assert [w[:6] for w in want] == [(0, r[1], r[2], 1, 1, -1) for r in rows]


@pytest.mark.parametrize("name,rows,sig,params,want", HAND, ids=[h[0] for h in HAND])
def test_chain_breaks_by_hand(name, rows, sig, params, want):
    """a contig change, a direction flip, max_gap and max_skip at their edges, significant rows that are no candidates: each alone"""
    assert [w[:10] for w in check(rows, sig, **params)] == want


def test_the_filter_at_its_edges():
    import struct
    rows, sig = table(257)
    raw = dmrs(rows, sig, len(CONTIGS), 300, 1, 1, 0.0)
    r = next(r for r in raw if r[4] >= 3 and abs(r[10]) > 0.0)
    mine = lambda regions: [w for w in regions if w[:2] == r[:2]]
    assert mine(check(rows, sig, max_gap=300, max_skip=1, min_sites=r[4], min_diff=0.0)) == [r]
    assert mine(check(rows, sig, max_gap=300, max_skip=1, min_sites=r[4] + 1, min_diff=0.0)) == []
    edge = abs(r[10])                                       # the double the rule gives
    above = struct.unpack("<d", struct.pack("<q", bits(edge) + 1))[0]
    assert mine(check(rows, sig, max_gap=300, max_skip=1, min_sites=1, min_diff=edge)) == [r]
    assert mine(check(rows, sig, max_gap=300, max_skip=1, min_sites=1, min_diff=above)) == []


def test_simpson_is_dropped_and_its_sites_alone_are_regions():
    for min_diff in (0.0, 1.0, 40.0):
        assert check(SIMPSON, [1, 1], max_gap=10, max_skip=0, min_sites=1, min_diff=min_diff) == []
    alone = check(SIMPSON, [1, 1], max_gap=0, max_skip=0, min_sites=1, min_diff=0.0)
    assert [w[:10] for w in alone] == [(0, 100, 101, 1, 1, 1, 1, 9, 20, 80), (0, 101, 102, 1, 1, 1, 80, 20, 9, 1)]


def test_agreement_with_diff_counts():
    """a kept region's pvalue and meth_diff are, bit for bit, diff_counts' for a 2 x 1 matrix of its sums"""
    import torch
    import methyldackel_amd as mdk
    rows, sig = table(513)
    r, got = on_device(rows, sig, **PARAMS)
    assert len(r) >= 2
    m, u = torch.stack([r.nmeth_a, r.nmeth_b]), torch.stack([r.nunmeth_a, r.nunmeth_b])
    out = mdk.diff_counts(m, u, [0], [1])
    assert torch.equal(out[4].view(torch.int64), r.meth_diff.view(torch.int64)) and torch.equal(out[5].view(torch.int64), r.pvalue.view(torch.int64))
    assert torch.equal(out[0], r.nmeth_a) and torch.equal(out[3], r.nunmeth_b)
    k = 1
    one = mdk.diff_counts(m[:, k:k + 1].contiguous(), u[:, k:k + 1].contiguous(), [0], [1])
    assert bits(float(one[5][0])) == got[k][11] and bits(float(one[4][0])) == got[k][10]


@pytest.mark.parametrize("name,rows,sig,bit,first", refusal_tables(), ids=[r[0] for r in refusal_tables()])
def test_refusals_name_the_first_row(name, rows, sig, bit, first):
    """each refused condition alone, at row 300 of 513 and again behind it: rc -3, the message, the first row that has it (of a region:
    its first row); the call after a refused one is as any other"""
    import methyldackel_amd as mdk
    d, mask = diff_of(rows), mask_of(sig)
    for params in (PARAMS, dict(PARAMS, min_sites=100)):
        with pytest.raises(mdk.MdkError, match=re.escape(MESSAGES[bit]) + rf".*\(row {first}\)") as e:
            d.dmrs(mask, **params)
        assert e.value.rc == -3
    rows, sig = table(257)
    want = dmrs(rows, sig, len(CONTIGS), **PARAMS)
    good = diff_of(rows)
    good._text = d._text                                    # the refused call's own renderer
    assert [exact((CONTIGS.index(x[0]),) + x[1:]) for x in good.dmrs(mask_of(sig), **PARAMS).rows()] == [exact(w) for w in want]


def test_just_inside_the_bounds_is_accepted():
    rows = [site(0, 10, (LIMIT // 2 - 3, 0), (3, 5)), site(0, 11, (LIMIT // 2 - 4, 0), (3, 5)), site(1, 5, (0, LIMIT - 1), (1, 0))]
    want = check(rows, [1, 1, 1], max_gap=10, max_skip=0, min_sites=1, min_diff=0.0)
    assert [w[:10] for w in want] == [(0, 10, 12, 2, 2, -1, LIMIT - 7, 0, 6, 10), (1, 5, 6, 1, 1, 1, 0, LIMIT - 1, 1, 0)]


def test_arguments_refused_on_the_device():
    import torch
    import methyldackel_amd as mdk
    d = diff_of(line(6))
    mask = mask_of([1] * 6)
    with pytest.raises(mdk.MdkError, match="significant is a cpu tensor"):
        d.dmrs(mask.cpu())
    with pytest.raises(mdk.MdkError, match="significant must be contiguous"):
        d.dmrs(mask_of([1] * 12)[::2])
    with pytest.raises(mdk.MdkError, match="significant has the shape"):
        d.dmrs(mask[:5])
    with pytest.raises(mdk.MdkError, match="torch.bool"):
        d.dmrs(mask.to(torch.uint8))
    d.nmeth_b = torch.stack([d.nmeth_b, d.nmeth_b], 1)[:, 0]
    assert not d.nmeth_b.is_contiguous()
    with pytest.raises(mdk.MdkError, match="nmeth_b column must be a contiguous int64"):
        d.dmrs(mask)
    d.nmeth_b = d.nmeth_b.contiguous().to(torch.int32)
    with pytest.raises(mdk.MdkError, match="nmeth_b column must be a contiguous int64"):
        d.dmrs(mask)


def test_select_rows_write_qvalue(tmp_path):
    import torch
    rows, sig = table(513)
    r, got = on_device(rows, sig, **dict(PARAMS, min_sites=1))
    assert len(r) > 8
    host = r.rows()
    assert [x[0] for x in host] == [CONTIGS[g[0]] for g in got] and r.merged is False
    path = r.write(str(tmp_path / "dmr.tsv"))
    back = [l.rstrip("\n").split("\t") for l in open(path)]
    assert [tuple([b[0]] + [int(x) for x in b[1:10]] + [bits(float(x)) for x in b[10:]]) for b in back] == [x[:10] + (bits(x[10]), bits(x[11])) for x in host]
    keep = r.direction > 0
    s = r.select(keep)
    assert 0 < len(s) < len(r) and s.rows() == [x for x, k in zip(host, keep.cpu().tolist()) if k] and s.contigs == r.contigs
    assert (r.end - r.start).min() >= 1 and len(r.select((r.end - r.start) >= 100)) < len(r)
    q = r.qvalue()
    assert q.dtype == torch.float64 and q.device == r.pvalue.device and q.shape == r.pvalue.shape
    assert [bits(x) for x in q.cpu().tolist()] == [bits(x) for x in bh([x[11] for x in host])]


def test_diff_qvalue_is_unchanged():
    """Diff.qvalue now shares its body with Dmrs.qvalue: the case of tests/test_gpu_diff.py, ties among its p-values"""
    import torch
    import methyldackel_amd as mdk
    from merge_rule import COLUMNS
    from unite_rule import CONTIGS as NAMES, sample
    samples = [mdk.Calls(list(NAMES), {n: torch.from_numpy(c.copy()).cuda() for n, c in zip(COLUMNS, sample(513, s))}) for s in range(3)]
    d = mdk.unite(samples, min_samples=2).diff([0, 1], [2])
    p = d.pvalue.cpu().tolist()
    assert len(set(p)) < len(p)
    assert [bits(x) for x in d.qvalue().cpu().tolist()] == [bits(x) for x in bh(p)]
    assert len(d.select(slice(0, 0)).qvalue()) == 0
    # ... and the regions of the same table go through the same helper
    r = d.dmrs(d.pvalue < 0.5, max_gap=1000, max_skip=3, min_sites=1)
    assert len(r) > 1 and [bits(x) for x in r.qvalue().cpu().tolist()] == [bits(x) for x in bh(r.pvalue.cpu().tolist())]


def test_intervals_fed_to_calls_regions():
    """a sample's own sums over the DMRs: every row of a span is counted, the rows between the regions are not"""
    import torch
    import methyldackel_amd as mdk
    rows = [site(0, 10, *UP), site(0, 12, *DOWN), site(0, 14, *UP), site(0, 40, *UP), site(1, 3, *DOWN), site(1, 4, *DOWN), site(1, 9, *UP)]
    sig = [1, 0, 1, 0, 1, 1, 0]
    r, got = on_device(rows, sig, max_gap=5, max_skip=1, min_sites=2, min_diff=0.0)
    assert [g[:6] for g in got] == [(0, 10, 15, 3, 2, 1), (1, 3, 5, 2, 2, -1)]
    iv = r.intervals()
    assert isinstance(iv, mdk.Intervals) and iv.contig is r.contig and iv.start is r.start and iv.end is r.end and iv.contigs == r.contigs
    n = len(rows)
    calls = mdk.Calls(list(CONTIGS), {"contig": torch.tensor([x[0] for x in rows], dtype=torch.int32).cuda(), "start": torch.tensor([x[1] for x in rows], dtype=torch.int32).cuda(),
                                      "end": torch.tensor([x[2] for x in rows], dtype=torch.int32).cuda(), "nmeth": torch.arange(1, n + 1, dtype=torch.int32).cuda(),
                                      "nunmeth": torch.full((n,), 2, dtype=torch.int32).cuda(), "context": torch.zeros(n, dtype=torch.uint8).cuda(), "strand": torch.ones(n, dtype=torch.int8).cuda()})
    sums = calls.regions(iv)
    assert sums.rows() == [("chr1", 10, 15, 3, 1 + 2 + 3, 6), ("chr2", 3, 5, 2, 5 + 6, 4)]


def test_unite_diff_dmrs_end_to_end():
    """three hand-built Calls united, two groups compared, the significant sites joined: against the rule applied to the Diff's own columns"""
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
    co = mdk.unite([calls(lambda i: 0.5, 30), calls(hyper, 40), calls(hyper, 25)])
    d = co.diff([0], [1, 2])
    q = d.qvalue()
    significant = q < 0.05
    r = d.dmrs(significant, max_gap=8, max_skip=1, min_sites=3, min_diff=20.0)
    rows = list(zip(*[getattr(d, n).cpu().tolist() for n in ROW_NAMES]))
    want = dmrs(rows, significant.cpu().tolist(), 2, 8, 1, 3, 20.0)
    assert [exact((r.contigs.index(x[0]),) + x[1:]) for x in r.rows()] == [exact(w) for w in want]
    assert [w[5] for w in want] == [1, -1] and r.merged and want[0][1] >= starts[5] and want[1][2] <= starts[31] + 2
    per_sample = [co.sample(i).regions(r.intervals()) for i in range(3)]
    assert sum(int(s.nmeth[0]) for s in per_sample[1:]) == want[0][8] and int(per_sample[0].nmeth[0]) == want[0][6]
