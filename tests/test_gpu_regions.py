"""GPU: sums of rows over intervals on the device (k_region_rows / k_region_blocks / k_region_sum, csrc/mdk_regions.hip) -- Calls.regions and
Cytosines.regions.  Every comparison is exact: against the Python restatement of the rule (tests/region_rule.py), against the torch
formulation (a key per row, searchsorted, cumsum) on the device, and on a session's own result."""
import pytest

from merge_rule import COLUMNS, DTYPES, SIZES, table
from region_rule import BIG, CONTIGS, ERRORS, FILTERS, KS, MESSAGES, SCAN_N, expected, intervals, region_sums, scan_expected, scan_intervals

pytestmark = pytest.mark.gpu


def calls_of(columns, contigs=CONTIGS):
    """a Calls of numpy columns or of (contig, start, end, nmeth, nunmeth, context, strand) tuples, on the device: no BAM"""
    import numpy as np
    import torch
    import methyldackel_amd as mdk
    if not (len(columns) and isinstance(columns[0], np.ndarray)):
        columns = [np.array([r[k] for r in columns], dtype=dt) for k, dt in enumerate(DTYPES)]
    return mdk.Calls(list(contigs), {n: torch.from_numpy(c.copy()).cuda() for n, c in zip(COLUMNS, columns)})


def intervals_of(ivs, contigs=CONTIGS, device="cpu"):
    import torch
    import methyldackel_amd as mdk
    return mdk.Intervals(list(contigs), *[torch.tensor([r[k] for r in ivs], dtype=torch.int32, device=device) for k in range(3)])


def same(r, want):
    """is the Regions' result exactly the restatement's list of (nsites, nmeth, nunmeth)?"""
    import torch
    return len(r) == len(want) and all(torch.equal(getattr(r, name).cpu(), torch.tensor([w[k] for w in want], dtype=dt))
                                       for k, (name, dt) in enumerate((("nsites", torch.int32), ("nmeth", torch.int64), ("nunmeth", torch.int64))))


def numpy_columns(c):
    return [getattr(c, n).cpu().numpy() for n in COLUMNS]


# first in the file: the kernels' first execution
@pytest.mark.parametrize("n", SIZES)
def test_blocking_on_the_device(n):
    """every table with every number of intervals, and the largest set with every filter"""
    import torch
    c = calls_of(list(table(n)))
    for k in KS:
        iv = intervals_of(intervals(n, k))
        r = c.regions(iv)
        assert r.contigs == c.contigs and len(r) == k
        for name, dt in (("contig", torch.int32), ("start", torch.int32), ("end", torch.int32), ("nsites", torch.int32), ("nmeth", torch.int64), ("nunmeth", torch.int64)):
            t = getattr(r, name)
            assert t.dtype == dt and t.device == c.start.device and t.is_contiguous() and t.shape == (k,), name
        assert all(torch.equal(getattr(r, name).cpu(), getattr(iv, name)) for name in ("contig", "start", "end"))          # the intervals' own order
        assert same(r, expected(n, k)), (n, k)
    k = KS[-1]
    iv = intervals_of(intervals(n, k), device="cuda")
    kept = [t.clone() for t in (iv.contig, iv.start, iv.end)]
    for ctx, strand, depth in FILTERS:
        r = c.regions(iv, contexts=ctx, strand=strand, min_depth=depth)
        assert same(r, expected(n, k, ctx, strand, depth)), (n, ctx, strand, depth)
        assert r.start.data_ptr() == iv.start.data_ptr()                      # intervals on the device are not copied
    assert same(c.regions(iv, contexts=("CHH", "CpG"), strand="-", min_depth=5), region_sums(table(n), intervals(n, k), (0, 2), "-", 5))
    # the inputs are as they were
    assert all(torch.equal(getattr(c, name).cpu(), torch.from_numpy(col.copy())) for name, col in zip(COLUMNS, table(n)))
    assert all(torch.equal(a, b) for a, b in zip(kept, (iv.contig, iv.start, iv.end)))


def test_second_round_of_the_block_scan():
    """more than 4096 blocks of 256 rows: the prefix entries behind the first round of k_region_blocks hold its carry"""
    c = calls_of(list(table(SCAN_N)))
    iv = intervals_of(scan_intervals(), device="cuda")
    for f in ((None, None, 1), ((0,), "-", 5), ((2,), "+", 0)):
        assert same(c.regions(iv, contexts=f[0], strand=f[1], min_depth=f[2]), scan_expected(*f)), f
    assert scan_expected()[-2][0] > 256 * 1024


def test_torch_formulation_agrees():
    """a second oracle at n = 300001: a 64-bit key per row, searchsorted, three cumsums of filtered int64 columns, in torch on the device"""
    import torch
    n, k = SIZES[-1], KS[-1]
    c = calls_of(list(table(n)))
    iv = intervals_of(intervals(n, k), device="cuda")
    key = (c.contig.to(torch.int64) << 32) | c.start.to(torch.int64)
    lo = torch.searchsorted(key, (iv.contig.to(torch.int64) << 32) | iv.start.to(torch.int64))
    hi = torch.searchsorted(key, (iv.contig.to(torch.int64) << 32) | iv.end.to(torch.int64))
    for ctx, strand, depth in ((None, None, 1), ((0,), "+", 5), ((2,), "-", 0)):
        ok = (c.nmeth.to(torch.int64) + c.nunmeth >= depth)
        if ctx is not None:
            ok &= c.context == ctx[0]
        if strand is not None:
            ok &= (c.strand > 0) if strand == "+" else (c.strand < 0)
        r = c.regions(iv, contexts=ctx, strand=strand, min_depth=depth)
        for got, col in ((r.nsites.to(torch.int64), ok.to(torch.int64)), (r.nmeth, ok * c.nmeth.to(torch.int64)), (r.nunmeth, ok * c.nunmeth.to(torch.int64))):
            pre = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(col, 0)])
            assert torch.equal(got, pre[hi] - pre[lo]), (ctx, strand, depth)


@pytest.mark.parametrize("n", [513, 300001])
def test_a_merged_table(n):
    """strand-0 rows and rows wider than a base: a row belongs to the interval that holds its start.  The merged rows of one context, or
    of one context and CHH, are strictly ascending.  CpG and CHG rows together need not be: in CGG the CpG site and the lone site of the
    second G, which the command calls a CHG G, both start at the C -- such a table is refused like any other that is not ascending"""
    import numpy as np
    import torch
    import methyldackel_amd as mdk
    from region_rule import intervals_over
    m = calls_of(list(table(n))).merge_context(0)
    assert int((m.strand == 0).sum()) > 0 and int((m.end - m.start > 1).sum()) > 0
    for keep in ((0,), (1,), (0, 2), (1, 2)):
        t = m.select(torch.isin(m.context, torch.tensor(keep, dtype=torch.uint8, device="cuda")))
        cols = numpy_columns(t)
        assert int((t.strand == 0).sum()) > 0 and int((t.end - t.start > 1).sum()) > 0
        ivs = intervals_over(cols, 257 if n > 1000 else 65)
        for ctx in (None,) + tuple((x,) for x in keep):
            for depth in (0, 1, 5):
                assert same(t.regions(intervals_of(ivs), contexts=ctx, min_depth=depth), region_sums(cols, ivs, ctx, None, depth)), (keep, ctx, depth)
        # strand "+" leaves only the CHH rows of a merged table
        assert same(t.regions(intervals_of(ivs), strand="+"), region_sums(cols, ivs, None, "+", 1))
    cols = numpy_columns(m)
    key = cols[0].astype(np.int64) << 32 | cols[1]
    ivs = intervals_over(cols, 65)
    if (np.diff(key) <= 0).any():
        assert (np.diff(key) >= 0).all()                    # two sites with one start, never a start below the one before
        with pytest.raises(mdk.MdkError, match="not ascending"):
            m.regions(intervals_of(ivs))
    else:
        assert same(m.regions(intervals_of(ivs)), region_sums(cols, ivs))


def test_a_tiling_adds_up_to_the_table():
    import torch
    import methyldackel_amd as mdk
    n = SIZES[-1]
    cols = table(n)
    c = calls_of(list(cols))
    lengths = [int(cols[1][cols[0] == t].max()) + 1 if (cols[0] == t).any() else 10 for t in range(len(CONTIGS))]
    for width, (ctx, strand, depth) in ((100, (None, None, 1)), (1000, ((0,), "-", 5)), (37, ((2,), None, 0))):
        r = c.regions(mdk.Intervals.windows(lengths, width, contigs=CONTIGS), contexts=ctx, strand=strand, min_depth=depth)
        whole = region_sums(cols, [(t, 0, BIG) for t in range(len(CONTIGS))], ctx, strand, depth)
        assert len(r) == sum((x + width - 1) // width for x in lengths)
        assert (int(r.nsites.sum()), int(r.nmeth.sum()), int(r.nunmeth.sum())) == tuple(sum(w[k] for w in whole) for k in range(3))
        assert int(r.nsites.sum()) > 1000
    # sliding windows count a row width / step = 4 times; only a row below 75 lies in fewer (3 + 2 + 1 missing per 25 bases: at most 150 a contig)
    r = c.regions(mdk.Intervals.windows(lengths, 100, step=25, contigs=CONTIGS), min_depth=0)
    assert n * 4 - 150 * len(CONTIGS) <= int(r.nsites.sum()) < n * 4 and r.nsites.dtype == torch.int32


def test_counts_past_int32():
    c = calls_of([(0, k, k + 1, BIG, BIG, 0, 1) for k in range(3)])
    r = c.regions(intervals_of([(0, 0, 3), (0, 1, 2), (0, 3, 9)]), min_depth=BIG)
    assert same(r, [(3, 3 * BIG, 3 * BIG), (1, BIG, BIG), (0, 0, 0)])
    assert r.rows() == [("c0", 0, 3, 3, 3 * BIG, 3 * BIG), ("c0", 1, 2, 1, BIG, BIG), ("c0", 3, 9, 0, 0, 0)]


@pytest.mark.parametrize("name,rows,ivs", ERRORS, ids=[f"{e[0]}{i}" for i, e in enumerate(ERRORS)])
def test_refusals(name, rows, ivs):
    """each refusal with rc -3 and its message: alone, and (rows) as rows 255 / 256 of a longer table, where the faulty row's neighbour
    belongs to another workgroup; the renderer goes on working"""
    import methyldackel_amd as mdk
    tables = [rows]
    if name in ("order", "context"):
        pad = [(0, k, k + 1, 1, 1, 2, 1) for k in range(256 - len(rows) + 1)]
        tables.append(pad + [(c, a + 1000, b + 1000, m, u, t, s) for c, a, b, m, u, t, s in rows])
    for tab in tables:
        c = calls_of(tab, ("a", "b"))
        with pytest.raises(mdk.MdkError, match=MESSAGES[name]) as e:
            c.regions(intervals_of(ivs, ("a", "b")))
        assert e.value.rc == -3
    good = calls_of([(0, 10, 11, 1, 1, 2, 1), (1, 0, 1, 1, 1, 0, -1)], ("a", "b"))
    good._text = c._text
    assert same(good.regions(intervals_of([(0, 0, 100), (1, 0, 0), (1, BIG, BIG)], ("a", "b"))), [(1, 1, 1), (0, 0, 0), (0, 0, 0)])


def test_cytosines():
    """a hand-built report: min_depth 0 counts the cytosines of an interval, min_depth 1 the covered ones"""
    import torch
    import methyldackel_amd as mdk
    # (contig, pos 1-based, strand, nmeth, nunmeth, context)
    rep = [(0, 3, 1, 0, 0, 0), (0, 4, -1, 2, 1, 0), (0, 9, 1, 0, 0, 2), (0, 10, 1, 4, 4, 1), (1, 1, -1, 0, 3, 2), (1, 7, 1, 0, 0, 0)]
    cols = {"contig": torch.tensor([r[0] for r in rep], dtype=torch.int32), "pos": torch.tensor([r[1] for r in rep], dtype=torch.int32),
            "strand": torch.tensor([r[2] for r in rep], dtype=torch.int8), "nmeth": torch.tensor([r[3] for r in rep], dtype=torch.int32),
            "nunmeth": torch.tensor([r[4] for r in rep], dtype=torch.int32), "context": torch.tensor([r[5] for r in rep], dtype=torch.uint8),
            "trinucleotide": torch.full((len(rep), 3), 67, dtype=torch.uint8)}
    y = mdk.Cytosines(["a", "b"], {k: v.cuda() for k, v in cols.items()})
    iv = intervals_of([(0, 0, 10), (0, 2, 3), (0, 3, 4), (1, 0, 100), (0, 9, 10)], ("a", "b"))
    assert same(y.regions(iv), [(4, 6, 5), (1, 0, 0), (1, 2, 1), (2, 0, 3), (1, 4, 4)])                       # pos 3 is the base [2, 3)
    assert same(y.regions(iv, min_depth=1), [(2, 6, 5), (0, 0, 0), (1, 2, 1), (1, 0, 3), (1, 4, 4)])
    assert same(y.regions(iv, contexts=("CpG",), strand="+"), [(1, 0, 0), (1, 0, 0), (0, 0, 0), (1, 0, 0), (0, 0, 0)])
    assert torch.equal(y.pos.cpu(), cols["pos"])


def test_session_result_in_windows(small_synth, tmp_path):
    import methyldackel_amd as mdk
    fa, bam = small_synth / "pe.fa", small_synth / "pe.bam"
    with mdk.Session(0) as s, mdk.Reference(fa) as ref:
        c = s.extract([fa, bam, "--CHG", "--CHH"])
        iv = mdk.Intervals.windows(ref, 1000)
        r = c.regions(iv)
        rows = c.rows()
        want = []
        for t, a, b in zip(iv.contig.tolist(), iv.start.tolist(), iv.end.tolist()):
            sel = [x for x in rows if x[0] == ref.contigs[t] and a <= x[1] < b and x[3] + x[4] >= 1]
            want.append((len(sel), sum(x[3] for x in sel), sum(x[4] for x in sel)))
        assert same(r, want) and len(r) == 60 and sum(w[0] for w in want) == len(c) > 10000
        cpg = c.regions(iv, contexts=("CpG",), min_depth=10)
        assert same(cpg, region_sums(numpy_columns(c), list(zip(iv.contig.tolist(), iv.start.tolist(), iv.end.tolist())), (0,), None, 10))
        assert 0 < int(cpg.nsites.sum()) < int(r.nsites.sum())
        path = r.write(tmp_path / "tiles.tsv")
        assert open(path, "rb").read() == "".join(f"{ref.contigs[t]}\t{a}\t{b}\t{w[0]}\t{w[1]}\t{w[2]}\n" for (t, a, b), w in zip(zip(iv.contig.tolist(), iv.start.tolist(), iv.end.tolist()), want)).encode()
        top = r.select(r.nsites > int(r.nsites.float().mean()))
        assert 0 < len(top) < len(r) and top.rows() == [x for x in r.rows() if x[3] > int(r.nsites.float().mean())]
