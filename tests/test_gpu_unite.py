"""GPU: samples joined into one site table on the device (the k_unite_* kernels of csrc/mdk_unite.hip) -- mdk.unite and its Cohort.
Every comparison is exact: against the Python restatement of the rule (tests/unite_rule.py), against the torch formulation (a key per
row, cat, unique, scatter) on the device, on a session's own results and against its cytosine reports."""
import pytest

from merge_rule import COLUMNS, DTYPES, SIZES
from unite_rule import BIG, CONTIGS, ERROR_CONTIGS, ERRORS, FAR, HAND, MESSAGES, combos, expected, rounds, sample, sample_rows, unite_rows

pytestmark = pytest.mark.gpu
SITE = (("contig", "int32"), ("start", "int32"), ("end", "int32"), ("context", "uint8"), ("strand", "int8"), ("nsamples", "int32"))


def calls_of(columns, contigs=CONTIGS, **kw):
    """a Calls of numpy columns or of (contig, start, end, nmeth, nunmeth, context, strand) tuples, on the device: no BAM"""
    import numpy as np
    import torch
    import methyldackel_amd as mdk
    if not (len(columns) and isinstance(columns[0], np.ndarray)):
        columns = [np.array([r[k] for r in columns], dtype=dt) for k, dt in enumerate(DTYPES)]
    return mdk.Calls(list(contigs), {n: torch.from_numpy(c.copy()).cuda() for n, c in zip(COLUMNS, columns)}, **kw)


def numpy_rows(c):
    return list(zip(*[getattr(c, n).cpu().tolist() for n in COLUMNS]))


def same(co, want):
    """is the Cohort exactly the restatement's list of united rows?"""
    import torch
    S = co.n_samples
    ok = len(co) == len(want) and all(torch.equal(getattr(co, name).cpu(), torch.tensor([w[k] for w in want], dtype=getattr(torch, dt))) for k, (name, dt) in enumerate(SITE))
    for k, mat in enumerate((co.nmeth, co.nunmeth)):
        ok = ok and torch.equal(mat.cpu(), torch.tensor([[w[6 + s][k] for w in want] for s in range(S)], dtype=torch.int32).reshape(S, len(want)))
    return bool(ok)


@pytest.fixture(scope="module")
def seeded():
    """the samples of every universe on the device, made once"""
    made = {}

    def get(n, s):
        if (n, s) not in made:
            made[n, s] = calls_of(list(sample(n, s)))
        return made[n, s]
    return get


# first in the file: the kernels' first execution
@pytest.mark.parametrize("n", SIZES)
def test_seeded_tables_on_the_device(n, seeded):
    """every universe with every number of samples, min_samples and min_depth; dtypes, devices, shapes; the inputs as they were"""
    import torch
    import methyldackel_amd as mdk
    for S, k, d in combos(n):
        samples = [seeded(n, s) for s in range(S)]
        co = mdk.unite(samples, min_samples=k, min_depth=d)
        want = expected(n, S, k, d)
        assert same(co, want), (n, S, k, d)
        assert co.n_union == len(expected(n, S, 1, d)) and co.contigs == list(CONTIGS) and co.merged is False and co.contexts_on == (0, 1, 2)
        for name, dt in SITE:
            t = getattr(co, name)
            assert t.dtype == getattr(torch, dt) and t.device == samples[0].start.device and t.is_contiguous() and t.shape == (len(want),), name
        for t in (co.nmeth, co.nunmeth):
            assert t.dtype == torch.int32 and t.device == samples[0].start.device and t.is_contiguous() and t.shape == (S, len(want))
        if n > 1000:
            # more than 16 x 1024 words of bitmap and more than 256 x 1024 sites: k_unite_blocks takes a second round over either table
            assert min(rounds([sample_rows(n, s) for s in range(S)], co.n_union)) >= 2
    assert mdk.unite([seeded(n, 0), seeded(n, 1)]).n_samples == 2          # min_samples defaults to all
    assert same(mdk.unite([seeded(n, 0), seeded(n, 1)]), expected(n, 2, 2, 1))
    for s in range(5):
        assert all(torch.equal(getattr(seeded(n, s), name).cpu(), torch.from_numpy(col.copy())) for name, col in zip(COLUMNS, sample(n, s)))
    if n >= 255:
        for S in (2, 3, 5) if n < 1000 else (3,):
            assert len(expected(n, S, S, 1)) < len(expected(n, S, 1, 1)) and len(expected(n, S, 1, 5)) < len(expected(n, S, 1, 1)), (n, S)


def test_more_samples_than_lanes():
    import methyldackel_amd as mdk
    n, S = 513, 70
    rows = [sample_rows(n, s) for s in range(S)]
    samples = [calls_of(list(sample(n, s))) for s in range(S)]
    for k, d in ((1, 1), (52, 1), (70, 0), (45, 5)):
        assert same(mdk.unite(samples, k, d), unite_rows(rows, k, d)), (k, d)


@pytest.mark.parametrize("n", [1, 257, 513])
def test_one_sample_is_its_own_rows_after_the_depth_cut(n, seeded):
    import methyldackel_amd as mdk
    for d in (0, 1, 5):
        assert same(mdk.unite([seeded(n, 0)], min_depth=d), [(c, p, e, t, s, 1, (m, u)) for c, p, e, m, u, t, s in sample_rows(n, 0) if m + u >= d])


@pytest.mark.parametrize("name,samples,kw", HAND + [FAR], ids=[h[0] for h in HAND + [FAR]])
def test_by_hand(name, samples, kw):
    """the last case needs about 1 GiB of temporaries: bit offsets pass 2^32"""
    import torch
    import methyldackel_amd as mdk
    co = mdk.unite([calls_of(rows) for rows in samples], **kw)
    want = unite_rows(samples, **kw)
    assert same(co, want)
    if name == "all samples empty":
        assert len(co) == 0 and co.n_union == 0 and co.nmeth.shape == (3, 0) and co.nmeth.dtype == torch.int32 and co.start.dtype == torch.int32 and co.context.dtype == torch.uint8
        assert co.rows() == [] and len(co.sample(2)) == 0
    if name == FAR[0]:
        assert len(co) == 4 and co.rows()[2] == ("c1", BIG - 1, BIG, 2, 1, 2, (2, 3), (4, 5))


@pytest.mark.parametrize("name,samples,kw", ERRORS, ids=[f"{e[0]}{i}" for i, e in enumerate(ERRORS)])
def test_refusals(name, samples, kw):
    """each refusal with rc -3 and its message; the renderer goes on working"""
    import methyldackel_amd as mdk
    contigs = [f"c{i}" for i in range(ERROR_CONTIGS.get(name, 2))]
    cs = [calls_of(rows, contigs) for rows in samples]
    with pytest.raises(mdk.MdkError, match=MESSAGES[name]) as e:
        mdk.unite(cs, **kw)
    assert e.value.rc == -3
    good = calls_of([(0, 10, 11, 1, 1, 2, 1), (1, 0, 1, 1, 1, 0, -1)], contigs)
    good._text = cs[0]._text
    assert same(mdk.unite([good, good], min_samples=2), [(0, 10, 11, 2, 1, 2, (1, 1), (1, 1)), (1, 0, 1, 0, -1, 2, (1, 1), (1, 1))])


def test_derived_methods(seeded):
    import numpy as np
    import torch
    import methyldackel_amd as mdk
    from region_rule import intervals_over, region_sums
    n, S = 513, 3
    co = mdk.unite([seeded(n, s) for s in range(S)], min_samples=2)
    want = expected(n, S, 2, 1)
    assert len(co) == len(want) > 100 and co.n_samples == S
    # rows(): the contig by its name
    assert co.rows() == [(CONTIGS[w[0]],) + w[1:] for w in want]
    # sample(i): a view of row i of the matrices over all the sites
    for i in range(S):
        c = co.sample(i)
        assert isinstance(c, mdk.Calls) and len(c) == len(co) and c.contigs == co.contigs
        assert c.nmeth.data_ptr() == co.nmeth[i].data_ptr() and c.nunmeth.data_ptr() == co.nunmeth[i].data_ptr() and c.start.data_ptr() == co.start.data_ptr()
        assert c.nmeth.is_contiguous() and c.nmeth.untyped_storage().data_ptr() == co.nmeth.untyped_storage().data_ptr()
        cols = [np.array([w[k] for w in want], dtype=dt) for k, dt in zip((0, 1, 2), DTYPES)] + [np.array([w[6 + i][k] for w in want], dtype="int32") for k in (0, 1)] + \
               [np.array([w[3] for w in want], dtype="uint8"), np.array([w[4] for w in want], dtype="int8")]
        ivs = intervals_over(cols, 65)
        iv = mdk.Intervals(list(CONTIGS), *[torch.tensor([r[k] for r in ivs], dtype=torch.int32) for k in range(3)])
        for depth in (0, 1):
            r = c.regions(iv, min_depth=depth)
            sums = region_sums(cols, ivs, None, None, depth)
            assert list(zip(r.nsites.tolist(), r.nmeth.tolist(), r.nunmeth.tolist())) == sums, (i, depth)
    with pytest.raises(mdk.MdkError, match="sample 3"):
        co.sample(3)
    # select by mask: along the site axis
    mask = co.nsamples == 3
    sel = co.select(mask)
    assert 0 < len(sel) < len(co) and same(sel, [w for w in want if w[5] == 3]) and sel.nmeth.is_contiguous() and sel.nmeth.shape == (S, len(sel))
    assert same(co.select(slice(5, 40)), list(want[5:40])) and sel.sample(1).nmeth.data_ptr() == sel.nmeth[1].data_ptr()


def test_torch_formulation_agrees(seeded):
    """a second oracle at 300001 x 5: a 64-bit key per row, cat, unique(return_inverse, return_counts), scatter, in torch on the device"""
    import torch
    import methyldackel_amd as mdk
    n, S = SIZES[-1], 5
    samples = [seeded(n, s) for s in range(S)]
    for k, d in ((1, 1), (5, 1), (3, 5), (2, 0)):
        co = mdk.unite(samples, min_samples=k, min_depth=d)
        present = [c.nmeth.to(torch.int64) + c.nunmeth >= d for c in samples]
        keys = torch.cat([((c.contig.to(torch.int64) << 32) | c.start.to(torch.int64))[p] for c, p in zip(samples, present)])
        uniq, inverse, counts = torch.unique(keys, return_inverse=True, return_counts=True)
        keep = counts >= k
        place = torch.cumsum(keep, 0) - 1
        assert len(co) == int(keep.sum()) and co.n_union == len(uniq)
        assert torch.equal((co.contig.to(torch.int64) << 32) | co.start.to(torch.int64), uniq[keep]) and torch.equal(co.nsamples.to(torch.int64), counts[keep])
        at = 0
        for s, (c, p) in enumerate(zip(samples, present)):
            inv = inverse[at:at + int(p.sum())]
            at += int(p.sum())
            for mat, col in ((co.nmeth, c.nmeth), (co.nunmeth, c.nunmeth)):
                row = torch.zeros(len(co), dtype=torch.int32, device="cuda")
                row[place[inv][keep[inv]]] = col[p][keep[inv]]
                assert torch.equal(mat[s], row), (k, d, s)
        assert min(rounds([sample_rows(n, s) for s in range(S)], co.n_union)) >= 2


def dict_join(tables, min_samples):
    """(chrom, start) -> what Calls.rows() gives of it per sample: the united rows' chrom, start, end, nsamples and counts"""
    sites = {}
    for s, rows in enumerate(tables):
        for chrom, a, b, m, u in rows:
            sites.setdefault((chrom, a), {})[s] = (b, m, u)
    return {key: held for key, held in sites.items() if len(held) >= min_samples}


def test_a_real_session(small_synth):
    """three extract results of one session with different row sets -- plain, -q 50, -d 5 --, and -q 40: the sample's MAPQs are 40 to 60
    (2 % below 10, which the default -q 10 drops already), so -q 40 keeps what the plain run keeps, and it takes -q 50 to drop sites"""
    import torch
    import methyldackel_amd as mdk
    fa, bam = small_synth / "pe.fa", small_synth / "pe.bam"
    with mdk.Session(0) as s:
        cs = [s.extract([fa, bam, "--CHG", "--CHH"] + extra) for extra in ([], ["-q", "40"], ["-d", "5"], ["-q", "50"])]
    assert len({len(cs[i]) for i in (0, 2, 3)}) == 3 and min(len(c) for c in cs) > 1000
    order = {name: i for i, name in enumerate(cs[0].contigs)}
    for k in (1, 3, 4):
        co = mdk.unite(cs, min_samples=k)
        want = dict_join([c.rows() for c in cs], k)
        got = co.rows()
        assert len(got) == len(want) and [(r[0], r[1]) for r in got] == sorted(want, key=lambda key: (order[key[0]], key[1]))
        for r in got:
            held = want[r[0], r[1]]
            assert r[5] == len(held) and all(r[6 + i] == (held[i][1:] if i in held else (0, 0)) for i in range(4)) and all(h[0] == r[2] for h in held.values())
        assert same(co, unite_rows([numpy_rows(c) for c in cs], k))
    assert len(mdk.unite(cs, min_samples=4)) < len(mdk.unite(cs, min_samples=3)) < len(mdk.unite(cs, min_samples=1))
    # the merged rows, context by context: CpG and CHG rows merged into one table are not ascending (a CGG holds two sites at one start)
    ms = [c.merge_context() for c in cs]
    for ctx in (0, 1, 2):
        per = [m.select(m.context == ctx) for m in ms]
        for k in (1, 3, 4):
            co = mdk.unite(per, min_samples=k)
            assert co.merged is True and same(co, unite_rows([numpy_rows(c) for c in per], k)) and len(co) > 100
            if ctx < 2:
                assert bool((co.strand == 0).all()) and bool((co.end - co.start == ctx + 2).all())
    with pytest.raises(mdk.MdkError, match="merged"):
        mdk.unite([cs[0], ms[0]])


def test_counts_are_the_cytosine_reports(small_synth):
    """two samples united at min_samples 1, min_depth 0: at every site both reports list, the counts are the reports' own"""
    import methyldackel_amd as mdk
    fa, bam = small_synth / "pe.fa", small_synth / "pe.bam"
    args = [[fa, bam, "--CHG", "--CHH"], [fa, bam, "--CHG", "--CHH", "-q", "50"]]
    with mdk.Session(0) as s:
        cs = [s.extract(a) for a in args]
        reports = [{(r[0], r[1]): r for r in s.cytosine_report(a).rows()} for a in args]
    co = mdk.unite(cs, min_samples=1, min_depth=0)
    both = [r for r in co.rows() if all((r[0], r[1] + 1) in rep for rep in reports)]
    assert len(both) == len(co) > 10000 and len(co) >= max(len(c) for c in cs)
    one = 0
    for r in both:
        for i, rep in enumerate(reports):
            y = rep[r[0], r[1] + 1]
            assert (y[3], y[4]) == r[6 + i], (r, y)
        one += r[5] == 1
    assert one > 0          # sites only the unfiltered run holds: 0 0 in the other sample, and 0 0 in its report
