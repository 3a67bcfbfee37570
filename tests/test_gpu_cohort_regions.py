"""GPU: every sample's sums over intervals in one pass (k_cregion_sites / _ranges / _totals / _scan / _sum, csrc/mdk_cregion.hip) --
Cohort.regions.  Every comparison is exact: against the rule per sample (tests/cohort_region_rule.py over tests/region_rule.py), and against
the loop the call replaces, torch.stack of cohort.sample(s).regions(...)."""
import threading

import pytest

from cohort_region_rule import BIG_COUNTS, BIG_DEPTH, BIG_INTERVALS, BIG_ROWS, big_expected, expected, matrices, sample_cols
from merge_rule import COLUMNS, SIZES, table
from region_rule import BIG, CONTIGS, ERRORS, FILTERS, KS, MESSAGES, SCAN_N, intervals, region_sums, scan_expected, scan_intervals

pytestmark = pytest.mark.gpu
SITE = {"contig": 0, "start": 1, "end": 2, "context": 5, "strand": 6}              # the site columns among merge_rule's seven


@pytest.fixture(autouse=True)
def default_limits():
    import methyldackel_amd as mdk
    yield
    mdk.cohort_limits(0, 0, 0, 0)


def cohort_of(cols, m, u, contigs=CONTIGS, names=None):
    """a Cohort of numpy site columns (merge_rule's seven) and [S, n] count matrices, on the device"""
    import torch
    import methyldackel_amd as mdk
    site = {name: torch.from_numpy(cols[at].copy()).cuda() for name, at in SITE.items()}
    m, u = torch.from_numpy(m.copy()).cuda(), torch.from_numpy(u.copy()).cuda()
    site["nsamples"] = ((m + u) > 0).sum(0).to(torch.int32)
    return mdk.Cohort(list(contigs), site, m, u, names=names)


def cohort_rows(rows, S=2, contigs=("a", "b")):
    """rows of region_rule's seven fields as a Cohort in which every sample holds the row's counts"""
    import numpy as np
    from merge_rule import DTYPES
    cols = [np.array([r[k] for r in rows], dtype=dt) for k, dt in enumerate(DTYPES)]
    return cohort_of(cols, np.stack([cols[3]] * S), np.stack([cols[4]] * S), contigs)


def intervals_of(ivs, contigs=CONTIGS, device="cpu"):
    import torch
    import methyldackel_amd as mdk
    return mdk.Intervals(list(contigs), *[torch.tensor([r[k] for r in ivs], dtype=torch.int32, device=device) for k in range(3)])


def same(r, want):
    """are the result's three matrices exactly the rule's?"""
    import torch
    return all(torch.equal(getattr(r, name).cpu(), torch.from_numpy(w).to(dt)) for name, dt, w in zip(("nsites", "nmeth", "nunmeth"), (torch.int32, torch.int64, torch.int64), want))


def looped(c, iv, *f):
    """the loop the call replaces: three [S, k] matrices"""
    import torch
    per = [c.sample(s).regions(iv, *f) for s in range(c.n_samples)]
    return [torch.stack([getattr(p, name) for p in per]) for name in ("nsites", "nmeth", "nunmeth")]


# first in the file: the kernels' first execution
@pytest.mark.parametrize("n", (0, 1, 2, 255, 256, 257, 513))
def test_blocking_on_the_device(n):
    """every table with 1, 2, 3 and 5 samples in batches of 2 under a grid of 3, and 5 under the defaults: every number of intervals, and
    the largest set under every filter"""
    import torch
    import methyldackel_amd as mdk
    k = KS[-1]
    for limits, S in [((0, 2, 3), S) for S in (1, 2, 3, 5)] + [((0, 0, 0), 5)]:
        mdk.cohort_limits(0, *limits)
        m, u = matrices(n, S)
        c = cohort_of(table(n), m, u)
        for kk in KS:
            iv = intervals_of(intervals(n, kk))
            r = c.regions(iv)
            assert r.contigs == c.contigs and len(r) == kk and r.n_samples == S and r.names is None
            for name, dt, shape in (("contig", torch.int32, (kk,)), ("start", torch.int32, (kk,)), ("end", torch.int32, (kk,)),
                                    ("nsites", torch.int32, (S, kk)), ("nmeth", torch.int64, (S, kk)), ("nunmeth", torch.int64, (S, kk))):
                t = getattr(r, name)
                assert t.dtype == dt and t.device == c.start.device and t.is_contiguous() and t.shape == shape, name
            assert all(torch.equal(getattr(r, name).cpu(), getattr(iv, name)) for name in ("contig", "start", "end"))          # the intervals' own order
            assert same(r, expected(n, S, kk)), (n, S, kk, limits)
        iv = intervals_of(intervals(n, k), device="cuda")
        kept = [t.clone() for t in (iv.contig, iv.start, iv.end)]
        for f in FILTERS:
            r = c.regions(iv, contexts=f[0], strand=f[1], min_depth=f[2])
            assert same(r, expected(n, S, k, *f)), (n, S, f, limits)
            assert r.start.data_ptr() == iv.start.data_ptr()                      # intervals on the device are not copied
        assert same(c.regions(iv, contexts=("CHH", "CpG"), strand="-", min_depth=5), expected(n, S, k, (0, 2), "-", 5))
        # the inputs are as they were
        assert all(torch.equal(getattr(c, name).cpu(), torch.from_numpy(table(n)[at].copy())) for name, at in SITE.items())
        assert torch.equal(c.nmeth.cpu(), torch.from_numpy(m)) and torch.equal(c.nunmeth.cpu(), torch.from_numpy(u))
        assert all(torch.equal(a, b) for a, b in zip(kept, (iv.contig, iv.start, iv.end)))


def test_the_loop_as_second_oracle():
    """S = 16 at n = 300001 with 5003 intervals, six filters: the three matrices are the stacked loop's"""
    import torch
    n, k, S = SIZES[-1], KS[-1], 16
    m, u = matrices(n, S)
    c = cohort_of(table(n), m, u)
    iv = intervals_of(intervals(n, k), device="cuda")
    for f in ((None, None, 1), ((0,), "+", 5), ((2,), "-", 0), ((1,), None, 1), (None, "-", 5), (("CpG", "CHH"), "+", 0)):
        r = c.regions(iv, *f)
        want = looped(c, iv, *f)
        for got, w in zip((r.nsites, r.nmeth, r.nunmeth), want):
            assert got.dtype == w.dtype and got.shape == w.shape == (S, k) and torch.equal(got, w), f
    assert int(r.nsites[0].sum()) > 1000 and int(r.nsites[1].sum()) > 0 and int(c.regions(iv).nsites[1].sum()) == 0          # sample 1 is all 0 0


def test_second_round_of_the_block_scan():
    """more than 4096 blocks of 256 rows (no limit shrinks a round of k_cregion_scan): the prefix entries of EVERY sample behind the first
    round hold that sample's carry.  Sample 0 against region_rule's shared expectation, sample 2 (seeded) against region_sums"""
    import torch
    m, u = matrices(SCAN_N, 3)
    c = cohort_of(table(SCAN_N), m, u)
    iv = intervals_of(scan_intervals(), device="cuda")
    for f in ((None, None, 1), ((0,), "-", 5)):
        r = c.regions(iv, *f)
        for s, want in ((0, scan_expected(*f)), (2, region_sums(sample_cols(SCAN_N, 2), scan_intervals(), *f))):
            assert list(zip(r.nsites[s].tolist(), r.nmeth[s].tolist(), r.nunmeth[s].tolist())) == list(want), (f, s)
        assert int(r.nsites[1].sum()) == 0 and int(r.nsites[2].max()) > 4096          # sample 1 is all 0 0; sample 2 has an interval over many blocks
    assert scan_expected()[-2][0] > 256 * 1024          # the whole contig: whole blocks on both sides of the round's edge


def test_a_merged_table():
    """one context after merge_context on each sample, then unite: strand-0 rows wider than a base, and sites a sample does not hold"""
    import torch
    import methyldackel_amd as mdk
    from region_rule import intervals_over
    n = 513
    cols = table(n)
    calls = []
    for s in (0, 2, 3):
        m, u = sample_cols(n, s)[3:5]
        c = mdk.Calls(list(CONTIGS), {name: torch.from_numpy(col.copy()).cuda() for name, col in zip(COLUMNS, cols[:3] + (m, u) + cols[5:])}).merge_context(0)
        calls.append(c.select(c.context == 0))
    co = mdk.unite(calls, min_samples=1)
    assert int((co.strand == 0).sum()) > 0 and int((co.end - co.start > 1).sum()) > 0 and int((co.nsamples < 3).sum()) > 0
    site = [getattr(co, name).cpu().numpy() for name in ("contig", "start", "end")]
    ivs = intervals_over(site + [None, None, co.context.cpu().numpy(), co.strand.cpu().numpy()], 65)
    for f in ((None, None, 1), ((0,), None, 0), (None, None, 5), ((2,), None, 0), (None, "+", 1)):
        r = co.regions(intervals_of(ivs), *f)
        for s in range(3):
            rows = site + [co.nmeth[s].cpu().numpy(), co.nunmeth[s].cpu().numpy(), co.context.cpu().numpy(), co.strand.cpu().numpy()]
            assert list(zip(r.nsites[s].tolist(), r.nmeth[s].tolist(), r.nunmeth[s].tolist())) == region_sums(rows, ivs, *f), (f, s)
    assert int(co.regions(intervals_of(ivs)).nsites.sum()) > 0


def test_counts_past_int32():
    import numpy as np
    import torch
    from merge_rule import DTYPES
    cols = [np.array(c, dtype=DTYPES[at]) for c, at in zip(zip(*BIG_ROWS), (0, 1, 2, 5, 6))]
    c = cohort_of([cols[0], cols[1], cols[2], None, None, cols[3], cols[4]], np.array(BIG_COUNTS[0], dtype=np.int32), np.array(BIG_COUNTS[1], dtype=np.int32), names=("x", "y", "z"))
    r = c.regions(intervals_of(BIG_INTERVALS), min_depth=BIG_DEPTH)
    assert same(r, big_expected()) and int(r.nmeth[0, 0]) == 3 * BIG > 2 ** 32 and r.names == ("x", "y", "z")
    assert r.rows()[0] == ("c0", 0, 3, (3, 3 * BIG, 3 * BIG), (3, 2 * BIG, 3 * BIG), (0, 0, 0))
    assert r.sample(1).rows()[0] == ("c0", 0, 3, 3, 2 * BIG, 3 * BIG)


@pytest.mark.parametrize("name,rows,ivs", ERRORS, ids=[f"{e[0]}{i}" for i, e in enumerate(ERRORS)])
def test_refusals(name, rows, ivs):
    """each refusal with rc -3 and the library's phrase: alone, and (rows) with the bad row at a block's last and first place; the next call
    on the same handle is clean"""
    import methyldackel_amd as mdk
    tables = [rows]
    if name in ("order", "context"):
        for at in (255, 256):
            pad = [(0, k, k + 1, 1, 1, 2, 1) for k in range(at - len(rows) + 1)]
            tables.append(pad + [(c, a + 1000, b + 1000, m, u, t, s) for c, a, b, m, u, t, s in rows])
    for tab in tables:
        with pytest.raises(mdk.MdkError, match=MESSAGES[name]) as e:
            cohort_rows(tab).regions(intervals_of(ivs, ("a", "b")))
        assert e.value.rc == -3 and "md_cohort_regions" in str(e.value)
    good = cohort_rows([(0, 10, 11, 1, 1, 2, 1), (1, 0, 1, 1, 1, 0, -1)])
    r = good.regions(intervals_of([(0, 0, 100), (1, 0, 0), (1, BIG, BIG)], ("a", "b")))
    assert r.nsites.tolist() == [[1, 0, 0]] * 2 and r.nmeth.tolist() == [[1, 0, 0]] * 2 and r.nunmeth.tolist() == [[1, 0, 0]] * 2


def test_handle_reuse():
    """a second call and a call from another thread equal the first; the library still holds one handle on device 0"""
    import torch
    import methyldackel_amd as mdk
    n, k, S = 513, 257, 3
    m, u = matrices(n, S)
    c = cohort_of(table(n), m, u)
    iv = intervals_of(intervals(n, k), device="cuda")
    first = c.regions(iv, min_depth=5)
    assert same(first, expected(n, S, k, None, None, 5))
    mine = {key: h.value for key, h in mdk._side_handles.items() if key[0] == "cohort"}
    assert list(mine) == [("cohort", 0)] and mine["cohort", 0]
    got = [c.regions(iv, min_depth=5)]
    t = threading.Thread(target=lambda: got.append(c.regions(iv, min_depth=5)))
    t.start(); t.join()
    assert len(got) == 2 and all(torch.equal(getattr(g, name), getattr(first, name)) for g in got for name in ("nsites", "nmeth", "nunmeth"))
    assert {key: h.value for key, h in mdk._side_handles.items() if key[0] == "cohort"} == mine
    # the table's text, made on the same handle, is what it was before the sums
    text = c.render()
    c.regions(iv)
    assert torch.equal(c.render(), text)


def test_with_diff_replicates():
    """the matrices go into diff_replicates as they come: bit for bit what the stacked loop's give"""
    import torch
    import methyldackel_amd as mdk
    n, k, S = 513, 257, 5
    m, u = matrices(n, S)
    c = cohort_of(table(n), m, u)
    iv = intervals_of(intervals(n, k), device="cuda")
    r = c.regions(iv)
    _, lm, lu = looped(c, iv)
    a, b = [0, 2], [3, 4]
    got, want = mdk.diff_replicates(r.nmeth, r.nunmeth, a, b), mdk.diff_replicates(lm, lu, a, b)
    assert len(got) == len(want) and all(x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(got, want))
    assert int((got[5] < 1).sum()) > 0
