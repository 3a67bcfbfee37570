"""GPU: the count profile on the device (csrc/mdk_profile.hip in libmdk_stats.so) -- mdk.count_profile, mdk.profile_limits, Calls.profile,
Cytosines.profile, Cohort.profile, Calls.filter_depth and their CountProfile.  Every comparison is exact, against the restatement in
Python ints and numpy (tests/profile_rule.py); the derived statistics are held to the correctly rounded quotient."""
import math

import numpy as np
import pytest

import profile_rule as rule
from profile_tables import LEVEL_BINS, boundary_cells, check_mix, expected, groups, table

pytestmark = pytest.mark.gpu
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 4100)
SAMPLES = (1, 2, 3, 12, 65)
BINS = ((1, 1), (7, 3), (1024, 20), (4096, 256))
# the shortest range, bands of one, two and four samples, 1 and 3 workgroups
FORCED = (dict(range_sites=64, band_samples=1, max_workgroups=1), dict(range_sites=64, band_samples=1, max_workgroups=3), dict(range_sites=64, band_samples=4, max_workgroups=3),
          dict(range_sites=128, band_samples=2, max_workgroups=1), dict(band_samples=4), dict(range_sites=64))


def device(a, dtype="int64"):
    import torch
    return torch.from_numpy(np.array(a)).to(getattr(torch, dtype)).cuda().contiguous()      # (a copy: the shared tables are read-only)


def results(p):
    """a CountProfile as tests/profile_rule gives one: five numpy arrays"""
    return tuple(t.cpu().numpy() for t in (p.depth_hist, p.level_hist, p.nmeth_sum, p.nunmeth_sum, p.max_depth))


def same(got, want):
    return all(a.dtype == np.int64 and a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, want))


@pytest.fixture(autouse=True)
def default_limits():
    import methyldackel_amd as mdk
    yield
    mdk.profile_limits()


@pytest.mark.parametrize("n", SIZES)
def test_tables_against_the_rule(n):
    """every S at this n, int32 and int64 taking turns, without a group column and with one of 3 and of 4 groups, at every pair of bins
    and min_depth 1 and 5: the five tensors; the inputs as they were; a second run the same tensors"""
    import torch
    import methyldackel_amd as mdk
    for turn, S in enumerate(SAMPLES):
        dtype = ("int32", "int64")[(turn + SIZES.index(n)) % 2]
        for B, L in BINS:
            m, u = table(S, n, B)
            check_mix(m, u, B)                                      # depth 0, depths below min_depth, B - 1, B and B + 1 -- from 8 cells on
            dm, du = device(m, dtype), device(u, dtype)
            for G in (1, 3, 4):
                g = groups(n, G)
                dg = None if g is None else device(g, "uint8")
                for min_depth in (1, 5):
                    want = expected(S, n, G, B, L, min_depth)
                    p = mdk.count_profile(dm, du, dg, G, min_depth, B, L)
                    assert same(results(p), want), (S, n, dtype, G, B, L, min_depth)
                    assert (p.n_samples, p.n_groups, p.depth_bins, p.level_bins, p.min_depth, p.names, p.group_names) == (S, G, B, L, min_depth, None, None)
                    assert all(t.is_cuda and t.dtype == torch.int64 for t in (p.depth_hist, p.level_hist, p.nmeth_sum, p.nunmeth_sum, p.max_depth))
                    assert tuple(p.depth_hist.shape) == (S, G, B + 1) and tuple(p.level_hist.shape) == (S, G, L) and tuple(p.max_depth.shape) == (S, G)
                    assert p.sites().sum().item() == S * n
                assert same(results(mdk.count_profile(dm, du, dg, G, 5, B, L)), expected(S, n, G, B, L, 5))          # once more
                if dg is not None:
                    assert np.array_equal(dg.cpu().numpy(), g)
            assert np.array_equal(dm.cpu().numpy(), m) and np.array_equal(du.cpu().numpy(), u)


def test_1024_samples():
    import methyldackel_amd as mdk
    S, n = 1024, 65
    for G, (B, L) in ((3, (1024, 20)), (1, (7, 3))):
        m, u = table(S, n, B)
        check_mix(m, u, B)
        g = groups(n, G)
        p = mdk.count_profile(device(m, "int32"), device(u, "int32"), None if g is None else device(g, "uint8"), G, 1, B, L)
        assert same(results(p), expected(S, n, G, B, L, 1))


@pytest.mark.parametrize("what", ["deep", "empty"])
def test_the_contended_case(what):
    """4100 sites, every cell at depth 10 and all methylated, or every cell `0 0`: every lane of a wavefront counts into the same two
    words.  The counts are exact under the default blocking and under every forced one"""
    import torch
    import methyldackel_amd as mdk
    S, n = 5, 4100
    dm = torch.full((S, n), 10 if what == "deep" else 0, dtype=torch.int32, device="cuda")
    du = torch.zeros((S, n), dtype=torch.int32, device="cuda")
    g = groups(n, 3)
    per_group = np.bincount(g, minlength=3)
    dg = device(g, "uint8")
    for limits in (dict(),) + FORCED:
        mdk.profile_limits(**limits)
        for B in (1024, 7):
            p = mdk.count_profile(dm, du, dg, 3, 5, B, 20)
            dh, lh, ms, us, mx = results(p)
            want_dh = np.zeros((S, 3, B + 1), dtype=np.int64)
            want_dh[:, :, min(10, B) if what == "deep" else 0] = per_group
            want_lh = np.zeros((S, 3, 20), dtype=np.int64)
            if what == "deep":
                want_lh[:, :, 19] = per_group
            assert np.array_equal(dh, want_dh) and np.array_equal(lh, want_lh), (limits, B)
            assert np.array_equal(ms, np.broadcast_to(per_group * 10 if what == "deep" else per_group * 0, (S, 3))) and not us.any()
            assert np.array_equal(mx, np.full((S, 3), 10 if what == "deep" else 0))
        one = mdk.count_profile(dm, du, None, 1, 1, 1024, 20)       # no group column: the whole wavefront on one word
        assert one.depth_hist[:, 0, 10 if what == "deep" else 0].cpu().tolist() == [n] * S and one.sites().cpu().tolist() == [[n]] * S


@pytest.mark.parametrize("S,n,dtype", [(3, 257, "int64"), (12, 4100, "int32"), (65, 4100, "int64")])
def test_forced_blockings_give_the_same(S, n, dtype):
    """many workgroups on the same output cells, and one workgroup on all of them: the tensors of the defaults"""
    import methyldackel_amd as mdk
    for G, (B, L), min_depth in ((3, (1024, 20), 1), (4, (7, 3), 5), (1, (4096, 256), 1)):
        m, u = table(S, n, B)
        g = groups(n, G)
        dm, du, dg = device(m, dtype), device(u, dtype), None if g is None else device(g, "uint8")
        want = expected(S, n, G, B, L, min_depth)
        assert same(results(mdk.count_profile(dm, du, dg, G, min_depth, B, L)), want)
        for limits in FORCED:
            mdk.profile_limits(**limits)
            assert same(results(mdk.count_profile(dm, du, dg, G, min_depth, B, L)), want), (limits, G, B, L)
        mdk.profile_limits()


def test_limits_refusals():
    import methyldackel_amd as mdk
    for bad in (dict(range_sites=32), dict(range_sites=100), dict(range_sites=-64), dict(band_samples=3), dict(band_samples=8), dict(max_workgroups=-1)):
        with pytest.raises(mdk.MdkError, match="md_stats_profile_limits"):
            mdk.profile_limits(**bad)


@pytest.mark.parametrize("L", LEVEL_BINS)
def test_level_bins_of_every_magnitude(L):
    """the boundary cells of the CPU test, a sample per cell and one site: the cell's level bin, whose division is an estimate in floats
    put right in integers, is the one non-zero entry of its level_hist"""
    import methyldackel_amd as mdk
    cells = boundary_cells(L)
    for at in range(0, len(cells), 1024):
        some = cells[at:at + 1024]
        m, u = np.array([[a] for a, _ in some], dtype=np.int64), np.array([[b] for _, b in some], dtype=np.int64)
        p = mdk.count_profile(device(m, "int32"), device(u, "int32"), None, 1, 1, 1, L)
        lh = p.level_hist.cpu().numpy()[:, 0, :]
        assert lh.sum(1).tolist() == [1] * len(some)
        assert lh.argmax(1).tolist() == [rule.level_bin(a, a + b, L) for a, b in some]
        assert p.nmeth_sum[:, 0].cpu().tolist() == [a for a, _ in some] and p.max_depth[:, 0].cpu().tolist() == [a + b for a, b in some]
        assert p.depth_hist[:, 0, :].cpu().tolist() == [[0, 1]] * len(some)


def test_refusals_name_the_first_site():
    import torch
    import methyldackel_amd as mdk
    S, n, G = 12, 4100, 3
    m, u = table(S, n, 1024)
    g = groups(n, G)
    texts = {rule.E_NEGATIVE: "a count is negative", rule.E_ENTRY: r"a count is 2\^26 or more", rule.E_GROUP: "a site's group is 3 or more"}
    cases = ((((1, 3000, 0, -1),), None, (rule.E_NEGATIVE, 3000)),                      # a negative entry
             (((11, 77, 1, rule.LIMIT),), None, (rule.E_ENTRY, 77)),                    # 2^26
             ((), ((2100, 3),), (rule.E_GROUP, 2100)),                                  # group >= G
             (((5, 2000, 0, -1), (6, 130, 1, rule.LIMIT), (7, 131, 1, -1)), ((4000, 9),), (rule.E_ENTRY, 130)),      # several refusals in one table
             (((2, 4099, 1, -7), (9, 4099, 0, rule.LIMIT)), ((4099, 255),), (rule.E_NEGATIVE, 4099)),                # ... and at one site
             (((0, 1, 0, -1),), None, (rule.E_NEGATIVE, 1)))                            # a refused site after a good one
    for limits in (dict(), dict(range_sites=64, band_samples=1, max_workgroups=7)):
        mdk.profile_limits(**limits)
        for dtype in ("int32", "int64"):
            for changes, regroup, want in cases:
                mm, uu, gg = m.copy(), u.copy(), g.copy()
                for s, k, which, value in changes:
                    (mm, uu)[which][s, k] = value
                for k, value in regroup or ():
                    gg[k] = value
                assert rule.refusal(mm, uu, gg, G) == want
                with pytest.raises(mdk.MdkError, match="md_stats_profile.*" + texts[want[0]] + rf" \(site {want[1]}\)") as e:
                    mdk.count_profile(device(mm, dtype), device(uu, dtype), device(gg, "uint8"), G)
                assert e.value.rc == -3
            mm = m.copy()
            mm[4, 100] = rule.LIMIT - 1                             # the largest entry is taken
            assert same(results(mdk.count_profile(device(mm, dtype), device(u, dtype), device(g, "uint8"), G)), rule.profile_np(mm, u, g, G, 1, 1024, 20))
    mdk.profile_limits()
    big = torch.zeros((2, 70), dtype=torch.int64, device="cuda")
    big[1, 66] = 1 << 40                                            # (no 32 bits hold it)
    with pytest.raises(mdk.MdkError, match=r"a count is 2\^26 or more \(site 66\)"):
        mdk.count_profile(big, big.clone())
    with pytest.raises(mdk.MdkError, match=r"a site's group is 1 or more \(site 3\)"):          # a column and one group
        mdk.count_profile(big[:, :5].contiguous(), big[:, :5].contiguous(), torch.tensor([0, 0, 0, 1, 0], dtype=torch.uint8, device="cuda"), 1)


def test_api_refusals():
    import torch
    import methyldackel_amd as mdk
    m = torch.ones((3, 10), dtype=torch.int32, device="cuda")
    u = torch.ones((3, 10), dtype=torch.int32, device="cuda")
    g = torch.zeros(10, dtype=torch.uint8, device="cuda")
    mdk.profile_limits()                                            # (the handle is open)
    before = dict(mdk._side_handles)
    for args, text in (((m.cpu(), u), "there is no CPU path"), ((m, u.cpu()), "there is no CPU path"), ((m, u, g.cpu(), 2), "there is no CPU path"),
                       ((m, u.long()), "one dtype and one shape"), ((m, u[:, :9].contiguous()), "one dtype and one shape"), ((m.float(), u.float()), "int32 or int64"),
                       ((m[0], u[0]), r"\[samples, sites\]"), ((m.t(), u.t()), "contiguous"), ((m, u, torch.zeros(20, dtype=torch.uint8, device="cuda")[::2], 2), "contiguous"),
                       ((m, u, g[:9], 2), "group must be a uint8 tensor of 10 entries"), ((m, u, g.int(), 2), "group must be a uint8 tensor"),
                       ((m[:0], u[:0]), "1 to 1024 samples"), ((m[:1].expand(1025, 10), u[:1].expand(1025, 10)), "1 to 1024 samples"),
                       ((m[:1, :1].expand(1, (1 << 30) + 1), u[:1, :1].expand(1, (1 << 30) + 1)), "more than 2\\^30"),
                       ((m, u, g, 5), "n_groups"), ((m, u, g, 0), "n_groups"), ((m, u, None, 1, 0), "min_depth"), ((m, u, None, 1, 1 << 26), "min_depth"),
                       ((m, u, None, 1, 1, 0), "depth_bins"), ((m, u, None, 1, 1, 4097), "depth_bins"), ((m, u, None, 1, 1, 7, 0), "level_bins"), ((m, u, None, 1, 1, 7, 257), "level_bins")):
        with pytest.raises(mdk.MdkError, match=text):
            mdk.count_profile(*args)
    with pytest.raises(mdk.MdkError):
        mdk.count_profile(m, u, names=["a", "b"])
    with pytest.raises(mdk.MdkError, match="group_names"):
        mdk.count_profile(m, u, g, 2, group_names=["a"])
    assert dict(mdk._side_handles) == before                        # refused before the library was touched
    p = mdk.count_profile(m, u, None, 3, (1 << 26) - 1, names=["a", "b", "c"], group_names=["x", "y", "z"])       # groups without a column: all in group 0
    assert p.covered().cpu().tolist() == [[0] * 3] * 3 and p.sites().cpu().tolist() == [[10, 0, 0]] * 3 and (p.names, p.group_names) == (("a", "b", "c"), ("x", "y", "z"))


def objects(S=3, n=257, B=40):
    """a Cohort, and a Calls and a Cytosines of its sample 1, hand-built over table(S, n, B) with a context column of all three"""
    import torch
    import methyldackel_amd as mdk
    m, u = table(S, n, B)
    context = groups(n, 3)
    i = torch.arange(n, dtype=torch.int32)
    cols = {"contig": torch.zeros(n, dtype=torch.int32), "start": 10 * i, "end": 10 * i + 1, "context": torch.from_numpy(context.copy()),
            "strand": torch.ones(n, dtype=torch.int8), "nsamples": torch.full((n,), S, dtype=torch.int32)}
    names = tuple(f"lib{k}" for k in range(S))
    co = mdk.Cohort(["chr1"], {k: v.cuda() for k, v in cols.items()}, device(m, "int32"), device(u, "int32"), names=names)
    calls = mdk.Calls(["chr1"], {"contig": co.contig, "start": co.start, "end": co.end, "nmeth": device(m[1], "int32"), "nunmeth": device(u[1], "int32"),
                                 "context": co.context, "strand": co.strand})
    cyt = mdk.Cytosines(["chr1"], {"contig": co.contig, "pos": co.end, "strand": co.strand, "nmeth": calls.nmeth, "nunmeth": calls.nunmeth, "context": co.context,
                                   "trinucleotide": torch.full((n, 3), 67, dtype=torch.uint8, device="cuda")})
    return m, u, context, co, calls, cyt


def test_methods_are_count_profile_of_the_columns():
    import torch
    import methyldackel_amd as mdk
    m, u, context, co, calls, cyt = objects()
    S = len(m)
    for by, G, g, group_names in (("context", 3, context, ("CpG", "CHG", "CHH")), (None, 1, None, None)):
        for kw in (dict(), dict(min_depth=5, depth_bins=40, level_bins=7)):
            want = rule.profile_np(m, u, g, G, kw.get("min_depth", 1), kw.get("depth_bins", 1024), kw.get("level_bins", 20))
            p = co.profile(by=by, **kw)
            assert same(results(p), want) and p.names == co.names and p.group_names == group_names
            direct = mdk.count_profile(co.nmeth, co.nunmeth, None if g is None else co.context, G, kw.get("min_depth", 1), kw.get("depth_bins", 1024), kw.get("level_bins", 20))
            assert same(results(direct), want)
            one = tuple(a[1:2] for a in want)
            for obj in (calls, cyt, co.sample(1)):
                q = obj.profile(by=by, **kw)
                assert same(results(q), one) and q.names is None and q.group_names == group_names and q.n_samples == 1
            # the table's profile is the stack of its samples'
            stack = [co.sample(s).profile(by=by, **kw) for s in range(S)]
            for k, name in enumerate(("depth_hist", "level_hist", "nmeth_sum", "nunmeth_sum", "max_depth")):
                assert torch.equal(getattr(p, name), torch.cat([getattr(q, name) for q in stack]))
    # the uncovered cytosines of the reference are bin 0, and breadth the share covered
    p = cyt.profile()
    d = (m[1] + u[1])
    assert p.depth_hist[0, :, 0].cpu().tolist() == [int(((d == 0) & (context == k)).sum()) for k in range(3)] and (d == 0).sum() > 0
    assert p.breadth().cpu().tolist()[0] == [int(((d > 0) & (context == k)).sum()) / int((context == k).sum()) for k in range(3)]
    # row order does not matter
    perm = torch.randperm(len(calls), generator=torch.Generator().manual_seed(5)).cuda()
    assert same(results(calls.select(perm).profile()), results(calls.profile()))
    with pytest.raises(mdk.MdkError, match="by must be"):
        co.profile(by="strand")
    bad = calls.select(slice(None))
    bad.context[200] = 3
    with pytest.raises(mdk.MdkError, match=r"a site's group is 3 or more \(site 200\)"):
        bad.profile()


def test_two_parts_add_to_the_whole_on_the_device():
    import methyldackel_amd as mdk
    S, n, G, B, L = 12, 4100, 3, 1024, 20
    m, u = table(S, n, B)
    g = groups(n, G)
    names = [f"lib{i}" for i in range(S)]
    want = expected(S, n, G, B, L, 5)
    for cut in (1, n // 2, n - 1):
        a = mdk.count_profile(device(m[:, :cut], "int32"), device(u[:, :cut], "int32"), device(g[:cut], "uint8"), G, 5, B, L, names=names)
        b = mdk.count_profile(device(m[:, cut:], "int32"), device(u[:, cut:], "int32"), device(g[cut:], "uint8"), G, 5, B, L, names=names)
        both = a + b
        assert same(results(both), want) and both.names == tuple(names) and both.min_depth == 5 and not same(results(a), want)
    with pytest.raises(mdk.MdkError, match="profiles add over the same"):
        a + mdk.count_profile(device(m[:, :cut], "int32"), device(u[:, :cut], "int32"), device(g[:cut], "uint8"), G, 1, B, L, names=names)


def test_depth_quantile_filter_depth_and_the_derived_statistics():
    import torch
    import methyldackel_amd as mdk
    m, u, context, co, calls, cyt = objects(S=3, n=4100, B=40)
    S, n = m.shape
    d = m + u
    for min_depth in (1, 5):
        p = co.profile(min_depth=min_depth, depth_bins=64)
        for q in (0, 0.5, 0.999, 1):
            want = [[rule.depth_quantile(d[s][context == k], min_depth, 64, q) for k in range(3)] for s in range(S)]
            got = p.depth_quantile(q)
            assert got.is_cuda and got.dtype == torch.int64 and got.cpu().tolist() == want, (min_depth, q)
        assert p.median_depth().cpu().tolist() == p.depth_quantile(0.5).cpu().tolist()
        # the derived statistics: int / int in Python is the correctly rounded quotient
        dh, lh, ms, us, mx = (a.tolist() for a in results(p))
        for s in range(S):
            for k in range(3):
                sites, covered = sum(dh[s][k]), sum(lh[s][k])
                assert (p.sites()[s, k].item(), p.covered()[s, k].item()) == (sites, covered) and covered > 0
                assert p.breadth()[s, k].item() == covered / sites and p.mean_depth()[s, k].item() == (ms[s][k] + us[s][k]) / covered
                assert p.rate()[s, k].item() == ms[s][k] / (ms[s][k] + us[s][k])
    # the planted depths 39, 40 and 41 are the largest: at 40 bins the last percentile lies in the overflow bin
    shallow = co.profile(min_depth=1, depth_bins=40)
    assert shallow.depth_quantile(0.5).cpu().tolist() == co.profile(depth_bins=64).depth_quantile(0.5).cpu().tolist()
    with pytest.raises(mdk.MdkError, match=r"sample lib\d, group C.*overflow bin, depth 40 or more \(max_depth 4[01]\): raise depth_bins"):
        shallow.depth_quantile(1)
    with pytest.raises(mdk.MdkError, match="overflow bin"):         # min_depth >= depth_bins: every covered cell is there
        co.profile(min_depth=8, depth_bins=8).depth_quantile(0)
    nothing = mdk.count_profile(torch.zeros((2, 9), dtype=torch.int32, device="cuda"), torch.zeros((2, 9), dtype=torch.int32, device="cuda"))
    assert nothing.depth_quantile(0.5).cpu().tolist() == [[-1], [-1]] and torch.isnan(nothing.rate()).all() and nothing.breadth().cpu().tolist() == [[0.0], [0.0]]
    # filter_depth against a numpy selection
    d1 = d[1]
    for lo, hq in ((10, 0.999), (5, 0.5), (1, 1), (12, None), (3, 0.0)):
        keep = d1 >= lo
        if hq is not None:
            hi = np.array([rule.depth_quantile(d1[context == k], lo, 4096, hq) for k in range(3)])
            keep &= d1 <= hi[context]
        got = calls.filter_depth(lo, hq)
        assert isinstance(got, mdk.Calls) and len(got) == int(keep.sum()) and 0 < len(got) < n
        assert np.array_equal(got.start.cpu().numpy(), calls.start.cpu().numpy()[keep]) and np.array_equal(got.nmeth.cpu().numpy(), m[1][keep])
    with pytest.raises(mdk.MdkError, match="raise depth_bins"):
        calls.filter_depth(1, 1, depth_bins=40)


def test_diff_replicates_before_and_after_a_profile():
    """one handle: the F test's outputs are the same bits around a profile call, forced blockings among them"""
    import torch
    import methyldackel_amd as mdk
    m, u = table(4, 257, 40)
    dm, du = device(m, "int32"), device(u, "int32")
    before = mdk.diff_replicates(dm, du, [0, 1], [2, 3])
    mdk.profile_limits(range_sites=64, band_samples=1, max_workgroups=3)
    assert same(results(mdk.count_profile(dm, du, None, 1, 1, 40, 20)), rule.profile_np(m, u, None, 1, 1, 40, 20))
    after = mdk.diff_replicates(dm, du, [0, 1], [2, 3])
    assert len(after) == len(before) == 9
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert [name for (name, dev) in mdk._side_handles if dev == 0].count("stats") == 1
