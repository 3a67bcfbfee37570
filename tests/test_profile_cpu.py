"""CPU-only: the count profile (csrc/mdk_profile_core.h), driven through tools/profile_emu -- the host build of the header: its tensors
against the restatement in Python ints (tests/profile_rule.py), the level bin at every boundary, the refusals, the additivity of the
profiles, what the header declares and lib_profile() binds, and what mdk.count_profile and CountProfile refuse and write without a
device."""
import math
import re
import subprocess

import numpy as np
import pytest

import profile_rule as rule
from conftest import REPO
from profile_tables import LEVEL_BINS, boundary_cells, check_mix, expected, groups, table

EMU = REPO / "tools" / "_build" / "profile_emu"


def job_text(m, u, group, G, min_depth, B, L):
    S, n = len(m), len(m[0]) if len(m) else 0
    lines = ["P %d %d %d %d %d %d %d" % (S, n, G, min_depth, B, L, group is not None)]
    for s in range(S):
        lines += ["%d %d" % (a, b) for a, b in zip(m[s], u[s])]
    if group is not None:
        lines.append(" ".join(str(int(g)) for g in group))
    return "\n".join(lines) + "\n"


def run(text, jobs):
    """the emulator's results for the jobs of `text`, `jobs` their (S, G, B, L): (err, at) for a refused one, otherwise the five as
    nested lists"""
    r = subprocess.run([str(EMU)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = iter(r.stdout.splitlines())
    out = []
    for S, G, B, L in jobs:
        err, at = (int(v) for v in next(lines).split("\t"))
        if err:
            out.append((err, at))
            continue
        dh, lh, ms, us, mx = ([[None] * G for _ in range(S)] for _ in range(5))
        for s in range(S):
            for g in range(G):
                dh[s][g] = [int(v) for v in next(lines).split("\t")]
                lh[s][g] = [int(v) for v in next(lines).split("\t")]
                ms[s][g], us[s][g], mx[s][g] = (int(v) for v in next(lines).split("\t"))
                assert len(dh[s][g]) == B + 1 and len(lh[s][g]) == L
        out.append((dh, lh, ms, us, mx))
    assert next(lines, None) is None
    return out


def emu(m, u, group, G, min_depth, B, L):
    return run(job_text(m, u, group, G, min_depth, B, L), [(len(m), G, B, L)])[0]


def as_lists(arrays):
    return tuple(a.tolist() for a in arrays)


@pytest.mark.parametrize("S,n", [(1, 1), (2, 65), (3, 257), (12, 300), (17, 63)])
def test_emulator_is_the_rule(S, n):
    """seeded tables, with and without a group column, at the smallest and at ordinary bins and both depths: the five tensors exactly --
    and the bincounts the larger tests use are the loop over samples and sites"""
    for G, (B, L) in ((1, (1, 1)), (3, (7, 3)), (4, (1024, 20)), (3, (40, 256))):
        m, u = table(S, n, B)
        check_mix(m, u, B)
        g = groups(n, G)
        for min_depth in (1, 5):
            want = rule.profile(m, u, g, G, min_depth, B, L)
            assert emu(m.tolist(), u.tolist(), g, G, min_depth, B, L) == want
            assert as_lists(expected(S, n, G, B, L, min_depth)) == want
            if S * n >= 8:
                assert sum(sum(row[B] for row in sample) for sample in want[0]) >= 2           # B and B + 1 share the overflow bin
                assert sum(map(sum, want[4])) > 0 and max(max(row) for row in want[4]) >= B + 1


def test_no_sites_no_cover_and_an_empty_group():
    assert emu([[], []], [[], []], None, 2, 1, 4, 3) == rule.profile([[], []], [[], []], None, 2, 1, 4, 3)
    m, u, g = [[0, 1, 2, 9], [3, 0, 0, 0]], [[0, 2, 1, 0], [0, 0, 0, 0]], [0, 2, 2, 0]
    got = emu(m, u, g, 3, 4, 5, 2)
    assert got == rule.profile(m, u, g, 3, 4, 5, 2)
    assert got[0][0] == [[1, 0, 0, 0, 0, 1], [0] * 6, [0, 0, 0, 2, 0, 0]] and got[1][0] == [[0, 1], [0, 0], [0, 0]]
    assert got[2] == [[9, 0, 0], [0, 0, 0]] and got[4] == [[9, 0, 3], [3, 0, 0]]


@pytest.mark.parametrize("L", LEVEL_BINS)
def test_level_bin_at_every_boundary(L):
    """a sample per cell, one site, one depth bin: the cell's level bin is the one non-zero entry of its level_hist.  The bin is the
    integer l with l d <= m L < (l + 1) d, capped at L - 1, whatever the float estimate's last bits"""
    cells = boundary_cells(L)
    top = rule.LIMIT - 1
    assert (top, top) in cells and (0, 1) in cells and (1, 0) in cells and max(a + b for a, b in cells) == (1 << 27) - 2
    seen = set()
    for a, b in cells:
        d = a + b
        l = rule.level_bin(a, d, L)
        assert 0 <= l <= L - 1 and l * d <= a * L and (a * L < (l + 1) * d or (a == d and l == L - 1))
        seen |= {a * L - k * d for k in (l, l + 1) if 1 <= k <= L and abs(a * L - k * d) <= 1}
    assert seen == ({-1, 0} if L == 1 else {-1, 0, 1})               # m L is l d - 1, l d and l d + 1 for some cells and some l >= 1 (m <= d: no + 1 at l = L)
    for at in range(0, len(cells), 1024):
        some = cells[at:at + 1024]
        got = emu([[a] for a, _ in some], [[b] for _, b in some], None, 1, 1, 1, L)
        for i, (a, b) in enumerate(some):
            want = [0] * L
            want[rule.level_bin(a, a + b, L)] = 1
            assert got[1][i][0] == want, (a, b, L)
            assert got[0][i][0] == [0, 1] and (got[2][i][0], got[3][i][0], got[4][i][0]) == (a, b, a + b)


def test_refusals():
    m, u = table(3, 65, 7)
    g = groups(65, 3)
    m, u = m.tolist(), u.tolist()
    cases = [(((1, 40, 0, -1),), None, (rule.E_NEGATIVE, 40)), (((2, 7, 1, rule.LIMIT),), None, (rule.E_ENTRY, 7)), ((), (30, 3), (rule.E_GROUP, 30)),
             (((0, 64, 1, -3),), (64, 200), (rule.E_NEGATIVE, 64)),               # at one site the lowest code is named
             (((0, 50, 1, rule.LIMIT),), (50, 3), (rule.E_ENTRY, 50)),
             (((2, 9, 0, rule.LIMIT), (0, 9, 1, -1), (1, 30, 0, -1)), (8, 255), (rule.E_GROUP, 8)),      # ... and the smallest site
             (((1, 1, 0, -1),), (0, 3), (rule.E_GROUP, 0))]                        # a refused site before a good one and a refused one
    for changes, regroup, want in cases:
        mm, uu, gg = [list(r) for r in m], [list(r) for r in u], g.copy()
        for s, k, which, value in changes:
            (mm, uu)[which][s][k] = value
        if regroup:
            gg[regroup[0]] = regroup[1]
        assert rule.refusal(mm, uu, gg, 3) == want and emu(mm, uu, gg, 3, 1, 7, 3) == want
    mm = [list(r) for r in m]
    mm[0][5] = rule.LIMIT - 1                                       # the largest entry is taken
    assert rule.refusal(mm, u, g, 3) is None and emu(mm, u, g, 3, 1, 7, 3) == rule.profile(mm, u, g, 3, 1, 7, 3)
    assert emu(m, u, None, 1, 1, 7, 3) == rule.profile(m, u, None, 1, 1, 7, 3)


def test_two_parts_add_to_the_whole():
    S, n, G, B, L = 12, 300, 3, 7, 20
    m, u = table(S, n, B)
    g = groups(n, G)
    for min_depth in (1, 5):
        whole = expected(S, n, G, B, L, min_depth)
        for cut in (1, n // 2, n - 1):
            a = rule.profile_np(m[:, :cut], u[:, :cut], g[:cut], G, min_depth, B, L)
            b = rule.profile_np(m[:, cut:], u[:, cut:], g[cut:], G, min_depth, B, L)
            assert all(np.array_equal(x, y) for x, y in zip(rule.add(a, b), whole))
            assert as_lists(rule.add(a, b)) == tuple(emu(m.tolist(), u.tolist(), g, G, min_depth, B, L))
            assert not np.array_equal(a[0], whole[0])


def test_the_header_declares_what_lib_profile_binds():
    import methyldackel_amd as mdk
    header = (REPO / "include" / "mdk_profile.h").read_text()
    stats = (REPO / "include" / "mdk_stats.h").read_text()
    assert stats.index('#include "mdk_moments.h"') < stats.index('#include "mdk_profile.h"')
    declared = set(re.findall(r"\b(md_stats_\w+)\s*\(", header))
    assert declared == {"md_stats_profile", "md_stats_profile_limits"}
    L = mdk.lib_profile()                                           # (loading it needs no device)
    assert L is mdk.lib_stats()
    bound = {name for name in vars(L) if name.startswith("md_stats_")}
    assert declared <= bound
    for name, count in (("md_stats_profile", 16), ("md_stats_profile_limits", 4)):
        decl = re.search(r"int %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(decl.split(",")) == count == len(getattr(L, name).argtypes), name
    core = (REPO / "methyldackel_amd" / "csrc" / "mdk_profile_core.h").read_text()
    for name, value in (("PROF_MAX_GROUPS", mdk.PROFILE_MAX_GROUPS), ("PROF_MAX_DEPTH_BINS", mdk.PROFILE_MAX_DEPTH_BINS), ("PROF_MAX_LEVEL_BINS", mdk.PROFILE_MAX_LEVEL_BINS)):
        assert re.search(r"\b%s = %d\b" % (name, value), core), name
    assert (rule.MAX_GROUPS, rule.MAX_DEPTH_BINS, rule.MAX_LEVEL_BINS) == (mdk.PROFILE_MAX_GROUPS, mdk.PROFILE_MAX_DEPTH_BINS, mdk.PROFILE_MAX_LEVEL_BINS)
    assert (REPO / "methyldackel_amd" / "csrc" / "mdk_qdiff.hip").read_text().rstrip().endswith('#include "mdk_profile.hip"')


def test_refused_without_a_device():
    import torch
    import methyldackel_amd as mdk
    m, u = torch.ones((3, 5), dtype=torch.int32), torch.ones((3, 5), dtype=torch.int32)
    g = torch.zeros(5, dtype=torch.uint8)
    with pytest.raises(mdk.MdkError, match="there is no CPU path"):
        mdk.count_profile(m, u)
    with pytest.raises(mdk.MdkError, match="there is no CPU path"):
        mdk.count_profile(m, u, g, 3)
    with pytest.raises(mdk.MdkError, match="one dtype and one shape"):
        mdk.count_profile(m, u.long())
    with pytest.raises(mdk.MdkError, match="int32 or int64"):
        mdk.count_profile(m.float(), u.float())
    with pytest.raises(mdk.MdkError, match="1 to 1024 samples"):
        mdk.count_profile(m[:0], u[:0])
    with pytest.raises(mdk.MdkError, match="contiguous"):
        mdk.count_profile(m.t(), u.t())
    for bad in (g[:4], g.int(), g.reshape(1, 5), [0] * 5):
        with pytest.raises(mdk.MdkError, match="group must be a uint8 tensor of 5 entries"):
            mdk.count_profile(m, u, bad, 3)
    for name, values in (("min_depth", (0, -1, 1 << 26, 1.0, True, None)), ("n_groups", (0, 5, 2.0)), ("depth_bins", (0, 4097, "7")), ("level_bins", (0, 257, False))):
        for bad in values:
            with pytest.raises(mdk.MdkError, match=name):
                mdk.count_profile(m, u, **{name: bad})
    calls = mdk.Calls(["chr1"], {name: torch.zeros(5, dtype=getattr(torch, dt)) for name, dt in mdk.CALL_COLUMNS})
    with pytest.raises(mdk.MdkError, match="there is no CPU path"):
        calls.profile()
    with pytest.raises(mdk.MdkError, match="by must be"):
        calls.profile(by="strand")
    for bad in (0, 1 << 26, 2.5, True):
        with pytest.raises(mdk.MdkError, match="filter_depth: lo"):
            calls.filter_depth(lo=bad)
    assert callable(mdk.Cytosines.profile) and callable(mdk.Cohort.profile) and callable(mdk.profile_limits)
    assert mdk.PROFILE_WHAT == ("summary", "depth", "level")
    assert "type 7" in mdk.Calls.filter_depth.__doc__ and "type 7" in mdk.CountProfile.depth_quantile.__doc__


def hand_made(names=None, group_names=None):
    """two samples, two groups, depth_bins 5, level_bins 2, min_depth 2; sample 1's group 1 holds nothing, and sample 1's group 0 has
    cells in the overflow bin"""
    import torch
    import methyldackel_amd as mdk
    t = lambda v: torch.tensor(v, dtype=torch.int64)
    dh = t([[[4, 1, 3, 0, 2, 0], [0, 0, 0, 1, 0, 0]], [[0, 5, 1, 0, 0, 2], [7, 2, 0, 0, 0, 0]]])
    lh = t([[[2, 3], [1, 0]], [[0, 3], [0, 0]]])
    return mdk.CountProfile(dh, lh, t([[8, 1], [30, 0]]), t([[6, 2], [3, 0]]), t([[4, 3], [19, 1]]), 2, names, group_names)


def test_hand_made_profile_statistics_and_quantiles():
    import torch
    import methyldackel_amd as mdk
    p = hand_made()
    assert (p.n_samples, p.n_groups, p.depth_bins, p.level_bins, p.min_depth, p.names, p.group_names) == (2, 2, 5, 2, 2, None, None)
    assert p.sites().tolist() == [[10, 1], [8, 9]] and p.covered().tolist() == [[5, 1], [3, 0]]
    assert all(t.dtype == torch.float64 for t in (p.breadth(), p.mean_depth(), p.rate()))
    assert p.breadth().tolist() == [[5 / 10, 1 / 1], [3 / 8, 0 / 9]]
    mean, rate = p.mean_depth().tolist(), p.rate().tolist()
    assert mean[0] == [14 / 5, 3 / 1] and mean[1][0] == 33 / 3 and math.isnan(mean[1][1])
    assert rate[0] == [8 / 14, 1 / 3] and rate[1][0] == 30 / 33 and math.isnan(rate[1][1])
    empty = mdk.CountProfile(torch.zeros((1, 1, 3), dtype=torch.int64), torch.zeros((1, 1, 2), dtype=torch.int64), *[torch.zeros((1, 1), dtype=torch.int64)] * 3)
    assert math.isnan(empty.breadth().item()) and empty.depth_quantile(0.5).tolist() == [[-1]]
    # sample 0: covered depths 2 2 2 4 4 in group 0, 3 in group 1; sample 1: 2 and two cells of 5 or more in group 0, none in group 1
    first = mdk.CountProfile(p.depth_hist[:1], p.level_hist[:1], p.nmeth_sum[:1], p.nunmeth_sum[:1], p.max_depth[:1], 2)
    for q, want in ((0, [[2, 3]]), (0.2, [[2, 3]]), (0.5, [[2, 3]]), (0.6, [[2, 3]]), (0.61, [[4, 3]]), (1, [[4, 3]]), (1.0, [[4, 3]])):
        got = first.depth_quantile(q)
        assert got.dtype == torch.int64 and got.tolist() == want, q
        assert want == [[rule.depth_quantile([0] * 4 + [1] + [2] * 3 + [4] * 2, 2, 5, q), rule.depth_quantile([3], 2, 5, q)]]
    assert first.median_depth().tolist() == [[2, 3]]
    assert p.depth_quantile(1 / 3).tolist() == [[2, 3], [2, -1]] and p.depth_quantile(0).tolist() == [[2, 3], [2, -1]]
    for q in (0.34, 0.5, 1):
        with pytest.raises(mdk.MdkError, match=r"sample s1, group g0.*overflow bin.*max_depth 19.*raise depth_bins"):
            p.depth_quantile(q)
        with pytest.raises(rule.Overflow):
            rule.depth_quantile([1] * 5 + [2, 19, 7], 2, 5, q)
    named = hand_made(("a", "b"), ("CpG", "CHH"))
    with pytest.raises(mdk.MdkError, match=r"sample b, group CpG"):
        named.median_depth()
    deep = mdk.CountProfile(p.depth_hist[:1], p.level_hist[:1], p.nmeth_sum[:1], p.nunmeth_sum[:1], p.max_depth[:1], 5)      # min_depth >= depth_bins
    assert deep.depth_quantile(0).tolist() == [[-1, -1]]             # (its overflow bins are empty)
    deep = mdk.CountProfile(p.depth_hist[1:], p.level_hist[1:], p.nmeth_sum[1:], p.nunmeth_sum[1:], p.max_depth[1:], 7)
    with pytest.raises(mdk.MdkError, match="overflow bin"):
        deep.depth_quantile(0)
    for bad in (-0.1, 1.5, float("nan"), "0.5", None, True):
        with pytest.raises(mdk.MdkError, match="q must be a number within 0 and 1"):
            p.depth_quantile(bad)
    with pytest.raises(mdk.MdkError, match="a CountProfile is made of"):
        mdk.CountProfile(p.depth_hist, p.level_hist[:1], p.nmeth_sum, p.nunmeth_sum, p.max_depth)


def test_sum_of_hand_made_profiles():
    import torch
    import methyldackel_amd as mdk
    p, q = hand_made(("a", "b")), hand_made(("a", "b"))
    q.max_depth = torch.tensor([[9, 1], [2, 4]])
    both = p + q
    assert both.depth_hist.tolist() == (2 * p.depth_hist).tolist() and both.level_hist.tolist() == (2 * p.level_hist).tolist()
    assert both.nmeth_sum.tolist() == [[16, 2], [60, 0]] and both.nunmeth_sum.tolist() == [[12, 4], [6, 0]] and both.max_depth.tolist() == [[9, 3], [19, 4]]
    assert (both.min_depth, both.names, both.group_names) == (2, ("a", "b"), None)
    others = [hand_made(), hand_made(("a", "c")), hand_made(("a", "b"), ("x", "y")),
              mdk.CountProfile(p.depth_hist, p.level_hist, p.nmeth_sum, p.nunmeth_sum, p.max_depth, 3, ("a", "b")),
              mdk.CountProfile(p.depth_hist[:, :, :5], p.level_hist, p.nmeth_sum, p.nunmeth_sum, p.max_depth, 2, ("a", "b")),
              mdk.CountProfile(p.depth_hist, p.level_hist[:, :, :1], p.nmeth_sum, p.nunmeth_sum, p.max_depth, 2, ("a", "b")),
              mdk.CountProfile(p.depth_hist[:1], p.level_hist[:1], p.nmeth_sum[:1], p.nunmeth_sum[:1], p.max_depth[:1], 2)]
    for other in others:
        with pytest.raises(mdk.MdkError, match="profiles add over the same samples, groups, bins and min_depth"):
            p + other
    with pytest.raises(TypeError):
        p + 1


def test_write_layouts(tmp_path):
    import methyldackel_amd as mdk
    p = hand_made(("libA", "libB"), ("CpG", "CHH"))
    first = mdk.CountProfile(p.depth_hist[:1], p.level_hist[:1], p.nmeth_sum[:1], p.nunmeth_sum[:1], p.max_depth[:1], 2, ("libA",), ("CpG", "CHH"))
    assert first.rows() == [("libA", "CpG", 10, 5, 8, 6, 8 / 14, 14 / 5, 2, 4), ("libA", "CHH", 1, 1, 1, 2, 1 / 3, 3.0, 3, 3)]
    lines = open(first.write(tmp_path / "summary.tsv")).read().split("\n")
    assert lines[0] == "#count_profile\tsummary\tmin_depth=2\tdepth_bins=5\tlevel_bins=2"
    assert lines[1] == "#sample\tgroup\tsites\tcovered\tnmeth\tnunmeth\trate\tmean_depth\tmedian_depth\tmax_depth"
    assert lines[2] == "libA\tCpG\t10\t5\t8\t6\t%.17g\t%.17g\t2\t4" % (8 / 14, 14 / 5) and lines[3] == "libA\tCHH\t1\t1\t1\t2\t%.17g\t3\t3\t3" % (1 / 3)
    assert lines[4:] == [""] and float(lines[2].split("\t")[6]) == 8 / 14
    with pytest.raises(mdk.MdkError, match="overflow bin"):         # sample libB's median lies there
        p.write(tmp_path / "no.tsv")
    lines = open(p.write(tmp_path / "depth.tsv", "depth")).read().split("\n")
    assert lines[0] == "#count_profile\tdepth\tmin_depth=2\tdepth_bins=5\tlevel_bins=2" and lines[1] == "#sample\tgroup\tdepth\tcount"
    assert len(lines) == 2 + 2 * 2 * 6 + 1 and lines[2] == "libA\tCpG\t0\t4" and lines[7] == "libA\tCpG\t5\t0" and lines[8] == "libA\tCHH\t0\t0"
    assert lines[2 + 12 + 5] == "libB\tCpG\t5\t2" and lines[-2] == "libB\tCHH\t5\t0"
    assert p.rows("depth")[2 + 12 + 3] == ("libB", "CpG", 5, 2)
    lines = open(p.write(tmp_path / "level.tsv", "level")).read().split("\n")
    assert lines[0] == "#count_profile\tlevel\tmin_depth=2\tdepth_bins=5\tlevel_bins=2" and lines[1] == "#sample\tgroup\tbin\tlower\tupper\tcount"
    assert lines[2:] == ["libA\tCpG\t0\t0\t0.5\t2", "libA\tCpG\t1\t0.5\t1\t3", "libA\tCHH\t0\t0\t0.5\t1", "libA\tCHH\t1\t0.5\t1\t0",
                         "libB\tCpG\t0\t0\t0.5\t0", "libB\tCpG\t1\t0.5\t1\t3", "libB\tCHH\t0\t0\t0.5\t0", "libB\tCHH\t1\t0.5\t1\t0", ""]
    assert hand_made().rows("level")[0] == ("s0", "g0", 0, 0.0, 0.5, 2)
    with pytest.raises(mdk.MdkError, match="unknown table"):
        p.rows("joint")
    nan = mdk.CountProfile(p.depth_hist[1:, 1:], p.level_hist[1:, 1:], p.nmeth_sum[1:, 1:], p.nunmeth_sum[1:, 1:], p.max_depth[1:, 1:], 2)
    assert open(nan.write(tmp_path / "nan.tsv")).read().split("\n")[2] == "s0\tall\t9\t0\t0\t0\tnan\tnan\t-1\t1"
