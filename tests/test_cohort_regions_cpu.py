"""CPU-only: every sample's sums over intervals (csrc/mdk_cregion_core.h over csrc/mdk_region_core.h, the functions the kernels of
csrc/mdk_cregion.hip run), driven through tools/cregion_emu -- the kernels' passes on the host with the same sample batches and the same
grid cap -- against the rule per sample (tests/cohort_region_rule.py over tests/region_rule.py); the cell offset as a 64-bit value; what
Cohort.regions refuses without a device; and CohortRegions on tensors built by hand."""
import functools
import subprocess

import numpy as np
import pytest

import methyldackel_amd as mdk
from conftest import REPO
from cohort_region_rule import BIG_COUNTS, BIG_DEPTH, BIG_INTERVALS, BIG_ROWS, CONTEXT_MASK, big_expected, expected, sample_cols, sample_expected, sites_text
from merge_rule import SIZES
from region_rule import BIG, CONTIGS, ERRORS, FILTERS, KS, STRAND_MASK, covers, intervals, region_sums

EMU = REPO / "tools" / "_build" / "cregion_emu"
EMU_BLOCK, EMU_GRID = 4, 8                                    # the tool's defaults: the samples of a batch, the most workgroups of a launch
OVER_GRID = 256 * EMU_GRID + 77                               # sites: every grid-stride loop over blocks of sites takes a second turn
TABLES = SIZES[:-1] + (OVER_GRID,)
BLOCKINGS = [((), (1, 2, EMU_BLOCK, EMU_BLOCK + 1)), ((2, 3), (1, 2, 3))]          # (sample_block, max_workgroups) or the defaults, and the sample counts under it


def text(rows):
    return "".join("\t".join(str(v) for v in row) + "\n" for row in rows)


@functools.lru_cache(maxsize=None)
def intervals_text(n, k):
    return text(intervals(n, k))


def emu_text(inp, S, filters=((None, None, 1),), contigs=len(CONTIGS), blocking=()):
    """the emulator over `inp`: (the process, per filter the three [S, k] matrices as int64 arrays)"""
    args = [str(EMU), "--samples", str(S), "--contigs", str(contigs)]
    for ctx, strand, depth in filters:
        args += ["--filter", f"{CONTEXT_MASK(ctx)}:{STRAND_MASK[strand]}:{depth}"]
    if blocking:
        args += ["--sample-block", str(blocking[0]), "--max-workgroups", str(blocking[1])]
    r = subprocess.run(args, input=inp, capture_output=True, text=True)
    cells = np.array([[int(v) for v in l.split("\t")] for l in r.stdout.splitlines()], dtype=np.int64).reshape(len(filters), -1, S, 3) if r.stdout else np.zeros((len(filters), 0, S, 3), np.int64)
    return r, [tuple(np.ascontiguousarray(f[:, :, w].T) for w in range(3)) for f in cells]


def same(got, want):
    return all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("n", TABLES)
def test_emulator_against_the_rule(n):
    """every table with every number of samples under both blockings: every number of intervals, and the largest set under every filter"""
    k = KS[-1]
    if n > 1000:
        assert covers(n, k) == {"empty", "no rows", "one block", "lo on 256", "hi on 256", "whole blocks"}
    for blocking, counts in BLOCKINGS:
        for S in counts:
            sites = sites_text(n, S)
            for kk in KS:
                r, got = emu_text(sites + intervals_text(n, kk), S, blocking=blocking)
                assert r.returncode == 0, r.stderr
                assert same(got[0], expected(n, S, kk)), (n, S, kk, blocking)
            r, got = emu_text(sites + intervals_text(n, k), S, FILTERS, blocking=blocking)
            assert r.returncode == 0, r.stderr
            assert len(got) == len(FILTERS)
            for f, g in zip(FILTERS, got):
                assert same(g, expected(n, S, k, *f)), (n, S, f, blocking)
    if n >= 255:                                                                        # the depth cuts differently per sample
        at5, at0 = expected(n, 5, k, None, None, 5)[0].sum(axis=1), expected(n, 5, k, None, None, 0)[0].sum(axis=1)
        assert at0[1] == at0[0] > at5[0] > 0 == at5[1] and 0 < at5[2] < at0[2] and len({int(v) for v in at5}) == 5


@pytest.mark.parametrize("n", TABLES)
def test_the_expected_cells_are_region_sums(n):
    """what the tests compare against, held against region_rule.region_sums itself: every sample, three filters, the largest set"""
    k = KS[-1]
    for s in range(5):
        for f in ((None, None, 1), ((0,), "+", 5), ((2,), "-", 0)):
            want = region_sums(sample_cols(n, s), intervals(n, k), *f)
            got = sample_expected(n, s, k, *f)
            assert [tuple(int(got[w][j]) for w in range(3)) for j in range(k)] == want, (n, s, f)


def test_counts_past_int32():
    sites = text([(c, a, ctx, strand) + tuple(v for s in range(3) for v in (BIG_COUNTS[0][s][i], BIG_COUNTS[1][s][i])) for i, (c, a, b, ctx, strand) in enumerate(BIG_ROWS)])
    r, got = emu_text(sites + text(BIG_INTERVALS), 3, [(None, None, BIG_DEPTH)], contigs=1)
    assert r.returncode == 0, r.stderr
    assert same(got[0], big_expected()) and int(got[0][1][0][0]) == 3 * BIG > 2 ** 32 and int(got[0][2][1][0]) == 3 * BIG


def cohort_rows(rows, S=2):
    """rows of region_rule's seven fields as the emulator's sites: every sample holds the row's counts"""
    return text([(c, a, ctx, strand) + (m, u) * S for c, a, b, m, u, ctx, strand in rows])


@pytest.mark.parametrize("name,rows,ivs", ERRORS, ids=[f"{e[0]}{i}" for i, e in enumerate(ERRORS)])
def test_refusals(name, rows, ivs):
    """each refused condition alone, and (rows) with the bad row at a block's last and first place: rows 255 and 256"""
    r, got = emu_text(cohort_rows(rows) + text(ivs), 2, contigs=2)
    assert r.returncode == 3 and r.stderr.split() == ["error:", name] and r.stdout == "", (r.returncode, r.stderr)
    if name in ("order", "context"):
        for at in (255, 256):
            pad = [(0, k, k + 1, 1, 1, 2, 1) for k in range(at - len(rows) + 1)]
            r, _ = emu_text(cohort_rows(pad + [(c, a + 1000, b + 1000, m, u, t, s) for c, a, b, m, u, t, s in rows]) + text(ivs), 2, contigs=2)
            assert r.returncode == 3 and r.stderr.split() == ["error:", name], (at, r.returncode, r.stderr)
    good = [(0, 10, 11, 1, 1, 2, 1), (1, 0, 1, 1, 1, 0, -1)]
    r, got = emu_text(cohort_rows(good) + text([(0, 0, 100), (1, 0, 0), (1, BIG, BIG)]), 2, contigs=2)
    assert r.returncode == 0 and [g.tolist() for g in got[0]] == [[[1, 0, 0]] * 2] * 3


def test_cell_offset_in_64_bits():
    """cell (S - 1, n - 1) of the largest matrix, and the last entry of its block table: past 2^32, compared as 64-bit values"""
    S, n = 1024, 2 ** 30
    r = subprocess.run([str(EMU), "--cell", str(S - 1), str(n - 1), str(n)], capture_output=True, text=True)
    assert r.returncode == 0 and [int(v) for v in r.stdout.split()] == [S * n - 1, (S - 1) * (n // 256 + 1) + n // 256]
    assert S * n - 1 == 2 ** 40 - 1


def cohort(S=2, n=3, contigs=("a", "b"), **change):
    import torch
    cols = {"contig": torch.zeros(n, dtype=torch.int32), "start": torch.arange(n, dtype=torch.int32) * 10, "end": torch.arange(n, dtype=torch.int32) * 10 + 1,
            "context": torch.zeros(n, dtype=torch.uint8), "strand": torch.ones(n, dtype=torch.int8), "nsamples": torch.full((n,), S, dtype=torch.int32)}
    m, u = torch.ones((S, n), dtype=torch.int32), torch.ones((S, n), dtype=torch.int32)
    cols.update({k: v for k, v in change.items() if k in cols})
    return mdk.Cohort(list(contigs), cols, change.get("nmeth", m), change.get("nunmeth", u))


def test_refused_without_a_device():
    import torch
    iv = mdk.Intervals.windows([100, 50], 10, contigs=["a", "b"])
    with pytest.raises(mdk.MdkError, match="summed on the device.*no CPU path"):
        cohort().regions(iv)
    with pytest.raises(mdk.MdkError, match="nmeth column must be a contiguous int32 tensor of shape \\(2, 3\\)"):
        cohort(nmeth=torch.ones((2, 3), dtype=torch.int64)).regions(iv)
    with pytest.raises(mdk.MdkError, match="nunmeth column must be a contiguous int32"):
        cohort(nunmeth=torch.ones((3, 2), dtype=torch.int32).t()).regions(iv)
    with pytest.raises(mdk.MdkError, match="strand column must be a contiguous int8"):
        cohort(strand=torch.ones(3, dtype=torch.int32)).regions(iv)
    for S in (0, 1025):
        with pytest.raises(mdk.MdkError, match="1 to 1024 samples"):
            cohort(S=S).regions(iv)
    with pytest.raises(mdk.MdkError, match="contigs"):
        cohort(contigs=("a", "c")).regions(iv)
    with pytest.raises(mdk.MdkError, match="context"):
        cohort().regions(iv, contexts=("CpG", "CHX"))
    with pytest.raises(mdk.MdkError, match="context"):
        cohort().regions(iv, contexts=(3,))
    with pytest.raises(mdk.MdkError, match="strand"):
        cohort().regions(iv, strand="*")
    for depth in (-1, 2 ** 31):
        with pytest.raises(mdk.MdkError, match="min_depth"):
            cohort().regions(iv, min_depth=depth)
    with pytest.raises(mdk.MdkError, match="Intervals"):
        cohort().regions([(0, 0, 10)])


def test_cohort_regions_object(tmp_path):
    import torch
    t = lambda v, dt: torch.tensor(v, dtype=dt)
    r = mdk.CohortRegions(["a", "b"], t([0, 1, 0], torch.int32), t([0, 5, 10], torch.int32), t([10, 9, 20], torch.int32),
                          t([[1, 2, 3], [4, 5, 6]], torch.int32), t([[10, 20, 30], [40, 50, 3 * BIG]], torch.int64), t([[7, 8, 9], [0, 0, 0]], torch.int64), names=("ctl", "trt"))
    assert len(r) == 3 and r.n_samples == 2 and r.names == ("ctl", "trt") and r.contigs == ["a", "b"]
    assert r.rows() == [("a", 0, 10, (1, 10, 7), (4, 40, 0)), ("b", 5, 9, (2, 20, 8), (5, 50, 0)), ("a", 10, 20, (3, 30, 9), (6, 3 * BIG, 0))]
    head = "#chrom\tstart\tend\tctl.nsites\tctl.nmeth\tctl.nunmeth\ttrt.nsites\ttrt.nmeth\ttrt.nunmeth\n"
    body = "a\t0\t10\t1\t10\t7\t4\t40\t0\nb\t5\t9\t2\t20\t8\t5\t50\t0\na\t10\t20\t3\t30\t9\t6\t6442450941\t0\n"
    path = tmp_path / "r.tsv"
    assert r.write(path) == path and path.read_bytes() == (head + body).encode()
    r.write(path, names=["x", "y"])
    assert path.read_text() == head.replace("ctl", "x").replace("trt", "y") + body
    with pytest.raises(mdk.MdkError, match="names"):
        r.write(path, names=["x"])
    s1 = r.sample(1)
    assert isinstance(s1, mdk.Regions) and s1.rows() == [("a", 0, 10, 4, 40, 0), ("b", 5, 9, 5, 50, 0), ("a", 10, 20, 6, 3 * BIG, 0)]
    assert s1.nmeth.data_ptr() == r.nmeth[1].data_ptr() and s1.start is r.start                  # views, not copies
    with pytest.raises(mdk.MdkError, match="sample 2"):
        r.sample(2)
    iv = r.intervals()
    assert isinstance(iv, mdk.Intervals) and iv.contigs == ["a", "b"] and iv.start is r.start and iv.end is r.end and iv.contig is r.contig
    for index in (torch.tensor([True, False, True]), torch.tensor([0, 2]), slice(0, 3, 2)):
        c = r.select(index)
        assert c.rows() == [r.rows()[0], r.rows()[2]] and c.names == r.names and all(x.is_contiguous() for x in (c.nsites, c.nmeth, c.nunmeth, c.start))
    unnamed = mdk.CohortRegions(["a"], t([], torch.int32), t([], torch.int32), t([], torch.int32), torch.zeros((2, 0), dtype=torch.int32), torch.zeros((2, 0), dtype=torch.int64), torch.zeros((2, 0), dtype=torch.int64))
    assert len(unnamed) == 0 and unnamed.rows() == [] and unnamed.n_samples == 2
    unnamed.write(path)
    assert path.read_text() == "#chrom\tstart\tend\ts0.nsites\ts0.nmeth\ts0.nunmeth\ts1.nsites\ts1.nmeth\ts1.nunmeth\n"
