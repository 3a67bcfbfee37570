"""CPU-only: sums of rows over intervals (csrc/mdk_region_core.h, the functions k_region_rows and k_region_sum of csrc/mdk_regions.hip run),
driven through tools/region_emu -- the kernels' 256-row block totals, their scan and the two partial blocks per interval on the host --
against a plain Python restatement (tests/region_rule.py) and the oracle's `extract -l`; Intervals.read and Intervals.windows; and what
Calls.regions refuses without a device."""
import subprocess

import pytest

import methyldackel_amd as mdk
from conftest import REPO, run_oracle
from merge_rule import SIZES, table_rows
from region_rule import BIG, CONTIGS, ERRORS, FILTERS, KS, SCAN_N, STRAND_MASK, covers, expected, intervals, region_sums, scan_expected, scan_intervals

EMU = REPO / "tools" / "_build" / "region_emu"


def text(rows):
    return "".join("\t".join(str(v) for v in row) + "\n" for row in rows)


def emu_text(inp, contexts=None, strand=None, min_depth=1, contigs=len(CONTIGS)):
    mask = 7 if contexts is None else sum(1 << t for t in contexts)
    r = subprocess.run([str(EMU), "--contigs", str(contigs), "--contexts", str(mask), "--strands", str(STRAND_MASK[strand]), "--min-depth", str(min_depth)],
                       input=inp, capture_output=True, text=True)
    return r, [tuple(int(v) for v in l.split("\t")) for l in r.stdout.splitlines()]


def emu(rows, ivs, *args, **kw):
    return emu_text(text(rows) + text(ivs), *args, **kw)


@pytest.mark.parametrize("n", SIZES)
def test_blocking(n):
    """every table with every number of intervals, and the largest set with every filter"""
    rows = text(table_rows(n))
    if n > 1000:
        assert covers(n, KS[-1]) == {"empty", "no rows", "one block", "lo on 256", "hi on 256", "whole blocks"}
    for k in KS:
        r, got = emu_text(rows + text(intervals(n, k)))
        assert r.returncode == 0, r.stderr
        assert len(got) == k and got == list(expected(n, k)), (n, k)
    k = KS[-1]
    for f in FILTERS if n < 1000 else FILTERS[::5] + FILTERS[-1:]:         # (a run over the large table parses 300,001 lines of text)
        r, got = emu_text(rows + text(intervals(n, k)), *f)
        assert r.returncode == 0, r.stderr
        assert got == list(expected(n, k, *f)), (n, f)
    if n >= 255:
        assert sum(e[0] for e in expected(n, k, (0,), "+", 5)) < sum(e[0] for e in expected(n, k, (0,), None, 5)) < sum(e[0] for e in expected(n, k, None, None, 0))


def test_second_round_of_the_block_scan():
    """more than 4096 blocks of 256 rows: the prefix entries behind the first round of k_region_blocks hold its carry"""
    inp = text(table_rows(SCAN_N)) + text(scan_intervals())
    for f in ((None, None, 1), ((0,), "-", 5)):
        r, got = emu_text(inp, *f)
        assert r.returncode == 0, r.stderr
        assert got == list(scan_expected(*f)), f
    assert scan_expected()[-2][0] > 256 * 1024          # the whole contig: whole blocks on both sides of the round's edge


def test_edges_by_hand():
    rows = [(0, 10, 11, 1, 2, 0, 1), (0, 11, 12, 3, 4, 0, -1), (0, 20, 23, 5, 6, 1, 0), (1, 5, 6, 0, 0, 2, -1)]
    ivs = [(0, 10, 11), (0, 11, 11), (0, 0, 10), (0, 0, BIG), (1, 0, BIG), (0, 21, 30), (0, 20, 21), (1, 5, 5), (1, 6, 9), (0, 10, 12), (0, 10, 12)]
    # a merged row belongs to the interval that holds its start, however wide it is; the end is exclusive; min_depth 0 counts the 0 0 row
    assert emu(rows, ivs, min_depth=0, contigs=2)[1] == [(1, 1, 2), (0, 0, 0), (0, 0, 0), (3, 9, 12), (1, 0, 0), (0, 0, 0), (1, 5, 6), (0, 0, 0), (0, 0, 0), (2, 4, 6), (2, 4, 6)]
    assert emu(rows, ivs, contigs=2)[1][4] == (0, 0, 0)
    assert emu(rows, [(0, 0, BIG)], strand="+", contigs=2)[1] == [(1, 1, 2)] and emu(rows, [(0, 0, BIG)], strand="-", contigs=2)[1] == [(1, 3, 4)]
    assert emu(rows, [(0, 0, BIG)], contexts=(1,), contigs=2)[1] == [(1, 5, 6)] and emu(rows, [(0, 0, BIG)], contexts=(2,), contigs=2)[1] == [(0, 0, 0)]
    assert emu(rows, [], contigs=2)[1] == [] and emu([], ivs[:3], contigs=2)[1] == [(0, 0, 0)] * 3
    # the depth is formed in 64 bits, the sums in int64
    big = [(0, k, k + 1, BIG, BIG, 0, 1) for k in range(3)]
    assert emu(big, [(0, 0, 3), (0, 1, 2)], min_depth=BIG)[1] == [(3, 3 * BIG, 3 * BIG), (1, BIG, BIG)]


@pytest.mark.parametrize("name,rows,ivs", ERRORS, ids=[f"{e[0]}{i}" for i, e in enumerate(ERRORS)])
def test_error_bits(name, rows, ivs):
    """each refused condition alone (and at a workgroup's edge: row 256 looks at row 255)"""
    r, got = emu(rows, ivs, contigs=2)
    assert r.returncode == 3 and r.stderr.split() == ["error:", name] and got == [], (r.returncode, r.stderr)
    if name in ("order", "context"):
        pad = [(0, k, k + 1, 1, 1, 2, 1) for k in range(256 - len(rows) + 1)]
        r, _ = emu(pad + [(c, a + 1000, b + 1000, m, u, t, s) for c, a, b, m, u, t, s in rows], ivs, contigs=2)
        assert r.returncode == 3 and r.stderr.split() == ["error:", name], (r.returncode, r.stderr)
    good = [(0, 10, 11, 1, 1, 2, 1), (1, 0, 1, 1, 1, 0, -1)]
    assert emu(good, [(0, 0, 100), (1, 0, 0), (1, BIG, BIG)], contigs=2)[0].returncode == 0


def test_intervals_read(tmp_path):
    import torch
    bed = tmp_path / "a.bed"
    bed.write_text("track name=x\n#c\tcomment\nbrowser position b:1-2\n\nb\t5\t9\tisland\t0\t+\na 0 0\n  a\t7  \t 2147483647\nb\t5\t9\n")
    iv = mdk.Intervals.read(bed, ["a", "b"])
    assert iv.contigs == ["a", "b"] and len(iv) == 4
    assert all(t.dtype == torch.int32 and t.device.type == "cpu" for t in (iv.contig, iv.start, iv.end))
    assert list(zip(iv.contig.tolist(), iv.start.tolist(), iv.end.tolist())) == [(1, 5, 9), (0, 0, 0), (0, 7, BIG), (1, 5, 9)]
    assert iv.to("cpu") is iv
    (tmp_path / "e.bed").write_text("#only\n\n")
    assert len(mdk.Intervals.read(tmp_path / "e.bed", ["a"])) == 0
    for line, what in (("c\t1\t2", "contig"), ("a\tx\t2", "not a decimal"), ("a\t1\t2.5", "not a decimal"), ("a\t-1\t2", "not a decimal"), ("a\t9\t8", "end 8 < start 9"),
                       ("a\t1\t2147483648", "2\\^31 - 1"), ("a\t1", "three fields")):
        bad = tmp_path / "bad.bed"
        bad.write_text("a\t1\t2\n\n" + line + "\n")
        with pytest.raises(mdk.MdkError, match=what) as e:
            mdk.Intervals.read(bad, ["a", "b"])
        assert f"{bad}:3:" in str(e.value)


def test_intervals_windows():
    def rows(iv):
        return list(zip(iv.contig.tolist(), iv.start.tolist(), iv.end.tolist()))
    iv = mdk.Intervals.windows([25, 0, 10, 3], 10, contigs=["a", "z", "b", "c"])
    assert iv.contigs == ["a", "z", "b", "c"]
    assert rows(iv) == [(0, 0, 10), (0, 10, 20), (0, 20, 25), (2, 0, 10), (3, 0, 3)]          # the last window clipped, the empty contig without one
    assert rows(mdk.Intervals.windows([25], 10, step=4, contigs=["a"])) == [(0, 0, 10), (0, 4, 14), (0, 8, 18), (0, 12, 22), (0, 16, 25), (0, 20, 25), (0, 24, 25)]
    assert rows(mdk.Intervals.windows([25], 4, step=10, contigs=["a"])) == [(0, 0, 4), (0, 10, 14), (0, 20, 24)]
    assert len(mdk.Intervals.windows([], 10, contigs=[])) == 0
    import torch
    assert all(t.dtype == torch.int32 for t in (iv.contig, iv.start, iv.end))
    for args, kw in ((([5], 0), {"contigs": ["a"]}), (([5], 3), {"step": 0, "contigs": ["a"]}), (([BIG, BIG], 1), {"contigs": ["a", "b"]}), (([5], 3), {}), (([5, 6], 3), {"contigs": ["a"]})):
        with pytest.raises(mdk.MdkError):
            mdk.Intervals.windows(*args, **kw)


def test_windows_of_a_reference(small_synth):
    with mdk.Reference(small_synth / "pe.fa") as ref:
        iv = mdk.Intervals.windows(ref, 1000)
        assert iv.contigs == ref.contigs and len(iv) == sum((x + 999) // 1000 for x in ref.lengths) == 60
        assert int(iv.end[39]) == 40000 and int(iv.start[40]) == 0 and int(iv.contig[40]) == 1


def columns(rows, contigs=("a", "b")):
    import torch
    from merge_rule import COLUMNS, DTYPES
    cols = {n: torch.tensor([r[k] for r in rows], dtype=getattr(torch, dt)) for k, (n, dt) in enumerate(zip(COLUMNS, DTYPES))}
    return mdk.Calls(list(contigs), cols)


def test_refused_without_a_device():
    rows = [(0, 10, 11, 1, 2, 0, 1), (0, 11, 12, 3, 4, 0, -1)]
    iv = mdk.Intervals.windows([100, 50], 10, contigs=["a", "b"])
    with pytest.raises(mdk.MdkError, match="summed on the device.*no CPU path"):
        columns(rows).regions(iv)
    with pytest.raises(mdk.MdkError, match="contigs"):
        columns(rows, ("a", "c")).regions(iv)
    with pytest.raises(mdk.MdkError, match="context"):
        columns(rows).regions(iv, contexts=("CpG", "CHX"))
    with pytest.raises(mdk.MdkError, match="context"):
        columns(rows).regions(iv, contexts=(3,))
    with pytest.raises(mdk.MdkError, match="strand"):
        columns(rows).regions(iv, strand="*")
    with pytest.raises(mdk.MdkError, match="min_depth"):
        columns(rows).regions(iv, min_depth=-1)
    with pytest.raises(mdk.MdkError, match="Intervals"):
        columns(rows).regions([(0, 0, 10)])
    assert "md_text_regions" in mdk.HIP_SYMBOLS


@pytest.mark.parametrize("strand", ["+", "-"])
def test_sums_equal_the_oracles_extract_with_a_bed(tmp_path_factory, small_synth, strand):
    """small_synth/pe, CpG, per strand.  The premise first: the rows of the oracle's `extract -l bed` are exactly the rows of its
    unrestricted run whose start lies inside an interval.  Then: the emulator's sums over the unrestricted rows are the sums of the -l rows"""
    d = tmp_path_factory.mktemp("regions")
    fa, bam = small_synth / "pe.fa", small_synth / "pe.bam"
    names, seqs = [], {}
    for l in open(fa).read().splitlines():
        if l.startswith(">"):
            names.append(l[1:].split()[0]); seqs[names[-1]] = []
        else:
            seqs[names[-1]].append(l.upper())
    seqs = ["".join(seqs[n]) for n in names]
    ivs = [(0, 1000, 1800), (0, 1800, 1801), (0, 5000, 9000), (0, 20000, 20001), (0, 39000, 40000), (1, 0, 700), (1, 3000, 3000), (1, 4000, 12000), (1, 19990, 20000)]
    (d / "iv.bed").write_text("".join(f"{names[c]}\t{a}\t{b}\n" for c, a, b in ivs if a < b))
    assert run_oracle([fa, bam, "-o", "all"], cwd=d).returncode == 0
    assert run_oracle([fa, bam, "-l", d / "iv.bed", "-o", "bed"], cwd=d).returncode == 0

    def rows_of(path):
        out = []
        for f in (l.split("\t") for l in open(path).read().splitlines()[1:]):
            c, a = names.index(f[0]), int(f[1])
            out.append((c, a, int(f[2]), int(f[4]), int(f[5]), 0, 1 if seqs[c][a] == "C" else -1))
        return out
    every, inside = rows_of(d / "all_CpG.bedGraph"), rows_of(d / "bed_CpG.bedGraph")
    assert every == sorted(every) and len(every) > 1000
    assert inside == [r for r in every if any(c == r[0] and a <= r[1] < b for c, a, b in ivs)] and 200 < len(inside) < len(every)
    want = [(len(sel), sum(r[3] for r in sel), sum(r[4] for r in sel)) for sel in ([r for r in inside if r[0] == c and a <= r[1] < b and r[6] == (1 if strand == "+" else -1)] for c, a, b in ivs)]
    r, got = emu(every, ivs, strand=strand, contigs=len(names))
    assert r.returncode == 0, r.stderr
    assert got == want and sum(w[0] for w in want) > 100 and want[6] == (0, 0, 0)
    import numpy as np
    from merge_rule import DTYPES
    assert got == region_sums([np.array(c, dtype=dt) for c, dt in zip(zip(*every), DTYPES)], ivs, strand=strand)
