"""CPU-only: samples joined into one site table (csrc/mdk_unite_core.h, the functions the kernels of csrc/mdk_unite.hip run), driven
through tools/unite_emu -- the kernels' extents, bitmap words, segmented OR, block tables, ranks, tally and keep map on the host --
against a plain Python restatement (tests/unite_rule.py); and what mdk.unite refuses without a device."""
import re
import subprocess

import pytest

import methyldackel_amd as mdk
from conftest import REPO
from merge_rule import COLUMNS, DTYPES, SIZES
from unite_rule import BIG, CONTIGS, ERROR_CONTIGS, ERRORS, FAR, HAND, Disagree, combos, expected, rounds, sample_rows, unite_rows

EMU = REPO / "tools" / "_build" / "unite_emu"


def text(samples):
    return "#\n".join("".join("\t".join(str(v) for v in row) + "\n" for row in rows) for rows in samples)


def emu_text(inp, min_samples=None, min_depth=1, contigs=len(CONTIGS)):
    cmd = [str(EMU), "--contigs", str(contigs), "--min-depth", str(min_depth), "--stats"] + ([] if min_samples is None else ["--min-samples", str(min_samples)])
    r = subprocess.run(cmd, input=inp, capture_output=True, text=True)
    got = []
    for l in r.stdout.splitlines():
        v = [int(x) for x in l.split("\t")]
        got.append(tuple(v[:6]) + tuple(zip(v[6::2], v[7::2])))
    stats = re.search(r"stats: words (\d+) word_rounds (\d+) union (\d+) site_rounds (\d+) atomics (\d+)", r.stderr)
    return r, got, tuple(int(x) for x in stats.groups()) if stats else None


def emu(samples, **kw):
    return emu_text(text(samples), **kw)


@pytest.mark.parametrize("n", SIZES)
def test_seeded_tables(n):
    """every universe with every number of samples, min_samples and min_depth"""
    inputs = {}
    for S, k, d in combos(n):
        if S not in inputs:
            inputs[S] = text([sample_rows(n, s) for s in range(S)])
        r, got, stats = emu_text(inputs[S], k, d)
        assert r.returncode == 0, r.stderr
        assert got == list(expected(n, S, k, d)), (n, S, k, d)
        assert stats[2] == len(expected(n, S, 1, d))
        assert stats[1:4:2] == rounds([sample_rows(n, s) for s in range(S)], stats[2])
        if n > 1000:
            # more than 16 x 1024 words of bitmap and more than 256 x 1024 sites: k_unite_blocks takes a second round over either table
            assert stats[1] >= 2 and stats[3] >= 2, stats
            # the rows ascend, so k_unite_mark combines: fewer atomics than present rows
            assert stats[4] < sum(1 for s in range(S) for row in sample_rows(n, s) if row[3] + row[4] >= d)
    if n >= 255:
        for S in (2, 3, 5) if n < 1000 else (3,):
            assert len(expected(n, S, S, 1)) < len(expected(n, S, 1, 1)) and len(expected(n, S, 1, 5)) < len(expected(n, S, 1, 1)), (n, S)


def test_more_samples_than_lanes():
    n, S = 513, 70
    samples = [sample_rows(n, s) for s in range(S)]
    inp = text(samples)
    for k, d in ((1, 1), (52, 1), (70, 0), (45, 5)):
        r, got, _ = emu_text(inp, k, d)
        assert r.returncode == 0, r.stderr
        assert got == unite_rows(samples, k, d), (k, d)
    assert 0 < len(unite_rows(samples, 52, 1)) < len(unite_rows(samples, 1, 1)) == n


@pytest.mark.parametrize("n", [1, 257, 513])
def test_one_sample_is_its_own_rows_after_the_depth_cut(n):
    rows = sample_rows(n, 0)
    for d in (0, 1, 5):
        r, got, _ = emu([rows], min_depth=d)
        assert r.returncode == 0, r.stderr
        assert got == [(c, p, e, t, s, 1, (m, u)) for c, p, e, m, u, t, s in rows if m + u >= d]


@pytest.mark.parametrize("name,samples,kw", HAND, ids=[h[0] for h in HAND])
def test_by_hand(name, samples, kw):
    r, got, stats = emu(samples, **kw)
    assert r.returncode == 0, r.stderr
    want = unite_rows(samples, **kw)
    assert got == want
    if name == "all samples empty":
        assert got == [] and stats[0] == 0
    if name.startswith("powers of two"):
        assert stats[0] == 2 ** 16 // 32 + 1 and stats[2] == 36 and (len(want) == 36 if kw.get("min_samples") == 1 else 0 < len(want) < 36)
    if name.startswith("identical"):
        assert [row[:2] for row in got] == [row[:2] for row in samples[0]] and all(row[5] == 4 for row in got)
    if name == "disjoint samples, all":
        assert got == []
    if name.startswith("counts of INT32_MAX"):
        assert got == [(0, 5, 6, 2, 1, 2, (BIG, BIG), (0, BIG)), (0, 6, 7, 2, 1, 1, (BIG, 0), (0, 0)), (0, 7, 8, 2, 1, 2, (BIG - 1, 0), (1, BIG - 1))][:1] + \
                      [(0, 6, 7, 2, 1, 1, (BIG, 0), (0, 0)), (0, 7, 8, 2, 1, 1, (0, 0), (1, BIG - 1))]


def test_bit_offsets_past_2_32():
    name, samples, kw = FAR
    r, got, stats = emu(samples, **kw)
    assert r.returncode == 0, r.stderr
    assert got == unite_rows(samples, **kw) and len(got) == 4 and stats[0] == 2 * 2 ** 26 + 1
    assert got[2] == (1, BIG - 1, BIG, 2, 1, 2, (2, 3), (4, 5))


@pytest.mark.parametrize("name,samples,kw", ERRORS, ids=[f"{e[0]}{i}" for i, e in enumerate(ERRORS)])
def test_error_bits(name, samples, kw):
    """each refused condition alone"""
    r, got, _ = emu(samples, contigs=ERROR_CONTIGS.get(name, 2), **kw)
    assert r.returncode == 3 and r.stderr.split() == ["error:", name] and got == [], (r.returncode, r.stderr)
    if name == "disagree":
        with pytest.raises(Disagree):
            unite_rows(samples, **kw)


def test_a_disagreement_at_a_site_that_is_dropped_is_not_looked_at():
    """the comparison is made where the counts are written: at the sites of the result"""
    samples = [[(0, 10, 11, 1, 1, 0, 1), (0, 20, 21, 1, 1, 1, -1)], [(0, 10, 11, 1, 1, 0, 1)], [(0, 10, 11, 1, 1, 0, 1), (0, 20, 22, 1, 1, 1, -1)]]
    r, got, _ = emu(samples, contigs=2)
    assert r.returncode == 0 and got == unite_rows(samples) == [(0, 10, 11, 0, 1, 3, (1, 1), (1, 1), (1, 1))]
    assert emu(samples, contigs=2, min_samples=2)[0].returncode == 3


def columns(rows, contigs=("a", "b"), **kw):
    import torch
    return mdk.Calls(list(contigs), {n: torch.tensor([r[k] for r in rows], dtype=getattr(torch, dt)) for k, (n, dt) in enumerate(zip(COLUMNS, DTYPES))}, **kw)


def test_refused_without_a_device():
    import torch
    rows = [(0, 10, 11, 1, 2, 0, 1), (0, 11, 12, 3, 4, 0, -1)]
    with pytest.raises(mdk.MdkError, match="united on the device.*no CPU path"):
        mdk.unite([columns(rows), columns(rows)])
    with pytest.raises(mdk.MdkError, match="1 to 1024 samples"):
        mdk.unite([])
    with pytest.raises(mdk.MdkError, match="1 to 1024 samples"):
        mdk.unite([columns(rows)] * 1025)
    with pytest.raises(mdk.MdkError, match="takes Calls"):
        mdk.unite([columns(rows), rows])
    with pytest.raises(mdk.MdkError, match="contigs"):
        mdk.unite([columns(rows), columns(rows, ("a", "c"))])
    with pytest.raises(mdk.MdkError, match="merged"):
        mdk.unite([columns(rows), columns(rows, merged=True)])
    for k in (0, 3, -1):
        with pytest.raises(mdk.MdkError, match="min_samples"):
            mdk.unite([columns(rows), columns(rows)], min_samples=k)
    with pytest.raises(mdk.MdkError, match="min_depth"):
        mdk.unite([columns(rows)], min_depth=-1)
    bad = columns(rows)
    bad.nmeth = bad.nmeth.to(torch.int64)
    with pytest.raises(mdk.MdkError, match="sample 1: the nmeth column must be a contiguous int32"):
        mdk.unite([columns(rows), bad])
    bad = columns(rows)
    bad.strand = bad.strand[:1]
    with pytest.raises(mdk.MdkError, match="strand column.*one entry per row"):
        mdk.unite([bad])
    bad = columns(rows + rows)
    bad.start = bad.start[::2]
    bad.contig, bad.end, bad.nmeth, bad.nunmeth, bad.context, bad.strand = (getattr(bad, n)[:2] for n in ("contig", "end", "nmeth", "nunmeth", "context", "strand"))
    with pytest.raises(mdk.MdkError, match="start column must be a contiguous"):
        mdk.unite([bad])
    assert {"md_text_unite_measure", "md_text_unite_fill"} <= set(mdk.HIP_SYMBOLS)
