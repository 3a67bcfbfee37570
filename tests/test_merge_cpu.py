"""CPU-only: mergeContext over rows (csrc/mdk_merge_core.h, the function k_merge_len and k_merge_fill of csrc/mdk_merge.hip run), driven
through tools/merge_emu -- the kernels' 256-row blocking, halo rows and two passes on the host -- against the oracle's `extract --mergeContext`,
this build's `mergeContext` tool and a plain Python restatement (tests/merge_rule.py); and what Calls.merge_context refuses without a device."""
import subprocess

import pytest

import methyldackel_amd as mdk
from conftest import REPO, run_oracle
from merge_rule import BIG, ERRORS, SIZES, crosses_contigs, expected, merge_rows, pairs, table_rows

EMU = REPO / "tools" / "_build" / "merge_emu"
CTX = ("CpG", "CHG", "CHH")


def emu(rows, *args):
    r = subprocess.run([str(EMU)] + [str(a) for a in args], input="".join("\t".join(str(v) for v in row) + "\n" for row in rows), capture_output=True, text=True)
    return r, [tuple(int(v) for v in l.split("\t")) for l in r.stdout.splitlines()]


def bedgraph(path, contigs):
    """(contig index, start, end, nmeth, nunmeth) of every line behind the header"""
    return [(contigs[f[0]], int(f[1]), int(f[2]), int(f[4]), int(f[5])) for f in (l.split("\t") for l in open(path).read().splitlines()[1:])]


@pytest.fixture(scope="module")
def sample(tmp_path_factory, small_synth):
    """the oracle's per-strand files of small_synth/pe in all contexts as one ascending table (strand from the FASTA), and its merged files"""
    d = tmp_path_factory.mktemp("merge")
    fa, bam = small_synth / "pe.fa", small_synth / "pe.bam"
    assert run_oracle([fa, bam, "--CHG", "--CHH", "-o", "s"], cwd=d).returncode == 0
    assert run_oracle([fa, bam, "--CHG", "--CHH", "--mergeContext", "-o", "m"], cwd=d).returncode == 0
    assert run_oracle([fa, bam, "--CHG", "--CHH", "--mergeContext", "-d", "10", "-o", "m10"], cwd=d).returncode == 0
    names, seqs = [], {}
    for l in open(fa).read().splitlines():
        if l.startswith(">"):
            names.append(l[1:].split()[0]); seqs[names[-1]] = []
        else:
            seqs[names[-1]].append(l.upper())
    seqs = ["".join(seqs[n]) for n in names]
    contigs = {n: i for i, n in enumerate(names)}
    rows = []
    for t, ctx in enumerate(CTX):
        for c, a, b, m, u in bedgraph(d / f"s_{ctx}.bedGraph", contigs):
            assert seqs[c][a] in "CG"
            rows.append((c, a, b, m, u, t, 1 if seqs[c][a] == "C" else -1))
    rows.sort()
    assert all(x[:2] < y[:2] for x, y in zip(rows, rows[1:]))
    return d, fa, names, contigs, rows


@pytest.mark.parametrize("depth,prefix", [(1, "m"), (10, "m10")])
def test_rule_equals_the_oracles_mergecontext(sample, depth, prefix):
    d, _, _, contigs, rows = sample
    p = pairs(rows)
    assert len(p) > 2000 and any((i + 1) % 256 == 0 for i in p), (len(p), "no pair across a 256-row boundary")
    r, got = emu(rows, "--min-depth", depth)
    assert r.returncode == 0, r.stderr
    assert got == merge_rows(rows, depth)
    for t, ctx in enumerate(CTX):
        want = bedgraph(d / f"{prefix}_{ctx}.bedGraph", contigs)
        assert [g[:5] for g in got if g[5] == t] == want and len(want) > 500, ctx
        assert all(g[6] == (0 if t < 2 else g[6]) and g[6] in (-1, 0, 1) for g in got if g[5] == t)


@pytest.mark.parametrize("t,ctx", list(enumerate(CTX)))
def test_rule_equals_the_mergecontext_tool(sample, tmp_path, t, ctx):
    d, fa, names, _, rows = sample
    r, got = emu(rows)
    assert r.returncode == 0, r.stderr
    tool = subprocess.run([str(mdk.CLI), "mergeContext", str(fa), str(d / f"s_{ctx}.bedGraph")], cwd=tmp_path, capture_output=True, text=True)
    assert tool.returncode == 0, tool.stderr
    lines = ["%s\t%d\t%d\t%d\t%d\t%d" % (names[c], a, b, int(100.0 * float(m) / (m + u)), m, u) for c, a, b, m, u, x, _ in got if x == t]
    assert lines == tool.stdout.splitlines()[1:] and len(lines) > 500


@pytest.mark.parametrize("n", SIZES)
def test_blocking(n):
    rows = list(table_rows(n))
    if n >= 255:
        assert crosses_contigs(rows) and len({r[0] for r in rows}) == 3
        assert len(pairs(rows)) > n // 20
    for depth in (1, 5, 0) if n < 1000 else (1, 5):
        r, got = emu(rows, "--min-depth", depth, "--contigs", 3)
        assert r.returncode == 0, r.stderr
        assert got == (list(expected(n, depth)) if depth else merge_rows(rows, 0)), (n, depth)
    if n >= 255:
        assert 0 < len(expected(n, 5)) < len(expected(n, 1)) < n


def test_a_c_and_a_g_in_different_contigs_stay_apart():
    rows = [(0, 10, 11, 1, 2, 0, 1), (1, 11, 12, 3, 4, 0, -1)]
    assert emu(rows)[1] == [(0, 10, 12, 1, 2, 0, 0), (1, 10, 12, 3, 4, 0, 0)]
    # the same two in one contig are one row; a CHG pair; a CHG G behind a CpG C is not its partner
    assert emu([(0, 10, 11, 1, 2, 0, 1), (0, 11, 12, 3, 4, 0, -1)])[1] == [(0, 10, 12, 4, 6, 0, 0)]
    assert emu([(0, 10, 11, 1, 2, 1, 1), (0, 12, 13, 3, 4, 1, -1)])[1] == [(0, 10, 13, 4, 6, 1, 0)]
    assert emu([(0, 10, 11, 1, 2, 0, 1), (0, 12, 13, 3, 4, 1, -1)])[1] == [(0, 10, 12, 1, 2, 0, 0), (0, 10, 13, 3, 4, 1, 0)]
    # the depth cut looks at the merged counts, and cuts CHH rows too
    assert emu([(0, 10, 11, 1, 2, 0, 1), (0, 11, 12, 3, 4, 0, -1), (0, 20, 21, 2, 2, 2, -1)], "--min-depth", 5)[1] == [(0, 10, 12, 4, 6, 0, 0)]


@pytest.mark.parametrize("name,rows", ERRORS, ids=[f"{e[0]}{i}" for i, e in enumerate(ERRORS)])
def test_error_bits(name, rows):
    """each refused condition alone, in a small table with good rows around it (and at a workgroup's edge: row 256 looks at row 255)"""
    good = [(0, k, k + 1, 1, 1, 2, 1) for k in range(2, 8)]
    r, got = emu(rows, "--contigs", 2)
    assert r.returncode == 3 and r.stderr.split() == ["error:", name] and got == [], (r.returncode, r.stderr)
    pad = [(0, k, k + 1, 1, 1, 2, 1) for k in range(256 - len(rows) + 1)]
    shifted = [(c, a + 1000, b + 1000, m, u, t, s) for c, a, b, m, u, t, s in rows]
    if name not in ("lone_g", "contig") and rows[0][0] == 0:
        r, _ = emu(pad + shifted, "--contigs", 2)
        assert r.returncode == 3 and r.stderr.split() == ["error:", name], (r.returncode, r.stderr)
    assert emu(good, "--contigs", 2)[0].returncode == 0
    # just inside: the largest sum, a G at q == d
    assert emu([(0, 10, 11, BIG - 1, 0, 0, 1), (0, 11, 12, 1, 0, 0, -1)])[1] == [(0, 10, 12, BIG, 0, 0, 0)]
    assert emu([(0, 2, 3, 1, 1, 1, -1)])[1] == [(0, 0, 3, 1, 1, 1, 0)]


def columns(rows, merged=False):
    import torch
    from merge_rule import COLUMNS, DTYPES
    cols = {n: torch.tensor([r[k] for r in rows], dtype=getattr(torch, dt)) for k, (n, dt) in enumerate(zip(COLUMNS, DTYPES))}
    return mdk.Calls(["a", "b"], cols, merged=merged)


def test_refused_without_a_device():
    rows = [(0, 10, 11, 1, 2, 0, 1), (0, 11, 12, 3, 4, 0, -1)]
    with pytest.raises(mdk.MdkError, match="merged already"):
        columns([(0, 10, 12, 4, 6, 0, 0)], merged=True).merge_context()
    with pytest.raises(mdk.MdkError, match="no CPU path"):
        columns(rows).merge_context()
    with pytest.raises(mdk.MdkError, match="min_depth"):
        columns(rows).merge_context(min_depth=-1)
    assert "md_text_merge_measure" in mdk.HIP_SYMBOLS and "md_text_merge_fill" in mdk.HIP_SYMBOLS
