"""CPU-only: the text parser (csrc/mdk_parse_core.h, the functions k_parse_len and k_parse_fill of csrc/mdk_parse.hip run), driven through
tools/parse_emu -- the kernels' 4096-byte spans, look-ahead, rounds of 256 and two passes on the host -- against a bytes.split restatement
(tests/parse_rule.py) and, through tools/merge_emu, against this build's `mergeContext` command; the FASTA behind mdk.Reference; and what
Calls.read / Cytosines.read refuse without a device.  Every comparison is exact."""
import subprocess

import pytest

import methyldackel_amd as mdk
import parse_rule as R
from conftest import REPO, run_oracle

EMU = REPO / "tools" / "_build" / "parse_emu"
MERGE_EMU = REPO / "tools" / "_build" / "merge_emu"
CTX = ("CpG", "CHG", "CHH")


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    d = tmp_path_factory.mktemp("parse_tables")
    (d / "with_bases").write_bytes(R.contigs_file(True)); (d / "names_only").write_bytes(R.contigs_file(False))
    return d


def emu(text, fmt, contigs_path):
    r = subprocess.run([str(EMU), "report" if fmt == R.REPORT else "bedgraph", str(contigs_path)], input=text, capture_output=True)
    rows = [tuple(v.decode() if fmt == R.REPORT and k == 6 else int(v) for k, v in enumerate(l.split(b"\t"))) for l in r.stdout.splitlines()]
    return r, rows


def refused(r):
    """(the names behind `error:`, the first refusal, its offset, its message) of a run that ended with 3"""
    e = r.stderr.decode().splitlines()
    return ({l.split()[1] for l in e if l.startswith("error:")}, next(l.split()[1] for l in e if l.startswith("first:")),
            int(next(l.split()[1] for l in e if l.startswith("offset:"))), next(l.split(" ", 1)[1] for l in e if l.startswith("message:")))


@pytest.fixture(scope="module")
def sample(tmp_path_factory, small_synth):
    """the oracle's per-strand files of small_synth/pe in all contexts at -d 1, its cytosine report, and the sample's contigs as parse_emu takes them"""
    d = tmp_path_factory.mktemp("parse")
    fa, bam = small_synth / "pe.fa", small_synth / "pe.bam"
    assert run_oracle([fa, bam, "--CHG", "--CHH", "-d", "1", "-o", "s"], cwd=d).returncode == 0
    assert run_oracle([fa, bam, "--CHG", "--CHH", "--cytosine_report", "-o", "r"], cwd=d).returncode == 0
    ref = mdk.Reference(fa)
    (d / "contigs").write_bytes(b"".join(n.encode() + b"\t" + ref.bases(i) + b"\n" for i, n in enumerate(ref.contigs)))
    return d, fa, ref


@pytest.mark.parametrize("ctx", CTX)
def test_emulator_equals_the_restatement_on_a_samples_files(sample, ctx):
    d, _, ref = sample
    text = (d / f"s_{ctx}.bedGraph").read_bytes()
    want, bad = R.parse_text(text, R.BEDGRAPH, ref.contigs, [ref.bases(i) for i in range(len(ref.contigs))])
    r, got = emu(text, R.BEDGRAPH, d / "contigs")
    assert r.returncode == 0 and not bad, (r.stderr, bad[:3])
    assert got == want and len(got) == text.count(b"\n") - 1 > 500
    assert {g[5] for g in got} == {CTX.index(ctx)} and {g[6] for g in got} == {1, -1}


def test_emulator_equals_the_restatement_on_a_cytosine_report(sample):
    d, _, ref = sample
    text = (d / "r.cytosine_report.txt").read_bytes()
    want, bad = R.parse_text(text, R.REPORT, ref.contigs)
    r, got = emu(text, R.REPORT, d / "contigs")
    assert r.returncode == 0 and not bad, (r.stderr, bad[:3])
    assert got == want and len(got) == text.count(b"\n") > 10000
    assert {g[5] for g in got} == {0, 1, 2}


@pytest.mark.parametrize("ctx", CTX)
def test_emulator_then_merge_equals_the_command(sample, tmp_path, ctx):
    d, fa, ref = sample
    path = d / f"s_{ctx}.bedGraph"
    r, got = emu(path.read_bytes(), R.BEDGRAPH, d / "contigs")
    assert r.returncode == 0, r.stderr
    m = subprocess.run([str(MERGE_EMU), "--min-depth", "0", "--contigs", str(len(ref.contigs))], input="".join("\t".join(str(v) for v in row) + "\n" for row in got), capture_output=True, text=True)
    assert m.returncode == 0, m.stderr
    tool = subprocess.run([str(mdk.CLI), "mergeContext", str(fa), str(path)], cwd=tmp_path, capture_output=True, text=True)
    assert tool.returncode == 0, tool.stderr
    lines = []
    for l in m.stdout.splitlines():
        c, a, b, nm, nu = [int(v) for v in l.split("\t")[:5]]
        lines.append("%s\t%d\t%d\t%d\t%d\t%d" % (ref.contigs[c], a, b, int(100.0 * float(nm) / (nm + nu)), nm, nu))
    assert lines == tool.stdout.splitlines()[1:] and len(lines) > 500


@pytest.mark.parametrize("name", list(R.blocking()))
def test_blocking(tables, name):
    text = R.blocking()[name]
    r, got = emu(text, R.BEDGRAPH, tables / "with_bases")
    assert r.returncode == 0, (name, r.stderr)
    assert got == list(R.expected(name)), name
    if name not in ("empty", "header only", "header only, no newline"):
        assert len(got) >= 1


def test_blocking_texts_are_what_their_names_say():
    b = R.blocking()
    S = R.SPAN
    assert b["a line starts at byte 4096, a newline ends the span"][S - 1:S] == b"\n"
    assert b["and at 8192"][2 * S - 1:2 * S] == b"\n"
    assert b"\n" not in b["a line straddles two spans"][S - 9:S + 3]
    assert b["track at 4094"][S - 2:S + 3] == b"track" and b["track at 4092"][S - 4:S + 1] == b"track"
    t = b["a 512-byte line over the edge"]
    assert t[S - 201:S - 200] == b"\n" and t.find(b"\n", S - 200) == S - 200 + 511
    t = b["a 512-byte line from the span's last byte"]
    assert t[S - 2:S - 1] == b"\n" and t.find(b"\n", S - 1) == S - 1 + 511
    t = b["a 512-byte line ends the text without a newline"]
    assert len(t) == S - 1 + 512 and not t.endswith(b"\n")
    assert S < len(b["the look-ahead passes the end"]) < S + 64 and len(b["the text ends with the span"]) == S
    assert not b["no final newline"].endswith(b"\n") and b["crlf"].count(b"\r\n") == b["crlf"].count(b"\n") == 41
    assert len(R.expected("tracks in between")) == 80 and len(R.expected("1025 spans")) > 200000


def test_a_span_of_newlines_is_refused_not_crashed(tables):
    """4096 one-byte lines in a span: sixteen times the 256 lanes' worth of line starts, every one an empty line"""
    text = b"\n" * R.SPAN + R.bed_lines(1)[0]
    r, got = emu(text, R.BEDGRAPH, tables / "with_bases")
    assert r.returncode == 3 and got == []
    assert refused(r)[:3] == ({"empty"}, "empty", 0)
    # and 2048 two-byte lines that are rows of too few fields, the good line behind them not among the refused
    text = b"x\n" * (R.SPAN // 2) + R.bed_lines(1)[0]
    r, _ = emu(text, R.BEDGRAPH, tables / "with_bases")
    assert r.returncode == 3 and refused(r)[:3] == ({"few"}, "few", 0)
    assert R.parse_text(text, R.BEDGRAPH, R.CONTIGS, R.reference())[1] == [(2 * k, "few") for k in range(R.SPAN // 2)]


REFUSALS = R.refusals()


@pytest.mark.parametrize("ident,name,fmt,bad", REFUSALS, ids=[x[0] for x in REFUSALS])
def test_refusals(tables, ident, name, fmt, bad):
    """every refusal on its own between good lines, and as the line that straddles a span edge: the bit, the offset and the message"""
    import re
    for edge in (False, True):
        text, at = R.around(bad, fmt, edge)
        assert R.parse_text(text, fmt, R.CONTIGS, R.reference())[1] == [(at, name)]
        r, got = emu(text, fmt, tables / "with_bases")
        assert r.returncode == 3 and got == [], (r.returncode, r.stderr)
        names, first, offset, message = refused(r)
        assert (names, first, offset) == ({name}, name, at), (edge, r.stderr)
        assert re.search(R.MESSAGES[name], message), message
        # the same text without the bad line is taken
        good = text[:at] + text[at + len(bad):]
        assert emu(good, fmt, tables / "with_bases")[0].returncode == 0


def test_two_refusals_name_the_earlier_line(tables):
    a, b = R.bed_line(0, R.other_base(0), 1, 1), b"zz\t1\t2\t0\t1\t1\n"
    text = R.fill(R.SPAN + 100) + b + R.fill(3 * R.SPAN, 5) + a
    r, _ = emu(text, R.BEDGRAPH, tables / "with_bases")
    assert r.returncode == 3 and refused(r)[:3] == ({"contig", "base"}, "contig", R.SPAN + 100)


def test_without_resident_bases(tables):
    text = b"".join(R.bed_lines(3))
    r, _ = emu(text, R.BEDGRAPH, tables / "names_only")
    assert r.returncode == 3 and refused(r)[:3] == ({"noref"}, "noref", 0)
    assert R.parse_text(text, R.BEDGRAPH, R.CONTIGS, None)[1][0] == (0, "noref")
    # a report needs none
    rep = R.report_line(2, 9, b"-", 0, 0, b"CG", b"CGN")
    r, got = emu(rep, R.REPORT, tables / "names_only")
    assert r.returncode == 0 and got == [(2, 9, -1, 0, 0, 0, "CGN")]


def test_stricter_than_the_command(tables, tmp_path):
    """`+5`, ` 5`, doubled tabs and a seventh column are refused, although the command takes them"""
    (tmp_path / "ref.fa").write_bytes(R.fasta_text())
    p = R.cytosines(0)[5]
    n0 = R.CONTIGS[0].encode()
    good = R.bed_line(0, p, 3, 4)
    for bad, name in ((b"%s\t+%d\t%d\t42\t3\t4\n" % (n0, p, p + 1), "digit"), (b"%s\t %d\t%d\t42\t3\t4\n" % (n0, p, p + 1), "digit"),
                      (good.replace(b"\t", b"\t\t", 1), "many"), (good[:-1] + b"\t9\n", "many")):
        (tmp_path / "in.bedGraph").write_bytes(bad)
        tool = subprocess.run([str(mdk.CLI), "mergeContext", str(tmp_path / "ref.fa"), str(tmp_path / "in.bedGraph")], cwd=tmp_path, capture_output=True, text=True)
        assert tool.returncode == 0 and len(tool.stdout.splitlines()) == 2, (bad, tool.stderr)          # the command prints the site
        r, _ = emu(bad, R.BEDGRAPH, tables / "with_bases")
        assert r.returncode == 3 and refused(r)[:3] == ({name}, name, 0), bad


def test_reference(tmp_path, small_synth):
    fa = small_synth / "pe.fa"
    ref = mdk.Reference(fa)
    # the sample ships no .fai (this build never writes one): its first two columns, NAME and LENGTH, made here from the file's text
    fai = []
    for l in open(fa, "rb").read().splitlines():
        if l.startswith(b">"):
            fai.append([l[1:].split()[0].decode(), 0])
        else:
            fai[-1][1] += len(l.strip())
    assert ref.contigs == [f[0] for f in fai] and ref.lengths == [f[1] for f in fai] == [40000, 20000]         # (conftest: -L 40000,20000)
    assert ref.bases(1) == b"".join(open(fa, "rb").read().split(b">")[2].splitlines()[1:])
    ref.close(); ref.close()
    with pytest.raises(mdk.MdkError, match="closed"):
        ref.bases(0)
    # a wrapped multi-contig file with lower case and N, names cut at the first blank
    (tmp_path / "ref.fa").write_bytes(R.fasta_text())
    with mdk.Reference(tmp_path / "ref.fa") as ref:
        assert ref.contigs == R.CONTIGS and ref.lengths == list(R.LENGTHS)
        assert tuple(ref.bases(i) for i in range(3)) == R.reference()
        assert any(c in R.reference()[0] for c in b"acgtn") and b"N" in R.reference()[2]
    with pytest.raises(mdk.MdkError, match="cannot read"):
        mdk.Reference(tmp_path / "none.fa")


def test_refused_without_a_device(tmp_path):
    if mdk.lib_hip().md_dev_count() > 0:
        return
    (tmp_path / "ref.fa").write_bytes(R.fasta_text())
    (tmp_path / "x.bedGraph").write_bytes(R.HEADER + b"".join(R.bed_lines(3)))
    with mdk.Reference(tmp_path / "ref.fa") as ref:
        with pytest.raises(mdk.MdkError, match="no CPU path"):
            mdk.Calls.read(tmp_path / "x.bedGraph", ref)
    with pytest.raises(mdk.MdkError, match="no CPU path"):
        mdk.Cytosines.read(tmp_path / "x.cytosine_report.txt", R.CONTIGS)
    for s in ("md_text_reference", "md_text_parse_measure", "md_text_parse_fill_calls", "md_text_parse_fill_cytosines", "md_text_parse_error_offset"):
        assert s in mdk.HIP_SYMBOLS
