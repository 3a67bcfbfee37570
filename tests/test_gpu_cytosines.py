"""GPU: Session.cytosine_report on the MI355X -- k_cyto_count / k_cyto_fill / k_cyto_gather (csrc/mdk_cytosines.hip), the cytosine sink of
the extract pipeline, md_dev_reset between runs.  Every comparison is of all seven fields of every row, in order, against the parsed lines
of <prefix>.cytosine_report.txt written by this build's own command on the same arguments and, where noted, by the oracle.

As in test_gpu_calls.py the session is opened after torch has put a tensor on the device."""
import os
import resource

import pytest

from bamwriter import record, write_bam, write_fasta
from conftest import GOLDEN, run_oracle, synth

pytestmark = pytest.mark.gpu
COLS = ("contig", "pos", "strand", "nmeth", "nunmeth", "context", "trinucleotide")


def report_rows(path):
    rows = []
    for l in path.read_text().splitlines():
        t = l.split("\t")
        assert len(t) == 7, l
        rows.append((t[0], int(t[1]), t[2], int(t[3]), int(t[4]), t[5], t[6]))
    return rows


def cli_report(tmp, args, name, env=None):
    import methyldackel_amd as mdk
    d = tmp / name; d.mkdir()
    r = mdk.run_cli([str(a) for a in args] + ["--cytosine_report", "-o", "out"], cwd=d, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    return report_rows(d / "out.cytosine_report.txt")


def oracle_report(tmp, args, name):
    d = tmp / name; d.mkdir()
    r = run_oracle([str(a) for a in args] + ["--cytosine_report", "-o", "out"], cwd=d)
    assert r.returncode == 0, r.stderr[-800:]
    return report_rows(d / "out.cytosine_report.txt")


def same(c, want):
    got = c.rows()
    assert len(c) == len(got) == len(want), (len(c), len(got), len(want))
    assert got == want, next((i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b)
    return len(got)


def both_kinds(rows):
    return any(r[3] + r[4] == 0 for r in rows) and any(r[3] + r[4] > 0 for r in rows)


def with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def fasta_cytosines(path, ctx_on):
    """(contig index, 1-based position, strand, context) of every cytosine of the FASTA in the contexts switched on: the classification
    of common.c:49-82 written out independently -- a C looks one and two bases ahead for a G, a G one and two bases back for a C, and a
    contig's ends cut that short"""
    seqs = []
    for l in open(path):
        if l.startswith(">"):
            seqs.append([]); continue
        seqs[-1].append(l.strip().upper())
    out = []
    for k, parts in enumerate(seqs):
        s = "".join(parts); n = len(s)
        for i, ch in enumerate(s):
            if ch == "C":
                x = 0 if i + 1 < n and s[i + 1] == "G" else 1 if i + 2 < n and s[i + 2] == "G" else 2
                if ctx_on[x]:
                    out.append((k, i + 1, 1, x))
            elif ch == "G":
                x = 0 if i >= 1 and s[i - 1] == "C" else 1 if i >= 2 and s[i - 2] == "C" else 2
                if ctx_on[x]:
                    out.append((k, i + 1, -1, x))
    return out


@pytest.fixture(scope="module")
def session():
    import torch
    import methyldackel_amd as mdk
    x = torch.arange(1 << 20, device="cuda", dtype=torch.int64)          # torch's runtime is up and has a live allocation first
    assert int(x.sum().item()) == (1 << 20) * ((1 << 20) - 1) // 2
    s = mdk.Session(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def sdata(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_cyto")
    synth(d / "s", "-L", "90000,40000", "-c", "8", "-s", "51", "--extras", "--bbm", "--bw")
    return d


def test_tensors(session, tmp_path):
    """dtypes, the [len, 3] trinucleotide, the device, and every column equal to its device_tensors=False copy; the rows are the golden
    file's 99 (the 99 C/G of the 100-base contig), 50 of them 0 0"""
    import torch
    args = [GOLDEN / "cg100.fa", GOLDEN / "cg_aln.bam", "-q", "2", "--CHG", "--CHH"]
    c = session.cytosine_report(args)
    h = session.cytosine_report(args, device_tensors=False)
    want = {"contig": torch.int32, "pos": torch.int32, "strand": torch.int8, "nmeth": torch.int32, "nunmeth": torch.int32, "context": torch.uint8, "trinucleotide": torch.uint8}
    for name in COLS:
        a, b = getattr(c, name), getattr(h, name)
        assert a.device == torch.device("cuda", 0) and b.device.type == "cpu", name
        assert a.dtype == b.dtype == want[name] and a.shape == b.shape, name
        assert torch.equal(a.cpu(), b), name
    assert tuple(c.trinucleotide.shape) == (len(c), 3) and tuple(c.pos.shape) == (len(c),)
    golden = report_rows(GOLDEN / "expected" / "extract_cg_cytosine_report.out.cytosine_report.txt")
    assert same(c, golden) == 99 and sum(1 for r in golden if r[3] + r[4] == 0) == 50
    assert c.contigs == ["chrCG"]


FIXTURES = [
    ("cg100.fa", "cg_aln.bam", ["-q", "2", "--CHG", "--CHH"]), ("ct100.fa", "ct_aln.bam", ["-q", "2"]),
    ("chgchh.fa", "chgchh_aln.bam", ["-q", "5", "--CHG", "--CHH", "--chunkSize", "3"]),
    ("cg100.fa", "cg_with_variants.bam", ["-p", "1", "-q", "0", "--minOppositeDepth", "3", "--maxVariantFrac", "0.25"]),
    ("cg100.fa", "cg_aln.bam", ["-q", "2", "-r", "chrCG:10-50", "--chunkSize", "7"]),
]


@pytest.mark.parametrize("fa,bam,extra", FIXTURES)
def test_fixtures_equal_cli_and_oracle(session, tmp_path, fa, bam, extra):
    args = [GOLDEN / fa, GOLDEN / bam] + extra
    c = session.cytosine_report(args)
    n = same(c, cli_report(tmp_path, args, "cli"))
    assert same(c, oracle_report(tmp_path, args, "oracle")) == n
    if (fa, bam) == ("cg100.fa", "cg_aln.bam") and "-r" not in extra:
        assert same(c, report_rows(GOLDEN / "expected" / "extract_cg_cytosine_report.out.cytosine_report.txt")) == 99
    if fa != "ct100.fa":
        assert n > 0


SYNTH = [
    ([], {}), (["--CHG", "--CHH"], {}), (["--noCpG", "--CHH"], {}), (["-d", "5"], {}), (["-r", "chrS1:5000-30000"], {}),
    (["-l", "BED"], {}), (["-l", "BED", "--keepStrand", "--CHH", "--chunkSize", "5000"], {}), (["-M", "BW", "-t", "0.6", "-b", "100"], {}),
    (["--OT", "6,146,6,146"], {}), (["--chunkSize", "100"], {}), (["--chunkSize", "7000", "--minOppositeDepth", "2", "--maxVariantFrac", "0.2"], {}),
    ([], {"MDK_HOST_PREP": "1"}), ([], {"MDK_TILE": "512"}), ([], {"MDK_GROUPS_IN_FLIGHT": "2"}),
]


@pytest.mark.parametrize("extra,env", SYNTH)
def test_synthetic_equal_cli(session, sdata, tmp_path, extra, env):
    """every row equals the command's; zero-count and non-zero rows are both there; without -l / -r the rows are exactly the cytosines of
    the FASTA in the contexts switched on, counted here; -d changes nothing"""
    import torch
    bed = tmp_path / "r.bed"
    bed.write_text("chrS1\t1000\t30000\t.\t0\t+\nchrS1\t50000\t70000\t.\t0\t-\nchrS2\t500\t20000\t.\t0\t.\n")
    sub = {"BED": str(bed), "BW": str(sdata / "s.bw")}
    args = [sdata / "s.fa", sdata / "s.bam", "-@", "4"] + [sub.get(e, e) for e in extra]
    c = with_env(env, lambda: session.cytosine_report(args))
    want = cli_report(tmp_path, args, "cli", env=env)
    assert same(c, want) > 0
    assert both_kinds(want)
    if "-l" not in extra and "-r" not in extra:
        on = [int("--noCpG" not in extra), int("--CHG" in extra), int("--CHH" in extra)]
        cyt = fasta_cytosines(sdata / "s.fa", on)
        assert len(c) == len(cyt)
        got = list(zip(c.contig.cpu().tolist(), c.pos.cpu().tolist(), c.strand.cpu().tolist(), c.context.cpu().tolist()))
        assert got == cyt, next((i, a, b) for i, (a, b) in enumerate(zip(got, cyt)) if a != b)
    if "-d" in extra:
        plain = session.cytosine_report([a for a in args if str(a) not in ("-d", "5")])
        for name in COLS:
            assert torch.equal(getattr(c, name), getattr(plain, name)), name


def test_bed_chunk_lists_every_cytosine(session, sdata, tmp_path):
    """under -l a 5000-base chunk that a BED interval touches reports all its cytosines, on both strands, even with --keepStrand: the rows
    of chrS1 start before the first interval and both strands appear inside the '+' interval"""
    bed = tmp_path / "r.bed"
    bed.write_text("chrS1\t1000\t8000\t.\t0\t+\nchrS1\t12000\t20000\t.\t0\t-\nchrS2\t500\t4000\t.\t0\t.\n")
    args = [sdata / "s.fa", sdata / "s.bam", "-l", bed, "--keepStrand", "--CHH", "--chunkSize", "5000"]
    c = session.cytosine_report(args)
    want = cli_report(tmp_path, args, "cli")
    same(c, want)
    s1 = [r for r in want if r[0] == "chrS1"]
    assert s1[0][1] < 1000 and s1[-1][1] > 19000 and s1[-1][1] <= 20000
    assert {r[2] for r in s1 if 1000 < r[1] <= 8000} == {"+", "-"}
    assert all(r[3] + r[4] == 0 for r in s1 if r[1] <= 1000) and any(r[3] + r[4] > 0 for r in s1)


def test_reference_quirks(session, tmp_path):
    """lower case, N runs, IUPAC letters, and C/G in the first and last two bases of a contig: contexts and trinucleotides there equal the
    command's (and the oracle's)"""
    ref1 = "GCgcNNNNacgtRYKMcgnCGNcatgSWCCGGccggBDHVcNgNNcGaCtCCCGGGttagcnnnnnCGCGcatCAGcTGG" + "acgtTGCAacgtCCGGaattNNCG" * 8 + "AGC"
    ref2 = "CG" + "TTACGGATCCNNgcatCWGG" * 6 + "GC"
    write_fasta(tmp_path / "q.fa", [("q1", ref1), ("q2", ref2)])
    up = lambda s: "".join(ch if ch in "ACGT" else "N" for ch in s.upper())
    recs = [record(0, p, 0, "30M", up(ref1[p:p + 30]).replace("C", "T", 1), 40, qname=f"a{p}") for p in range(0, len(ref1) - 30, 7)]
    recs += [record(1, p, 16, "30M", up(ref2[p:p + 30]), 40, qname=f"b{p}") for p in range(0, len(ref2) - 30, 11)]
    write_bam(tmp_path / "q.bam", [("q1", len(ref1)), ("q2", len(ref2))], recs)
    for k, extra in enumerate((["--CHG", "--CHH"], ["--CHG", "--CHH", "--chunkSize", "5"], ["--noCpG", "--CHG"])):
        args = [tmp_path / "q.fa", tmp_path / "q.bam", "-q", "0", "-p", "1"] + extra
        c = session.cytosine_report(args)
        want = cli_report(tmp_path, args, f"cli{k}")
        same(c, want)
        same(c, oracle_report(tmp_path, args, f"oracle{k}"))
        if k == 0:
            assert both_kinds(want)
            tri = {r[6] for r in want}
            assert any("N" in t for t in tri) and (want[0][0], want[0][1]) == ("q1", 1) and want[-1][1] == len(ref2)
            assert [r[:3] for r in want if r[0] == "q1"][:2] == [("q1", 1, "-"), ("q1", 2, "+")]


def test_chunks_without_reads(session, tmp_path):
    """a contig of the header without a read; a read-free stretch several chunks long; a contig the FASTA lacks (it gives no rows)"""
    import random
    rnd = random.Random(5)
    a, b, x = ("".join(rnd.choice("ACGT") for _ in range(n)) for n in (6000, 900, 700))
    write_fasta(tmp_path / "n.fa", [("a", a), ("b", b)])
    recs = [record(0, p, 0, "50M", a[p:p + 50], 40, qname=f"r{p}") for p in list(range(0, 400, 9)) + list(range(5200, 5900, 13))]
    write_bam(tmp_path / "one.bam", [("a", len(a)), ("b", len(b))], recs)
    write_bam(tmp_path / "lack.bam", [("a", len(a)), ("x", len(x)), ("b", len(b))], recs + [record(1, 10, 0, "50M", x[10:60], 40, qname="rx"), record(2, 100, 16, "50M", b[100:150], 40, qname="rb")])
    for k, (bam, extra) in enumerate((("one.bam", ["--chunkSize", "500"]), ("one.bam", ["--CHG", "--CHH", "--chunkSize", "300"]), ("lack.bam", ["--chunkSize", "500", "--CHH"]))):
        args = [tmp_path / "n.fa", tmp_path / bam, "-q", "0"] + extra
        c = session.cytosine_report(args)
        want = cli_report(tmp_path, args, f"cli{k}")
        same(c, want)
        assert both_kinds(want)
        names = {r[0] for r in want}
        assert "b" in names and "x" not in names
        if bam == "one.bam":      # every cytosine of both contigs, read or no read
            on = [1, int("--CHG" in extra), int("--CHH" in extra)]
            assert len(c) == len(fasta_cytosines(tmp_path / "n.fa", on))
            assert all(r[3] + r[4] == 0 for r in want if r[0] == "b" or 1000 < r[1] <= 5000)


def test_aligned_rows_across_samples(session):
    """three BAM files against one reference with the same options: the row set is the reference's, so everything but the counts is equal
    column for column"""
    import torch
    res = [session.cytosine_report([GOLDEN / "cg100.fa", GOLDEN / bam, "-q", "0", "--CHG", "--CHH"]) for bam in ("cg_aln.bam", "cg_with_variants.bam", "NH.bam")]
    for other in res[1:]:
        for name in ("contig", "pos", "strand", "context", "trinucleotide"):
            assert torch.equal(getattr(res[0], name), getattr(other, name)), name
    m = torch.stack([r.nmeth for r in res])
    assert tuple(m.shape) == (3, len(res[0])) and len(res[0]) == 99
    assert not torch.equal(m[0], m[1]) or not torch.equal(m[0], m[2]) or not torch.equal(m[1], m[2])


def test_one_session_every_command(session, sdata, tmp_path):
    """mbias, extract, cytosine_report, perRead and cytosine_report again with other options on one handle: each equals a fresh command;
    extract still refuses --cytosine_report in between, and the session works afterwards"""
    import methyldackel_amd as mdk
    from test_gpu_bias import compare
    from test_gpu_calls import cli_rows, same as same_calls
    from test_gpu_reads import cli_text, render
    base = [sdata / "s.fa", sdata / "s.bam"]
    compare(session, tmp_path, base, "mb")
    same_calls(session.extract(base + ["--CHG"]), cli_rows(tmp_path, base + ["--CHG"], "x0"))
    a1 = base + ["--CHG", "--chunkSize", "30000"]
    same(session.cytosine_report(a1), cli_report(tmp_path, a1, "c1"))
    with pytest.raises(mdk.MdkError) as e:
        session.extract(base + ["--cytosine_report"])
    assert e.value.rc == -23
    r = session.perread(base)
    assert len(r) > 0 and render(r) == cli_text(tmp_path, base)
    a2 = base + ["--noCpG", "--CHH", "-r", "chrS2:1000-30000", "--minOppositeDepth", "2", "--maxVariantFrac", "0.2"]
    same(session.cytosine_report(a2), cli_report(tmp_path, a2, "c2"))
    same_calls(session.extract(base), cli_rows(tmp_path, base, "x1"))


def test_growth_and_reuse(session, tmp_path):
    """a 9 Mb sample with every context: more rows than the run arena's floor (CYTO_ROWS_FLOOR = 1 << 20 in mdk_hip_internal.hpp), nine
    1 Mb chunks in two groups, so the later group makes the arena grow with the earlier group's rows in it.  Twice on the module's session
    with equal columns, and rows equal to the command's; then ten more runs keep free HBM and the resident set within 64 MiB"""
    import torch
    synth(tmp_path / "g", "-L", "9000000", "-c", "4", "-s", "7")
    args = [tmp_path / "g.fa", tmp_path / "g.bam", "-@", "4", "--CHG", "--CHH"]
    c, again = session.cytosine_report(args), session.cytosine_report(args)
    print("rows", len(c))
    assert len(c) > 1 << 20
    for name in COLS:
        assert torch.equal(getattr(c, name), getattr(again, name)), name
    assert same(c, cli_report(tmp_path, args, "cli")) == len(c)
    n = len(c)
    del c, again
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    cur0 = int(open("/proc/self/statm").read().split()[1]) * os.sysconf("SC_PAGE_SIZE")
    for _ in range(10):
        r = session.cytosine_report(args)
        assert len(r) == n
        del r
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    cur1 = int(open("/proc/self/statm").read().split()[1]) * os.sysconf("SC_PAGE_SIZE")
    assert free0 - free1 <= 64 << 20, (free0, free1)
    assert cur1 - cur0 <= 64 << 20, (cur0, cur1, resource.getrusage(resource.RUSAGE_SELF).ru_maxrss)
