"""GPU: the text of `extract`'s files made on the device (k_text_len / k_text_blocks / k_text_fill, csrc/mdk_text.hip) from a session's
columns -- Calls.render / Calls.write, Cytosines.render / Cytosines.write.  Every file set must be byte-identical, names included, to what
this build's own `MethylDackel extract -o out ...` writes with the matching option (the command is pinned to the oracle elsewhere), and to
tests/golden/expected where a golden exists."""
import os

import pytest

from conftest import GOLDEN, synth

pytestmark = pytest.mark.gpu
EXPECTED = GOLDEN / "expected"
FORMATS = (("bedGraph", []), ("fraction", ["--fraction"]), ("counts", ["--counts"]), ("methylKit", ["--methylKit"]))


def files(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}


def cli_files(tmp, args, name, env=None):
    import methyldackel_amd as mdk
    d = tmp / name; d.mkdir()
    r = mdk.run_cli([str(a) for a in args] + ["-o", "out"], cwd=d, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    return files(d)


def same_files(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for n in want:
        if got[n] != want[n]:
            a, b = got[n].splitlines(), want[n].splitlines()
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            raise AssertionError((what, n, len(a), len(b), first, a[first:first + 2], b[first:first + 2]))
    return sum(v.count(b"\n") for v in want.values())


def written(result, tmp, name, *a, **kw):
    d = tmp / name; d.mkdir()
    paths = result.write("out", *a, directory=str(d), **kw)
    assert sorted(os.path.basename(p) for p in ([paths] if isinstance(paths, str) else paths)) == sorted(os.listdir(d))
    return files(d)


def check_formats(session, tmp, args, formats=FORMATS, env=None):
    """one session run, every format written from it, each against the command with that format's option; returns the lines compared"""
    c = session.extract(args)
    lines = 0
    for fmt, opt in formats:
        lines += same_files(written(c, tmp, "s_" + fmt, fmt), cli_files(tmp, list(args) + opt, "c_" + fmt, env=env), (fmt, args))
    return c, lines


def check_report(session, tmp, args):
    y = session.cytosine_report(args)
    return y, same_files(written(y, tmp, "s_report"), cli_files(tmp, list(args) + ["--cytosine_report"], "c_report"), ("cytosine_report", args))


@pytest.fixture(scope="module")
def session():
    import methyldackel_amd as mdk
    s = mdk.Session(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def sdata(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_text")
    synth(d / "s", "-L", "90000,40000", "-c", "22", "-s", "51", "--extras", "--bbm", "--bw")
    return d


# the fixture list of tests/test_gpu_calls.py
FIXTURES = [
    ("ct100.fa", "ct_aln.bam", ["-q", "2"]), ("cg100.fa", "cg_aln.bam", ["-q", "2"]), ("cg100.fa", "cg_aln.bam", ["-q", "2", "--mergeContext", "--CHG"]),
    ("cg100.fa", "cg_aln.bam", ["-q", "2", "-r", "chrCG:10-50", "--chunkSize", "7"]), ("chgchh.fa", "chgchh_aln.bam", ["-q", "5", "--CHG", "--CHH"]),
    ("chgchh.fa", "chgchh_aln.bam", ["-q", "5", "--CHG", "--CHH", "--mergeContext", "--chunkSize", "3"]), ("cg100.fa", "NH.bam", ["-q", "1"]),
    ("cg100.fa", "cg_with_variants.bam", ["-p", "1", "-q", "0", "--minOppositeDepth", "3", "--maxVariantFrac", "0.25"]),
    ("cg100.fa", "cg_with_variants.bam", ["--mergeContext", "-p", "1", "-q", "0", "--minOppositeDepth", "3", "--maxVariantFrac", "0.25"]),
]


@pytest.mark.parametrize("fa,bam,extra", FIXTURES)
def test_fixture_file_sets_equal_the_command(session, tmp_path, fa, bam, extra):
    """the four call formats (three under --mergeContext: the command refuses --methylKit with it) and, without --mergeContext, the report"""
    args = [GOLDEN / fa, GOLDEN / bam] + extra
    merged = "--mergeContext" in extra
    c, _ = check_formats(session, tmp_path, args, FORMATS[:3] if merged else FORMATS)
    assert c.merged == merged
    if not merged:
        check_report(session, tmp_path, args)


def test_goldens(session, tmp_path):
    """where tests/golden/expected holds the command's file: the rendered bytes are that file"""
    base = [GOLDEN / "cg100.fa", GOLDEN / "cg_aln.bam", "-q", "2"]
    c = session.extract(base)
    assert bytes(c.render(prefix="out").cpu().numpy()) == (EXPECTED / "extract_cg_q2.out_CpG.bedGraph").read_bytes()
    assert bytes(c.render("fraction", prefix="out").cpu().numpy()) == (EXPECTED / "extract_cg_fraction.out_CpG.meth.bedGraph").read_bytes()
    a = session.extract(base + ["--CHG", "--CHH"])
    for k, ctx in enumerate(("CpG", "CHG", "CHH")):
        assert bytes(a.render(context=k, prefix="out").cpu().numpy()) == (EXPECTED / f"extract_cg_all_contexts.out_{ctx}.bedGraph").read_bytes(), ctx
        assert bytes(a.render("methylKit", context=k).cpu().numpy()) == (EXPECTED / f"extract_cg_methylkit.out_{ctx}.methylKit").read_bytes(), ctx
    y = session.cytosine_report(base + ["--CHG", "--CHH"])
    assert bytes(y.render().cpu().numpy()) == (EXPECTED / "extract_cg_cytosine_report.out.cytosine_report.txt").read_bytes()


def test_synthetic_all_contexts(session, sdata, tmp_path):
    args = [sdata / "s.fa", sdata / "s.bam", "-@", "4", "--CHG", "--CHH"]
    c, lines = check_formats(session, tmp_path, args)
    assert lines > 4 * 20000 and c.contexts_on == (0, 1, 2)
    _, n = check_report(session, tmp_path, args)
    assert n > 40000


def test_synthetic_merged(session, sdata, tmp_path):
    args = [sdata / "s.fa", sdata / "s.bam", "-@", "4", "--mergeContext", "--CHG"]
    c, lines = check_formats(session, tmp_path, args, FORMATS[:3])
    assert lines > 3000 and c.merged and c.contexts_on == (0, 1)
    assert b" CpG merged methylation levels" in written(c, tmp_path, "again")["out_CpG.bedGraph"].splitlines()[0]


def test_region_chunks_and_bed(session, sdata, tmp_path):
    """-r with small chunks for the call formats; -l for the report (a chunk a BED interval touches lists all its cytosines)"""
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    _, lines = check_formats(session, tmp_path / "a", [sdata / "s.fa", sdata / "s.bam", "-r", "chrS1:5000-9000", "--CHG", "--chunkSize", "700"])
    assert lines > 400
    bed = tmp_path / "r.bed"
    bed.write_text("chrS1\t1000\t30000\t.\t0\t+\nchrS1\t50000\t70000\t.\t0\t-\nchrS2\t500\t20000\t.\t0\t.\n")
    _, n = check_report(session, tmp_path / "b", [sdata / "s.fa", sdata / "s.bam", "-l", bed, "--CHG"])
    assert n > 1000


def test_filtered_copy_equals_min_depth(session, sdata, tmp_path):
    """what the command cannot do: rows filtered with torch are still a valid bedGraph -- here the filter is -d 10, so the command can say"""
    args = [sdata / "s.fa", sdata / "s.bam", "-@", "4", "--CHG", "--CHH"]
    c = session.extract(args)
    f = c.select((c.nmeth + c.nunmeth) >= 10)
    assert 0 < len(f) < len(c)
    for fmt, opt in FORMATS:
        want = cli_files(tmp_path, args + ["-d", "10"] + opt, "c_" + fmt)
        for k, ctx in enumerate(("CpG", "CHG", "CHH")):
            name = next(n for n in want if n.startswith(f"out_{ctx}."))
            assert bytes(f.render(fmt, context=k, prefix="out").cpu().numpy()) == want[name], (fmt, ctx)
    # the rows in another order are rendered in that order
    import torch
    rev = f.select(torch.arange(len(f) - 1, -1, -1, device=f.start.device))
    body = bytes(f.render("counts", context=0, header=False).cpu().numpy()).splitlines()
    assert bytes(rev.render("counts", context=0, header=False).cpu().numpy()).splitlines() == body[::-1] and len(body) > 100


def test_empty_results_render_the_header(session, sdata, tmp_path):
    c = session.extract([GOLDEN / "ct100.fa", GOLDEN / "ct_aln.bam", "-q", "2"])          # no rows under these options
    assert len(c) == 0
    assert bytes(c.render(prefix="out").cpu().numpy()) == b'track type="bedGraph" description="out CpG methylation levels"\n'
    assert c.render(header=False).numel() == 0
    assert written(c, tmp_path, "w", "methylKit") == {"out_CpG.methylKit": b"chrBase\tchr\tbase\tstrand\tcoverage\tfreqC\tfreqT\n"}
    full = session.extract([sdata / "s.fa", sdata / "s.bam"])
    none = full.select(full.nmeth < 0)
    assert len(full) > 0 and len(none) == 0
    assert bytes(none.render("fraction", prefix="x y").cpu().numpy()) == b'track type="bedGraph" description="x y CpG methylation fractions"\n'


def test_refusals(session, sdata):
    import methyldackel_amd as mdk
    args = [sdata / "s.fa", sdata / "s.bam", "--mergeContext"]
    c = session.extract(args)
    with pytest.raises(mdk.MdkError) as e:
        c.render("logit", prefix="out")
    assert e.value.rc == -23
    with pytest.raises(mdk.MdkError, match="strand"):
        c.render("methylKit")
    h = session.extract(args, device_tensors=False)
    with pytest.raises(mdk.MdkError, match="no CPU path"):
        h.render(prefix="out")
    with pytest.raises(mdk.MdkError, match="no CPU path"):
        h.write("out")
    with pytest.raises(mdk.MdkError, match="no CPU path"):
        session.cytosine_report(args[:2], device_tensors=False).write("out")
    with pytest.raises(mdk.MdkError) as e:              # the text-shaping options stay refused on the command line
        session.extract(args + ["--fraction"])
    assert e.value.rc == -23


def test_block_boundaries(session, sdata, tmp_path, monkeypatch):
    """blocks of 1000 and of 257 rows (not a multiple of the 256 rows of a workgroup), by keyword and by the environment hook: the files do
    not change"""
    args = [sdata / "s.fa", sdata / "s.bam", "-@", "4", "--CHG", "--CHH"]
    c, y = session.extract(args), session.cytosine_report(args)
    for fmt, _ in FORMATS:
        want = written(c, tmp_path, "w_" + fmt, fmt)
        assert written(c, tmp_path, "b1000_" + fmt, fmt, block_rows=1000) == want
        assert written(c, tmp_path, "b257_" + fmt, fmt, block_rows=257) == want
    want = written(y, tmp_path, "w_report")
    assert written(y, tmp_path, "b1000_report", block_rows=1000) == want
    monkeypatch.setenv("MDK_TEXT_BLOCK_ROWS", "4099")
    assert written(y, tmp_path, "benv_report") == want
    assert written(c, tmp_path, "benv_calls") == written(c, tmp_path, "w_again", block_rows=1 << 22)
    assert bytes(c.render("methylKit", context=2, block_rows=777).cpu().numpy()) == written(c, tmp_path, "mk", "methylKit")["out_CHH.methylKit"]


def python_lines(fmt, contigs, rows):
    """the command's lines from Python's own % formatting, which prints a double's exact value rounded half-even as glibc does"""
    out = []
    for t, a, b, m, u, s in rows:
        cov = m + u
        if cov == 0:
            continue
        ch = contigs[t]
        if fmt == "bedGraph":
            out.append("%s\t%d\t%d\t%d\t%d\t%d\n" % (ch, a, b, int(100.0 * float(m) / cov), m, u))
        elif fmt == "fraction":
            out.append("%s\t%d\t%d\t%f\n" % (ch, a, b, float(m) / cov))
        elif fmt == "counts":
            out.append("%s\t%d\t%d\t%d\n" % (ch, a, b, cov))
        else:
            out.append("%s.%d\t%s\t%d\t%s\t%d\t%6.2f\t%6.2f\n" % (ch, a + 1, ch, a + 1, "F" if s > 0 else "R", cov, 100.0 * float(m) / cov, 100.0 * float(u) / cov))
    return "".join(out).encode()


def hand_made(contigs, n, seed, big):
    """Calls of n seeded random rows on the device: counts up to 2^30 (big) or small ones with many exact halves, positions up to 2^31 - 4"""
    import torch
    import methyldackel_amd as mdk
    g = torch.Generator().manual_seed(seed)
    hi = 1 << 30 if big else 41
    cols = {"contig": torch.randint(0, len(contigs), (n,), generator=g, dtype=torch.int32), "start": torch.randint(0, (1 << 31) - 4, (n,), generator=g, dtype=torch.int64).to(torch.int32),
            "nmeth": (torch.randint(0, hi, (n,), generator=g, dtype=torch.int64) >> torch.randint(0, 30 if big else 1, (n,), generator=g)).to(torch.int32),
            "nunmeth": (torch.randint(0, hi, (n,), generator=g, dtype=torch.int64) >> torch.randint(0, 30 if big else 1, (n,), generator=g)).to(torch.int32),
            "context": torch.zeros(n, dtype=torch.uint8), "strand": (torch.randint(0, 2, (n,), generator=g, dtype=torch.int8) * 2 - 1)}
    cols["end"] = cols["start"] + 1
    rows = list(zip(*[cols[k].tolist() for k in ("contig", "start", "end", "nmeth", "nunmeth", "strand")]))
    return mdk.Calls(contigs, {k: v.cuda() for k, v in cols.items()}), rows


@pytest.mark.parametrize("big", [False, True])
def test_device_arithmetic_on_random_rows(big):
    """the device's own double division and integer rounding over 200,000 rows no BAM file gives: every format against Python's formatting"""
    contigs = ["chr1", "chrUn_KI270742v1", "X"]
    c, rows = hand_made(contigs, 200000, 5 + big, big)
    for fmt, _ in FORMATS:
        assert bytes(c.render(fmt, header=False).cpu().numpy()) == python_lines(fmt, contigs, rows), fmt


def test_long_names_and_bad_rows():
    """names of 255 bytes: a workgroup's text is longer than its LDS image and goes straight to global memory; 256 bytes are refused, and so
    is a contig index outside the name table"""
    import torch
    import methyldackel_amd as mdk
    contigs = ["L" * 255, "s", "M" * 130]
    c, rows = hand_made(contigs, 3000, 9, False)
    for fmt, _ in FORMATS:
        assert bytes(c.render(fmt, header=False, block_rows=1001).cpu().numpy()) == python_lines(fmt, contigs, rows), fmt
    with pytest.raises(mdk.MdkError, match="255"):
        hand_made(["N" * 256], 10, 1, False)[0].render(header=False)
    bad, _ = hand_made(["a", "b"], 1000, 2, False)
    bad.contig[777] = 2
    with pytest.raises(mdk.MdkError, match="contig"):
        bad.render(header=False)
    bad.contig[777] = -1
    with pytest.raises(mdk.MdkError, match="contig"):
        bad.render("counts", header=False, block_rows=100)
