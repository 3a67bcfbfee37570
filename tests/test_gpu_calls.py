"""GPU: the resident extract session (methyldackel_amd.Session) on the MI355X -- k_calls_compact / k_calls_gather, the calls sink of the
extract pipeline, md_dev_reset between runs.  Every run's rows must equal the bedGraph lines (columns 1, 2, 3, 5, 6) of the product's own
command on the same inputs, and, where the oracle reads the same options, the oracle's.

The first test is the torch-first case: torch brings its own HIP runtime (same SONAME as the one libmdk_hip.so was linked against), puts a
tensor on the device, and only then is the session opened in the same process."""
import os
import resource

import pytest

from conftest import GOLDEN, run_oracle, synth

pytestmark = pytest.mark.gpu
CTX = ("CpG", "CHG", "CHH")


def bedgraph_rows(d, prefix="out"):
    rows = []
    for k in CTX:
        f = d / f"{prefix}_{k}.bedGraph"
        rows.append(None if not f.exists() else [(t[0], int(t[1]), int(t[2]), int(t[4]), int(t[5])) for t in (l.split("\t") for l in f.read_text().splitlines()[1:])])
    return rows


def same(calls, want):
    n = 0
    for k in range(3):
        got = calls.rows(k)
        if want[k] is None:
            assert got == [], CTX[k]
            continue
        n += len(want[k])
        assert got == want[k], (CTX[k], len(got), len(want[k]), next(((i, a, b) for i, (a, b) in enumerate(zip(got, want[k])) if a != b), None))
    assert len(calls) == n
    return n


def cli_rows(tmp, args, name, env=None):
    import methyldackel_amd as mdk
    d = tmp / name; d.mkdir()
    r = mdk.run_cli([str(a) for a in args] + ["-o", "out"], cwd=d, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    return bedgraph_rows(d)


def oracle_rows(tmp, args, name, dump=None):
    d = tmp / name; d.mkdir()
    r = run_oracle([str(a) for a in args] + ["-o", "out"], cwd=d, dump=dump)
    assert r.returncode == 0, r.stderr[-800:]
    return bedgraph_rows(d)


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
    d = tmp_path_factory.mktemp("gpu_calls")
    synth(d / "s", "-L", "90000,40000", "-c", "22", "-s", "51", "--extras", "--bbm", "--bw")
    return d


def test_torch_first_tensors_on_device(session, tmp_path):
    """first GPU use of the library in a process where torch came first: the columns are cuda tensors whose sums agree with the CPU copy,
    and the rows equal the command's"""
    import torch
    args = [GOLDEN / "cg100.fa", GOLDEN / "cg_aln.bam", "-q", "2", "--CHG", "--CHH"]
    c = session.extract(args)
    assert c.start.device == torch.device("cuda", 0) and c.contig.device == torch.device("cuda", 0)
    h = session.extract(args, device_tensors=False)
    for name in ("contig", "start", "end", "nmeth", "nunmeth", "context", "strand"):
        a, b = getattr(c, name), getattr(h, name)
        assert b.device.type == "cpu" and a.dtype == b.dtype and a.shape == b.shape
        assert int(a.long().sum().item()) == int(b.long().sum().item()), name
        assert torch.equal(a.cpu(), b), name
    assert same(c, cli_rows(tmp_path, args, "cli")) > 10


FIXTURES = [
    ("ct100.fa", "ct_aln.bam", ["-q", "2"]), ("cg100.fa", "cg_aln.bam", ["-q", "2"]), ("cg100.fa", "cg_aln.bam", ["-q", "2", "--mergeContext", "--CHG"]),
    ("cg100.fa", "cg_aln.bam", ["-q", "2", "-r", "chrCG:10-50", "--chunkSize", "7"]), ("chgchh.fa", "chgchh_aln.bam", ["-q", "5", "--CHG", "--CHH"]),
    ("chgchh.fa", "chgchh_aln.bam", ["-q", "5", "--CHG", "--CHH", "--mergeContext", "--chunkSize", "3"]), ("cg100.fa", "NH.bam", ["-q", "1"]),
    ("cg100.fa", "cg_with_variants.bam", ["-p", "1", "-q", "0", "--minOppositeDepth", "3", "--maxVariantFrac", "0.25"]),
    ("cg100.fa", "cg_with_variants.bam", ["--mergeContext", "-p", "1", "-q", "0", "--minOppositeDepth", "3", "--maxVariantFrac", "0.25"]),
]


@pytest.mark.parametrize("fa,bam,extra", FIXTURES)
def test_fixtures_equal_cli_and_oracle(session, tmp_path, fa, bam, extra):
    args = [GOLDEN / fa, GOLDEN / bam] + extra
    c = session.extract(args)
    same(c, cli_rows(tmp_path, args, "cli"))          # (ct100 and NH.bam under these options have no rows: the command writes none either)
    same(c, oracle_rows(tmp_path, args, "oracle"))


@pytest.mark.parametrize("mo,mf", [("2", "0.2"), ("1", "0.1")])
def test_merge_variant_g_next_to_covered_c(session, sdata, tmp_path, mo, mf):
    """the quirk a naive merge gets wrong: a G dropped as a variant zeroes the counts of the covered C of its CpG (mdk_emit.c:86-88), so
    the key has no row at all -- the synthetic sample holds such pairs (checked on the oracle's per-column counters), and the merged rows
    equal the command's and the oracle's"""
    from conftest import read_dump
    args = [sdata / "s.fa", sdata / "s.bam", "--mergeContext", "--CHG", "--minOppositeDepth", mo, "--maxVariantFrac", mf, "--chunkSize", "7000"]
    want = oracle_rows(tmp_path, args, "oracle", dump=tmp_path / "dump.tsv")
    d = read_dump(tmp_path / "dump.tsv")
    pairs = [(t, p) for (t, p), v in d.items() if v[0] == 0 and v[1] == 0 and v[2] + v[3] > 0 and (t, p + 1) in d and d[(t, p + 1)][1] == 1
             and d[(t, p + 1)][4] >= int(mo) and d[(t, p + 1)][5] / d[(t, p + 1)][4] >= float(mf)]
    assert pairs, "no covered C with a variant G in the sample"
    c = session.extract(args)
    same(c, want)
    same(c, cli_rows(tmp_path, args, "cli"))
    keys = {(r[0], r[1]) for r in c.rows(0)}
    assert not any((c.contigs[t], p) in keys for t, p in pairs)          # such a key has no row


SYNTH = [
    (["--CHG", "--CHH"], {}), (["--mergeContext", "-d", "3", "--CHG"], {}), (["-r", "chrS1:5000-9000", "--CHG"], {}),
    (["-l", "BED"], {}), (["-l", "BED", "--keepStrand"], {}), (["-M", "BW", "-t", "0.6", "-b", "100"], {}), (["-B", "BBM", "--mergeContext"], {}),
    (["--OT", "6,146,6,146", "--nOB", "0,9,0,0"], {}), (["--chunkSize", "100"], {}), (["--chunkSize", "2500", "--CHG"], {}), (["--chunkSize", "7000", "--CHH"], {}),
    ([], {"MDK_HOST_PREP": "1"}), (["--CHG"], {"MDK_TILE": "512"}),
    (["--mergeContext", "--CHG", "--minOppositeDepth", "2", "--maxVariantFrac", "0.2", "--chunkSize", "20000"], {}),
]


@pytest.mark.parametrize("extra,env", SYNTH)
def test_synthetic_equal_cli(session, sdata, tmp_path, extra, env):
    bed = tmp_path / "r.bed"
    bed.write_text("chrS1\t1000\t30000\t.\t0\t+\nchrS1\t50000\t70000\t.\t0\t-\nchrS2\t500\t20000\t.\t0\t.\n")
    sub = {"BED": str(bed), "BW": str(sdata / "s.bw"), "BBM": str(sdata / "s.bbm")}
    args = [sdata / "s.fa", sdata / "s.bam", "-@", "4"] + [sub.get(e, e) for e in extra]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = session.extract(args)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert same(c, cli_rows(tmp_path, args, "cli", env=env)) > 0


def test_session_reuse_equals_fresh_runs(session, sdata, tmp_path):
    """one session: a run with -l and -M, then one without them (neither may be inherited), then the first input again with other contexts"""
    bed = tmp_path / "r.bed"
    bed.write_text("chrS1\t3000\t40000\nchrS2\t100\t9000\n")
    a1 = [sdata / "s.fa", sdata / "s.bam", "-l", bed, "-M", sdata / "s.bw", "-t", "0.6", "-b", "100"]
    a2 = [GOLDEN / "chgchh.fa", GOLDEN / "chgchh_aln.bam", "-q", "5", "--CHG", "--CHH"]
    a3 = [sdata / "s.fa", sdata / "s.bam", "--noCpG", "--CHG", "--CHH", "--chunkSize", "30000"]
    a4 = [sdata / "s.fa", sdata / "s.bam"]
    for i, a in enumerate((a1, a2, a3, a4)):
        same(session.extract(a), cli_rows(tmp_path, a, f"cli{i}"))


def test_no_leak_over_ten_calls(session, sdata):
    """ten identical runs: free HBM and the process's resident memory after them stay within a stated tolerance of their values after the
    first (HBM: 64 MiB; resident set: 64 MiB)"""
    import torch
    args = [sdata / "s.fa", sdata / "s.bam", "--CHG", "--CHH", "--chunkSize", "20000"]
    ref = session.extract(args)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    rss0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    cur0 = int(open("/proc/self/statm").read().split()[1]) * os.sysconf("SC_PAGE_SIZE")
    for _ in range(10):
        c = session.extract(args)
        assert len(c) == len(ref)
        del c
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    cur1 = int(open("/proc/self/statm").read().split()[1]) * os.sysconf("SC_PAGE_SIZE")
    assert free0 - free1 <= 64 << 20, (free0, free1)
    assert cur1 - cur0 <= 64 << 20, (cur0, cur1, rss0)


def test_tables_grow_with_rows_in_them(session, tmp_path):
    """a sample past the floors of both run tables (CALLS_ROWS_FLOOR = 1 << 20 rows, CALLS_TILES_FLOOR = 1 << 14 tiles in
    mdk_hip_internal.hpp): nine 1 Mb chunks in two groups (a group holds at most eight), so the later group makes the row arena and the tile
    table grow with the earlier group's rows and tiles in them.  Twice on the module's session -- the second run starts from the grown
    tables -- with equal columns, and rows equal to the command's"""
    import torch
    synth(tmp_path / "g", "-L", "9000000", "-c", "4", "-s", "7")
    length = sum(len(l.strip()) for l in open(tmp_path / "g.fa") if not l.startswith(">"))
    args = [tmp_path / "g.fa", tmp_path / "g.bam", "-@", "4", "--CHG", "--CHH"]
    env = {"MDK_TILE": "512"}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c, again = session.extract(args), session.extract(args)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    print("rows", len(c), "tiles of 512 at least", length // 512)
    assert len(c) > 1 << 20
    assert length // 512 > 1 << 14
    for name in ("contig", "start", "end", "nmeth", "nunmeth", "context", "strand"):
        assert torch.equal(getattr(c, name), getattr(again, name)), name
    assert same(c, cli_rows(tmp_path, args, "cli", env=env)) == len(c)
