"""GPU: the resident session's perRead (methyldackel_amd.Session.perread) on the MI355X -- k_reads_len / k_reads_blocks behind
k_perread_raw on the slot's stream, k_reads_rows / k_reads_names appending each chunk to the run's rows, md_dev_reset between runs.  Rows
rendered as the command renders them (addRead, perRead.c:16-36) must equal `MethylDackel perRead`'s output and the oracle's, byte for byte.

The first test is the torch-first case: torch's runtime is up and holds a live allocation before the session opens."""
import os
import struct

import pytest

from bamwriter import record, write_bam, write_fasta
from conftest import GOLDEN, synth
from test_perread import FIX, SYN, oracle_perread

pytestmark = pytest.mark.gpu


def render(r):
    out = []
    for name, chrom, pos, m, u in r.rows():
        out.append("%s\t%s\t%d\t%f\t%u\n" % (name, chrom, pos, 100.0 * m / (m + u), m + u) if m + u else "%s\t%s\t%d\t0.0\t%u\n" % (name, chrom, pos, m + u))
    return "".join(out)


def cli_text(tmp, args, env=None):
    import methyldackel_amd as mdk
    r = mdk.run_cli([str(a) for a in args], cwd=tmp, command="perRead", env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    return r.stdout


def oracle_text(tmp, args):
    o = oracle_perread([str(a) for a in args], cwd=tmp)
    assert o.returncode == 0, o.stderr[-800:]
    return o.stdout


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
def names_data(tmp_path_factory):
    """reads whose names are 2, 63, 64, 65, 200 and 254 bytes long with their NUL -- longer than k_prep_scan's windows -- on CpG-rich contigs"""
    import random
    d = tmp_path_factory.mktemp("reads_names")
    rnd = random.Random(5)
    ref = "".join(rnd.choice("ACGTCG") for _ in range(6000))
    recs = []
    lens = (2, 63, 64, 65, 200, 254)
    for i, pos in enumerate(range(10, 5700, 23)):
        l = lens[i % len(lens)]
        name = "".join(rnd.choice("ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789:_-") for _ in range(l - 1))
        seq = "".join(("T" if c == "C" and rnd.random() < 0.5 else c) for c in ref[pos:pos + 100])
        recs.append(record(0, pos, 0 if i % 3 else 16, "100M", seq, 30, qname=name, mapq=30))
    write_fasta(d / "n.fa", [("chrN", ref)])
    write_bam(d / "n.bam", [("chrN", len(ref))], recs)
    return d


def test_torch_first_tensors_on_device(session, tmp_path):
    """the columns are cuda:0 tensors whose contents equal the device_tensors=False copy, and the rows render as the command prints them"""
    import torch
    args = [GOLDEN / "cg100.fa", GOLDEN / "cg_aln.bam", "-q", "2"]
    r = session.perread(args)
    h = session.perread(args, device_tensors=False)
    for name in ("contig", "pos", "nmeth", "nunmeth", "name_offsets", "name_bytes"):
        t = getattr(r, name)
        assert t.device == torch.device("cuda", 0), name
        assert getattr(h, name).device.type == "cpu" and torch.equal(t.cpu(), getattr(h, name)), name
    assert len(r) > 0 and int(r.name_offsets[0]) == 0 and int(r.name_offsets[-1]) == r.name_bytes.shape[0]
    assert render(r) == cli_text(tmp_path, args)


@pytest.mark.parametrize("args", FIX, ids=[" ".join(a[1:]).replace(str(GOLDEN) + "/", "") for a in FIX])
def test_fixtures_equal_cli_and_oracle(session, tmp_path, args):
    text = render(session.perread(args))
    assert text == cli_text(tmp_path, args) == oracle_text(tmp_path, args)


@pytest.mark.parametrize("which,extra", SYN, ids=[f"{w}:{' '.join(e)}" for w, e in SYN])
def test_synthetic_equal_cli_and_oracle(session, tmp_path, small_synth, which, extra):
    args = [small_synth / f"{which}.fa", small_synth / f"{which}.bam"] + extra
    text = render(session.perread(args))
    assert text.count("\n") > 100
    assert text == cli_text(tmp_path, args) == oracle_text(tmp_path, args)


@pytest.mark.parametrize("name,cmd", [("perread_cg", ["cg100.fa", "cg_aln.bam", "-q", "2"]), ("perread_chgchh", ["chgchh.fa", "chgchh_aln.bam", "-q", "5", "-p", "20"])])
def test_golden_expected(session, name, cmd):
    """the two perRead command lines of tests/golden/make_expected.py (its -o is left out: a session ignores it)"""
    want = (GOLDEN / "expected" / f"{name}.out.perRead.txt").read_text()
    assert render(session.perread([GOLDEN / cmd[0], GOLDEN / cmd[1]] + cmd[2:])) == want


def test_other_paths_give_the_same_rows(session, tmp_path, small_synth):
    """host selection (MDK_HOST_PREP=1, md_dev_perread_submit + md_dev_reads_host), -l / -r / --chunkSize 700, and -@ 4"""
    base = [small_synth / "pe.fa", small_synth / "pe.bam", "-p", "20"]
    want = render(session.perread(base))
    os.environ["MDK_HOST_PREP"] = "1"
    try:
        assert render(session.perread(base)) == want
    finally:
        del os.environ["MDK_HOST_PREP"]
    assert render(session.perread(base + ["-@", "4"])) == want
    bed = tmp_path / "b.bed"
    bed.write_text("chrS1\t5000\t5100\nchrS2\t100\t200\n")
    for extra in (["-l", bed, "--chunkSize", "2000"], ["-r", "chrS1:3000-20000"], ["--chunkSize", "700"]):
        args = base + extra
        assert render(session.perread(args)) == cli_text(tmp_path, args) == oracle_text(tmp_path, args), extra


def test_long_and_short_names_are_exact(session, names_data, tmp_path):
    args = [names_data / "n.fa", names_data / "n.bam", "-q", "0", "--chunkSize", "1000"]
    r = session.perread(args)
    want = [l.split("\t")[0] for l in cli_text(tmp_path, args).splitlines()]
    assert len(want) == len(r) > 200
    assert r.names() == want
    assert sorted({len(n) + 1 for n in want}) == [2, 63, 64, 65, 200, 254]
    off = r.name_offsets.cpu().tolist()
    assert off[0] == 0 and all(off[i + 1] - off[i] == len(want[i]) for i in range(len(want)))
    assert bytes(r.name_bytes.cpu().tolist()) == "".join(want).encode()
    assert render(r) == oracle_text(tmp_path, args)


def test_contig_missing_from_fasta(session, tmp_path, small_synth):
    fa = tmp_path / "one.fa"
    txt = (small_synth / "pe.fa").read_text()
    fa.write_text(txt[: txt.index(">", 1)])
    args = [fa, small_synth / "pe.bam"]
    text = render(session.perread(args))
    assert any(l.split("\t")[1] == "chrS2" and l.endswith("\t0.0\t0") for l in text.splitlines())
    assert text == cli_text(tmp_path, args) == oracle_text(tmp_path, args)


def test_malformed_record_gives_the_commands_rc_and_the_session_goes_on(session, names_data, tmp_path):
    import methyldackel_amd as mdk
    ref = (names_data / "n.fa").read_text().split("\n", 1)[1].replace("\n", "")
    recs = [record(0, p, 0, "50M", ref[p:p + 50], 30, qname=f"r{p}") for p in range(100, 3000, 40)]
    bad = bytearray(recs[20])
    bad[20:24] = struct.pack("<i", 5000)                      # l_seq far beyond the record's block_size
    recs[20] = bytes(bad)
    write_bam(tmp_path / "bad.bam", [("chrN", len(ref))], recs)
    args = [names_data / "n.fa", tmp_path / "bad.bam", "-q", "0"]
    cli = mdk.run_cli([str(a) for a in args], cwd=tmp_path, command="perRead", timeout=300)
    assert cli.returncode != 0
    with pytest.raises(mdk.MdkError) as e:
        session.perread(args)
    assert e.value.rc == (cli.returncode - 256 if cli.returncode > 127 else cli.returncode)
    good = [GOLDEN / "cg100.fa", GOLDEN / "cg_aln.bam", "-q", "2"]
    assert render(session.perread(good)) == oracle_text(tmp_path, good)


def test_alternating_with_extract_equals_fresh_runs(session, small_synth):
    import methyldackel_amd as mdk
    xa = [small_synth / "pe.fa", small_synth / "pe.bam", "--CHG", "--chunkSize", "6000"]
    pa = [small_synth / "pe.fa", small_synth / "pe.bam", "--chunkSize", "5000", "-p", "20"]
    got = [session.extract(xa), session.perread(pa), session.extract(xa), session.perread(pa)]
    with mdk.Session(0) as f1:
        fx = f1.extract(xa)
    with mdk.Session(0) as f2:
        fp = f2.perread(pa)
    assert got[0].rows() == got[2].rows() == fx.rows() and len(fx) > 100
    assert render(got[1]) == render(got[3]) == render(fp) and len(fp) > 100


def test_reads_outlive_the_session(small_synth):
    import methyldackel_amd as mdk
    args = [small_synth / "se.fa", small_synth / "se.bam", "-p", "24"]
    s = mdk.Session(0)
    r = s.perread(args)
    want = render(r)
    s.close()
    assert render(r) == want and len(r) > 100
    with pytest.raises(mdk.MdkError):
        s.perread(args)


def test_no_leak_over_ten_calls(session, small_synth, tmp_path):
    """ten alternating calls, one of them failing: free HBM and the resident set stay within 64 MiB of their values after the first"""
    import torch
    import methyldackel_amd as mdk
    pa = [small_synth / "pe.fa", small_synth / "pe.bam", "--chunkSize", "8000"]
    xa = [small_synth / "pe.fa", small_synth / "pe.bam", "--chunkSize", "8000"]
    ref = session.perread(pa); session.extract(xa)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    cur0 = int(open("/proc/self/statm").read().split()[1]) * os.sysconf("SC_PAGE_SIZE")
    for i in range(10):
        if i == 4:
            with pytest.raises(mdk.MdkError):
                session.perread(pa + ["-r", "nochrom:1-5"])
        elif i % 2:
            del_ = session.extract(xa); del del_
        else:
            r = session.perread(pa)
            assert len(r) == len(ref)
            del r
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    cur1 = int(open("/proc/self/statm").read().split()[1]) * os.sysconf("SC_PAGE_SIZE")
    assert free0 - free1 <= 64 << 20, (free0, free1)
    assert cur1 - cur0 <= 64 << 20, (cur0, cur1)


def test_tables_grow_with_rows_in_them(session, tmp_path):
    """a sample past the floors of both run tables (READS_ROWS_FLOOR = 1 << 18 rows, READS_BYTES_FLOOR = 1 << 22 name bytes in
    mdk_hip_internal.hpp), in three chunks none of which passes a floor alone: the tables are appended at exact size, so the rows grow at
    the second and third chunk and the name bytes at the third, each time with the earlier chunks' rows in them.  Twice on the module's
    session -- the second run starts from the grown tables -- with equal columns, and rows rendered as the command prints them"""
    import torch
    synth(tmp_path / "g", "-L", "3000000", "-c", "30", "-s", "7")
    args = [tmp_path / "g.fa", tmp_path / "g.bam"]
    r, again = session.perread(args), session.perread(args)
    print("rows", len(r), "name bytes", r.name_bytes.numel())
    assert len(r) > 1 << 18
    assert r.name_bytes.numel() > 1 << 22
    for name in ("contig", "pos", "nmeth", "nunmeth", "name_offsets", "name_bytes"):
        assert torch.equal(getattr(r, name), getattr(again, name)), name
    assert render(r) == cli_text(tmp_path, args)
