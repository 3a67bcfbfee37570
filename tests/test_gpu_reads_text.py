"""GPU: perRead's file made on the device (k_rtext_len / k_text_blocks / k_rtext_fill, csrc/mdk_text.hip) from a session's Reads --
Reads.render / Reads.write --, the ragged gather behind Reads.select (k_rtext_gather), and Bias.render.  Every comparison is byte for byte
against what this build's own `MethylDackel perRead -o file` writes (the command is pinned to the oracle elsewhere), and against
tests/golden/expected where a golden exists.  The bad-column cases are error returns of the length pass: nothing here makes the device
fault."""
import ctypes as C
import random

import pytest

from bamwriter import record, write_bam, write_fasta
from conftest import GOLDEN
from test_perread import FIX, SYN

pytestmark = pytest.mark.gpu
EXPECTED = GOLDEN / "expected"
IMAGE_BYTES = 30 * 1024           # READS_IMG_BYTES of csrc/mdk_text.hip


def cli_file(tmp, args, name="cli.perRead.txt", env=None):
    import methyldackel_amd as mdk
    r = mdk.run_cli([str(a) for a in args] + ["-o", str(tmp / name)], cwd=tmp, command="perRead", env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    return (tmp / name).read_bytes()


def text(t):
    return bytes(t.cpu().numpy())


def same(got, want, what):
    if got != want:
        a, b = got.splitlines(), want.splitlines()
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        raise AssertionError((what, len(got), len(want), len(a), len(b), first, a[first:first + 2], b[first:first + 2]))
    return want.count(b"\n")


def check(session, tmp, args):
    """one session run: the written file and the rendered tensor against the command's file; returns the Reads and the lines compared"""
    r = session.perread(args)
    want = cli_file(tmp, args)
    path = r.write(tmp / "session.perRead.txt")
    assert str(path) == str(tmp / "session.perRead.txt")
    same((tmp / "session.perRead.txt").read_bytes(), want, ("write", args))
    return r, same(text(r.render()), want, ("render", args))


@pytest.fixture(scope="module")
def session():
    import methyldackel_amd as mdk
    s = mdk.Session(0)
    yield s
    s.close()


def names_sample(d, contig):
    """reads whose names are 2, 63, 64, 65, 200 and 254 bytes long with their NUL on one CpG-rich contig (the shape of names_data in
    tests/test_gpu_reads.py), 1,240 of them: several workgroups"""
    rnd = random.Random(5)
    ref = "".join(rnd.choice("ACGTCG") for _ in range(6000))
    recs, lens = [], (2, 63, 64, 65, 200, 254)
    for i, pos in enumerate(p for p in range(10, 5700, 23) for _ in range(5)):
        name = "".join(rnd.choice("ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789:_-") for _ in range(lens[i % len(lens)] - 1))
        seq = "".join(("T" if c == "C" and rnd.random() < 0.5 else c) for c in ref[pos:pos + 100])
        recs.append(record(0, pos, 0 if i % 3 else 16, "100M", seq, 30, qname=name, mapq=30))
    write_fasta(d / "n.fa", [(contig, ref)])
    write_bam(d / "n.bam", [(contig, len(ref))], recs)
    return [d / "n.fa", d / "n.bam", "-q", "0", "--chunkSize", "1000"]


@pytest.fixture(scope="module")
def names_args(tmp_path_factory):
    return names_sample(tmp_path_factory.mktemp("reads_text_names"), "chrN")


@pytest.mark.parametrize("args", FIX, ids=[" ".join(a[1:]).replace(str(GOLDEN) + "/", "") for a in FIX])
def test_fixture_files_equal_the_command(session, tmp_path, args):
    check(session, tmp_path, args)


@pytest.mark.parametrize("which,extra", SYN, ids=[f"{w}:{' '.join(e)}" for w, e in SYN])
def test_synthetic_files_equal_the_command(session, tmp_path, small_synth, which, extra):
    _, lines = check(session, tmp_path, [small_synth / f"{which}.fa", small_synth / f"{which}.bam"] + extra)
    assert lines > 100


@pytest.mark.parametrize("name,cmd", [("perread_cg", ["cg100.fa", "cg_aln.bam", "-q", "2"]), ("perread_chgchh", ["chgchh.fa", "chgchh_aln.bam", "-q", "5", "-p", "20"])])
def test_goldens(session, tmp_path, name, cmd):
    want = (EXPECTED / f"{name}.out.perRead.txt").read_bytes()
    r = session.perread([GOLDEN / cmd[0], GOLDEN / cmd[1]] + cmd[2:])
    assert text(r.render()) == want
    assert open(r.write(tmp_path / "g.txt"), "rb").read() == want


def test_name_lengths(session, names_args, tmp_path):
    """names of 1 to 253 characters on a short contig name.  256 of them are 27 KB, more than the stage holds: the full workgroups write
    directly; the same names go through the stage and the image where the blocks are small (test_block_rows, test_fill_into_misaligned_buffers'
    sub-range) and in the synthetic samples above"""
    r, lines = check(session, tmp_path, names_args)
    assert lines == len(r) > 1000
    assert sorted({len(n) + 1 for n in r.names()}) == [2, 63, 64, 65, 200, 254]


def test_contig_name_of_255_bytes_takes_the_direct_path(session, tmp_path):
    args = names_sample(tmp_path, "L" * 255)
    r, lines = check(session, tmp_path, args)
    assert lines == len(r) > 1000
    sizes = [len(l) + 1 for l in text(r.render()).splitlines()]
    assert min(sum(sizes[i:i + 256]) for i in range(0, len(sizes) - 255, 256)) > IMAGE_BYTES        # every full workgroup is over the image


def test_block_rows(session, names_args, small_synth, tmp_path):
    """the concatenation of the blocks' text is the one-block text, whatever the block: 1, 7, and around the 256 rows of a workgroup"""
    for args in (names_args, [small_synth / "pe.fa", small_synth / "pe.bam", "-p", "20"]):
        r = session.perread(args)
        want = text(r.render(block_rows=1 << 22))
        assert want.count(b"\n") == len(r) > 1000
        for k in (1, 7, 255, 256, 257, 1000, None):
            assert text(r.render(block_rows=k)) == want, k
        assert open(r.write(tmp_path / "b.txt", block_rows=257), "rb").read() == want


def raw_renderer(r):
    """the md_text_* entry points on a Reads' columns: (library, renderer, view, name bytes)"""
    import methyldackel_amd as mdk
    L = mdk._text_lib()
    t = mdk._TextRenderer(L, 0, r.contigs)
    cols = [getattr(r, n) for n, _ in mdk.READ_COLUMNS]
    return L, t, mdk.md_reads_cols(*[C.c_void_p(c.data_ptr()) for c in cols]), int(r.name_bytes.shape[0])


@pytest.mark.parametrize("sample", ["names", "pe"])
def test_fill_into_misaligned_buffers(session, names_args, small_synth, sample):
    """md_text_fill into a buffer 0..15 bytes off a 16-byte boundary: the same bytes, and the bytes around them untouched -- for the names of
    every length (full workgroups direct) and for a sample whose workgroups all take the image"""
    import torch
    r = session.perread(names_args if sample == "names" else [small_synth / "pe.fa", small_synth / "pe.bam", "-p", "20"])
    want = text(r.render())
    L, t, view, nnb = raw_renderer(r)
    torch.cuda.synchronize()
    size = C.c_int64()
    assert L.md_text_measure_reads(t.h, C.byref(view), nnb, 0, len(r), C.byref(size)) == 0 and size.value == len(want)
    for k in range(0, 16):
        buf = torch.full((size.value + 96,), 0xEE, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        assert L.md_text_fill(t.h, C.c_void_p(buf.data_ptr() + 32 + k), size.value) == 0, L.md_dev_last_error()
        got = text(buf)
        assert got[32 + k:32 + k + size.value] == want, k
        assert set(got[:32 + k]) == {0xEE} and set(got[32 + k + size.value:]) == {0xEE}, k
    # a sub-range that starts inside the column: the workgroup's span does not begin at offset 0
    assert L.md_text_measure_reads(t.h, C.byref(view), nnb, 301, 900, C.byref(size)) == 0
    buf = torch.full((size.value + 7,), 0xEE, dtype=torch.uint8, device="cuda")
    assert L.md_text_fill(t.h, C.c_void_p(buf.data_ptr() + 7), size.value) == 0
    assert text(buf)[7:] == b"".join(want.splitlines(keepends=True)[301:900])


def test_select(session, small_synth, names_args, tmp_path):
    import torch
    args = [small_synth / "pe.fa", small_synth / "pe.bam", "-p", "20"]
    r = session.perread(args)
    lines = cli_file(tmp_path, args).splitlines(keepends=True)
    assert len(lines) == len(r) > 1000
    names = r.names()
    k = int((r.nmeth + r.nunmeth).float().mean().item()) + 1          # above the mean coverage: some reads pass, some do not
    f = r.select(r.nmeth + r.nunmeth >= k)
    keep = [i for i, l in enumerate(lines) if int(l.split(b"\t")[4]) >= k]
    assert 0 < len(keep) < len(lines) and len(f) == len(keep)
    assert open(f.write(tmp_path / "min.txt"), "rb").read() == b"".join(lines[i] for i in keep)
    assert f.names() == [names[i] for i in keep]
    assert int(f.name_offsets[0]) == 0 and int(f.name_offsets[-1]) == f.name_bytes.shape[0] and f.name_bytes.device == r.name_bytes.device
    rev = r.select(torch.arange(len(r) - 1, -1, -1, device=r.pos.device))
    assert text(rev.render()) == b"".join(lines[::-1]) and rev.names() == names[::-1]
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, len(r), (3000,), generator=g)
    idx[100:400] = 17                                           # a run of one row
    rep = r.select(idx.cuda())
    assert text(rep.render(block_rows=500)) == b"".join(lines[i] for i in idx.tolist()) and rep.names() == [names[i] for i in idx.tolist()]
    assert text(r.select(slice(5, 700, 3)).render()) == b"".join(lines[5:700:3])
    assert text(f.select(slice(10, 60)).render()) == b"".join(lines[i] for i in keep[10:60])       # a selection of a selection
    none = r.select(r.nmeth < 0)
    assert len(none) == 0 and none.names() == [] and none.render().numel() == 0
    assert open(none.write(tmp_path / "none.txt"), "rb").read() == b""
    assert len(r.select(torch.zeros(0, dtype=torch.int64, device="cuda"))) == 0
    # names of every length, in the gather's image and over it
    n = session.perread(names_args)
    nn = n.names()
    perm = torch.randperm(len(n), generator=g)
    assert n.select(perm.cuda()).names() == [nn[i] for i in perm.tolist()]
    long = [i for i, q in enumerate(nn) if len(q) >= 199]
    assert n.select(torch.tensor(long * 3, device="cuda")).names() == [nn[i] for i in long * 3]


def hand_made(names, contigs=("chrA", "b")):
    import torch
    import methyldackel_amd as mdk
    n, off = len(names), [0]
    for q in names:
        off.append(off[-1] + len(q))
    cols = {"contig": torch.tensor([i % len(contigs) for i in range(n)], dtype=torch.int32), "pos": torch.arange(n, dtype=torch.int32) * 1000 - 3,
            "nmeth": torch.arange(n, dtype=torch.int32) % 50, "nunmeth": torch.arange(n, dtype=torch.int32) % 7,
            "name_offsets": torch.tensor(off, dtype=torch.int64), "name_bytes": torch.tensor(list("".join(names).encode()), dtype=torch.uint8)}
    return mdk.Reads(list(contigs), {k: v.cuda() for k, v in cols.items()})


def python_lines(r):
    return "".join("%s\t%s\t%d\t%f\t%d\n" % (q, c, p, 100.0 * m / (m + u), m + u) if m + u else "%s\t%s\t%d\t0.0\t0\n" % (q, c, p) for q, c, p, m, u in r.rows()).encode()


def test_bad_columns_are_errors_not_faults():
    import torch
    import methyldackel_amd as mdk
    names = ["read%d/%s" % (i, "x" * (i % 40)) for i in range(1000)]
    good = hand_made(names)
    assert text(good.render()) == python_lines(good) and b"\t-3\t0.0\t0\n" in text(good.render())
    bad = hand_made(names)
    bad.contig[777] = 2
    with pytest.raises(mdk.MdkError, match="contig"):
        bad.render()
    bad.contig[777] = -1
    with pytest.raises(mdk.MdkError, match="contig"):
        bad.render(block_rows=100)
    bad = hand_made(names)
    bad.name_offsets[500] = bad.name_offsets[499] - 1
    with pytest.raises(mdk.MdkError, match="decrease"):
        bad.render()
    with pytest.raises(mdk.MdkError, match="decrease"):
        bad.select(slice(None))
    bad = hand_made(names)
    bad.name_offsets[-1] += 1
    with pytest.raises(mdk.MdkError, match="outside"):
        bad.render()
    with pytest.raises(mdk.MdkError, match="outside"):
        bad.select(torch.tensor([len(names) - 1], device="cuda"))
    bad.name_offsets[-1] = 1 << 40
    with pytest.raises(mdk.MdkError, match="outside"):
        bad.render()
    bad = hand_made(names)
    bad.name_offsets[0] = -5
    with pytest.raises(mdk.MdkError, match="outside"):
        bad.render()
    bad = hand_made(names[:10] + ["N" * 300] + names[10:])
    with pytest.raises(mdk.MdkError, match="255"):
        bad.render()
    with pytest.raises(mdk.MdkError, match="255"):
        bad.select(torch.tensor([10], device="cuda"))
    assert bad.select(torch.tensor([9, 11], device="cuda")).names() == [names[9], names[10]]
    ok = hand_made(names[:10] + ["N" * 255] + names[10:])
    assert text(ok.render()) == python_lines(ok)


def test_columns_changed_between_measure_and_fill():
    import torch
    import methyldackel_amd as mdk
    r = hand_made(["read%d" % i for i in range(2000)])
    L, t, view, nnb = raw_renderer(r)
    torch.cuda.synchronize()
    size = C.c_int64()
    assert L.md_text_measure_reads(t.h, C.byref(view), nnb, 0, len(r), C.byref(size)) == 0
    buf = torch.full((size.value + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    for change in ("a longer line", "a bad offset"):
        if change == "a longer line":
            r.nmeth[1500] = 1234567
        else:
            r.nmeth[1500] = 1500 % 50
            r.name_offsets[700] = 1 << 40
        torch.cuda.synchronize()
        assert L.md_text_fill(t.h, C.c_void_p(buf.data_ptr() + 32), size.value) != 0, change
        assert b"not the ones that were measured" in L.md_dev_last_error()
        assert set(text(buf)[:32]) == {0xEE} and set(text(buf)[32 + size.value:]) == {0xEE}
    with pytest.raises(mdk.MdkError):
        r.render()
    assert L.md_text_fill(t.h, C.c_void_p(buf.data_ptr()), size.value + 1) != 0              # not the measured size


def test_bias_render_equals_txt(session, small_synth, tmp_path):
    import methyldackel_amd as mdk
    for args in ([GOLDEN / "cg100.fa", GOLDEN / "cg_aln.bam", "-q", "2"], [small_synth / "pe.fa", small_synth / "pe.bam", "--CHG", "--CHH"]):
        c = mdk.run_cli([str(a) for a in args] + ["--txt", "--noSVG"], cwd=tmp_path, command="mbias", timeout=600)
        assert c.returncode == 0, c.stderr[-1500:]
        b = session.mbias(list(args) + ["--noSVG"])
        assert b.render() == c.stdout.encode() and c.stdout.count("\n") > 10
        assert open(b.write(tmp_path / "b.txt"), "rb").read() == c.stdout.encode()
    assert session.mbias([GOLDEN / "cg100.fa", GOLDEN / "cg_aln.bam", "-q", "2", "--noSVG"]).render() == (EXPECTED / "mbias_cg.stdout").read_bytes()


def test_alternating_runs_give_the_files_of_fresh_runs(session, small_synth, tmp_path):
    import os
    import methyldackel_amd as mdk
    pa = [small_synth / "pe.fa", small_synth / "pe.bam", "-p", "20"]
    ea = [small_synth / "pe.fa", small_synth / "pe.bam", "--CHG"]
    want_reads = cli_file(tmp_path, pa)
    d = tmp_path / "cli"; d.mkdir()
    c = mdk.run_cli([str(a) for a in ea] + ["-o", "out"], cwd=d, timeout=600)
    assert c.returncode == 0, c.stderr[-1500:]
    want_calls = {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}
    with mdk.Session(0) as s:
        a = s.perread(pa)
        assert open(a.write(tmp_path / "a.txt"), "rb").read() == want_reads
        e = s.extract(ea)
        w = tmp_path / "ses"; w.mkdir()
        e.write("out", directory=str(w))
        assert {n: (w / n).read_bytes() for n in sorted(os.listdir(w))} == want_calls
        b = s.perread(pa)
        assert open(b.write(tmp_path / "b.txt"), "rb").read() == want_reads
        assert open(a.write(tmp_path / "a2.txt"), "rb").read() == want_reads          # the first result still renders after the later runs
