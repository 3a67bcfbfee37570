"""GPU: BGZF made and read on the device.  k_deflate (csrc/mdk_deflate.hip) must give the bytes of tools/deflate_emu -- the same
csrc/mdk_deflate_core.h on the host, which tests/test_deflate_cpu.py holds against zlib -- for every content at the sizes where its paths
change; `render` / `write` with compress=True must gunzip to what they give without it, whatever block_rows is; Calls.read and Cytosines.read
must give the same columns from a .gz file as from the plain one, with pieces that end inside lines; and what they refuse must name the path.
Nothing here is over ~200 KB of text."""
import gzip
import os
import zlib

import pytest

import bgzf_cases as B
import deflate_zoo as Z

pytestmark = pytest.mark.gpu
ROWS = 4000


def dev_bytes(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if data else torch.empty(0, dtype=torch.uint8, device="cuda")


def host(t):
    return bytes(t.cpu().numpy())


# first in the file: the kernels' first execution
@pytest.mark.parametrize("kind", B.KINDS)
def test_device_bytes_are_the_emulators(kind):
    import methyldackel_amd as mdk
    for n in B.GPU_SIZES:
        data = B.content(kind, n)
        got = host(mdk.bgzf_compress(dev_bytes(data)))
        assert got == B.emu(data), (kind, n)
        if n in (0, 65, 65281):
            assert host(mdk.bgzf_compress(dev_bytes(data), eof=False)) == got[:-28], (kind, n)
    assert gzip.decompress(got) == data


def test_an_unaligned_view_and_a_cpu_tensor():
    import torch
    import methyldackel_amd as mdk
    data = B.content("bedgraph", 70003)
    t = dev_bytes(b"xyz" + data)[3:]                                   # the input starts 3 bytes behind an aligned address
    assert t.is_contiguous() and t.data_ptr() % 4 == 3
    assert host(mdk.bgzf_compress(t)) == B.emu(data)
    with pytest.raises(mdk.MdkError, match="no CPU path"):
        mdk.bgzf_compress(torch.zeros(5, dtype=torch.uint8))


@pytest.fixture(scope="module")
def results(small_synth):
    """a small session's calls, cytosines and reads, the first ROWS rows of each (~100 KB of text a file), and the same cut to 40 rows"""
    import methyldackel_amd as mdk
    fa, bam = small_synth / "pe.fa", small_synth / "pe.bam"
    with mdk.Session(0) as s:
        calls = s.extract([fa, bam, "--CHG", "--CHH"]).select(slice(0, ROWS))
        cyto = s.cytosine_report([fa, bam, "--CHG", "--CHH"]).select(slice(0, ROWS))
        reads = s.perread([fa, bam]).select(slice(0, ROWS // 2))
    assert len(calls) == len(cyto) == ROWS and len(reads) > 500
    return {"fa": fa, "calls": calls, "cyto": cyto, "reads": reads, "calls40": calls.select(slice(0, 40)), "cyto40": cyto.select(slice(0, 40)),
            "reads40": reads.select(slice(0, 40)), "calls0": calls.select(slice(0, 0)), "cyto0": cyto.select(slice(0, 0)), "reads0": reads.select(slice(0, 0))}


def check_bgzf(raw, text):
    """a BGZF file of `text`: members that zlib inflates and whose CRC32 and ISIZE check, then the EOF member, once"""
    assert raw.endswith(Z.BGZF_EOF) and raw.count(Z.BGZF_EOF) == 1
    got = b""
    for io, il, isz, crc in Z.bgzf_members(raw):
        d = zlib.decompress(raw[io:io + il], -15)
        assert len(d) == isz and zlib.crc32(d) == crc and isz <= B.MEMBER and il + 26 <= 18 + 5 + isz + 8
        got += d
    assert got == text == gzip.decompress(raw)


@pytest.mark.parametrize("size,block_rows", [("", None), ("40", 1), ("40", 7), ("0", None), ("0", 1)])
def test_render_and_write_compressed(results, tmp_path, size, block_rows):
    calls, cyto, reads = results["calls" + size], results["cyto" + size], results["reads" + size]
    plain, comp = tmp_path / "plain", tmp_path / "comp"
    plain.mkdir(); comp.mkdir()
    for fmt in ("bedGraph", "methylKit"):
        for k in range(3):
            want = host(calls.render(fmt=fmt, context=k, prefix="s"))
            check_bgzf(host(calls.render(fmt=fmt, context=k, prefix="s", block_rows=block_rows, compress=True)), want)
            assert size != "" or want.count(b"\n") > 100
        a = calls.write("s", fmt=fmt, directory=str(plain))
        b = calls.write("s", fmt=fmt, directory=str(comp), block_rows=block_rows, compress=True)
        assert [os.path.basename(p) + ".gz" for p in a] == [os.path.basename(p) for p in b] and len(b) == 3
        for p, q in zip(a, b):
            check_bgzf(open(q, "rb").read(), open(p, "rb").read())
    check_bgzf(host(calls.render(header=False, block_rows=block_rows, compress=True)), host(calls.render(header=False)))
    check_bgzf(host(cyto.render(block_rows=block_rows, compress=True)), host(cyto.render()))
    p, q = cyto.write("r", directory=str(plain)), cyto.write("r", directory=str(comp), block_rows=block_rows, compress=True)
    assert q == str(comp / "r.cytosine_report.txt.gz")
    check_bgzf(open(q, "rb").read(), open(p, "rb").read())
    check_bgzf(host(reads.render(block_rows=block_rows, compress=True)), host(reads.render()))
    p, q = reads.write(plain / "reads.txt"), reads.write(comp / "reads.anyname", block_rows=block_rows, compress=True)
    assert q == str(comp / "reads.anyname")                             # the path as given
    check_bgzf(open(q, "rb").read(), open(p, "rb").read())
    if size == "0":
        assert open(q, "rb").read() == Z.BGZF_EOF                       # no rows, no header: the EOF member alone is a valid BGZF file
        assert len(Z.bgzf_members(open(calls.write("s", directory=str(comp), compress=True)[0], "rb").read())) == 2       # the header's member and the EOF member


def same(a, b, columns):
    import torch
    return len(a) == len(b) and all(torch.equal(getattr(a, n), getattr(b, n)) for n, _ in columns)


@pytest.fixture(scope="module")
def files(results, tmp_path_factory):
    """the three bedGraphs and the report, plain and compressed, and the columns read from the plain ones"""
    import methyldackel_amd as mdk
    d = tmp_path_factory.mktemp("gz")
    calls, cyto = results["calls"], results["cyto"]
    plain, gz = calls.write("s", directory=str(d)), calls.write("s", directory=str(d), compress=True)
    rp, rgz = cyto.write("s", directory=str(d)), cyto.write("s", directory=str(d), compress=True)
    ref = mdk.Reference(results["fa"])
    want = mdk.Calls.read(plain, ref)
    assert len(want) > ROWS // 2
    yield {"dir": d, "plain": plain, "gz": gz, "report": rp, "report_gz": rgz, "ref": ref, "calls": want, "cyto": mdk.Cytosines.read(rp, cyto.contigs), "contigs": cyto.contigs}
    ref.close()


def zlib_bgzf(text, cut, eof):
    """BGZF by Python's zlib, a member every `cut` bytes: lines straddle every member"""
    return b"".join(Z.bgzf_member(Z.zraw(text[o:o + cut], 1 + o // cut % 9), len(text[o:o + cut]), zlib.crc32(text[o:o + cut])) for o in range(0, len(text), cut)) + (Z.BGZF_EOF if eof else b"")


def test_read_of_gz_files_equals_read_of_plain_files(files, monkeypatch):
    import methyldackel_amd as mdk
    assert same(mdk.Calls.read(files["gz"], files["ref"]), files["calls"], mdk.CALL_COLUMNS)
    assert same(mdk.Cytosines.read(files["report_gz"], files["contigs"]), files["cyto"], mdk.CYTOSINE_COLUMNS)
    # pieces of one member each: every piece but the last ends inside a line, which is carried on the device to the front of the next
    assert os.path.getsize(files["report"]) > B.MEMBER
    monkeypatch.setenv("MDK_PARSE_BLOCK_BYTES", "5000")
    assert same(mdk.Calls.read(files["gz"], files["ref"]), files["calls"], mdk.CALL_COLUMNS)
    assert same(mdk.Cytosines.read(files["report_gz"], files["contigs"]), files["cyto"], mdk.CYTOSINE_COLUMNS)
    monkeypatch.delenv("MDK_PARSE_BLOCK_BYTES")
    # Python's zlib in 1000-byte members, no EOF member: lines straddle every member, and pieces of 1, 2, 3 and all members
    text = open(files["report"], "rb").read()
    assert text[999:1000] != b"\n" and len(text) > 100000
    path = files["dir"] / "zlib_members.txt"                            # recognised by content, not by name
    path.write_bytes(zlib_bgzf(text, 1000, eof=False))
    for block in (None, 1000, 2500, 3000):
        assert same(mdk.Cytosines.read(path, files["contigs"], block_bytes=block), files["cyto"], mdk.CYTOSINE_COLUMNS), block
    bed = open(files["plain"][0], "rb").read()
    path.write_bytes(zlib_bgzf(bed, 1000, eof=True))
    assert same(mdk.Calls.read(path, files["ref"], block_bytes=1500), mdk.Calls.read(files["plain"][0], files["ref"]), mdk.CALL_COLUMNS)
    hdr = files["dir"] / "hdr.gz"                                        # header only, compressed: no rows
    hdr.write_bytes(zlib_bgzf(bed[:bed.index(b"\n") + 1], 1000, eof=True))
    assert len(mdk.Calls.read(hdr, files["ref"])) == 0
    hdr.write_bytes(Z.BGZF_EOF)
    assert len(mdk.Cytosines.read(hdr, files["contigs"])) == 0


def test_refusals_name_the_path(files):
    import methyldackel_amd as mdk
    text = open(files["report"], "rb").read()
    d = files["dir"]
    (d / "plain_gzip.txt.gz").write_bytes(gzip.compress(text))
    with pytest.raises(mdk.MdkError, match=r"plain_gzip\.txt\.gz.*not BGZF.*bgzip"):
        mdk.Cytosines.read(d / "plain_gzip.txt.gz", files["contigs"])
    # a stored member in the middle with one payload byte flipped: the stream still inflates, its CRC32 does not check
    part = text[:text.rindex(b"\n", 0, 9000) + 1]
    cut = [part[:3000], part[3000:5000], part[5000:]]
    mem = [Z.bgzf_member(Z.zraw(c, 0 if i == 1 else 6), len(c), zlib.crc32(c)) for i, c in enumerate(cut)]
    good = b"".join(mem) + Z.BGZF_EOF
    (d / "good.gz").write_bytes(good)
    assert len(mdk.Cytosines.read(d / "good.gz", files["contigs"])) == part.count(b"\n")
    at = len(mem[0]) + 18 + 5 + 700
    (d / "flipped.gz").write_bytes(good[:at] + bytes([good[at] ^ 1]) + good[at + 1:])
    with pytest.raises(mdk.MdkError, match=rf"flipped\.gz.*member at byte {len(mem[0])} .*CRC32"):
        mdk.Cytosines.read(d / "flipped.gz", files["contigs"])
    isz = good[:len(mem[0]) - 4] + (2999).to_bytes(4, "little") + good[len(mem[0]):]
    (d / "isize.gz").write_bytes(isz)
    with pytest.raises(mdk.MdkError, match=r"isize\.gz.*member at byte 0 "):
        mdk.Cytosines.read(d / "isize.gz", files["contigs"])
    raw = open(files["report_gz"], "rb").read()
    (d / "cut.gz").write_bytes(raw[:len(raw) - 28 - 100])
    with pytest.raises(mdk.MdkError, match=r"cut\.gz.*cut short"):
        mdk.Cytosines.read(d / "cut.gz", files["contigs"])
    with pytest.raises(mdk.MdkError, match=r"cut\.gz.*cut short"):
        mdk.Calls.read([files["gz"][0], d / "cut.gz"], files["ref"])


@pytest.mark.parametrize("block", [None, 5000])
def test_a_malformed_line_in_a_compressed_file_has_its_number(files, block):
    import methyldackel_amd as mdk
    lines = open(files["report"], "rb").read().split(b"\n")[:-1]
    assert len(lines) == ROWS
    k = 3100                                                            # ~90 KB in: the second member
    lines[k] = lines[k].replace(b"\t", b" ", 1)
    text = b"\n".join(lines) + b"\n"
    assert len(b"\n".join(lines[:k])) > B.MEMBER
    path = files["dir"] / "badline.gz"
    path.write_bytes(host(mdk.bgzf_compress(dev_bytes(text))))
    with pytest.raises(mdk.MdkError, match=rf"badline\.gz, line {k + 1}: ") as e:
        mdk.Cytosines.read(path, files["contigs"], block_bytes=block)
    assert e.value.rc == -3
