"""The host side of compressed tables, without a GPU: how a file is recognised as BGZF (by content), the member table the host walks out of
the 18-byte headers, what that walk refuses, Intervals.read of .gz files, and what `compress=True`, `bgzf_compress` and a read of a .gz file
refuse before any device is touched.  The compressor itself: tests/test_deflate_cpu.py; all of it on the device: tests/test_gpu_deflate.py."""
import gzip
import struct
import zlib

import pytest
import torch

import methyldackel_amd as mdk
import bgzf_cases as B
import deflate_zoo as Z


def member(data, extra_before=b"", extra_after=b"", level=6):
    """one BGZF member by hand, optionally with other subfields around BC"""
    s = Z.zraw(data, level)
    xlen = len(extra_before) + 6 + len(extra_after)
    bsize = 12 + xlen + len(s) + 8
    return (struct.pack("<BBBBIBBH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, xlen) + extra_before + b"BC" + struct.pack("<HH", 2, bsize - 1) + extra_after
            + s + struct.pack("<II", zlib.crc32(data), len(data)))


def test_a_file_is_recognised_by_its_content(tmp_path):
    text = B.bedgraph(50)
    cases = {"plain.gz": (text, "plain"), "empty": (b"", "plain"), "gz.bedGraph": (gzip.compress(text), "gzip"),
             "bgzf.txt": (member(text) + Z.BGZF_EOF, "bgzf"), "emu": (B.emu(text), "bgzf"),
             "subfields": (member(text, extra_before=b"XY\x03\x00abc", extra_after=b"ZZ\x00\x00") + Z.BGZF_EOF, "bgzf"),
             "fname": (b"\x1f\x8b\x08\x0c" + member(text)[4:], "gzip"),                          # FLG has more than FEXTRA
             "other_subfield": (struct.pack("<BBBBIBBH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6) + b"BD\x02\x00\x00\x00" + Z.zraw(text) + struct.pack("<II", zlib.crc32(text), len(text)), "gzip")}
    for name, (data, kind) in cases.items():
        (tmp_path / name).write_bytes(data)
        assert mdk._gz_kind(str(tmp_path / name)) == kind, name


def test_member_table_of_hand_made_files():
    parts = [b"first\n", b"x" * 70000, b"", b"tail without newline"]
    members, want, o = b"", [], 0
    for i, p in enumerate(parts):
        for c in range(0, max(len(p), 1), 65280):
            d = p[c:c + 65280]
            m = member(d, extra_before=b"QQ\x01\x00!" if i == 1 else b"")
            x = 5 if i == 1 else 0
            if d:
                want.append((o, o + 18 + x, len(m) - 26 - x, len(d), zlib.crc32(d)))
            members += m; o += len(m)
    for tail in (Z.BGZF_EOF, b""):                                   # a missing EOF member is accepted
        got = mdk._bgzf_members("f", members + tail)
        assert got == want
        assert b"".join(zlib.decompress((members + tail)[so:so + sl], -15) for _, so, sl, _, _ in got) == b"".join(parts)
    assert mdk._bgzf_members("f", Z.BGZF_EOF) == [] and mdk._bgzf_members("f", b"") == []
    assert mdk._bgzf_members("f", B.emu(b"")) == []
    data = B.bedgraph(5000)
    out = B.emu(data)
    assert [(fo, so - fo, isz) for fo, so, _, isz, _ in mdk._bgzf_members("f", out)] == [(io - 18, 18, isz) for io, _, isz, _ in Z.bgzf_members(out)[:-1]]


def test_what_the_member_walk_refuses():
    good = member(b"one\n") + member(b"two\n")
    for bad, word in ((good[:-1], "cut short"), (good[:-9], "cut short"), (good[:len(member(b"one\n")) + 7], "cut short"), (good + b"\x1f\x8b", "cut short"),
                      (good + gzip.compress(b"three\n"), "no BGZF member"), (good + b"garbage that is no header at all", "no BGZF member"),
                      (member(b"one\n")[:-4] + struct.pack("<I", 70000), "at most 65536")):
        with pytest.raises(mdk.MdkError, match=word) as e:
            mdk._bgzf_members("some/path.gz", bad)
        assert "some/path.gz" in str(e.value)


def test_intervals_read_takes_gz_of_either_kind(tmp_path):
    bed = b"# islands\ntrack name=x\nchr2\t5\t9\tname\nchr1 100 200\n\nchr2\t0\t0\n"
    contigs = ["chr1", "chr2"]
    (tmp_path / "a.bed").write_bytes(bed)
    (tmp_path / "a.bed.gz").write_bytes(gzip.compress(bed))
    (tmp_path / "b.bed.gz").write_bytes(B.emu(bed))
    (tmp_path / "named.bed").write_bytes(member(bed[:20]) + member(bed[20:]))            # BGZF without the EOF member, under a plain name
    want = mdk.Intervals.read(tmp_path / "a.bed", contigs)
    assert len(want) == 3
    for f in ("a.bed.gz", "b.bed.gz", "named.bed"):
        got = mdk.Intervals.read(tmp_path / f, contigs)
        assert all(torch.equal(getattr(got, c), getattr(want, c)) for c in ("contig", "start", "end")), f
    (tmp_path / "bad.bed.gz").write_bytes(gzip.compress(bed)[:-12])
    with pytest.raises(mdk.MdkError, match="bad.bed.gz"):
        mdk.Intervals.read(tmp_path / "bad.bed.gz", contigs)
    (tmp_path / "line.bed.gz").write_bytes(gzip.compress(b"chr1\t1\t2\nchr9\t1\t2\n"))
    with pytest.raises(mdk.MdkError, match="line.bed.gz:2"):
        mdk.Intervals.read(tmp_path / "line.bed.gz", contigs)


def test_refusals_that_need_no_device(tmp_path):
    """CPU tensors are refused by `bgzf_compress` and by `compress=True` as they are without it; a .gz file is refused when no device is
    visible, and a gzip file that is not BGZF is refused where one is"""
    with pytest.raises(mdk.MdkError, match="no CPU path"):
        mdk.bgzf_compress(torch.zeros(10, dtype=torch.uint8))
    for bad in (torch.zeros(10, dtype=torch.int8), torch.zeros((2, 5), dtype=torch.uint8), torch.zeros(10, dtype=torch.uint8)[::2], b"bytes"):
        with pytest.raises(mdk.MdkError, match="contiguous one-dimensional uint8"):
            mdk.bgzf_compress(bad)
    c = mdk.Calls(["chrA"], {n: torch.zeros(2, dtype=getattr(torch, dt)) for n, dt in mdk.CALL_COLUMNS})
    y = mdk.Cytosines(["chrA"], {n: torch.zeros((2, 3) if n == "trinucleotide" else 2, dtype=getattr(torch, dt)) for n, dt in mdk.CYTOSINE_COLUMNS})
    r = mdk.Reads(["chrA"], {n: torch.zeros(3 if n == "name_offsets" else 2, dtype=getattr(torch, dt)) for n, dt in mdk.READ_COLUMNS})
    for call in (lambda: c.render(prefix="p", compress=True), lambda: c.write("p", directory=str(tmp_path), compress=True), lambda: y.render(compress=True),
                 lambda: y.write("p", directory=str(tmp_path), compress=True), lambda: r.render(compress=True), lambda: r.write(tmp_path / "r.gz", compress=True)):
        with pytest.raises(mdk.MdkError, match="no CPU path"):
            call()
    assert not list(tmp_path.iterdir())                                  # refused before a file is opened
    with pytest.raises(mdk.MdkError, match="-23|log"):
        c.write("p", fmt="logit", compress=True)
    (tmp_path / "plain.cytosine_report.txt.gz").write_bytes(gzip.compress(b"chrA\t1\t+\t1\t0\tCG\tCGA\n"))
    with pytest.raises(mdk.MdkError, match="no device is visible|not BGZF"):
        mdk.Cytosines.read(tmp_path / "plain.cytosine_report.txt.gz", ["chrA"])
    assert mdk.BGZF_EOF == Z.BGZF_EOF and mdk.BGZF_MEMBER == B.MEMBER
    assert {"md_text_deflate_measure", "md_text_deflate_fill", "md_piece_copy"} <= set(mdk.HIP_SYMBOLS)
