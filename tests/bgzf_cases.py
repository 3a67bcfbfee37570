"""TEST INFRASTRUCTURE: the inputs of the BGZF compressor's tests (csrc/mdk_deflate.hip, tools/deflate_emu.cpp) and the checks every
compressed file has to pass, shared by tests/test_deflate_cpu.py (through the host emulation) and tests/test_gpu_deflate.py (on the device).
Everything is seeded: nothing made here is committed."""
import gzip
import random
import struct
import subprocess
import zlib
from pathlib import Path

import deflate_zoo as Z

REPO = Path(__file__).resolve().parent.parent
EMU = REPO / "tools/_build/deflate_emu"
INFLATE_EMU = REPO / "tools/_build/inflate_emu"
MEMBER = 65280
SIZES = [0, 1, 2, 3, 4, 63, 64, 65, 257, 258, 259, 4096, 65279, 65280, 65281, 2 * 65280, 2 * 65280 + 1]
GPU_SIZES = [0, 1, 64, 65, 4096, 65280, 65281, 2 * 65280 + 1]
KINDS = ["bedgraph", "A", "random", "rotation", "period32767", "period32768", "period32769", "edge_match", "one_symbol"]


def bedgraph(n_lines, seed=20261019):
    """seeded bedGraph lines (no header) as `extract` prints them: contig, start, end, percentage, methylated, unmethylated"""
    rnd = random.Random(seed)
    out, pos, chrom = [], 10000, 1
    for i in range(n_lines):
        pos += rnd.choice((1, 1, 2, 5, 17, 40, 120, 700))
        if rnd.randrange(6000) == 0:
            chrom, pos = chrom + 1, 3000 + rnd.randrange(500)
        m, u = rnd.randrange(0, 30), rnd.randrange(0, 12)
        if m + u == 0:
            m = 1
        out.append(b"chr%d\t%d\t%d\t%d\t%d\t%d\n" % (chrom, pos, pos + 1, round(100 * m / (m + u)), m, u))
    return b"".join(out)


_TEXT = []


def _text(n):
    if not _TEXT:
        _TEXT.append(bedgraph(6000))
    t = _TEXT[0]
    assert len(t) >= n
    return t[:n]


def content(kind, n):
    rnd = random.Random(f"{kind}:{n}")
    if kind == "bedgraph":                # the workload
        return _text(n)
    if kind == "A":                       # length-258 matches at distance 1
        return b"A" * n
    if kind == "random":                  # every member stored
        return rnd.randbytes(n)
    if kind == "rotation":                # all 256 byte values: the whole literal alphabet of a dynamic block (the encoder writes no fixed blocks)
        return bytes((i * 7 + i // 256) & 255 for i in range(n))
    if kind.startswith("period"):         # a 300-byte phrase every P bytes: the distance limit.  Zeros between: they share one entry of the
        period = int(kind[6:])            # matcher's table (4096 entries), so the phrase's entries are still there a period later
        phrase = random.Random(kind).randbytes(300)
        d = bytearray(n)
        for o in range(0, n, period):
            k = min(300, n - o)
            d[o:o + k] = phrase[:k]
        return bytes(d)
    if kind == "edge_match":              # every member of 200 bytes or more ends: phrase, 8 bytes of noise, the phrase again.  The noise is
        d = bytearray(_text(n))           # literals, so the greedy walk stands on the second phrase's first byte: a match ends on the last byte
        for a in range(0, n, MEMBER):
            b = min(n, a + MEMBER)
            if b - a >= 200:
                phrase = rnd.randbytes(40)
                d[b - 88:b] = phrase + rnd.randbytes(8) + phrase
        return bytes(d)
    if kind == "one_symbol":              # a single distinct symbol, and it is symbol 0: a one-code tree
        return bytes(n)
    raise ValueError(kind)


def emu(data, eof=True):
    assert EMU.exists(), f"{EMU} is not built (make tools)"
    return subprocess.run([str(EMU)] + ([] if eof else ["--no-eof"]), input=data, capture_output=True, check=True).stdout


def zlib_members_size(data, **kw):
    """the bytes of `data` cut into 65280-byte members compressed by zlib, with 26 bytes of BGZF frame each"""
    return sum(len(Z.zraw(data[o:o + MEMBER], **kw)) + 26 for o in range(0, len(data), MEMBER))


def check_file(out, data, eof=True, cut=MEMBER):
    """everything a compressed file must be: headers, BSIZE, ISIZE, CRC32, one stream per member that zlib inflates to the member's slice
    with nothing left over, the size limits, the EOF member once and last; returns [audit(stream)] of the members"""
    audits, o, at = [], 0, 0
    n_mem = (len(data) + cut - 1) // cut
    for i in range(n_mem):
        piece = data[at:at + cut]
        assert out[o:o + 16] == b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0", (i, out[o:o + 16])
        bs = struct.unpack_from("<H", out, o + 16)[0] + 1
        assert bs <= 65536 and bs <= 18 + 5 + len(piece) + 8, (i, bs, len(piece))
        stream = out[o + 18:o + bs - 8]
        crc, isz = struct.unpack_from("<II", out, o + bs - 8)
        assert isz == len(piece) and crc == zlib.crc32(piece), i
        d = zlib.decompressobj(-15)
        assert d.decompress(stream) == piece and d.eof and d.unused_data == b"", i
        a = Z.audit(stream)
        assert a["bytes"] == piece and (a["end_bit"] + 7) // 8 == len(stream) and a["max_dist"] <= 32768, i
        audits.append(a)
        o += bs; at += len(piece)
    if eof:
        assert out[o:] == Z.BGZF_EOF and out.count(Z.BGZF_EOF) == 1
    else:
        assert o == len(out)
    if eof or data:
        assert gzip.decompress(out) == data
    return audits
