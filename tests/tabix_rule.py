"""The tabix rule of csrc/mdk_tabix_core.h, twice and independently: a BUILDER (the rule restated with numpy: text + member table ->
payload bytes, or the refusal and its line) and a READER written from the SAM/tabix specification alone (struct, zlib, gzip: parse a .tbi,
reg2bins, drop the chunks at or before the linear index, seek to the virtual offsets, return the overlapping lines), whose yardstick is
brute force over gzip.decompress(file).  Also the tables the CPU and GPU tests share, the BGZF cuts, the region grid and the refusals."""
import functools
import gzip
import re
import struct
import subprocess
import zlib
from pathlib import Path

import numpy as np

import deflate_zoo as Z

REPO = Path(__file__).resolve().parent.parent
EMU = REPO / "tools/_build/tabix_emu"
UCSC = 0x10000
PRESETS = {"bed": (UCSC, 1, 2, 3, ord("#")), "methylKit": (0, 2, 3, 3, ord("#")), "cytosine_report": (0, 1, 2, 2, ord("#"))}
E_FEW, E_COORD, E_RANGE, E_BIG, E_NAME, E_LONG, E_EMPTY, E_ORDER, E_RETURN = range(1, 10)
MESSAGES = {E_FEW: "fewer fields", E_COORD: "coordinate", E_RANGE: "begins before", E_BIG: "512 Mb, and CSI is not written", E_NAME: "sequence name",
            E_LONG: "longer than 512 bytes", E_EMPTY: "an empty line", E_ORDER: "not sorted", E_RETURN: "appears in two places"}


def conf(preset, skip):
    return PRESETS[preset] + (int(skip),)


class Refused(Exception):
    def __init__(self, line, code):
        super().__init__(f"line {line}: code {code}")
        self.line, self.code = line, code


# ---- BGZF by zlib, cut where the caller says ----
def bgzf(text, cuts, eof=True):
    """`text` as BGZF: members of the sizes in `cuts` (an int: every member that size; a list: those sizes, the last repeated; 0 is an empty member)"""
    out, o, k = [], 0, 0
    if isinstance(cuts, int):
        cuts = [cuts]
    while o < len(text) or k < len(cuts):
        n = cuts[min(k, len(cuts) - 1)]
        piece = text[o:o + n]
        out.append(Z.bgzf_member(Z.zraw(piece, 1 + k % 9), len(piece), zlib.crc32(piece)))
        o += n; k += 1
        if k >= len(cuts) and o >= len(text):
            break
    return b"".join(out) + (Z.BGZF_EOF if eof else b"")


def members(raw):
    """every member of a BGZF file, empty ones too: [(file offset, decompressed start, isize)], and the decompressed length"""
    out, o, u = [], 0, 0
    while o + 18 <= len(raw):
        bs = struct.unpack_from("<H", raw, o + 16)[0] + 1
        isz = struct.unpack_from("<I", raw, o + bs - 4)[0]
        out.append((o, u, isz))
        o += bs; u += isz
    assert o == len(raw)
    return out, u


# ---- the builder: the rule restated ----
def reg2bin(beg, end):
    """vectorised: the bin of [beg, end)"""
    beg, end = np.asarray(beg, dtype=np.int64), np.asarray(end, dtype=np.int64) - 1
    out = np.zeros(beg.shape, dtype=np.int64)
    done = np.zeros(beg.shape, dtype=bool)
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        hit = ~done & (beg >> shift == end >> shift)
        out[hit] = first + (beg[hit] >> shift)
        done |= hit
    return out


def entries(text, cf):
    """the entries of the text, a column each (name index in order of first appearance, beg0, end0, line begin, line end), and the names;
    Refused with the 1-based line and the code where the rule refuses"""
    fmt, cs, cb, ce, meta, skip = cf
    names, seen, rows, prev = [], {}, [], None
    at, line_no = 0, 0
    while at < len(text):
        nl = text.find(b"\n", at)
        end, nxt = (len(text), len(text)) if nl < 0 else (nl, nl + 1)
        line, begin = text[at:end], at
        at = nxt; line_no += 1
        if line_no <= skip:
            continue
        if not line:
            raise Refused(line_no, E_EMPTY)
        if len(line) > 511:
            raise Refused(line_no, E_LONG)
        if line[0] == meta:
            continue
        f = line.split(b"\t")
        if len(f) < max(cs, cb, ce):
            raise Refused(line_no, E_FEW)
        if not re.fullmatch(rb"[0-9]{1,10}", f[cb - 1]) or not re.fullmatch(rb"[0-9]{1,10}", f[ce - 1]):
            raise Refused(line_no, E_COORD)
        vb, ve = int(f[cb - 1]), int(f[ce - 1])
        beg0, end0 = (vb, ve) if fmt & UCSC else (vb - 1, ve)
        if beg0 < 0 or end0 <= beg0:
            raise Refused(line_no, E_RANGE)
        if end0 > 1 << 29:
            raise Refused(line_no, E_BIG)
        name = f[cs - 1]
        if not name or len(name) > 255:
            raise Refused(line_no, E_NAME)
        if prev is not None and prev[0] == name and beg0 < prev[1]:
            raise Refused(line_no, E_ORDER)
        if (prev is None or prev[0] != name):
            if name in seen:
                raise Refused(line_no, E_RETURN)
            seen[name] = len(names); names.append(name)
        rows.append((seen[name], beg0, end0, begin, nxt))
        prev = (name, beg0)
    cols = np.array(rows, dtype=np.int64).reshape(-1, 5).T
    return cols, names


def payload(text, raw, cf):
    """the .tbi payload of the BGZF file `raw` whose decompressed text is `text`"""
    (tid, beg0, end0, lbeg, lend), names = entries(text, cf)
    mem, total = members(raw)
    assert total == len(text)
    holds = [(c, u, n) for c, u, n in mem if n]
    starts = np.array([u for _, u, _ in holds], dtype=np.int64)
    c_end = holds[-1][0] + struct.unpack_from("<H", raw, holds[-1][0] + 16)[0] + 1 if holds else 0

    def voff(u):
        if u >= total:
            return c_end << 16
        j = int(np.searchsorted(starts, u, side="right")) - 1
        return holds[j][0] << 16 | (u - holds[j][1])

    out = [b"TBI\x01", struct.pack("<7i", len(names), *cf), struct.pack("<i", sum(len(n) + 1 for n in names))] + [n + b"\0" for n in names]
    bins = reg2bin(beg0, end0) if len(tid) else np.zeros(0, dtype=np.int64)
    for t in range(len(names)):
        rows = np.nonzero(tid == t)[0]                               # consecutive: a name does not return
        assert rows[-1] - rows[0] + 1 == len(rows)
        b = bins[rows]
        first = np.nonzero(np.concatenate(([True], b[1:] != b[:-1])))[0]
        last = np.concatenate((first[1:], [len(rows)])) - 1
        run_bin, run_beg, run_end = b[first], lbeg[rows][first], lend[rows][last]
        order = np.argsort(run_bin, kind="stable")
        distinct = np.unique(run_bin)
        out.append(struct.pack("<i", len(distinct) + 1))
        for x in distinct:
            sel = order[run_bin[order] == x]
            out.append(struct.pack("<Ii", int(x), len(sel)))
            out += [struct.pack("<QQ", voff(int(run_beg[k])), voff(int(run_end[k]))) for k in sel]
        out.append(struct.pack("<IiQQQQ", 37450, 2, voff(int(lbeg[rows][0])), voff(int(lend[rows][-1])), len(rows), 0))
        w0, w1 = beg0[rows] >> 14, (end0[rows] - 1) >> 14
        ioff = np.full(int(w1.max()) + 1, -1, dtype=np.int64)
        for k in np.argsort(-lbeg[rows], kind="stable"):             # later lines first: the smallest begin is written last
            ioff[w0[k]:w1[k] + 1] = lbeg[rows][k]
        for w in range(len(ioff) - 2, -1, -1):
            if ioff[w] < 0:
                ioff[w] = ioff[w + 1]
        out.append(struct.pack("<i", len(ioff)))
        out += [struct.pack("<Q", voff(int(u))) for u in ioff]
    out.append(struct.pack("<Q", 0))
    return b"".join(out)


def emu(path, cf, out, raw_payload=False):
    """tools/tabix_emu on a file: the CompletedProcess"""
    return subprocess.run([str(EMU)] + (["--payload"] if raw_payload else []) + [str(path)] + [str(x) for x in cf] + [str(out)], capture_output=True, text=True)


# ---- the reader: the specification alone ----
def read_tbi(data):
    p = gzip.decompress(data)
    assert p[:4] == b"TBI\x01"
    n_ref, fmt, cs, cb, ce, meta, skip, l_nm = struct.unpack_from("<8i", p, 4)
    o = 36
    names = p[o:o + l_nm].split(b"\0")[:-1] if l_nm else []
    assert len(names) == n_ref
    o += l_nm
    refs = []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", p, o); o += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", p, o); o += 8
            bins[b] = [struct.unpack_from("<QQ", p, o + 16 * k) for k in range(n_chunk)]
            o += 16 * n_chunk
        n_intv, = struct.unpack_from("<i", p, o); o += 4
        ioff = list(struct.unpack_from(f"<{n_intv}Q", p, o)); o += 8 * n_intv
        refs.append((bins, ioff))
    rest = p[o:]
    assert rest in (b"", struct.pack("<Q", 0))
    return {"conf": (fmt, cs, cb, ce, meta, skip), "names": names, "refs": refs, "payload": p}


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


def interval(line, cf):
    fmt, cs, cb, ce, meta, skip = cf
    f = line.split(b"\t")
    vb, ve = int(f[cb - 1]), int(f[ce - 1])
    return f[cs - 1], (vb if fmt & UCSC else vb - 1), ve


@functools.lru_cache(maxsize=4096)
def _member(raw, c):
    """the member at file offset c inflated, and its length in the file (kept: the grid asks for the same members again and again)"""
    xlen = struct.unpack_from("<H", raw, c + 10)[0]
    bs = struct.unpack_from("<H", raw, c + 16)[0] + 1
    return zlib.decompress(raw[c + 12 + xlen:c + bs - 8], -15), bs


def read_from(raw, vbeg, vend):
    """the decompressed bytes of the BGZF file `raw` from virtual offset vbeg up to vend"""
    out, c, o = [], vbeg >> 16, vbeg & 0xffff
    while c < len(raw) and (c << 16) < vend:
        d, bs = _member(raw, c)
        hi = vend & 0xffff if vend >> 16 == c else len(d)
        out.append(d[o:hi])
        c += bs; o = 0
    return b"".join(out)


def query(raw, tbi, name, beg, end, stats=None):
    """the lines of `raw` that overlap name:[beg, end), through the index alone"""
    if name not in tbi["names"] or end <= beg:
        return []
    bins, ioff = tbi["refs"][tbi["names"].index(name)]
    if beg >> 14 >= len(ioff):
        return []
    low = ioff[beg >> 14]
    chunks = sorted(ch for b in reg2bins(beg, min(end, 1 << 29)) if b in bins for ch in bins[b] if ch[1] > low)
    out = []
    for vb, ve in chunks:
        text = read_from(raw, vb, ve)
        assert text.endswith(b"\n") or ve >> 16 >= len(raw) - 28
        for line in text.split(b"\n"):
            if not line or line[0] == tbi["conf"][4]:
                continue
            n, b0, e0 = interval(line, tbi["conf"])
            if n == name and b0 < end and e0 > beg:
                out.append(line)
    if stats is not None:
        stats["chunks"] = len(chunks)
    return out


@functools.lru_cache(maxsize=4)
def _all_lines(raw, cf):
    return [interval(line, cf) + (line,) for k, line in enumerate(gzip.decompress(raw).split(b"\n")) if k >= cf[5] and line and line[0] != cf[4]]


def brute(raw, cf, name, beg, end):
    """the yardstick: every line of the decompressed file against the region"""
    return [line for n, b0, e0, line in _all_lines(raw, cf) if n == name and b0 < end and e0 > beg]


EDGES = [0, 1, 16383, 16384, 16385, 131071, 131072, 131073, 1048575, 1048576, 8388607, 8388608, 8388609, 67108863, 67108864, 67108865, 69999999, 1 << 29]


def grid(names, edges=EDGES):
    """regions over every name and one the file does not hold: every pair of edges, one-base regions at each"""
    out = []
    for n in list(names) + [b"nowhere"]:
        out += [(n, a, b) for i, a in enumerate(edges) for b in edges[i + 1:]] + [(n, a, a + 1) for a in edges[:-1]]
    return out


# ---- the tables ----
CONTIGS = ["chrA", "chrNone", "chrLong"]
LENGTHS = [200000, 5000, 70000000]
STRADDLE = [16383, 131071, 1048575, 8388607, 67108863]                 # end = start + 2: a boundary of every level, up to bin 0
HEADER = b'track type="bedGraph" description="t CpG methylation levels"\n'
MK_HEADER = b"chrBase\tchr\tbase\tstrand\tcoverage\tfreqC\tfreqT\n"


def calls_table(seed=20261019):
    """~6,000 rows as columns (numpy): chrA and chrLong have rows, chrNone none; the straddling rows; two rows that share a start"""
    rng = np.random.default_rng(seed)
    a = np.sort(rng.choice(LENGTHS[0] - 2, 3000, replace=False))
    b = np.sort(rng.choice(LENGTHS[2] - 2, 2990, replace=False))
    b = b[~np.isin(b, STRADDLE) & ~np.isin(b, np.array(STRADDLE) + 1)]
    b = np.sort(np.concatenate((b, STRADDLE, b[100:101])))             # b[100] twice
    start = np.concatenate((a, b)).astype(np.int32)
    end = start + 1
    end[np.isin(start, STRADDLE) & (np.arange(len(start)) >= len(a))] += 1
    n = len(start)
    return {"contig": np.concatenate((np.zeros(len(a)), np.full(len(b), 2))).astype(np.int32), "start": start, "end": end.astype(np.int32),
            "nmeth": rng.integers(1, 40, n).astype(np.int32), "nunmeth": rng.integers(0, 40, n).astype(np.int32),
            "context": np.zeros(n, dtype=np.uint8), "strand": np.where(rng.integers(0, 2, n) == 1, 1, -1).astype(np.int8)}


def bed_text(t, contigs=CONTIGS, header=HEADER):
    return header + b"".join(b"%s\t%d\t%d\t%d\t%d\t%d\n" % (contigs[c].encode(), s, e, 100 * m // (m + u), m, u)
                             for c, s, e, m, u in zip(t["contig"], t["start"], t["end"], t["nmeth"], t["nunmeth"]))


def methylkit_text(t, contigs=CONTIGS):
    return MK_HEADER + b"".join(b"%s.%d\t%s\t%d\t%s\t%d\t%.2f\t%.2f\n" % (contigs[c].encode(), s + 1, contigs[c].encode(), s + 1, b"F" if st > 0 else b"R", m + u, 100.0 * m / (m + u), 100.0 * u / (m + u))
                                for c, s, m, u, st in zip(t["contig"], t["start"], t["nmeth"], t["nunmeth"], t["strand"]))


def report_text(t, contigs=CONTIGS):
    return b"".join(b"%s\t%d\t%s\t%d\t%d\tCG\tCGA\n" % (contigs[c].encode(), s + 1, b"+" if st > 0 else b"-", m, u)
                    for c, s, m, u, st in zip(t["contig"], t["start"], t["nmeth"], t["nunmeth"], t["strand"]))


def cpu_tables():
    """{name: (text, conf, cuts, eof)}: every table of the CPU tests, with the way its BGZF file is cut"""
    t = calls_table()
    bed, mk, rep = bed_text(t), methylkit_text(t), report_text(t)
    small = bed[:bed.index(b"\n", 3000) + 1]
    nl = small.index(b"\n", 200) + 1                                      # a member that ends exactly on a newline
    alt = HEADER + b"".join(b"c\t%d\t%d\t0\t1\t1\n" % (16000 + k, 16400 if k % 2 else 16001 + k) for k in range(380))      # bins alternate line by line: a leaf, its parent
    meta = HEADER + b"#c\n" + b"x\t5\t6\t0\t1\t1\n#between\n#two\nx\t7\t9\t0\t1\t1\nx\t20000\t20001\t0\t1\t1\n#mid\ny\t1\t2\t0\t1\t1\n#last\n"
    return {
        "bed": (bed, conf("bed", 1), 65280, True),
        "bed_1000": (bed, conf("bed", 1), 1000, True),
        "bed_7": (small, conf("bed", 1), 7, False),
        "methylKit": (mk, conf("methylKit", 1), 65280, True),
        "report": (rep, conf("cytosine_report", 0), 65280, True),
        "report_4097": (rep, conf("cytosine_report", 0), 4097, False),
        "header_only": (HEADER, conf("bed", 1), 65280, True),
        "empty": (b"", conf("bed", 0), 65280, True),
        "ends_on_newline": (small, conf("bed", 1), [nl, 1000], True),
        "one_byte_members": (small[:small.index(b"\n", 600) + 1], conf("bed", 1), 1, True),
        "empty_member": (small, conf("bed", 1), [500, 0, 0, 700, 0, 900], True),
        "no_last_newline": (small[:-1], conf("bed", 1), 300, True),
        "alternating": (alt, conf("bed", 1), 65280, True),
        "meta_lines": (meta, conf("bed", 1), 40, True),
        "longest_line": (HEADER + b"c\t1\t2\t" + b"9" * 505 + b"\nc\t3\t4\n", conf("bed", 1), 100, True),          # 511 bytes before the newline
        "skip_3": (b"a\nb\n\n" + small[len(HEADER):], conf("bed", 3), 2000, True),
    }


def refusals():
    """[(name, text behind the header, conf, 1-based line of the whole text, code)]"""
    ok = [b"c\t%d\t%d\t0\t1\t1\n" % (p, p + 1) for p in range(10, 400, 10)]
    cf, mk = conf("bed", 1), conf("methylKit", 1)

    def at(k, bad, c=cf, lines=ok):
        return (b"".join(lines[:k]) + bad + b"".join(lines[k:]), c, k + 2)

    out = [("few", *at(5, b"c\t55\n"), E_FEW), ("nondigit", *at(7, b"c\t5x\t80\t0\n"), E_COORD), ("empty_coord", *at(0, b"c\t\t80\n"), E_COORD),
           ("sign", *at(3, b"c\t-1\t80\n"), E_COORD), ("eleven_digits", *at(3, b"c\t35\t12345678901\n"), E_COORD), ("end_before", *at(9, b"c\t95\t95\t0\t1\t1\n"), E_RANGE),
           ("past_512mb", *at(38, b"c\t536870911\t536870913\t0\t1\t1\n"), E_BIG), ("no_name", *at(4, b"\t45\t46\n"), E_NAME),
           ("long_name", *at(39, b"d" * 256 + b"\t45\t46\n"), E_NAME), ("long_line", *at(39, b"c\t400\t401\t" + b"9" * 502 + b"\n"), E_LONG),
           ("empty_line", *at(20, b"\n"), E_EMPTY), ("unsorted", *at(30, b"c\t5\t6\t0\t1\t1\n"), E_ORDER),
           ("returns", b"".join(ok[:5]) + b"d\t1\t2\n" + b"".join(ok[5:]), cf, 8, E_RETURN),
           ("few_before_bad_coord", *at(2, b"c\tx\n"), E_FEW), ("two_bad_lines", *at(6, b"c\t1\t1\n" + b"\n"), E_RANGE),
           ("zero_position", MK_HEADER + b"c.0\tc\t0\tF\t1\t0\t0\n", mk, 2, E_RANGE)]
    return [(n, (t if c is mk else HEADER + t), c, line, code) for n, t, c, line, code in out]
