"""The rule of csrc/mdk_bigwig_core.h restated in Python and numpy -- float64 and float32 with the rule's own order of operations, one numpy
operation per rounding --, a reader that takes a bigWig apart with nothing but struct and zlib, and the tables the tests of the bigWig
writer share (test_bigwig_cpu.py drives tools/bigwig_emu with them; a device writer is to be held to the same)."""
import struct
import subprocess
import zlib
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
EMU = REPO / "tools" / "_build" / "bigwig_emu"
MAGIC, CHROM_MAGIC, RTREE_MAGIC = 0x888FFC26, 0x78CA8C91, 0x2468ACE0
ITEMS, ZITEMS, BLOCK, LEVELS = 1024, 512, 256, 8
E_ROW, E_NEGATIVE, E_EMPTY, E_ORDER, E_OVERLAP = 1, 2, 3, 4, 5
MESSAGES = {E_ROW: "its contig is not in the list", E_NEGATIVE: "a negative count", E_EMPTY: "nmeth + nunmeth is 0",
            E_ORDER: "strictly ascending", E_OVERLAP: "pass one context"}


class Refused(Exception):
    def __init__(self, code, row):
        super().__init__(f"row {row}: {MESSAGES[code]}")
        self.code, self.row = code, row


def width(k):
    return 1024 * 4 ** k


# ------------------------------------------------------------------------------------------------
# the reader
# ------------------------------------------------------------------------------------------------
def _chrom_walk(d, off, key, out):
    leaf, _, count = struct.unpack_from("<BBH", d, off)
    assert count <= BLOCK
    keys = []
    for i in range(count):
        o = off + 4 + i * (key + 8)
        k = d[o:o + key]
        keys.append(k)
        if leaf:
            out.append((k.rstrip(b"\0").decode(),) + struct.unpack_from("<II", d, o + key))
        else:
            first = len(out)
            _chrom_walk(d, struct.unpack_from("<Q", d, o + key)[0], key, out)
            assert out[first][0].encode().ljust(key, b"\0") == k            # a node's key is its subtree's first
    assert keys == sorted(keys)
    return out


def _rtree(d, off, data_begin, data_end, per_slot):
    """the leaves of the R-tree at ``off``, walked from the root: [(c0, s0, c1, e1, offset, size)] in file order.  Every section of
    [data_begin, data_end) must be reached exactly once, inside the bounds of every node above it"""
    magic, block, n, c0, s0, c1, e1, end_off, slot, _ = struct.unpack_from("<IIQIIIIQII", d, off)
    assert magic == RTREE_MAGIC and block == BLOCK and slot == per_slot and end_off == data_end == off
    leaves, depth = [], []

    def walk(o, lo, hi, level):
        leaf, _, count = struct.unpack_from("<BBH", d, o)
        assert count <= BLOCK
        for i in range(count):
            it = struct.unpack_from("<IIIIQQ" if leaf else "<IIIIQ", d, o + 4 + i * (32 if leaf else 24))
            assert lo <= (it[0], it[1]) and (it[2], it[3]) <= hi and (it[0], it[1]) < (it[2], it[3]), (it, lo, hi)
            if leaf:
                leaves.append(it); depth.append(level)
            else:
                assert count >= 1
                walk(it[4], (it[0], it[1]), (it[2], it[3]), level + 1)

    walk(off + 48, (c0, s0), (c1, e1), 0)
    assert len(leaves) == n and len(set(depth)) <= 1                          # complete: every leaf at one depth
    at = data_begin
    for it in sorted(leaves, key=lambda it: it[4]):                            # reached once each, and together they are all of the data
        assert it[4] == at and it[5] > 0, (it, at)
        at += it[5]
    assert at == data_end
    assert leaves == sorted(leaves, key=lambda it: it[4])
    if leaves:
        assert (c0, s0) == (leaves[0][0], leaves[0][1]) and (c1, e1) == max((it[2], it[3]) for it in leaves)
    else:
        assert (c0, s0, c1, e1) == (0, 0, 0, 0)
    return leaves, (len(set(depth)) and depth[0] + 1)


def _inflate(d, leaf, bufsize):
    comp = d[leaf[4]:leaf[4] + leaf[5]]
    assert comp[:2] == b"\x78\x9c"
    z = zlib.decompressobj()
    raw = z.decompress(comp)
    assert z.eof and not z.unused_data and 0 < len(raw) <= bufsize
    assert struct.unpack(">I", comp[-4:])[0] == zlib.adler32(raw)
    return raw, comp


def read_bigwig(d):
    """everything a bigWig holds, from its bytes"""
    (magic, version, n_levels, chrom_at, data_at, index_at, fields, defined, autosql, summary_at, bufsize, reserved) = struct.unpack_from("<IHHQQQHHQQIQ", d, 0)
    assert magic == MAGIC and version == 4 and (fields, defined, autosql, reserved) == (0, 0, 0, 0)
    assert summary_at == 64 + 24 * n_levels and chrom_at == summary_at + 40
    assert struct.unpack_from("<I", d, len(d) - 4)[0] == MAGIC
    f = {"levels": n_levels, "uncompress": bufsize}
    f["summary"] = struct.unpack_from("<Qdddd", d, summary_at)
    cmagic, block, key, val, n_chrom, _ = struct.unpack_from("<IIIIQQ", d, chrom_at)
    assert cmagic == CHROM_MAGIC and block == BLOCK and val == 8
    chroms = _chrom_walk(d, chrom_at + 32, key, [])
    assert len(chroms) == n_chrom and sorted(c[1] for c in chroms) == list(range(n_chrom))
    f["chroms"] = [(name, length) for name, _, length in sorted(chroms, key=lambda c: c[1])]
    f["key"] = key
    f["count"] = struct.unpack_from("<Q", d, data_at)[0]
    leaves, f["index_depth"] = _rtree(d, index_at, data_at + 8, index_at, ITEMS)
    assert len(leaves) == f["count"]
    sections, stored, sizes = [], 0, []
    for leaf in leaves:
        raw, comp = _inflate(d, leaf, bufsize)
        c, s, e, step, span, kind, _, cnt = struct.unpack_from("<IIIIIBBH", raw, 0)
        assert (step, span, kind) == (0, 0, 1) and 1 <= cnt <= ITEMS and len(raw) == 24 + 12 * cnt
        items = np.frombuffer(raw, dtype="<u4", offset=24).reshape(cnt, 3)
        assert (c, s, c, e) == leaf[:4] and s == items[0, 0] and e == items[-1, 1]
        sections.append((c, items))
        stored += comp[2] & 7 == 1                                             # BFINAL 1, BTYPE 00
        sizes.append((len(raw), len(comp)))
        assert len(comp) <= len(raw) + 11                                     # 2 + 5 + 4: no section outgrows its raw form by more than the framing
    f["sections"], f["stored"], f["sizes"] = sections, stored, sizes
    f["zoom"] = []
    at = index_at                                                              # the levels follow the main index, a level after the other
    for k in range(n_levels):
        reduction, _, zdata, zindex = struct.unpack_from("<IIQQ", d, 64 + 24 * k)
        n_rec = struct.unpack_from("<I", d, zdata)[0]
        zl, depth = _rtree(d, zindex, zdata + 4, zindex, ZITEMS)
        recs = []
        for leaf in zl:
            raw, _ = _inflate(d, leaf, bufsize)
            assert len(raw) % 32 == 0 and len(raw) <= 32 * ZITEMS
            r = np.frombuffer(raw, dtype="<u4").reshape(-1, 8)
            assert (r[0, 0], r[0, 1], r[-1, 0], r[-1, 2]) == leaf[:4]
            recs.append(r)
        assert all(len(r) == ZITEMS for r in recs[:-1])
        recs = np.concatenate(recs) if recs else np.zeros((0, 8), "<u4")
        assert len(recs) == n_rec
        f["zoom"].append({"reduction": reduction, "records": recs, "index_depth": depth})
        assert zdata > at
        at = zindex
    return f


# ------------------------------------------------------------------------------------------------
# the expectation
# ------------------------------------------------------------------------------------------------
def values(m, u, value):
    m64, cov = m.astype(np.int64), m.astype(np.int64) + u.astype(np.int64)
    if value == "coverage":
        return cov.astype(np.float32)
    return ((m64.astype(np.float64) * np.float64(100.0)) / cov.astype(np.float64)).astype(np.float32)


def check(lengths, cols, value):
    """Refused for the row the rule names: the smallest row number, of two refusals of one row the smaller code"""
    c, s, e, m, u = (cols[k].astype(np.int64) for k in ("contig", "start", "end", "nmeth", "nunmeth"))
    n, L = len(c), np.asarray(lengths, dtype=np.int64)
    keys = []
    inside = (c >= 0) & (c < len(L))
    bad = ~inside | (s < 0) | (e <= s)
    bad[inside] |= e[inside] > L[c[inside]]
    keys += [(int(i), E_ROW) for i in np.nonzero(bad)[0]]
    keys += [(int(i), E_NEGATIVE) for i in np.nonzero(~bad & ((m < 0) | (u < 0)))[0]]
    if value == "percent":
        keys += [(int(i), E_EMPTY) for i in np.nonzero(~bad & (m >= 0) & (u >= 0) & (m + u == 0))[0]]
    if n > 1:
        order = (c[1:] < c[:-1]) | ((c[1:] == c[:-1]) & (s[1:] <= s[:-1]))
        keys += [(int(i) + 1, E_ORDER) for i in np.nonzero(order)[0]]
        keys += [(int(i), E_OVERLAP) for i in np.nonzero(~order & (c[1:] == c[:-1]) & (e[:-1] > s[1:]))[0]]
    if keys:
        row, code = min(keys)
        raise Refused(code, row)


def _ordered_sum(n_bins, bins, terms):
    """per bin, its terms added one after the other in the order they stand in (float64, one rounding per addition)"""
    acc = np.zeros(n_bins, dtype=np.float64)
    if len(bins):
        start = np.r_[0, np.nonzero(np.diff(bins))[0] + 1]                      # bins is ascending: the first term of every bin
        rank = np.arange(len(bins)) - np.repeat(start, np.diff(np.r_[start, len(bins)]))
        for r in range(int(rank.max()) + 1):
            sel = rank == r
            acc[bins[sel]] = acc[bins[sel]] + terms[sel]
    return acc


def expect(lengths, cols, value):
    """what the file must hold: the items, the sections' cuts, the records of all eight levels, which of them are written, the summary"""
    check(lengths, cols, value)
    c, s, e = (cols[k].astype(np.int64) for k in ("contig", "start", "end"))
    v = values(cols["nmeth"], cols["nunmeth"], value)
    n, L = len(c), np.asarray(lengths, dtype=np.int64)
    out = {"items": np.stack([s, e, v.view(np.uint32).astype(np.int64)], axis=1).astype(np.uint32) if n else np.zeros((0, 3), np.uint32), "contig": c}
    cuts = []
    for t in range(len(L)):
        rows = np.nonzero(c == t)[0]
        cuts += [(t, int(rows[0]) + k, min(ITEMS, len(rows) - k)) for k in range(0, len(rows), ITEMS)]
    out["cuts"] = cuts
    # level 0: a row's bases in every bin it touches, in the rows' order
    nb = [(L + width(k) - 1) // width(k) for k in range(LEVELS)]
    base = [np.r_[0, np.cumsum(b)] for b in nb]
    pieces = []
    j = 0
    while n:
        lo = ((s >> 10) + j) << 10
        sel = lo < e
        if not sel.any():
            break
        a, b = np.maximum(s[sel], lo[sel]), np.minimum(e[sel], lo[sel] + 1024)
        pieces.append((base[0][c[sel]] + (lo[sel] >> 10), np.nonzero(sel)[0], b - a, v[sel]))
        j += 1
    levels = []
    if pieces:
        gb, row, bases, val = (np.concatenate([p[i] for p in pieces]) for i in range(4))
        o = np.lexsort((row, gb))
        gb, bases, val = gb[o], bases[o], val[o]
    else:
        gb, bases, val = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    T = int(base[0][-1])
    dv, db = val.astype(np.float64), bases.astype(np.float64)
    lvl = {"valid": np.bincount(gb, weights=bases, minlength=T).astype(np.int64)[:T] if T else np.zeros(0, np.int64),
           "sum": _ordered_sum(T, gb, dv * db), "sq": _ordered_sum(T, gb, (dv * dv) * db),
           "mn": np.zeros(T, np.float32), "mx": np.zeros(T, np.float32)}
    if len(gb):
        mn, mx = np.full(T, np.inf, np.float32), np.full(T, -np.inf, np.float32)
        np.minimum.at(mn, gb, val); np.maximum.at(mx, gb, val)
        lvl["mn"], lvl["mx"] = np.where(lvl["valid"] > 0, mn, np.float32(0)), np.where(lvl["valid"] > 0, mx, np.float32(0))
    levels.append(lvl)
    for k in range(1, LEVELS):
        T = int(base[k][-1])
        up = {"valid": np.zeros(T, np.int64), "sum": np.zeros(T), "sq": np.zeros(T), "mn": np.zeros(T, np.float32), "mx": np.zeros(T, np.float32)}
        below = levels[-1]
        for t in range(len(L)):
            kids, mine = int(nb[k - 1][t]), int(nb[k][t])
            b0, p0 = int(base[k - 1][t]), int(base[k][t])
            for jj in range(4):
                idx = np.arange(mine) * 4 + jj
                idx = idx[idx < kids]
                par = p0 + np.arange(len(idx))
                ch = b0 + idx
                on = below["valid"][ch] > 0
                par, ch = par[on], ch[on]
                fresh = up["valid"][par] == 0
                up["sum"][par] = up["sum"][par] + below["sum"][ch]
                up["sq"][par] = up["sq"][par] + below["sq"][ch]
                up["mn"][par] = np.where(fresh, below["mn"][ch], np.minimum(up["mn"][par], below["mn"][ch]))
                up["mx"][par] = np.where(fresh, below["mx"][ch], np.maximum(up["mx"][par], below["mx"][ch]))
                up["valid"][par] += below["valid"][ch]
        levels.append(up)
    out["records"] = []
    for k in range(LEVELS):
        lv, w = levels[k], width(k)
        on = np.nonzero(lv["valid"] > 0)[0]
        t = np.searchsorted(base[k], on, side="right") - 1
        b = on - base[k][t]
        rec = np.zeros((len(on), 8), np.uint32)
        rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = t, b * w, np.minimum((b + 1) * w, L[t]), lv["valid"][on]
        rec[:, 4], rec[:, 5] = lv["mn"][on].view(np.uint32), lv["mx"][on].view(np.uint32)
        rec[:, 6], rec[:, 7] = lv["sum"][on].astype(np.float32).view(np.uint32), lv["sq"][on].astype(np.float32).view(np.uint32)
        out["records"].append(rec)
    last, out["written"] = n, []
    for k in range(LEVELS):
        if 2 * len(out["records"][k]) < last:
            out["written"].append(k); last = len(out["records"][k])
    top = levels[-1]
    bases_cov, mn, mx, sm, sq = 0, 0.0, 0.0, 0.0, 0.0
    for i in range(len(top["valid"])):
        if top["valid"][i]:
            mn = float(top["mn"][i]) if not bases_cov else min(mn, float(top["mn"][i]))
            mx = float(top["mx"][i]) if not bases_cov else max(mx, float(top["mx"][i]))
            sm, sq = sm + float(top["sum"][i]), sq + float(top["sq"][i])
            bases_cov += int(top["valid"][i])
    out["summary"] = (bases_cov, mn, mx, sm, sq)
    return out


def compare(data, contigs, cols, value):
    """the file ``data`` against the expectation, bit for bit; what the reader found, for the caller's own checks"""
    f = read_bigwig(data)
    x = expect([l for _, l in contigs], cols, value)
    assert f["chroms"] == list(contigs) and f["key"] == max([1] + [len(n.encode()) for n, _ in contigs])
    assert f["count"] == len(x["cuts"]) == len(f["sections"])
    for (c, items), (t, r0, cnt) in zip(f["sections"], x["cuts"]):
        assert c == t and len(items) == cnt and np.array_equal(items, x["items"][r0:r0 + cnt]), (t, r0)
    assert f["uncompress"] == max([0] + [24 + 12 * cnt for _, _, cnt in x["cuts"]] + [32 * min(ZITEMS, len(x["records"][k])) for k in x["written"]])
    assert [z["reduction"] for z in f["zoom"]] == [width(k) for k in x["written"]]
    for z, k in zip(f["zoom"], x["written"]):
        assert np.array_equal(z["records"], x["records"][k]), k
    assert struct.pack("<Qdddd", *f["summary"]) == struct.pack("<Qdddd", *x["summary"]), (f["summary"], x["summary"])
    f["expected"] = x
    return f


# ------------------------------------------------------------------------------------------------
# the emulator, and the tables
# ------------------------------------------------------------------------------------------------
def emu(tmp, contigs, cols, value):
    """tools/bigwig_emu over the table: (exit status, the file's bytes or None, stderr)"""
    tmp = Path(tmp)
    (tmp / "contigs.tsv").write_text("".join(f"{n}\t{l}\n" for n, l in contigs))
    np.savetxt(tmp / "rows.tsv", np.stack([cols[k].astype(np.int64) for k in ("contig", "start", "end", "nmeth", "nunmeth")], axis=1).reshape(-1, 5), fmt="%d")
    out = tmp / "emu.bw"
    r = subprocess.run([str(EMU)] + (["--coverage"] if value == "coverage" else []) + [str(tmp / "contigs.tsv"), str(tmp / "rows.tsv"), str(out)], capture_output=True, text=True)
    return r.returncode, (out.read_bytes() if r.returncode == 0 else None), r.stderr


def table(contig, start, end, m, u, context=None):
    n = len(contig)
    return {"contig": np.asarray(contig, np.int32), "start": np.asarray(start, np.int32), "end": np.asarray(end, np.int32),
            "nmeth": np.asarray(m, np.int32), "nunmeth": np.asarray(u, np.int32),
            "context": np.zeros(n, np.uint8) if context is None else np.asarray(context, np.uint8), "strand": np.ones(n, np.int8)}


def _hash(i, salt):
    x = (np.asarray(i, np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(29); x *= np.uint64(0xBF58476D1CE4E5B9); x ^= x >> np.uint64(32)
    return x


def _run(n, step=3, first=7, contig=0, salt=1, depth=40):
    i = np.arange(n)
    cov = 1 + (_hash(i, salt) % np.uint64(depth)).astype(np.int64)
    m = (_hash(i, salt + 77) % (cov.astype(np.uint64) + np.uint64(1))).astype(np.int64)
    return np.full(n, contig), first + step * i, first + step * i + 1, m, cov - m


def _cat(*runs):
    return table(*[np.concatenate([r[k] for r in runs]) for k in range(5)])


def cases():
    """name -> (contigs, columns, value).  Every table is valid"""
    C = {}
    two = [("chr1", 5000), ("chr2", 100)]
    C["no_rows"] = (two, table([], [], [], [], []), "percent")
    C["one_row"] = (two, table([1], [42], [43], [3], [1]), "percent")
    for n in (1023, 1024, 1025):
        C[f"rows_{n}"] = ([("chr1", 40000)], _cat(_run(n)), "percent")
    # the first contig ends inside a section, the next has no row, a name sorts before its neighbours
    C["contig_ends_mid_section"] = ([("chrB", 5000), ("chrEmpty", 3000), ("chrA", 9000)], _cat(_run(1500, 3, 7, 0), _run(600, 5, 0, 2, salt=5)), "percent")
    # merged rows of two bases over the bin boundaries of level 0 (1024, 2048) and of level 1 (4096), among single bases
    r = _run(400, 20, 3)
    s, e = r[1].copy(), r[2].copy()
    for at in (1024, 2048, 4096):
        k = np.argmin(np.abs(s - at))
        s[k], e[k] = at - 1, at + 1
    C["rows_straddle_bins"] = ([("chr1", 10000)], table(r[0], s, e, r[3], r[4]), "percent")
    # a row at a contig's last base: a contig that ends inside a bin, and one that ends on a bin's edge
    C["last_base"] = ([("chr1", 5000), ("chr2", 2048)], table([0, 0, 1, 1], [17, 4999, 1000, 2047], [18, 5000, 1002, 2048], [1, 2, 3, 0], [1, 0, 4, 9]), "percent")
    # 257 sections and 300 contigs: the R-tree and the chromosome tree get a second level
    many = [(f"c{t}", 257 * 1024 * 8 + 100 if t == 3 else 50 + t) for t in range(300)]
    C["sections_257"] = (many, _cat(_run(2, 9, 1, 2), _run(257 * 1024 - 2, 8, 5, 3, salt=9), _run(3, 4, 0, 299)), "percent")
    # hashed starts and counts.  A full section of valid rows still has structure -- starts ascend, an end is near its start, the floats share
    # their exponents --, so a dynamic block wins by a few percent ("hashed_full"); sections of eight such rows have too little of it to pay for a
    # dynamic block's header and are stored ("hashed"); one value at a regular distance is a few bytes a section ("constant")
    i = np.arange(3000)
    st = np.cumsum(1 + (_hash(i, 3) % np.uint64(600000)).astype(np.int64))
    C["hashed_full"] = ([("chr1", int(st[-1]) + 50)], table(np.zeros(3000), st, st + 1, (_hash(i, 4) % np.uint64(1 << 20)).astype(np.int64), 1 + (_hash(i, 5) % np.uint64(1 << 20)).astype(np.int64)), "percent")
    j = np.arange(320)
    gap = 1 + (_hash(j, 3) % np.uint64(3000000)).astype(np.int64)
    C["hashed"] = ([(f"k{t}", 40000000) for t in range(40)], table(j // 8, np.concatenate([np.cumsum(gap[8 * t:8 * t + 8]) for t in range(40)]), np.concatenate([np.cumsum(gap[8 * t:8 * t + 8]) for t in range(40)]) + 1,
                                                                 (_hash(j, 4) % np.uint64(1 << 20)).astype(np.int64), 1 + (_hash(j, 5) % np.uint64(1 << 20)).astype(np.int64)), "percent")
    C["constant"] = ([("chr1", 3000 * 16 + 50)], table(np.zeros(3000), 16 * i, 16 * i + 1, np.full(3000, 5), np.full(3000, 5)), "percent")
    # a count above 2^24: the float of the sum is not the sum of the floats
    C["coverage_above_2_24"] = (two, table([0, 0, 0, 1], [5, 9, 2000, 7], [6, 11, 2001, 8], [(1 << 24) + 1, 2 ** 30, 0, 3], [2, 2 ** 30 + 129, 0, 4]), "coverage")
    return C


def refusals():
    """name -> (contigs, columns, value, code, row): one refusal each, then tables with two, where the first row wins"""
    two = [("chr1", 5000), ("chr2", 100)]
    base = _run(700, 3, 7)

    def with_rows(edit):
        cols = [x.copy() for x in base]
        edit(*cols)
        return table(*cols)

    def set_(k, i, v):
        def f(*cols):
            cols[k][i] = v
        return f

    R = {}
    R["zero_coverage"] = (two, with_rows(lambda c, s, e, m, u: (m.__setitem__(300, 0), u.__setitem__(300, 0))), "percent", E_EMPTY, 300)
    R["negative_count"] = (two, with_rows(set_(4, 650, -1)), "coverage", E_NEGATIVE, 650)
    R["not_ascending"] = (two, with_rows(set_(1, 257, base[1][256])), "percent", E_ORDER, 257)
    R["contig_descends"] = (two, with_rows(set_(0, 0, 1)), "percent", E_ORDER, 1)
    R["overlap"] = (two, with_rows(set_(2, 511, base[1][512] + 1)), "percent", E_OVERLAP, 511)
    R["past_the_contig"] = (two, with_rows(set_(0, 699, 1)), "percent", E_ROW, 699)
    R["contig_outside"] = (two, with_rows(set_(0, 699, 2)), "percent", E_ROW, 699)
    R["empty_interval"] = (two, with_rows(set_(2, 64, base[1][64])), "percent", E_ROW, 64)

    def both(c, s, e, m, u):
        m[600], u[600] = 0, 0
        e[100] = s[101] + 1
    R["the_first_of_two"] = (two, with_rows(both), "percent", E_OVERLAP, 100)
    return R
