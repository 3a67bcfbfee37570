"""TEST INFRASTRUCTURE: a deterministic zoo of raw deflate streams for the device inflate (k_inflate, k_crc32: csrc/mdk_inflate.hip,
csrc/mdk_inflate_core.h), a plain RFC 1951 parser that audits what each stream exercises, and the containers the tests hand them over in.

  build_zoo()        [Member(name, raw, stream)], every stream legal (zlib inflates it to `raw`).  Encoders: zlib at every level / strategy /
                     memLevel / window, flushes inside a member, libdeflate (ctypes, the library csrc/host/mdk_io.c loads) when present, and
                     BlockWriter, which writes tokens chosen one by one where no library goes (distances 32507..32768, single-code trees, an
                     empty dynamic block, 15-bit codes).
  malformed()        [(name, stream, out_len)]: streams the kernel must refuse -- wrong ISIZE, cut short, a distance behind byte 0.
  audit(stream)      block types, empty blocks, code lengths, distances, symbols per 608-bit stretch -- and the bytes.
  bgzf_file(...)     members as one BGZF file (tools/inflate_emu reads it); piece_layout(...): members as one md_piece_submit buffer.
Nothing here needs a GPU; the builder is deterministic, so nothing it makes is committed."""
import ctypes
import random
import struct
import zlib
from collections import namedtuple

Member = namedtuple("Member", "name raw stream")

SIZES = [0, 1, 2, 3, 4, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4096, 65280, 65535, 65536]
BGZF_MAX_STREAM = 65536 - 18 - 8          # BSIZE <= 65536 with the 18-byte header and the 8-byte trailer
STRETCH_BITS = 608                         # a lane's stretch of a Huffman batch (INF_SW_MAX = 19 words)
TOK_STEPS = 256                            # INF_TOK_STEPS

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLORD = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


def len_sym(n):
    for k in range(28, -1, -1):
        if n >= LBASE[k]:
            return k if n < 258 or k == 28 else 28
    raise ValueError(n)


def dist_sym(d):
    for k in range(29, -1, -1):
        if d >= DBASE[k]:
            return k
    raise ValueError(d)


def canonical(lens):
    """RFC 1951 3.2.2: code of every symbol (0 where its length is 0)"""
    bl = [0] * 16
    for l in lens:
        if l:
            bl[l] += 1
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        out.append(nxt[l] if l else 0)
        if l:
            nxt[l] += 1
    return out


def rev(v, n):
    r = 0
    for _ in range(n):
        r, v = (r << 1) | (v & 1), v >> 1
    return r


def huffman_lengths(freq, limit):
    """lengths of a Huffman code for `freq` (a complete code whenever two or more symbols are used), at most `limit` bits"""
    import heapq
    used = [i for i, f in enumerate(freq) if f]
    if len(used) == 1:
        out = [0] * len(freq); out[used[0]] = 1
        return out
    f = list(freq)
    while True:
        h = [(f[i], i, (i, )) for i in used]
        heapq.heapify(h)
        depth = [0] * len(freq); k = len(freq)
        while len(h) > 1:
            a, b = heapq.heappop(h), heapq.heappop(h)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(h, (a[0] + b[0], k, a[2] + b[2])); k += 1
        if max(depth) <= limit:
            return depth
        f = [(x + 1) // 2 if x else 0 for x in f]       # flatten the skew and try again


class BlockWriter:
    """A raw deflate stream, block by block, from tokens chosen one by one: an int is a literal, (length, distance) a match."""

    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, nbits):
        self.acc |= v << self.n; self.n += nbits
        while self.n >= 8:
            self.buf.append(self.acc & 255); self.acc >>= 8; self.n -= 8

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def getvalue(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.n else b"")

    def stored(self, data, final=False):
        assert len(data) <= 65535
        self.put(int(final), 1); self.put(0, 2); self.align()
        self.put(len(data), 16); self.put(len(data) ^ 0xffff, 16)
        self.buf += data

    def _tokens(self, tokens, lit_lens, dist_lens):
        lc, dc = canonical(lit_lens), canonical(dist_lens)
        lr = [rev(c, l) for c, l in zip(lc, lit_lens)]; dr = [rev(c, l) for c, l in zip(dc, dist_lens)]
        for t in list(tokens) + [256]:
            if isinstance(t, int):
                assert lit_lens[t], t
                self.put(lr[t], lit_lens[t])
            else:
                n, d = t; k, j = len_sym(n), dist_sym(d)
                assert lit_lens[257 + k] and dist_lens[j], (n, d)
                self.put(lr[257 + k], lit_lens[257 + k]); self.put(n - LBASE[k], LEXT[k])
                self.put(dr[j], dist_lens[j]); self.put(d - DBASE[j], DEXT[j])

    def fixed(self, tokens, final=False):
        self.put(int(final), 1); self.put(1, 2)
        self._tokens(tokens, FIXED_LIT, FIXED_DIST)

    def dynamic(self, tokens, final=False, lit_lens=None, dist_lens=None, runs=False):
        """lit_lens / dist_lens: given code lengths (any legal set), else a Huffman code of the tokens.  runs: the code lengths with the
        run-length codes 16 / 17 / 18 where they apply, else every length written as itself"""
        if lit_lens is None or dist_lens is None:
            lf, df = [0] * 286, [0] * 30
            lf[256] = 1
            for t in tokens:
                if isinstance(t, int):
                    lf[t] += 1
                else:
                    lf[257 + len_sym(t[0])] += 1; df[dist_sym(t[1])] += 1
            lit_lens = lit_lens or huffman_lengths(lf, 15)
            dist_lens = dist_lens if dist_lens is not None else (huffman_lengths(df, 15) if any(df) else [0])
        nlit = max(257, max(i for i, l in enumerate(lit_lens) if l) + 1)
        nd = [i for i, l in enumerate(dist_lens) if l]
        ndist = max(1, (nd[-1] + 1) if nd else 1)
        seq = list(lit_lens[:nlit]) + [0] * (nlit - len(lit_lens)) + list(dist_lens[:ndist]) + [0] * (ndist - len(dist_lens))
        cl = []                                           # (symbol, extra value, extra bits)
        i = 0
        while i < len(seq):
            v, r = seq[i], 1
            while i + r < len(seq) and seq[i + r] == v:
                r += 1
            if runs and v == 0 and r >= 11:
                r = min(r, 138); cl.append((18, r - 11, 7))
            elif runs and v == 0 and r >= 3:
                r = min(r, 10); cl.append((17, r - 3, 3))
            elif runs and v and r >= 4:
                cl.append((v, 0, 0)); r = min(r - 1, 6); cl.append((16, r - 3, 2)); r += 1
            else:
                r = 1; cl.append((v, 0, 0))
            i += r
        cf = [0] * 19
        for s, _, _ in cl:
            cf[s] += 1
        if sum(1 for x in cf if x) < 2:                   # a single code-length code would be an incomplete code: give it a partner
            cf[0 if not cf[0] else 1] += 1
        cll = huffman_lengths(cf, 7)
        ncode = max(4, max(k for k in range(19) if cll[CLORD[k]]) + 1)
        self.put(int(final), 1); self.put(2, 2)
        self.put(nlit - 257, 5); self.put(ndist - 1, 5); self.put(ncode - 4, 4)
        for k in range(ncode):
            self.put(cll[CLORD[k]], 3)
        cc = canonical(cll)
        for s, x, nb in cl:
            self.put(rev(cc[s], cll[s]), cll[s])
            if nb:
                self.put(x, nb)
        self._tokens(tokens, list(lit_lens[:nlit]) + [0] * (nlit - len(lit_lens)) + [0] * (286 - nlit), list(dist_lens[:ndist]) + [0] * (30 - ndist))


def apply_tokens(tokens, out=None):
    out = bytearray() if out is None else out
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            n, d = t
            for _ in range(n):
                out.append(out[-d])
    return out


# ---- the auditor: RFC 1951, written out plainly ----
class StreamError(Exception):
    pass


def _table(lens):
    """decode table of 2^maxlen entries: reversed code bits -> (symbol, length); None where no code starts"""
    mx = max(lens) if any(lens) else 0
    if mx == 0:
        return 0, []
    t = [None] * (1 << mx)
    for s, (c, l) in enumerate(zip(canonical(lens), lens)):
        if l:
            r = rev(c, l)
            for j in range(r, 1 << mx, 1 << l):
                t[j] = (s, l)
    return mx, t


def audit(stream, out_limit=1 << 20):
    """Walk a raw deflate stream.  Returns a dict: the bytes, and what the stream exercises."""
    data = bytes(stream) + b"\0" * 8
    nbits_total = 8 * len(stream)
    pos = 0

    def bits(n):
        nonlocal pos
        if pos + n > nbits_total:
            raise StreamError("stream cut short")
        v = (int.from_bytes(data[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << n) - 1)
        pos += n
        return v

    def sym(mx, t):
        nonlocal pos
        if not mx:
            raise StreamError("no code")
        e = t[(int.from_bytes(data[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << mx) - 1)]
        if e is None:
            raise StreamError("not a code")
        pos += e[1]
        if pos > nbits_total:
            raise StreamError("stream cut short")
        return e

    out = bytearray()
    st = dict(blocks=[], n_blocks=0, empty_blocks=[], max_lit_len=0, max_dist_len=0, min_dist_codes=None, single_dist_len1=False,
              dist_tree_zero=False, eob_only_1bit=False, cl_runs=set(), max_dist=0, far_4096=0, dist_32507=0, m258_32768=False,
              match_to_byte0=False, match_across_block=False, midbyte_block_start=False, max_syms_per_stretch=0, stored_sizes=[], dists=set(),
              m258_dists=set())
    while True:
        bstart, ostart = pos, len(out)
        if st["n_blocks"] and bstart % 8:
            st["midbyte_block_start"] = True
        final, btype = bits(1), bits(2)
        starts = []
        if btype == 0:
            pos = (pos + 7) & ~7
            n, nn = bits(16), bits(16)
            if n ^ 0xffff != nn:
                raise StreamError("stored length")
            if pos + 8 * n > nbits_total:
                raise StreamError("stream cut short")
            out += data[pos >> 3:(pos >> 3) + n]; pos += 8 * n
            st["stored_sizes"].append(n)
        elif btype in (1, 2):
            if btype == 1:
                lit_lens, dist_lens = FIXED_LIT, FIXED_DIST
            else:
                nlit, ndist, ncode = bits(5) + 257, bits(5) + 1, bits(4) + 4
                if nlit > 286 or ndist > 30:
                    raise StreamError("counts")
                cll = [0] * 19
                for k in range(ncode):
                    cll[CLORD[k]] = bits(3)
                cmx, ct = _table(cll)
                seq = []
                while len(seq) < nlit + ndist:
                    s, _ = sym(cmx, ct)
                    if s < 16:
                        seq.append(s)
                    else:
                        st["cl_runs"].add(s)
                        if s == 16:
                            if not seq:
                                raise StreamError("repeat with nothing before")
                            seq += [seq[-1]] * (3 + bits(2))
                        else:
                            seq += [0] * ((3 + bits(3)) if s == 17 else (11 + bits(7)))
                if len(seq) > nlit + ndist:
                    raise StreamError("code lengths overrun")
                lit_lens, dist_lens = seq[:nlit], seq[nlit:]
                if not lit_lens[256]:
                    raise StreamError("no end-of-block code")
                nd = sum(1 for l in dist_lens if l)
                st["min_dist_codes"] = nd if st["min_dist_codes"] is None else min(st["min_dist_codes"], nd)
                if nd == 1 and max(dist_lens) == 1:
                    st["single_dist_len1"] = True
                if ndist == 1 and dist_lens[0] == 0:
                    st["dist_tree_zero"] = True
                if sum(1 for l in lit_lens if l) == 1 and lit_lens[256] == 1:
                    st["eob_only_1bit"] = True
            lmx, lt = _table(lit_lens)
            dmx, dt = _table(dist_lens)
            while True:
                starts.append(pos)
                s, l = sym(lmx, lt)
                st["max_lit_len"] = max(st["max_lit_len"], l)
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                elif s > 285:
                    raise StreamError("length symbol")
                else:
                    n = LBASE[s - 257] + bits(LEXT[s - 257])
                    ds, dl = sym(dmx, dt)
                    if ds > 29:
                        raise StreamError("distance symbol")
                    st["max_dist_len"] = max(st["max_dist_len"], dl)
                    d = DBASE[ds] + bits(DEXT[ds])
                    if d > len(out):
                        raise StreamError("distance too far back")
                    st["max_dist"] = max(st["max_dist"], d)
                    st["far_4096"] += d > 4096
                    st["dist_32507"] += d >= 32507
                    st["m258_32768"] |= n == 258 and d == 32768
                    st["dists"].add(d)
                    if n == 258:
                        st["m258_dists"].add(d)
                    st["match_to_byte0"] |= d == len(out)
                    st["match_across_block"] |= len(out) - d < ostart
                    if d >= n:
                        out += out[len(out) - d:len(out) - d + n]
                    else:
                        for _ in range(n):
                            out.append(out[-d])
                if len(out) > out_limit:
                    raise StreamError("output overrun")
            j = 0                                          # the most symbols (end of block included) starting inside any 608 bits
            for i, p in enumerate(starts):
                while starts[j] + STRETCH_BITS <= p:
                    j += 1
                st["max_syms_per_stretch"] = max(st["max_syms_per_stretch"], i - j + 1)
        else:
            raise StreamError("block type 3")
        st["blocks"].append((btype, bstart, pos, len(out) - ostart))
        if len(out) == ostart:
            st["empty_blocks"].append(btype)
        st["n_blocks"] += 1
        if final:
            break
    st["bytes"] = bytes(out)
    st["end_bit"] = pos
    st["types"] = {b[0] for b in st["blocks"]}
    return st


# ---- contents (tools/inflate_emu.cpp selftest()'s kinds, and more) ----
def content(kind, n, rnd):
    if kind == "random":                  # incompressible: stored blocks
        return rnd.randbytes(n)
    if kind == "A":                       # distance-1 runs of 258; 1-bit codes under Huffman-only
        return b"A" * n
    if kind == "acgt":
        return bytes(rnd.choice(b"ACGT") for _ in range(n))
    if kind == "maxdist":                 # matches at the longest distance zlib emits
        r = bytearray(rnd.randbytes(min(n, 40000)))
        for i in range(len(r), n):
            r.append(r[i - 32768] if i >= 32768 else 0)
        return bytes(r)
    if kind == "mid":                     # many symbols: long codes, mid-range matches
        r = bytearray()
        for i in range(n):
            r.append(rnd.randrange(200) if (i % 600) < 300 or i < 300 else r[i - 300])
        return bytes(r)
    if kind == "ramp":
        return bytes((i // 3) % 251 for i in range(n))
    if kind == "x":
        return bytes(ord("x") if rnd.randrange(3) else rnd.randrange(256) for _ in range(n))
    if kind == "mix":
        return bytes(rnd.randrange(256) if i % 7 == 0 else i & 255 for i in range(n))
    if kind == "u128":                    # an exact 7-bit code: wrong-phase chains never synchronise, batches cut by the pass cap
        return bytes(b & 127 for b in rnd.randbytes(n))
    if kind == "u240":                    # slow synchronisation: 3 to 6 passes
        return bytes(rnd.choices(range(240), k=n))
    if kind == "skew":                    # geometric symbol frequencies: literal codes of 11-15 bits
        r = bytearray()
        p = 0.5
        for s in range(256):
            r += bytes([s]) * (int(n * p) + 1)
            if s < 14:
                p /= 2
        r = r[:n] if len(r) >= n else r + bytes(n - len(r))
        r = bytearray(r); rnd.shuffle(r)
        return bytes(r)
    if kind == "zero":
        return bytes(n)
    if kind == "ff":
        return b"\xff" * n
    raise ValueError(kind)


KINDS = ["random", "A", "acgt", "maxdist", "mid", "ramp", "x", "mix", "u128", "u240", "skew"]
# (level, strategy, wbits, memLevel)
ENCODERS = [(0, zlib.Z_DEFAULT_STRATEGY, -15, 8), (1, zlib.Z_DEFAULT_STRATEGY, -15, 8), (4, zlib.Z_FILTERED, -15, 8), (6, zlib.Z_DEFAULT_STRATEGY, -15, 8),
            (9, zlib.Z_DEFAULT_STRATEGY, -15, 9), (6, zlib.Z_HUFFMAN_ONLY, -15, 8), (6, zlib.Z_RLE, -15, 8), (6, zlib.Z_FIXED, -15, 8),
            (9, zlib.Z_DEFAULT_STRATEGY, -9, 8), (9, zlib.Z_DEFAULT_STRATEGY, -15, 1), (1, zlib.Z_FILTERED, -9, 1), (4, zlib.Z_RLE, -15, 9)]
STRAT = {zlib.Z_DEFAULT_STRATEGY: "def", zlib.Z_FILTERED: "filt", zlib.Z_HUFFMAN_ONLY: "huff", zlib.Z_RLE: "rle", zlib.Z_FIXED: "fixed"}


def zraw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=-15, memlevel=8, flushes=(), zdict=None):
    """raw deflate by zlib; flushes: [(offset, mode)] -- the input up to `offset` is flushed with `mode` inside the member"""
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, memlevel, strategy, **({"zdict": zdict} if zdict is not None else {}))
    out, prev = bytearray(), 0
    for off, mode in flushes:
        out += c.compress(data[prev:off]) + c.flush(mode); prev = off
    return bytes(out + c.compress(data[prev:]) + c.flush())


_LD = []


def libdeflate():
    """libdeflate's compressor through ctypes, or None (then its members are left out)"""
    if not _LD:
        try:
            L = ctypes.CDLL("libdeflate.so.0")
            L.libdeflate_alloc_compressor.restype = ctypes.c_void_p; L.libdeflate_alloc_compressor.argtypes = [ctypes.c_int]
            L.libdeflate_deflate_compress.restype = ctypes.c_size_t
            L.libdeflate_deflate_compress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
            L.libdeflate_free_compressor.argtypes = [ctypes.c_void_p]; L.libdeflate_free_compressor.restype = None
            _LD.append(L)
        except (OSError, AttributeError):
            _LD.append(None)
    return _LD[0]


def ldraw(data, level):
    L = libdeflate()
    c = L.libdeflate_alloc_compressor(level)
    assert c, level
    cap = len(data) + len(data) // 8 + 1024
    buf = ctypes.create_string_buffer(cap)
    n = L.libdeflate_deflate_compress(c, data, len(data), buf, cap)
    L.libdeflate_free_compressor(c)
    assert n > 0
    return buf.raw[:n]


def bam_records(rnd, n_bytes):
    """BAM records (tests/bamwriter.py) of about n_bytes, as a list of byte strings"""
    from bamwriter import record
    recs, tot, pos = [], 0, 1000
    ref = "".join(rnd.choice("ACGT") for _ in range(5000))
    while tot < n_bytes:
        pos += rnd.randrange(0, 40); o = rnd.randrange(0, 4000); l = rnd.choice((76, 100, 150))
        seq = ref[o:o + l].replace("C", "T") if rnd.randrange(2) else ref[o:o + l]
        r = record(0, pos, rnd.choice((0, 16, 99, 147)), f"{l}M", seq, [rnd.randrange(2, 41) for _ in range(l)], qname=f"read{rnd.randrange(10 ** 6)}")
        recs.append(r); tot += len(r)
    return recs


def writer_members(rnd):
    """what only BlockWriter writes: each one is checked against zlib by build_zoo"""
    out = []

    def add(name, w, raw):
        out.append(Member("writer_" + name, bytes(raw), w.getvalue()))

    lit = [rnd.randrange(128) for _ in range(32768)]
    # distances 32507..32768: 32768 literals in a fixed block, then matches in a dynamic block whose distance tree is ONE code of length 1
    # (symbol 29: 24577..32768); the first match (258 at distance 32768) reaches exactly to byte 0
    far = [(258, 32768), (3, 32768), (200, 32507), (258, 32600), (4, 32767), (100, 32750)] + [(rnd.randrange(3, 259), rnd.randrange(32507, 32769)) for _ in range(60)]
    w = BlockWriter(); w.fixed(lit); dl = [0] * 29 + [1]
    w.dynamic(far, final=True, dist_lens=dl, lit_lens=huffman_lengths([1 if i < 256 or i == 256 or 257 <= i <= 285 else 0 for i in range(286)], 15))
    add("dist32768_single_code", w, apply_tokens(lit + far))
    # the same distances from fixed blocks, with literals in between (far gather of scattered sources)
    toks = lit[:32769] + [t for k in range(40) for t in ((rnd.randrange(3, 259), rnd.randrange(32507, 32769)), rnd.randrange(256))]
    w = BlockWriter(); w.fixed(toks[:20000]); w.fixed(toks[20000:], final=True)
    add("dist32507_fixed", w, apply_tokens(toks))
    # a distance tree with a single code of length 1 (symbol 0: distance 1)
    t1 = [65, 66] + [(258, 1)] * 40 + [67] + [(17, 1)] * 5
    w = BlockWriter(); w.dynamic(t1, final=True, dist_lens=[1])
    add("single_dist_code_d1", w, apply_tokens(t1))
    # a literal-only block whose distance tree is one zero length; then an empty dynamic block whose only literal/length code is the end
    # of block, one bit; then a stored block
    t2 = [rnd.randrange(256) for _ in range(3000)]
    w = BlockWriter(); w.dynamic(t2, dist_lens=[0]); w.dynamic([], lit_lens=[0] * 256 + [1], dist_lens=[0]); w.dynamic([], lit_lens=[0] * 256 + [1], dist_lens=[1])
    w.stored(b"tail", final=True)
    add("literal_only_and_eob_only", w, bytes(t2) + b"tail")
    # literal codes of exactly 15 bits and distance codes longer than the table's 8 bits: both alphabets a chain of lengths 1, 2, .., 14, 15, 15
    chain = [97, 98, 99, 100, 101, 102, 103, 104, 105, 106, 257, 258, 284, 285, 65, 256]      # 'A' and the end of block get the two 15-bit codes
    ll = [0] * 286
    for i, s in enumerate(chain):
        ll[s] = min(i + 1, 15)
    dchain = list(range(0, 30, 2)) + [29]
    dls = [0] * 30
    for i, s in enumerate(dchain):
        dls[s] = min(i + 1, 15)
    t3 = [97 + rnd.randrange(10) for _ in range(600)] + [(258, 600)] * 127 + [65] * 8
    for k in range(150):
        ds = dchain[k % 16]; d = DBASE[ds] + (rnd.randrange(1 << DEXT[ds]) if DEXT[ds] else 0)
        t3 += [(rnd.choice((3, 4, 227, 230, 258)), d), 97 + rnd.randrange(10), 65]
    w = BlockWriter(); w.dynamic(t3, final=True, lit_lens=ll, dist_lens=dls, runs=True)
    add("codes15_both_tables", w, apply_tokens(t3))
    # a header with all three run-length codes: 16 (the 7-bit literals' equal lengths), 18 (the unused literals), 17 (the distance tree's zeros in
    # front of its one code); the stored block in front is a match's source across two block boundaries
    body = rnd.randbytes(700)
    t5 = [rnd.randrange(128) for _ in range(4000)] + [(8, 7), (7, 8), (258, 9)]
    w = BlockWriter(); w.stored(body); w.dynamic(t5, runs=True, dist_lens=[0, 0, 0, 0, 0, 1, 1]); w.fixed([(258, 4966)], final=True)
    add("header_runs_16_17_18", w, apply_tokens(t5 + [(258, 4966)], bytearray(body)))
    # stored blocks of 0, 1, 511, 512, 513 bytes in one member; 65535 bytes in a member of its own (too long for a BGZF frame)
    w = BlockWriter(); parts = b""
    for n in (0, 1, 511, 512, 513):
        d = rnd.randbytes(n); w.stored(d); parts += d
    w.stored(b"", final=True)
    add("stored_0_1_511_512_513", w, parts)
    d = rnd.randbytes(65535); w = BlockWriter(); w.stored(d, final=True)
    add("stored_65535", w, d)
    d = rnd.randbytes(65535) + b"!"; w = BlockWriter(); w.stored(d[:65535]); w.fixed([33], final=True)
    add("stored_65535_plus_fixed", w, d)
    return out


def build_zoo(seed=20261016, with_libdeflate=True):
    """[Member]: every stream legal and equal under zlib to its bytes (asserted here)"""
    rnd = random.Random(seed)
    zoo = []

    def add(name, raw, stream):
        zoo.append(Member(name, bytes(raw), bytes(stream)))

    # sizes x contents, the encoders in rotation (every encoder meets every size)
    for si, n in enumerate(SIZES):
        for ki, kind in enumerate(KINDS):
            lv, stg, wb, ml = ENCODERS[(si + 5 * ki) % len(ENCODERS)]
            d = content(kind, n, rnd)
            add(f"{kind}_{n}_l{lv}_{STRAT[stg]}_w{-wb}_m{ml}", d, zraw(d, lv, stg, wb, ml))
    # the named regimes
    for stg in (zlib.Z_HUFFMAN_ONLY, zlib.Z_FIXED, zlib.Z_DEFAULT_STRATEGY):
        for kind in ("u128", "u240"):
            d = content(kind, 65280, rnd); add(f"{kind}_65280_{STRAT[stg]}", d, zraw(d, 6, stg))
    d = b"A" * 65536; add("A_65536_huff", d, zraw(d, 6, zlib.Z_HUFFMAN_ONLY))
    for unit in (b"A", b"AB", b"ABC"):              # distance-1/2/3 runs of length 258
        d = unit * (60000 // len(unit)); add(f"run_d{len(unit)}", d, zraw(d, 9))
    for dist in (2040, 2047, 2048, 2049, 2056, 4090, 4095, 4096, 4097, 4102, 31990, 32000):
        r = bytes(b & 127 for b in rnd.randbytes(dist)); d = (r + r + r)[:65280]
        add(f"dist_{dist}", d, zraw(d, 9))
    d = content("skew", 65536, rnd)
    for lv in (1, 6, 9):
        add(f"skew_l{lv}_huff", d, zraw(d, lv, zlib.Z_HUFFMAN_ONLY)); add(f"skew_l{lv}_def", d, zraw(d, lv))
    # flushes inside a member
    d = content("mid", 60000, rnd)
    add("sync_flush", d, zraw(d, 6, flushes=[(10000, zlib.Z_SYNC_FLUSH), (10000, zlib.Z_SYNC_FLUSH), (30000, zlib.Z_SYNC_FLUSH)]))
    add("full_flush", d, zraw(d, 6, flushes=[(20000, zlib.Z_FULL_FLUSH), (45000, zlib.Z_FULL_FLUSH)]))
    add("partial_flush", d, zraw(d, 6, flushes=[(777, zlib.Z_PARTIAL_FLUSH), (15000, zlib.Z_PARTIAL_FLUSH), (15001, zlib.Z_PARTIAL_FLUSH)]))
    add("block_flush", d, zraw(d, 6, flushes=[(1234, zlib.Z_BLOCK), (20001, zlib.Z_BLOCK), (40003, zlib.Z_BLOCK)]))
    r = bytes(b & 63 for b in rnd.randbytes(3000)); d = r + r      # the second copy matches across the sync-flushed boundary
    add("match_across_sync_flush", d, zraw(d, 9, flushes=[(3000, zlib.Z_SYNC_FLUSH)]))
    d = content("acgt", 65280, rnd)
    add("many_blocks_memlevel1", d, zraw(d, 9, memlevel=1)); add("memlevel9_w9", d, zraw(d, 9, wbits=-9, memlevel=9))
    # BAM record payloads cut on record boundaries
    recs = bam_records(rnd, 400000)
    blk, n_bam = bytearray(), 0
    for r in recs:
        if len(blk) + len(r) > 65280:
            n_bam += 1
            lv, stg = (6, 1, 9, 4)[n_bam % 4], (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED)[n_bam % 2]
            add(f"bam_{n_bam}_l{lv}_{STRAT[stg]}", blk, zraw(bytes(blk), lv, stg))
            blk = bytearray()
        blk += r
    # libdeflate
    if with_libdeflate and libdeflate():
        for lv in (1, 6, 9, 12):
            for kind in ("acgt", "mid", "maxdist", "u240", "skew"):
                d = content(kind, 65280, rnd); add(f"libdeflate{lv}_{kind}", d, ldraw(d, lv))
            add(f"libdeflate{lv}_bam", bytes(blk), ldraw(bytes(blk), lv))
            add(f"libdeflate{lv}_1", b"q", ldraw(b"q", lv))
    zoo += writer_members(rnd)
    for m in zoo:
        assert zlib.decompress(m.stream, -15) == m.raw, m.name
        assert len(m.raw) <= 65536, m.name
    return zoo


# the good members around every malformed one in the tests of refusal: a far-match member, stored blocks of several sizes, a Huffman-only
# member whose batches are cut by the pass cap, a sync-flushed member, distance-3 runs, BAM records
AROUND_MALFORMED = ("writer_dist32768_single_code", "writer_stored_0_1_511_512_513", "u128_65280_huff", "sync_flush", "run_d3", "bam_1_l1_filt")


def around_malformed(zoo):
    by = {m.name: m for m in zoo}
    return [by[n] for n in AROUND_MALFORMED]


def malformed(seed=7):
    """[(name, stream, out_len)]: streams (or ISIZEs) the kernel must refuse -- zlib does not inflate any of them to out_len bytes"""
    rnd = random.Random(seed)
    d = content("mid", 20000, rnd)
    s = zraw(d, 6)
    out = [("isize_plus_1", s, len(d) + 1), ("isize_minus_1", s, len(d) - 1)]
    st = zraw(d[:3000], 0)
    out += [("stored_isize_plus_1", st, 3001), ("stored_isize_minus_1", st, 2999)]
    for k in (1, 2, 3, 4):
        out.append((f"cut_{k}", s[:-k], len(d)))
    out.append(("stored_cut_2", st[:-2], 3000))
    w = BlockWriter(); w.fixed(list(b"abc") + [(3, 4)] + list(b"xyz"), final=True)            # distance 4 with 3 bytes made
    out.append(("dist_one_too_far", w.getvalue(), 9))
    w = BlockWriter(); w.fixed(list(rnd.randbytes(5000)) + [(258, 5001)], final=True)
    out.append(("dist_5001_at_5000", w.getvalue(), 5258))
    zd = content("mid", 4000, rnd)
    zs = zraw(zd[2000:], 6, zdict=zd[:2000])                                                     # matches into a preset dictionary
    out.append(("zdict", zs, 2000))
    for name, stream, n in out:
        try:
            ok = len(zlib.decompress(stream, -15)) == n
        except zlib.error:
            ok = False
        assert not ok, name
    return out


# ---- containers ----
def bgzf_member(stream, raw_len, crc):
    assert len(stream) <= BGZF_MAX_STREAM
    return struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(stream) + 25) + stream + struct.pack("<II", crc, raw_len)


BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_file(items):
    """items: [(stream, out_len, crc)] -> one BGZF file (those too long for a frame must be left out by the caller)"""
    return b"".join(bgzf_member(s, n, c) for s, n, c in items) + BGZF_EOF


def piece_layout(items, seed=1):
    """items: [(stream, out_len, crc)] -> (comp, [(in_off, in_len, out_len, out_off, crc)]) for md_piece_submit: junk bytes between the
    streams so that in_off % 4 takes every value; the last stream ends the buffer, at a length that is not a multiple of 4"""
    rnd = random.Random(seed)
    comp, tab, out_off = bytearray(), [], 0
    for i, (s, n, c) in enumerate(items):
        want = i % 4
        if i == len(items) - 1:                     # the end of the last one must not fall on a word boundary
            want = next(a for a in (want, (want + 1) % 4, (want + 2) % 4) if (a + len(s)) % 4)
        gap = (want - len(comp)) % 4 + 4 * rnd.randrange(3)
        comp += rnd.randbytes(gap)
        tab.append((len(comp), len(s), n, out_off, c))
        comp += s; out_off += n
    return bytes(comp), tab


def bgzf_members(raw):
    """[(stream offset, stream length, ISIZE, CRC32)] of a BGZF file"""
    out, o = [], 0
    while o + 18 <= len(raw):
        xlen = struct.unpack_from("<H", raw, o + 10)[0]
        bs = struct.unpack_from("<H", raw, o + 16)[0] + 1
        crc, isz = struct.unpack_from("<II", raw, o + bs - 8)
        out.append((o + 12 + xlen, bs - 12 - xlen - 8, isz, crc))
        o += bs
    return out


def bam_split(raw):
    """a BGZF-compressed BAM -> (header bytes, [record bytes])"""
    data = b"".join(zlib.decompress(raw[io:io + il], -15) for io, il, isz, _ in bgzf_members(raw) if isz)
    l_text = struct.unpack_from("<i", data, 4)[0]
    o = 8 + l_text
    n_ref = struct.unpack_from("<i", data, o)[0]; o += 4
    for _ in range(n_ref):
        o += 4 + struct.unpack_from("<i", data, o)[0] + 4
    hdr, recs = data[:o], []
    while o < len(data):
        n = 4 + struct.unpack_from("<i", data, o)[0]
        recs.append(data[o:o + n]); o += n
    return hdr, recs


def bam_reencode(hdr, recs, enc, limit=65280, sync=False, threads=8):
    """The BAM again as htslib frames it -- the header in a member of its own, records never across members, at most `limit` bytes a
    member -- with `enc(bytes) -> raw deflate` (sync: zlib level 6 with a Z_SYNC_FLUSH behind every record).  The members are compressed
    on a few threads (zlib and ctypes calls let go of the interpreter lock)."""
    from concurrent.futures import ThreadPoolExecutor
    groups, blk, n = [[hdr]], [], 0
    for r in recs:
        if n + len(r) > limit and blk:
            groups.append(blk); blk, n = [], 0
        blk.append(r); n += len(r)
    if blk:
        groups.append(blk)

    def one(g):
        data = b"".join(g)
        if sync:
            c = zlib.compressobj(6, zlib.DEFLATED, -15)
            s = b"".join(c.compress(r) + c.flush(zlib.Z_SYNC_FLUSH) for r in g) + c.flush()
        else:
            s = enc(data)
        return bgzf_member(s, len(data), zlib.crc32(data))
    with ThreadPoolExecutor(threads) as ex:
        return b"".join(ex.map(one, groups)) + BGZF_EOF
