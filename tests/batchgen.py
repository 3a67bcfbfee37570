"""TEST INFRASTRUCTURE: hand-built device batches (include/mdk_hip.h md_read_batch) and the named cases that aim each at one
mechanism of the pileup and mbias kernels (csrc/mdk_hip.hip).

A case is a function without arguments that returns ``(reference bytes, cfg fields, regions or None, batch, reaches)``:
  * cfg fields: ``minPhred``, ``bounds``, ``absoluteBounds`` (what a case may set of md_dev_cfg), and optionally ``keeps`` -- keep masks
    the case runs under besides the kernels' own -- and ``mod`` -- the only minOppositeDepth values the case is meant for;
  * ``reaches(batch, tile, result)``: the case hits the edge it is named for, at that tile size, given the evaluator's result
    (tests/batch_eval.py eval_batch under keep (1, 1, 1) and minOppositeDepth 1, or eval_mbias).
Batches do not depend on the tile size: tile edges are aimed at through multiples of 512 from ``beg``, which are edges of every
geometry the library has (512, 1024, 1536, 2048).  Everything is seeded; nothing here is imported by the product."""
import ctypes as C
import random

import numpy as np

import methyldackel_amd as mdk
from bamwriter import NT16
from batch_eval import eval_batch, eval_mbias

TILES = (512, 1024, 1536, 2048)
ERR_STRAND0 = -5
SEG_DT = np.dtype([("rpos", "<i4"), ("off4", "<u4"), ("l_qseq", "<u4"), ("q0", "<u4"), ("len", "<u2"), ("sf", "u1"), ("msf", "u1"),
                   ("m_off4", "<u4"), ("m_l_qseq", "<u4"), ("m_q0", "<u4")])
assert SEG_DT.itemsize == C.sizeof(mdk.md_seg) == 32
BUDGET = 300000          # evaluated segment bases per case


class Builder:
    """reads and segments of one batch"""

    def __init__(self):
        self.blob = bytearray()
        self.reads = []          # (off4, l_qseq)
        self.segs = []

    def read(self, seq, qual):
        """seq: a string over the BAM base letters (any case) or a list of 4-bit codes; qual: one value or one per base -> read index"""
        codes = [NT16[c.upper()] for c in seq] if isinstance(seq, str) else list(seq)
        lq = len(codes)
        qual = [qual] * lq if isinstance(qual, int) else list(qual)
        assert len(qual) == lq and len(self.blob) % 4 == 0
        nib = bytearray((((lq + 1) // 2) + 3) & ~3)
        for i, c in enumerate(codes):
            nib[i >> 1] |= (c & 15) << (0 if i & 1 else 4)
        self.reads.append((len(self.blob) // 4, lq))
        self.blob += nib + bytes(qual) + bytes(-lq & 3)
        return len(self.reads) - 1

    def seg(self, rpos, read, q0, len, strand, read2, second, partner=None, m_q0=0, m_strand=0, m_read2=0):
        off4, lq = self.reads[read]
        assert len >= 1 and q0 + len <= lq and len <= 65535
        sf = (strand & 7) | (8 if read2 else 0) | (16 if second else 0)
        m_off4 = m_lq = msf = 0
        if partner is not None:
            m_off4, m_lq = self.reads[partner]
            assert m_q0 + len <= m_lq
            sf |= 32
            msf = (m_strand & 7) | (8 if m_read2 else 0)
        else:
            m_q0 = 0
        self.segs.append((rpos, off4, lq, q0, len, sf, msf, m_off4, m_lq, m_q0))

    def batch(self, tid, beg, end):
        """-> md_read_batch; the arrays it points to live as long as the batch object"""
        segs = np.array(self.segs, dtype=SEG_DT) if self.segs else np.zeros(1, dtype=SEG_DT)
        blob = (C.c_uint8 * max(len(self.blob), 4)).from_buffer_copy(bytes(self.blob) + bytes(max(0, 4 - len(self.blob))))
        b = mdk.md_read_batch()
        b.tid, b.beg, b.end, b.n_segs = tid, beg, end, len(self.segs)
        b.seg = segs.ctypes.data_as(C.POINTER(mdk.md_seg))
        b.blob = C.cast(blob, C.POINTER(C.c_uint8))
        b.blob_bytes = len(self.blob)
        b.n_reads = len(self.reads)
        b.algo_bytes = sum(16 + 4 + (lq + 1) // 2 + lq for _, lq in self.reads)
        b._keep = (segs, blob)
        return b


def seg_array(batch):
    """the batch's segments as a numpy record array (a view)"""
    return batch._keep[0][:batch.n_segs]


def seg_payload(batch, s):
    """(base letters, qualities) of the bases a segment covers, untrimmed"""
    base = C.addressof(batch.blob.contents) + 4 * int(s["off4"])
    lq, q0, n = int(s["l_qseq"]), int(s["q0"]), int(s["len"])
    seq = bytes((C.c_uint8 * ((lq + 1) // 2)).from_address(base))
    qual = bytes((C.c_uint8 * lq).from_address(base + ((((lq + 1) // 2) + 3) & ~3)))
    letters = "=ACMGRSVTWYHKDBN"
    return "".join(letters[(seq[q >> 1] >> (0 if q & 1 else 4)) & 15] for q in range(q0, q0 + n)), list(qual[q0:q0 + n])


def evaluated_bases(batch):
    return int(seg_array(batch)["len"].astype(np.int64).sum())


def make_cfg(fields, keep, mod, tile, n_slots=2):
    cfg = mdk.md_dev_cfg()
    cfg.keepCpG, cfg.keepCHG, cfg.keepCHH = keep
    cfg.minPhred = fields.get("minPhred", 5)
    cfg.minOppositeDepth = mod
    for i in range(16):
        cfg.bounds[i] = fields.get("bounds", (0,) * 16)[i]
        cfg.absoluteBounds[i] = fields.get("absoluteBounds", (0,) * 16)[i]
    cfg.tile, cfg.n_slots = tile, n_slots
    return cfg


def expected_sites(ref, fields, regions, batch, keep, mod):
    """eval_batch, or MDK_ERR_STRAND0 where the evaluator meets the reference's abort (common.c:122-125)"""
    try:
        return eval_batch(batch, ref, make_cfg(fields, keep, mod, 0), regions)
    except AssertionError as e:
        if "strand 0" not in str(e):
            raise
        return ERR_STRAND0


def expected_hist(ref, fields, batch, keep):
    try:
        return {k: tuple(v) for k, v in eval_mbias(batch, ref, make_cfg(fields, keep, 0, 0)).items()}
    except AssertionError:
        return ERR_STRAND0


def device_sites(dev, slot, batch):
    """submit + download -> {pos: (type, isG, nmeth, nunmeth, noff, nvar)}, the shape eval_batch returns, or the error code"""
    rc = dev.L.md_dev_submit(dev.h, slot, C.byref(batch))
    if rc:
        return rc
    s = mdk.md_sites()
    rc = dev.L.md_dev_download(dev.h, slot, C.byref(s))
    if rc:
        return rc
    return sites_dict(s, batch.beg, batch.end)


def sites_dict(s, beg, end):
    """md_sites as a dictionary, once the sites are seen to be ascending, inside [beg, end) and not duplicated"""
    rows = mdk.sites_to_rows(s)
    order = [r[0] for r in rows]
    assert all(a < b for a, b in zip(order, order[1:])), "sites not strictly ascending"
    assert all(beg <= p < end for p in order), "site outside [beg, end)"
    return {r[0]: tuple(r[1:]) for r in rows}


def device_hist(dev):
    """mbias_read -> {(strand, read number, q): (meth, unmeth)} for the non-zero entries, or the error code"""
    m = mdk.md_mbias()
    rc = dev.L.md_dev_mbias_read(dev.h, C.byref(m))
    if rc:
        return rc
    out = {}
    if m.len > 0:
        a = np.ctypeslib.as_array(m.count, shape=(m.len * 16,)).reshape(m.len, 4, 2, 2)
        for q, s, r in zip(*np.nonzero(a.sum(axis=3))):
            out[(int(s) + 1, int(r) + 1, int(q))] = (int(a[q, s, r, 0]), int(a[q, s, r, 1]))
    return out


def first_difference(got, want):
    if not isinstance(got, dict) or not isinstance(want, dict):
        return f"device {got if not isinstance(got, dict) else 'sites'} evaluator {want if not isinstance(want, dict) else 'sites'}"
    for p in sorted(set(got) | set(want)):
        if got.get(p) != want.get(p):
            return f"first difference at {p}: device {got.get(p)} evaluator {want.get(p)}"
    return "equal"


# ---- geometry helpers for the `reaches` predicates ----
def tiles_of(batch, tile):
    return [(t0, min(t0 + tile, batch.end)) for t0 in range(batch.beg, batch.end, tile)]


def tile_runs(batch, tile):
    """(first, last) of every tile's run of the segment array, as build_tiles makes it: the run may hold segments that are not on the tile"""
    S = seg_array(batch)
    lo = np.maximum(S["rpos"].astype(np.int64), batch.beg)
    hi = np.minimum(S["rpos"].astype(np.int64) + S["len"], batch.end)
    out = []
    for t0, t1 in tiles_of(batch, tile):
        on = np.nonzero((lo < t1) & (hi > t0) & (hi > lo))[0]
        out.append((int(on[0]), int(on[-1]) + 1, len(on)) if len(on) else (0, 0, 0))
    return out


def list_counts(ref, batch, tile):
    """(nC, nG) of every tile under keep (1, 1, 1)"""
    up = bytes(ref).upper()
    return [(up.count(b"C", t0, min(t1, len(up))), up.count(b"G", t0, min(t1, len(up)))) for t0, t1 in tiles_of(batch, tile)]


def is_pow2(n):
    return n > 0 and n & (n - 1) == 0


STRAND_READS = [(s, r2) for s in (1, 2, 3, 4) for r2 in (0, 1)]


def rand_read(B, rng, lq, like=None, at=0):
    """a read of lq bases: random, or (like = reference bytes) mostly equal to the reference from `at` with conversions and errors"""
    if like is None:
        seq = [rng.choice((1, 2, 4, 8, 15, 2, 4, 8, 1)) for _ in range(lq)]
    else:
        seq = []
        for i in range(lq):
            p = at + i
            c = NT16.get(chr(like[p]).upper(), 15) if 0 <= p < len(like) else 15
            x = rng.random()
            if x < 0.3 and c == 2:
                c = 8
            elif x < 0.3 and c == 4:
                c = 1
            elif x > 0.93:
                c = rng.choice((1, 2, 4, 8, 15))
            seq.append(c)
    return B.read(seq, [rng.choice((0, 2, 4, 5, 6, 19, 20, 21, 30, 40, 41)) for _ in range(lq)])


def sprinkle(B, rng, ref, n, lq_lo=30, lq_hi=150, lo=0, hi=None, partner_frac=0.0, strands=(1, 2, 3, 4)):
    """n random reads over [lo, hi) of every strand and read number; a read gives one whole-read segment, two segments around a gap, or
    (partner_frac) a pair of overlapping mates with every partner field random inside the contract"""
    hi = len(ref) if hi is None else hi
    for _ in range(n):
        lq = rng.randint(lq_lo, lq_hi)
        pos = rng.randint(max(0, lo - lq // 2), hi - 1)          # rpos >= 0: the header's contract
        strand, r2 = rng.choice(strands), rng.random() < 0.5
        a = rand_read(B, rng, lq, ref, pos)
        if rng.random() < partner_frac:
            mlq = rng.randint(lq_lo, lq_hi)
            shift = rng.randint(-mlq + 1, lq - 1)          # the mate starts `shift` bases after this read
            b = rand_read(B, rng, mlq, ref, pos + shift)
            o0, o1 = max(0, shift), min(lq, shift + mlq)    # overlap in this read's query coordinates
            mstrand, mr2 = rng.choice(strands), rng.random() < 0.5
            if o0 > 0:
                B.seg(pos, a, 0, o0, strand, r2, 0)
            B.seg(pos + o0, a, o0, o1 - o0, strand, r2, 0, partner=b, m_q0=o0 - shift, m_strand=mstrand, m_read2=mr2)
            if o1 < lq:
                B.seg(pos + o1, a, o1, lq - o1, strand, r2, 0)
            B.seg(pos + o0, b, o0 - shift, o1 - o0, mstrand, mr2, 1, partner=a, m_q0=o0, m_strand=strand, m_read2=r2)
        elif lq > 20 and rng.random() < 0.3:
            k = rng.randint(1, lq - 10)
            B.seg(pos, a, 0, k, strand, r2, 0)
            B.seg(pos + k + rng.randint(0, 9), a, k + rng.randint(0, 3), lq - k - 3, strand, r2, 0)
        else:
            B.seg(pos, a, 0, lq, strand, r2, 0)


def rand_ref(rng, n, density, letters="ATat", cg="CGcg"):
    return bytes(ord(rng.choice(cg) if rng.random() < density else rng.choice(letters)) for _ in range(n))


def nonzero(result):
    return isinstance(result, dict) and len(result) > 0


# ---- context carpet: k_classify, load_codes and its keep mask ----
KEEPS4 = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1))
CARPET_TAILS = ("CG", "CAG", "CC")


def carpet_ref(length, variant):
    """mixed case, N and IUPAC letters; CG / CAG / CC (by variant, rotating) across 511|512 and 2047|2048 and as the contig's last bases"""
    rng = random.Random(1000 * length + variant)
    s = bytearray(ord(rng.choice("ACGTacgtACGTacgtNnRYKMSWrykm")) for _ in range(length))

    def plant(motif, at):
        m = motif if rng.random() < 0.5 else motif.lower()
        for i, ch in enumerate(m):
            if 0 <= at + i < length:
                s[at + i] = ord(ch)
    tail = CARPET_TAILS[(variant + 2) % 3][:length]
    plant(tail, length - len(tail))
    for k, edge in enumerate((512, 2048)):             # after the tail: where the two meet (513, 2051) the motif across the edge wins
        motif = CARPET_TAILS[(variant + k) % 3]
        if edge < length:
            plant(motif, edge - len(motif) + 1)        # its last base is the first of the next tile
    if length == 1:
        s[:] = (b"C", b"g", b"N")[variant]
    return bytes(s)


def carpet_batch(ref):
    B = Builder()
    for strand in (1, 2):
        for at in range(0, len(ref), 65535):
            part = ref[at:at + 65535]
            B.seg(at, B.read(part.decode(), 30), 0, len(part), strand, 0, 0)
    return B.batch(0, 0, len(ref))


def carpet_case(length, variant):
    def case():
        ref = carpet_ref(length, variant)
        up = ref.upper()

        def reaches(batch, tile, result):
            return isinstance(result, dict) and len(result) == up.count(b"C") + up.count(b"G") and all(v[2] == 1 for v in result.values())
        return ref, {"keeps": KEEPS4}, None, carpet_batch(ref), reaches
    return case


REGION_SETS = {
    "strands": [(3, 40, 0), (40, 90, 1), (90, 91, 2), (100, 300, 2), (505, 512, 1), (512, 530, 2), (2040, 2048, 0), (2049, 2051, 1)],
    "edges": [(0, 511, 1), (511, 512, 2), (512, 513, 0), (513, 2047, 2), (2047, 2048, 1), (2048, 2051, 0)],
    "one": [(2048, 2049, 0)],
    "none": [],
}


def region_case(name):
    def case():
        ref = carpet_ref(2051, 0)
        runs = REGION_SETS[name]
        B = Builder()
        whole = B.read(ref.decode(), 30)
        for strand in (1, 2, 3, 4):
            B.seg(0, whole, 0, len(ref), strand, 0, 0)
        # a read of unknown strand is invisible in '+' and '-' runs; over the Cs of an either-strand run it is opposite-strand evidence
        c_any = [p for p in range(len(ref)) if ref[p] in b"Cc" and any(a <= p < b and s == 0 for a, b, s in runs)]
        for p in c_any[:3]:
            B.seg(p, whole, p, 1, 0, 0, 0)
        for a, b, s in runs:
            if s:
                B.seg(a, whole, a, b - a, 0, 0, 0)

        def reaches(batch, tile, result):
            if not runs:
                return result == {}
            return nonzero(result) and all(any(a <= p < b for a, b, _ in runs) for p in result)
        return ref, {"keeps": KEEPS4}, runs, B.batch(0, 0, len(ref)), reaches
    return case


# ---- saturated and empty lists: build_lists, list_lower_bound, the w packing of seg_setup ----
N_LISTS = 2 * 2048 + 37
POW2_WINDOWS = (128, 127, 257, 0, 255, 256, 1, 1, 511, 512, 0, 0)      # Cs per 512 positions from beg: every tile size meets 2^k - 1, 2^k and 2^k + 1


def lists_case(kind):
    def case():
        rng = random.Random(sum(map(ord, kind)))
        n, beg = N_LISTS, 7
        if kind == "allC":
            ref = b"C" * n
        elif kind == "allG":
            ref = b"G" * n
        elif kind == "CG":
            ref = (b"CG" * n)[:n]
        elif kind == "oneC":
            ref = b"A" * 1500 + b"C" + b"A" * (n - 1501)
        else:
            s = bytearray()
            for w in POW2_WINDOWS:
                at = set(rng.sample(range(512), w))
                s += bytes(ord("C") if i in at else ord(rng.choice("AGTAT")) for i in range(512))
            ref = b"T" * beg + bytes(s) + b"ATTAT"
            n = len(ref)
        end = n - 5
        B = Builder()
        sprinkle(B, rng, ref, 300, 60, 150)
        batch = B.batch(0, beg, end)

        def reaches(batch, tile, result):
            cnt = list_counts(ref, batch, tile)
            nC = [c for c, _ in cnt]
            short_last = (batch.end - batch.beg) % tile != 0
            if kind == "allC":
                return tile in nC and short_last and all(g == 0 for _, g in cnt) and nonzero(result)
            if kind == "allG":
                return all(c == 0 for c in nC) and tile in [g for _, g in cnt] and nonzero(result)
            if kind == "CG":
                return tile // 2 in nC and short_last and nonzero(result)
            if kind == "oneC":
                return sorted(set(nC)) == [0, 1] and 1500 in result
            return any(is_pow2(c) for c in nC) and any(is_pow2(c + 1) and c > 2 for c in nC) and any(is_pow2(c - 1) and c > 2 for c in nC) \
                and (tile != 512 or 512 in nC) and nonzero(result)
        return ref, {}, None, batch, reaches
    return case


# ---- tile edges: lane_seg and seg_setup, lo_off / hi_off ----
def edge_ref(n, seed):
    return rand_ref(random.Random(seed), n, 0.6)


def edges_points():
    """one-base segments at every T0 and T1 - 1 and at end - 1, two-base segments across every T1 - 1 | T1"""
    rng = random.Random(21)
    beg, end = 11, 11 + 3 * 2048 + 300
    ref = bytearray(edge_ref(end + 40, 22))
    for e in range(beg, end, 512):              # sites on both sides of every edge, of both kinds
        ref[e - 2:e + 2] = rng.choice((b"CGCG", b"GCCG", b"CCGG", b"cgGC"))
    ref[end - 2:end] = b"CG"
    ref = bytes(ref)
    B = Builder()
    whole = B.read(ref.decode(), 30)
    for e in list(range(beg, end, 512)) + [end]:
        for strand in (1, 2, 3, 4):
            if e < end:
                B.seg(e, whole, e, 1, strand, 0, 0)
            if e > beg:
                B.seg(e - 1, whole, e - 1, 1, strand, 1, 0)
                B.seg(e - 1, whole, e - 1, 2, strand, 0, 0)
    batch = B.batch(0, beg, end)

    def reaches(batch, tile, result):
        edges = [t0 for t0, _ in tiles_of(batch, tile)]
        return all(e in result and (e == batch.beg or e - 1 in result) for e in edges) and batch.end - 1 in result and batch.end not in result
    return ref, {}, None, batch, reaches


def edges_span():
    """a segment over three whole tiles and more, one from before beg to after end, and short ones hanging over beg and end"""
    beg, end = 700, 700 + 3 * 2048 + 2 * 512
    ref = edge_ref(end + 900, 23)
    B = Builder()
    whole = B.read(ref.decode(), 30)
    B.seg(beg - 650, whole, beg - 650, end - beg + 1300, 1, 0, 0)        # before beg to after end
    B.seg(beg, whole, beg, 3 * 2048, 2, 0, 0)                            # exactly three whole tiles of the largest geometry, more of the others
    B.seg(beg + 100, whole, beg + 100, 3 * 2048 + 700, 4, 1, 0)          # the same unaligned
    B.seg(beg - 20, whole, beg - 20, 40, 2, 0, 0)
    B.seg(end - 20, whole, end - 20, 40, 3, 0, 0)
    B.seg(beg - 50, whole, beg - 50, 50, 1, 0, 0)                        # ends at beg: not in the interval at all
    B.seg(end, whole, end, 50, 1, 0, 0)                                  # starts at end
    batch = B.batch(0, beg, end)

    def reaches(batch, tile, result):
        S = seg_array(batch)
        return nonzero(result) and min(result) < batch.beg + 40 and max(result) >= batch.end - 40 and \
            any(int(s["rpos"]) < batch.beg and int(s["rpos"]) + int(s["len"]) > batch.end for s in S) and \
            any(int(s["rpos"]) == batch.beg and int(s["len"]) >= 3 * tile and int(s["len"]) % tile == 0 for s in S)
    return ref, {}, None, batch, reaches


def edges_contig_end():
    """end == contig length; segments run past the contig's end, one starts at its last base"""
    n = 2048 + 512 + 77
    ref = edge_ref(n - 2, 24) + b"CG"
    B = Builder()
    long = B.read((ref + b"CGCGCGCGCGCGCGCGCGCGCGCGCGCGCGCGCGCGCGCG").decode(), 30)
    for strand in (1, 2, 3, 4):
        B.seg(n - 100, long, n - 100, 140, strand, 0, 0)
        B.seg(n - 1, long, n - 1, 30, strand, 1, 0)
        B.seg(n, long, n, 20, strand, 0, 0)                              # wholly past the end
    batch = B.batch(0, 5, n)

    def reaches(batch, tile, result):
        return batch.end == len(ref) and nonzero(result) and max(result) == len(ref) - 1 and len(ref) - 2 in result
    return ref, {}, None, batch, reaches


def edges_gap():
    """tiles that no segment touches between occupied ones (their run is empty), at every tile size"""
    beg, end = 3, 3 + 5 * 2048 + 100
    ref = edge_ref(end + 10, 25)
    B = Builder()
    rng = random.Random(26)
    sprinkle(B, rng, ref, 40, 30, 100, lo=beg + 50, hi=beg + 400)                     # only on the first 512 positions ...
    sprinkle(B, rng, ref, 40, 30, 100, lo=beg + 4 * 2048 + 50, hi=beg + 4 * 2048 + 400)   # ... and on the first of the fifth 2048
    batch = B.batch(0, beg, end)

    def reaches(batch, tile, result):
        n = [r[2] for r in tile_runs(batch, tile)]
        return any(n[i] == 0 and any(n[:i]) and any(n[i + 1:]) for i in range(len(n))) and nonzero(result)
    return ref, {}, None, batch, reaches


def edges_nosegs():
    ref = edge_ref(3000, 27)
    return ref, {}, None, Builder().batch(0, 10, 2900), lambda batch, tile, result: batch.n_segs == 0 and result == {}


def edges_empty():
    """beg == end: no tile at all, with and without segments around"""
    ref = edge_ref(3000, 28)
    B = Builder()
    sprinkle(B, random.Random(29), ref, 20, 30, 100, lo=900, hi=1100)
    return ref, {}, None, B.batch(0, 1000, 1000), lambda batch, tile, result: batch.beg == batch.end and batch.n_segs > 0 and result == {}


# ---- rounds and order: pileup_tile phase 2, build_tiles ----
def rounds_case(n_on_tile, shuffle):
    def case():
        rng = random.Random(n_on_tile * 2 + shuffle)
        beg, end = 20, 20 + 2 * 2048 + 90
        ref = edge_ref(end + 200, 30)
        B = Builder()
        reads = [rand_read(B, rng, 60, ref, beg + 100 + 7 * k) for k in range(40)]
        segs = []
        for i in range(n_on_tile):                    # all inside the first 512 positions: one tile at every tile size
            k = rng.randrange(40)
            q0 = rng.randint(0, 30)
            segs.append((beg + 100 + 7 * k + q0, reads[k], q0, rng.randint(1, 60 - q0), rng.choice((1, 2, 3, 4)), rng.random() < 0.5))
        far = (beg + 2 * 2048 + 10, reads[0], 0, 50, 1, 0)      # on the last tile of every geometry
        if shuffle:
            rng.shuffle(segs)
            segs.insert(len(segs) // 2, far)                     # inside the first tile's run without being on it
        else:
            segs.append(far)
        for s in segs:
            B.seg(*s, 0)
        batch = B.batch(0, beg, end)

        def reaches(batch, tile, result):
            first, last, n = tile_runs(batch, tile)[0]
            return n == n_on_tile and nonzero(result) and (last - first == n + 1 if shuffle else last - first == n)
        return ref, {}, None, batch, reaches
    return case


# ---- deep pile: the LDS counters and the width of md_site ----
def deep_case(kind):
    def case():
        ref = b"ATTACGTTAT" * 60
        p = 304 if kind != "ob" else 305              # the C / the G of one CpG
        B = Builder()
        meth = B.read("C" if kind != "ob" else "G", 30)
        unmeth = B.read("T" if kind != "ob" else "A", 30)
        low = B.read("C" if kind != "ob" else "G", 3)
        other = B.read("A", 30)
        own, opp = (1, 2) if kind != "ob" else (2, 1)
        for i in range(70000):
            if kind == "opposite":
                B.seg(p, other if i % 3 else meth, 0, 1, opp if i % 2 else opp + 2, i & 1, 0)
            else:
                B.seg(p, meth, 0, 1, own, i & 1, 0)
        if kind != "opposite":                         # 66,000 of the other call and a few below -p: both counters pass 16 bits
            for i in range(66000):
                B.seg(p, unmeth if i % 1000 else low, 0, 1, own + 2, 0, 0)
        batch = B.batch(0, 0, len(ref))

        def reaches(batch, tile, result):
            if kind == "opposite":
                return result[p][4] > 65535 and result[p][5] > 40000
            return result[p][2] > 65535 and result[p][3] > 65535 and len(result) == 1
        return ref, ({"mod": (1,)} if kind == "opposite" else {}), None, batch, reaches
    return case


# ---- trimming: trim_window, make_rd, the padding between sequence and qualities ----
LQS = (37, 40)
TRIM_SETS = [        # (bounds pair, absoluteBounds pair as a function of lq): every listed value at least once
    ((0, 0), lambda lq: (0, 0)),
    ((5, 0), lambda lq: (3, 4)),
    ((0, 20), lambda lq: (lq, 0)),
    ((5, 20), lambda lq: (0, lq)),
    ((30, 20), lambda lq: (lq + 5, lq + 5)),
    ((200, 0), lambda lq: (0, 0)),
    ((0, 200), lambda lq: (3, 4)),
    ((5, 20), lambda lq: (3, 4)),
    ((0, 0), lambda lq: (lq, 0)),
    ((0, 0), lambda lq: (0, lq)),
]


def trim_case(k, lq):
    def case():
        rng = random.Random(100 * k + lq)
        bounds, ab = [0] * 16, [0] * 16
        for s, r2 in STRAND_READS:                          # the same pair for every strand and read number (trim_mixed: all different)
            bnd, absf = TRIM_SETS[k]
            o = 4 * (s - 1) + 2 * r2
            bounds[o:o + 2] = bnd
            ab[o:o + 2] = absf(lq)
        ref = edge_ref(1200, 31)
        B = Builder()
        for s, r2 in STRAND_READS:
            for rep in range(6):
                pos = 20 + 97 * rep + 13 * s + r2
                a = rand_read(B, rng, lq, ref, pos)
                B.seg(pos, a, 0, lq, s, r2, 0)                                  # whole read, even q0
                B.seg(pos + 1, a, 1, lq - 1, s, r2, 0)                          # odd q0
                B.seg(pos + 6, a, 6, 9, s, r2, 0)
                B.seg(pos + 21, a, 21, lq - 21, s, r2, 0)
        batch = B.batch(0, 0, len(ref))

        def reaches(batch, tile, result):
            from batch_eval import _window
            cfg = make_cfg({"bounds": bounds, "absoluteBounds": ab}, (1, 1, 1), 1, 0)
            lo, hi = _window(cfg, 1, 0, lq)
            return (nonzero(result)) == (hi > lo) and all(_window(cfg, s, r2, lq) == (lo, hi) for s, r2 in STRAND_READS)
        return ref, {"bounds": tuple(bounds), "absoluteBounds": tuple(ab), "minPhred": 5}, None, batch, reaches
    return case


def trim_mixed():
    """different bounds for every strand and read number, empty and over-long windows among them"""
    rng = random.Random(33)
    pairs = [(0, 0), (5, 0), (0, 20), (5, 20), (30, 20), (200, 0), (0, 200), (5, 20)]
    apairs = [(3, 4), (0, 0), (40, 0), (0, 37), (45, 45), (3, 4), (0, 0), (37, 0)]
    bounds = [v for p in pairs for v in p]
    ab = [v for p in apairs for v in p]
    ref = edge_ref(1500, 34)
    B = Builder()
    for rep in range(80):
        lq = rng.choice(LQS)
        pos = rng.randint(0, 1450)
        s, r2 = rng.choice(STRAND_READS)
        a = rand_read(B, rng, lq, ref, pos)
        q0 = rng.randint(0, 10)
        B.seg(pos + q0, a, q0, lq - q0, s, r2, 0)
    batch = B.batch(0, 0, len(ref))
    return ref, {"bounds": tuple(bounds), "absoluteBounds": tuple(ab)}, None, batch, lambda batch, tile, result: nonzero(result)


# ---- partner: resolve_overlap / resolve_own, the partner's window ----
PQ = (0, 4, 5, 213, 214, 255)


def partner_case(min_phred, seconds):
    """every base pair of {C, T, G, A, N}^2 x every quality pair of PQ^2 on sites of both kinds, the owner being the earlier or the later
    mate; the partner has another strand and read number than the owner, its own bounds trim it part-way through the segment"""
    def case():
        bounds, ab = [0] * 16, [0] * 16
        bounds[0:4] = (0, 0, 3, 0)             # OT: read 1 untrimmed, read 2 loses its first 3
        bounds[4:8] = (0, 30, 0, 0)            # OB: read 1 keeps [0, 30)
        ab[8:12] = (0, 0, 0, 8)                # CTOT read 2 loses its last 8
        ab[12:16] = (7, 0, 0, 0)               # CTOB read 1 loses its first 7
        unit = "CGATCGTA"
        ref = (unit * 400).encode()
        B = Builder()
        combos = [(a, b, qa, qb) for a in (2, 8, 4, 1, 15) for b in (2, 8, 4, 1, 15) for qa in PQ for qb in PQ]
        L = 40
        at = 0
        for strand, r2, mstrand, mr2 in ((1, 0, 2, 0), (2, 1, 1, 1), (3, 0, 4, 0), (4, 1, 3, 1), (1, 1, 4, 0), (2, 0, 3, 1)):
            for c0 in range(0, len(combos), L):
                part = combos[c0:c0 + L]
                own = B.read([c[0] for c in part] + [15] * (L - len(part)), [c[2] for c in part] + [0] * (L - len(part)))
                mate = B.read([15] * 5 + [c[1] for c in part] + [15] * (L - len(part)), [9] * 5 + [c[3] for c in part] + [0] * (L - len(part)))
                for second in seconds:
                    for sh in range(4):            # four consecutive places: every base pair meets a C site and a G site of the unit
                        B.seg(at + sh, own, 0, L, strand, r2, second, partner=mate, m_q0=5, m_strand=mstrand, m_read2=mr2)
                at += 11
        batch = B.batch(0, 0, len(ref))

        def reaches(batch, tile, result):
            from batch_eval import _window
            cfg = make_cfg({"bounds": bounds, "absoluteBounds": ab}, (1, 1, 1), 1, 0)
            S = seg_array(batch)
            cut = 0
            for s in S[:50]:                    # the partner's index leaves its window inside the segment
                lo, hi = _window(cfg, int(s["msf"]) & 7, bool(s["msf"] & 8), int(s["m_l_qseq"]))
                a, b = int(s["m_q0"]), int(s["m_q0"]) + int(s["len"])
                cut += (a < lo < b) or (a < hi < b)
            return cut > 0 and nonzero(result) and all(s["sf"] & 32 for s in S)
        return ref, {"bounds": tuple(bounds), "absoluteBounds": tuple(ab), "minPhred": min_phred}, None, batch, reaches
    return case


def partner_mix():
    """steps of the quarter-wavefront kernel where all eight segments have partners, none has, and both kinds (seg_sort, the anyp split)"""
    rng = random.Random(35)
    ref = edge_ref(2 * 2048 + 300, 36)
    B = Builder()
    pat = [1] * 64 + [0] * 64 + [1, 0] * 32 + [1, 1, 1, 0, 0, 0, 0, 1] * 8 + [0] * 63 + [1] + [1] * 63 + [0]
    for p in pat * 3:
        lq = rng.randint(40, 120)
        pos = rng.randint(10, 380)
        a = rand_read(B, rng, lq, ref, pos)
        s, r2 = rng.choice(STRAND_READS)
        if p:
            mlq = rng.randint(40, 120)
            n = rng.randint(1, min(lq, mlq))
            q0, mq0 = rng.randint(0, lq - n), rng.randint(0, mlq - n)
            ms, mr2 = rng.choice(STRAND_READS)
            B.seg(pos + q0, a, q0, n, s, r2, rng.random() < 0.5, partner=rand_read(B, rng, mlq, ref, pos + q0 - mq0), m_q0=mq0, m_strand=ms, m_read2=mr2)
        else:
            B.seg(pos, a, 0, lq, s, r2, 0)
    batch = B.batch(0, 0, len(ref))

    def reaches(batch, tile, result):
        S = seg_array(batch)
        flags = [bool(s & 32) for s in S["sf"]]
        waves = [flags[i:i + 64] for i in range(0, len(flags) - 63, 64)]
        return nonzero(result) and any(all(w) for w in waves) and any(not any(w) for w in waves) and any(any(w) and not all(w) for w in waves)
    return ref, {"minPhred": 5}, None, batch, reaches


# ---- strand 0 ----
def strand0_case(over_g):
    def case():
        ref = b"ATTACGTTAT" * 60
        B = Builder()
        rng = random.Random(37)
        sprinkle(B, rng, ref, 30, 30, 80)
        whole = B.read(ref.decode().replace("C", "A"), 30)
        for k in range(20, 40):                        # ATTAC (over_g: ATTACG, the G of the CpG included) read as ATTAA: evidence against the C
            B.seg(10 * k, whole, 10 * k, 6 if over_g and k == 33 else 5, 0, k & 1, 0)
        batch = B.batch(0, 0, len(ref))

        def reaches(batch, tile, result):
            if over_g:
                return result == ERR_STRAND0
            return nonzero(result) and any(v[4] > 0 and v[5] > 0 for v in result.values())
        return ref, {}, None, batch, reaches
    return case


# ---- seeded fuzz ----
def fuzz_case(seed):
    def case():
        rng = random.Random(7000 + seed)
        density = (0.05, 0.5, 1.0)[seed % 3]
        ntiles = 2 + seed % 4
        tile = TILES[(seed // 3) % 4]
        beg = rng.randint(0, 600)
        end = beg + (ntiles - 1) * tile + rng.randint(1, tile)
        n = end + rng.randint(0, 200)
        ref = rand_ref(rng, n, density, letters="ATatNn", cg="CGCGcg")
        nsegs = rng.randint(200, 1500)
        B = Builder()
        while len(B.segs) < nsegs:
            sprinkle(B, rng, ref, 1, 1, 150, lo=beg - 100, hi=min(n, end + 100), partner_frac=0.4, strands=(1, 2, 3, 4))
        del B.segs[nsegs:]
        rng.shuffle(B.segs)
        fields = {"minPhred": (1, 5, 20)[seed % 3],
                  "bounds": tuple(rng.choice((0, 0, 3, 10, 60, 140, 200)) for _ in range(16)),
                  "absoluteBounds": tuple(rng.choice((0, 0, 0, 2, 9, 50)) for _ in range(16))}
        batch = B.batch(0, beg, end)

        def reaches(batch, tile_, result):
            return batch.n_segs == nsegs and nonzero(result) and len(tiles_of(batch, tile)) == ntiles
        return ref, fields, None, batch, reaches
    return case


CASES = []
for _l in (1, 2, 3, 5, 513, 2051):
    for _v in range(3):
        CASES.append((f"carpet_{_l}_{'abc'[_v]}", carpet_case(_l, _v)))
CASES += [(f"regions_{k}", region_case(k)) for k in REGION_SETS]
CASES += [(f"lists_{k}", lists_case(k)) for k in ("allC", "allG", "CG", "oneC", "pow2")]
CASES += [("edges_points", edges_points), ("edges_span", edges_span), ("edges_contig_end", edges_contig_end), ("edges_gap", edges_gap),
          ("edges_nosegs", edges_nosegs), ("edges_empty", edges_empty)]
CASES += [(f"rounds_{n}", rounds_case(n, 0)) for n in (512, 513, 1024, 1025)] + [("rounds_shuffled", rounds_case(700, 1))]
CASES += [(f"deep_{k}", deep_case(k)) for k in ("ot", "ob", "opposite")]
CASES += [(f"trim_{k}_{lq}", trim_case(k, lq)) for k in range(len(TRIM_SETS)) for lq in LQS]
CASES += [("trim_mixed", trim_mixed)]
CASES += [("partner_p1", partner_case(1, (0, 1))), ("partner_p5", partner_case(5, (0,))), ("partner_p209", partner_case(209, (1,))),
          ("partner_p210", partner_case(210, (0, 1))), ("partner_mix", partner_mix)]
CASES += [("strand0_over_g", strand0_case(1)), ("strand0_over_c", strand0_case(0))]
CASES += [(f"fuzz_{s}", fuzz_case(s)) for s in range(20)]
CASE_FN = dict(CASES)
WIDE_TILES = ("lists_", "edges_", "fuzz_")          # these also run at 1024 and 1536


def tiles_for(name):
    return TILES if name.startswith(WIDE_TILES) else (512, 2048)


_built = {}


def build(name):
    """a case built once: (ref, fields, regions, batch, reaches)"""
    if name not in _built:
        _built[name] = CASE_FN[name]()
    return _built[name]


_expected = {}


def expected(name, keep, mod):
    """the evaluator's answer, computed once per (case, keep) with minOppositeDepth on; without it the opposite-strand counters are
    dropped, as the kernels without VARIANT never make them"""
    ref, fields, regions, batch, _ = build(name)
    k = (name, keep)
    if k not in _expected:
        _expected[k] = expected_sites(ref, fields, regions, batch, keep, 1)
    return without_opposite(_expected[k], mod)


def without_opposite(want, mod):
    if mod or not isinstance(want, dict):
        return want
    return {p: v[:4] + (0, 0) for p, v in want.items() if v[2] + v[3] > 0}


# ---- mbias: k_mbias, mbias_seg, the window-relative contexts ----
def mbias_edges(variant):
    """G at beg and beg + 1, C at end - 1 and end - 2, with beg and end inside the contig and the deciding neighbour just outside the
    chunk's window [beg, end] (a: the C at end - 1 keeps its G at end; b: its G at end + 1 is outside)"""
    def case():
        ref = bytearray(edge_ref(3400, 41))
        beg, end = 500, 500 + 2048 + 600
        ref[beg - 2:beg + 3] = b"CCGGA"           # G at beg (CpG by the C before the window: CHH inside), G at beg + 1 (CHG by it: CHH inside)
        ref[end - 3:end + 2] = b"ACCGG" if variant == "a" else b"TTCAG"
        ref = bytes(ref)
        B = Builder()
        whole = B.read(ref.decode(), 30)
        for strand in (1, 2, 3, 4):
            for r2 in (0, 1):
                B.seg(beg - 10, whole, beg - 10, 40, strand, r2, 0)
                B.seg(end - 30, whole, end - 30, 40, strand, r2, 0)
        sprinkle(B, random.Random(42), ref, 60, 30, 120, lo=beg, hi=end)
        batch = B.batch(0, beg, end)
        return ref, {"keeps": KEEPS4}, None, batch, lambda batch, tile, result: isinstance(result, dict) and len(result) > 40
    return case


def mbias_long():
    """reads of 511, 512, 513 and 700 bases: the histogram rows on both sides of the 512 kept in LDS"""
    rng = random.Random(43)
    ref = edge_ref(3 * 2048, 44)
    B = Builder()
    for lq in (511, 512, 513, 700) * 4:
        pos = rng.randint(0, len(ref) - 300)
        a = rand_read(B, rng, lq, ref, pos)
        B.seg(pos, a, 0, lq, rng.choice((1, 2, 3, 4)), rng.random() < 0.5, 0)
    batch = B.batch(0, 0, len(ref))

    def reaches(batch, tile, result):
        qs = {k[2] for k in result}
        return max(qs) > 600 and any(500 <= q < 512 for q in qs) and any(512 <= q < 530 for q in qs)
    return ref, {"minPhred": 5}, None, batch, reaches


def mbias_trimmed():
    rng = random.Random(45)
    ref = edge_ref(2500, 46)
    B = Builder()
    sprinkle(B, rng, ref, 200, 37, 40)
    bounds = tuple(v for p in [(0, 0), (5, 0), (0, 20), (5, 20), (30, 20), (200, 0), (0, 200), (5, 20)] for v in p)
    ab = tuple(v for p in [(3, 4), (0, 0), (40, 0), (0, 37), (45, 45), (3, 4), (0, 0), (37, 0)] for v in p)
    batch = B.batch(0, 10, 2400)
    return ref, {"bounds": bounds, "absoluteBounds": ab}, None, batch, lambda batch, tile, result: len(result) > 20


def mbias_deep():
    ref = b"ATTACGTTAT" * 60
    B = Builder()
    a = B.read("TTCAA", 30)
    for i in range(70000):
        B.seg(304 - 2, a, 0, 5, 1, 0, 0) if i % 2 else B.seg(304, a, 2, 1, 1, 0, 0)
    batch = B.batch(0, 0, len(ref))
    return ref, {}, None, batch, lambda batch, tile, result: result == {(1, 1, 2): (70000, 0)}


def mbias_strand0():
    ref, fields, regions, batch, _ = strand0_case(1)()
    return ref, fields, None, batch, lambda batch, tile, result: result == ERR_STRAND0


MBIAS_CASES = [("mbias_edges_a", mbias_edges("a")), ("mbias_edges_b", mbias_edges("b")), ("mbias_long", mbias_long), ("mbias_trimmed", mbias_trimmed), ("mbias_deep", mbias_deep),
               ("mbias_strand0", mbias_strand0)]
MBIAS_FN = dict(MBIAS_CASES)


def build_mbias(name):
    if name not in _built:
        _built[name] = MBIAS_FN[name]()
    return _built[name]


def expected_mbias(name, keep):
    k = (name, keep)
    if k not in _expected:
        ref, fields, _, batch, _ = build_mbias(name)
        _expected[k] = expected_hist(ref, fields, batch, keep)
    return _expected[k]
