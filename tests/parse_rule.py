"""What tests/test_parse_cpu.py and tests/test_gpu_parse.py share: the parser's rule (csrc/mdk_parse_core.h) restated with bytes.split, a small
seeded reference, texts built so that lines fall on the kernels' 4096-byte span edges, and the list of refusals with their messages.
A calls row is (contig, start, end, nmeth, nunmeth, context, strand), a report row (contig, pos, strand, nmeth, nunmeth, context, tri)."""
import functools

import numpy as np

BEDGRAPH, REPORT = 0, 1
MAX_LINE, SPAN = 512, 4096
BIG = 2 ** 31 - 1
CALL_COLUMNS = ("contig", "start", "end", "nmeth", "nunmeth", "context", "strand")
CALL_DTYPES = ("int32", "int32", "int32", "int32", "int32", "uint8", "int8")
REPORT_COLUMNS = ("contig", "pos", "strand", "nmeth", "nunmeth", "context", "trinucleotide")
REPORT_DTYPES = ("int32", "int32", "int8", "int32", "int32", "uint8", "uint8")
HEADER = b'track type="bedGraph" description="x CpG methylation levels"\n'


# ---- the rule ----
def number(f):
    if not f.isdigit() or any(c < 48 or c > 57 for c in f):
        return "digit"
    if len(f) > 10 or int(f) > BIG:
        return "overflow"
    return int(f)


def site(seq, p):
    """(context, strand) of position p of a contig by mergeContext's site_of -- k_classify's rule --, or None where the base is neither C nor G"""
    up = lambda q: seq[q:q + 1].upper() if 0 <= q < len(seq) else b""
    if up(p) == b"C":
        return (0 if up(p + 1) == b"G" else 1 if up(p + 2) == b"G" else 2), 1
    if up(p) == b"G":
        return (0 if up(p - 1) == b"C" else 1 if up(p - 2) == b"C" else 2), -1
    return None


def parse_line(line, has_newline, fmt, contigs, bases):
    """the row of one line (its newline taken off), or the name of the one refusal: the first that applies"""
    if len(line) + (1 if has_newline else 0) > MAX_LINE:
        return "long"
    if line.endswith(b"\r"):
        line = line[:-1]
    if not line:
        return "empty"
    f = line.split(b"\t")
    want = 7 if fmt == REPORT else 6
    if len(f) != want:
        return "few" if len(f) < want else "many"
    if any(not x for x in f):
        return "field"
    name = f[0].decode("latin-1")
    if name not in contigs:
        return "contig"
    c = contigs.index(name)
    a = number(f[1])
    if isinstance(a, str):
        return a
    if fmt == REPORT:
        if a < 1:
            return "range"
        if f[2] not in (b"+", b"-"):
            return "strand"
        m = number(f[3])
        if isinstance(m, str):
            return m
        u = number(f[4])
        if isinstance(u, str):
            return u
        if f[5] not in (b"CG", b"CHG", b"CHH"):
            return "context"
        if len(f[6]) != 3 or any(x not in b"ACGTN" for x in f[6]):
            return "tri"
        return (c, a, 1 if f[2] == b"+" else -1, m, u, (b"CG", b"CHG", b"CHH").index(f[5]), f[6].decode())
    b = number(f[2])
    if isinstance(b, str):
        return b
    m = number(f[4])
    if isinstance(m, str):
        return m
    u = number(f[5])
    if isinstance(u, str):
        return u
    if b != a + 1:
        return "merged"
    if bases is None or bases[c] is None:
        return "noref"
    if a >= len(bases[c]):
        return "range"
    s = site(bases[c], a)
    if s is None:
        return "base"
    return (c, a, b, m, u, s[0], s[1])


def parse_text(text, fmt, contigs, bases=None):
    """(rows, refusals): the rows of every line that is no `track` line, and (offset, name) of every refused line, ascending"""
    rows, refused, at, n = [], [], 0, len(text)
    while at < n:
        e = text.find(b"\n", at)
        has_newline = e >= 0
        if not has_newline:
            e = n
        if text[at:at + 5] != b"track":
            r = parse_line(text[at:e], has_newline, fmt, contigs, bases)
            if isinstance(r, str):
                refused.append((at, r))
            else:
                rows.append(r)
        at = e + 1
    return rows, refused


# what the library says for a refusal (csrc/mdk_parse_core.h prs_error_text), by the name tools/parse_emu prints
MESSAGES = {"long": "longer than 512 bytes", "empty": "an empty line", "few": "too few fields", "many": "too many fields", "field": "an empty field",
            "contig": "not among the contig names", "digit": "something else than decimal digits", "overflow": "larger than INT32_MAX",
            "merged": "looks merged already", "noref": "no resident reference", "range": "outside the contig", "base": "neither C nor G",
            "strand": "neither \\+ nor -", "context": "none of CG, CHG, CHH", "tri": "not three letters of ACGTN", "changed": "not the one that was measured"}


# ---- a reference: three contigs with lower case and N, one name a prefix of another ----
CONTIGS = ["c1", "c10", "scaffold_2"]
LENGTHS = (3001, 5003, 120001)


@functools.lru_cache(maxsize=None)
def reference():
    rng = np.random.default_rng(5)
    out = []
    for n in LENGTHS:
        s = rng.choice(np.frombuffer(b"ACGTacgtNn", dtype=np.uint8), n, p=[.2, .2, .2, .2, .04, .04, .04, .04, .02, .02])
        out.append(s.tobytes())
    return tuple(out)


def fasta_text(width=60):
    out = []
    for k, (name, seq) in enumerate(zip(CONTIGS, reference())):
        out.append(b">" + name.encode() + (b" a description\n" if k else b"\n"))
        out += [seq[i:i + width] + b"\n" for i in range(0, len(seq), width)]
    return b"".join(out)


def contigs_file(bases=True):
    """what tools/parse_emu takes as its CONTIGS argument"""
    return b"".join(n.encode() + (b"\t" + s if bases else b"") + b"\n" for n, s in zip(CONTIGS, reference()))


@functools.lru_cache(maxsize=None)
def cytosines(c):
    """the positions of contig c whose base is a C or a G"""
    s = np.frombuffer(reference()[c].upper(), dtype=np.uint8)
    return np.nonzero((s == ord("C")) | (s == ord("G")))[0].tolist()


def other_base(c=0):
    s = reference()[c].upper()
    return next(p for p in range(10, len(s)) if s[p:p + 1] in (b"A", b"T", b"N"))


def bed_line(c, p, m, u, pct=None, end=None):
    return b"%s\t%d\t%d\t%s\t%d\t%d\n" % (CONTIGS[c].encode(), p, p + 1 if end is None else end, pct if pct is not None else b"%d" % (100 * m // max(m + u, 1)), m, u)


def bed_lines(n, seed=1):
    """n good lines, contigs and positions in no particular order"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        c = int(rng.integers(0, 3)); ps = cytosines(c)
        out.append(bed_line(c, ps[int(rng.integers(0, len(ps)))], int(rng.integers(0, 1000)), int(rng.integers(0, 1000))))
    return out


def fill(target, seed=2):
    """good lines of exactly `target` bytes in all: the last one's percentage column is stretched to fit (the parser does not look at it)"""
    out, n = [], 0
    for l in bed_lines(target // 16 + 2, seed):
        if n + len(l) + 40 > target:
            break
        out.append(l); n += len(l)
    last = bed_line(0, cytosines(0)[3], 4, 5, pct=b"")
    pad = target - n - len(last)
    assert 0 < pad < MAX_LINE - len(last), (target, pad)
    out.append(bed_line(0, cytosines(0)[3], 4, 5, pct=b"7" * pad))
    text = b"".join(out)
    assert len(text) == target and text.endswith(b"\n")
    return text


def line_of(size):
    """a good line of exactly `size` bytes, newline included"""
    l = bed_line(1, cytosines(1)[7], 12, 3, pct=b"")
    return bed_line(1, cytosines(1)[7], 12, 3, pct=b"5" * (size - len(l)))


@functools.lru_cache(maxsize=None)
def blocking():
    """name -> text: bedGraph texts whose lines meet the edges of the 4096-byte spans in every way"""
    tail = b"".join(bed_lines(40, 3))
    track = b'track type="bedGraph" description="another file"\n'
    t = {
        "a line starts at byte 4096, a newline ends the span": fill(SPAN) + tail,
        "and at 8192": fill(SPAN) + fill(SPAN, 4) + tail,
        "a line straddles two spans": fill(SPAN - 9) + tail,
        "track at 4094": fill(SPAN - 2) + track + tail,
        "track at 4092": fill(SPAN - 4) + track + tail,
        "track at 4095": fill(SPAN - 1) + track + tail,
        "track at 4096": fill(SPAN) + track + tail,
        "a 512-byte line over the edge": fill(SPAN - 200) + line_of(MAX_LINE) + tail,
        "a 512-byte line from the span's last byte": fill(SPAN - 1) + line_of(MAX_LINE) + tail,
        "a 512-byte line ends the text without a newline": fill(SPAN - 1) + line_of(MAX_LINE + 1)[:-1],
        "the look-ahead passes the end": fill(SPAN - 9) + bed_lines(1, 5)[0],
        "the text ends with the span": fill(SPAN),
        "no final newline": (HEADER + tail)[:-1],
        "crlf": (HEADER + tail).replace(b"\n", b"\r\n"),
        "one line": bed_lines(1, 6)[0],
        "one line, no newline": bed_lines(1, 6)[0][:-1],
        "empty": b"",
        "header only": HEADER,
        "header only, no newline": HEADER[:-1],
        "tracks in between": HEADER + tail + track + track + tail + track,
        "1025 spans": HEADER + b"".join(bed_lines((1025 * SPAN) // 20, 8)),
    }
    assert len(t["1025 spans"]) > 1025 * SPAN - SPAN and len(t["1025 spans"]) > 1024 * SPAN
    return t


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement over blocking()[name]: computed once, shared by the tests"""
    rows, refused = parse_text(blocking()[name], BEDGRAPH, CONTIGS, reference())
    assert not refused, (name, refused[:3])
    return tuple(rows)


def report_line(c, pos, strand, m, u, ctx, tri):
    return b"%s\t%d\t%s\t%d\t%d\t%s\t%s\n" % (CONTIGS[c].encode(), pos, strand, m, u, ctx, tri)


def refusals():
    """(id, the refusal's name, fmt, the bad line): every refusal on its own; the lines around it are good"""
    p, q = cytosines(0)[5], other_base(0)
    n0 = CONTIGS[0].encode()
    good = bed_line(0, p, 3, 4)
    rep = lambda **k: report_line(**{**dict(c=0, pos=7, strand=b"+", m=1, u=2, ctx=b"CHG", tri=b"CAG"), **k})
    return [
        ("empty", "empty", BEDGRAPH, b"\n"), ("empty-crlf", "empty", BEDGRAPH, b"\r\n"),
        ("few", "few", BEDGRAPH, b"%s\t%d\t%d\t50\t1\n" % (n0, p, p + 1)), ("few-one", "few", BEDGRAPH, b"x\n"),
        ("many-seventh-column", "many", BEDGRAPH, good[:-1] + b"\textra\n"), ("many-doubled-tab", "many", BEDGRAPH, good.replace(b"\t", b"\t\t", 1)),
        ("many-trailing-tab", "many", BEDGRAPH, good[:-1] + b"\t\n"),
        ("field-pct", "field", BEDGRAPH, bed_line(0, p, 3, 4, pct=b"")), ("field-chrom", "field", BEDGRAPH, good[len(n0):]),
        ("field-last", "field", BEDGRAPH, b"%s\t%d\t%d\t50\t1\t\n" % (n0, p, p + 1)),
        ("contig", "contig", BEDGRAPH, b"c\t%d\t%d\t50\t1\t1\n" % (p, p + 1)), ("contig-longer", "contig", BEDGRAPH, b"c100\t%d\t%d\t50\t1\t1\n" % (p, p + 1)),
        ("digit-plus", "digit", BEDGRAPH, b"%s\t+%d\t%d\t50\t1\t1\n" % (n0, p, p + 1)), ("digit-blank", "digit", BEDGRAPH, b"%s\t %d\t%d\t50\t1\t1\n" % (n0, p, p + 1)),
        ("digit-minus", "digit", BEDGRAPH, b"%s\t%d\t%d\t50\t-1\t1\n" % (n0, p, p + 1)), ("digit-tail", "digit", BEDGRAPH, b"%s\t%d\t%d\t50\t1\t1x\n" % (n0, p, p + 1)),
        ("digit-end", "digit", BEDGRAPH, b"%s\t%d\t%d.\t50\t1\t1\n" % (n0, p, p + 1)),
        ("overflow", "overflow", BEDGRAPH, b"%s\t%d\t%d\t50\t2147483648\t1\n" % (n0, p, p + 1)), ("overflow-11-digits", "overflow", BEDGRAPH, b"%s\t%d\t%d\t50\t1\t00000000001\n" % (n0, p, p + 1)),
        ("overflow-start", "overflow", BEDGRAPH, b"%s\t4294967296\t4294967297\t50\t1\t1\n" % n0),
        ("merged", "merged", BEDGRAPH, bed_line(0, p, 3, 4, end=p + 2)), ("merged-same", "merged", BEDGRAPH, bed_line(0, p, 3, 4, end=p)),
        ("merged-at-the-top", "merged", BEDGRAPH, bed_line(0, BIG, 3, 4, end=BIG)),
        ("range", "range", BEDGRAPH, bed_line(0, LENGTHS[0], 3, 4)), ("range-far", "range", BEDGRAPH, bed_line(1, BIG - 1, 3, 4)),
        ("base", "base", BEDGRAPH, bed_line(0, q, 3, 4)),
        ("long", "long", BEDGRAPH, line_of(MAX_LINE + 1)), ("long-garbage", "long", BEDGRAPH, b"z" * 700 + b"\n"),
        ("report-few", "few", REPORT, good), ("report-many", "many", REPORT, rep()[:-1] + b"\t1\n"),
        ("report-pos-0", "range", REPORT, rep(pos=0)), ("report-strand", "strand", REPORT, rep(strand=b"*")), ("report-strand-2", "strand", REPORT, rep(strand=b"+-")),
        ("report-context", "context", REPORT, rep(ctx=b"CHX")), ("report-context-lower", "context", REPORT, rep(ctx=b"cg")), ("report-context-long", "context", REPORT, rep(ctx=b"CHGG")),
        ("report-tri", "tri", REPORT, rep(tri=b"CGX")), ("report-tri-short", "tri", REPORT, rep(tri=b"CG")), ("report-tri-lower", "tri", REPORT, rep(tri=b"cag")),
        ("report-digit", "digit", REPORT, rep(pos=7).replace(b"\t7\t", b"\t7.0\t")), ("report-contig", "contig", REPORT, rep()[1:]),
    ]


def around(bad, fmt, edge=False):
    """(text, the offset of the bad line): good lines before and after it; edge: the bad line straddles the first span edge (or starts at
    the span's last byte when it is too short to straddle)"""
    good = b"".join(bed_lines(5, 9)) if fmt == BEDGRAPH else b"".join(report_line(0, 5 + k, b"-", k, 1, b"CHH", b"CTN") for k in range(5))
    if not edge:
        return good + bad + good, len(good)
    at = SPAN - max(1, min(len(bad) // 2, 300))
    if fmt == BEDGRAPH:
        return fill(at) + bad + good, at
    # a report's fields cannot be stretched: a `track` line, which is no row, takes up what is missing
    head = good * ((at - 300) // len(good))
    pad = at - len(head)
    assert 6 <= pad <= MAX_LINE
    return head + b"track" + b"." * (pad - 6) + b"\n" + bad + good, at
