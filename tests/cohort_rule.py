"""What tests/test_cohort_io_cpu.py and tests/test_gpu_cohort_io.py share: the two formats of Cohort.write and the strictness of Cohort.read
(csrc/mdk_cohort_core.h) restated with str.join / bytes.split, seeded tables, and the list of refusals with their messages.
A table is a dict: contigs (names), names (samples), merged, contexts_on, n_union, sites -- a list of (contig, start, end, context, strand,
nsamples) --, and m, u: S lists of n counts."""
import functools
import random

BIG = 2 ** 31 - 1
MAX_LINE = 32768
SIGNATURE = "#methyldackel_amd cohort 1"
SITE_NAMES = ["#chrom", "start", "end", "context", "strand", "nsamples"]
SITE_COLUMNS = (("contig", "int32"), ("start", "int32"), ("end", "int32"), ("context", "uint8"), ("strand", "int8"), ("nsamples", "int32"))
CONTEXT = ("CG", "CHG", "CHH")
# the refusals of a line in the order in which the first wins, with what the library says
MESSAGES = {"long": "a line is longer than 32768 bytes", "hash": "a # line behind the two header lines", "empty": "an empty line",
            "few": "a line has too few fields", "many": "a line has too many fields", "field": "a line has an empty field",
            "contig": "a line's contig is not among the contig names", "digit": "a number holds something else than decimal digits",
            "overflow": "a number is larger than INT32_MAX", "context": "a context is none of CG, CHG, CHH", "strand": "a strand is none of +, - and .",
            "end": "end is not above start", "nsamples": "nsamples is above the number of samples", "order": "a row is not strictly ascending"}
WRITE_MESSAGES = {"position": "a contig or a start is negative", "contig": "a contig index lies outside the contig names", "end": "end is not above start",
                  "context": "a context is above 2", "negative": "a count is negative"}


# ---- write ----
def header(fmt, t):
    S = len(t["names"])
    if fmt == "methylBase":
        return "\t".join(["chr", "start", "end", "strand"] + ["%s%d" % (w, k + 1) for k in range(S) for w in ("coverage", "numCs", "numTs")]) + "\n"
    first = "\t".join([SIGNATURE, "samples=%d" % S, "merged=%d" % int(t["merged"]), "contexts=" + ",".join(str(x) for x in t["contexts_on"]), "n_union=%d" % t["n_union"]])
    second = "\t".join(SITE_NAMES + ["%s.%s" % (v, w) for v in t["names"] for w in ("nmeth", "nunmeth")])
    return first + "\n" + second + "\n"


def line(fmt, t, i):
    c, a, b, x, s, k = t["sites"][i]
    S = len(t["m"])
    if fmt == "methylBase":
        f = [t["contigs"][c], str(a + 1), str(a + 1), "+" if s >= 0 else "-"]
        for j in range(S):
            m, u = t["m"][j][i], t["u"][j][i]
            f += [str((m + u) & 0xffffffff), str(m), str(u)]
    else:
        f = [t["contigs"][c], str(a), str(b), CONTEXT[x], "+" if s > 0 else "-" if s < 0 else ".", str(k)]
        for j in range(S):
            f += [str(t["m"][j][i]), str(t["u"][j][i])]
    return "\t".join(f) + "\n"


def body(fmt, t):
    return "".join(line(fmt, t, i) for i in range(len(t["sites"]))).encode("latin-1")


def render(fmt, t):
    return header(fmt, t).encode("latin-1") + body(fmt, t)


def write_refusal(t):
    """(reason, site, sample or None) of the first site a writer refuses, or None"""
    for i, (c, a, b, x, s, k) in enumerate(t["sites"]):
        if c < 0 or a < 0:
            return "position", i, None
        if c >= len(t["contigs"]):
            return "contig", i, None
        if b <= a:
            return "end", i, None
        if x > 2:
            return "context", i, None
        for j in range(len(t["m"])):
            if t["m"][j][i] < 0 or t["u"][j][i] < 0:
                return "negative", i, j
    return None


# ---- read ----
def number(f):
    head = f[:11]
    if any(c < 48 or c > 57 for c in head):
        return "digit"
    if len(f) > 10 or int(f) > BIG:
        return "overflow"
    return int(f)


def parse_line(ln, has_newline, S, contigs):
    """the row of one line (its newline taken off) -- (contig, start, end, context, strand, nsamples, [m], [u]) -- or the name of the one refusal"""
    if len(ln) + (1 if has_newline else 0) > MAX_LINE:
        return "long"
    if ln.endswith(b"\r"):
        ln = ln[:-1]
    if ln.startswith(b"#"):
        return "hash"
    if not ln:
        return "empty"
    f = ln.split(b"\t")
    if len(f) != 6 + 2 * S:
        return "few" if len(f) < 6 + 2 * S else "many"
    if any(not x for x in f):
        return "field"
    name = f[0].decode("latin-1")
    if len(name) > 255 or name not in contigs:
        return "contig"
    out = [contigs.index(name)]
    for k in (1, 2):
        v = number(f[k])
        if isinstance(v, str):
            return v
        out.append(v)
    if f[3].decode("latin-1") not in CONTEXT:
        return "context"
    out.append(CONTEXT.index(f[3].decode("latin-1")))
    if f[4] not in (b"+", b"-", b"."):
        return "strand"
    out.append({b"+": 1, b"-": -1, b".": 0}[f[4]])
    counts = []
    for x in f[5:]:
        v = number(x)
        if isinstance(v, str):
            return v
        counts.append(v)
    out.append(counts[0])
    if out[2] <= out[1]:
        return "end"
    if counts[0] > S:
        return "nsamples"
    return tuple(out) + (counts[1::2], counts[2::2])


def parse(text, S, contigs, first_line=3):
    """the rows of the text behind a file's two header lines -- (sites, m, u) as a table holds them -- or (refusal, line number)"""
    lines = text.split(b"\n")
    last_has_newline = text.endswith(b"\n")
    if last_has_newline or not text:                                       # (no line behind the last newline, and none in no text)
        lines.pop()
    sites, m, u, prev = [], [[] for _ in range(S)], [[] for _ in range(S)], None
    for k, ln in enumerate(lines):
        r = parse_line(ln, k < len(lines) - 1 or last_has_newline, S, contigs)
        if isinstance(r, str):
            return r, first_line + k
        if prev is not None and not (r[0] > prev[0] or (r[0] == prev[0] and r[1] > prev[1])):
            return "order", first_line + k
        prev = r
        sites.append(r[:6])
        for j in range(S):
            m[j].append(r[6][j]); u[j].append(r[7][j])
    return sites, m, u


# ---- tables ----
def sample_names(S, length=None, seed=0):
    rng = random.Random(1000 + S + seed)
    if length is None:
        return ["s%d" % k for k in range(S)]
    out = set()
    while len(out) < S:
        out.add("".join(chr(rng.randrange(0x21, 0x7f)) for _ in range(length)))
    return sorted(out)


@functools.lru_cache(maxsize=None)
def shared_table(n, S, seed=0, merged=False):
    """a seeded table, strictly ascending: three contigs whose changes fall off every multiple of 64; cells mix 1- and 10-digit counts, so
    that neighbouring lines differ widely in length; `0 0` cells; every context and strand.  Cached: treat it as read-only"""
    rng = random.Random(77 * n + S + seed)
    contigs = ["chr1", "chrUn_gl000220", "c" * 255]
    cuts = sorted({(n * 2) // 5 + 3, (n * 7) // 10 + 5} if n > 12 else {1} if n > 1 else set())
    sites, c, x = [], 0, 0
    for i in range(n):
        if i in cuts:
            c, x = c + 1, 0
        x += rng.choice((1, 1, 2, 9, 1000, 123456))
        ctx = rng.randrange(3)
        strand = 0 if merged and ctx == 0 else rng.choice((1, -1))
        sites.append((c, x, x + (2 if strand == 0 else 1), ctx, strand, rng.randrange(S + 1)))
        if i == n - 1 and n > 3:
            sites[-1] = (c, BIG - 2, BIG, ctx, strand, S)                  # ten digits in the site columns too
    heavy = [rng.random() < 0.3 for _ in range(n)]                         # whole lines of ten-digit counts next to lines of one-digit ones
    count = lambda i: 0 if rng.random() < 0.2 else rng.randrange(1 << 30, BIG + 1) if heavy[i] or rng.random() < 0.05 else rng.randrange(10)
    m = [[count(i) for i in range(n)] for _ in range(S)]
    u = [[count(i) for i in range(n)] for _ in range(S)]
    return {"contigs": contigs, "names": sample_names(S), "merged": merged, "contexts_on": (0, 1, 2), "n_union": n + 5, "sites": sites, "m": m, "u": u}


def with_names(t, names):
    out = dict(t)
    out["names"] = list(names)
    return out
