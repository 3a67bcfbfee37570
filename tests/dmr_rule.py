"""The rule of csrc/mdk_dmr_core.h restated in plain Python loops over lists -- the numbers from tests/diff_rule.py --, the cases by hand
and the seeded tables the tests of Diff.dmrs share (test_dmr_cpu.py, test_gpu_dmr.py)."""
import random

from diff_rule import E_ENTRY, E_MARGIN, E_NEGATIVE, LIMIT, entry_check, margin_check, meth_diff, pvalue

E_ORDER, E_CONTIG = 8, 16
MESSAGES = {E_NEGATIVE: "a count is negative", E_ENTRY: "a count is 2^26 or more", E_ORDER: "not ascending in (contig, start), strictly",
            E_CONTIG: "contig is not an index into the contig names", E_MARGIN: "a region's pooled margin"}
CONTIGS = ["chr1", "chr2", "chrM"]
# both sides of a wavefront's 64 rows and of a workgroup's 256; 2049 and 4100: many workgroups and a short last one
SIZES = (1, 63, 64, 65, 255, 256, 257, 513, 2049, 4100)


class Refused(Exception):
    def __init__(self, bit, row):
        super().__init__(f"{MESSAGES[bit]} (row {row})")
        self.bit, self.row = bit, row


def direction(a, b, c, d):
    x = c * (a + b) - a * (c + d)
    return 1 if x > 0 else -1 if x < 0 else 0


def raw_regions(rows, sig, n_contigs, max_gap, max_skip):
    """rows: (contig, start, end, a, b, c, d) tuples; sig: a flag per row.  The raw regions as dicts, in ascending order; Refused for
    the first refused row, or -- where no row is refused -- for the first region whose pooled margins are"""
    n = len(rows)
    for i in range(n):
        contig, start, _, a, b, c, d = rows[i]
        err = entry_check(a) | entry_check(b) | entry_check(c) | entry_check(d)
        if contig < 0 or contig >= n_contigs:
            err |= E_CONTIG
        if i > 0 and not (rows[i - 1][0], rows[i - 1][1]) < (contig, start):
            err |= E_ORDER
        if err:
            raise Refused(err & -err, i)
    dirs = []
    for i in range(n):
        _, _, _, a, b, c, d = rows[i]
        dirs.append(direction(a, b, c, d) if sig[i] and a + b > 0 and c + d > 0 else 0)
    candidates = [i for i in range(n) if dirs[i] != 0]
    spans = []
    for k, i in enumerate(candidates):
        p = candidates[k - 1] if k else None
        if p is not None and rows[i][0] == rows[p][0] and dirs[i] == dirs[p] and rows[i][1] - rows[p][1] <= max_gap and i - p - 1 <= max_skip:
            spans[-1][1] = i
        else:
            spans.append([i, i])
    out = []
    for f, l in spans:
        sums = [0, 0, 0, 0]
        nsig = 0
        for i in range(f, l + 1):
            for q in range(4):
                sums[q] += rows[i][3 + q]
            nsig += dirs[i] != 0
        if margin_check(*sums):
            raise Refused(E_MARGIN, f)
        out.append({"first": f, "last": l, "contig": rows[f][0], "start": rows[f][1], "end": rows[l][2], "nsites": l - f + 1, "nsig": nsig,
                    "direction": dirs[f], "sums": tuple(sums), "meth_diff": meth_diff(*sums), "pooled": direction(*sums)})
    return out


def kept(r, min_sites, min_diff):
    return r["nsig"] >= min_sites and abs(r["meth_diff"]) >= min_diff and r["pooled"] == r["direction"]


def dmrs(rows, sig, n_contigs, max_gap, max_skip, min_sites, min_diff):
    """what Diff.dmrs gives: (contig, start, end, nsites, nsig, direction, a, b, c, d, meth_diff, pvalue) per kept region"""
    return [(r["contig"], r["start"], r["end"], r["nsites"], r["nsig"], r["direction"]) + r["sums"] + (r["meth_diff"], pvalue(*r["sums"])[0])
            for r in raw_regions(rows, sig, n_contigs, max_gap, max_skip) if kept(r, min_sites, min_diff)]


def census(rows, sig, n_contigs, max_gap, max_skip, min_sites, min_diff):
    """what a table holds: kept regions of two candidates or more, regions min_sites alone drops, regions min_diff alone drops"""
    raw = raw_regions(rows, sig, n_contigs, max_gap, max_skip)
    return {"kept2": sum(1 for r in raw if kept(r, min_sites, min_diff) and r["nsig"] >= 2),
            "by_min_sites": sum(1 for r in raw if r["nsig"] < min_sites and kept(r, 1, min_diff)),
            "by_min_diff": sum(1 for r in raw if abs(r["meth_diff"]) < min_diff and kept(r, min_sites, 0.0)),
            "raw": len(raw)}


PARAMS = {"max_gap": 300, "max_skip": 1, "min_sites": 2, "min_diff": 20.0}


def _draw(n, rng):
    """n rows over three contigs in stretches of 2 to 9 rows: of strong difference (either direction), of weak difference, of none;
    most rows of the first two kinds are significant, few of the last"""
    rows, sig = [], []
    contig, start = 0, rng.randint(0, 50)
    while len(rows) < n:
        kind = rng.choice(("up", "down", "weak", "none", "none"))
        if rng.random() < 0.04 and contig < 2 and len(rows) > n // 4:
            contig, start = contig + 1, rng.randint(0, 50)
        for _ in range(rng.randint(2, 9)):
            if len(rows) == n:
                break
            start += rng.randint(1, 120) if rng.random() < 0.93 else rng.randint(301, 900)
            na, nb = rng.randint(8, 40), rng.randint(8, 40)
            fa = rng.uniform(0.2, 0.6)
            fb = {"up": fa + rng.uniform(0.3, 0.4), "down": fa - rng.uniform(0.1, 0.2) - 0.1, "weak": fa + rng.uniform(0.04, 0.12), "none": fa}[kind]
            a, c = round(fa * na), max(0, round(fb * nb))
            if rng.random() < 0.03:
                na = a = 0                                  # no coverage in group A
            rows.append((contig, start, start + (2 if rng.random() < 0.5 else 1), a, na - a, c, nb - c))
            sig.append(rng.random() < (0.06 if kind == "none" else 0.85))
    return rows, sig


def table(n, seed=20261019):
    """(rows, sig) of n rows for PARAMS, the same for a size and a seed: the first draw that, by the rule alone, holds at least two kept
    regions of two candidates or more, one region that min_sites alone drops and one that min_diff alone drops.  A table of one row can
    hold none of these: it is one significant row of direction +1."""
    if n == 1:
        return [(1, 7, 9, 3, 9, 8, 2)], [True]
    for k in range(2000):
        rng = random.Random(seed * 10007 + n * 131 + k)
        rows, sig = _draw(n, rng)
        got = census(rows, sig, len(CONTIGS), **PARAMS)
        if got["kept2"] >= 2 and got["by_min_sites"] >= 1 and got["by_min_diff"] >= 1:
            return rows, sig
    raise AssertionError(f"no table of {n} rows holds every kind of region")


def site(contig, start, A, B):
    """a one-base row from (nmeth, nunmeth) of either group"""
    return (contig, start, start + 1, A[0], A[1], B[0], B[1])


UP, DOWN, FLAT, BARE = ((2, 8), (8, 2)), ((8, 2), (2, 8)), ((5, 5), (5, 5)), ((0, 0), (6, 4))
# (name, rows, sig, parameters, the regions by hand without their two doubles)
HAND = [
    ("three in a row", [site(0, 10, *UP), site(0, 20, *UP), site(0, 30, *UP)], [1, 1, 1], dict(max_gap=10, max_skip=0, min_sites=3, min_diff=0.0),
     [(0, 10, 31, 3, 3, 1, 6, 24, 24, 6)]),
    ("a gap of max_gap joins, one more breaks", [site(0, 10, *UP), site(0, 110, *UP), site(0, 211, *UP)], [1, 1, 1], dict(max_gap=100, max_skip=0, min_sites=1, min_diff=0.0),
     [(0, 10, 111, 2, 2, 1, 4, 16, 16, 4), (0, 211, 212, 1, 1, 1, 2, 8, 8, 2)]),
    ("max_skip rows between join, one more breaks", [site(0, 1, *DOWN), site(0, 2, *UP), site(0, 3, *DOWN), site(0, 4, *UP), site(0, 5, *UP), site(0, 6, *DOWN)],
     [1, 0, 1, 0, 0, 1], dict(max_gap=100, max_skip=1, min_sites=1, min_diff=0.0),
     [(0, 1, 4, 3, 2, -1, 18, 12, 12, 18), (0, 6, 7, 1, 1, -1, 8, 2, 2, 8)]),
    ("a contig change breaks", [site(0, 10, *UP), site(1, 11, *UP)], [1, 1], dict(max_gap=1000, max_skip=5, min_sites=1, min_diff=0.0),
     [(0, 10, 11, 1, 1, 1, 2, 8, 8, 2), (1, 11, 12, 1, 1, 1, 2, 8, 8, 2)]),
    ("a direction flip breaks", [site(0, 10, *UP), site(0, 11, *DOWN), site(0, 12, *DOWN)], [1, 1, 1], dict(max_gap=1000, max_skip=5, min_sites=1, min_diff=0.0),
     [(0, 10, 11, 1, 1, 1, 2, 8, 8, 2), (0, 11, 13, 2, 2, -1, 16, 4, 4, 16)]),
    ("a significant row without coverage is a skipped row", [site(0, 10, *UP), site(0, 11, *BARE), site(0, 12, *UP)], [1, 1, 1], dict(max_gap=1000, max_skip=0, min_sites=1, min_diff=0.0),
     [(0, 10, 11, 1, 1, 1, 2, 8, 8, 2), (0, 12, 13, 1, 1, 1, 2, 8, 8, 2)]),
    ("... and is summed where max_skip lets the chain pass it", [site(0, 10, *UP), site(0, 11, *BARE), site(0, 12, *UP)], [1, 1, 1], dict(max_gap=1000, max_skip=1, min_sites=2, min_diff=0.0),
     [(0, 10, 13, 3, 2, 1, 4, 16, 22, 8)]),
    ("a significant row of equal fractions is a skipped row", [site(0, 10, *DOWN), site(0, 11, *FLAT), site(0, 12, *DOWN)], [1, 1, 1], dict(max_gap=1000, max_skip=0, min_sites=1, min_diff=0.0),
     [(0, 10, 11, 1, 1, -1, 8, 2, 2, 8), (0, 12, 13, 1, 1, -1, 8, 2, 2, 8)]),
    ("min_sites drops the short one", [site(0, 10, *UP), site(0, 11, *UP), site(2, 5, *UP)], [1, 1, 1], dict(max_gap=10, max_skip=0, min_sites=2, min_diff=0.0),
     [(0, 10, 12, 2, 2, 1, 4, 16, 16, 4)]),
    ("min_diff drops the weak one", [site(0, 10, *UP), site(0, 500, (5, 5), (6, 4))], [1, 1], dict(max_gap=10, max_skip=0, min_sites=1, min_diff=10.5),
     [(0, 10, 11, 1, 1, 1, 2, 8, 8, 2)]),
    ("nothing significant", [site(0, 10, *UP), site(0, 11, *DOWN)], [0, 0], dict(max_gap=10, max_skip=0, min_sites=1, min_diff=0.0), []),
]
# Simpson's paradox: B is the more methylated at either site (10 % < 20 %, 80 % < 90 %); pooled, A is (81 / 110 > 29 / 110)
SIMPSON = [site(0, 100, (1, 9), (20, 80)), site(0, 101, (80, 20), (9, 1))]


def refusal_tables():
    """(name, rows, sig, bit, the row named): each refusal alone in the table of 513 rows, at row 300 and again behind it"""
    out = []
    for name, bit in (("unsorted", E_ORDER), ("equal twice", E_ORDER), ("contig out of range", E_CONTIG), ("negative", E_NEGATIVE), ("2^26", E_ENTRY), ("pooled margin", E_MARGIN)):
        rows, sig = table(513)
        rows, sig, first = [list(r) for r in rows], list(sig), 300
        for at in (300, 400, 512):
            if name == "unsorted":
                rows[at][0], rows[at][1] = rows[at - 1][0], rows[at - 1][1] - 1
            elif name == "equal twice":
                rows[at][0], rows[at][1] = rows[at - 1][0], rows[at - 1][1]
            elif name == "negative":
                rows[at][5] = -1
            elif name == "2^26":
                rows[at][4] = LIMIT
        if name == "contig out of range":
            for k in range(300, 513):                     # every row from 300 on: the contigs stay ascending, so the index is row 300's only refusal
                rows[k][0] = len(CONTIGS)
        if name == "pooled margin":
            # a chain of four rows from row 298, each entry below 2^26, group A's depth 2^26 together, apart from its neighbours; another from row 400
            for f in (298, 400):
                for k in range(f, f + 4):
                    rows[k] = [rows[f][0], rows[f][1] + (k - f), rows[f][1] + (k - f) + 1, LIMIT // 4 + 300 if k == f else LIMIT // 4 - 100, 0, 5, 5]
                    sig[k] = True
                sig[f - 2] = sig[f - 1] = sig[f + 4] = sig[f + 5] = False
            first = 298
        out.append((name, [tuple(r) for r in rows], sig, bit, first))
    return out
