"""What tests/test_regions_cpu.py and tests/test_gpu_regions.py share: the rule of Calls.regions restated in plain Python and numpy -- a loop
over the intervals and a mask over the rows, no search and no prefix --, and seeded interval sets over the tables of tests/merge_rule.py.
A row is (contig, start, end, nmeth, nunmeth, context, strand) and an interval (contig, start, end), half-open, everywhere."""
import functools

import numpy as np

from merge_rule import SIZES, table

CONTIGS = ("c0", "c1", "c2", "c3")            # table(n) has rows on c0 (n < 8) or c0..c2: c3 never has one
KS = (0, 1, 63, 64, 65, 257, 5003)            # intervals per set: around the 64 of a wavefront and the 256 of a workgroup, and many
SCAN_N = 256 * 4096 + 513                     # rows of a table whose block totals are more than one round of k_region_blocks (4096 entries): the carry
BIG = 2 ** 31 - 1
STRAND_MASK = {None: 7, "+": 1, "-": 2}
FILTERS = [(ctx, strand, depth) for ctx in (None, (0,), (1,), (2,)) for strand in (None, "+", "-") for depth in (0, 1, 5)]


def counted(cols, contexts=None, strand=None, min_depth=1):
    """the mask over the rows: which of them count"""
    _, _, _, m, u, ctx, s = cols
    ok = np.isin(ctx, (0, 1, 2) if contexts is None else contexts) & (m.astype(np.int64) + u.astype(np.int64) >= min_depth)
    if strand is not None:
        ok &= (s > 0) if strand == "+" else (s < 0)
    return ok


def members(cols, intervals):
    """per interval, the indices of the rows whose start lies inside it: a mask over all rows for each"""
    contig, start = cols[0], cols[1]
    return [np.nonzero((contig == c) & (start >= a) & (start < b))[0] for c, a, b in intervals]


def sums_of(cols, mem, ok):
    """(nsites, nmeth, nunmeth) per interval from its member rows and the mask of the rows that count"""
    m, u = cols[3].astype(np.int64), cols[4].astype(np.int64)
    return [(int(ok[i].sum()), int(m[i][ok[i]].sum()), int(u[i][ok[i]].sum())) for i in mem]


def region_sums(cols, intervals, contexts=None, strand=None, min_depth=1):
    """the rule: for every interval, in the intervals' order, the rows with the interval's contig and a start inside it that count"""
    return sums_of(cols, members(cols, intervals), counted(cols, contexts, strand, min_depth))


def intervals_over(cols, k, seed=3, n_contigs=len(CONTIGS)):
    """k intervals over the rows `cols`, all kinds together, shuffled, with duplicates: empty ones; a start on a row's start (inclusive)
    and an end on a row's start (exclusive); lo and hi inside one block of 256 rows; lo or hi on a row index that is a multiple of 256;
    two and more whole blocks spanned; whole contigs; before a contig's first row and after its last; a contig without rows; nested and
    overlapping pairs; sliding windows with step < width"""
    contig, start = cols[0], cols[1]
    n = len(contig)
    rng = np.random.default_rng(seed + 31 * n + k)
    out, whole, turn = [], 0, 0

    def row(i=None):
        i = int(rng.integers(0, n)) if i is None else min(i, n - 1)
        return i, int(contig[i]), int(start[i])

    def until(i, j):
        """row j, or the last row of row i's contig before it"""
        j = min(j, n - 1)
        while contig[j] != contig[i]:
            j -= 1
        return j

    while len(out) < k:
        kind, turn = (turn % 12 if k >= 12 else int(rng.integers(0, 12))), turn + 1
        if n == 0 or kind == 8:                                     # a contig without rows (with n == 0, every contig)
            c = n_contigs - 1 if n else int(rng.integers(0, n_contigs))
            a = int(rng.integers(0, 1000))
            out.append((c, a, a + int(rng.integers(0, 3)) * 500))
            continue
        i, c, s = row()
        w = int(rng.integers(1, 40))
        if kind == 0:
            out.append((c, s, s))                                   # empty
        elif kind == 1:
            out.append((c, s, s + w))                               # the row at `start` is inside
        elif kind == 2:
            out.append((c, max(0, s - w), s))                       # the row at `end` is outside
        elif kind == 3:                                             # inside one block
            j = until(i, i + int(rng.integers(0, 256 - i % 256)))
            out.append((c, s, int(start[j]) + int(rng.integers(0, 2))))
        elif kind == 4:                                             # lo or hi on a multiple of 256
            i, c, s = row(256 * int(rng.integers(0, n // 256 + 1)))
            j = until(i, i + int(rng.integers(0, 700)))
            out.append((c, s, int(start[j]) + 1) if rng.integers(0, 2) else (c, max(0, s - 10 * w), s))
        elif kind == 5:                                             # whole blocks between the ends
            j = until(i, i + 512 + int(rng.integers(0, 1200)))
            out.append((c, s, int(start[j])))
        elif kind == 6:
            if whole < 6:
                whole += 1
                out.append((int(rng.integers(0, n_contigs)), 0, BIG))
            else:
                out.append((c, s, s + 1))
        elif kind == 7:                                             # before the first row of the contig, after its last
            rows = np.nonzero(contig == c)[0]
            first, last = int(start[rows[0]]), int(start[rows[-1]])
            out.append((c, 0, first) if rng.integers(0, 2) else (c, last + 1, last + 1 + 100 * w))
        elif kind == 9:                                             # a nested pair
            out += [(c, s, s + 8 * w), (c, s + 2 * w, s + 6 * w)]
        elif kind == 10:                                            # an overlapping pair
            out += [(c, s, s + 8 * w), (c, s + 4 * w, s + 12 * w)]
        else:                                                       # sliding windows, step < width
            out += [(c, s + 7 * t, s + 7 * t + 20) for t in range(5)]
    out = out[:k]
    for _ in range(k // 16):                                        # duplicates
        out[int(rng.integers(0, k))] = out[int(rng.integers(0, k))]
    return tuple(out[i] for i in rng.permutation(k))


@functools.lru_cache(maxsize=None)
def intervals(n, k):
    """the seeded intervals over table(n)"""
    return intervals_over(table(n), k)


@functools.lru_cache(maxsize=None)
def scan_intervals():
    """over table(SCAN_N): a seeded set, and intervals whose lo, hi or both lie behind row 256 * 4096, where the prefix entries hold a carry"""
    contig, start = table(SCAN_N)[0], table(SCAN_N)[1]
    edge, c = 256 * 4096, int(contig[256 * 4096])
    assert contig[edge - 700] == c and contig[SCAN_N - 1] == c
    at = lambda i: int(start[i])
    return intervals(SCAN_N, 257) + ((c, at(edge - 700), at(edge + 300)), (c, at(edge + 10), at(SCAN_N - 1) + 1), (c, at(edge), at(edge + 256)), (c, at(edge - 256), at(edge)),
                                     (c, at(edge + 256), at(edge + 512)), (c, 0, BIG), (c, at(1000 * 256 + 7), at(edge + 257)))


@functools.lru_cache(maxsize=None)
def scan_expected(contexts=None, strand=None, min_depth=1):
    return tuple(region_sums(table(SCAN_N), scan_intervals(), contexts, strand, min_depth))


@functools.lru_cache(maxsize=None)
def _members(n, k):
    return members(table(n), intervals(n, k))


@functools.lru_cache(maxsize=None)
def _counted(n, contexts, strand, min_depth):
    return counted(table(n), contexts, strand, min_depth)


@functools.lru_cache(maxsize=None)
def expected(n, k, contexts=None, strand=None, min_depth=1):
    """the restatement over table(n) and intervals(n, k): the member rows found once per set, the mask once per filter, both shared"""
    return tuple(sums_of(table(n), _members(n, k), _counted(n, contexts, strand, min_depth)))


def covers(n, k):
    """which of the kinds the set really holds, by their ranges: (empty, within a block, lo on 256, hi on 256, two whole blocks, no rows)"""
    contig, start = table(n)[0], table(n)[1]
    key = contig.astype(np.int64) << 32 | start
    got = set()
    for c, a, b in intervals(n, k):
        lo, hi = int(np.searchsorted(key, c << 32 | a)), int(np.searchsorted(key, c << 32 | b))
        if a == b:
            got.add("empty")
        if lo == hi and a < b:
            got.add("no rows")
        if lo < hi and lo // 256 == (hi - 1) // 256 and lo % 256 and hi % 256:
            got.add("one block")
        if lo < hi and lo % 256 == 0:
            got.add("lo on 256")
        if lo < hi and hi % 256 == 0:
            got.add("hi on 256")
        if hi // 256 - (lo + 255) // 256 >= 2:
            got.add("whole blocks")
    return got


# what is refused: (the name region_emu prints, rows, intervals)
GOOD = [(0, 10, 11, 1, 1, 2, 1), (0, 20, 21, 1, 1, 2, 1)]
ERRORS = [
    ("order", [(0, 10, 11, 1, 1, 2, 1), (0, 10, 11, 1, 1, 2, 1)], [(0, 0, 100)]), ("order", [(0, 10, 11, 1, 1, 2, 1), (0, 9, 10, 1, 1, 2, 1)], [(0, 0, 100)]),
    ("order", [(1, 10, 11, 1, 1, 2, 1), (0, 20, 21, 1, 1, 2, 1)], [(0, 0, 100)]),
    ("contig", [(2, 10, 11, 1, 1, 0, 1)], [(0, 0, 100)]), ("contig", [(-1, 10, 11, 1, 1, 2, 1)], [(0, 0, 100)]),
    ("context", [(0, 10, 11, 1, 1, 3, 1)], [(0, 0, 100)]),
    ("iv_contig", GOOD, [(0, 0, 100), (2, 0, 100)]), ("iv_contig", GOOD, [(-1, 0, 100)]),
    ("iv_range", GOOD, [(0, -1, 100)]), ("iv_range", GOOD, [(0, 0, 100), (1, 50, 49)]),
]
MESSAGES = {"order": "not ascending", "contig": "row's contig", "context": "row's context", "iv_contig": "interval's contig", "iv_range": "start < 0 or end < start"}      # of the library
