"""What tests/test_unite_cpu.py and tests/test_gpu_unite.py share: the rule of mdk.unite restated in plain Python -- a dict keyed by
(contig, start), no bitmap and no rank --, seeded samples cut from the tables of tests/merge_rule.py, the cases made by hand and what is
refused.  A row is (contig, start, end, nmeth, nunmeth, context, strand); a united row is (contig, start, end, context, strand, nsamples,
(nmeth, nunmeth) of sample 0, of sample 1, ...)."""
import functools

import numpy as np

from merge_rule import DTYPES, SIZES, table

CONTIGS = ("c0", "c1", "c2", "c3")            # table(n) has rows on c0 (n < 8) or c0..c2: c3 never has one
BIG = 2 ** 31 - 1
BLOCK_WORDS, SCAN, ROWS = 16, 1024, 256       # csrc/mdk_unite_core.h: words per entry of the bitmap's block table, entries of a round of k_unite_blocks, sites per entry of the sites' block table


class Disagree(Exception):
    pass


def unite_rows(samples, min_samples=None, min_depth=1):
    """the rule: a sample holds (contig, start) if it has a row there with nmeth + nunmeth >= min_depth; the sites at least min_samples
    samples hold, ascending; the samples that hold a kept site must give the same end, context and strand"""
    S = len(samples)
    min_samples = S if min_samples is None else min_samples
    sites = {}
    for s, rows in enumerate(samples):
        for c, p, e, m, u, t, strand in rows:
            if m + u >= min_depth:
                sites.setdefault((c, p), []).append((s, (e, t, strand), (m, u)))
    out = []
    for c, p in sorted(sites):
        held = sites[c, p]
        if len(held) < min_samples:
            continue
        if any(h[1] != held[0][1] for h in held):
            raise Disagree((c, p))
        counts = [(0, 0)] * S
        for s, _, mu in held:
            counts[s] = mu
        out.append((c, p) + held[0][1] + (len(held),) + tuple(counts))
    return out


@functools.lru_cache(maxsize=None)
def sample(n, s):
    """sample s of universe n, as numpy columns: the rows of table(n) kept with probability 0.7, their counts drawn anew from 0..9 --
    one reference, so the samples agree about every site, and `0 0` rows among them"""
    cols = table(n)
    rng = np.random.default_rng(1000 + 17 * s + n)
    keep = rng.random(n) < 0.7
    m, u = rng.integers(0, 10, n), rng.integers(0, 10, n)
    out = [c[keep] for c in cols]
    out[3], out[4] = m[keep].astype(DTYPES[3]), u[keep].astype(DTYPES[4])
    for c in out:
        c.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def sample_rows(n, s):
    return tuple(zip(*[c.tolist() for c in sample(n, s)]))


@functools.lru_cache(maxsize=None)
def _union(n, S, min_depth):
    return tuple(unite_rows([sample_rows(n, s) for s in range(S)], 1, min_depth))


@functools.lru_cache(maxsize=None)
def expected(n, S, min_samples, min_depth):
    """the restatement over samples 0 .. S - 1 of universe n: the dict is built once per (n, S, min_depth) and shared -- the sites at
    least min_samples samples hold are the union's rows with nsamples >= min_samples (the samples are cut from one table: none disagree)"""
    return tuple(r for r in _union(n, S, min_depth) if r[5] >= min_samples)


def combos(n):
    """(S, min_samples, min_depth) for universe n: S in 1, 2, 3, 5, min_samples in 1, 2, S, min_depth in 0, 1, 5; thinned out at 300001,
    where a run parses or uploads a million rows"""
    if n > 1000:
        return [(3, 1, 1), (3, 3, 5), (2, 2, 0)]
    return [(S, k, d) for S in (1, 2, 3, 5) for k in sorted({1, min(2, S), S}) for d in (0, 1, 5)]


def rounds(samples, n_union):
    """the rounds k_unite_blocks takes over the block table of the bitmap's words and over that of the union's sites, from the samples'
    extents: per contig the largest start + 1 of any row, in whole words"""
    top = {}
    for rows in samples:
        for r in rows:
            top[r[0]] = max(top.get(r[0], 0), r[1] + 1)
    words = sum((x + 31) // 32 for x in top.values())
    up = lambda a, b: (a + b - 1) // b
    return up(up(words, BLOCK_WORDS), SCAN), up(up(n_union, ROWS), SCAN)


# ---- by hand: (name, samples, keyword arguments); every case is run as it is and compared with unite_rows ----
def _site(c, p, m=1, u=1, t=2, strand=1):
    return (c, p, p + 1, m, u, t, strand)


_EDGES = sorted({(1 << k) + d for k in range(5, 17) for d in (-1, 0, 1)})        # both sides of every power of two: word, block and round edges of the bitmap
_FULL = [_site(0, p, 1 + p % 7, p % 5) for p in _EDGES]
HAND = [
    ("powers of two, union", [_FULL, _FULL[::2], [r for r in _FULL if r[1] & (r[1] - 1) == 0]], {"min_samples": 1}),
    ("powers of two, two of three", [_FULL, _FULL[::2], [r for r in _FULL if r[1] & (r[1] - 1) == 0]], {"min_samples": 2}),
    ("powers of two, all", [_FULL, _FULL[::2], [r for r in _FULL if r[1] & (r[1] - 1) == 0]], {}),
    ("a contig no sample touches between two that have rows", [[_site(0, 5), _site(2, 7)], [_site(0, 5), _site(2, 7), _site(2, 9)]], {"min_samples": 1}),
    ("a contig only one sample touches", [[_site(0, 5), _site(1, 3), _site(1, 64), _site(2, 7)], [_site(0, 5), _site(2, 7)]], {"min_samples": 1}),
    ("a contig only one sample touches, all", [[_site(0, 5), _site(1, 3), _site(1, 64), _site(2, 7)], [_site(0, 5), _site(2, 7)]], {}),
    ("an empty sample among full ones, union", [_FULL[:9], [], _FULL[:9]], {"min_samples": 1}),
    ("an empty sample among full ones, two", [_FULL[:9], [], _FULL[:9]], {"min_samples": 2}),
    ("an empty sample among full ones, all", [_FULL[:9], [], _FULL[:9]], {}),
    ("all samples empty", [[], [], []], {"min_samples": 1}),
    ("one empty sample", [[]], {}),
    ("rows, none of them present", [[_site(0, 5, 0, 0)], [_site(0, 6, 0, 0)]], {"min_samples": 1}),
    ("0 0 rows kept at depth 0", [[_site(0, 5, 0, 0)], [_site(0, 5, 0, 0), _site(0, 6, 0, 0)]], {"min_samples": 1, "min_depth": 0}),
    ("identical samples", [_FULL, _FULL, _FULL, _FULL], {}),
    ("disjoint samples, union", [_FULL[::2], _FULL[1::2]], {"min_samples": 1}),
    ("disjoint samples, all", [_FULL[::2], _FULL[1::2]], {}),
    ("merged rows", [[(0, 10, 12, 3, 4, 0, 0), (1, 0, 3, 1, 1, 1, 0)], [(0, 10, 12, 5, 6, 0, 0), (0, 40, 41, 1, 0, 2, -1)]], {"min_samples": 1}),
    ("counts of INT32_MAX at that depth", [[_site(0, 5, BIG, BIG), _site(0, 6, BIG, 0), _site(0, 7, BIG - 1, 0)], [_site(0, 5, 0, BIG), _site(0, 7, 1, BIG - 1)]], {"min_samples": 1, "min_depth": BIG}),
]
# bit offsets pass 2^32 (a word index does not): 2 x 2^26 + 1 words, half a GiB of bitmap and as much of ranks
FAR = ("three contigs, rows at 2^31 - 2, 2^31 - 2 and 5", [[_site(0, BIG - 1), _site(1, BIG - 1, 2, 3), _site(2, 5)], [_site(0, 7), _site(1, BIG - 1, 4, 5), _site(2, 5)]], {"min_samples": 1})

# ---- what is refused: (the name unite_emu prints, samples, keyword arguments) ----
_A, _B = _site(0, 10, t=0), _site(0, 20, t=1, strand=-1)
_PAD = [_site(0, k) for k in range(255)]


def _odd(which, where):
    """three samples that hold (0, 10) and (0, 20); in sample `where`, column `which` of the second site is another"""
    bad = list(_B)
    bad[which] = {2: 22, 5: 2, 6: 1}[which]
    return [[_A, tuple(bad)] if s == where else [_A, _B] for s in range(3)]


ERRORS = [
    ("order", [[_A, _B], [_B, _A]], {}), ("order", [[_A, _A]], {}), ("order", [[_site(1, 5), _site(0, 9)]], {}),
    ("order", [[_A], _PAD + [_site(0, 300), _site(0, 300)]], {"min_samples": 1}),             # row 256 looks at row 255: another wavefront's, from the table
    ("contig", [[_A], [_site(2, 5)]], {"min_samples": 1}), ("contig", [[_site(-1, 5)]], {}),
    ("context", [[_A], [_site(0, 5, t=3)]], {"min_samples": 1}),
    ("context", [_PAD + [_site(0, 300), _site(0, 301, t=3)]], {}),
    ("start", [[_site(0, -1), _A]], {}),
] + [("disagree", _odd(which, where), {"min_samples": k}) for which in (2, 5, 6) for where in (0, 2) for k in (1, 3)] + [
    ("extent", [[_site(c, BIG - 1) for c in range(33)], [_site(0, 5)]], {"min_samples": 1}),  # 33 x 2^26 words: past 2^35 bits, refused before the bitmap is allocated
]
ERROR_CONTIGS = {"extent": 33}                # the contig names a case needs (default 2)
MESSAGES = {"order": "not ascending", "contig": "row's contig", "context": "row's context", "start": "start is negative",
            "disagree": "samples disagree about a site", "extent": r"more than 2\^35 bits"}      # of the library
