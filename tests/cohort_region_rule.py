"""What tests/test_cohort_regions_cpu.py and tests/test_gpu_cohort_regions.py share: seeded [S, n] count matrices over the site columns of
merge_rule.table(n), and the cells Cohort.regions must give for them -- region_rule.region_sums per sample, with the member rows of an
interval set found once per set and shared (region_rule._members), as region_rule.expected shares them (see sample_expected).  Sample 0 holds the table's own
counts, sample 1 is all `0 0`, and every later sample holds seeded counts with about half its cells `0 0`, so that min_depth cuts
differently per sample.  A sample's counts depend on (n, s) alone: the first S samples of a larger table are the smaller table."""
import functools

import numpy as np

from merge_rule import table
from region_rule import BIG, _members, counted

CONTEXT_MASK = lambda contexts: 7 if contexts is None else sum(1 << t for t in contexts)


@functools.lru_cache(maxsize=None)
def sample_counts(n, s):
    """(nmeth, nunmeth) of sample s over table(n): int32, read-only"""
    cols = table(n)
    if s == 0:
        return cols[3], cols[4]
    if s == 1:
        m, u = np.zeros(n, np.int32), np.zeros(n, np.int32)
    else:
        rng = np.random.default_rng(1000 * s + n)
        held = rng.random(n) < 0.5
        m, u = (rng.integers(0, 12, n) * held).astype(np.int32), (rng.integers(0, 12, n) * held).astype(np.int32)
    m.setflags(write=False); u.setflags(write=False)
    return m, u


def sample_cols(n, s):
    """the seven columns of sample s as region_rule takes them"""
    cols = table(n)
    m, u = sample_counts(n, s)
    return cols[:3] + (m, u) + cols[5:]


def matrices(n, S):
    """nmeth and nunmeth, int32 [S, n]"""
    pairs = [sample_counts(n, s) for s in range(S)]
    return np.stack([p[0] for p in pairs]).reshape(S, n), np.stack([p[1] for p in pairs]).reshape(S, n)


@functools.lru_cache(maxsize=None)
def _flat_members(n, k):
    """region_rule._members(n, k) laid end to end: (the row indices, where each interval's begin, where they end)"""
    mem = _members(n, k)
    ends = np.cumsum([len(i) for i in mem], dtype=np.int64) if mem else np.zeros(0, np.int64)
    return (np.concatenate(mem) if mem else np.zeros(0, np.int64)), ends - np.array([len(i) for i in mem], dtype=np.int64), ends


@functools.lru_cache(maxsize=None)
def sample_expected(n, s, k, contexts=None, strand=None, min_depth=1):
    """region_sums of sample s over intervals(n, k) as three int64 arrays of k entries (nsites, nmeth, nunmeth): region_rule's member rows
    and region_rule's mask of the rows that count, as in region_sums; only sums_of's Python loop over the intervals is taken as one
    running sum over the members laid end to end, which is exact in int64.  tests/test_cohort_regions_cpu.py holds this against
    region_sums itself"""
    cols = sample_cols(n, s)
    ok = counted(cols, contexts, strand, min_depth)
    idx, begins, ends = _flat_members(n, k)
    out = []
    for v in (ok.astype(np.int64), cols[3].astype(np.int64) * ok, cols[4].astype(np.int64) * ok):
        run = np.concatenate([np.zeros(1, np.int64), np.cumsum(v[idx], dtype=np.int64)])
        out.append(run[ends] - run[begins])
    return tuple(out)


def expected(n, S, k, contexts=None, strand=None, min_depth=1):
    """the three [S, k] matrices as int64 numpy arrays: (nsites, nmeth, nunmeth)"""
    per = [sample_expected(n, s, k, contexts, strand, min_depth) for s in range(S)]
    return tuple(np.stack([row[w] for row in per]).reshape(S, k) for w in range(3))


@functools.lru_cache(maxsize=None)
def sites_text(n, S):
    """the table as tools/cregion_emu reads it: contig start context strand m0 u0 m1 u1 ..."""
    cols = table(n)
    m, u = matrices(n, S)
    parts = [cols[0], cols[1], cols[5], cols[6]] + [x for s in range(S) for x in (m[s], u[s])]
    return "".join("\t".join(map(str, row)) + "\n" for row in zip(*[p.tolist() for p in parts]))


# three rows of INT32_MAX counts in two samples (and a third of small ones): the sums of (0, 0, 3) pass 2^32
BIG_ROWS = [(0, k, k + 1, 0, 1) for k in range(3)]                                   # contig, start, end, context, strand
BIG_COUNTS = ([[BIG] * 3, [BIG, 0, BIG], [1, 2, 3]], [[BIG] * 3, [BIG] * 3, [0, 0, 0]])        # nmeth, nunmeth: [S, n]
BIG_INTERVALS = [(0, 0, 3), (0, 1, 2), (0, 3, 9)]
BIG_DEPTH = BIG


def big_expected():
    """region_sums per sample over the INT32_MAX table, as `expected` lays the cells out"""
    from merge_rule import DTYPES
    from region_rule import region_sums
    site = list(zip(*BIG_ROWS))
    per = [region_sums([np.array(c, dtype=dt) for c, dt in zip(site[:3] + [BIG_COUNTS[0][s], BIG_COUNTS[1][s]] + site[3:], DTYPES)], BIG_INTERVALS, None, None, BIG_DEPTH)
           for s in range(3)]
    return tuple(np.array([[cell[w] for cell in row] for row in per], dtype=np.int64) for w in range(3))
