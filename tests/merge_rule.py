"""What tests/test_merge_cpu.py and tests/test_gpu_merge.py share: the mergeContext rule restated in plain Python, and seeded per-strand
tables cut from random references.  A row is (contig, start, end, nmeth, nunmeth, context, strand) everywhere."""
import functools

import numpy as np

SIZES = (0, 1, 2, 255, 256, 257, 513, 300001)        # rows; 300,001 is more than 256 x 1024: the scan of the block table takes a second round
COLUMNS = ("contig", "start", "end", "nmeth", "nunmeth", "context", "strand")
DTYPES = ("int32", "int32", "int32", "int32", "int32", "uint8", "int8")


def merge_rows(rows, min_depth=1):
    """the rule, row by row: a CpG / CHG C takes the G of its site if that is the next row, a G whose C is the row before gives nothing, any
    other C or G is its site alone; CHH rows pass; then the depth cut"""
    out = []
    for i, (c, p, e, m, u, t, s) in enumerate(rows):
        if t == 2:
            row = (c, p, e, m, u, t, s)
        else:
            d = t + 1
            if s > 0:
                nxt = rows[i + 1] if i + 1 < len(rows) else None
                if nxt is not None and nxt[0] == c and nxt[5] == t and nxt[6] < 0 and nxt[1] == p + d:
                    m, u = m + nxt[3], u + nxt[4]
                row = (c, p, p + d + 1, m, u, t, 0)
            else:
                prv = rows[i - 1] if i > 0 else None
                if prv is not None and prv[0] == c and prv[5] == t and prv[6] > 0 and prv[1] == p - d:
                    continue
                row = (c, p - d, p + 1, m, u, t, 0)
        if row[3] + row[4] >= min_depth:
            out.append(row)
    return out


def pairs(rows):
    """the indices i whose row is a C merged with row i + 1"""
    return [i for i in range(len(rows) - 1)
            if rows[i][5] < 2 and rows[i][6] > 0 and rows[i + 1][6] < 0 and rows[i + 1][0] == rows[i][0] and rows[i + 1][5] == rows[i][5] and rows[i + 1][1] == rows[i][1] + rows[i][5] + 1]


def classify(seq):
    """context (0 CpG, 1 CHG, 2 CHH) and strand (+1 C, -1 G, 0 neither) of every base of an uppercase ACGT uint8 array, by the reference's
    isCpG / isCHG / isCHH (common.c:49-82): a C looks one and two bases ahead, a G one and two bases back, all inside the contig"""
    n = len(seq)
    isc, isg = seq == ord("C"), seq == ord("G")
    nxt1 = np.zeros(n, bool); nxt1[:-1] = isg[1:]
    nxt2 = np.zeros(n, bool); nxt2[:-2] = isg[2:]
    prv1 = np.zeros(n, bool); prv1[1:] = isc[:-1]
    prv2 = np.zeros(n, bool); prv2[2:] = isc[:-2]
    ctx = np.where(isc, np.where(nxt1, 0, np.where(nxt2, 1, 2)), np.where(prv1, 0, np.where(prv2, 1, 2)))
    return ctx, isc.astype(np.int64) - isg.astype(np.int64)


@functools.lru_cache(maxsize=None)
def table(n, seed=7):
    """n rows (numpy columns, in COLUMNS order) of three contigs: random ACGT, every C and G classified, about 30 % of the rows dropped --
    lone Cs and lone Gs --, counts 0..9.  Contig k ends in CG with only the C kept as its last row, and contig k + 1 holds CG at the same
    offsets with the G as its FIRST row: a G at start + d right behind a C, in another contig.  The table is the first n rows of that."""
    rng = np.random.default_rng(seed + n)
    if n < 8:
        lens = [6 * n + 16]
    else:
        l0 = max(8, n); lens = [l0, l0 + n, 6 * n + 64]
    cols = [[] for _ in COLUMNS]
    for k, ln in enumerate(lens):
        seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), ln)
        keep = rng.random(ln) >= 0.3
        if len(lens) > 1:
            if k + 1 < len(lens):
                seq[ln - 3:ln] = np.frombuffer(b"ACG", dtype=np.uint8); keep[ln - 2] = True; keep[ln - 1] = False
            if k > 0:
                e = lens[k - 1]
                seq[e - 3:e] = np.frombuffer(b"ACG", dtype=np.uint8); keep[:e - 1] = False; keep[e - 1] = True
        ctx, strand = classify(seq)
        pos = np.nonzero(keep & (strand != 0))[0]
        m = rng.integers(0, 10, len(pos)); u = rng.integers(0, 10, len(pos))
        for col, v in zip(cols, (np.full(len(pos), k), pos, pos + 1, m, u, ctx[pos], strand[pos])):
            col.append(v)
    cols = [np.concatenate(c)[:n].astype(dt) for c, dt in zip(cols, DTYPES)]
    assert len(cols[0]) == n, (n, len(cols[0]))
    for c in cols:
        c.setflags(write=False)
    return tuple(cols)


@functools.lru_cache(maxsize=None)
def table_rows(n):
    return tuple(zip(*[c.tolist() for c in table(n)]))


@functools.lru_cache(maxsize=None)
def expected(n, min_depth):
    """the restatement over table(n): computed once, shared by the tests"""
    return tuple(merge_rows(table_rows(n), min_depth))


def crosses_contigs(rows):
    """is there a C that ends a contig with the first row of the next contig a G of its context at start + d?"""
    return any(a[0] != b[0] and a[5] < 2 and a[6] > 0 and b[6] < 0 and b[5] == a[5] and b[1] == a[1] + a[5] + 1 for a, b in zip(rows, rows[1:]))


# what is refused: (the name merge_emu prints, a table that holds only that fault)
BIG = 2 ** 31 - 1
ERRORS = [
    ("merged", [(0, 10, 11, 1, 1, 0, 0)]), ("merged", [(0, 10, 12, 1, 1, 0, 1)]), ("merged", [(0, 10, 13, 1, 1, 2, 1)]),
    ("context", [(0, 10, 11, 1, 1, 3, 1)]),
    ("contig", [(2, 10, 11, 1, 1, 0, 1)]), ("contig", [(-1, 10, 11, 1, 1, 2, 1)]),
    ("order", [(0, 10, 11, 1, 1, 2, 1), (0, 10, 11, 1, 1, 2, 1)]), ("order", [(0, 10, 11, 1, 1, 2, 1), (0, 9, 10, 1, 1, 2, 1)]), ("order", [(1, 10, 11, 1, 1, 2, 1), (0, 20, 21, 1, 1, 2, 1)]),
    ("lone_g", [(0, 0, 1, 1, 1, 0, -1)]), ("lone_g", [(0, 1, 2, 1, 1, 1, -1)]),
    ("sum", [(0, 10, 11, BIG, 0, 0, 1), (0, 11, 12, 1, 0, 0, -1)]), ("sum", [(0, 10, 11, 0, BIG - 1, 1, 1), (0, 12, 13, 0, 2, 1, -1)]),
]
MESSAGES = {"merged": "merged already", "context": "context", "contig": "contig", "order": "not ascending", "lone_g": "G without its C", "sum": "INT32_MAX"}      # of the library
