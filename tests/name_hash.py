"""TEST INFRASTRUCTURE: the read-name hash of the device preparation (scan_record in csrc/mdk_prep.hip), restated in Python integers,
and names that collide under it.

The chunk's name table (k_prep_scan, table_insert) knows a name by the high 32 bits of its hash and files it at slot `hash & hmask`;
two names that agree in both are linked into ONE chain, and only same_name in k_prep_segs tells them apart.  The pairs below agree in
`h >> 32` and in the low 12 bits of h, so they share an entry in every table of up to 4096 entries (a chunk of up to ~3270 records).
They were found with find_collisions() -- a birthday search, not called by any test -- and are kept as literals;
tests/test_name_hash_cpu.py holds them against the restatement, and the probe of tests/test_gpu_prep_cases.py holds the restatement
against the device."""
import numpy as np

M64 = (1 << 64) - 1
SEED, MUL_WORD, MUL_LEN = 0x9e3779b97f4a7c15, 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53
LOW_BITS = 12                      # the pairs share a home slot in tables of up to 1 << LOW_BITS entries


def name_hash(name) -> int:
    """the hash of a read name as strcmp sees it: its letters up to the first NUL"""
    b = name.encode() if isinstance(name, str) else bytes(name)
    b = b.split(b"\0")[0]
    h = SEED
    for o in range(0, len(b), 16):                 # 16-byte blocks, zero padded; a block with fewer than 16 letters is the last one
        blk = b[o:o + 16].ljust(16, b"\0")
        for d in range(4):
            w = int.from_bytes(blk[4 * d:4 * d + 4], "little")
            h = ((h ^ w) * MUL_WORD) & M64
            h ^= h >> 29
    h = ((h ^ len(b)) * MUL_LEN) & M64
    h ^= h >> 32
    return h or 1


def table_key(name) -> int:
    """what an entry of the name table keeps of the name"""
    return name_hash(name) >> 32


def home_slot(name, hmask: int) -> int:
    return name_hash(name) & hmask


def collide(a, b, low_bits: int = LOW_BITS) -> bool:
    """a and b are one name to the table: same key, same home slot in every table of up to 1 << low_bits entries"""
    ha, hb = name_hash(a), name_hash(b)
    return a != b and ha >> 32 == hb >> 32 and (ha ^ hb) & ((1 << low_bits) - 1) == 0


def unrelated(a, b, low_bits: int = LOW_BITS) -> bool:
    """a and b agree neither in the key nor in the home slot"""
    ha, hb = name_hash(a), name_hash(b)
    return ha >> 32 != hb >> 32 and (ha ^ hb) & ((1 << low_bits) - 1) != 0


# (name, name, control): the two names collide, the control is unrelated to both
SHORT_PAIRS = [                    # 16 letters or fewer: the names differ in the PrepRead's first block
    ("rdHEEGIAAA", "rd7TXCLAAA", "rdCTL00000"),
    ("rdTE6RPAAA", "rdH45HQAAA", "rdCTL00001"),
    ("rdLB2XIAAA", "rdHKPARAAA", "rdCTL00002"),
    ("rdUYS4FAAA", "rdMUNROAAA", "rdCTL00003"),
    ("rdHTFKFAAA", "rdWQFKHAAA", "rdCTL00004"),
    ("rdR2C7CAAA", "rdEEYGRAAA", "rdCTL00005"),
]
TAIL_PAIRS = [                     # 24 letters, equal in the first 16 and in length: only same_name's tail loop tells them apart
    ("HWI-ST1234:C0ABCSU5PEAAA", "HWI-ST1234:C0ABCCHCLGAAA", "HWI-ST1234:C0ABCCTL00000"),
    ("HWI-ST1234:C0ABCCBRVMAAA", "HWI-ST1234:C0ABCBUGZUAAA", "HWI-ST1234:C0ABCCTL00001"),
    ("HWI-ST1234:C0ABCVHSIEAAA", "HWI-ST1234:C0ABC3YI2WAAA", "HWI-ST1234:C0ABCCTL00002"),
    ("HWI-ST1234:C0ABCMAKVNAAA", "HWI-ST1234:C0ABCBQ6VQAAA", "HWI-ST1234:C0ABCCTL00003"),
]
LENGTH_PAIRS = [                   # equal in the first 16 letters, unequal in length (23 and 24)
    ("A00123:45:HXYZ7:XJF6AAA", "A00123:45:HXYZ7:KJ4JKAAA", "A00123:45:HXYZ7:CTL00000"),
    ("A00123:45:HXYZ7:UFUFMAA", "A00123:45:HXYZ7:GYSAOAAA", "A00123:45:HXYZ7:CTL00001"),
    ("A00123:45:HXYZ7:QEKUNAAA", "A00123:45:HXYZ7:4WF67AA", "A00123:45:HXYZ7:CTL00002"),
    ("A00123:45:HXYZ7:7PO5YAAA", "A00123:45:HXYZ7:7VUY6AA", "A00123:45:HXYZ7:CTL00003"),
]
ALL_PAIRS = SHORT_PAIRS + TAIL_PAIRS + LENGTH_PAIRS

ALPHABET = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ234567", dtype=np.uint8)


def _hash_rows(rows: np.ndarray, nlen: int) -> np.ndarray:
    """name_hash of every row of an (n, 16 k) uint8 array holding names of nlen letters, zero padded"""
    words = np.ascontiguousarray(rows).view("<u4").astype(np.uint64)
    h = np.full(rows.shape[0], SEED, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for d in range(4 * ((nlen + 15) // 16)):
            h = (h ^ words[:, d]) * np.uint64(MUL_WORD)
            h ^= h >> np.uint64(29)
        h = (h ^ np.uint64(nlen)) * np.uint64(MUL_LEN)
        h ^= h >> np.uint64(32)
    h[h == 0] = 1
    return h


def _names(prefix: bytes, slen: int, first: int, n: int) -> np.ndarray:
    """n names prefix + slen letters that spell the numbers first, first + 1, ... in base 32; zero padded to whole blocks"""
    nlen = len(prefix) + slen
    rows = np.zeros((n, 16 * ((nlen + 15) // 16)), dtype=np.uint8)
    rows[:, :len(prefix)] = np.frombuffer(prefix, dtype=np.uint8)
    idx = np.arange(first, first + n, dtype=np.uint64)
    for j in range(slen):
        rows[:, len(prefix) + j] = ALPHABET[((idx >> np.uint64(5 * j)) & np.uint64(31)).astype(np.intp)]
    return rows


def find_collisions(prefix: str, suffix_lens=(8,), n_names: int = 24_000_000, low_bits: int = LOW_BITS, batch: int = 2_000_000):
    """Birthday search: n_names names `prefix` + a base-32 counter, the batches taking the suffix lengths in turn; returns the pairs that
    collide(), as strings.  32 + low_bits bits agree by chance in about n_names^2 / 2^(33 + low_bits) pairs: 24 million names give
    some sixteen 44-bit pairs in about ten seconds and 1 GB.  A prefix of 16 letters and suffixes of one length give TAIL_PAIRS' kind, of
    several lengths (pick the pairs of unequal length) LENGTH_PAIRS'."""
    p = prefix.encode()
    keys, origin = [], []
    for k, first in enumerate(range(0, n_names, batch)):
        slen, n = suffix_lens[k % len(suffix_lens)], min(batch, n_names - first)
        h = _hash_rows(_names(p, slen, first, n), len(p) + slen)
        keys.append((h >> np.uint64(32)) << np.uint64(low_bits) | (h & np.uint64((1 << low_bits) - 1)))
        origin.append((slen, first))
    keys = np.concatenate(keys)
    order = np.argsort(keys, kind="stable")
    srt = keys[order]
    out = []
    for at in np.nonzero(srt[1:] == srt[:-1])[0]:
        pair = []
        for g in (int(order[at]), int(order[at + 1])):
            slen, first = origin[g // batch]
            pair.append(bytes(_names(p, slen, g, 1)[0, :len(p) + slen]).decode())
        if collide(pair[0], pair[1], low_bits):
            out.append(tuple(pair))
    return out
