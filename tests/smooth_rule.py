"""The smoothing rule of csrc/mdk_smooth_core.h restated in Python floats, independently of the header's formulation by runs: d_k comes
from SORTED distances, and a window from a SCAN outwards from its site.  Python's floats are IEEE doubles and nothing
here is fused, so the bits are the header's."""
import struct

TRICUBE, FLAT = 0, 1
KERNELS = {"tricube": TRICUBE, "flat": FLAT}
E_ORDER, E_POSITION, E_NEGATIVE, E_ENTRY = 1, 2, 4, 8
LIMIT = 1 << 26
NAN_BITS = 0x7FF8000000000000


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def refusal(contig, start, nmeth, nunmeth):
    """(bit, site) of the refusal that is reported -- the smallest refused site, and of its bits the lowest --, or None"""
    for i in range(len(start)):
        err = 0
        if i and not (contig[i - 1], start[i - 1]) < (contig[i], start[i]):
            err |= E_ORDER
        if contig[i] < 0 or start[i] < 0:
            err |= E_POSITION
        for m, u in zip(nmeth, nunmeth):
            for v in (m[i], u[i]):
                if v < 0:
                    err |= E_NEGATIVE
                elif v >= LIMIT:
                    err |= E_ENTRY
        if err:
            return err & -err, i
    return None


def windows(contig, start, half_bases, min_sites):
    """[(lo, hi, half)] of every site of a valid table.  The rows ascend, so the k nearest sites of a contig lie among the k - 1 rows to
    either side: their distances are sorted for d_k; then the window is scanned outwards from the site"""
    n = len(start)
    first, last = {}, {}
    for j in range(n):
        first.setdefault(contig[j], j)
        last[contig[j]] = j
    out = []
    for i in range(n):
        c0, c1 = first[contig[i]], last[contig[i]] + 1
        k = min(min_sites, c1 - c0)
        dk = sorted(abs(start[j] - start[i]) for j in range(max(c0, i - k + 1), min(c1, i + k)))[k - 1]
        half = max(half_bases, dk)
        lo, hi = i, i + 1
        while lo > c0 and start[i] - start[lo - 1] <= half:
            lo -= 1
        while hi < c1 and start[hi] - start[i] <= half:
            hi += 1
        out.append((lo, hi, half))
    return out


def weight(kernel, d, half):
    if kernel == FLAT or half == 0:
        return 1.0
    if d >= half:
        return 0.0
    inv = 1.0 / float(half)
    r = float(d) * inv
    c = (r * r) * r
    t = 1.0 - c
    return (t * t) * t


def smooth(contig, start, nmeth, nunmeth, half_bases, min_sites, kernel, win=None):
    """(level, depth, nsites, half): level and depth lists per sample of the 64-bit PATTERNS of the doubles, nsites and half lists of
    ints; ``win``: what ``windows`` gave for the same table and parameters, if the caller has it"""
    if win is None:
        win = windows(contig, start, half_bases, min_sites)
    level, depth = [], []
    for m, u in zip(nmeth, nunmeth):
        lv, dp = [], []
        for i, (lo, hi, half) in enumerate(win):
            M = D = 0.0
            for j in range(lo, hi):
                w = weight(kernel, abs(start[j] - start[i]), half)
                M = M + w * float(m[j])
                D = D + w * float(m[j] + u[j])
            lv.append(bits(M / D) if D > 0.0 else NAN_BITS)
            dp.append(bits(D))
        level.append(lv)
        depth.append(dp)
    return level, depth, [hi - lo for lo, hi, _ in win], [h for _, _, h in win]
