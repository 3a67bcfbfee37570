"""Wall clock of Diff.dmrs on a warm renderer (k_dmr_*):
  dmr_wall.py [LOG2_ROWS]     a Diff of 2^LOG2_ROWS rows (default 24) made on the device -- four contigs, starts 1 to 100 bases apart,
                              depths 10 to 40 a group; stretches of 16 rows, an eighth of them differentially methylated in either
                              direction, four fifths of their rows significant: about a tenth of the rows are candidates --, joined
                              with the defaults six times, the first call discarded; next to it the only way to the same regions without
                              the kernels, a torch composition on the same device and rows (nonzero for the candidates, differences of
                              neighbours for the heads, four cumsums for the sums, diff_counts for the kept regions' p-values), six calls,
                              with its peak temporary memory; the two results compared column by column."""
import os, statistics, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch
import methyldackel_amd as mdk

LOG2 = int(sys.argv[1]) if len(sys.argv) > 1 else 24
PARAMS = dict(max_gap=300, max_skip=0, min_sites=3, min_diff=0.0)


def timed(f, n=6):
    ts, out = [], None
    for _ in range(n):
        out = None
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return ts, out


def line(what, ts, note=""):
    print(f"  {what:58s}: {ts[0]:.4f} | " + " ".join(f"{t:.4f}" for t in ts[1:]) + f"   median {statistics.median(ts[1:]):.4f} s {note}", flush=True)


def make(n, dev):
    g = torch.Generator(device=dev); g.manual_seed(20261019)
    i = torch.arange(n, device=dev)
    contig = (i * 4 // n).to(torch.int32)
    step = torch.randint(1, 101, (n,), generator=g, device=dev)
    pos = torch.cumsum(step, 0)
    first = torch.searchsorted(contig.to(torch.int64), torch.arange(4, device=dev))          # every contig starts anew
    start = (pos - pos[first][contig.to(torch.int64)] + 1).to(torch.int32)
    stretch = i // 16
    kind = (stretch * 2654435761 >> 7) % 16                                                 # 0: b above a, 1: a above b, else no difference
    active = kind < 2
    na, nb = (torch.randint(10, 41, (n,), generator=g, device=dev) for _ in range(2))
    a = (na * torch.empty(n, device=dev).uniform_(0.4, 0.6, generator=g)).round().to(torch.int64)
    fb = torch.where(kind == 0, 0.85, torch.where(kind == 1, 0.15, 0.5)) + torch.empty(n, device=dev).uniform_(-0.1, 0.1, generator=g)
    c = (nb * fb).round().to(torch.int64)
    sig = active & (torch.rand(n, generator=g, device=dev) < 0.8)
    cols = {"contig": contig, "start": start, "end": start + 1, "context": torch.zeros(n, dtype=torch.uint8, device=dev), "strand": torch.ones(n, dtype=torch.int8, device=dev),
            "nmeth_a": a, "nunmeth_a": na - a, "nmeth_b": c, "nunmeth_b": nb - c,
            "meth_diff": torch.zeros(n, dtype=torch.float64, device=dev), "pvalue": torch.ones(n, dtype=torch.float64, device=dev)}
    return mdk.Diff(["c0", "c1", "c2", "c3"], {k: v.contiguous() for k, v in cols.items()}), sig


def torch_dmrs(d, sig, max_gap, max_skip, min_sites, min_diff):
    """the same twelve columns without the kernels of mdk_dmr.hip (no refusals: the rows are known to be valid)"""
    a, b, c, e = d.nmeth_a, d.nunmeth_a, d.nmeth_b, d.nunmeth_b
    dirs = torch.sign(c * (a + b) - a * (c + e)) * (sig & (a + b > 0) & (c + e > 0))
    idx = torch.nonzero(dirs).squeeze(1)
    ci, cs, cd = d.contig[idx], d.start[idx].to(torch.int64), dirs[idx]
    cont = (ci[1:] == ci[:-1]) & (cd[1:] == cd[:-1]) & (cs[1:] - cs[:-1] <= max_gap) & (idx[1:] - idx[:-1] - 1 <= max_skip)
    head = torch.cat([cont.new_ones(1), ~cont])
    hpos = torch.nonzero(head).squeeze(1)
    ends = torch.cat([hpos[1:], hpos.new_full((1,), idx.shape[0])])
    first, last, nsig = idx[hpos], idx[ends - 1], ends - hpos
    sums = []
    for col in (a, b, c, e):
        pre = torch.cat([col.new_zeros(1), torch.cumsum(col, 0)])
        sums.append(pre[last + 1] - pre[first])
    sa, sb, sc, se = sums
    diff = 100.0 * (sc.to(torch.float64) / (sc + se).to(torch.float64) - sa.to(torch.float64) / (sa + sb).to(torch.float64))
    keep = (nsig >= min_sites) & (diff.abs() >= min_diff) & (torch.sign(sc * (sa + sb) - sa * (sc + se)) == cd[hpos])
    first, last = first[keep], last[keep]
    sa, sb, sc, se = (s[keep] for s in sums)
    p = mdk.diff_counts(torch.stack([sa, sc]), torch.stack([sb, se]), [0], [1])[5]
    return {"contig": d.contig[first], "start": d.start[first], "end": d.end[last], "nsites": (last - first + 1).to(torch.int32), "nsig": nsig[keep].to(torch.int32),
            "direction": cd[hpos][keep].to(torch.int8), "nmeth_a": sa, "nunmeth_a": sb, "nmeth_b": sc, "nunmeth_b": se, "meth_diff": diff[keep], "pvalue": p}


dev = torch.device("cuda", 0)
d, sig = make(1 << LOG2, dev)
a, b, c, e = d.nmeth_a, d.nunmeth_a, d.nmeth_b, d.nunmeth_b
candidates = int((sig & (c * (a + b) != a * (c + e))).sum())
print(f"{len(d)} rows, {candidates} candidates ({100.0 * candidates / len(d):.1f} %)", flush=True)
tr, r = timed(lambda: d.dmrs(sig, **PARAMS))
line("d.dmrs(sig)", tr, f"({len(r)} regions, {int(r.nsig.sum())} significant rows in them)")
torch.cuda.synchronize(); base = torch.cuda.memory_allocated(); torch.cuda.reset_peak_memory_stats()
tt, t = timed(lambda: torch_dmrs(d, sig, **PARAMS))
peak = torch.cuda.max_memory_allocated() - base
equal = all(torch.equal(getattr(r, n).view(torch.int64) if dt == "float64" else getattr(r, n), t[n].view(torch.int64) if dt == "float64" else t[n]) for n, dt in mdk.DMR_COLUMNS)
line("torch: nonzero, neighbour differences, cumsums, diff_counts", tt, f"(peak temporary memory {peak / 1e6:.0f} MB; equal columns: {equal})")
