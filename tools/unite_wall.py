"""Wall clock of mdk.unite on a warm session (k_unite_*; profiles/unite_session_commands.txt):
  unite_wall.py session W   the all-context result of the sample, S = 2 and S = 8 copies of it subsampled at 0.7 (seeded), united at
                            min_samples = S and at min_samples = 1, six calls each, the first discarded; next to each the only way to
                            the same table without it, the torch formulation on the same device and rows (a 64-bit key per present row,
                            cat, unique with inverse and counts, scatter), six calls, with its peak temporary memory; the library's own
                            temporaries as the device memory the first call took beyond torch's; the two results compared column by column
  unite_wall.py prof W      one extract and three unite calls per S, to be run under rocprofv3 --kernel-trace --stats
W = a scratch directory holding the sample m.fa / m.bam (tools/_build/mdk_synth -o W/m -L 128000000 -c 30 -s 5 -j 16)."""
import os, statistics, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch
import methyldackel_amd as mdk

mode, W = sys.argv[1], sys.argv[2]
fa = os.path.join(W, "m.fa")
args = [fa, os.path.join(W, "m.bam"), "-@", "16", "--CHG", "--CHH"]


def timed(f, n=6):
    ts, out = [], None
    for _ in range(n):
        out = None
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return ts, out


def line(what, ts, note=""):
    print(f"  {what:44s}: {ts[0]:.4f} | " + " ".join(f"{t:.4f}" for t in ts[1:]) + f"   median {statistics.median(ts[1:]):.4f} s {note}", flush=True)


def torch_unite(samples, min_samples, min_depth=1):
    """the same table without the kernels: (keys of the kept sites, nsamples, nmeth [S, n], nunmeth [S, n])"""
    present = [(c.nmeth.to(torch.int64) + c.nunmeth) >= min_depth for c in samples]
    keys = torch.cat([((c.contig.to(torch.int64) << 32) | c.start.to(torch.int64))[p] for c, p in zip(samples, present)])
    uniq, inverse, counts = torch.unique(keys, return_inverse=True, return_counts=True)
    del keys
    keep = counts >= min_samples
    place = torch.cumsum(keep, 0) - 1
    n = int(keep.sum())
    nmeth, nunmeth = (torch.zeros((len(samples), n), dtype=torch.int32, device=uniq.device) for _ in range(2))
    at = 0
    for s, (c, p) in enumerate(zip(samples, present)):
        k = int(p.sum())
        inv = inverse[at:at + k]
        at += k
        ok = keep[inv]
        to = place[inv][ok]
        nmeth[s][to] = c.nmeth[p][ok]
        nunmeth[s][to] = c.nunmeth[p][ok]
    return uniq[keep], counts[keep], nmeth, nunmeth


def free_beyond_torch():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0] + torch.cuda.memory_reserved()


s = mdk.Session(0)
c = s.extract(args)
n = len(c)
print(f"{n} per-strand rows in all contexts", flush=True)
for S in (2, 8):
    samples = []
    for k in range(S):
        g = torch.Generator(device=c.start.device); g.manual_seed(1000 + k)
        samples.append(c.select(torch.rand(n, device=c.start.device, generator=g) < 0.7))
    rows = sum(len(x) for x in samples)
    if mode == "prof":
        for _ in range(3):
            co = mdk.unite(samples)
        print(f"S = {S}: {rows} rows, {co.n_union} sites in the union, {len(co)} in all samples", flush=True)
        del samples, co
        continue
    print(f"S = {S}: {rows} rows", flush=True)
    for k in (S, 1):
        before = free_beyond_torch()
        tu, co = timed(lambda: mdk.unite(samples, min_samples=k))
        own = before - free_beyond_torch()
        line(f"mdk.unite(samples, min_samples={k})", tu, f"({co.n_union} sites in the union, {len(co)} kept; the library's tables grew by {own / 1e6:.0f} MB)")
        torch.cuda.synchronize(); base = torch.cuda.memory_allocated(); torch.cuda.reset_peak_memory_stats()
        tt, t = timed(lambda: torch_unite(samples, k))
        peak = torch.cuda.max_memory_allocated() - base - sum(x.numel() * x.element_size() for x in t)
        equal = torch.equal((co.contig.to(torch.int64) << 32) | co.start.to(torch.int64), t[0]) and torch.equal(co.nsamples.to(torch.int64), t[1]) and torch.equal(co.nmeth, t[2]) and torch.equal(co.nunmeth, t[3])
        line("torch: key, cat, unique, scatter", tt, f"(peak temporary memory {peak / 1e6:.0f} MB; equal columns: {equal})")
        del co, t
    del samples
