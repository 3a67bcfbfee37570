"""Wall clock of Calls.regions on a warm session (k_region_*; profiles/regions_session_commands.txt):
  regions_wall.py session W   the all-context result of the sample summed over 1 kb tiles, 100 bp tiles and 1 kb windows at step 100, six
                              calls each, the first discarded; next to each the only way to the same sums without it, the torch formulation
                              on the same device and rows (a 64-bit key per row, searchsorted, three cumsums of filtered int64 columns), six
                              calls, with its peak temporary memory; the two results compared column by column
  regions_wall.py prof W      one extract and three regions calls per interval set, to be run under rocprofv3 --kernel-trace --stats
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


def torch_regions(c, iv, min_depth=1):
    """the same sums without the kernels: all contexts, any strand"""
    key = (c.contig.to(torch.int64) << 32) | c.start.to(torch.int64)
    lo = torch.searchsorted(key, (iv.contig.to(torch.int64) << 32) | iv.start.to(torch.int64))
    hi = torch.searchsorted(key, (iv.contig.to(torch.int64) << 32) | iv.end.to(torch.int64))
    del key
    ok = (c.nmeth.to(torch.int64) + c.nunmeth) >= min_depth
    out = []
    for col in (ok.to(torch.int64), ok * c.nmeth.to(torch.int64), ok * c.nunmeth.to(torch.int64)):
        pre = torch.cumsum(col, 0)
        del col
        pre = torch.cat([pre.new_zeros(1), pre])
        out.append(pre[hi] - pre[lo])
    return out


s = mdk.Session(0)
c = s.extract(args)
ref = mdk.Reference(fa)
print(f"{len(c)} per-strand rows in all contexts", flush=True)
sets = [("1 kb tiles", mdk.Intervals.windows(ref, 1000)), ("100 bp tiles", mdk.Intervals.windows(ref, 100)), ("1 kb windows, step 100", mdk.Intervals.windows(ref, 1000, 100))]
for what, iv in sets:
    iv = iv.to(c.start.device)
    if mode == "prof":
        for _ in range(3):
            r = c.regions(iv)
        print(f"{what}: {len(r)} intervals, {int(r.nsites.sum())} rows counted", flush=True)
        continue
    print(f"{what}: {len(iv)} intervals", flush=True)
    tr, r = timed(lambda: c.regions(iv))
    line("c.regions(iv)", tr, f"({int(r.nsites.sum())} rows counted)")
    torch.cuda.synchronize(); base = torch.cuda.memory_allocated(); torch.cuda.reset_peak_memory_stats()
    tt, t = timed(lambda: torch_regions(c, iv))
    peak = torch.cuda.max_memory_allocated() - base
    equal = torch.equal(r.nsites.to(torch.int64), t[0]) and torch.equal(r.nmeth, t[1]) and torch.equal(r.nunmeth, t[2])
    line("torch: key, searchsorted, three cumsums", tt, f"(peak temporary memory {peak / 1e6:.0f} MB; equal columns: {equal})")
    del r, t
