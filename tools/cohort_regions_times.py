"""The times DESIGN.md quotes for `Cohort.regions`: every sample's sums over intervals in one call, and next to it the way it replaces -- the
loop `[cohort.sample(s).regions(iv) for s in range(S)]` and the three `torch.stack` behind it.  A seeded cohort as tools/cohort_times.py
builds it (a site about every 100 bases, two contigs; 2^22 sites and 16 samples by default, `--sites 1048576 --samples 64` is the second size
quoted) and three interval sets: 1 kb tiles, 100 bp tiles, and 1 kb windows at step 100.  After a warm-up on a small table that loads the
code objects, the call and the loop are timed in turns, `--repeats` (5) times each, between device events with a synchronise; both must
give equal matrices at the size timed.  One JSON line: per set the intervals, and of each way the median and the range in ms.
`--calls-only` leaves the loop out, warm-up included: the run for `rocprofv3 --kernel-trace --stats`, whose statistics then hold the
call's kernels alone.
    cohort_regions_times.py [--sites N] [--samples S] [--repeats R] [--sets tiles1k,tiles100,slide1k] [--calls-only]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
SETS = {"tiles1k": (1000, 1000), "tiles100": (100, 100), "slide1k": (1000, 100)}          # width, step


def timed(f):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(); out = f(); b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def looped(c, iv):
    import torch
    per = [c.sample(s).regions(iv) for s in range(c.n_samples)]
    return [torch.stack([getattr(p, name) for p in per]) for name in ("nsites", "nmeth", "nunmeth")]


def windows(c, width, step):
    import methyldackel_amd as mdk
    lengths = [int(c.start[c.contig == t].max()) + 1 for t in range(len(c.contigs))]
    return mdk.Intervals.windows(lengths, width, step, contigs=c.contigs).to(c.start.device)


def main():
    import torch
    from cohort_times import table
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=1 << 22)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sets", default=",".join(SETS))
    ap.add_argument("--calls-only", action="store_true")
    a = ap.parse_args()
    small = table(5000, a.samples, 2)
    iv = windows(small, 1000, 1000)
    small.regions(iv)
    if not a.calls_only:
        looped(small, iv)
    c = table(a.sites, a.samples, 1)
    out = {"sites": a.sites, "samples": a.samples, "repeats": a.repeats, "sets": {}}
    for name in a.sets.split(","):
        iv = windows(c, *SETS[name])
        call, loop = [], []
        for _ in range(a.repeats):
            r, ms = timed(lambda: c.regions(iv)); call.append(ms)
            if not a.calls_only:
                w, ms = timed(lambda: looped(c, iv)); loop.append(ms)
                assert all(torch.equal(x, y) for x, y in zip((r.nsites, r.nmeth, r.nunmeth), w)), name
                del w
            del r
        side = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
        out["sets"][name] = {"intervals": len(iv), "call": side(call)}
        if loop:
            out["sets"][name].update(loop=side(loop), loop_over_call=round(statistics.median(loop) / statistics.median(call), 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
