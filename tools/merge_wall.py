"""Wall clock of Calls.merge_context on a warm session (k_merge_*; profiles/merge_session_commands.txt):
  merge_wall.py session W   the all-context result of the sample merged on the device, six calls, the first discarded; next to it the only
                            way to the same rows without it, a second Session.extract(... --mergeContext) on the warm session, six calls; the
                            two results compared column by column; the same at min_depth 10 against -d 10
  merge_wall.py prof W      one extract and three merge_context calls, to be run under rocprofv3 --kernel-trace --stats
W = a scratch directory holding the sample m.fa / m.bam (tools/_build/mdk_synth -o W/m -L 128000000 -c 30 -s 5 -j 16)."""
import os, statistics, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch
import methyldackel_amd as mdk

mode, W = sys.argv[1], sys.argv[2]
args = [os.path.join(W, "m.fa"), os.path.join(W, "m.bam"), "-@", "16", "--CHG", "--CHH"]


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


def same(a, b):
    return len(a) == len(b) and all(torch.equal(getattr(a, n), getattr(b, n)) for n, _ in mdk.CALL_COLUMNS)


s = mdk.Session(0)
c = s.extract(args)
print(f"{len(c)} per-strand rows in all contexts", flush=True)
if mode == "prof":
    for _ in range(3):
        m = c.merge_context()
    print(f"{len(m)} merged rows", flush=True)
    sys.exit(0)
for depth, extra in ((1, []), (10, ["-d", "10"])):
    tm, m = timed(lambda: c.merge_context(min_depth=depth))
    line(f"c.merge_context(min_depth={depth})", tm, f"({len(m)} rows)")
    te, e = timed(lambda: s.extract(args + ["--mergeContext"] + extra))
    line("s.extract(... --mergeContext" + (" -d 10)" if extra else ")"), te, f"({len(e)} rows; equal columns: {same(m, e)})")
    del m, e
