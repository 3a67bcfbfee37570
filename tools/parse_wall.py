"""Wall clock of reading bedGraph files back on the device (k_parse_*; profiles/parse_session_commands.txt):
  parse_wall.py session W   the three per-context files of the sample (written once by Calls.write) read, sorted, merged and written again --
                            Calls.read(paths, ref).sorted().merge_context().write(...) --, six calls, the first discarded; the read alone, six
                            calls; next to it the only other way to those bytes, `MethylDackel mergeContext` on each of the three files, six
                            runs; the two outputs compared byte for byte behind their header lines
  parse_wall.py prof W      three reads of the three files, to be run under rocprofv3 --kernel-trace --stats
W = a scratch directory holding the sample m.fa / m.bam (tools/_build/mdk_synth -o W/m -L 128000000 -c 30 -s 5 -j 16)."""
import os, statistics, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch
import methyldackel_amd as mdk

mode, W = sys.argv[1], sys.argv[2]
fa = os.path.join(W, "m.fa")
args = [fa, os.path.join(W, "m.bam"), "-@", "16", "--CHG", "--CHH"]
CTX = ("CpG", "CHG", "CHH")


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


def body(path):
    with open(path, "rb") as f:
        f.readline()
        return f.read()


paths = [os.path.join(W, f"p_{c}.bedGraph") for c in CTX]
if not all(os.path.exists(p) for p in paths):
    s = mdk.Session(0)
    c = s.extract(args)
    c.write("p", directory=W)
    print(f"{len(c)} per-strand rows in all contexts written", flush=True)
    del c
    s.close()
size = sum(os.path.getsize(p) for p in paths)
t0 = time.perf_counter()
ref = mdk.Reference(fa)
ref._renderer(0)
torch.cuda.synchronize()
print(f"{size} bytes of bedGraph in three files; the reference read and uploaded once in {time.perf_counter() - t0:.3f} s", flush=True)
if mode == "prof":
    for _ in range(3):
        c = mdk.Calls.read(paths, ref)
    print(f"{len(c)} rows", flush=True)
    sys.exit(0)
tr, c = timed(lambda: mdk.Calls.read(paths, ref))
line("Calls.read(three files, ref)", tr, f"({len(c)} rows, {size / statistics.median(tr[1:]) / 1e9:.2f} GB/s of text)")
del c
ta, out = timed(lambda: mdk.Calls.read(paths, ref).sorted().merge_context().write("q", directory=W))
line("Calls.read(...).sorted().merge_context().write(q)", ta)


def command():
    for ctx, p in zip(CTX, paths):
        r = subprocess.run([str(mdk.CLI), "mergeContext", "-o", os.path.join(W, f"t_{ctx}.bedGraph"), fa, p], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    return True


tc, _ = timed(command)
line("MethylDackel mergeContext, the three files in turn", tc)
for ctx in CTX:
    print(f"  {ctx}: equal bytes behind the header line: {body(os.path.join(W, f'q_{ctx}.bedGraph')) == body(os.path.join(W, f't_{ctx}.bedGraph'))}", flush=True)
