"""Wall clock of the files a session writes (k_text_*; profiles/text_session_commands.txt):
  text_wall.py cmd W CLI [LEGS]   CLI = a MethylDackel binary (the parent commit's build): `extract -o out` per format and `perRead -o file`, six runs
                                  each, the first discarded
  text_wall.py session W [LEGS]   a warm Session's run + write per format, and perread + write, six each, files compared with what `cmd` kept; write
                                  split into its device part
  text_wall.py prof W [LEGS]      three extract + write, cytosine_report + write and perread + write + select calls, to be run under
                                  rocprofv3 --kernel-trace --stats
W = a scratch directory holding the sample m.fa / m.bam (tools/_build/mdk_synth -o W/m -L 128000000 -c 30 -s 5 -j 16).  LEGS: "calls" (the
extract formats), "reads" (perRead) or "all" (the default)."""
import os, shutil, statistics, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
mode, W = sys.argv[1], sys.argv[2]
LEGS = sys.argv[4 if mode == "cmd" else 3] if len(sys.argv) > (4 if mode == "cmd" else 3) else "all"
CALLS, READS = LEGS in ("calls", "all"), LEGS in ("reads", "all")
SETS = (("CpG only", []), ("--CHG --CHH", ["--CHG", "--CHH"]))
base = [os.path.join(W, "m.fa"), os.path.join(W, "m.bam"), "-@", "16"]


def fresh(name):
    d = os.path.join(W, name)
    shutil.rmtree(d, ignore_errors=True); os.makedirs(d)
    return d


def line(what, ts, note=""):
    print(f"  {what:34s}: {ts[0]:.4f} | " + " ".join(f"{t:.4f}" for t in ts[1:]) + f"   median {statistics.median(ts[1:]):.3f} {note}", flush=True)


if mode == "cmd":
    PARENT = os.path.abspath(sys.argv[3])
    env = dict(os.environ, MDK_NO_RANKS="1", HSA_DISABLE_COREDUMP_ON_EXCEPTION="1")
    if READS:
        print("perRead", flush=True)
        ts = []
        for i in range(6):
            d = fresh("cmd_out")
            t0 = time.perf_counter()
            r = subprocess.run([PARENT, "perRead"] + base + ["-o", "out.perRead.txt"], cwd=d, env=env, capture_output=True, text=True, timeout=600)
            ts.append(time.perf_counter() - t0)
            if r.returncode:
                print("command failed", r.returncode, r.stderr[-2000:]); sys.exit(1)
        line("parent's command perRead -o", ts, f"({os.path.getsize(os.path.join(d, 'out.perRead.txt')) / 1e6:.1f} MB of text)")
        keep = os.path.join(W, "keep_perRead")
        shutil.rmtree(keep, ignore_errors=True); shutil.move(d, keep)
    for label, extra in SETS if CALLS else ():
        print(label, flush=True)
        for what, opt in (("parent's command -o", []), ("parent's command --cytosine_report", ["--cytosine_report"]), ("parent's command --fraction", ["--fraction"]), ("parent's command --methylKit", ["--methylKit"])):
            ts = []
            for i in range(6):
                d = fresh("cmd_out")
                t0 = time.perf_counter()
                r = subprocess.run([PARENT, "extract"] + base + extra + opt + ["-o", "out"], cwd=d, env=env, capture_output=True, text=True, timeout=120)
                ts.append(time.perf_counter() - t0)
                if r.returncode:
                    print("command failed", r.returncode, r.stderr[-2000:]); sys.exit(1)
            size = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
            line(what, ts, f"({size / 1e6:.1f} MB of text)")
            keep = os.path.join(W, "keep_" + label.split()[0] + "_" + (opt[0].strip("-") if opt else "default"))
            shutil.rmtree(keep, ignore_errors=True); shutil.move(d, keep)
    sys.exit(0)

import torch
import methyldackel_amd as mdk
x = torch.zeros(1 << 20, device="cuda"); torch.cuda.synchronize()
s = mdk.Session(0)


def same(d, keep):
    a, b = sorted(os.listdir(d)), sorted(os.listdir(keep))
    ok = a == b and all(subprocess.run(["cmp", "-s", os.path.join(d, f), os.path.join(keep, f)]).returncode == 0 for f in a)
    return "files identical to the command's" if ok else "FILES DIFFER FROM THE COMMAND'S"


if mode == "session" and READS:
    print("perRead", flush=True)
    ts, te, tw = [], [], []
    for i in range(6):
        d = fresh("ses_out")
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = s.perread(base)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        r.write(os.path.join(d, "out.perRead.txt"))
        t2 = time.perf_counter()
        ts.append(t2 - t0); te.append(t1 - t0); tw.append(t2 - t1)
    line("Session.perread + write", ts, f"({len(r)} rows, {r.name_bytes.shape[0] / 1e6:.1f} MB of names; {same(d, os.path.join(W, 'keep_perRead'))})")
    line("  of which the run", te); line("  of which write", tw)
    # where write's time goes: the text made and dropped (k_rtext_len, k_text_blocks, k_rtext_fill and their waits); then made and copied to pinned
    # memory without the file.  The rest of write is the file append
    tr, tc = [], []
    for i in range(4):
        torch.cuda.synchronize(); t0 = time.perf_counter(); nb = 0
        for b in r._text_blocks(mdk.TEXT_PERREAD, None, None):
            nb += b.numel()
        torch.cuda.synchronize(); tr.append(time.perf_counter() - t0)
    pin = None
    for i in range(4):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for b in r._text_blocks(mdk.TEXT_PERREAD, None, None):
            if pin is None or pin.numel() < b.numel():
                pin = torch.empty(b.numel() + b.numel() // 8, dtype=torch.uint8, pin_memory=True)
            pin[:b.numel()].copy_(b, non_blocking=True); torch.cuda.synchronize()
        tc.append(time.perf_counter() - t0)
    print(f"    text made on the device and dropped: " + " ".join(f"{t:.4f}" for t in tr) + f"   ({nb / 1e6:.1f} MB)", flush=True)
    print(f"    text made and copied to pinned memory, no file: " + " ".join(f"{t:.4f}" for t in tc), flush=True)
    ts = []
    for i in range(4):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        f = r.select(r.nmeth + r.nunmeth >= 5)
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    print(f"    select(nmeth + nunmeth >= 5): " + " ".join(f"{t:.4f}" for t in ts) + f"   ({len(f)} of {len(r)} rows, {f.name_bytes.shape[0] / 1e6:.1f} MB of names)", flush=True)
    del r, f, pin

if mode == "session":
    for label, extra in SETS if CALLS else ():
        print(label, flush=True)
        tag = label.split()[0]
        for what, run, fmt, keep in (("Session.extract + write", s.extract, "bedGraph", "default"), ("Session.extract + write fraction", s.extract, "fraction", "fraction"),
                                     ("Session.extract + write methylKit", s.extract, "methylKit", "methylKit"), ("Session.cytosine_report + write", s.cytosine_report, None, "cytosine_report")):
            ts, te, tw = [], [], []
            for i in range(6):
                d = fresh("ses_out")
                torch.cuda.synchronize(); t0 = time.perf_counter()
                c = run(base + extra)
                torch.cuda.synchronize(); t1 = time.perf_counter()
                if fmt is None:
                    c.write("out", directory=d)
                else:
                    c.write("out", fmt, directory=d)
                t2 = time.perf_counter()
                ts.append(t2 - t0); te.append(t1 - t0); tw.append(t2 - t1)
            line(what, ts, f"({len(c)} rows; {same(d, os.path.join(W, 'keep_' + tag + '_' + keep))})")
            line("  of which the run", te); line("  of which write", tw)
            # where write's time goes: the text made and dropped (k_text_len, k_text_blocks, k_text_fill and their waits), then with the copy to pinned memory
            tr = []
            for i in range(4):
                torch.cuda.synchronize(); t0 = time.perf_counter(); nb = 0
                for k in (c.contexts_on if fmt is not None else (None,)):
                    for b in c._text_blocks(mdk.TEXT_FORMATS[fmt] if fmt is not None else mdk.TEXT_CYTOSINE_REPORT, k, None):
                        nb += b.numel()
                torch.cuda.synchronize(); tr.append(time.perf_counter() - t0)
            print(f"    text made on the device and dropped: " + " ".join(f"{t:.4f}" for t in tr) + f"   ({nb / 1e6:.1f} MB)", flush=True)
            if fmt is not None:
                print("    rows per context:", [int((c.context == k).sum().item()) for k in range(3)], flush=True)
            del c
    sys.exit(0)

if mode == "prof":
    args = base + ["--CHG", "--CHH"]
    for i in range(3 if READS else 0):
        d = fresh("prof_out")
        r = s.perread(base); r.write(os.path.join(d, "out.perRead.txt"))
        f = r.select(r.nmeth + r.nunmeth >= 5)
        print(len(r), int(r.name_bytes.shape[0]), os.path.getsize(os.path.join(d, "out.perRead.txt")), len(f), int(f.name_bytes.shape[0]), flush=True)
        del r, f
    for i in range(3 if CALLS else 0):
        d = fresh("prof_out")
        c = s.extract(args); c.write("out", directory=d); c.write("out", "methylKit", directory=d)
        y = s.cytosine_report(args); y.write("out", directory=d)
        print(len(c), len(y), [int((c.context == k).sum().item()) for k in range(3)], {f: os.path.getsize(os.path.join(d, f)) for f in sorted(os.listdir(d))}, flush=True)
        del c, y
