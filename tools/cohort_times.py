"""The times DESIGN.md quotes for the united table as text: one `Cohort.render` and one `Cohort.read` of a seeded table (2^20 sites, 16
samples by default, about 150 MB of text), and next to them the S calls of `cohort.sample(i).render("bedGraph")` that were the only way to
get the counts out before.  Every call is timed ONCE, between device events, after a warm-up on a small table that loads the code objects;
one JSON line.  `render` leaves the file `read` takes:
    cohort_times.py render --file F;  cohort_times.py read --file F;  cohort_times.py bedgraph"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
CONTIGS = ["chr1", "chr2"]


def table(n, S, seed):
    import torch
    import methyldackel_amd as mdk
    g = torch.Generator(device="cuda").manual_seed(seed)
    start = (torch.arange(n, device="cuda", dtype=torch.int64) * 100 + torch.randint(0, 99, (n,), device="cuda", generator=g)).to(torch.int32)
    contig = (torch.arange(n, device="cuda") >= (n * 3) // 5).to(torch.int32)
    cols = {"contig": contig, "start": start, "end": start + 1, "context": torch.zeros(n, dtype=torch.uint8, device="cuda"),
            "strand": (torch.randint(0, 2, (n,), device="cuda", generator=g) * 2 - 1).to(torch.int8), "nsamples": torch.full((n,), S, dtype=torch.int32, device="cuda")}
    m, u = (torch.randint(0, 60, (S, n), device="cuda", generator=g).to(torch.int32) for _ in range(2))
    return mdk.Cohort(CONTIGS, cols, m, u, contexts_on=(0,))


def timed(f):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(); out = f(); b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def main():
    import tempfile
    import methyldackel_amd as mdk
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("render", "read", "bedgraph"))
    ap.add_argument("--sites", type=int, default=1 << 20)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--file")
    a = ap.parse_args()
    small = table(5000, a.samples, 2)
    out = {"what": a.what, "sites": a.sites, "samples": a.samples}
    if a.what == "read":
        with tempfile.TemporaryDirectory() as d:
            mdk.Cohort.read(small.write(Path(d) / "warm.tsv"), CONTIGS)
        c, ms = timed(lambda: mdk.Cohort.read(a.file, CONTIGS))
        out.update(rows=len(c), text_bytes=Path(a.file).stat().st_size)
    else:
        c = table(a.sites, a.samples, 1)
        if a.what == "render":
            small.render()
            t, ms = timed(lambda: c.render())
            out["text_bytes"] = t.numel()
            if a.file:
                Path(a.file).write_bytes(bytes(t.cpu().numpy()))
        else:
            small.sample(0).render("bedGraph", header=False)
            texts, ms = timed(lambda: [c.sample(i).render("bedGraph", header=False) for i in range(a.samples)])
            out["text_bytes"] = sum(t.numel() for t in texts)
    out.update(ms=round(ms, 2), gb_per_s=round(out["text_bytes"] / ms / 1e6, 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
