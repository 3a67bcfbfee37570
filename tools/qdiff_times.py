"""The times DESIGN.md quotes for the replicates' F test: a seeded [6, 2^22] int32 cohort, three samples against three, depths 20 to 40 --
`diff_replicates` and, on the same matrices, `diff_counts` (Fisher's test of the pooled tables: existing code, the yardstick) --, and the
same pair at [24, 2^20], twelve against twelve.  Medians of warm calls, host clock around calls that return when the device is done; the
mean and the maximum of `steps`, the terms a site's series took, and the mean over wavefronts of the longest series among a wavefront's
64 sites.  One JSON line.  --once: every call once (for a kernel trace)."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def median_ms(f, n):
    out = []
    for _ in range(n):
        t = time.perf_counter(); f(); out.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(out), 3)


def cohort(S, n, seed):
    """replicates as the calibration has them, made on the device: a fraction per site, every sample's own fraction around it (sd 0.1:
    over-dispersed), depths 20 to 40, the methylated count the rounded product"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    depth = torch.randint(20, 41, (S, n), device="cuda", generator=g)
    site = torch.rand((1, n), device="cuda", generator=g) * 0.8 + 0.1
    own = (site + torch.randn((S, n), device="cuda", generator=g) * 0.1).clamp(0.0, 1.0)
    m = torch.round(depth * own).to(torch.int32)
    return m.contiguous(), (depth.to(torch.int32) - m).contiguous()


def main():
    import torch
    import methyldackel_amd as mdk
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--shapes", default="6x22,24x20", help="samples x log2(sites), comma-separated")
    a = ap.parse_args()
    rep = 1 if a.once else a.repeat
    out = {"repeat": rep, "shapes": []}
    for k, shape in enumerate(a.shapes.split(",")):
        S, lg = (int(x) for x in shape.split("x"))
        n = 1 << lg
        m, u = cohort(S, n, 20261019 + k)
        ga, gb = list(range(S // 2)), list(range(S // 2, S))
        if not a.once:
            mdk.diff_replicates(m, u, ga, gb); mdk.diff_counts(m, u, ga, gb)                 # warm: libraries, code objects, the handle
        r = {"samples": S, "sites": n}
        r["diff_replicates_ms"] = median_ms(lambda: mdk.diff_replicates(m, u, ga, gb), rep)
        r["diff_counts_ms"] = median_ms(lambda: mdk.diff_counts(m, u, ga, gb), rep)
        r["ratio"] = round(r["diff_replicates_ms"] / r["diff_counts_ms"], 3)
        got = mdk.diff_replicates(m, u, ga, gb, steps=True)
        steps = got[9].to(torch.int64)
        r["steps_mean"], r["steps_max"] = round(float(steps.double().mean()), 2), int(steps.max())
        if n >= 64:
            r["steps_wavefront"] = round(float(steps.view(-1, 64).max(1).values.double().mean()), 2)   # a wavefront waits for the longest of its 64
        r["rejected_at_0.05"] = round(float((got[5] < 0.05).double().mean()), 4)
        r["matrix_bytes_per_site"], r["output_bytes_per_site"] = 2 * S * m.element_size(), 60
        out["shapes"].append(r)
        del m, u, got, steps
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
