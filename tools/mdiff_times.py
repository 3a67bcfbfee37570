"""The times DESIGN.md quotes for the F test of a design's columns: tools/qdiff_times.py's seeded int32 cohort at [12, 2^22], `diff_model`
with a design of four columns -- an intercept, a batch of the samples' second half, a continuous column and the group, which is
tested -- and, on the same matrices, `diff_groups` of the two groups (k_gdiff: existing code, the yardstick).  Medians of warm calls, host
clock around calls that return when the device is done; the mean and the maximum of `iterations`, the passes a site's two fits took,
and the mean over wavefronts of the most passes among a wavefront's 64 sites.  One JSON line.  --once: every call once (for a kernel
trace)."""
import argparse
import json
import random
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from qdiff_times import cohort, median_ms


def main():
    import torch
    import methyldackel_amd as mdk
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--shapes", default="12x22x4", help="samples x log2(sites) x columns (2 to 4), comma-separated")
    a = ap.parse_args()
    rep = 1 if a.once else a.repeat
    out = {"repeat": rep, "shapes": []}
    for shape in a.shapes.split(","):
        S, lg, p = (int(x) for x in shape.split("x"))
        n = 1 << lg
        m, u = cohort(S, n, 20261021)
        rng = random.Random(20261021)
        design = [[1.0, float(s >= S // 2), round(rng.uniform(-2.0, 2.0), 2), float(s % 2)] for s in range(S)]
        design = [row[:p - 1] + [row[3]] for row in design]                                          # the group is the last column, and it is tested
        groups = [[s for s in range(S) if s % 2 == g] for g in (0, 1)]
        if not a.once:
            mdk.diff_model(m, u, design, p - 1)                                                      # warm: the library, the code object, the handle
            mdk.diff_groups(m, u, groups)
        r = {"samples": S, "sites": n, "columns": p}
        r["diff_model_ms"] = median_ms(lambda: mdk.diff_model(m, u, design, p - 1), rep)
        r["diff_groups_ms"] = median_ms(lambda: mdk.diff_groups(m, u, groups), rep)
        r["ratio"] = round(r["diff_model_ms"] / r["diff_groups_ms"], 3)
        got = mdk.diff_model(m, u, design, p - 1, steps=True)
        passes = got[8].to(torch.int64)
        r["passes_mean"], r["passes_max"] = round(float(passes.double().mean()), 2), int(passes.max())
        if n >= 64:
            r["passes_wavefront"] = round(float(passes.view(-1, 64).max(1).values.double().mean()), 2)   # a wavefront waits for the longest of its 64
        r["flagged"] = int((got[7] != 0).sum())
        r["rejected_at_0.05"] = round(float((got[3] < 0.05).double().mean()), 4)
        r["matrix_bytes_per_site"], r["output_bytes_per_site"] = 2 * S * m.element_size(), 8 * p + 49
        out["shapes"].append(r)
        del m, u, got, passes
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
