"""The times DESIGN.md quotes for the F test of several groups: tools/qdiff_times.py's seeded int32 cohorts, split into G equal groups --
`diff_groups` and, where G is 2, `diff_replicates` on the same matrices (k_qdiff: existing code, the yardstick) -- at [6, 2^22] and
[24, 2^20] in two groups, [9, 2^22] in three and [24, 2^20] in four.  Medians of warm calls, host clock around calls that return when
the device is done; the mean and the maximum of `steps`, the terms a site's series took, and the mean over wavefronts of the longest
series among a wavefront's 64 sites.  One JSON line.  --once: every call once (for a kernel trace)."""
import argparse
import json
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
    ap.add_argument("--shapes", default="6x22x2,24x20x2,9x22x3,24x20x4", help="samples x log2(sites) x groups, comma-separated")
    a = ap.parse_args()
    rep = 1 if a.once else a.repeat
    out = {"repeat": rep, "shapes": []}
    for shape in a.shapes.split(","):
        S, lg, G = (int(x) for x in shape.split("x"))
        n = 1 << lg
        m, u = cohort(S, n, 20261019 + {(6, 22): 0, (24, 20): 1}.get((S, lg), 2))                # (qdiff_times' seeds at its two shapes: the same matrices)
        groups = [list(range(g * S // G, (g + 1) * S // G)) for g in range(G)]
        if not a.once:
            mdk.diff_groups(m, u, groups)                                                        # warm: the library, the code object, the handle
            if G == 2:
                mdk.diff_replicates(m, u, groups[0], groups[1])
        r = {"samples": S, "sites": n, "groups": G}
        r["diff_groups_ms"] = median_ms(lambda: mdk.diff_groups(m, u, groups), rep)
        if G == 2:
            r["diff_replicates_ms"] = median_ms(lambda: mdk.diff_replicates(m, u, groups[0], groups[1]), rep)
            r["ratio"] = round(r["diff_groups_ms"] / r["diff_replicates_ms"], 3)
        got = mdk.diff_groups(m, u, groups, steps=True)
        steps = got[10].to(torch.int64)
        r["steps_mean"], r["steps_max"] = round(float(steps.double().mean()), 2), int(steps.max())
        if n >= 64:
            r["steps_wavefront"] = round(float(steps.view(-1, 64).max(1).values.double().mean()), 2)   # a wavefront waits for the longest of its 64
        r["rejected_at_0.05"] = round(float((got[5] < 0.05).double().mean()), 4)
        r["matrix_bytes_per_site"], r["output_bytes_per_site"] = 2 * S * m.element_size(), 16 * G + 48
        out["shapes"].append(r)
        del m, u, got, steps
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
