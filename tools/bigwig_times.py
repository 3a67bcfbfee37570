"""The times DESIGN.md quotes for the bigWig track: 2^LOG2 CpG rows (default 22) on one contig, a C every third base, seeded counts of
depth 1 to 40 -- `Calls.write_bigwig` and, in the same process on the same rows, `Calls.write(prefix)` and `Calls.write(prefix,
compress=True)`: the parent commit's code, the yardstick.  Alternating, medians of warm calls, a host clock around calls that return
when the device is done and the file is written; `render_bigwig` (no file) beside them; the file's size and its sections.  One JSON
line.  --once: write_bigwig once after nothing but the table's upload (the run to put under a kernel trace).  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def table(n):
    import numpy as np
    import torch
    import methyldackel_amd as mdk
    rng = np.random.default_rng(20261019)
    start = (7 + 3 * np.arange(n, dtype=np.int64)).astype(np.int32)
    cov = rng.integers(1, 41, n)
    m = (rng.random(n) * (cov + 1)).astype(np.int64).clip(0, cov)
    t = {"contig": np.zeros(n, np.int32), "start": start, "end": start + 1, "nmeth": m.astype(np.int32), "nunmeth": (cov - m).astype(np.int32),
         "context": np.zeros(n, np.uint8), "strand": np.ones(n, np.int8)}
    return mdk.Calls(["chr1"], {k: torch.from_numpy(v).cuda() for k, v in t.items()}, contexts_on=(0,)), [int(start[-1]) + 50]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-rows", type=int, default=22)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bigwig_times: no GPU, and there is no CPU path")
    calls, lengths = table(1 << a.log2_rows)
    with tempfile.TemporaryDirectory(dir=a.dir) as td:
        bw = os.path.join(td, "t.bw")
        if a.once:
            calls.write_bigwig(bw, lengths)
            print(json.dumps({"mode": "once", "rows": len(calls), "file_bytes": os.path.getsize(bw)}))
            return
        legs = {"write_bigwig": lambda: calls.write_bigwig(bw, lengths), "write_plain": lambda: calls.write("w", directory=td),
                "write_compress": lambda: calls.write("w", directory=td, compress=True), "render_bigwig": lambda: calls.render_bigwig(lengths)}
        times = {k: [] for k in legs}
        for f in legs.values():
            f()                                                    # warm: libraries, code objects, handles, buffers, the page cache of the target
        for _ in range(a.repeat):
            for k, f in legs.items():                              # alternating
                torch.cuda.synchronize(); t0 = time.perf_counter(); f(); torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
        sizes = {"bigwig": os.path.getsize(bw), "bedGraph": os.path.getsize(os.path.join(td, "w_CpG.bedGraph")), "bedGraph_gz": os.path.getsize(os.path.join(td, "w_CpG.bedGraph.gz"))}
        n = len(calls)
        data_sections = (n + 1023) // 1024
        print(json.dumps({"mode": "wall", "rows": n, "repeat": a.repeat, "median_ms": {k: round(statistics.median(v), 3) for k, v in times.items()},
                          "min_ms": {k: round(min(v), 3) for k, v in times.items()}, "max_ms": {k: round(max(v), 3) for k, v in times.items()},
                          "bytes": sizes, "data_sections": data_sections, "raw_section_bytes": 24 * data_sections + 12 * n}))


if __name__ == "__main__":
    main()
