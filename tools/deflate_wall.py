#!/usr/bin/env python3
"""TEST INFRASTRUCTURE: the wall times DESIGN.md section 4 quotes for BGZF made and read on the device (csrc/mdk_deflate.hip).

  python tools/deflate_wall.py wall [LOG2_ROWS] [RUNS] [DIR]    one block of 2^LOG2_ROWS CpG rows (default 22) on a seeded reference:
        the caller's wall time of Calls.write(prefix) / Calls.write(prefix, compress=True) / the plain write followed by host zlib level 1
        over the file, alternating, medians of RUNS (default 7) after a warm-up of each; Calls.read of the plain file and of the .gz;
        bgzf_compress of the block's text alone (a host clock around the synchronous call: CRC, compress, scan, pack); the file's size
        against zlib level 1 and level 6 over the same text in 65280-byte members.  One JSON line.
  python tools/deflate_wall.py kernel [LOG2_ROWS] [ITERS]       bgzf_compress of the same text ITERS times and nothing else: the run to put
        under `rocprofv3 --kernel-trace --stats` for k_deflate's own time.
Needs a GPU: there is no CPU path."""
import json
import os
import statistics
import sys
import tempfile
import time
import zlib
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def make(log2_rows, d):
    """a seeded reference of four contigs, and Calls of 2^log2_rows rows on its first C / G positions"""
    import numpy as np
    import torch
    import methyldackel_amd as mdk
    n = 1 << log2_rows
    rng = np.random.default_rng(20261019)
    per = (n * 2 + (n >> 2)) // 4 + 1000                                # half the bases are C or G
    fa, cols = d / "ref.fa", {k: [] for k in ("contig", "start")}
    with open(fa, "wb") as f:
        for c in range(4):
            b = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, per)]
            f.write(b">chr%d\n" % (c + 1)); f.write(b.tobytes()); f.write(b"\n")
            pos = np.nonzero((b == 67) | (b == 71))[0].astype(np.int32)
            cols["contig"].append(np.full(pos.shape, c, np.int32)); cols["start"].append(pos)
    contig, start = np.concatenate(cols["contig"])[:n], np.concatenate(cols["start"])[:n]
    assert contig.shape[0] == n
    m, u = rng.integers(0, 40, n).astype(np.int32), rng.integers(0, 15, n).astype(np.int32)
    m[(m + u) == 0] = 1
    t = {"contig": contig, "start": start, "end": start + 1, "nmeth": m, "nunmeth": u, "context": np.zeros(n, np.uint8), "strand": np.ones(n, np.int8)}
    calls = mdk.Calls(["chr1", "chr2", "chr3", "chr4"], {k: torch.from_numpy(v).cuda() for k, v in t.items()}, contexts_on=(0,))
    return fa, calls


def timed(f):
    import torch
    torch.cuda.synchronize(); t0 = time.perf_counter(); r = f(); torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def main():
    import torch
    import methyldackel_amd as mdk
    mode = sys.argv[1] if len(sys.argv) > 1 else "wall"
    log2_rows = int(sys.argv[2]) if len(sys.argv) > 2 else 22
    runs = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    if not torch.cuda.is_available():
        sys.exit("deflate_wall: no GPU, and there is no CPU path")
    with tempfile.TemporaryDirectory(dir=sys.argv[4] if len(sys.argv) > 4 else None) as td:
        d = Path(td)
        fa, calls = make(log2_rows, d)
        text = calls.render(prefix="w", header=False)
        if mode == "kernel":
            for _ in range(runs):
                mdk.bgzf_compress(text)
            torch.cuda.synchronize()
            print(json.dumps({"mode": "kernel", "rows": len(calls), "text_bytes": text.numel(), "iters": runs}))
            return

        def gz_level1(p):
            data, c = open(p, "rb").read(), zlib.compressobj(1, zlib.DEFLATED, 31)
            with open(p + ".gz", "wb") as f:
                f.write(c.compress(data)); f.write(c.flush())

        legs = {"write_plain": lambda: calls.write("w", directory=td), "write_compress": lambda: calls.write("w", directory=td, compress=True),
                "write_plain_then_zlib1": lambda: gz_level1(calls.write("z", directory=td)[0]), "bgzf_compress_text": lambda: mdk.bgzf_compress(text)}
        times = {k: [] for k in legs}
        for k, f in legs.items():
            f()                                                          # warm-up: code objects, buffers, the page cache of the target
        for _ in range(runs):
            for k, f in legs.items():                                    # alternating
                times[k].append(timed(f)[0])
        plain, gz = str(d / "w_CpG.bedGraph"), str(d / "w_CpG.bedGraph.gz")
        with mdk.Reference(fa) as ref:
            rlegs = {"read_plain": lambda: mdk.Calls.read(plain, ref), "read_gz": lambda: mdk.Calls.read(gz, ref)}
            a, b = rlegs["read_plain"](), rlegs["read_gz"]()
            assert len(a) == len(b) == len(calls) and all(torch.equal(getattr(a, n), getattr(b, n)) for n, _ in mdk.CALL_COLUMNS)
            for k in rlegs:
                times[k] = []
            for _ in range(runs):
                for k, f in rlegs.items():
                    times[k].append(timed(f)[0])
        data = open(plain, "rb").read()
        import gzip
        assert gzip.decompress(open(gz, "rb").read()) == data
        body = data[data.index(b"\n") + 1:]
        sizes = {"text": len(data), "gz": os.path.getsize(gz)}
        for lv in (1, 6):
            sizes[f"zlib{lv}_members"] = sum(len(zlib.compress(body[o:o + 65280], lv)) - 6 + 26 for o in range(0, len(body), 65280))
        med = {k: statistics.median(v) for k, v in times.items()}
        print(json.dumps({"mode": "wall", "rows": len(calls), "runs": runs, "text_bytes": text.numel(), "median_s": {k: round(v, 5) for k, v in med.items()},
                          "min_s": {k: round(min(v), 5) for k, v in times.items()}, "max_s": {k: round(max(v), 5) for k, v in times.items()},
                          "bgzf_compress_GBps_text_in": round(text.numel() / med["bgzf_compress_text"] / 1e9, 3), "sizes": sizes,
                          "ratio": {k: round(sizes["text"] / v, 3) for k, v in sizes.items() if k != "text"}}))


if __name__ == "__main__":
    main()
