"""The times DESIGN.md quotes for the tabix index: a table of 2^22 CpG rows written with and without its index, `tabix_index` of the written
file, and one 1 Mb region read against the whole file.  Medians of warm calls, one JSON line.  --once: every call once (for a kernel trace)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def median_ms(f, n):
    out = []
    for _ in range(n):
        t = time.perf_counter(); f(); out.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(out), 2)


def main():
    import torch
    import methyldackel_amd as mdk
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    n, rep = a.rows, 1 if a.once else a.repeat
    g = torch.Generator(device="cuda").manual_seed(1)
    start = (torch.arange(n, device="cuda", dtype=torch.int64) * 100 + torch.randint(0, 99, (n,), device="cuda", generator=g)).to(torch.int32)      # a CpG per ~100 bases: 420 Mb
    m, u = torch.randint(0, 40, (n,), device="cuda", generator=g).to(torch.int32), torch.randint(1, 40, (n,), device="cuda", generator=g).to(torch.int32)
    zero8, one8 = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.ones(n, dtype=torch.int8, device="cuda")
    contig = torch.zeros(n, dtype=torch.int32, device="cuda")
    calls = mdk.Calls(["chr1"], {"contig": contig, "start": start, "end": start + 1, "nmeth": m, "nunmeth": u, "context": zero8, "strand": one8}, contexts_on=(0,))
    cyto = mdk.Cytosines(["chr1"], {"contig": contig, "pos": start + 1, "strand": one8, "nmeth": m, "nunmeth": u, "context": zero8,
                                    "trinucleotide": torch.tensor(list(b"CGA"), dtype=torch.uint8, device="cuda").repeat(n, 1).contiguous()})
    cyto.contexts_on = (0,)
    with tempfile.TemporaryDirectory() as d:
        if not a.once:
            calls.write("w", directory=d, compress=True, index=True); cyto.write("w", directory=d, compress=True, index=True)       # warm: libraries, code objects, buffers
        out = {"rows": n}
        out["write_gz_ms"] = median_ms(lambda: calls.write("a", directory=d, compress=True), rep)
        out["write_gz_tbi_ms"] = median_ms(lambda: calls.write("b", directory=d, compress=True, index=True), rep)
        bed = os.path.join(d, "b_CpG.bedGraph.gz")
        out["text_bytes"], out["gz_bytes"], out["tbi_bytes"] = None, os.path.getsize(bed), os.path.getsize(bed + ".tbi")
        tbi = open(bed + ".tbi", "rb").read()
        out["tabix_index_ms"] = median_ms(lambda: mdk.tabix_index(bed, "bed", skip=1), rep)
        assert open(bed + ".tbi", "rb").read() == tbi
        rep_path = cyto.write("c", directory=d, compress=True, index=True)
        out["report_gz_bytes"] = os.path.getsize(rep_path)
        whole = [None]
        out["read_whole_ms"] = median_ms(lambda: whole.__setitem__(0, mdk.Cytosines.read(rep_path, ["chr1"])), rep)
        part = [None]
        out["read_region_1mb_ms"] = median_ms(lambda: part.__setitem__(0, mdk.Cytosines.read(rep_path, ["chr1"], region=("chr1", 200000000, 201000000))), rep)
        w, p = whole[0], part[0]
        keep = (w.pos - 1 < 201000000) & (w.pos > 200000000)
        assert torch.equal(p.pos, w.pos[keep]) and torch.equal(p.nmeth, w.nmeth[keep]) and len(p) > 5000
        out["region_rows"], out["members_inflated"] = len(p), p.members_inflated
        import gzip
        out["text_bytes"] = sum(len(x) for x in iter(lambda f=gzip.open(bed, "rb"): f.read(1 << 24), b""))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
