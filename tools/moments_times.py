"""The times DESIGN.md quotes beside tools/moments_bench for the alternative a user had before `sample_moments`: the four Gram products
as float64 matrix products in torch, on seeded [S, 2^22] int32 tables (depths 1 to 30, a tenth of the cells uncovered), S = 2, 12, 96 and
1024 -- the float64 copies made first (levels x, the mask c, x^2), then c c^T, x c^T, x^2 c^T and x x^T --, and `mdk.sample_moments` on
the same tensors.  Medians of warm calls, host clock around calls that end with a device synchronisation; the peak of torch's allocator
over the matmul formulation, and whether its sums equal the exact ones (they need not: they pass 2^53).  One JSON line."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def median_ms(f, n):
    import torch
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter(); f(); torch.cuda.synchronize(); out.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(out), 3)


def table(S, n, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    depth = torch.randint(1, 31, (S, n), device="cuda", generator=g, dtype=torch.int32)
    depth *= (torch.rand((S, n), device="cuda", generator=g) >= 0.1)
    m = (torch.rand((S, n), device="cuda", generator=g) * (depth + 1)).to(torch.int32).clamp_(max=depth)
    return m.contiguous(), (depth - m).contiguous()


def by_matmul(m, u, min_depth=1):
    """the four sums as float64 matrix products"""
    import torch
    d = (m + u).double()
    c = (d >= min_depth).double()
    x = torch.where(c > 0, torch.floor((2.0 * 65536.0 * m.double() + d) / (2.0 * d).clamp_(min=1.0)), torch.zeros_like(d))
    ct = c.t()
    return c @ ct, x @ ct, (x * x) @ ct, x @ x.t()


def main():
    import torch
    import methyldackel_amd as mdk
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--samples", default="2,12,96,1024")
    ap.add_argument("--log2-sites", type=int, default=22)
    a = ap.parse_args()
    n = 1 << a.log2_sites
    out = {"repeat": a.repeat, "sites": n, "shapes": []}
    for k, S in enumerate(int(v) for v in a.samples.split(",")):
        m, u = table(S, n, 20261020 + k)
        r = {"samples": S}
        mo = mdk.sample_moments(m, u)                                # warm: the library, the code object, the handle
        rep = a.repeat if S < 512 else 2
        r["sample_moments_ms"] = median_ms(lambda: mdk.sample_moments(m, u), rep)
        try:
            got = by_matmul(m, u)
            torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            r["matmul_ms"] = median_ms(lambda: by_matmul(m, u), rep)
            r["matmul_peak_bytes_over_table"] = round((torch.cuda.max_memory_allocated() - base) / (2 * m.numel() * m.element_size()), 2)
            r["matmul_sums_exact"] = [bool(torch.equal(g.to(torch.int64), e)) for g, e in zip(got, (mo.n, mo.sx, mo.sxx, mo.sxy))]
            r["ratio"] = round(r["matmul_ms"] / r["sample_moments_ms"], 2)
            del got
        except torch.OutOfMemoryError as e:
            r["matmul_error"] = str(e)[:120]
        out["shapes"].append(r)
        del m, u, mo
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
