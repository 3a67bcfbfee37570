"""The times DESIGN.md quotes beside tools/profile_bench for the alternative a user had before `count_profile`: the same five tensors
composed in torch, per sample and group -- `bincount` of the clamped depth, `bincount` of the level bin, the masked sums and the masked
maximum --, on seeded [S, 2^22] int32 tables with the concentration of a real library (depths Poisson around 10, a tenth of the cells
uncovered, levels bimodal), S = 1, 6, 12 and 96, G = 1 and 3 -- and `mdk.count_profile` on the same tensors, in the same process.
Medians of warm calls, host clock around calls that end with a device synchronisation; the peak of torch's allocator over the
composition, and whether its tensors equal the kernel's (they must: both are exact).  One JSON line."""
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
    depth = torch.poisson(torch.full((S, n), 10.0, device="cuda"), generator=g).to(torch.int32)
    depth *= (torch.rand((S, n), device="cuda", generator=g) >= 0.1)
    kind = torch.rand((S, n), device="cuda", generator=g)
    m = (torch.rand((S, n), device="cuda", generator=g) * (depth + 1)).to(torch.int32).clamp_(max=depth)
    m = torch.where(kind < 0.4, depth, torch.where(kind < 0.7, torch.zeros_like(m), m))
    group = torch.bucketize(torch.rand(n, device="cuda", generator=g), torch.tensor([1 / 16, 4 / 16], device="cuda")).to(torch.uint8)
    return m.contiguous(), (depth - m).contiguous(), group.contiguous()


def by_torch(m, u, group, G, min_depth=1, B=1024, L=20):
    """the five tensors composed per sample and group"""
    import torch
    S = m.shape[0]
    dh, lh = torch.zeros((S, G, B + 1), dtype=torch.int64, device=m.device), torch.zeros((S, G, L), dtype=torch.int64, device=m.device)
    ms, us, mx = (torch.zeros((S, G), dtype=torch.int64, device=m.device) for _ in range(3))
    masks = [None] if group is None else [group == k for k in range(G)]
    for s in range(S):
        a, b = m[s].long(), u[s].long()
        d = a + b
        covered = d >= min_depth
        level = torch.clamp(a * L // d.clamp(min=1), max=L - 1)
        for k, mask in enumerate(masks):
            dk = d if mask is None else d[mask]
            dh[s, k] = torch.bincount(dk.clamp(max=B), minlength=B + 1)
            mx[s, k] = dk.max() if dk.numel() else 0
            c = covered if mask is None else covered & mask
            lh[s, k] = torch.bincount(level[c], minlength=L)
            ms[s, k], us[s, k] = a[c].sum(), b[c].sum()
    return dh, lh, ms, us, mx


def main():
    import torch
    import methyldackel_amd as mdk
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--samples", default="1,6,12,96")
    ap.add_argument("--groups", default="1,3")
    ap.add_argument("--log2-sites", type=int, default=22)
    a = ap.parse_args()
    n = 1 << a.log2_sites
    out = {"repeat": a.repeat, "sites": n, "shapes": []}
    for k, S in enumerate(int(v) for v in a.samples.split(",")):
        m, u, group = table(S, n, 20261020 + k)
        for G in (int(v) for v in a.groups.split(",")):
            g = group if G > 1 else None
            r = {"samples": S, "groups": G}
            p = mdk.count_profile(m, u, g, G)                         # warm: the library, the code object, the handle
            r["count_profile_ms"] = median_ms(lambda: mdk.count_profile(m, u, g, G), a.repeat)
            got = by_torch(m, u, g, G)
            torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            r["torch_ms"] = median_ms(lambda: by_torch(m, u, g, G), a.repeat if S < 64 else 2)
            r["torch_peak_bytes_over_table"] = round((torch.cuda.max_memory_allocated() - base) / (2 * m.numel() * m.element_size()), 2)
            r["torch_equals_kernel"] = all(bool(torch.equal(x, y)) for x, y in zip(got, (p.depth_hist, p.level_hist, p.nmeth_sum, p.nunmeth_sum, p.max_depth)))
            r["ratio"] = round(r["torch_ms"] / r["count_profile_ms"], 2)
            out["shapes"].append(r)
            del got, p
        del m, u, group
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
