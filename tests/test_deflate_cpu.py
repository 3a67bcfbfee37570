"""The BGZF compressor on the host (no GPU): tools/deflate_emu is csrc/mdk_deflate_core.h in the decomposition of k_deflate
(csrc/mdk_deflate.hip), so what holds for its bytes holds for the device's, which tests/test_gpu_deflate.py compares with them byte for byte.
zlib is the reference: every stream must inflate to its slice of the input; tools/inflate_emu -- the device's own inflater on the host -- must
inflate the files too, which closes the loop without a GPU."""
import json
import subprocess
import zlib

import pytest

import bgzf_cases as B
import deflate_zoo as Z


@pytest.fixture(scope="module")
def built():
    assert B.EMU.exists() and B.INFLATE_EMU.exists(), "make tools"


@pytest.mark.parametrize("kind", B.KINDS)
def test_every_size_of_a_content(built, kind, tmp_path):
    seen = set()
    for n in B.SIZES:
        data = B.content(kind, n)
        assert len(data) == n
        out = B.emu(data)
        assert out == B.emu(data), (kind, n, "two runs differ")
        audits = B.check_file(out, data)
        for a in audits:
            seen |= a["types"]
        if kind == "random":
            assert len(out) == n + 31 * len(audits) + 28 and all(a["types"] == {0} for a in audits), (kind, n)
        if kind == "A" and n >= 65280:
            assert all(1 in a["m258_dists"] for a in audits if len(a["bytes"]) > 300), (kind, n)      # length-258 matches at distance 1
        if kind.startswith("period") and n >= 65280:
            period = int(kind[6:])
            far = max(a["max_dist"] for a in audits)
            assert far == period if period <= 32768 else far < 32768, (kind, n, far)      # 32769 is out of reach: nothing may point that far
        # the device's own inflater (k_inflate's phases on the host) reads the file: every member equals zlib's bytes
        f = tmp_path / f"{kind}_{n}.gz"
        f.write_bytes(out)
        r = subprocess.run([str(B.INFLATE_EMU), str(f)], capture_output=True, text=True)
        assert r.returncode == 0, (kind, n, r.stderr[-300:])
        rep = json.loads(r.stdout)
        assert rep["mismatching_members"] == 0 and rep["inflated_bytes"] == n, (kind, n, rep)
        assert B.emu(data, eof=False) == out[:-28]
    if kind in ("bedgraph", "rotation", "A", "edge_match"):
        assert 2 in seen, seen                  # a dynamic block


def test_last_match_ends_on_the_members_last_byte(built):
    for n in (4096, 65280, 2 * 65280 + 1):
        data = B.content("edge_match", n)
        out = B.emu(data)
        for i, (io, il, isz, _) in enumerate(Z.bgzf_members(out)[:-1]):
            if isz >= 200:
                toks = _tokens(out[io:io + il])
                assert sum(t[0] if t[0] >= 3 else 1 for t in toks) == isz
                assert toks[-1][0] >= 36 and toks[-1][1] == 48, (n, i, toks[-3:])           # the last token is a match: it ends on the member's last byte


def _tokens(stream):
    """[(length, distance)] (a literal: (0, 0)) of a one-block stream, by the zoo's tables"""
    a = Z.audit(stream)
    assert a["n_blocks"] == 1
    out, pos, bits = [], [a["blocks"][0][1] + 3], int.from_bytes(stream, "little")

    def take(n):
        v = (bits >> pos[0]) & ((1 << n) - 1); pos[0] += n
        return v
    btype = a["blocks"][0][0]
    if btype == 0:
        return []
    if btype == 1:
        lit_lens, dist_lens = Z.FIXED_LIT, Z.FIXED_DIST
    else:
        nlit, ndist, ncode = take(5) + 257, take(5) + 1, take(4) + 4
        cll = [0] * 19
        for k in range(ncode):
            cll[Z.CLORD[k]] = take(3)
        cmx, ct = Z._table(cll)
        seq = []
        while len(seq) < nlit + ndist:
            s, l = ct[(bits >> pos[0]) & ((1 << cmx) - 1)]; pos[0] += l
            if s < 16:
                seq.append(s)
            elif s == 16:
                seq += [seq[-1]] * (3 + take(2))
            else:
                seq += [0] * ((3 + take(3)) if s == 17 else (11 + take(7)))
        lit_lens, dist_lens = seq[:nlit], seq[nlit:]
    lmx, lt = Z._table(lit_lens); dmx, dt = Z._table(dist_lens)
    while True:
        s, l = lt[(bits >> pos[0]) & ((1 << lmx) - 1)]; pos[0] += l
        if s == 256:
            return out
        if s < 256:
            out.append((0, 0)); continue
        n = Z.LBASE[s - 257] + take(Z.LEXT[s - 257])
        ds, dl = dt[(bits >> pos[0]) & ((1 << dmx) - 1)]; pos[0] += dl
        out.append((n, Z.DBASE[ds] + take(Z.DEXT[ds])))


def test_matches_and_fitted_codes_beat_fitted_codes_alone(built):
    """20,000 seeded bedGraph lines in 65280-byte members: the file is no larger than the same members compressed by zlib with
    Z_HUFFMAN_ONLY (plus 26 bytes of frame each).  zlib level 1 passes that bound with room (asserted: the bound is one a real encoder with
    matches meets).  Measured here: deflate_emu 3.12x, zlib level 1 2.80x, level 6 3.67x, Z_HUFFMAN_ONLY 2.11x."""
    data = B.bedgraph(20000)
    bound = B.zlib_members_size(data, level=6, strategy=zlib.Z_HUFFMAN_ONLY)
    level1 = B.zlib_members_size(data, level=1)
    level6 = B.zlib_members_size(data, level=6)
    out = B.emu(data)
    B.check_file(out, data)
    print(f"text {len(data)}; deflate_emu {len(out)} ({len(data) / len(out):.2f}x); zlib level 1 {level1} ({len(data) / level1:.2f}x); level 6 {level6} "
          f"({len(data) / level6:.2f}x); Z_HUFFMAN_ONLY {bound} ({len(data) / bound:.2f}x)")
    assert level1 + 28 <= bound, (level1, bound)
    assert len(out) <= bound, (len(out), bound)
