"""CPU: the deflate stream zoo (tests/deflate_zoo.py) that tests/test_gpu_inflate.py sends to k_inflate and k_crc32 -- the auditor against zlib,
the zoo's coverage of the kernel's regimes (asserted through the auditor, so that an edit of the builder cannot drop one quietly), and the
shared decoder (tools/inflate_emu: csrc/mdk_inflate_core.h and the kernel's 64-lane phases on the host) on the very members and the very
malformed set the GPU test uses."""
import json
import subprocess
import zlib

import pytest

import deflate_zoo as Z
from conftest import REPO

EMU = REPO / "tools" / "_build" / "inflate_emu"


@pytest.fixture(scope="module")
def zoo():
    return Z.build_zoo()


@pytest.fixture(scope="module")
def audits(zoo):
    return {m.name: Z.audit(m.stream) for m in zoo}


def test_auditor_bytes_equal_zlib(zoo, audits):
    for m in zoo:
        a = audits[m.name]
        assert a["bytes"] == zlib.decompress(m.stream, -15) == m.raw, m.name
        assert a["end_bit"] <= 8 * len(m.stream) < a["end_bit"] + 8, m.name


def test_auditor_refuses_the_malformed_set():
    for name, stream, out_len in Z.malformed():
        try:
            got = Z.audit(stream)["bytes"]
        except Z.StreamError:
            continue
        assert len(got) != out_len, name


def test_zoo_covers_every_regime(zoo, audits):
    A = audits.values()
    has = lambda f: [n for n, a in audits.items() if f(a)]      # noqa: E731
    need = {
        "stored blocks": has(lambda a: 0 in a["types"]),
        "fixed-Huffman blocks": has(lambda a: 1 in a["types"]),
        "dynamic blocks": has(lambda a: 2 in a["types"]),
        "many blocks per member (>= 100)": has(lambda a: a["n_blocks"] >= 100),
        "empty stored block inside a member (sync / full flush)": has(lambda a: 0 in a["empty_blocks"] and a["n_blocks"] > 1),
        "empty fixed block (partial flush)": has(lambda a: 1 in a["empty_blocks"]),
        "empty dynamic block": has(lambda a: 2 in a["empty_blocks"]),
        "a block that starts in the middle of a byte": has(lambda a: a["midbyte_block_start"]),
        "15-bit literal/length code decoded": has(lambda a: a["max_lit_len"] == 15),
        "long literal/length codes (11..15 bits) from zlib": [n for n in has(lambda a: a["max_lit_len"] > 10) if not n.startswith("writer_")],
        "distance code longer than the table's 8 bits": has(lambda a: a["max_dist_len"] > 8),
        "15-bit distance code decoded": has(lambda a: a["max_dist_len"] == 15),
        "a distance tree of one code of length 1": has(lambda a: a["single_dist_len1"]),
        "a distance tree of one zero length (literals only)": has(lambda a: a["dist_tree_zero"]),
        "an end-of-block code alone, one bit": has(lambda a: a["eob_only_1bit"]),
        "run-length codes 16, 17 and 18 in one header": has(lambda a: a["cl_runs"] == {16, 17, 18}),
        "distance 32768": has(lambda a: a["max_dist"] == 32768),
        "distances 32507..32768": has(lambda a: a["dist_32507"] >= 10),
        "length 258 at distance 32768": has(lambda a: a["m258_32768"]),
        "a match reaching exactly to byte 0": has(lambda a: a["match_to_byte0"]),
        "a match across a block boundary": has(lambda a: a["match_across_block"]),
        "matches at distances > 4096": has(lambda a: a["far_4096"] >= 100),
        "more than 256 symbols in one 608-bit stretch": has(lambda a: a["max_syms_per_stretch"] > Z.TOK_STEPS),
    }
    for d in (1, 2, 3):
        need[f"length 258 at distance {d}"] = has(lambda a, d=d: d in a["m258_dists"])
    zlib_only = lambda f: [n for n in has(f) if not n.startswith(("writer_", "libdeflate"))]      # noqa: E731
    for edge in (2048, 4096):
        need[f"zlib distances just below {edge}"] = zlib_only(lambda a, e=edge: any(e - 8 <= d < e for d in a["dists"]))
        need[f"zlib distance {edge}"] = zlib_only(lambda a, e=edge: e in a["dists"])
        need[f"zlib distances just above {edge}"] = zlib_only(lambda a, e=edge: any(e < d <= e + 8 for d in a["dists"]))
    need["zlib distances of about 32000"] = zlib_only(lambda a: a["max_dist"] >= 31990)
    for n in (0, 1, 511, 512, 513, 65535):
        need[f"a stored block of {n} bytes"] = has(lambda a, n=n: n in a["stored_sizes"])
    missing = [k for k, v in need.items() if not v]
    assert not missing, missing
    names = [m.name for m in zoo]
    for want in ("sync_flush", "full_flush", "partial_flush", "block_flush", "match_across_sync_flush", "many_blocks_memlevel1"):
        assert want in names
    assert audits["match_across_sync_flush"]["match_across_block"] and 0 in audits["match_across_sync_flush"]["empty_blocks"]
    assert audits["block_flush"]["midbyte_block_start"]
    sizes = {len(m.raw) for m in zoo}
    assert set(Z.SIZES) <= sizes, set(Z.SIZES) - sizes
    for lv, stg, wb, ml in Z.ENCODERS:
        assert any(n.endswith(f"_l{lv}_{Z.STRAT[stg]}_w{-wb}_m{ml}") for n in names), (lv, stg, wb, ml)
    for kind in ("u128", "u240"):
        for s in ("huff", "fixed", "def"):
            assert f"{kind}_65280_{s}" in names
    assert any(n.startswith("bam_") for n in names)
    assert max(a["n_blocks"] for a in A) > 1


def test_zoo_has_libdeflate_members(zoo):
    """libdeflate's members are left out of the zoo only where the library is missing, and then visibly"""
    if not Z.libdeflate():
        pytest.skip("libdeflate.so.0 is not on this machine: the zoo has no libdeflate members")
    names = {m.name for m in zoo}
    for lv in (1, 6, 9, 12):
        assert {f"libdeflate{lv}_{k}" for k in ("acgt", "mid", "maxdist", "u240", "skew", "bam", "1")} <= names


def test_piece_layout_takes_every_alignment(zoo):
    items = [(m.stream, len(m.raw), zlib.crc32(m.raw)) for m in zoo]
    for order in (items, items[::-1]):
        comp, tab = Z.piece_layout(order)
        assert {t[0] % 4 for t in tab} == {0, 1, 2, 3}
        assert {t[3] % 16 for t in tab} == set(range(16))
        assert tab[-1][0] + tab[-1][1] == len(comp) and len(comp) % 4
        for (s, n, c), (io, il, ol, oo, cc) in zip(order, tab):
            assert comp[io:io + il] == s and ol == n and cc == c


def emu_each(tmp_path, items, name):
    f = tmp_path / name
    f.write_bytes(Z.bgzf_file(items))
    r = subprocess.run([str(EMU), "--each", str(f)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)["rc"]


def test_emulator_inflates_the_zoo(zoo, tmp_path):
    """the zoo as one BGZF file with right trailers (minus the streams too long for a frame): the shared decoder on what the GPU sees"""
    items = [(m.stream, len(m.raw), zlib.crc32(m.raw)) for m in zoo if len(m.stream) <= Z.BGZF_MAX_STREAM]
    assert all(len(m.raw) >= 65000 for m in zoo if len(m.stream) > Z.BGZF_MAX_STREAM)
    f = tmp_path / "zoo.bam"
    f.write_bytes(Z.bgzf_file(items))
    r = subprocess.run([str(EMU), str(f)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    st = json.loads(r.stdout)
    assert st["mismatching_members"] == 0 and st["members"] == len(items) + 1
    assert st["batches_cut_by_passes"] > 0, st          # the pass cap (uniform 7-bit codes)
    assert st["far_bytes"] > 0, st                      # sources older than the LDS ring, from global memory
    assert st["chain_passes_hist"][-1] > 0, st          # batches that ran to the last pass (INF_MAX_PASSES)
    assert all(rc == 0 for rc in emu_each(tmp_path, items, "each.bam"))


def test_emulator_refuses_the_malformed_set(zoo, tmp_path):
    """the GPU test's malformed members, each between the same good ones (Z.AROUND_MALFORMED, none of them empty): refused, and the good ones
    on either side still inflate to zlib's bytes (the decoder's state is kept from one member to the next)"""
    good = [(m.stream, len(m.raw), zlib.crc32(m.raw)) for m in Z.around_malformed(zoo)]
    assert len(good) == 6 and all(n >= 1000 and len(s) <= Z.BGZF_MAX_STREAM for s, n, _ in good)
    bad = Z.malformed()
    items = []
    for name, stream, out_len in bad:
        items += good[:3] + [(stream, out_len, 0)] + good[3:]
    rc = emu_each(tmp_path, items, "bad.bam")
    assert len(rc) == 7 * len(bad) + 1
    for k, (name, _, _) in enumerate(bad):
        assert rc[7 * k + 3] > 0, (name, rc[7 * k + 3])
        assert rc[7 * k:7 * k + 3] == [0, 0, 0] and rc[7 * k + 4:7 * k + 7] == [0, 0, 0], (name, rc[7 * k:7 * k + 7])
