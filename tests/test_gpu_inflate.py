"""GPU tests of the device BGZF inflate (include/mdk_hip.h md_piece_*, csrc/mdk_inflate.hip):
  * C-ABI level: every member of a piece inflates byte-identical to zlib, the record table equals a walk of the records, the
    member digests equal what a walk computes (this is what csrc/host/mdk_io.c note_records leaves for host-inflated slabs);
  * command level: `MethylDackel extract` with every piece but the header's inflated on the device (MDK_DEVICE_INFLATE_ONLY=1)
    must produce the oracle's bytes, over chunk sizes far below a member's span (a member then serves many chunks), regions
    through the index, dense contexts, --mergeContext, a file whose records straddle BGZF members (read back to the host) and a
    chunk the device preparation hands back to the host (its records exist only on the device);
  * the deflate stream zoo (tests/deflate_zoo.py: every zlib level / strategy / memLevel / window, flushes, libdeflate, hand-written blocks)
    as pieces against zlib, k_crc32 at every length edge and alignment with one CRC bit flipped at a time, malformed members refused with
    the emulator's error code, and BAMs re-encoded by other encoders through the command against the oracle."""
import ctypes as C
import struct
import warnings
import zlib

import pytest

import deflate_zoo as Z
import methyldackel_amd as mdk
from conftest import REPO, synth
from test_gpu_parity import compare_cli

pytestmark = pytest.mark.gpu


CRCS = {}            # deflate stream offset -> CRC32 of the member's trailer (filled by bgzf_members)


def bgzf_members(raw):
    out, o = [], 0
    while o + 18 <= len(raw):
        xlen = struct.unpack_from("<H", raw, o + 10)[0]
        bs = struct.unpack_from("<H", raw, o + 16)[0] + 1
        isz = struct.unpack_from("<I", raw, o + bs - 4)[0]
        out.append((o + 12 + xlen, bs - 12 - xlen - 8, isz))
        CRCS[o + 12 + xlen] = struct.unpack_from("<I", raw, o + bs - 8)[0]
        o += bs
    return out


def walk(data):
    """records of one inflated member -> (offsets, digest) or None when it does not start and end on record boundaries"""
    offs, o, L = [], 0, len(data)
    tid0 = pos0 = tidN = posN = -1; mn, mx, srt = 0x7fffffff, -0x80000000, 1
    while o + 4 <= L:
        bs = struct.unpack_from("<I", data, o)[0]
        if bs < 32 or o + 4 + bs > L:
            return None
        tid, pos = struct.unpack_from("<ii", data, o + 4)
        lq, nc = data[o + 12], struct.unpack_from("<H", data, o + 16)[0]
        if 32 + lq + 4 * nc > bs:
            return None
        rl = 0
        for k in range(nc):
            v = struct.unpack_from("<I", data, o + 36 + lq + 4 * k)[0]
            if (v & 15) in (0, 2, 3, 7, 8):
                rl += v >> 4
        endp = pos + (rl if rl > 0 else 1)
        if not offs:
            tid0, pos0 = tid, pos
        elif tid < 0 or tid < tidN or (tid == tidN and pos < posN):
            srt = 0
        if tid < 0:
            srt = 0
        tidN, posN = tid, pos; mn, mx = min(mn, endp), max(mx, endp)
        offs.append(o); o += 4 + bs
    if o != L:
        return None
    return offs, (len(offs), tid0, pos0, tidN, posN, mn, mx, srt)


def test_piece_inflate_equals_zlib_and_record_walk(tmp_path):
    synth(tmp_path / "s", "-L", "400000", "-c", "30", "-s", "77", "--extras")
    raw = (tmp_path / "s.bam").read_bytes()
    mem = bgzf_members(raw)
    L = mdk.lib_hip()
    cfg = mdk.md_dev_cfg(); cfg.keepCpG = 1; cfg.minPhred = 5
    dev = mdk.Device(cfg)
    L.md_host_alloc.restype = C.c_void_p
    stage = L.md_host_alloc(C.c_uint64(len(raw) + 64)); C.memmove(stage, raw, len(raw))
    tab = (mdk.md_inf_member * len(mem))(); o = 0
    for i, (io, il, isz) in enumerate(mem):
        tab[i].in_off, tab[i].in_len, tab[i].out_len, tab[i].out_off, tab[i].crc32 = io, il, isz, o, CRCS[io]; o += isz
    piece = C.c_void_p(); info = mdk.md_piece_info()
    assert L.md_piece_create(dev.h, C.byref(piece)) == 0, L.md_dev_last_error()
    for variant_pass in range(2):       # twice: the second submit reuses the piece's buffers
        assert L.md_piece_submit(piece, C.c_void_p(stage), len(raw), tab, len(mem)) == 0, L.md_dev_last_error()
        assert L.md_piece_wait(piece, C.byref(info)) == 0, L.md_dev_last_error()
        assert info.n_mem == len(mem) and info.out_bytes == o
        got = C.create_string_buffer(o)
        assert L.md_piece_read(piece, 0, o, got) == 0
        recs = (C.c_uint32 * max(1, info.n_records))()
        assert L.md_piece_read_records(piece, 0, info.n_records, recs) == 0
        first = 0
        for i, (io, il, isz) in enumerate(mem):
            ref = zlib.decompress(raw[io:io + il], wbits=-15) if isz else b""
            assert len(ref) == isz and got.raw[tab[i].out_off:tab[i].out_off + isz] == ref, f"member {i}"
            w = walk(ref); g = info.digest[i]
            assert g.first_rec == first
            if w is None:               # the member holding the BAM header (and the records behind it in the same member)
                assert g.ok == 0 and g.n_rec == 0
                continue
            assert g.ok == 1
            offs, dg = w
            assert (g.n_rec, ) + ((g.tid0, g.pos0, g.tidN, g.posN, g.min_endp, g.max_endp, g.sorted) if offs else ()) == (dg[0], ) + (dg[1:] if offs else ())
            assert [recs[first + k] for k in range(len(offs))] == [tab[i].out_off + x for x in offs]
            first += len(offs)
        assert first == info.n_records
    L.md_piece_destroy(piece); L.md_host_free(C.c_void_p(stage)); dev.close()


DEV = {"MDK_DEVICE_INFLATE_ONLY": "1", "MDK_GPU_PIECE_MB": "3", "MDK_HOST_PROFILE": "1"}      # test hooks (csrc/host/mdk_io.c): the host teams leave after the header, small device pieces


@pytest.fixture(scope="module")
def mid_synth(tmp_path_factory):
    d = tmp_path_factory.mktemp("inflate")
    synth(d / "pe", "-L", "1500000,700000", "-c", "25", "-s", "31", "--extras")
    return d


@pytest.mark.parametrize("extra", [[], ["--chunkSize", "7000"], ["--chunkSize", "250000", "--CHG", "--CHH"], ["--mergeContext", "--chunkSize", "90000"],
                                   ["-r", "chr2:100000-420000"], ["--minOppositeDepth", "3", "--maxVariantFrac", "0.2", "--chunkSize", "333333"], ["--keepDupes", "--keepSingleton", "--keepDiscordant", "-q", "0"]])
def test_cli_with_device_inflate_equals_oracle(mid_synth, tmp_path, extra):
    od, gd = compare_cli(tmp_path, [str(mid_synth / "pe.fa"), str(mid_synth / "pe.bam")] + extra, env=DEV)


def test_device_pieces_were_used(mid_synth, tmp_path):
    r = mdk.run_cli([str(mid_synth / "pe.fa"), str(mid_synth / "pe.bam"), "-o", "out"], cwd=tmp_path, env=DEV)
    assert r.returncode == 0, r.stderr
    line = [l for l in r.stderr.splitlines() if "on the device" in l]
    assert line, r.stderr[-2000:]
    n_dev = int(line[0].split("on the device ")[1].split()[0])
    assert n_dev >= 1


def test_records_straddling_members_are_read_back(tmp_path):
    """a BAM whose BGZF members are cut at arbitrary bytes (legal BGZF, never written by htslib): the device's walk reports members that
    do not start on a record, the slab comes back to the host and is scanned there"""
    synth(tmp_path / "s", "-L", "300000", "-c", "20", "-s", "5")
    raw = (tmp_path / "s.bam").read_bytes()
    data = b"".join(zlib.decompress(raw[io:io + il], wbits=-15) for io, il, isz in bgzf_members(raw) if isz)
    out, o = bytearray(), 0
    while o < len(data):
        blk = data[o:o + 40001]; o += len(blk)
        c = zlib.compressobj(6, zlib.DEFLATED, -15); comp = c.compress(blk) + c.flush()
        out += struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(blk), len(blk))
    out += bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    (tmp_path / "cut.bam").write_bytes(bytes(out))
    compare_cli(tmp_path, [str(tmp_path / "s.fa"), str(tmp_path / "cut.bam")], env=DEV)


def test_chunk_handed_back_to_the_host_with_device_resident_records(tmp_path):
    """20 records of one read name in a chunk: the device preparation gives the chunk up (MDK_ERR_PREP_HOST); its records were
    inflated on the device, so they are read back for the host preparation"""
    import random
    from bamwriter import record, write_fasta
    rnd = random.Random(3)
    ref = "".join(rnd.choice("ACGT") for _ in range(30000))
    write_fasta(tmp_path / "r.fa", [("chrA", ref)])
    recs = []
    for i in range(6000):
        pos = rnd.randrange(0, 29800)
        dup = i % 300 == 0          # 20 records of one name, paired flags: the name's chain is walked (a lane keeps 16) -> the chunk goes back to the host
        recs.append((pos, record(0, pos, 0x43 if dup else 0, "100M", ref[pos:pos + 100], 30, qname="dup" if dup else f"r{i}")))
    recs.sort(key=lambda r: r[0])
    text = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chrA\tLN:30000\n"
    hdr = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chrA\0" + struct.pack("<i", 30000)
    out, blk = bytearray(), bytearray()

    def flush():
        nonlocal blk
        if blk:
            c = zlib.compressobj(6, zlib.DEFLATED, -15); comp = c.compress(bytes(blk)) + c.flush()
            out.extend(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(bytes(blk)), len(blk)))
            blk = bytearray()
    blk += hdr; flush()                 # the header in a member of its own, then members that end on record boundaries
    for _, r in recs:
        if len(blk) + len(r) > 50000:
            flush()
        blk += r
    flush()
    out += bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    (tmp_path / "r.bam").write_bytes(bytes(out))
    od, gd = compare_cli(tmp_path, [str(tmp_path / "r.fa"), str(tmp_path / "r.bam"), "-q", "0"], env=dict(DEV, MDK_HOST_PROFILE="1"))
    assert fell_back(tmp_path) >= 1, "the chunk was expected to fall back to the host preparation"


def fell_back(tmp_path):
    """chunks the command prepared on the host after all (MDK_HOST_PROFILE line of extract_main)"""
    import re
    m = re.search(r"chunks prepared on the host after all: (\d+)", (tmp_path / "gpu_stderr.txt").read_text())
    return int(m.group(1)) if m else -1


def test_handed_back_chunks_drop_the_neighbours_records(tmp_path):
    """The same with two contigs and chunks smaller than a BGZF member's span: the members read back for a handed-back chunk also hold
    the records of the neighbouring chunks and -- the member that straddles the contig boundary -- of the other contig; the host
    preparation must redo the chunk's region query on them (chrB is short: its single chunk starts at 0, where chrA's reads would
    otherwise be counted at chrB's coordinates)."""
    import random
    from bamwriter import record, write_fasta
    rnd = random.Random(5)
    refs = [("chrA", "".join(rnd.choice("ACGT") for _ in range(30000))), ("chrB", "".join(rnd.choice("ACGT") for _ in range(2500)))]
    write_fasta(tmp_path / "r.fa", refs)
    recs = []
    for tid, (_, ref) in enumerate(refs):
        n = 6000 if tid == 0 else 900
        for i in range(n):
            pos = rnd.randrange(0, len(ref) - 120)
            dup = i % 10 == 0
            recs.append((tid, pos, record(tid, pos, 0x43 if dup else 0, "100M", ref[pos:pos + 100], 30, qname=f"dup{tid}" if dup else f"r{tid}_{i}")))
    recs.sort(key=lambda r: (r[0], r[1]))
    text = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chrA\tLN:30000\n@SQ\tSN:chrB\tLN:2500\n"
    hdr = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", 2) + struct.pack("<i", 5) + b"chrA\0" + struct.pack("<i", 30000) + struct.pack("<i", 5) + b"chrB\0" + struct.pack("<i", 2500)
    out, blk = bytearray(), bytearray()

    def flush():
        nonlocal blk
        if blk:
            c = zlib.compressobj(6, zlib.DEFLATED, -15); comp = c.compress(bytes(blk)) + c.flush()
            out.extend(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(bytes(blk)), len(blk)))
            blk = bytearray()
    blk += hdr; flush()
    for _, _, r in recs:                  # members end on record boundaries, wherever the contig changes
        if len(blk) + len(r) > 50000:
            flush()
        blk += r
    flush()
    out += bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    (tmp_path / "r.bam").write_bytes(bytes(out))
    od, gd = compare_cli(tmp_path, [str(tmp_path / "r.fa"), str(tmp_path / "r.bam"), "-q", "0", "--chunkSize", "2000"], env=dict(DEV, MDK_HOST_PROFILE="1"))
    assert fell_back(tmp_path) >= 2


def stored_members_bam(raw, flip_member=None):
    """the same BAM with every member re-written as STORED deflate blocks (level 0); optionally one payload byte of one member flipped, the
    member's CRC32 and ISIZE left as they were: it still inflates to ISIZE bytes, but not to the bytes the trailer vouches for"""
    out = bytearray()
    for k, (io, il, isz) in enumerate(bgzf_members(raw)):
        data = zlib.decompress(raw[io:io + il], wbits=-15) if isz else b""
        c = zlib.compressobj(0, zlib.DEFLATED, -15); comp = bytearray(c.compress(data) + c.flush())
        if flip_member is not None and k == flip_member:
            assert len(comp) > 40 and isz
            comp[20] ^= 0x5a                  # (5 bytes of stored-block header, then the bytes themselves)
        out += b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + bytes(comp) + struct.pack("<II", zlib.crc32(data), len(data))
    return bytes(out)


def test_a_byte_flipped_inside_a_stored_block_fails_the_crc32_check(tmp_path):
    """What htslib verifies behind sam_itr_next (bgzf_read_block: CRC32 and ISIZE of every block): a damaged byte that raw inflate cannot
    notice must stop the run on the host's inflate path and on the device's (k_crc32), and stops the oracle; the undamaged file passes"""
    synth(tmp_path / "s", "-L", "120000", "-c", "20", "-s", "9")
    raw = (tmp_path / "s.bam").read_bytes()
    (tmp_path / "ok.bam").write_bytes(stored_members_bam(raw))
    (tmp_path / "bad.bam").write_bytes(stored_members_bam(raw, flip_member=7))
    compare_cli(tmp_path, [str(tmp_path / "s.fa"), str(tmp_path / "ok.bam")], env=DEV)
    from conftest import run_oracle
    (tmp_path / "o2").mkdir()
    assert run_oracle([str(tmp_path / "s.fa"), str(tmp_path / "bad.bam"), "-o", "out"], cwd=tmp_path / "o2").returncode != 0
    for name, env in (("device", DEV), ("host", {"MDK_HOST_INFLATE": "1"})):
        d = tmp_path / name; d.mkdir()
        r = mdk.run_cli([str(tmp_path / "s.fa"), str(tmp_path / "bad.bam"), "-o", "out"], cwd=d, env=env)
        assert r.returncode != 0 and "CRC32" in r.stderr, (name, r.returncode, r.stderr[-800:])
        r = mdk.run_cli([str(tmp_path / "s.fa"), str(tmp_path / "bad.bam"), "-o", "out"], cwd=d, env=dict(env, MDK_NO_CRC="1"))
        assert r.returncode == 0, (name, "without the check the damage goes unnoticed", r.stderr[-800:])


# ---- the deflate stream zoo (tests/deflate_zoo.py) through the C ABI: every stream kind the encoders write, against zlib ----
EMU = REPO / "tools" / "_build" / "inflate_emu"


@pytest.fixture(scope="module")
def zoo():
    return Z.build_zoo()


class PieceRig:
    """one device handle and one piece, reused by every submit (buffers grown on demand, then used again at other offsets)"""

    def __init__(self):
        self.L = mdk.lib_hip()
        self.L.md_host_alloc.restype = C.c_void_p
        cfg = mdk.md_dev_cfg(); cfg.keepCpG = 1; cfg.minPhred = 5
        self.dev = mdk.Device(cfg)
        self.piece = C.c_void_p()
        assert self.L.md_piece_create(self.dev.h, C.byref(self.piece)) == 0, self.L.md_dev_last_error()
        self.stage, self.cap = None, 0

    def submit(self, items, seed=1):
        """items: [(stream, out_len, crc)] -> (rc of md_piece_wait, error text, info, member table)"""
        comp, tab = Z.piece_layout(items, seed)
        if len(comp) + 64 > self.cap:
            if self.stage:
                self.L.md_host_free(C.c_void_p(self.stage))
            self.cap = len(comp) + 64 + (1 << 20)
            self.stage = self.L.md_host_alloc(C.c_uint64(self.cap))
        C.memmove(self.stage, comp, len(comp))
        mt = (mdk.md_inf_member * len(tab))()
        for i, (io, il, ol, oo, c) in enumerate(tab):
            mt[i].in_off, mt[i].in_len, mt[i].out_len, mt[i].out_off, mt[i].crc32 = io, il, ol, oo, c
        assert self.L.md_piece_submit(self.piece, C.c_void_p(self.stage), len(comp), mt, len(tab)) == 0, self.L.md_dev_last_error()
        info = mdk.md_piece_info()
        rc = self.L.md_piece_wait(self.piece, C.byref(info))
        return rc, (self.L.md_dev_last_error() or b"").decode(), info, tab

    def read(self, tab):
        n = tab[-1][3] + tab[-1][2]
        got = C.create_string_buffer(max(1, n))
        assert self.L.md_piece_read(self.piece, 0, n, got) == 0
        return got.raw[:n]

    def close(self):
        self.L.md_piece_destroy(self.piece)
        if self.stage:
            self.L.md_host_free(C.c_void_p(self.stage))
        self.dev.close()


@pytest.fixture(scope="module")
def rig():
    r = PieceRig()
    yield r
    r.close()


def check_piece(rig, members, seed=1):
    """members: [Member] submitted as one piece with right CRCs: every member's bytes equal zlib's; BAM payload members' digests equal walk()'s"""
    rc, err, info, tab = rig.submit([(m.stream, len(m.raw), zlib.crc32(m.raw)) for m in members], seed)
    assert rc == 0, err
    assert info.n_mem == len(members) and info.out_bytes == tab[-1][3] + tab[-1][2] == sum(len(m.raw) for m in members)
    got = rig.read(tab)
    recs = (C.c_uint32 * max(1, info.n_records))()
    assert rig.L.md_piece_read_records(rig.piece, 0, info.n_records, recs) == 0
    first, n_bam = 0, 0
    for i, m in enumerate(members):
        oo = tab[i][3]
        assert got[oo:oo + len(m.raw)] == m.raw == zlib.decompress(m.stream, -15), (i, m.name)
        g = info.digest[i]
        assert g.first_rec == first, (i, m.name)
        if "bam" in m.name:
            offs, dg = walk(m.raw)
            assert g.ok == 1 and (g.n_rec, g.tid0, g.pos0, g.tidN, g.posN, g.min_endp, g.max_endp, g.sorted) == dg, m.name
            assert [recs[first + k] for k in range(len(offs))] == [oo + x for x in offs], m.name
            n_bam += 1
        first += g.n_rec
    assert first == info.n_records
    return n_bam


def test_piece_zoo_equals_zlib(rig, zoo):
    """the whole zoo as one piece; again reversed on the same piece (its buffers reused at other offsets); libdeflate's members with it,
    or a warning that names them as left out"""
    if not Z.libdeflate():
        warnings.warn("libdeflate.so.0 is not on this machine: the zoo's libdeflate members are left out of the piece")
    else:
        assert sum(m.name.startswith("libdeflate") for m in zoo) == 28
    assert check_piece(rig, zoo) >= 5
    assert check_piece(rig, zoo[::-1], seed=2) >= 5


def test_pieces_of_one_round_and_one_more(rig, zoo):
    """exactly the members k_inflate keeps resident at once, and one more (a second round of one member)"""
    n = rig.L.md_piece_members_per_round(rig.dev.h)
    assert n > 0
    for k in (n, n + 1):
        check_piece(rig, [zoo[(7 * i) % len(zoo)] for i in range(k)], seed=k)


CRC_LENGTHS = list(range(1, 66)) + [0, 1007, 1008, 1009, 1023, 1024, 1025, 16127, 16128, 16129, 65279, 65280, 65535, 65536]


def crc_items():
    """zero / 0xFF / random members of CRC_LENGTHS; the long ones at every out_off % 16 (a short member in front sets the offset)"""
    import random
    rnd = random.Random(11)
    raw = []
    for L in CRC_LENGTHS:
        for kind in ("zero", "ff", "random"):
            raw.append(Z.content(kind, L, rnd))
    at = sum(map(len, raw))
    for L in CRC_LENGTHS[66:]:
        for r in range(16):
            pad = (r - at) % 16
            if pad:
                raw.append(rnd.randbytes(pad)); at += pad
            raw.append(Z.content(("zero", "ff", "random")[r % 3], L, rnd)); at += L
    return [(Z.zraw(d, 1), len(d), zlib.crc32(d)) for d in raw]


def test_crc32_every_length_edge_and_alignment(rig):
    items = crc_items()
    _, tab = Z.piece_layout(items)
    assert {t[3] % 16 for t in tab if t[2] >= 1007} == set(range(16))
    rc, err, info, tab = rig.submit(items)
    assert rc == 0, err
    # one flipped CRC bit at a time: first, middle and last member, short and long members
    lens = [n for _, n, _ in items]
    picks = [0, 1, 2, 5, 64, 100, 150, 194, len(items) // 2, len(items) - 1]
    for L in (1007, 1008, 1024, 16128, 16129, 65279, 65536):
        picks.append(lens.index(L))
    seen = set()
    for k, i in enumerate(picks):
        if i in seen or lens[i] == 0:
            continue
        seen.add(i)
        bad = list(items); s, n, c = bad[i]; bad[i] = (s, n, c ^ (1 << (k % 32)))
        rc, err, _, _ = rig.submit(bad)
        assert rc != 0 and "CRC32" in err and f"member {i} of the piece" in err, (i, n, err)
    assert len(seen) >= 16 and 0 in seen and len(items) - 1 in seen
    # a member of no bytes with a CRC that is not 0
    z = lens.index(0)
    bad = list(items); bad[z] = (items[z][0], 0, 0x1234)
    rc, err, _, _ = rig.submit(bad)
    assert rc != 0 and f"member {z} of the piece" in err, err
    rc, err, _, _ = rig.submit(items)
    assert rc == 0, err


def test_malformed_members_are_refused_and_the_piece_recovers(rig, zoo, tmp_path):
    """ISIZE one off, streams cut short, a distance behind byte 0: refused naming the member, with the error code the shared decoder gives
    (tools/inflate_emu --each on the same members); the good members on either side of it in the same launch (Z.AROUND_MALFORMED: far
    matches, stored blocks, pass-capped batches, none empty) are byte-exact all the same, and so is the next submit on the same piece"""
    import json
    import re
    import subprocess
    good = Z.around_malformed(zoo)
    gi = [(m.stream, len(m.raw), zlib.crc32(m.raw)) for m in good]
    assert all(n >= 1000 for _, n, _ in gi) and sum(n for _, n, _ in gi) > 200000
    bad = Z.malformed()
    f = tmp_path / "bad.bam"
    f.write_bytes(Z.bgzf_file([(s, n, 0) for _, s, n in bad]))
    r = subprocess.run([str(EMU), "--each", str(f)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    want = json.loads(r.stdout)["rc"]
    for k, (name, s, n) in enumerate(bad):
        assert want[k] > 0, name
        rc, err, _, tab = rig.submit(gi[:3] + [(s, n, 0)] + gi[3:], seed=k)
        m = re.search(r"error (\d+) in member (\d+) of the piece", err)
        assert rc != 0 and m and int(m.group(2)) == 3, (name, err)
        # (a stream cut short is read on into the bytes behind it, which differ between the emulator's file and the piece: any refusal)
        assert int(m.group(1)) == want[k] if "cut" not in name else 0 < int(m.group(1)) < 12, (name, want[k], err)
        got = rig.read(tab)
        for i, g in zip((0, 1, 2, 4, 5, 6), good):
            assert got[tab[i][3]:tab[i][3] + tab[i][2]] == g.raw, (name, "good member", i, g.name)
        assert check_piece(rig, good, seed=k + 100) == 1


# ---- command level: a BAM re-encoded the way other writers encode it ----
@pytest.fixture(scope="module")
def reenc(tmp_path_factory):
    d = tmp_path_factory.mktemp("reenc")
    synth(d / "s", "-L", "1500000", "-c", "25", "-s", "41", "--extras")
    hdr, recs = Z.bam_split((d / "s.bam").read_bytes())
    return d, hdr, recs


def _z(level, strategy=zlib.Z_DEFAULT_STRATEGY, memlevel=8):
    return lambda data: Z.zraw(data, level, strategy, -15, memlevel)


REENC = {"zlib0": (_z(0), 65280), "zlib1": (_z(1), 65280), "zlib6": (_z(6), 65280), "zlib9": (_z(9), 65280), "filtered": (_z(6, zlib.Z_FILTERED), 65280),
         "huffman_only": (_z(6, zlib.Z_HUFFMAN_ONLY), 65280), "rle": (_z(6, zlib.Z_RLE), 65280), "fixed": (_z(6, zlib.Z_FIXED), 65280),
         "zlib9_memlevel1": (_z(9, memlevel=1), 65280), "sync_every_record": (None, 65280), "small_members": (_z(6), 5000), "members_65536": (_z(6), 65536),
         "libdeflate1": ("ld", 1), "libdeflate6": ("ld", 6), "libdeflate12": ("ld", 12)}


def device_pieces(stderr):
    line = [l for l in stderr.splitlines() if "on the device" in l]
    assert line, stderr[-2000:]
    return int(line[0].split("on the device ")[1].split()[0])


@pytest.mark.parametrize("variant", list(REENC))
def test_cli_reencoded_bam_equals_oracle(reenc, tmp_path, variant):
    d, hdr, recs = reenc
    enc, lim = REENC[variant]
    if enc == "ld":
        if not Z.libdeflate():
            pytest.skip("libdeflate.so.0 is not on this machine")
        enc, lim = (lambda data, lv=lim: Z.ldraw(data, lv)), 65280
    (tmp_path / "v.bam").write_bytes(Z.bam_reencode(hdr, recs, enc, lim, sync=variant == "sync_every_record"))
    compare_cli(tmp_path, [str(d / "s.fa"), str(tmp_path / "v.bam")], env=DEV)
    assert device_pieces((tmp_path / "gpu_stderr.txt").read_text()) >= 1


@pytest.mark.parametrize("damage", ["truncated_member", "isize_plus_1"])
def test_cli_damaged_member_is_refused_by_every_path(reenc, tmp_path, damage):
    """a member in the middle of the file cut short by two bytes (BSIZE says so), or its ISIZE one too large: the device's inflate, the host's
    and the oracle (htslib's bgzf_read_block: inflate error / "Inflated block size mismatch") all stop, each product path with its own
    refusal of the member (csrc/mdk_inflate.hip md_piece_wait, csrc/host/mdk_io.c inflate_worker)"""
    from conftest import run_oracle
    d, hdr, recs = reenc
    raw = Z.bam_reencode(hdr, recs, _z(6), 65280)
    mem = Z.bgzf_members(raw)
    k = len(mem) // 2
    io, il, isz, crc = mem[k]
    s = raw[io:io + il]
    if damage == "truncated_member":
        s = s[:-2]
    bad = raw[:io - 18] + Z.bgzf_member(s, isz + (damage == "isize_plus_1"), crc) + raw[io + il + 8:]
    (tmp_path / "bad.bam").write_bytes(bad)
    (tmp_path / "o").mkdir()
    assert run_oracle([str(d / "s.fa"), str(tmp_path / "bad.bam"), "-o", "out"], cwd=tmp_path / "o").returncode != 0
    for name, env, says in (("device", DEV, "BGZF inflate failed on the device"), ("host", {"MDK_HOST_INFLATE": "1"}, "BGZF inflate failed (corrupt file?)")):
        w = tmp_path / name; w.mkdir()
        r = mdk.run_cli([str(d / "s.fa"), str(tmp_path / "bad.bam"), "-o", "out"], cwd=w, env=env)
        assert r.returncode != 0 and says in r.stderr, (name, r.returncode, r.stderr[-800:])
