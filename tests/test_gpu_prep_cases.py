"""GPU: the device chunk preparation (csrc/mdk_prep.hip: k_prep_scan, k_prep_segs) on hand-built records at its edges.

tests/test_gpu_prep.py holds the preparation against the host's and the oracle on what generators happen to write.  Here every record is
placed on purpose, with tests/bamwriter.py, so that a named branch decides the result:

  * two read names under ONE entry of the chunk's name table (names from tests/name_hash.py): same_name in the two-read branch and in
    pair_of_many's chain walk, its tail loop beyond 16 letters, the LDS grouping that sees two full hashes;
  * where D.prev, "the read admitted just before", comes from: a lane of the wavefront, an earlier wavefront of the workgroup,
    cntA[tk - 1], block_prev / prev_of walking back over workgroups that admitted nothing, PREP_PREV_NONE;
  * tile runs of a workgroup whose segments reach SEG_TSPAN tiles or more, written by the lanes instead of merged in LDS.

Every case is held against the oracle (compare_cli: byte-identical output of the command) and against the host preparation chunk by chunk
(both_ways of test_gpu_prep.py: the segments as a multiset, the sites exactly, every chunk with rc 0).  The builders are plain functions of
a directory, so tests/test_name_hash_cpu.py can ask the oracle alone whether a collision case would notice a mix-up of the two names."""
import ctypes as C
import os
from pathlib import Path

import pytest

import methyldackel_amd as mdk
import name_hash as nh
from bamwriter import cigar, record, write_bam, write_fasta
from test_gpu_parity import compare_cli
from test_gpu_prep import both_ways

pytestmark = pytest.mark.gpu

UNIT = "ACGTCGCGTTCGAACGCGTA"          # 6 CpGs in 20 bases: every overlap of 30 bases covers some
Q10 = ["-q", "10"]                    # the commands' admission: MAPQ 0 filler is filtered out
MAX_CHUNK_RECORDS = 3000              # a name table of at most 4096 entries: what the literal pairs share a slot in


class Layout:
    """records of one contig in file order: `add` appends one at a position not below the last, `fill` pads with filler (unique names,
    unpaired) up to an index; `marks` remembers which name was put at which index"""

    def __init__(self, start=10):
        self.recs, self.pos, self.nfill, self.marks = [], start, 0, {}

    def add(self, name, flag, pos, length=60, meth=True, mapq=40, cig=None, mark=True):
        assert pos >= self.pos, "records are written in coordinate order"
        self.pos = pos
        if mark:
            self.marks[len(self.recs)] = name
        self.recs.append((name, flag, pos, cig or f"{length}M", meth, mapq))
        return len(self.recs) - 1

    def fill(self, upto, admitted=True, still=False):
        """filler up to index `upto` (exclusive): admitted reads every 3 bases, or records the command filters out (MAPQ 0), four to a
        position; still: all at the last position"""
        assert len(self.recs) <= upto, (len(self.recs), upto)
        while len(self.recs) < upto:
            self.nfill += 1
            step = 0 if still else 3 if admitted else int(self.nfill % 4 == 0)
            self.add(f"fill{self.nfill}", 16 if self.nfill % 4 == 0 else 0, self.pos + step, meth=self.nfill % 3 != 0, mapq=40 if admitted else 0, mark=False)

    def write(self, d, tag, length=None):
        L = max(length or 0, max(p + sum(c >> 4 for c in cigar(cg) if c & 15 in (0, 2, 3)) for _, _, p, cg, _, _ in self.recs) + 200)
        ref = (UNIT * (L // len(UNIT) + 1))[:L]
        out = []
        for name, flag, pos, cg, meth, mapq in self.recs:
            seq, x = "", pos
            for c in cigar(cg):
                if c & 15 == 0: seq += ref[x:x + (c >> 4)]
                if c & 15 in (0, 2, 3): x += c >> 4
            out.append(record(0, pos, flag, cg, seq if meth else seq.replace("C", "T"), 35, qname=name, mapq=mapq, mpos=pos))
        write_bam(d / f"{tag}.bam", [("c1", L)], out)
        write_fasta(d / f"{tag}.fa", [("c1", ref)])
        return [str(d / f"{tag}.fa"), str(d / f"{tag}.bam")], L


# ---- motifs: a few records whose outcome depends on the names, on `prev`, or on the links.  `at` is the index of the motif's first record;
#      the reads of a pair disagree in every C of their overlap (one keeps them, one reads T), so resolving the wrong two changes counts ----
def m_pair(lay, at, admitted, tag):
    """an overlapping proper pair (99, 147): the two-read branch, mdk_pair_two"""
    lay.fill(at, admitted)
    p = lay.pos + 4
    lay.add(f"pair{tag}", 99, p, meth=True); lay.add(f"pair{tag}", 147, p + 20, meth=False)


def m_swept_pair(lay, at, admitted, tag, gap=0):
    """two records of one name with a read of another name starting beyond the first's end in between (and `gap` records the command
    filters out behind that): the two-read branch, where mdk_pair_two's `rend_f < prev_s` leaves the two unpaired -- if the second's prev
    is that read's start.  The two do not overlap, so only the segments' flags (the comparison with the host preparation) tell"""
    lay.fill(at, admitted)
    p = lay.pos + 4
    lay.add(f"swept{tag}", 99, p, length=40, meth=True)
    lay.add(f"sweeper{tag}", 0, p + 45, meth=True)
    lay.fill(len(lay.recs) + gap, admitted=False, still=True)
    lay.add(f"swept{tag}", 147, p + 50, meth=False)


def m_evict(lay, at, admitted, tag, gap=0):
    """three records of one name; a read of another name starts beyond the first one's end before the second arrives: the first is swept
    out of the buffer, the name's pending entry erased, and the SECOND pairs with the THIRD (pair_of_many; the second's prev decides).
    gap: records the command filters out between that read and the second"""
    lay.fill(at, admitted)
    p = lay.pos + 4
    lay.add(f"evict{tag}", 99, p, length=40, meth=True)
    lay.add(f"sweep{tag}", 0, p + 45, meth=True)
    lay.fill(len(lay.recs) + gap, admitted=False, still=True)
    lay.add(f"evict{tag}", 147, p + 50, meth=False); lay.add(f"evict{tag}", 99, p + 70, meth=True)


def m_keep(lay, at, admitted, tag, filtered_between=False):
    """the same three records without that read (or with it filtered out, which must not count): the FIRST pairs with the second, the
    third stays alone"""
    lay.fill(at, admitted)
    p = lay.pos + 4
    lay.add(f"keep{tag}", 99, p, length=40, meth=True)
    if filtered_between:
        lay.add(f"nosweep{tag}", 0, p + 45, meth=True, mapq=0)
    lay.add(f"keep{tag}", 147, p + 50, meth=False); lay.add(f"keep{tag}", 99, p + 70, meth=True)


def m_collide_a(lay, at, admitted, names):
    """two names under one table entry, one read each (99, 147, overlapping): the two-read branch, where same_name's failure means
    "two names with one hash, each alone": the reads stay unpaired"""
    lay.fill(at, admitted)
    p = lay.pos + 4
    lay.add(names[0], 99, p, meth=True); lay.add(names[1], 147, p + 20, meth=False)


def m_collide_b(lay, at, admitted, names, order="ABAB"):
    """two names under one table entry, a proper overlapping pair each, interleaved in coordinate order: one chain of four, walked by
    pair_of_many, where same_name's failure is the `continue`: A pairs with A and B with B.  (order AABB: not interleaved; taking the two
    names for one would pair the same reads, so that order says nothing about same_name, only about the links)"""
    lay.fill(at, admitted)
    p = lay.pos + 4
    seen = {"A": 0, "B": 0}
    for k, w in enumerate(order):
        lay.add(names[0] if w == "A" else names[1], 147 if seen[w] else 99, p + 10 * k, meth=(w == "A") == (seen[w] == 0))
        seen[w] += 1


def m_collide_swept(lay, at, admitted, names):
    """two names under one table entry, A's records all before B's: A1, a read of another name that starts beyond A1's end, A2, B1, B2.
    A1 is swept out when A2 arrives, so A2 is left pending; B1 and B2 pair.  Taken for one name, B1 would pair with the pending A2."""
    lay.fill(at, admitted)
    p = lay.pos + 4
    lay.add(names[0], 99, p, length=40, meth=True)
    lay.add(f"sweep{names[0]}", 0, p + 45, meth=True)
    lay.add(names[0], 147, p + 50, meth=False)
    lay.add(names[1], 99, p + 60, meth=True); lay.add(names[1], 147, p + 80, meth=False)


def pair_names(pair, merged):
    """merged: what the device would make of the case if it took the two names for one"""
    return (pair[0], pair[0]) if merged else (pair[0], pair[1])


# ---- section 2: collision cases.  A case is a list of (motif, index, pair); `merged` names the entry whose two names become one ----
COLLISION_CASES = {
    "ab-short": [("a", 40, nh.SHORT_PAIRS[0]), ("b", 120, nh.SHORT_PAIRS[1])],
    "ab-tail24": [("a", 40, nh.TAIL_PAIRS[0]), ("b", 120, nh.TAIL_PAIRS[1])],
    "ab-lengths": [("a", 40, nh.LENGTH_PAIRS[0]), ("b", 120, nh.LENGTH_PAIRS[1]), ("a", 150, nh.LENGTH_PAIRS[2])],
    "d-one-workgroup": [("b", 100, nh.SHORT_PAIRS[2])],
    "d-A-below-256-B-from-256": [("swept", 253, nh.SHORT_PAIRS[3]), ("AABB", 510, nh.SHORT_PAIRS[5])],
    "d-A1-at-255": [("b", 255, nh.SHORT_PAIRS[4])],
}


def collision_bam(d, case, merged=None, tag="c"):
    lay = Layout()
    for k, (motif, at, pair) in enumerate(COLLISION_CASES[case]):
        names = pair_names(pair, merged == k)
        if motif == "a": m_collide_a(lay, at, True, names)
        elif motif == "swept": m_collide_swept(lay, at, True, names)
        else: m_collide_b(lay, at, True, names, "AABB" if motif == "AABB" else "ABAB")
    lay.fill(len(lay.recs) + 60)
    return lay.write(d, tag)[0], lay


def probe_bam(d, names, tag="p"):
    """18 records of 60 bases every 10 bases (test_gpu_prep.many_records_one_name with n = 18), the two names taking turns: 9 records each"""
    lay = Layout()
    for k in range(18):
        lay.add(names[k % 2], 99 if (k // 2) % 2 == 0 else 147, 10 + 10 * k, meth=k % 3 != 0)
    return lay.write(d, tag, 800)[0]


# ---- section 3: the pairing machine's inputs at chosen indices ----
def m_collide_b3(lay, at, admitted, tag):
    m_collide_b(lay, at, admitted, nh.SHORT_PAIRS[5 - int(tag) % 3][:2])      # (a pair of its own per placement in a file)


MOTIFS = [("pair", m_pair, 1), ("evict", m_evict, 2), ("keep", m_keep, 1), ("collide-b", m_collide_b3, 2)]       # (name, builder, records below the boundary)


def admitted_layout(d, rot):
    """motif rot, rot + 1, rot + 2 (of the four) straddling index 63|64, 255|256 and 511|512, padded with admitted reads"""
    lay = Layout()
    for k, B in enumerate((64, 256, 512)):
        _, fn, below = MOTIFS[(rot + k) % 4]
        fn(lay, B - below, True, f"{k}")
    m_keep(lay, len(lay.recs) + 20, True, "f", filtered_between=True)
    lay.fill(len(lay.recs) + 40)
    return lay.write(d, f"adm{rot}"), lay


def filtered_layout(d, rot):
    """padded with records the command filters out (MAPQ 0 under -q 10).  The chunk's first 256 records are all filtered, so its first
    admitted read, at index 319 or 318, finds PREP_PREV_NONE across a whole block; motifs straddle 319|320, 511|512, 767|768; then the
    evict motif with 300 filtered records between the sweeping read (index 1023) and the name's second record, so that the workgroup of
    records 1024..1279 admits nothing and prev_of walks over it; and two records of a name with the read that sweeps the first out at
    index 1791 and 300 filtered records before the second, so that block_prev walks over the workgroup of records 1792..2047"""
    lay = Layout()
    for k, B in enumerate((320, 512, 768)):
        _, fn, below = MOTIFS[(rot + k) % 4]
        fn(lay, B - below, False, f"{k}")
    m_evict(lay, 1022, False, "g", gap=300)
    m_swept_pair(lay, 1790, False, "g", gap=300)
    lay.fill(len(lay.recs) + 10, admitted=False)
    return lay.write(d, f"flt{rot}"), lay


# ---- section 4: tile runs ----
TILE = 512
CONTIG = 40000


def sparse_bam(d):
    """300 reads of 100 bases every 130 bases: the first workgroup's 256 reads lie over 65 tiles of 512"""
    lay = Layout(0)
    for k in range(300):
        lay.add(f"s{k}", 16 if k % 3 == 0 else 0, 20 + 130 * k, length=100, meth=k % 2 == 0)
    return lay.write(d, "sparse", CONTIG)[0]


def far_read_bam(d):
    """20x of 100-base reads over 3 kb, among them one read 50M17000N50M whose pieces are 33 tiles of 512 apart, and its mate over the
    second piece"""
    lay = Layout(0)
    for k in range(600):
        if k == 200:
            lay.add("far", 99, 5 * k + 2, cig="50M17000N50M", meth=True)
        lay.add(f"d{k}", 16 if k % 3 == 0 else 0, 5 * k + 3, length=100, meth=k % 2 == 0)
    lay.add("far", 147, 5 * 200 + 2 + 17050 + 10, length=60, meth=False)
    return lay.write(d, "far", CONTIG)[0]


def threshold_bam(d, tiles):
    """256 admitted reads, one workgroup, from position 0 to exactly the end of tile 31 (thi - tlo == 31 < SEG_TSPAN: merged in LDS) or
    one base into tile 32 (thi - tlo == 32: written by the lanes)"""
    assert tiles in (32, 33)
    lay = Layout(0)
    last = 32 * TILE - 100 + (tiles - 32)
    for k in range(256):
        lay.add(f"t{k}", 16 if k % 3 == 0 else 0, last * k // 255, length=100, meth=k % 2 == 0)
    assert lay.recs[-1][2] + 100 == 32 * TILE + (tiles - 32)
    return lay.write(d, f"thr{tiles}", CONTIG)[0]


# ---- what a test does with a file ----
def candidate_names(args):
    """per chunk that is not passed over, the names of its candidate records in the order the device sees them"""
    plan = mdk.Plan(list(args) + ["-o", str(Path(args[0]).parent / "plan")]); plan.set_prep(1)
    out = []
    while (c := plan.next_chunk()) is not None:
        if c.skipped:
            continue
        raw = c.raw
        blob = b"".join(C.string_at(raw.range[i].ptr, raw.range[i].bytes) for i in range(raw.n_ranges))
        out.append([blob[o + 36:o + 36 + blob[o + 12] - 1].decode() for o in mdk.raw_record_offsets(raw)])
    plan.close()
    return out


def check_placement(args, lay):
    """one chunk, its candidate records are the file's records, and every motif record lies at the index it was built for"""
    chunks = candidate_names(args)
    assert len(chunks) == 1 and len(chunks[0]) == len(lay.recs) <= MAX_CHUNK_RECORDS
    assert {i: chunks[0][i] for i in lay.marks} == lay.marks


def hold(tmp_path, args, min_chunks=1, env=None):
    """the two references: the oracle (the command, byte for byte) and the host preparation (chunk by chunk, every chunk rc 0: both_ways
    downloads each with a call that raises on any other answer)"""
    old = {k: os.environ.get(k) for k in (env or {})}
    try:
        os.environ.update(env or {})
        n_chunks, n_reads, n_segs = both_ways(list(args) + ["-o", str(tmp_path / "x")])
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
    assert n_chunks >= min_chunks and n_reads > 0 and n_segs >= n_reads, (n_chunks, n_reads, n_segs)
    compare_cli(tmp_path, args, env=env)
    return n_chunks


def eight_chunks(L):
    return ["--chunkSize", str(L // 9)]


@pytest.mark.parametrize("case", ["ab-short", "ab-tail24", "ab-lengths"])
def test_two_names_under_one_table_entry(tmp_path, case):
    """Cases a, b, c.  Two names that agree in hash >> 32 and in the home slot are linked into one chain by table_insert.
    a: one read each (99, 147, overlapping): k_prep_segs' two-read branch, same_name fails = "two names with one hash, each alone", the
    reads stay unpaired.  b: a proper pair each, A1 B1 A2 B2: pair_of_many's chain walk, same_name fails = the `continue`; A pairs with A
    and B with B.  ab-short: names of 10 letters, told apart by the PrepRead's first block; ab-tail24: 24 letters, equal in the first
    16 and in length, told apart by same_name's tail loop alone; ab-lengths: equal in the first 16 letters, 23 and 24 letters long (in
    both orders), told apart by the length."""
    args, lay = collision_bam(tmp_path, case)
    check_placement(args + Q10, lay)
    assert hold(tmp_path, args + Q10) == 1


@pytest.mark.parametrize("case", ["d-one-workgroup", "d-A-below-256-B-from-256", "d-A1-at-255"])
def test_collision_chain_across_workgroups(tmp_path, case):
    """Case d: the chain of case b at three placements.  d-one-workgroup: all four records among one workgroup's 256 (indices 100..103):
    k_prep_scan groups them in LDS first, by the FULL hash, which differs: two groups, each inserted by one lane, the second behind the
    first's head.  d-A-below-256-B-from-256: each workgroup inserts one name's group: A1 A2 at 510, 511 and B1 B2 at 512, 513, two proper pairs -- a
    placement that holds the links but, not interleaved, cannot tell a mix-up of the names --, and its rebuilt form at 253..257: A1, a
    read that sweeps it out, A2 below 256, B1 B2 from 256 on; A2 stays pending and unpaired, where one name would give it B1.
    d-A1-at-255: A1 alone in its workgroup, B1 A2 B2 grouped in the next; A1's prev comes from a lane, B1's from cntA[0]."""
    args, lay = collision_bam(tmp_path, case)
    check_placement(args + Q10, lay)
    assert hold(tmp_path, args + Q10) == 1


@pytest.mark.parametrize("colliding", [True, False], ids=["colliding", "control"])
def test_probe_restated_hash_is_the_device_s(tmp_path, colliding):
    """Case e.  9 records under each of two names.  If the two share a table entry the chain holds 18 records, more than MAXG, and the
    device hands the chunk back (md_dev_download: -7); with the control name in place of one of them there are two chains of 9 and it
    stays (0).  The command's output equals the oracle's either way."""
    a, b, ctl = nh.SHORT_PAIRS[0]
    args = probe_bam(tmp_path, (a, b if colliding else ctl)) + ["-F", "0", "-q", "0", "--keepDupes"]
    compare_cli(tmp_path, args)
    plan = mdk.Plan(args + ["-o", str(tmp_path / "x")]); plan.set_prep(1)
    dev = mdk.Device(plan.dev_cfg()); dev.set_prep(plan.prep_cfg())
    c = plan.next_chunk(); plan.ensure_reference(dev, c.tid)
    assert c.raw.n_records == 18
    dev.submit_raw(0, c.raw)
    rc = dev.L.md_dev_download(dev.h, 0, C.byref(mdk.md_sites()))
    dev.close(); plan.close()
    if colliding:
        assert rc == -7, (f"md_dev_download answered {rc}, not -7: the device does not file {a} and {b} under one table entry, so tests/name_hash.py's "
                          "restatement of the hash or its literals are wrong and every other collision case of this file is vacuous")
    else:
        assert rc == 0, f"md_dev_download answered {rc} with the control name: 9 records of a name must stay on the device"


@pytest.mark.parametrize("chunks", ["one-chunk", "eight-chunks"])
@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_prev_from_lane_wavefront_and_cntA(tmp_path, rot, chunks):
    """D.prev at 63|64, 255|256, 511|512, admitted filler.  Motifs: an overlapping proper pair (mdk_pair_two); three records of a name
    with a read of another name starting beyond the first's end before the second (evict: the second's prev is that read's start and
    sweeps the first out); the same without it, and with it filtered out (keep); the collision chain.  Rotation `rot` puts motif rot at
    63|64 -- prev of the record at 64 from an EARLIER WAVEFRONT of the workgroup (wlast), of the record at 63 from a LANE of its
    wavefront --, motif rot + 1 at 255|256 and rot + 2 at 511|512 -- prev of the first record of a workgroup from cntA[tk - 1] (block_prev
    in the two-read branch, prev_of in the chain walk).  eight-chunks: the same file in nine chunks, one group launch of eight
    (chunk_of_block, static_ticket) and one more."""
    (args, L), lay = admitted_layout(tmp_path, rot)
    if chunks == "one-chunk":
        check_placement(args + Q10, lay)
        assert hold(tmp_path, args + Q10) == 1
    else:
        assert max(len(c) for c in candidate_names(args + Q10 + eight_chunks(L))) <= MAX_CHUNK_RECORDS
        hold(tmp_path, args + Q10 + eight_chunks(L), min_chunks=8)


@pytest.mark.parametrize("chunks", ["one-chunk", "eight-chunks"])
@pytest.mark.parametrize("rot", [0, 2])
def test_prev_across_workgroups_that_admit_nothing(tmp_path, rot, chunks):
    """D.prev with filler the command filters out (MAPQ 0 under -q 10).  The chunk's first 256 records are all filtered: the first admitted
    read (index 319 or 318, first wavefront of the second workgroup) gets PREP_PREV_NONE across a block -- rot 0: a pair, through
    block_prev; rot 2: three records of one name, through prev_of.  Motifs straddle 319|320 (earlier wavefront), 511|512 and 767|768
    (cntA[tk - 1], with nothing but filtered records in between: prev is the previous motif's last read, far back).  Last, the evict motif
    with the sweeping read at index 1023 and 300 filtered records before the name's second record -- the workgroup of records 1024..1279
    admits nothing and prev_of walks back over it (chain walk) --, and two records of a name (1790, 2092) with the read that sweeps the
    first out at 1791 and 300 filtered records behind it: cntA of the workgroup of records 1792..2047 is PREP_PREV_NONE and block_prev
    walks back over it to that read's start, which leaves the two unpaired (two-read branch, mdk_pair_two's rend_f < prev_s)."""
    (args, L), lay = filtered_layout(tmp_path, rot)
    if chunks == "one-chunk":
        check_placement(args + Q10, lay)
        names = candidate_names(args + Q10)[0]
        assert all(n.startswith("fill") for n in names[:256] + names[1024:1280] + names[1792:2048])
        assert hold(tmp_path, args + Q10) == 1
    else:
        assert max(len(c) for c in candidate_names(args + Q10 + eight_chunks(L))) <= MAX_CHUNK_RECORDS
        hold(tmp_path, args + Q10 + eight_chunks(L), min_chunks=8)


TILE_ENVS = [pytest.param({"MDK_TILE": str(TILE)}, id="tile-512"), pytest.param(None, id="tile-default")]


@pytest.mark.parametrize("env", TILE_ENVS)
def test_tile_runs_sparse_coverage(tmp_path, env):
    """Tile runs, sparse: the first workgroup's 256 reads lie over 65 tiles of 512 (thi - tlo >= SEG_TSPAN): k_prep_segs leaves the LDS
    merge and every lane writes tiles[t].first/last itself; the second workgroup (44 reads, 12 tiles) merges in LDS.  At the default tile
    (2048) both merge in LDS."""
    assert hold(tmp_path, sparse_bam(tmp_path), env=env) == 1


@pytest.mark.parametrize("env", TILE_ENVS)
def test_tile_runs_sparse_coverage_split(tmp_path, env):
    """Tile runs, the sparse case cut into chunks of 8000 positions, fewer than 32 tiles of 512 each: the same reads through the LDS
    merge, the same expected output."""
    assert hold(tmp_path, sparse_bam(tmp_path) + ["--chunkSize", "8000"], env=env) >= 5


@pytest.mark.parametrize("env", TILE_ENVS)
def test_tile_runs_read_with_a_long_N(tmp_path, env):
    """Tile runs, dense with one far read: 50M17000N50M among 20x coverage.  Its workgroup's segments reach 34 tiles of 512, so all its
    lanes write their runs themselves, the far read for every tile between its pieces; its mate, 400 records on, is linked through the
    name table and cuts the second piece."""
    assert hold(tmp_path, far_read_bam(tmp_path), env=env) == 1


@pytest.mark.parametrize("env", TILE_ENVS)
@pytest.mark.parametrize("tiles", [32, 33])
def test_tile_runs_at_the_threshold(tmp_path, tiles, env):
    """Tile runs, the threshold: one workgroup of 256 admitted reads whose extent is exactly 32 tiles of 512 (thi - tlo == 31: the last
    span merged in LDS) and exactly 33 (thi - tlo == 32 == SEG_TSPAN: the first written by the lanes)."""
    assert hold(tmp_path, threshold_bam(tmp_path, tiles), env=env) == 1
