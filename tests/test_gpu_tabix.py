"""GPU: tabix indexes made on the device (csrc/mdk_tabix.hip, libmdk_index.so) and regions read through them.  No session is opened: the
tables are hand-built tensors (tests/tabix_rule.py).  The .tbi of every file `write(compress=True, index=True)` and `tabix_index` make must
be the emulator's (tools/tabix_emu: csrc/mdk_tabix_core.h on the host) byte for byte, its payload the numpy builder's, and the reader
written from the specification must answer every region of the grid through it as brute force over the decompressed file does; every
refusal must name the path and the line and leave no .tbi; and `read(region=)` must give the rows of `read().select(overlap)`.
Region reads see leaf bins only: `Calls.read` and `Cytosines.read` take one-base rows alone (a merged file is refused by name), and a
one-base row never straddles a window, so the upper levels -- up to bin 0 -- are what the first tests hold against the emulator, the
builder and the specification reader on the table with the straddling rows."""
import gzip
import os

import numpy as np
import pytest

import tabix_rule as T

pytestmark = pytest.mark.gpu
SMALL_EDGES = [0, 1, 100, 1000, 16383, 16384, 16385, 17000, 20001, 131072, 1 << 29]


def make_calls(t, contigs=T.CONTIGS, rows=slice(None)):
    import torch
    import methyldackel_amd as mdk
    return mdk.Calls(list(contigs), {n: torch.from_numpy(t[n][rows].copy()).cuda() for n, _ in mdk.CALL_COLUMNS}, contexts_on=(0,))


def make_cytosines(t, contigs=T.CONTIGS):
    import torch
    import methyldackel_amd as mdk
    n = len(t["start"])
    cols = {"contig": t["contig"], "pos": t["start"] + 1, "strand": t["strand"], "nmeth": t["nmeth"], "nunmeth": t["nunmeth"], "context": t["context"],
            "trinucleotide": np.tile(np.frombuffer(b"CGA", dtype=np.uint8), (n, 1))}
    c = mdk.Cytosines(list(contigs), {k: torch.from_numpy(np.ascontiguousarray(cols[k]).astype(dt)).cuda() for k, dt in mdk.CYTOSINE_COLUMNS})
    c.contexts_on = (0,)
    return c


def check_index(path, cf, tmp_path, edges=T.EDGES):
    """the .tbi next to `path` is the emulator's, its payload the builder's, and the specification reader answers the grid through it"""
    raw, tbi = open(path, "rb").read(), open(str(path) + ".tbi", "rb").read()
    out = tmp_path / (os.path.basename(str(path)) + ".emu.tbi")
    r = T.emu(path, cf, out)
    assert r.returncode == 0, r.stderr
    assert tbi == out.read_bytes(), path
    text = gzip.decompress(raw)
    assert gzip.decompress(tbi) == T.payload(text, raw, cf), path
    parsed = T.read_tbi(tbi)
    for n, b, e in T.grid(parsed["names"] or [b"chrA"], edges):
        assert T.query(raw, parsed, n, b, e) == T.brute(raw, cf, n, b, e), (path, n, b, e)
    return raw, parsed


@pytest.fixture(scope="module")
def table():
    return T.calls_table()


# first in the file: the kernels' first execution
@pytest.mark.parametrize("block_rows", [None, 1000, 7])
def test_write_with_an_index_bedgraph(table, tmp_path, block_rows):
    calls = make_calls(table)
    assert 5900 < len(calls) < 6100
    path, = calls.write("t", directory=str(tmp_path), block_rows=block_rows, compress=True, index=True)
    assert path.endswith("t_CpG.bedGraph.gz") and os.path.exists(path + ".tbi")
    raw, parsed = check_index(path, T.conf("bed", 1), tmp_path)
    assert parsed["names"] == [b"chrA", b"chrLong"] and len(gzip.decompress(raw)) > 140000
    bins = set(parsed["refs"][1][0])                                  # every level up to bin 0
    assert 0 in bins and any(1 <= b < 9 for b in bins) and any(9 <= b < 73 for b in bins) and any(73 <= b < 585 for b in bins) and any(585 <= b < 4681 for b in bins)
    (tmp_path / "plain").mkdir()
    plain, = calls.write("t", directory=str(tmp_path / "plain"), block_rows=block_rows, compress=True)         # the data file is the one written without an index
    assert open(plain, "rb").read() == raw and not os.path.exists(plain + ".tbi")


@pytest.mark.parametrize("fmt", ["fraction", "counts", "methylKit"])
def test_write_with_an_index_other_formats(table, tmp_path, fmt):
    calls = make_calls(table)
    path, = calls.write("t", fmt=fmt, directory=str(tmp_path), block_rows=1500, compress=True, index=True)
    check_index(path, T.conf("methylKit" if fmt == "methylKit" else "bed", 1), tmp_path)


@pytest.mark.parametrize("block_rows", [None, 1000])
def test_write_with_an_index_cytosine_report(table, tmp_path, block_rows):
    cyto = make_cytosines(table)
    path = cyto.write("t", directory=str(tmp_path), block_rows=block_rows, compress=True, index=True)
    _, parsed = check_index(path, T.conf("cytosine_report", 0), tmp_path)
    assert parsed["names"] == [b"chrA", b"chrLong"]


def test_an_empty_table_and_what_index_needs(table, tmp_path):
    import methyldackel_amd as mdk
    empty = make_calls(table, rows=slice(0, 0))
    path, = empty.write("e", directory=str(tmp_path), compress=True, index=True)
    _, parsed = check_index(path, T.conf("bed", 1), tmp_path, SMALL_EDGES)
    assert parsed["names"] == []                                      # n_ref = 0
    with pytest.raises(mdk.MdkError, match="compress=True"):
        empty.write("x", directory=str(tmp_path), index=True)
    with pytest.raises(mdk.MdkError, match="compress=True"):
        make_cytosines(table).write("x", directory=str(tmp_path), index=True)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("x")]


@pytest.fixture(scope="module")
def written(table, tmp_path_factory):
    """the table and its first 40 rows written with their indexes: (path, raw, parsed .tbi) each"""
    d, out = tmp_path_factory.mktemp("tabix_written"), {}
    for name, rows in (("big", slice(None)), ("small", slice(0, 40))):
        path, = make_calls(table, rows=rows).write(name, directory=str(d), compress=True, index=True)
        raw = open(path, "rb").read()
        out[name] = (path, raw, T.read_tbi(open(path + ".tbi", "rb").read()))
    return out


CUTS = {"ends_on_a_newline": ("big", None, True, 5000), "one_byte_members": ("small", 1, True, None), "an_empty_member_in_the_middle": ("big", [500, 0, 0, 700, 0, 900], True, 3000),
        "a_line_across_three_members": ("small", 7, True, None), "no_eof_member": ("big", 4097, False, None), "a_piece_ends_inside_a_line": ("small", 40, True, 90),
        "pieces_of_one_byte_members": ("small", 1, False, 100)}


@pytest.mark.parametrize("case", list(CUTS))
def test_tabix_index_of_files_cut_by_hand(written, tmp_path, case):
    import methyldackel_amd as mdk
    which, cuts, eof, block_bytes = CUTS[case]
    path0, raw0, parsed0 = written[which]
    text = gzip.decompress(raw0)
    if cuts is None:
        cuts = [text.index(b"\n", 200) + 1, 1000]                     # the first member ends exactly on a newline
    raw = T.bgzf(text, cuts, eof)
    path = tmp_path / "cut.anyname"
    path.write_bytes(raw)
    assert mdk.tabix_index(path, block_bytes=block_bytes) == str(path) + ".tbi"           # preset "bed", the track line found
    cf = T.conf("bed", 1)
    _, parsed = check_index(path, cf, tmp_path, T.EDGES if which == "big" else SMALL_EDGES)
    assert parsed["names"] == parsed0["names"] and parsed["conf"] == parsed0["conf"]
    for n, b, e in T.grid(parsed["names"], T.EDGES if which == "big" else SMALL_EDGES):          # the answers of the file `write` made of the same rows
        assert T.query(raw, parsed, n, b, e) == T.query(raw0, parsed0, n, b, e), (case, n, b, e)


def test_tabix_index_of_a_written_file_is_writes_own(written, tmp_path):
    import methyldackel_amd as mdk
    path0, raw0, _ = written["big"]
    path = tmp_path / "copy.gz"
    path.write_bytes(raw0)
    for block_bytes in (None, 70000):
        mdk.tabix_index(path, "bed", skip=1, block_bytes=block_bytes)
        assert open(str(path) + ".tbi", "rb").read() == open(path0 + ".tbi", "rb").read()
    plain = tmp_path / "plain.bedGraph"
    plain.write_bytes(gzip.decompress(raw0))
    with pytest.raises(mdk.MdkError, match="plain.bedGraph.*not a BGZF file"):
        mdk.tabix_index(plain)
    gz = tmp_path / "plain.gz"
    gz.write_bytes(gzip.compress(gzip.decompress(raw0)[:5000]))
    with pytest.raises(mdk.MdkError, match="plain.gz.*not BGZF"):
        mdk.tabix_index(gz)
    with pytest.raises(mdk.MdkError, match="preset"):
        mdk.tabix_index(path, "vcf")
    assert not os.path.exists(str(plain) + ".tbi") and not os.path.exists(str(gz) + ".tbi")


@pytest.mark.parametrize("case", T.refusals(), ids=lambda c: c[0])
def test_every_refusal_names_the_path_and_the_line(tmp_path, case):
    import methyldackel_amd as mdk
    name, text, cf, line, code = case
    path = tmp_path / f"{name}.gz"
    for cuts, block_bytes in ((65280, None), (37, 100)):              # one piece; pieces that end inside lines, the line counted across them
        if block_bytes is not None and max(len(x) for x in text.split(b"\n")) >= 70:
            block_bytes = 2000                                        # (a piece holds the longest line)
        path.write_bytes(T.bgzf(text, cuts))
        (tmp_path / f"{name}.gz.tbi").write_bytes(b"stale")
        with pytest.raises(mdk.MdkError, match=rf"{name}\.gz, line {line}: .*{T.MESSAGES[code]}") as e:
            mdk.tabix_index(path, "methylKit" if cf[1] == 2 else "bed", skip=1, block_bytes=block_bytes)
        assert e.value.rc == -3 and not os.path.exists(str(path) + ".tbi")


def test_write_refuses_rows_out_of_order(table, tmp_path):
    import torch
    import methyldackel_amd as mdk
    calls = make_calls(table)
    order = torch.arange(len(calls), device="cuda")
    order[[2000, 2001]] = order[[2001, 2000]]                         # lines 2002 and 2003 swapped: header, then rows
    with pytest.raises(mdk.MdkError, match=r"u_CpG\.bedGraph\.gz, line 2003: .*not sorted"):
        calls.select(order).write("u", directory=str(tmp_path), block_rows=999, compress=True, index=True)
    path = str(tmp_path / "u_CpG.bedGraph.gz")
    assert not os.path.exists(path + ".tbi") and gzip.decompress(open(path, "rb").read()).count(b"\n") == len(calls) + 1       # the data file is whole
    back = torch.cat((torch.arange(3000, len(calls), device="cuda"), torch.arange(0, 3000, device="cuda"), torch.arange(3000, 3001, device="cuda")))
    with pytest.raises(mdk.MdkError, match=rf"line {len(calls) + 2}: not sorted: contig chrLong appears in two places"):
        calls.select(back).write("v", directory=str(tmp_path), compress=True, index=True)


# ---- regions read through the index ----
R_CONTIGS = ["r1", "r2", "r3"]
R_LENGTHS = [300000, 1000, 150000]


@pytest.fixture(scope="module")
def region_files(tmp_path_factory):
    """a table over short contigs (r2 has no row), its FASTA with C and G where the rows are, the bedGraph and the report written with
    their indexes in blocks of 500 rows, and the whole files read back"""
    import methyldackel_amd as mdk
    d = tmp_path_factory.mktemp("tabix_regions")
    rng = np.random.default_rng(7)
    p1, p3 = np.sort(rng.choice(R_LENGTHS[0] - 10, 2500, replace=False)), np.sort(rng.choice(R_LENGTHS[2] - 10, 1500, replace=False))
    p1 = np.unique(np.concatenate((p1, [16383, 16384, 131071, 131072, 262143, 262144])))
    start = np.concatenate((p1, p3)).astype(np.int32)
    n = len(start)
    t = {"contig": np.concatenate((np.zeros(len(p1)), np.full(len(p3), 2))).astype(np.int32), "start": start, "end": start + 1,
         "nmeth": rng.integers(1, 30, n).astype(np.int32), "nunmeth": rng.integers(0, 30, n).astype(np.int32), "context": np.zeros(n, dtype=np.uint8),
         "strand": np.where(rng.integers(0, 2, n) == 1, 1, -1).astype(np.int8)}
    seqs = [np.full(length, ord("A"), dtype=np.uint8) for length in R_LENGTHS]
    for c, s, st in zip(t["contig"], t["start"], t["strand"]):
        seqs[c][s] = ord("C") if st > 0 else ord("G")
    with open(d / "r.fa", "wb") as f:
        for name, s in zip(R_CONTIGS, seqs):
            f.write(b">" + name.encode() + b"\n" + b"\n".join(bytes(s[o:o + 60]) for o in range(0, len(s), 60)) + b"\n")
    bed, = make_calls(t, R_CONTIGS).write("r", directory=str(d), block_rows=500, compress=True, index=True)
    rep = make_cytosines(t, R_CONTIGS).write("r", directory=str(d), block_rows=500, compress=True, index=True)
    ref = mdk.Reference(d / "r.fa")
    calls, cyto = mdk.Calls.read(bed, ref), mdk.Cytosines.read(rep, R_CONTIGS)
    assert len(calls) == n == len(cyto)
    yield {"dir": d, "bed": bed, "report": rep, "ref": ref, "calls": calls, "cyto": cyto, "last": int(p1[-1]), "row": int(p1[1000])}
    ref.close()


def regions_of(f):
    return [("r1", 16384, 32768), ("r1", 16383, 16385), ("r1", 0, 16384), ("r1", 131072, 262144), ("r1", 0, 131072), ("r1", 131071, 131073), ("r1", 0, R_LENGTHS[0]),
            ("r1", f["last"] + 1, R_LENGTHS[0]), ("r1", f["row"], f["row"] + 1), ("r1", f["row"] - 1, f["row"]), ("r3", 0, R_LENGTHS[2]), ("r3", 40000, 40100),
            ("r3", 200000, 250000), ("r2", 0, 1000), ("nowhere", 0, 1000), ("r1", 0, 1 << 29)]


def same(a, b, columns):
    import torch
    return len(a) == len(b) and all(torch.equal(getattr(a, n), getattr(b, n)) for n, _ in columns)


def test_a_region_of_calls_is_the_selection_of_the_whole_file(region_files):
    import methyldackel_amd as mdk
    f = region_files
    full, hit = f["calls"], 0
    for name, beg, end in regions_of(f):
        got = mdk.Calls.read(f["bed"], f["ref"], region=(name, beg, end))
        mask = (full.contig == (R_CONTIGS.index(name) if name in R_CONTIGS else -1)) & (full.start < end) & (full.end > beg)
        assert same(got, full.select(mask), mdk.CALL_COLUMNS), (name, beg, end)
        assert got.contigs == full.contigs
        hit += len(got) > 0
    assert hit >= 10
    assert len(mdk.Calls.read(f["bed"], f["ref"], region=("r1", f["row"], f["row"] + 1))) == 1
    one = mdk.Calls.read(f["bed"], f["ref"], region=("r1", 16384, 32768), block_bytes=300)         # one window
    in_file = sum(1 for m in T.Z.bgzf_members(open(f["bed"], "rb").read()) if m[2])
    assert in_file > 8 and 0 < len(one) < 400 and 0 < one.members_inflated < in_file
    assert mdk.Calls.read(f["bed"], f["ref"], region=("r2", 0, 1000)).members_inflated == 0


def test_a_region_of_a_report_is_the_selection_of_the_whole_file(region_files):
    import methyldackel_amd as mdk
    f = region_files
    full = f["cyto"]
    for name, beg, end in regions_of(f):
        got = mdk.Cytosines.read(f["report"], R_CONTIGS, region=(name, beg, end))
        mask = (full.contig == (R_CONTIGS.index(name) if name in R_CONTIGS else -1)) & (full.pos - 1 < end) & (full.pos > beg)
        assert same(got, full.select(mask), mdk.CYTOSINE_COLUMNS), (name, beg, end)
    one = mdk.Cytosines.read(f["report"], R_CONTIGS, region=("r3", 16384, 32768))
    assert 0 < len(one) and 0 < one.members_inflated < sum(1 for m in T.Z.bgzf_members(open(f["report"], "rb").read()) if m[2])


def test_what_a_region_read_refuses(region_files, tmp_path):
    import methyldackel_amd as mdk
    f = region_files
    with pytest.raises(mdk.MdkError, match="one file"):
        mdk.Calls.read([f["bed"], f["bed"]], f["ref"], region=("r1", 0, 10))
    plain = tmp_path / "plain.bedGraph"
    plain.write_bytes(gzip.decompress(open(f["bed"], "rb").read()))
    with pytest.raises(mdk.MdkError, match="plain.bedGraph.*BGZF"):
        mdk.Calls.read(plain, f["ref"], region=("r1", 0, 10))
    bare = tmp_path / "bare.gz"
    bare.write_bytes(open(f["bed"], "rb").read())
    with pytest.raises(mdk.MdkError, match=r"bare\.gz\.tbi: no tabix index"):
        mdk.Calls.read(bare, f["ref"], region=("r1", 0, 10))
    with pytest.raises(mdk.MdkError, match=r"bare\.gz\.tbi: no tabix index"):
        mdk.Cytosines.read(bare, R_CONTIGS, region=("r1", 0, 10))
    for bad in (("r1", 5, 5), ("r1", -1, 5), ("r1", 5), "r1:1-5"):
        with pytest.raises(mdk.MdkError, match="region must be"):
            mdk.Calls.read(f["bed"], f["ref"], region=bad)
