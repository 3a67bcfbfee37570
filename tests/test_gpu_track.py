"""GPU: Calls.render_bigwig / write_bigwig (csrc/mdk_bigwig.hip -> libmdk_track.so) against the rule's two other builds -- tools/bigwig_emu,
byte for byte, and tests/bigwig_rule.py, which takes the device's file apart with struct and zlib and compares it with the numpy
restatement bit for bit.  Every comparison is exact.  (The file's name sorts behind the session tests on purpose: DESIGN.md section 4,
the recorded fault.)"""
import numpy as np
import pytest

import bigwig_rule as R

pytestmark = pytest.mark.gpu

CASES = R.cases()
REFUSALS = R.refusals()

# ---- tables of this file ----
# a row over several level-0 bins and a level-1 boundary (4096), among single bases on both sides
_w = R._run(400, 30, 5)
_ws, _we = _w[1].copy(), _w[2].copy()
_keep = (_we <= 1000) | (_ws >= 9000)
_wide = [x[_keep] for x in (_w[0], _ws, _we, _w[3], _w[4])]
_at = int(np.searchsorted(_wide[1], 1000))
_wide = [np.insert(x, _at, v) for x, v in zip(_wide, (0, 1000, 9000, 7, 3))]
CASES["row_spans_bins"] = ([("chr1", 12000)], R.table(*_wide), "percent")
# both sides of a wavefront's 64 rows and of a workgroup's 256
for _n in (63, 64, 65, 255, 256, 257):
    CASES[f"rows_{_n}"] = ([("chr1", 40000), ("chr2", 100)], R._cat(R._run(_n)), "percent")


def _edited(n, edit):
    cols = [x.copy() for x in R._run(n, 3, 7)]
    edit(*cols)
    return R.table(*cols)


_two = [("chr1", 5000), ("chr2", 100)]
for _a in (63, 255):           # the pair (a, a + 1) lies across a wavefront's / a workgroup's edge
    REFUSALS[f"order_across_{_a}"] = (_two, _edited(700, lambda c, s, e, m, u, a=_a: s.__setitem__(a + 1, s[a])), "percent", R.E_ORDER, _a + 1)
    REFUSALS[f"overlap_across_{_a}"] = (_two, _edited(700, lambda c, s, e, m, u, a=_a: e.__setitem__(a, s[a + 1] + 1)), "percent", R.E_OVERLAP, _a)
REFUSALS["last_row_empty"] = (_two, _edited(700, lambda c, s, e, m, u: (m.__setitem__(699, 0), u.__setitem__(699, 0))), "percent", R.E_EMPTY, 699)
REFUSALS["last_row_behind"] = (_two, _edited(257, lambda c, s, e, m, u: (s.__setitem__(256, s[255]), e.__setitem__(256, s[255] + 1))), "percent", R.E_ORDER, 256)


def calls(contigs, cols):
    import torch
    import methyldackel_amd as mdk
    return mdk.Calls([n for n, _ in contigs], {name: torch.from_numpy(np.ascontiguousarray(cols[name]).copy()).cuda() for name, _ in mdk.CALL_COLUMNS})


def lengths(contigs):
    return [l for _, l in contigs]


def rendered(contigs, cols, value, **kw):
    return calls(contigs, cols).render_bigwig(lengths(contigs), value, **kw).cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """name -> the emulator's file for that table, a fresh process's run, made at its first use and kept unchanged"""
    made = {}

    def get(name):
        if name not in made:
            assert R.EMU.exists(), "make tools"
            contigs, cols, value = CASES[name]
            rc, data, err = R.emu(tmp_path_factory.mktemp("emu"), contigs, cols, value)
            assert rc == 0, err
            made[name] = data
        return made[name]
    return get


@pytest.fixture
def limits():
    """md_track_limits for the test, the defaults again behind it"""
    import methyldackel_amd as mdk
    yield mdk.track_limits
    mdk.track_limits(0, 0, 0)


@pytest.mark.parametrize("name", list(CASES))
def test_the_device_s_file_is_the_emulator_s(emu, name):
    contigs, cols, value = CASES[name]
    got = rendered(contigs, cols, value)
    assert len(got) == len(emu(name))
    assert got == emu(name)
    R.compare(got, contigs, cols, value)                          # both trees walked, every section inflated by zlib, the restatement bit for bit


def test_a_table_without_rows_is_228_bytes(emu):
    import torch
    t = calls(*CASES["no_rows"][:2]).render_bigwig([5000, 100])
    assert t.dtype == torch.uint8 and t.device.type == "cuda" and t.numel() == 228 and t.cpu().numpy().tobytes() == emu("no_rows")


def test_the_row_over_the_bins(emu):
    contigs, cols, value = CASES["row_spans_bins"]
    x = R.expect(lengths(contigs), cols, value)
    lvl0 = {int(r[1]): int(r[3]) for r in x["records"][0]}
    plain = lambda lo: int(((cols["start"] >= lo) & (cols["end"] <= lo + 1024)).sum())      # noqa: E731
    assert lvl0[0] == plain(0) + 24 and [lvl0[w] for w in range(1024, 8192, 1024)] == [1024] * 7 and lvl0[8192] == plain(8192) + 808
    lvl1 = {int(r[1]): int(r[3]) for r in x["records"][1]}
    assert lvl1[0] == plain(0) + 24 + 3072 and lvl1[4096] == 4096 and lvl1[8192] == lvl0[8192] + sum(v for k, v in lvl0.items() if k > 8192)
    f = R.compare(rendered(contigs, cols, value), contigs, cols, value)
    assert f["summary"][0] == int((cols["end"] - cols["start"]).sum())


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_name_the_row(tmp_path, name):
    import methyldackel_amd as mdk
    contigs, cols, value, code, row = REFUSALS[name]
    with pytest.raises(R.Refused) as r:
        R.check(lengths(contigs), cols, value)
    assert (r.value.code, r.value.row) == (code, row)
    rc, data, err = R.emu(tmp_path, contigs, cols, value)
    assert rc == 3 and err.startswith(f"row {row}: ") and R.MESSAGES[code] in err, err
    c = calls(contigs, cols)
    for call in (lambda: c.render_bigwig(lengths(contigs), value), lambda: c.write_bigwig(tmp_path / "refused.bw", lengths(contigs), value)):
        with pytest.raises(mdk.MdkError) as e:
            call()
        assert e.value.rc == -3 and f"(row {row}: " in str(e.value) and R.MESSAGES[code] in str(e.value), str(e.value)
        assert err.strip() in str(e.value)                        # the emulator's words
    assert not (tmp_path / "refused.bw").exists()
    # the handle is as good as before
    assert rendered(*CASES["one_row"]) == R.emu(tmp_path, *CASES["one_row"])[1]


def test_fewer_workgroups_than_work(emu, limits):
    contigs, cols, value = CASES["sections_257"]
    limits(0, 3, 0)
    assert rendered(contigs, cols, value) == emu("sections_257")


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("name", ["rows_1025", "contig_ends_mid_section", "sections_257"])
def test_batch_edges(emu, limits, name, batch):
    """a batch's edge at a section, at a contig's end, and between the data and the zoom sections (259 data sections: odd)"""
    contigs, cols, value = CASES[name]
    limits(0, 0, batch)
    assert rendered(contigs, cols, value) == emu(name)
    limits(0, 2, batch)
    assert rendered(contigs, cols, value) == emu(name)


@pytest.mark.parametrize("name,piece", [("one_row", 1), ("last_base", 1), ("contig_ends_mid_section", 7), ("sections_257", 4093), ("rows_1025", 1000), ("rows_1025", None)])
def test_the_file_in_pieces_is_the_file(tmp_path, emu, name, piece):
    contigs, cols, value = CASES[name]
    c = calls(contigs, cols)
    path = c.write_bigwig(tmp_path / "t.bw", lengths(contigs), value, piece_bytes=piece)
    assert path == tmp_path / "t.bw" and path.read_bytes() == emu(name) == c.render_bigwig(lengths(contigs), value).cpu().numpy().tobytes()


def test_ranges_that_begin_and_end_anywhere(emu):
    """md_track_bigwig_fill_range itself: ranges inside the header, over the chromosome tree's end, inside a section, over the index, the last byte"""
    import ctypes as C
    import torch
    import methyldackel_amd as mdk
    contigs, cols, value = CASES["contig_ends_mid_section"]
    whole = emu("contig_ends_mid_section")
    f = R.read_bigwig(whole)
    c = calls(contigs, cols)
    assert c.render_bigwig(lengths(contigs), value).numel() == len(whole)        # the file stays measured on the handle
    L = mdk.lib_track()
    index_at = int(np.frombuffer(whole, "<u8", 1, 24)[0])
    ranges = [(0, 1), (3, 70), (60, 300), (index_at - 5, 60), (index_at + 40, 9), (len(whole) - 1, 1), (len(whole) - 9, 9), (1, len(whole) - 2), (17, 0)]
    assert f["levels"] >= 1
    with mdk._side_locks["track"]:
        h = mdk._side_handle(L, "track", 0)
        for at, n in ranges:
            buf = torch.full((n + 16,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert L.md_track_bigwig_fill_range(h, C.c_void_p(buf.data_ptr() + 8), at, n) == 0, L.md_track_last_error()
            got = buf.cpu().numpy().tobytes()
            assert got[8:8 + n] == whole[at:at + n] and got[:8] == got[8 + n:] == b"\xa5" * 8, (at, n)         # and not a byte outside the range
        for at, n in ((-1, 4), (len(whole), 1), (5, len(whole))):
            assert L.md_track_bigwig_fill_range(h, C.c_void_p(buf.data_ptr()), at, n) == -3


def test_handle_reuse_and_two_runs(emu):
    """a large table, a small one, the empty one and the large one again on one handle: no state is left over; and two runs give equal bytes"""
    order = ["sections_257", "one_row", "no_rows", "sections_257", "hashed", "hashed", "constant", "rows_64"]
    for name in order:
        assert rendered(*CASES[name]) == emu(name), name


def test_context_against_select(tmp_path):
    """rows of three contexts that are one valid table (no overlap); ``context=`` takes what ``select`` takes"""
    import methyldackel_amd as mdk
    contigs, cols, value = CASES["contig_ends_mid_section"]
    cols = dict(cols)
    cols["context"] = (np.arange(len(cols["start"])) % 3).astype(np.uint8)
    c = calls(contigs, cols)
    L = lengths(contigs)
    for k, name in enumerate(mdk.CONTEXT_FILES):
        sub = {n: v[cols["context"] == k] for n, v in cols.items()}
        want = R.emu(tmp_path, contigs, sub, value)[1]
        assert c.render_bigwig(L, context=k).cpu().numpy().tobytes() == want
        assert c.render_bigwig(L, context=name).cpu().numpy().tobytes() == want
        assert c.select(c.context == k).render_bigwig(L).cpu().numpy().tobytes() == want
    assert c.render_bigwig(L).cpu().numpy().tobytes() == R.emu(tmp_path, contigs, cols, value)[1]
    # merged CpG and CHG rows overlap at CGG: the whole table is refused and the message says what to do
    s, e = cols["start"].copy(), cols["end"].copy()
    e[10] = s[11] + 1
    with pytest.raises(mdk.MdkError, match=r"row 10: .*pass one context") as err:
        calls(contigs, dict(cols, start=s, end=e)).render_bigwig(L)
    assert err.value.rc == -3


def test_a_reference_gives_the_lengths(tmp_path, emu):
    import methyldackel_amd as mdk
    contigs, cols, value = CASES["last_base"]
    (tmp_path / "r.fa").write_text("".join(f">{n}\n{'ACGT' * (l // 4)}\n" for n, l in contigs))
    with mdk.Reference(tmp_path / "r.fa") as ref:
        assert ref.lengths == lengths(contigs)
        assert calls(contigs, cols).render_bigwig(ref).cpu().numpy().tobytes() == emu("last_base")


def test_coverage_and_percent_are_two_files(tmp_path, emu):
    contigs, cols, value = CASES["coverage_above_2_24"]
    got = rendered(contigs, cols, "coverage")
    assert got == emu("coverage_above_2_24")
    items = np.concatenate([it[:, 2] for _, it in R.read_bigwig(got)["sections"]]).view(np.float32)
    assert items.tolist() == [16777220.0, 2147483648.0 + 256, 0.0, 7.0]
    contigs, cols, _ = CASES["rows_257"]
    assert rendered(contigs, cols, "coverage") == R.emu(tmp_path, contigs, cols, "coverage")[1] != emu("rows_257")


def test_a_cohort_s_sample(tmp_path):
    import torch
    import methyldackel_amd as mdk
    contigs, cols, _ = CASES["rows_1025"]
    other = dict(cols, nmeth=cols["nunmeth"], nunmeth=cols["nmeth"] + 1)
    co = mdk.unite([calls(contigs, cols), calls(contigs, other)])
    assert len(co) == 1025
    for i, src in enumerate((cols, other)):
        s = co.sample(i)
        assert type(s) is mdk.Calls and torch.equal(s.nmeth, co.nmeth[i])
        want = R.emu(tmp_path, contigs, src, "coverage")[1]
        assert s.render_bigwig(lengths(contigs), "coverage").cpu().numpy().tobytes() == want
