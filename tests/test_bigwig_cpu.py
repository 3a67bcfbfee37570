"""The bigWig writer on the host (no GPU): tools/bigwig_emu is csrc/mdk_bigwig_core.h and csrc/mdk_deflate_core.h walked lane by lane, a whole
file made on the CPU.  Three parties are the yardstick (tests/bigwig_rule.py): the rule restated in numpy, bit for bit; Python's zlib, which must
inflate every section and agree about its Adler-32; and the product's own bigWig reader (csrc/host/mdk_bigwig.c, behind `extract -M`)."""
import subprocess

import numpy as np
import pytest

import bigwig_rule as R
import methyldackel_amd as mdk
from test_bigwig_edges import read_bbm

CASES = R.cases()
REFUSALS = R.refusals()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> the emulator's file, made at its first use and kept for the tests that look at it again"""
    made = {}

    def get(name):
        if name not in made:
            assert R.EMU.exists(), "make tools"
            contigs, cols, value = CASES[name]
            rc, data, err = R.emu(tmp_path_factory.mktemp(name), contigs, cols, value)
            assert rc == 0, err
            made[name] = data
        return made[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_the_file_holds_what_the_rule_says(files, name):
    contigs, cols, value = CASES[name]
    R.compare(files(name), contigs, cols, value)


def test_a_table_without_rows(files):
    f = R.read_bigwig(files("no_rows"))
    assert (f["count"], f["levels"], f["sections"], f["uncompress"], f["index_depth"]) == (0, 0, [], 0, 0)
    assert f["summary"] == (0, 0.0, 0.0, 0.0, 0.0) and f["chroms"] == [("chr1", 5000), ("chr2", 100)]
    assert R.read_bigwig(files("one_row"))["levels"] == 0                      # one record is not fewer than half of one row


def test_section_cuts(files):
    for n, want in ((1023, [1023]), (1024, [1024]), (1025, [1024, 1])):
        assert [len(items) for _, items in R.read_bigwig(files(f"rows_{n}"))["sections"]] == want
    f = R.read_bigwig(files("contig_ends_mid_section"))
    assert [(c, len(items)) for c, items in f["sections"]] == [(0, 1024), (0, 476), (2, 600)]            # no section spans contigs


def test_rows_over_a_bin_boundary_count_a_base_on_each_side(files):
    contigs, cols, value = CASES["rows_straddle_bins"]
    f = R.compare(files("rows_straddle_bins"), contigs, cols, value)
    x = f["expected"]
    covered = int((cols["end"] - cols["start"]).sum())
    assert covered == len(cols["start"]) + 3
    for k in range(R.LEVELS):
        assert int(x["records"][k][:, 3].sum()) == covered
    assert f["summary"][0] == covered
    lvl0 = {int(r[1]): int(r[3]) for r in x["records"][0]}
    plain = lambda lo: int(((cols["start"] >= lo) & (cols["end"] <= lo + 1024)).sum())      # noqa: E731
    assert lvl0[0] == plain(0) + 1 and lvl0[1024] == plain(1024) + 2 and lvl0[3072] == plain(3072) + 1 and lvl0[4096] == plain(4096) + 1


def test_the_last_base_of_a_contig(files):
    x = R.compare(files("last_base"), *CASES["last_base"])["expected"]
    assert [tuple(int(v) for v in r[:4]) for r in x["records"][0]] == [(0, 0, 1024, 1), (0, 4096, 5000, 1), (1, 0, 1024, 2), (1, 1024, 2048, 1)]


def test_both_trees_get_a_second_level(files):
    f = R.read_bigwig(files("sections_257"))
    assert f["count"] == 259 and f["index_depth"] == 2 and len(f["chroms"]) == 300
    assert f["levels"] >= 2 and f["zoom"][0]["reduction"] == 1024


def test_stored_and_constant_sections(files):
    h, full, c = R.read_bigwig(files("hashed")), R.read_bigwig(files("hashed_full")), R.read_bigwig(files("constant"))
    assert h["stored"] == len(h["sections"]) == 40 and all((raw, comp) == (120, 131) for raw, comp in h["sizes"])       # 2 + 5 + raw + 4
    assert full["stored"] == 0 and all(0.9 * raw < comp < raw for raw, comp in full["sizes"])
    # of a row's twelve bytes the value's four and the upper two of start and end stand twelve bytes back: matches take two thirds of the input
    assert c["stored"] == 0 and all(comp < raw // 2 for raw, comp in c["sizes"]), c["sizes"]


def test_coverage_above_2_24_is_rounded_once(files):
    f = R.read_bigwig(files("coverage_above_2_24"))
    got = np.concatenate([items[:, 2] for _, items in f["sections"]]).view(np.float32)
    assert got.tolist() == [16777220.0, 2147483648.0 + 256, 0.0, 7.0]          # 2^24 + 3 and 2^31 + 129 are halfway cases: ties to even


def test_two_runs_give_the_same_bytes(tmp_path):
    contigs, cols, value = CASES["contig_ends_mid_section"]
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    assert R.emu(tmp_path / "a", contigs, cols, value)[1] == R.emu(tmp_path / "b", contigs, cols, value)[1]


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_name_the_row(tmp_path, name):
    contigs, cols, value, code, row = REFUSALS[name]
    with pytest.raises(R.Refused) as e:
        R.check([l for _, l in contigs], cols, value)
    assert (e.value.code, e.value.row) == (code, row)
    rc, data, err = R.emu(tmp_path, contigs, cols, value)
    assert rc == 3 and data is None and err.startswith(f"row {row}: ") and R.MESSAGES[code] in err, err


def test_the_products_reader_reads_a_coverage_file(tmp_path):
    """csrc/host/mdk_bigwig.c, driven as tests/test_bigwig_edges.py drives it: `extract -M file -N prefix` re-encodes the track per base as
    (unsigned char)(value * 100 + 0.5), NaN -> 0.  Coverage 1 is 100, coverage 0 and no row are 0"""
    contigs = [("chrE", 9000), ("chrNone", 70), ("chrF", 300)]
    i = np.arange(1300)
    cols = R.table(np.r_[np.zeros(1300), np.full(3, 2)], np.r_[5 * i + 2, [0, 150, 299]], np.r_[5 * i + 3 + (i % 7 == 0), [2, 151, 300]], np.r_[i % 3 == 0, [1, 0, 1]], np.r_[i % 3 == 1, [0, 1, 0]])
    rc, data, err = R.emu(tmp_path, contigs, cols, "coverage")
    assert rc == 0, err
    R.compare(data, contigs, cols, "coverage")
    check_products_reader(tmp_path, data, contigs, cols)


def check_products_reader(tmp_path, data, contigs, cols):
    (tmp_path / "cov.bw").write_bytes(data)
    r = subprocess.run([str(mdk.CLI), "extract", "-M", str(tmp_path / "cov.bw"), "-N", str(tmp_path / "cov")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = read_bbm(tmp_path / "cov.bbm")
    for t, (name, length) in enumerate(contigs):
        want = np.zeros(length, dtype=np.int64)
        for c, s, e, m, u in zip(cols["contig"], cols["start"], cols["end"], cols["nmeth"], cols["nunmeth"]):
            if c == t:
                want[s:e] = 100 * (m + u)
        assert got[name] == want.tolist(), name
