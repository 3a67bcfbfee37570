"""CPU: the bigWig track as the package offers it -- Calls.render_bigwig, Calls.write_bigwig, libmdk_track.so's header -- as far as it goes
without a device: the names, the header against what lib_track() binds and against the rule's constants, the refusals that are made
before the library is touched, and the range cutter of csrc/mdk_bigwig_core.h through its host build (`bigwig_emu --pieces N`).  The
kernels' bytes are tests/test_gpu_track.py's."""
import inspect
import re
import subprocess

import numpy as np
import pytest

import bigwig_rule as R
from conftest import REPO

CASES = R.cases()


def cpu_calls(contigs=("chr1", "chr2"), n=4):
    import torch
    import methyldackel_amd as mdk
    cols = {name: torch.ones(n, dtype=getattr(torch, dt)) for name, dt in mdk.CALL_COLUMNS}
    cols["start"] = torch.arange(n, dtype=torch.int32) * 3
    cols["end"] = cols["start"] + 1
    cols["contig"] = torch.zeros(n, dtype=torch.int32)
    return mdk.Calls(list(contigs), cols)


def test_the_names_exist():
    import methyldackel_amd as mdk
    assert callable(mdk.Calls.render_bigwig) and callable(mdk.Calls.write_bigwig) and callable(mdk.lib_track) and callable(mdk.track_limits)
    assert mdk.LIB_TRACK.name == "libmdk_track.so" and mdk.LIB_TRACK.parent == mdk.LIB_INDEX.parent
    assert list(inspect.signature(mdk.Calls.render_bigwig).parameters) == ["self", "lengths", "value", "context"]
    assert list(inspect.signature(mdk.Calls.write_bigwig).parameters) == ["self", "path", "lengths", "value", "context", "piece_bytes"]
    assert inspect.signature(mdk.Calls.render_bigwig).parameters["value"].default == "percent"
    assert mdk.TRACK_PIECE_BYTES == 64 << 20


def test_the_header_declares_what_lib_track_binds(monkeypatch):
    import methyldackel_amd as mdk
    header = (REPO / "include" / "mdk_track.h").read_text()
    declared = set(re.findall(r"\b(md_track_\w+)\s*\(", header))
    monkeypatch.setattr(mdk, "_track", None)                       # a fresh load holds what lib_track() and the loader under it bound, and no more
    bound = {name for name in vars(mdk.lib_track()) if name.startswith("md_track_")}
    assert bound == {"md_track_open", "md_track_close", "md_track_last_error", "md_track_limits", "md_track_bigwig_measure", "md_track_bigwig_fill_range"}
    assert bound == declared
    for name, count in (("md_track_bigwig_measure", 12), ("md_track_bigwig_fill_range", 4), ("md_track_limits", 3), ("md_track_open", 2)):
        decl = re.search(rf"int {name}\((.*?)\);", header, re.S).group(1)
        assert len(decl.split(",")) == count, name
    L = mdk.lib_track()                                            # (loading it needs no device)
    assert len(L.md_track_bigwig_measure.argtypes) == 12 and len(L.md_track_bigwig_fill_range.argtypes) == 4 and len(L.md_track_limits.argtypes) == 3
    assert re.search(r"MD_TRACK_ERR_ARG = -3\b", header) and re.search(r"MD_TRACK_ERR_HIP = -2\b", header) and re.search(r"MD_TRACK_ERR_NOMEM = -4\b", header)


def test_the_rules_constants_are_the_restatements():
    import methyldackel_amd as mdk
    core = (REPO / "methyldackel_amd" / "csrc" / "mdk_bigwig_core.h").read_text()

    def define(name):
        return int(re.search(rf"#define {name} (\w+?)u?\b", core).group(1), 0)

    assert (define("BW_ITEMS"), define("BW_ZITEMS"), define("BW_BLOCK"), define("BW_LEVELS")) == (R.ITEMS, R.ZITEMS, R.BLOCK, R.LEVELS)
    assert (define("BW_MAGIC"), define("BW_CHROM_MAGIC"), define("BW_RTREE_MAGIC")) == (R.MAGIC, R.CHROM_MAGIC, R.RTREE_MAGIC)
    # a slot: 16 unused bytes, 78 9C, the stored form of the largest raw section (5 + bytes), the Adler-32, to a multiple of 64
    raw = define("BW_RAW_STRIDE")
    assert raw == max(24 + 12 * R.ITEMS, 32 * R.ZITEMS) == 16384
    assert define("BW_SLOT") == 16448 and define("BW_SLOT") >= define("BW_SLOT_LEAD") + 2 + 5 + raw + 4 and define("BW_SLOT") % 64 == 0
    codes = dict(re.findall(r"\b(BW_E_\w+) = (\d+)", core))
    assert {k: int(v) for k, v in codes.items()} == {"BW_E_ROW": R.E_ROW, "BW_E_NEGATIVE": R.E_NEGATIVE, "BW_E_EMPTY": R.E_EMPTY, "BW_E_ORDER": R.E_ORDER, "BW_E_OVERLAP": R.E_OVERLAP}
    values = dict(re.findall(r"\b(BW_VALUE_\w+) = (\d+)", core))
    assert {"percent": int(values["BW_VALUE_PERCENT"]), "coverage": int(values["BW_VALUE_COVERAGE"])} == mdk.TRACK_VALUES
    # every message the restatement quotes stands in the rule's text
    for text in R.MESSAGES.values():
        assert text in core, text


def test_arguments_are_refused_before_the_library_is_touched(tmp_path, monkeypatch):
    """every refusal that needs no device, with CPU tensors; write_bigwig leaves no file"""
    import torch
    import methyldackel_amd as mdk
    monkeypatch.setattr(mdk, "lib_track", lambda: pytest.fail("the library was asked for"))
    c = cpu_calls()
    cases = [(dict(lengths=[100, 100], value="fraction"), "unknown value 'fraction'"), (dict(lengths=[100]), "lengths has 1 entries, the rows have 2 contigs"),
             (dict(lengths=[100, 100, 100]), "lengths has 3 entries"), (dict(lengths=[100, -1]), "the length of chr2 must be an int between 0 and 2^31 - 1"),
             (dict(lengths=[2 ** 31, 5]), "the length of chr1"), (dict(lengths=[100.0, 5]), "the length of chr1"), (dict(lengths=[True, 5]), "the length of chr1"),
             (dict(lengths=7), "lengths is a Reference, or a sequence"), (dict(lengths=[100, 100], context=3), "unknown context 3"),
             (dict(lengths=[100, 100], context="CpH"), "unknown context 'CpH'"), (dict(lengths=[100, 100], context=True), "unknown context True"),
             (dict(lengths=[100, 100]), "the contig column is a cpu tensor, and there is no CPU path"),
             (dict(lengths=[100, 2 ** 31 - 1], value="coverage", context="CHH"), "no CPU path")]
    for kw, text in cases:
        with pytest.raises(mdk.MdkError, match=re.escape(text)):
            c.render_bigwig(**kw)
        with pytest.raises(mdk.MdkError, match=re.escape(text)):
            c.write_bigwig(tmp_path / "t.bw", **kw)
    for bad in (-1, -5, 2 ** 31):
        with pytest.raises(mdk.MdkError, match="piece_bytes"):
            c.write_bigwig(tmp_path / "t.bw", [100, 100], piece_bytes=bad)
    assert not (tmp_path / "t.bw").exists()
    # a select is a Calls, and a Cohort's sample is one
    with pytest.raises(mdk.MdkError, match="no CPU path"):
        c.select(torch.tensor([0, 2])).render_bigwig([100, 100])


def test_a_reference_with_other_contigs_is_refused(tmp_path):
    import methyldackel_amd as mdk
    (tmp_path / "r.fa").write_text(">chr1\nACGTACGTAC\n>chrOther\nACGT\n")
    (tmp_path / "s.fa").write_text(">chr1\nACGTACGTAC\n>chr2\nACGT\n")
    with mdk.Reference(tmp_path / "r.fa") as other, mdk.Reference(tmp_path / "s.fa") as same:
        with pytest.raises(mdk.MdkError, match="the reference's contigs are not the rows' contigs"):
            cpu_calls().render_bigwig(other)
        assert same.lengths == [10, 4]
        with pytest.raises(mdk.MdkError, match="no CPU path"):             # its lengths are taken: only the device is missing
            cpu_calls().render_bigwig(same)


def test_a_missing_library_names_make(tmp_path, monkeypatch):
    import methyldackel_amd as mdk
    monkeypatch.setattr(mdk, "_track", None)
    monkeypatch.setattr(mdk, "LIB_TRACK", tmp_path / "libmdk_track.so")
    with pytest.raises(mdk.MdkError, match=r"libmdk_track\.so is missing.*run `make`.*no fallback"):
        mdk.lib_track()


def emu_pieces(tmp, contigs, cols, value, pieces):
    """R.emu's files, run once more with --pieces: the assembled file's bytes"""
    out = tmp / f"pieces_{pieces}.bw"
    r = subprocess.run([str(R.EMU)] + (["--coverage"] if value == "coverage" else []) + ["--pieces", str(pieces), str(tmp / "contigs.tsv"), str(tmp / "rows.tsv"), str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out.read_bytes()


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """name -> (the directory with the table's files, the plain run's bytes), made at the first use and kept"""
    made = {}

    def get(name):
        if name not in made:
            contigs, cols, value = CASES[name]
            tmp = tmp_path_factory.mktemp(name)
            rc, whole, err = R.emu(tmp, contigs, cols, value)
            assert rc == 0, err
            made[name] = (tmp, whole)
        return made[name]
    return get


@pytest.mark.parametrize("pieces", [1, 7, 4093])
@pytest.mark.parametrize("name", list(CASES))
def test_the_file_cut_into_pieces_is_the_file(plain, name, pieces):
    """bw_cut_range over every table: the file assembled `pieces` bytes at a time is the plain run's"""
    contigs, cols, value = CASES[name]
    tmp, whole = plain(name)
    assert emu_pieces(tmp, contigs, cols, value, pieces) == whole


def test_pieces_takes_a_positive_number(tmp_path):
    r = subprocess.run([str(R.EMU), "--pieces", "0", "a", "b", "c"], capture_output=True, text=True)
    assert r.returncode == 2 and "--pieces" in r.stderr
    # a refusal is still a refusal under --pieces
    contigs, cols, value, code, row = R.refusals()["overlap"]
    R.emu(tmp_path, contigs, cols, value)
    r = subprocess.run([str(R.EMU), "--pieces", "7", str(tmp_path / "contigs.tsv"), str(tmp_path / "rows.tsv"), str(tmp_path / "o.bw")], capture_output=True, text=True)
    assert r.returncode == 3 and r.stderr.startswith(f"row {row}: ") and not (tmp_path / "o.bw").exists()
