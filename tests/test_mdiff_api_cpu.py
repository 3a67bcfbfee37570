"""CPU: the F test of a design's columns as the package offers it -- mdk.diff_model, Cohort.diff_model, ModelDiff, lib_model,
include/mdk_mdiff.h -- as far as it goes without a device: the names, the header against what lib_model() binds, the refusals that are
made before the library is touched, the columns.  The kernel's results are tests/test_gpu_mdiff.py's."""
import re

import pytest

from conftest import REPO

DESIGN = [[1.0, 0.0, 0.3], [1.0, 0.0, -1.0], [1.0, 0.0, 0.5], [1.0, 1.0, 0.1], [1.0, 1.0, 2.0], [1.0, 1.0, -0.7]]


def cpu_matrices(S=6, n=5):
    import torch
    return torch.ones((S, n), dtype=torch.int32), torch.ones((S, n), dtype=torch.int32)


def test_the_names_exist():
    import methyldackel_amd as mdk
    assert callable(mdk.diff_model) and callable(mdk.lib_model) and callable(mdk.Cohort.diff_model)
    assert not issubclass(mdk.ModelDiff, mdk.Diff) and not issubclass(mdk.ModelDiff, mdk.GroupDiff)
    for method in ("qvalue", "select", "rows", "write"):
        assert callable(getattr(mdk.ModelDiff, method)), method
    assert not hasattr(mdk.ModelDiff, "dmrs") and not hasattr(mdk.ModelDiff, "contrast")
    for doc in (mdk.diff_replicates.__doc__, mdk.diff_groups.__doc__):
        assert "diff_model" in doc and "Not here: covariates" not in doc
    assert mdk.MODEL_MAX_COLUMNS == 8 and mdk.MODEL_FLAGS == {"rank": 1, "numeric": 2, "reduced": 4, "full": 8}


def test_the_header_declares_what_lib_model_binds(monkeypatch):
    import methyldackel_amd as mdk
    header = (REPO / "include" / "mdk_mdiff.h").read_text()
    declared = set(re.findall(r"\b(md_stats_\w+)\s*\(", header))
    assert declared == {"md_stats_mdiff"}
    stats = (REPO / "include" / "mdk_stats.h").read_text()
    assert stats.index('#include "mdk_gdiff.h"') < stats.index('#include "mdk_mdiff.h"')
    got = re.search(r"enum \{ MD_STATS_MDIFF_RANK = (\d+), MD_STATS_MDIFF_NUMERIC = (\d+), MD_STATS_MDIFF_REDUCED = (\d+), MD_STATS_MDIFF_FULL = (\d+) \};", header)
    assert got and tuple(map(int, got.groups())) == tuple(mdk.MODEL_FLAGS[k] for k in ("rank", "numeric", "reduced", "full"))
    monkeypatch.setattr(mdk, "_stats", None)
    fresh = {name for name in vars(mdk.lib_stats()) if name.startswith("md_stats_")}
    assert fresh == {"md_stats_open", "md_stats_close", "md_stats_last_error", "md_stats_qdiff"}          # a fresh lib_stats() still binds its four
    L = mdk.lib_model()
    assert L is mdk.lib_stats()
    assert {name for name in vars(L) if name.startswith("md_stats_")} - fresh == declared
    decl = re.search(r"int md_stats_mdiff\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == 22 == len(L.md_stats_mdiff.argtypes)
    # the chain of includes: the kernel's source is the last of the library's
    csrc = REPO / "methyldackel_amd" / "csrc"
    assert (csrc / "mdk_gdiff.hip").read_text().rstrip().endswith('#include "mdk_mdiff.hip"')
    assert '#include "mdk_gdiff_core.h"' in (csrc / "mdk_mdiff_core.h").read_text() and "MDK_DIFF_NO_CONTRACT" in (csrc / "mdk_mdiff_core.h").read_text()
    # the design's buffers are made at the call's first use: md_stats_open allocates what it allocated before this call existed
    opened = re.search(r'extern "C" int md_stats_open\(.*?\n\}', (csrc / "mdk_qdiff.hip").read_text(), re.S).group(0)
    assert opened.count("hipMalloc") == 2 and "design" not in opened
    assert "h->d_design.need(" in (csrc / "mdk_mdiff.hip").read_text() and "h->pin_design.need(" in (csrc / "mdk_mdiff.hip").read_text()
    make = (REPO / "Makefile").read_text()
    assert "$(CSRC)/mdk_mdiff.hip $(CSRC)/mdk_mdiff_core.h" in make and "include/mdk_mdiff.h" in make and "tools/_build/mdiff_emu" in make


def test_every_function_of_the_header_has_contraction_off():
    """the rule's functions with floating-point arithmetic open with MDK_DIFF_NO_CONTRACT, and the header calls no math library"""
    text = (REPO / "methyldackel_amd" / "csrc" / "mdk_mdiff_core.h").read_text()
    code = text[text.index("#ifndef MDK_MDIFF_CORE_H"):]
    bodies = re.findall(r"MDK_DIFF [^;{]*?\)\s*\{\n(.*?)\n\}", code, re.S)
    assert len(bodies) >= 9
    for body in bodies:
        if re.search(r"\bdouble\b", body):
            assert body.lstrip().startswith("MDK_DIFF_NO_CONTRACT"), body[:80]
    assert not re.search(r"\b(exp|log|sqrt|pow|fma|ldexp|frexp)\s*\(", code) and "<math.h>" not in code and "<cmath>" not in code


def test_columns():
    import methyldackel_amd as mdk
    from mdiff_rule import NAMES
    assert tuple(n for n, _ in mdk.MODEL_RESULT_COLUMNS[2:]) == NAMES
    assert mdk.ModelDiff.COLUMNS == mdk.DIFF_SITE_COLUMNS + mdk.MODEL_RESULT_COLUMNS
    assert dict(mdk.MODEL_RESULT_COLUMNS) == {"nmeth": "int64", "nunmeth": "int64", "pvalue": "float64", "df": "int32", "dispersion": "float64", "statistic": "float64",
                                              "flags": "uint8", "iterations": "int32"}


def test_model_diff_holds_its_columns_on_the_host(tmp_path):
    """a ModelDiff made by hand from CPU tensors: the columns, the coefficients, n_columns, tested, names, select, rows and write need
    no device"""
    import torch
    import methyldackel_amd as mdk
    n, p = 4, 3
    cols = {name: torch.arange(n, dtype=getattr(torch, dt)) for name, dt in mdk.ModelDiff.COLUMNS}
    cols["contig"] = torch.zeros(n, dtype=torch.int32)
    coef = torch.arange(p * n, dtype=torch.float64).reshape(p, n) / 8.0
    d = mdk.ModelDiff(["chr1"], cols, coef, (2,), merged=True)
    assert len(d) == n and d.n_columns == p and d.tested == (2,) and d.names == ("x0", "x1", "x2") and d.merged is True
    for name, dt in mdk.ModelDiff.COLUMNS:
        assert getattr(d, name) is cols[name] and getattr(d, name).dtype == getattr(torch, dt)
    assert d.coef is coef
    s = d.select(slice(1, 3))
    assert len(s) == 2 and s.n_columns == p and s.coef.tolist() == [[0.125, 0.25], [0.625, 0.75], [1.125, 1.25]] and s.start.tolist() == [1, 2] and s.names == d.names and s.tested == (2,)
    rows = d.rows()
    assert rows[1] == ("chr1", 1, 1, 1, 1, 1, 1, (0.125, 0.625, 1.125), 1.0, 1, 1.0, 1.0, 1, 1)
    with pytest.raises(mdk.MdkError):
        mdk.ModelDiff(["chr1"], cols, coef, (2,), names=["a", "a", "b"])
    named = mdk.ModelDiff(["chr1"], cols, coef, (1, 2), names=["intercept", "batch", "dose"])
    assert named.names == ("intercept", "batch", "dose") and named.tested == (1, 2)
    lines = [l.rstrip("\n").split("\t") for l in open(named.write(str(tmp_path / "model.tsv")))]
    assert lines[0] == ["#chrom", "start", "end", "context", "strand", "nmeth", "nunmeth", "coef.intercept", "coef.batch", "coef.dose", "pvalue", "df", "dispersion", "statistic",
                        "flags", "iterations"]
    assert len(lines) == n + 1 and lines[2] == ["chr1", "1", "1", "1", "1", "1", "1", "0.125", "0.625", "1.125", "1", "1", "1", "1", "1", "1"]


@pytest.mark.parametrize("floor", [float("nan"), 0.0, -1.0, 2.0 ** -56, 2.0 ** 801, float("inf"), 10 ** 400, True, "1.0", None])
def test_min_dispersion_outside_its_range_is_refused(floor):
    import methyldackel_amd as mdk
    m, u = cpu_matrices()
    with pytest.raises(mdk.MdkError, match="min_dispersion"):
        mdk.diff_model(m, u, DESIGN, 1, min_dispersion=floor)


def test_arguments_are_refused_before_the_library_is_touched(monkeypatch):
    """every refusal that needs no device, with CPU tensors, in _diff_arguments' words under this call's name"""
    import numpy
    import torch
    import methyldackel_amd as mdk

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(mdk, "lib_model", touched)
    monkeypatch.setattr(mdk, "lib_stats", touched)
    m, u = cpu_matrices()
    wide = [[1.0] * 9 for _ in range(6)]
    bad = [row[:] for row in DESIGN]
    bad[3][2] = float("nan")
    large = [row[:] for row in DESIGN]
    large[5][1] = -2.0 ** 20 - 1.0
    cases = [((m, u, DESIGN, 3), {}, "test names column 3: the design has columns 0 to 2"), ((m, u, DESIGN, -1), {}, "test names column -1"),
             ((m, u, DESIGN, [1, 1]), {}, "test names a column twice"), ((m, u, DESIGN, [0, 1, 2]), {}, "3 tested columns of 3: 1 to 2"),
             ((m, u, DESIGN, []), {}, "0 tested columns of 3"), ((m, u, DESIGN, True), {}, "test names column True"), ((m, u, DESIGN, "1"), {}, "test must be a column index"),
             ((m, u, DESIGN, None), {}, "test must be a column index"),
             ((m, u, wide, 1), {}, "a design of 9 columns: 2 to 8"), ((m, u, [[1.0]] * 6, 0), {}, "a design of 1 columns"), ((m, u, [1.0] * 6, 0), {}, "design must be a [samples, columns] matrix"),
             ((m, u, [["a", "b"]] * 6, 1), {}, "design must be a [samples, columns] matrix of numbers"), ((m, u, [[1.0, 2.0], [1.0]], 1), {}, "design must be a"),
             ((m, u, DESIGN[:5], 1), {}, "the design has 5 rows for 6 samples"), ((m, u, DESIGN, 1), {"samples": [0, 1, 2]}, "the design has 6 rows for 3 samples"),
             ((m, u, DESIGN, 1), {"samples": [0, 1, 2, 3, 4, 4]}, "sample 4 is named twice"), ((m, u, DESIGN, 1), {"samples": [0, 1, 2, 3, 4, 6]}, "samples names sample 6: the matrices hold samples 0 to 5"),
             ((m, u, DESIGN, 1), {"samples": [0, 1, 2, 3, 4, -1]}, "samples names sample -1"), ((m, u, DESIGN, 1), {"samples": 6}, "samples must be a sequence"),
             ((m, u, bad, 1), {}, "the design's entry in row 3, column 2 is nan"), ((m, u, large, 2), {}, "the design's entry in row 5, column 1 is -1048577.0"),
             ((m, u.to(torch.int64), DESIGN, 1), {}, "one dtype and one shape"), ((m, u[:, :4], DESIGN, 1), {}, "one dtype and one shape"),
             ((m.to(torch.float32), u, DESIGN, 1), {}, "nmeth must be a"), ((m[0], u[0], DESIGN, 1), {}, "nmeth must be a"),
             ((m[:, ::2], u[:, ::2].contiguous(), DESIGN, 1), {}, "nmeth must be contiguous"), ((m, torch.ones((5, 6), dtype=torch.int32).t(), DESIGN, 1), {}, "nunmeth must be contiguous"),
             ((m, u, DESIGN, 1), {}, "nmeth is a cpu tensor, and there is no CPU path"), ((m, u, DESIGN, [2, 1]), {}, "no CPU path"),
             ((m, u, numpy.array(DESIGN), (2,)), {}, "no CPU path"), ((m, u, torch.tensor(DESIGN, dtype=torch.float32), 1), {}, "no CPU path"),
             ((m, u, DESIGN[:3], 1), {"samples": (5, 0, 2)}, "no CPU path"), ((m, u, [[1, 0], [1, 0], [1, 1], [1, 1], [1, 2], [1, 2]], 1), {}, "no CPU path")]
    for args, kwargs, text in cases:
        with pytest.raises(mdk.MdkError, match=re.escape(text)) as e:
            mdk.diff_model(*args, **kwargs)
        assert "diff_counts" not in str(e.value) and "diff_groups" not in str(e.value)
    for floor in (2.0 ** -55, 2.0 ** 800):
        with pytest.raises(mdk.MdkError, match="no CPU path"):
            mdk.diff_model(m, u, DESIGN, 1, min_dispersion=floor, steps=True)


def test_the_rows_and_columns_are_put_in_the_rule_s_order():
    """_model_arguments: the used samples ascending with their rows, the tested columns last in the order they were named, and the place
    of every column of the caller's among them"""
    import methyldackel_amd as mdk
    design = [[1.0, 10.0, 20.0, 30.0], [1.0, 11.0, 21.0, 31.0], [1.0, 12.0, 22.0, 32.0]]
    S, n, used, rows, p, q, place, tested, dev = _arguments_on_a_pretended_device(mdk, design, [2, 0], [5, 0, 3])
    assert (S, n, p, q) == (6, 5, 4, 2) and used == [0, 3, 5] and tested == (2, 0)
    assert rows == [[11.0, 31.0, 21.0, 1.0], [12.0, 32.0, 22.0, 1.0], [10.0, 30.0, 20.0, 1.0]]
    assert place == [3, 0, 2, 1]
    assert _arguments_on_a_pretended_device(mdk, [[1.0, float(k)] for k in range(6)], 1, None)[2:4] == ([0, 1, 2, 3, 4, 5], [[1.0, float(k)] for k in range(6)])


def _arguments_on_a_pretended_device(mdk, design, test, samples):
    """_model_arguments on tensors that say they are on a device: a subclass whose `device` is cuda:0"""
    import torch

    class Pretended(torch.Tensor):
        @property
        def device(self):
            return torch.device("cuda", 0)
    m = torch.ones((6, 5), dtype=torch.int32).as_subclass(Pretended)
    u = torch.ones((6, 5), dtype=torch.int32).as_subclass(Pretended)
    return mdk._model_arguments("diff_model", m, u, design, test, samples)


def test_cohort_diff_model_takes_the_same_path():
    import torch
    import methyldackel_amd as mdk
    m, u = cpu_matrices()
    cols = {n: torch.zeros(5, dtype=getattr(torch, dt)) for n, dt in mdk.SITE_COLUMNS}
    co = mdk.Cohort(["chr1"], cols, m, u)
    with pytest.raises(mdk.MdkError, match="test names column 7"):
        co.diff_model(DESIGN, 7)
    with pytest.raises(mdk.MdkError, match="min_dispersion"):
        co.diff_model(DESIGN, 1, min_dispersion=0.0)
    with pytest.raises(mdk.MdkError, match="no CPU path"):
        co.diff_model(DESIGN, [1, 2], names=["a", "b", "c"])
