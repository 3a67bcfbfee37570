"""CPU: the F test of three or more groups as the package offers it -- mdk.diff_groups, Cohort.diff_groups, GroupDiff, lib_groups,
include/mdk_gdiff.h -- as far as it goes without a device: the names, the header against what lib_groups() binds, the refusals that are
made before the library is touched, the columns.  The kernel's results are tests/test_gpu_gdiff.py's."""
import re

import pytest

from conftest import REPO


def cpu_matrices(S=6, n=5):
    import torch
    return torch.ones((S, n), dtype=torch.int32), torch.ones((S, n), dtype=torch.int32)


def test_the_names_exist():
    import methyldackel_amd as mdk
    assert callable(mdk.diff_groups) and callable(mdk.lib_groups) and callable(mdk.Cohort.diff_groups)
    assert not issubclass(mdk.GroupDiff, mdk.Diff)
    for method in ("qvalue", "select", "rows", "write", "contrast"):
        assert callable(getattr(mdk.GroupDiff, method)), method
    assert not hasattr(mdk.GroupDiff, "dmrs")
    for doc in (mdk.diff_counts.__doc__, mdk.diff_replicates.__doc__):
        assert "diff_groups" in doc
    assert "Fisher" in mdk.Diff.dmrs.__doc__ and "diff_replicates" in mdk.Diff.dmrs.__doc__


def test_the_header_declares_what_lib_groups_binds(monkeypatch):
    import methyldackel_amd as mdk
    header = (REPO / "include" / "mdk_gdiff.h").read_text()
    declared = set(re.findall(r"\b(md_stats_\w+)\s*\(", header))
    assert declared == {"md_stats_gdiff"}
    assert '#include "mdk_gdiff.h"' in (REPO / "include" / "mdk_stats.h").read_text()
    monkeypatch.setattr(mdk, "_stats", None)
    fresh = {name for name in vars(mdk.lib_stats()) if name.startswith("md_stats_")}
    assert fresh == {"md_stats_open", "md_stats_close", "md_stats_last_error", "md_stats_qdiff"}          # a fresh lib_stats() still binds its four
    L = mdk.lib_groups()
    assert L is mdk.lib_stats()
    assert {name for name in vars(L) if name.startswith("md_stats_")} - fresh == declared
    decl = re.search(r"int md_stats_gdiff\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == 21 == len(L.md_stats_gdiff.argtypes)
    assert mdk.lib_groups() is L and len(L.md_stats_gdiff.argtypes) == 21


def test_columns():
    import methyldackel_amd as mdk
    from gdiff_rule import NAMES
    assert tuple(n for n, _ in mdk.GROUP_RESULT_COLUMNS) == NAMES
    assert mdk.GroupDiff.COLUMNS == mdk.DIFF_SITE_COLUMNS + mdk.GROUP_RESULT_COLUMNS
    assert dict(mdk.GROUP_RESULT_COLUMNS) == {"meth_diff": "float64", "group_lo": "int32", "group_hi": "int32", "pvalue": "float64", "df": "int32",
                                              "df_groups": "int32", "dispersion": "float64", "statistic": "float64"}


def test_group_diff_holds_its_columns_on_the_host():
    """a GroupDiff made by hand from CPU tensors: the columns, the matrices, n_groups, names, select, rows and write need no device"""
    import torch
    import methyldackel_amd as mdk
    n, G = 4, 3
    cols = {name: torch.arange(n, dtype=getattr(torch, dt)) for name, dt in mdk.GroupDiff.COLUMNS}
    cols["contig"] = torch.zeros(n, dtype=torch.int32)
    m, u = torch.arange(G * n, dtype=torch.int64).reshape(G, n), torch.ones((G, n), dtype=torch.int64)
    g = mdk.GroupDiff(["chr1"], cols, m, u, merged=True)
    assert len(g) == n and g.n_groups == G and g.names == ("g0", "g1", "g2") and g.merged is True
    for name, dt in mdk.GroupDiff.COLUMNS:
        assert getattr(g, name) is cols[name] and getattr(g, name).dtype == getattr(torch, dt)
    assert g.nmeth is m and g.nunmeth is u
    s = g.select(slice(1, 3))
    assert len(s) == 2 and s.n_groups == G and s.nmeth.tolist() == [[1, 2], [5, 6], [9, 10]] and s.start.tolist() == [1, 2] and s.names == g.names
    rows = g.rows()
    assert rows[1] == ("chr1", 1, 1, 1, 1, (1, 1), (5, 1), (9, 1), 1.0, 1, 1, 1.0, 1, 1, 1.0, 1.0)
    with pytest.raises(mdk.MdkError):
        mdk.GroupDiff(["chr1"], cols, m, u, names=["a", "a", "b"])
    assert mdk.GroupDiff(["chr1"], cols, m, u, names=["ctl", "het", "hom"]).names == ("ctl", "het", "hom")


@pytest.mark.parametrize("floor", [float("nan"), 0.0, -1.0, 2.0 ** -56, 2.0 ** 801, float("inf"), 10 ** 400, True, "1.0", None])
def test_min_dispersion_outside_its_range_is_refused(floor):
    import methyldackel_amd as mdk
    m, u = cpu_matrices()
    with pytest.raises(mdk.MdkError, match="min_dispersion"):
        mdk.diff_groups(m, u, [[0, 1], [2, 3], [4, 5]], min_dispersion=floor)


def test_arguments_are_refused_before_the_library_is_touched(monkeypatch):
    """every refusal that needs no device, with CPU tensors, in _diff_arguments' words under this call's name"""
    import torch
    import methyldackel_amd as mdk

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(mdk, "lib_groups", touched)
    monkeypatch.setattr(mdk, "lib_stats", touched)
    m, u = cpu_matrices()
    three = [[0, 1], [2, 3], [4, 5]]
    cases = [((m, u, [[0], [], [1]]), "group 1 is empty"), ((m, u, [[0, 1], [1, 2], [3]]), "sample 1 is in both groups"),
             ((m, u, [[0], [1], [6]]), "group 2 names sample 6: the matrices hold samples 0 to 5"), ((m, u, [[-1], [2], [3]]), "group 0 names sample -1"),
             ((m, u, [[0], [True], [2]]), "group 1 names sample True"), ((m, u, [[0, 1, 2]]), "1 groups: 2 to 6"),
             ((m, u, [[0], [1], [2], [3], [4], [5], [0]]), "7 groups: 2 to 6"), ((m, u, []), "0 groups"), ((m, u, 3), "groups must be a sequence"),
             ((m, u, "ab"), "groups must be a sequence"), ((m, u, [[0], "1", [2]]), "group 1 must be a sequence"),
             ((m, u.to(torch.int64), three), "one dtype and one shape"), ((m, u[:, :4], three), "one dtype and one shape"),
             ((m.to(torch.float32), u, three), "nmeth must be a"), ((m[0], u[0], three), "nmeth must be a"),
             ((m[:, ::2], u[:, ::2].contiguous(), three), "nmeth must be contiguous"), ((m, torch.ones((5, 6), dtype=torch.int32).t(), three), "nunmeth must be contiguous"),
             ((m, u, three), "nmeth is a cpu tensor, and there is no CPU path"), ((m, u, [[0, 1], [2, 3]]), "no CPU path"), ((m, u, [0, 1, 2]), "no CPU path"),
             ((m, u, ((5, 4), (1, 0), [3])), "no CPU path")]
    for args, text in cases:
        with pytest.raises(mdk.MdkError, match=re.escape(text)) as e:
            mdk.diff_groups(*args)
        assert "diff_counts" not in str(e.value) and "diff_replicates" not in str(e.value)
    # the words are diff_counts' where it has the same refusal
    for args, text in cases[11:18]:
        with pytest.raises(mdk.MdkError, match=re.escape(text)):
            mdk.diff_counts(args[0], args[1], [0], [1])
    for floor in (2.0 ** -55, 2.0 ** 800):
        with pytest.raises(mdk.MdkError, match="no CPU path"):
            mdk.diff_groups(m, u, three, min_dispersion=floor, steps=True)


def test_cohort_diff_groups_takes_the_same_path():
    import torch
    import methyldackel_amd as mdk
    m, u = cpu_matrices()
    cols = {n: torch.zeros(5, dtype=getattr(torch, dt)) for n, dt in mdk.SITE_COLUMNS}
    co = mdk.Cohort(["chr1"], cols, m, u)
    with pytest.raises(mdk.MdkError, match="both groups"):
        co.diff_groups([[0, 1], [1], [2]])
    with pytest.raises(mdk.MdkError, match="min_dispersion"):
        co.diff_groups([[0, 1], [2, 3], [4]], min_dispersion=0.0)
    with pytest.raises(mdk.MdkError, match="no CPU path"):
        co.diff_groups([[0, 1], [2, 3], [4]], names=["a", "b", "c"])
