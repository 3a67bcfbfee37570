"""CPU: the replicates' F test as the package offers it -- mdk.diff_replicates, Cohort.diff_replicates, ReplicateDiff, libmdk_stats.so's
header -- as far as it goes without a device: the names, the header against what lib_stats() binds, the refusals that are made before
the library is touched, the columns.  The kernel's results are tests/test_gpu_qdiff.py's."""
import re

import pytest

from conftest import REPO


def cpu_matrices(S=4, n=5):
    import torch
    return torch.ones((S, n), dtype=torch.int32), torch.ones((S, n), dtype=torch.int32)


def test_the_names_exist():
    import methyldackel_amd as mdk
    assert callable(mdk.diff_replicates) and callable(mdk.lib_stats) and callable(mdk.Cohort.diff_replicates)
    assert issubclass(mdk.ReplicateDiff, mdk.Diff) and mdk.ReplicateDiff is not mdk.Diff
    assert mdk.LIB_STATS.name == "libmdk_stats.so" and mdk.LIB_STATS.parent == mdk.LIB_INDEX.parent
    for inherited in ("qvalue", "dmrs", "select"):
        assert getattr(mdk.ReplicateDiff, inherited) is getattr(mdk.Diff, inherited), inherited
    assert "Fisher" in mdk.Diff.dmrs.__doc__ and "diff_replicates" in mdk.Diff.dmrs.__doc__


def test_the_header_declares_what_lib_stats_binds(monkeypatch):
    import methyldackel_amd as mdk
    header = (REPO / "include" / "mdk_stats.h").read_text()
    declared = set(re.findall(r"\b(md_stats_\w+)\s*\(", header))
    monkeypatch.setattr(mdk, "_stats", None)                       # a fresh load holds what lib_stats() and the loader under it bound, and no more
    bound = {name for name in vars(mdk.lib_stats()) if name.startswith("md_stats_")}
    assert bound == {"md_stats_open", "md_stats_close", "md_stats_last_error", "md_stats_qdiff"}
    assert bound <= declared, bound - declared
    # the call's arguments, one by one: the binding has as many as the declaration
    decl = re.search(r"int md_stats_qdiff\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == 20
    L = mdk.lib_stats()                                            # (loading it needs no device)
    assert len(L.md_stats_qdiff.argtypes) == 20 and len(L.md_stats_open.argtypes) == 2
    for name in bound:
        assert getattr(L, name) is not None
    assert re.search(r"MD_STATS_ERR_ARG = -3\b", header) and re.search(r"MD_STATS_ERR_HIP = -2\b", header) and re.search(r"MD_STATS_ERR_NOMEM = -4\b", header)


def test_columns():
    import methyldackel_amd as mdk
    assert mdk.ReplicateDiff.COLUMNS == mdk.Diff.COLUMNS + (("df", "int32"), ("dispersion", "float64"), ("statistic", "float64"))
    from qdiff_rule import NAMES
    assert tuple(n for n, _ in mdk.ReplicateDiff.COLUMNS[5:]) == NAMES


@pytest.mark.parametrize("floor", [float("nan"), 0.0, -1.0, 2.0 ** -56, 2.0 ** 801, float("inf"), 10 ** 400, True, "1.0", None])
def test_min_dispersion_outside_its_range_is_refused(floor):
    import methyldackel_amd as mdk
    m, u = cpu_matrices()
    with pytest.raises(mdk.MdkError, match="min_dispersion"):
        mdk.diff_replicates(m, u, [0, 1], [2, 3], min_dispersion=floor)


def test_arguments_are_refused_as_diff_counts_refuses_them():
    """every refusal that needs no device, with CPU tensors: the wording is diff_counts's under this call's name"""
    import torch
    import methyldackel_amd as mdk
    m, u = cpu_matrices()
    cases = [((m, u, [], [1]), "group a is empty"), ((m, u, [0], []), "group b is empty"), ((m, u, [0, 1], [1, 2]), "sample 1 is in both groups"),
             ((m, u, [0], [4]), "group b names sample 4"), ((m, u, [-1], [2]), "group a names sample -1"), ((m, u, [0], [True]), "group b names sample True"),
             ((m, u.to(torch.int64), [0], [1]), "one dtype and one shape"), ((m, u[:, :4], [0], [1]), "one dtype and one shape"),
             ((m.to(torch.float32), u, [0], [1]), "nmeth must be a"), ((m[0], u[0], [0], [1]), "nmeth must be a"),
             ((m[:, ::2], u[:, ::2].contiguous(), [0], [1]), "nmeth must be contiguous"), ((m, torch.ones((5, 4), dtype=torch.int32).t(), [0], [1]), "nunmeth must be contiguous"),
             ((m, u, [0, 1], [2, 3]), "nmeth is a cpu tensor, and there is no CPU path")]
    for args, text in cases:
        with pytest.raises(mdk.MdkError, match=re.escape(text)) as e:
            mdk.diff_replicates(*args)
        assert "diff_counts" not in str(e.value)
        with pytest.raises(mdk.MdkError, match=re.escape(text)):
            mdk.diff_counts(*args)
    # limits of the two at the highest valid values: still only the device is missing
    with pytest.raises(mdk.MdkError, match="no CPU path"):
        mdk.diff_replicates(m, u, [0], [1], min_dispersion=2.0 ** -55)
    with pytest.raises(mdk.MdkError, match="no CPU path"):
        mdk.diff_replicates(m, u, [0], [1], min_dispersion=2.0 ** 800, steps=True)


def test_cohort_diff_replicates_takes_the_same_path():
    import torch
    import methyldackel_amd as mdk
    m, u = cpu_matrices()
    cols = {n: torch.zeros(5, dtype=getattr(torch, dt)) for n, dt in mdk.SITE_COLUMNS}
    co = mdk.Cohort(["chr1"], cols, m, u)
    with pytest.raises(mdk.MdkError, match="both groups"):
        co.diff_replicates([0, 1], [1])
    with pytest.raises(mdk.MdkError, match="min_dispersion"):
        co.diff_replicates([0, 1], [2, 3], min_dispersion=0.0)
    with pytest.raises(mdk.MdkError, match="no CPU path"):
        co.diff_replicates([0, 1], [2, 3])
