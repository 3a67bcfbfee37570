"""CPU-only: significant sites joined into regions (csrc/mdk_dmr_core.h, the functions the kernels of csrc/mdk_dmr.hip run), driven
through tools/dmr_emu, which walks the kernels' decomposition -- blocks of 256 rows, wavefronts of 64, the block table, prefix
differences plus partial blocks: its regions against the restatement in Python loops (tests/dmr_rule.py), the doubles as 64-bit
patterns; the cases by hand; and what Diff.dmrs refuses without a device."""
import struct
import subprocess

import pytest

import methyldackel_amd as mdk
from conftest import REPO
from diff_rule import LIMIT, bits
from dmr_rule import CONTIGS, HAND, PARAMS, SIMPSON, SIZES, Refused, census, dmrs, refusal_tables, site, table

EMU = REPO / "tools" / "_build" / "dmr_emu"
MASK = 2 ** 64 - 1


def emu(rows, sig, n_contigs, max_gap, max_skip, min_sites, min_diff):
    """the regions as the host build of the header gives them, the doubles as patterns; ("refused", bit, row) for a refused table"""
    text = "%d %d %d %d %d %016x\n" % (len(rows), n_contigs, max_gap, max_skip, min_sites, bits(float(min_diff)) & MASK)
    text += "".join("%d %d %d %d %d %d %d %d\n" % (r + (int(bool(s)),)) for r, s in zip(rows, sig))
    r = subprocess.run([str(EMU)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    if lines and lines[0].startswith("refused"):
        return ("refused",) + tuple(int(x) for x in lines[0].split()[1:])
    return [tuple(int(x, 16) if k >= 10 else int(x) for k, x in enumerate(l.split("\t"))) for l in lines]


def patterns(regions):
    """the rule's regions as the emulator prints them"""
    return [r[:10] + (bits(r[10]) & MASK, bits(r[11]) & MASK) for r in regions]


@pytest.mark.parametrize("n", SIZES)
def test_emulator_equals_the_rule_on_seeded_tables(n):
    """Every table holds, by the rule alone, at least two kept regions of two candidates or more, one region min_sites alone drops and
    one min_diff alone drops -- but the table of ONE row, which cannot hold seven: it is one candidate, kept at min_sites 1 and dropped
    at min_sites 2"""
    rows, sig = table(n)
    assert len(rows) == n
    if n == 1:
        assert len(dmrs(rows, sig, len(CONTIGS), 300, 1, 1, 20.0)) == 1 and dmrs(rows, sig, len(CONTIGS), 300, 1, 2, 20.0) == []
    else:
        got = census(rows, sig, len(CONTIGS), **PARAMS)
        assert got["kept2"] >= 2 and got["by_min_sites"] >= 1 and got["by_min_diff"] >= 1, got
    for params in (PARAMS, dict(PARAMS, min_sites=1), dict(PARAMS, max_skip=0, min_diff=0.0), dict(max_gap=40, max_skip=3, min_sites=3, min_diff=35.0)):
        want = dmrs(rows, sig, len(CONTIGS), **params)
        assert emu(rows, sig, len(CONTIGS), **params) == patterns(want), params
        assert [r[:2] for r in want] == sorted(r[:2] for r in want)


@pytest.mark.parametrize("name,rows,sig,params,want", HAND, ids=[h[0] for h in HAND])
def test_by_hand(name, rows, sig, params, want):
    rule = dmrs(rows, sig, len(CONTIGS), **params)
    assert [r[:10] for r in rule] == want
    assert emu(rows, sig, len(CONTIGS), **params) == patterns(rule)


def test_simpson_is_dropped_and_its_sites_alone_are_regions():
    for min_diff in (0.0, 1.0, 40.0):
        for f in (dmrs, emu):
            assert f(SIMPSON, [1, 1], 1, max_gap=10, max_skip=0, min_sites=1, min_diff=min_diff) == []
    alone = dmrs(SIMPSON, [1, 1], 1, max_gap=0, max_skip=0, min_sites=1, min_diff=0.0)
    assert [r[:10] for r in alone] == [(0, 100, 101, 1, 1, 1, 1, 9, 20, 80), (0, 101, 102, 1, 1, 1, 80, 20, 9, 1)]
    assert emu(SIMPSON, [1, 1], 1, 0, 0, 1, 0.0) == patterns(alone)


def test_the_filter_at_its_edges():
    rows, sig = table(257)
    raw = dmrs(rows, sig, len(CONTIGS), 300, 1, 1, 0.0)
    r = next(r for r in raw if r[4] >= 3 and abs(r[10]) > 0.0)
    for f, wrap in ((dmrs, lambda x: x), (emu, patterns)):
        # nsig == min_sites is kept, min_sites - 1 + 1 is not
        assert wrap([r]) == [x for x in f(rows, sig, len(CONTIGS), 300, 1, r[4], 0.0) if x[:2] == r[:2]]
        assert not [x for x in f(rows, sig, len(CONTIGS), 300, 1, r[4] + 1, 0.0) if x[:2] == r[:2]]
        # |meth_diff| == min_diff exactly is kept; the next double above drops it
        edge = abs(r[10])
        above = struct.unpack("<d", struct.pack("<q", bits(edge) + 1))[0]
        assert wrap([r]) == [x for x in f(rows, sig, len(CONTIGS), 300, 1, 1, edge) if x[:2] == r[:2]]
        assert not [x for x in f(rows, sig, len(CONTIGS), 300, 1, 1, above) if x[:2] == r[:2]]


@pytest.mark.parametrize("name,rows,sig,bit,first", refusal_tables(), ids=[r[0] for r in refusal_tables()])
def test_refusals_name_the_first_row(name, rows, sig, bit, first):
    with pytest.raises(Refused) as e:
        dmrs(rows, sig, len(CONTIGS), **PARAMS)
    assert (e.value.bit, e.value.row) == (bit, first)
    assert emu(rows, sig, len(CONTIGS), **PARAMS) == ("refused", bit, first)
    if name == "pooled margin":
        # margins are checked before the filter: the answer does not depend on min_sites
        assert emu(rows, sig, len(CONTIGS), **dict(PARAMS, min_sites=100)) == ("refused", bit, first)


def test_just_inside_the_bounds_is_accepted():
    """an entry of 2^26 - 1, and a region whose pooled methylated count is 2^26 - 1"""
    rows = [site(0, 10, (LIMIT // 2 - 3, 0), (3, 5)), site(0, 11, (LIMIT // 2 - 4, 0), (3, 5)), site(1, 5, (0, LIMIT - 1), (1, 0))]
    want = dmrs(rows, [1, 1, 1], 2, 10, 0, 1, 0.0)
    assert [r[:10] for r in want] == [(0, 10, 12, 2, 2, -1, LIMIT - 7, 0, 6, 10), (1, 5, 6, 1, 1, 1, 0, LIMIT - 1, 1, 0)]
    assert emu(rows, [1, 1, 1], 2, 10, 0, 1, 0.0) == patterns(want)


def hand_diff(device=None):
    import torch
    rows = HAND[0][1]
    names = ("contig", "start", "end", "nmeth_a", "nunmeth_a", "nmeth_b", "nunmeth_b")
    cols = {n: torch.tensor([r[k] for r in rows], dtype=getattr(torch, dict(mdk.Diff.COLUMNS)[n]), device=device) for k, n in enumerate(names)}
    for n, dt in mdk.Diff.COLUMNS:
        cols.setdefault(n, torch.zeros(len(rows), dtype=getattr(torch, dt), device=device))
    return mdk.Diff(list(CONTIGS), cols)


def test_module_constants():
    assert {"md_text_dmr_measure", "md_text_dmr_fill"} <= set(mdk.HIP_SYMBOLS)
    assert [n for n, _ in mdk.DMR_COLUMNS] == ["contig", "start", "end", "nsites", "nsig", "direction", "nmeth_a", "nunmeth_a", "nmeth_b", "nunmeth_b", "meth_diff", "pvalue"]
    assert dict(mdk.DMR_COLUMNS)["direction"] == "int8" and dict(mdk.DMR_COLUMNS)["nsig"] == "int32" and dict(mdk.DMR_COLUMNS)["nmeth_b"] == "int64"
    assert mdk.Dmrs.COLUMNS == mdk.DMR_COLUMNS and issubclass(mdk.Dmrs, mdk._Columns)


def test_refused_without_a_device():
    import torch
    d = hand_diff()
    mask = torch.ones(3, dtype=torch.bool)
    with pytest.raises(mdk.MdkError, match="joined on the device.*no CPU path"):
        d.dmrs(mask)
    for bad in (mask.to(torch.uint8), mask.to(torch.int32), [True, True, True]):
        with pytest.raises(mdk.MdkError, match="significant must be a torch.bool tensor"):
            d.dmrs(bad)
    for bad in (torch.ones(2, dtype=torch.bool), torch.ones((3, 1), dtype=torch.bool)):
        with pytest.raises(mdk.MdkError, match="significant has the shape"):
            d.dmrs(bad)
    for name, values in (("max_gap", (-1, 2 ** 31, 1.5, True)), ("max_skip", (-1, 2 ** 31, "1")), ("min_sites", (0, -3, 2 ** 31, 2.0))):
        for v in values:
            with pytest.raises(mdk.MdkError, match=name):
                d.dmrs(mask, **{name: v})
    for v in (-0.5, float("nan"), float("inf"), "10", True):
        with pytest.raises(mdk.MdkError, match="min_diff"):
            d.dmrs(mask, min_diff=v)


def test_dmrs_columns_and_file_format(tmp_path):
    """Dmrs without a device: select, rows, intervals, qvalue and the file, whose doubles read back to the same bits"""
    import torch
    from diff_rule import bh
    want = dmrs(SIMPSON + [site(1, 7, (1, 9), (9, 1)), site(1, 9, (2, 9), (9, 3))], [1, 1, 1, 1], 2, 0, 0, 1, 0.0)
    assert len(want) == 4
    r = mdk.Dmrs(["chr1", "chrM"], {n: torch.tensor([w[k] for w in want], dtype=getattr(torch, dt)) for k, (n, dt) in enumerate(mdk.DMR_COLUMNS)}, merged=True)
    assert len(r) == 4 and r.merged
    rows = r.rows()
    assert rows == [("chr1" if w[0] == 0 else "chrM",) + w[1:] for w in want]
    path = r.write(str(tmp_path / "dmr.tsv"))
    back = [l.rstrip("\n").split("\t") for l in open(path)]
    assert all(len(b) == 12 for b in back)
    assert [tuple([b[0]] + [int(x) for x in b[1:10]] + [bits(float(x)) for x in b[10:]]) for b in back] == [w[:10] + (bits(w[10]), bits(w[11])) for w in rows]
    s = r.select(torch.tensor([True, False, False, True]))
    assert s.rows() == [rows[0], rows[3]] and s.merged and s.contigs == r.contigs
    assert r.qvalue().tolist() == bh([w[11] for w in want])
    iv = r.intervals()
    assert isinstance(iv, mdk.Intervals) and iv.contigs == r.contigs and iv.contig is r.contig and iv.start is r.start and iv.end is r.end and len(iv) == 4
