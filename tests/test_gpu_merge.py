"""GPU: mergeContext over rows on the device (k_merge_len / k_merge_blocks / k_merge_fill, csrc/mdk_merge.hip) -- Calls.merge_context and
Cytosines.merge_context.  Every comparison is exact: against the Python restatement of the rule (tests/merge_rule.py), against this build's
`MethylDackel mergeContext` on the written file, and against the session's own `extract --mergeContext`."""
import ctypes as C
import subprocess

import pytest

from merge_rule import COLUMNS, DTYPES, ERRORS, MESSAGES, SIZES, expected, merge_rows, table

pytestmark = pytest.mark.gpu
CTX = ("CpG", "CHG", "CHH")


def calls_of(columns, contigs=("c0", "c1", "c2")):
    """a Calls of numpy columns or of (contig, start, end, nmeth, nunmeth, context, strand) tuples, on the device: no BAM"""
    import numpy as np
    import torch
    import methyldackel_amd as mdk
    if not (columns and isinstance(columns[0], np.ndarray)):
        columns = [np.array([r[k] for r in columns], dtype=dt) for k, dt in enumerate(DTYPES)]
    return mdk.Calls(list(contigs), {n: torch.from_numpy(c.copy()).cuda() for n, c in zip(COLUMNS, columns)})


def rows_of(c):
    return list(zip(*[getattr(c, n).cpu().tolist() for n in COLUMNS]))


def same_columns(a, b):
    import torch
    return len(a) == len(b) and all(torch.equal(getattr(a, n), getattr(b, n)) for n in COLUMNS)


# first in the file: the kernels' first execution
@pytest.mark.parametrize("n", SIZES)
def test_blocking_on_the_device(n):
    import torch
    c = calls_of(list(table(n)))
    for depth in (1, 5):
        m = c.merge_context(depth)
        assert m.merged and m.contigs == c.contigs and m.contexts_on == c.contexts_on
        for name, dt in zip(COLUMNS, DTYPES):
            t = getattr(m, name)
            assert t.dtype == getattr(torch, dt) and t.device == c.start.device and t.is_contiguous()
            assert len(m) == 0 or t.data_ptr() != getattr(c, name).data_ptr()          # new tensors, not views of the input
        assert rows_of(m) == list(expected(n, depth)), (n, depth)
    assert rows_of(c) == list(zip(*[col.tolist() for col in table(n)]))          # the input is as it was


@pytest.mark.parametrize("name,rows", ERRORS, ids=[f"{e[0]}{i}" for i, e in enumerate(ERRORS)])
def test_refused_rows(name, rows):
    """flagged by the measuring pass: alone, and as rows 255 / 256 of a longer table, where the faulty row's neighbour belongs to another workgroup"""
    import methyldackel_amd as mdk
    pad = [(0, k, k + 1, 1, 1, 2, 1) for k in range(256 - len(rows) + 1)]
    tables = [rows]
    if name not in ("lone_g", "contig") and rows[0][0] == 0:
        tables.append(pad + [(c, a + 1000, b + 1000, m, u, t, s) for c, a, b, m, u, t, s in rows])
    for tab in tables:
        with pytest.raises(mdk.MdkError, match=MESSAGES[name]) as e:
            calls_of(tab, ("a", "b")).merge_context(0)
        assert e.value.rc == -3


def test_changed_columns_end_the_fill():
    """the ABI's two steps with the counts raised in between: more rows pass the depth cut than were measured.  The fill says so and writes
    nothing past the measured rows (the buffers here hold a row per input row in any case)"""
    import torch
    import methyldackel_amd as mdk
    n = 513
    c = calls_of(list(table(n)))
    L = c._renderer(c.start.device)
    view = mdk.md_text_cols(*[C.c_void_p(getattr(c, name).data_ptr()) for name in COLUMNS])
    rows = C.c_int64()
    torch.cuda.synchronize()
    assert L.md_text_merge_measure(c._text.h, C.byref(view), n, 5, C.byref(rows)) == 0 and rows.value == len(expected(n, 5))
    out = {name: torch.full((n,), 77, dtype=getattr(torch, dt), device="cuda") for name, dt in zip(COLUMNS, DTYPES)}
    dst = mdk.md_text_cols(*[C.c_void_p(out[name].data_ptr()) for name in COLUMNS])
    assert L.md_text_merge_fill(c._text.h, C.byref(dst), rows.value + 1) == -3          # not the measured size
    c.nmeth += 9
    torch.cuda.synchronize()
    assert L.md_text_merge_fill(c._text.h, C.byref(dst), rows.value) == -3
    assert b"not the ones that were measured" in L.md_dev_last_error()
    assert all(int((t[rows.value:] != 77).sum()) == 0 for t in out.values())
    c.nmeth -= 9
    torch.cuda.synchronize()
    assert L.md_text_merge_fill(c._text.h, C.byref(dst), rows.value) == 0
    assert list(zip(*[out[name][:rows.value].cpu().tolist() for name in COLUMNS])) == list(expected(n, 5))
    # a text measure on the same renderer voids the merge's: there is one block table
    c.render("counts", header=False)
    assert L.md_text_merge_fill(c._text.h, C.byref(dst), rows.value) == -3


@pytest.fixture(scope="module")
def session():
    import methyldackel_amd as mdk
    s = mdk.Session(0)
    yield s
    s.close()


def test_session_result_equals_the_tool_and_extract_mergecontext(session, small_synth, tmp_path):
    import methyldackel_amd as mdk
    fa, bam = small_synth / "pe.fa", small_synth / "pe.bam"
    args = [fa, bam, "--CHG", "--CHH"]
    c = session.extract(args)
    m = c.merge_context()
    assert m.merged and not c.merged and m.contexts_on == (0, 1, 2) and 0 < len(m) < len(c)
    c.write("s", directory=str(tmp_path)); m.write("m", directory=str(tmp_path))
    for ctx in CTX:
        tool = subprocess.run([str(mdk.CLI), "mergeContext", str(fa), str(tmp_path / f"s_{ctx}.bedGraph")], cwd=tmp_path, capture_output=True, text=True)
        assert tool.returncode == 0, tool.stderr
        got = (tmp_path / f"m_{ctx}.bedGraph").read_text().splitlines()
        assert got[1:] == tool.stdout.splitlines()[1:] and len(got) > 500, ctx
    assert " merged" in (tmp_path / "m_CpG.bedGraph").read_text().splitlines()[0]
    e = session.extract(args + ["--mergeContext"])
    assert e.merged and same_columns(m, e)
    assert int((m.strand[m.context < 2] != 0).sum()) == 0 and int((m.strand[m.context == 2] == 0).sum()) == 0
    e10 = session.extract(args + ["--mergeContext", "-d", "10"])
    assert same_columns(c.merge_context(min_depth=10), e10) and 0 < len(e10) < len(e)


def test_a_filtered_input(session, small_synth):
    c = session.extract([small_synth / "pe.fa", small_synth / "pe.bam", "--CHG", "--CHH"])
    f = c.select(c.nmeth + c.nunmeth >= 3)
    assert 0 < len(f) < len(c)
    assert rows_of(f.merge_context()) == merge_rows(rows_of(f), 1)


def test_cytosines(session, small_synth):
    import torch
    args = [small_synth / "pe.fa", small_synth / "pe.bam", "--CHG"]
    y, y2 = session.cytosine_report(args), session.cytosine_report(args + ["-q", "40", "-p", "30"])
    m, m2 = y.merge_context(), y2.merge_context()
    view = list(zip(y.contig.cpu().tolist(), (y.pos - 1).cpu().tolist(), y.pos.cpu().tolist(), y.nmeth.cpu().tolist(), y.nunmeth.cpu().tolist(), y.context.cpu().tolist(), y.strand.cpu().tolist()))
    assert rows_of(m) == merge_rows(view, 0) and m.merged and 0 < len(m) < len(y)
    assert int((m.nmeth + m.nunmeth == 0).sum()) > 0
    for name in ("contig", "start", "end", "context"):
        assert torch.equal(getattr(m, name), getattr(m2, name)), name
    assert not torch.equal(m.nmeth, m2.nmeth) and not torch.equal(m.nunmeth, m2.nunmeth)
    assert torch.stack([m.nmeth, m2.nmeth]).shape == (2, len(m))


def test_refusals_on_device_tensors(session, small_synth):
    import torch
    import methyldackel_amd as mdk
    c = session.extract([small_synth / "pe.fa", small_synth / "pe.bam", "--CHG", "--CHH"])
    m = c.merge_context()
    with pytest.raises(mdk.MdkError, match="merged already"):
        m.merge_context()
    g = torch.Generator().manual_seed(3)
    shuffled = c.select(torch.randperm(len(c), generator=g).to(c.start.device))
    with pytest.raises(mdk.MdkError, match="not ascending") as e:
        shuffled.merge_context()
    assert e.value.rc == -3
    assert same_columns(c.merge_context(), m)            # and the renderer goes on working
