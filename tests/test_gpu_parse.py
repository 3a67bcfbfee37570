"""GPU: text read back into columns on the device (k_parse_len / k_parse_blocks / k_parse_fill, csrc/mdk_parse.hip) -- Calls.read,
Cytosines.read, Calls.sorted and the md_text_parse_* entry points.  Every comparison is exact: against the bytes.split restatement of the rule
(tests/parse_rule.py), against the session's own columns through a write -> read round trip, and against this build's `MethylDackel
mergeContext` on the same files."""
import ctypes as C
import re
import subprocess

import pytest

import parse_rule as R

pytestmark = pytest.mark.gpu
CTX = ("CpG", "CHG", "CHH")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    import methyldackel_amd as mdk
    d = tmp_path_factory.mktemp("parse_ref")
    (d / "ref.fa").write_bytes(R.fasta_text())
    r = mdk.Reference(d / "ref.fa")
    yield r
    r.close()


def rows_of(c, columns=R.CALL_COLUMNS):
    cols = [getattr(c, n).cpu().tolist() for n in columns]
    if columns is R.REPORT_COLUMNS:
        cols[6] = [bytes(t).decode() for t in cols[6]]
    return list(zip(*cols))


def same_columns(a, b, columns=R.CALL_COLUMNS):
    import torch
    return len(a) == len(b) and all(torch.equal(getattr(a, n), getattr(b, n)) for n in columns)


def well_formed(c, columns, dtypes, device):
    import torch
    for name, dt in zip(columns, dtypes):
        t = getattr(c, name)
        assert t.dtype == getattr(torch, dt) and t.device == device and t.is_contiguous() and t.shape[0] == len(c), name


# first in the file: the kernels' first execution
@pytest.mark.parametrize("name", list(R.blocking()))
def test_blocking_on_the_device(ref, tmp_path, name):
    import torch
    import methyldackel_amd as mdk
    (tmp_path / "t.bedGraph").write_bytes(R.blocking()[name])
    c = mdk.Calls.read(tmp_path / "t.bedGraph", ref)
    well_formed(c, R.CALL_COLUMNS, R.CALL_DTYPES, torch.device("cuda", 0))
    assert c.contigs == R.CONTIGS and not c.merged
    assert rows_of(c) == list(R.expected(name)), name
    assert c.contexts_on == tuple(sorted({r[5] for r in R.expected(name)}))


def test_a_span_of_newlines_is_refused_not_crashed(ref, tmp_path):
    import methyldackel_amd as mdk
    (tmp_path / "t.bedGraph").write_bytes(b"\n" * R.SPAN + R.bed_lines(1)[0])
    with pytest.raises(mdk.MdkError, match="line 1: .*an empty line") as e:
        mdk.Calls.read(tmp_path / "t.bedGraph", ref)
    assert e.value.rc == -3
    (tmp_path / "u.bedGraph").write_bytes(R.bed_lines(1)[0] + b"x\n" * (R.SPAN // 2) + R.bed_lines(1)[0])
    with pytest.raises(mdk.MdkError, match="line 2: .*too few fields"):
        mdk.Calls.read(tmp_path / "u.bedGraph", ref)


@pytest.fixture(scope="module")
def session():
    import methyldackel_amd as mdk
    s = mdk.Session(0)
    yield s
    s.close()


def test_calls_round_trip(session, small_synth, tmp_path):
    import methyldackel_amd as mdk
    fa, bam = small_synth / "pe.fa", small_synth / "pe.bam"
    c = session.extract([fa, bam, "--CHG", "--CHH"])
    paths = c.write("s", directory=str(tmp_path))
    with mdk.Reference(fa) as fasta:
        assert c.contigs == fasta.contigs                  # the BAM header's order is the FASTA's: contig indices mean the same on both sides
        back = mdk.Calls.read(paths, fasta)
        assert len(back) == len(c) > 5000 and not back.merged and back.contexts_on == (0, 1, 2) and back.contigs == c.contigs
        assert back.context.cpu().tolist() == sorted(back.context.cpu().tolist())          # the order of the paths, then of the lines
        s = back.sorted()
        assert same_columns(s, c)
        # the `mergeContext` command from the warm process: per file, and of the three files read together
        s.merge_context().write("q", directory=str(tmp_path))
        for ctx, path in zip(CTX, paths):
            tool = subprocess.run([str(mdk.CLI), "mergeContext", str(fa), str(path)], cwd=tmp_path, capture_output=True, text=True)
            assert tool.returncode == 0, tool.stderr
            got = (tmp_path / f"q_{ctx}.bedGraph").read_text().splitlines()
            assert got[1:] == tool.stdout.splitlines()[1:] and len(got) > 500, ctx
            one = mdk.Calls.read(path, fasta).merge_context()
            assert one.contexts_on == (CTX.index(ctx),)
            one.write("one", directory=str(tmp_path))
            assert (tmp_path / f"one_{ctx}.bedGraph").read_text().splitlines()[1:] == tool.stdout.splitlines()[1:]
        # what was read renders to the bytes it was read from
        for k, path in enumerate(paths):
            assert bytes(back.render(context=k, prefix="s").cpu().numpy()) == open(path, "rb").read()


def test_cytosines_round_trip(session, small_synth, tmp_path):
    import torch
    import methyldackel_amd as mdk
    cy = session.cytosine_report([small_synth / "pe.fa", small_synth / "pe.bam", "--CHG", "--CHH"])
    path = cy.write("r", directory=str(tmp_path))
    back = mdk.Cytosines.read(path, cy.contigs)
    well_formed(back, R.REPORT_COLUMNS, R.REPORT_DTYPES, torch.device("cuda", 0))
    assert len(back) == len(cy) > 10000 and back.trinucleotide.shape == (len(cy), 3) and back.contexts_on == (0, 1, 2)
    assert same_columns(back, cy, R.REPORT_COLUMNS)
    assert bytes(back.render().cpu().numpy()) == open(path, "rb").read()
    assert same_columns(back.merge_context(), cy.merge_context())
    assert same_columns(mdk.Cytosines.read(path, cy.contigs, block_bytes=5000), cy, R.REPORT_COLUMNS)


def test_block_sizes(ref, tmp_path, monkeypatch):
    import methyldackel_amd as mdk
    text = R.HEADER + R.fill(R.SPAN - len(R.HEADER)) + b"".join(R.bed_lines(700, 12)) + R.HEADER + R.line_of(R.MAX_LINE) + b"".join(R.bed_lines(50, 13))[:-1]
    path = tmp_path / "t.bedGraph"
    path.write_bytes(text)
    want, bad = R.parse_text(text, R.BEDGRAPH, R.CONTIGS, R.reference())
    assert not bad and len(want) > 750
    whole = mdk.Calls.read(path, ref)
    assert rows_of(whole) == want
    for b in (R.MAX_LINE, 4096, 4097, len(text) - 1, len(text)):
        assert same_columns(mdk.Calls.read(path, ref, block_bytes=b), whole), b
    monkeypatch.setenv("MDK_PARSE_BLOCK_BYTES", "5000")
    assert same_columns(mdk.Calls.read([path, path], ref), whole.select(list(range(len(whole))) * 2))
    monkeypatch.delenv("MDK_PARSE_BLOCK_BYTES")
    short = tmp_path / "short.bedGraph"
    short.write_bytes(b"".join(R.bed_lines(30, 14)))
    assert same_columns(mdk.Calls.read(short, ref, block_bytes=100), mdk.Calls.read(short, ref))
    for b in (100, 511):
        with pytest.raises(mdk.MdkError, match="a line longer than block_bytes"):
            mdk.Calls.read(path, ref, block_bytes=b)
    with pytest.raises(mdk.MdkError, match="block_bytes must be"):
        mdk.Calls.read(path, ref, block_bytes=-1)


REFUSALS = R.refusals()


@pytest.mark.parametrize("ident,name,fmt,bad", REFUSALS, ids=[x[0] for x in REFUSALS])
def test_refusals(ref, tmp_path, ident, name, fmt, bad):
    """every refusal between good lines and as the line over a span edge: MdkError with rc -3, the message, the path and the line"""
    import methyldackel_amd as mdk
    path = tmp_path / ("t.txt" if fmt == R.REPORT else "t.bedGraph")
    read = (lambda **k: mdk.Cytosines.read(path, R.CONTIGS, **k)) if fmt == R.REPORT else (lambda **k: mdk.Calls.read(path, ref, **k))
    for edge in (False, True):
        text, at = R.around(bad, fmt, edge)
        path.write_bytes(text)
        line = text[:at].count(b"\n") + 1
        with pytest.raises(mdk.MdkError, match=R.MESSAGES[name]) as e:
            read()
        assert e.value.rc == -3 and f"{path}, line {line}:" in str(e.value), str(e.value)
        path.write_bytes(text[:at] + text[at + len(bad):])
        assert len(read()) == text.count(b"\n") - 1 - text.count(b"track")


def test_where_the_refused_line_is(ref, tmp_path):
    """line 1, the last line without its newline, a line of the second piece, and of two refused lines the earlier"""
    import methyldackel_amd as mdk
    bad = R.bed_line(0, R.other_base(0), 1, 1)
    good = R.bed_lines(300, 15)
    path = tmp_path / "t.bedGraph"
    for text, line, kw in ((bad + b"".join(good), 1, {}), (b"".join(good) + bad[:-1], 301, {}), (b"".join(good) + bad + b"".join(good), 301, {"block_bytes": 1000}),
                           (R.HEADER + b"".join(good) + bad[:-1], 302, {"block_bytes": 600}), (b"".join(good[:200]) + b"zz\t1\t2\t0\t1\t1\n" + b"".join(good) + bad, 201, {})):
        path.write_bytes(text)
        with pytest.raises(mdk.MdkError, match=f"line {line}: ") as e:
            mdk.Calls.read(path, ref, **kw)
        assert e.value.rc == -3 and str(path) in str(e.value) and re.search(R.MESSAGES["contig" if line == 201 else "base"], str(e.value))
    # the second file of a list
    ok = tmp_path / "ok.bedGraph"
    ok.write_bytes(b"".join(good))
    with pytest.raises(mdk.MdkError, match=re.escape(str(path)) + ", line 201: "):
        mdk.Calls.read([ok, path], ref)


def device_text(text):
    import numpy as np
    import torch
    return torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()


def test_changed_text_ends_the_fill(ref):
    """the ABI's two steps with the text altered in between: a newline gone from one span, newlines added to another.  The fill says so and
    writes nothing past the measured rows"""
    import torch
    import methyldackel_amd as mdk
    text = R.blocking()["and at 8192"]
    want = list(R.expected("and at 8192"))
    t = ref._renderer(0)
    L = t.L
    d = device_text(text)
    rows = C.c_int64()
    torch.cuda.synchronize()
    assert L.md_text_parse_measure(t.h, C.c_void_p(d.data_ptr()), len(text), R.BEDGRAPH, C.byref(rows)) == 0 and rows.value == len(want)
    n = rows.value + 64
    out = {name: torch.full((n,), 77, dtype=getattr(torch, dt), device="cuda") for name, dt in zip(R.CALL_COLUMNS, R.CALL_DTYPES)}
    dst = mdk.md_text_cols(*[C.c_void_p(out[name].data_ptr()) for name in R.CALL_COLUMNS])
    torch.cuda.synchronize()
    assert L.md_text_parse_fill_calls(t.h, C.byref(dst), rows.value + 1) == -3            # not the measured size
    assert L.md_text_parse_fill_cytosines(t.h, C.byref(dst), rows.value) == -3           # not the measured format
    first, later = text.index(b"\n"), text.index(b"\n", R.SPAN + 100)
    for at, byte in ((first, ord("x")), (later + 1, 10), (later + 2, 10)):
        keep = int(d[at])
        d[at] = byte
        torch.cuda.synchronize()
        assert L.md_text_parse_fill_calls(t.h, C.byref(dst), rows.value) == -3
        assert b"not the one that was measured" in L.md_dev_last_error() and L.md_text_parse_error_offset(t.h) == -1
        assert all(int((v[rows.value:] != 77).sum()) == 0 for v in out.values())
        d[at] = keep
    torch.cuda.synchronize()
    assert L.md_text_parse_fill_calls(t.h, C.byref(dst), rows.value) == 0
    assert list(zip(*[out[name][:rows.value].cpu().tolist() for name in R.CALL_COLUMNS])) == want
    assert all(int((v[rows.value:] != 77).sum()) == 0 for v in out.values())
    # a measure of another kind on the same renderer voids this one: there is one block table
    c = mdk.Calls(R.CONTIGS, {name: out[name][:rows.value].contiguous() for name in R.CALL_COLUMNS})
    c._text = t
    c.render("counts", header=False)
    assert L.md_text_parse_fill_calls(t.h, C.byref(dst), rows.value) == -3
    # an unaligned text is refused by the measure
    assert L.md_text_parse_measure(t.h, C.c_void_p(d.data_ptr() + 1), len(text) - 1, R.BEDGRAPH, C.byref(rows)) == -3


def test_a_bedgraph_without_a_resident_reference_is_refused_by_name():
    import torch
    import methyldackel_amd as mdk
    L = mdk._text_lib()
    t = mdk._TextRenderer(L, 0, R.CONTIGS)
    text = b"".join(R.bed_lines(3))
    d = device_text(text)
    rows = C.c_int64()
    torch.cuda.synchronize()
    assert L.md_text_parse_measure(t.h, C.c_void_p(d.data_ptr()), len(text), R.BEDGRAPH, C.byref(rows)) == 0 and rows.value == 3
    out = {name: torch.zeros(3, dtype=getattr(torch, dt), device="cuda") for name, dt in zip(R.CALL_COLUMNS, R.CALL_DTYPES)}
    dst = mdk.md_text_cols(*[C.c_void_p(out[name].data_ptr()) for name in R.CALL_COLUMNS])
    torch.cuda.synchronize()
    assert L.md_text_parse_fill_calls(t.h, C.byref(dst), 3) == -3
    assert b"no resident reference" in L.md_dev_last_error() and L.md_text_parse_error_offset(t.h) == 0
    # one contig resident: its lines are taken, the others' are not; dropped again, none is
    only = [l for l in R.bed_lines(40) if l.startswith(b"c10\t")]
    text = b"".join(only)
    d = device_text(text)
    bases = R.reference()[1]
    assert L.md_text_reference(t.h, 1, bases, len(bases)) == 0
    torch.cuda.synchronize()
    assert L.md_text_parse_measure(t.h, C.c_void_p(d.data_ptr()), len(text), R.BEDGRAPH, C.byref(rows)) == 0 and rows.value == len(only) > 3
    out = {name: torch.zeros(rows.value, dtype=getattr(torch, dt), device="cuda") for name, dt in zip(R.CALL_COLUMNS, R.CALL_DTYPES)}
    dst = mdk.md_text_cols(*[C.c_void_p(out[name].data_ptr()) for name in R.CALL_COLUMNS])
    torch.cuda.synchronize()
    assert L.md_text_parse_fill_calls(t.h, C.byref(dst), rows.value) == 0
    assert list(zip(*[out[name].cpu().tolist() for name in R.CALL_COLUMNS])) == R.parse_text(text, R.BEDGRAPH, R.CONTIGS, R.reference())[0]
    assert L.md_text_reference(t.h, 1, None, 0) == 0
    assert L.md_text_parse_fill_calls(t.h, C.byref(dst), rows.value) == -3 and b"no resident reference" in L.md_dev_last_error()
    assert L.md_text_reference(t.h, 3, bases, len(bases)) == -3
