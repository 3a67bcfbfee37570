"""CPU: the tabix rule (csrc/mdk_tabix_core.h) through its host build, tools/tabix_emu.  The emulator's payload must equal the numpy
builder's bit for bit over every table, the file must gunzip to the payload, two runs must give equal files, the reader written from the
specification must answer every region of the grid as brute force over the decompressed file does, and every refusal must name its line."""
import gzip

import pytest

import tabix_rule as T

TABLES = T.cpu_tables()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{table: (BGZF bytes, the emulator's .tbi bytes, the emulator's payload)}"""
    d, out = tmp_path_factory.mktemp("tabix"), {}
    for name, (text, cf, cuts, eof) in TABLES.items():
        raw = T.bgzf(text, cuts, eof)
        assert gzip.decompress(raw) == text
        p = d / f"{name}.gz"
        p.write_bytes(raw)
        for k, flag in enumerate((False, False, True)):
            r = T.emu(p, cf, d / f"{name}.{k}", raw_payload=flag)
            assert r.returncode == 0, (name, r.stderr)
        a, b = (d / f"{name}.0").read_bytes(), (d / f"{name}.1").read_bytes()
        assert a == b, name                                           # two runs, equal files
        out[name] = (raw, a, (d / f"{name}.2").read_bytes())
    return out


@pytest.mark.parametrize("name", list(TABLES))
def test_payload_is_the_builders_and_the_file_gunzips_to_it(files, name):
    text, cf, _, _ = TABLES[name]
    raw, tbi, payload = files[name]
    assert payload == T.payload(text, raw, cf)
    assert gzip.decompress(tbi) == payload
    assert tbi.endswith(T.Z.BGZF_EOF)
    parsed = T.read_tbi(tbi)
    assert parsed["conf"] == cf
    if name in ("header_only", "empty"):
        assert parsed["names"] == [] and len(payload) == 4 + 8 * 4 + 8
    if name in ("bed", "bed_1000"):
        assert parsed["names"] == [b"chrA", b"chrLong"]
        levels = set(parsed["refs"][1][0])                             # every level up to bin 0 occurs
        assert 0 in levels and any(1 <= b < 9 for b in levels) and any(9 <= b < 73 for b in levels) and any(73 <= b < 585 for b in levels) and any(585 <= b < 4681 for b in levels)
    if name == "alternating":
        assert sum(len(c) for b, c in parsed["refs"][0][0].items() if b != 37450) == 380      # a chunk per line
    if name == "meta_lines":
        assert len(parsed["refs"][0][0][4681]) == 1                   # meta lines between two entries of one bin do not break the run


@pytest.mark.parametrize("name", list(TABLES))
def test_reader_answers_as_brute_force(files, name):
    text, cf, _, _ = TABLES[name]
    raw, tbi, _ = files[name]
    parsed = T.read_tbi(tbi)
    names = parsed["names"] or [b"chrA"]
    edges = T.EDGES if name in ("bed", "methylKit", "report") else [0, 1, 100, 1000, 16383, 16384, 16385, 17000, 20001, 131072, 1 << 29]
    hits = 0
    for n, b, e in T.grid(names, edges):
        got = T.query(raw, parsed, n, b, e)
        assert got == T.brute(raw, cf, n, b, e), (name, n, b, e)
        hits += bool(got)
    assert hits or name in ("header_only", "empty")


def test_a_small_region_reads_few_chunks(files):
    raw, tbi, _ = files["bed"]
    parsed, stats = T.read_tbi(tbi), {}
    assert T.query(raw, parsed, b"chrA", 50000, 50100, stats) == T.brute(raw, TABLES["bed"][1], b"chrA", 50000, 50100)
    assert stats["chunks"] == 1


@pytest.mark.parametrize("case", T.refusals(), ids=lambda c: c[0])
def test_every_refusal_names_its_line(tmp_path, case):
    name, text, cf, line, code = case
    with pytest.raises(T.Refused) as e:
        T.entries(text, cf)
    assert (e.value.line, e.value.code) == (line, code)
    for cuts in (65280, 37):
        p = tmp_path / f"{name}.{cuts}.gz"
        p.write_bytes(T.bgzf(text, cuts))
        r = T.emu(p, cf, tmp_path / "out.tbi")
        assert r.returncode == 3 and r.stderr.startswith(f"line {line}: ") and T.MESSAGES[code] in r.stderr, (name, r.stderr)
        assert not (tmp_path / "out.tbi").exists()
