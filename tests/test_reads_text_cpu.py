"""CPU: the perRead line of the device text formatter without a GPU, and what Reads / Bias do on the host.  csrc/mdk_text_core.h holds the
functions k_rtext_len / k_rtext_fill (csrc/mdk_text.hip) run -- txt_read_line_len, txt_put_read_tail, txt_copy_words --, and
tools/text_emu.cpp compiles them for the host: its --selfcheck-reads compares the line with the snprintf calls of the command,
--emulate-reads runs the fill's workgroup (staged name span, image, direct path), and --render perRead turns rows back into the committed
goldens.  Also here: Bias.render against the mbias goldens, Reads.select on CPU tensors, and the refusals that need no device.  The kernels
themselves are compared with the command's files on the GPU (tests/test_gpu_reads_text.py)."""
import json
import subprocess

import pytest

from conftest import GOLDEN, REPO

EMU = REPO / "tools" / "_build" / "text_emu"
EXPECTED = GOLDEN / "expected"


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", str(REPO), "tools/_build/text_emu"], check=True, capture_output=True)
    return EMU


def render(emu, rows):
    r = subprocess.run([str(emu), "--render", "perRead"], input=rows, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-1000:]
    return r.stdout


def test_selfcheck_reads_equals_snprintf(emu):
    """every (m, u) in 0..700 x 0..700, 10^7 seeded pairs with counts up to 2^31, rows without coverage and negative positions: the line and
    its length against the command's two snprintf calls -- zero mismatches"""
    r = subprocess.run([str(emu), "--selfcheck-reads", "10000000"], capture_output=True, text=True, timeout=1800)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["random_pairs"] >= 10000000 and out["cases"] > 10000000 + 701 * 701
    assert out["zero_coverage"] > 1000 and out["negative_positions"] > 1000
    assert r.returncode == 0 and out["mismatches"] == 0, r.stderr[-3000:]


def test_reads_fill_workgroup_emulation(emu):
    """k_rtext_fill's workgroup on the host: the name span staged at every misalignment of the source, names of every length 0..255, the
    image at every misalignment of the destination, both reasons for the direct path; a workgroup of 256 names of 80 bytes on a 5-byte
    contig name takes the image"""
    r = subprocess.run([str(emu), "--emulate-reads", "4000"], capture_output=True, text=True, timeout=600)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert r.returncode == 0 and out["mismatches"] == 0, r.stderr[-2000:]
    assert out["rounds"] == 4000 and out["image_blocks"] > 4000 and out["direct_text_blocks"] > 100 and out["direct_names_blocks"] > 100
    assert out["eighty_byte_blocks"] > 100 and out["stage_quads"] > 100000 and out["quads"] > 100000 and out["name_lengths"] == 256


def rows_of(text):
    """the TSV rows of a perRead file: the counts come back from a line as m = round(V * cov / 100)"""
    rows = []
    for t in (l.split(b"\t") for l in text.splitlines()):
        cov = int(t[4]); m = round(float(t[3]) * cov / 100.0)
        rows.append(b"%s\t%s\t%d\t%d\t%d\n" % (t[0], t[1], int(t[2]), m, cov - m))
    return rows


@pytest.mark.parametrize("name", ["perread_cg", "perread_chgchh"])
def test_perread_goldens_round_trip(emu, name):
    want = (EXPECTED / f"{name}.out.perRead.txt").read_bytes()
    rows = rows_of(want)
    assert len(rows) == want.count(b"\n") > 0
    for row, line in zip(rows, want.splitlines(keepends=True)):        # the inversion is exact for every line before the file is compared
        t = row.split(b"\t")
        m, u = int(t[3]), int(t[4])
        assert ("%s\t%s\t%d\t%f\t%d\n" % (t[0].decode(), t[1].decode(), int(t[2]), 100.0 * m / (m + u), m + u)).encode() == line
    assert render(emu, b"".join(rows)) == want


def test_row_without_coverage_prints_zero_point_zero(emu):
    got = render(emu, b"r1\tchrA\t5\t3\t4\nr2\tchrA\t7\t0\t0\nr3\tchrB\t-2\t0\t9\n")
    assert got == b"r1\tchrA\t5\t42.857143\t7\nr2\tchrA\t7\t0.0\t0\nr3\tchrB\t-2\t0.000000\t9\n"


@pytest.mark.parametrize("name", ["mbias_cg", "mbias_chgchh"])
def test_bias_render_equals_the_txt_table(name, tmp_path):
    import torch
    import methyldackel_amd as mdk
    want = (EXPECTED / f"{name}.stdout").read_bytes()
    rows = [l.split("\t") for l in want.decode().splitlines()[1:]]
    assert len(rows) > 10
    cols = {"strand": torch.tensor([mdk.STRANDS.index(r[0]) for r in rows], dtype=torch.int8), "read": torch.tensor([int(r[1]) for r in rows], dtype=torch.int8),
            "position": torch.tensor([int(r[2]) for r in rows], dtype=torch.int32), "nmeth": torch.tensor([int(r[3]) for r in rows], dtype=torch.int64),
            "nunmeth": torch.tensor([int(r[4]) for r in rows], dtype=torch.int64), "counts": torch.zeros((1, 4, 2, 2), dtype=torch.int64)}
    b = mdk.Bias(cols, {})
    assert b.render() == want
    assert open(b.write(tmp_path / "t.txt"), "rb").read() == want
    none = mdk.Bias({k: v[:0] for k, v in cols.items()}, {})
    assert none.render() == b"Strand\tRead\tPosition\tnMethylated\tnUnmethylated\n"


def host_reads(names, contigs=("chrA", "chrB")):
    import torch
    import methyldackel_amd as mdk
    n = len(names)
    off = [0]
    for q in names:
        off.append(off[-1] + len(q))
    cols = {"contig": torch.tensor([i % len(contigs) for i in range(n)], dtype=torch.int32), "pos": torch.arange(100, 100 + n, dtype=torch.int32),
            "nmeth": torch.arange(n, dtype=torch.int32), "nunmeth": torch.tensor([i % 3 for i in range(n)], dtype=torch.int32),
            "name_offsets": torch.tensor(off, dtype=torch.int64), "name_bytes": torch.tensor(list("".join(names).encode()), dtype=torch.uint8)}
    return mdk.Reads(list(contigs), cols)


NAMES = ["a", "", "read/2", "x" * 254, "q:7", "", "seventh", "HWI-ST:8:1101"]


@pytest.mark.parametrize("what", ["mask", "reversed", "repeats", "slice", "stepped slice", "backward slice", "empty mask", "empty index"])
def test_reads_select_on_cpu_tensors(what):
    import torch
    r = host_reads(NAMES)
    n = len(NAMES)
    index, want = {
        "mask": (torch.tensor([i % 3 != 1 for i in range(n)]), [i for i in range(n) if i % 3 != 1]),
        "reversed": (torch.arange(n - 1, -1, -1), list(range(n - 1, -1, -1))),
        "repeats": (torch.tensor([3, 3, 0, 7, 3, 1, 1, 6, 0, 0]), [3, 3, 0, 7, 3, 1, 1, 6, 0, 0]),
        "slice": (slice(2, 6), [2, 3, 4, 5]),
        "stepped slice": (slice(None, None, 3), [0, 3, 6]),
        "backward slice": (slice(None, 1, -2), [7, 5, 3]),
        "empty mask": (torch.zeros(n, dtype=torch.bool), []),
        "empty index": (torch.zeros(0, dtype=torch.int64), []),
    }[what]
    s = r.select(index)
    assert len(s) == len(want) and s.names() == [NAMES[i] for i in want]
    assert s.rows() == [r.rows()[i] for i in want]
    off = s.name_offsets.tolist()
    assert len(off) == len(want) + 1 and off[0] == 0 and off[-1] == s.name_bytes.shape[0] == sum(len(NAMES[i]) for i in want)
    assert s.name_offsets.dtype == torch.int64 and s.name_bytes.dtype == torch.uint8 and s.contigs == r.contigs
    assert r.names() == NAMES                                    # the source is untouched
    again = s.select(slice(None))
    assert again.names() == s.names()


def test_refusals_need_no_device(tmp_path):
    import torch
    import methyldackel_amd as mdk
    r = host_reads(NAMES)
    with pytest.raises(mdk.MdkError, match="no CPU path"):
        r.render()
    with pytest.raises(mdk.MdkError, match="no CPU path"):
        r.write(tmp_path / "x.txt")
    assert not (tmp_path / "x.txt").exists()                     # refused before a file is opened
    with pytest.raises(mdk.MdkError, match="not a row"):
        r.select(torch.tensor([0, len(NAMES)]))
    with pytest.raises(mdk.MdkError, match="one entry per row"):
        r.select(torch.ones(3, dtype=torch.bool))
    with pytest.raises(mdk.MdkError, match="mask"):
        r.select(torch.tensor([0.5]))
    short = host_reads(NAMES)
    short.name_offsets = short.name_offsets[:-1]
    with pytest.raises(mdk.MdkError, match=r"len \+ 1"):
        short.select(slice(None))
    with pytest.raises(mdk.MdkError, match=r"len \+ 1"):
        short.render()
    wrong = host_reads(NAMES)
    wrong.name_bytes = wrong.name_bytes.to(torch.int32)
    with pytest.raises(mdk.MdkError, match="uint8"):
        wrong.render()
    assert mdk.TEXT_PERREAD == 5 and "md_text_measure_reads" in mdk.HIP_SYMBOLS and "md_text_gather_names" in mdk.HIP_SYMBOLS
