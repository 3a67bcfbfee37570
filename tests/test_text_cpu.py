"""CPU: the device text formatter's arithmetic and layouts without a GPU.  csrc/mdk_text_core.h is the code k_text_len / k_text_fill
(csrc/mdk_text.hip) run; tools/text_emu.cpp compiles the same functions for the host.  Its self-check compares %f, %6.2f, the integer
percentage and the integer digits with snprintf; its render mode turns rows back into files, which must equal the committed goldens byte for
byte.  The kernels themselves are compared with the command's files on the GPU (tests/test_gpu_text.py).  Also here: what the session's
results know about their command line (mdk_calls_merged / mdk_calls_contexts, on the device stand-in), and the refusals of render / write
that need no device."""
import json
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, REPO

EMU = REPO / "tools" / "_build" / "text_emu"
EXPECTED = GOLDEN / "expected"
STANDIN = REPO / "tools" / "_build" / "libmdk_dev_standin.so"


@pytest.fixture(scope="module")
def emu():
    if not EMU.exists():
        subprocess.run(["make", "-C", str(REPO), "tools/_build/text_emu"], check=True, capture_output=True)
    return EMU


def render(emu, fmt, rows, *opts):
    r = subprocess.run([str(emu), "--render", fmt] + list(opts), input=rows, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-1000:]
    return r.stdout


def bedgraph_rows(name):
    """the rows of a default bedGraph as the tool's TSV: chrom start end nmeth nunmeth (columns 1, 2, 3, 5, 6)"""
    lines = (EXPECTED / name).read_bytes().splitlines()[1:]
    return b"".join(b"\t".join([t[0], t[1], t[2], t[4], t[5]]) + b"\n" for t in (l.split(b"\t") for l in lines))


def test_selfcheck_equals_snprintf(emu):
    """every (m, u) in 0..600 x 0..600, 2 * 10^7 seeded pseudo-random pairs with counts up to 2^31 and the int32 extremes: %f of m / cov,
    %6.2f of 100 m / cov and 100 u / cov, (int)(100.0 m / cov), %u and %i -- zero mismatches with glibc"""
    r = subprocess.run([str(emu), "--selfcheck", "20000000"], capture_output=True, text=True, timeout=1800)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["random_pairs"] >= 20000000 and out["cases"] > 3 * 20000000 + 3 * 600 * 600
    assert r.returncode == 0 and out["mismatches"] == 0, r.stderr[-3000:]


def test_fill_workgroup_emulation(emu):
    """k_text_fill's workgroup on the host: the LDS image at every misalignment of the destination, aligned quads plus head and tail bytes,
    the straight-to-global path of long names -- equal to the concatenated lines, nothing touched outside them"""
    r = subprocess.run([str(emu), "--emulate", "4000"], capture_output=True, text=True, timeout=600)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert r.returncode == 0 and out["mismatches"] == 0 and out["image_blocks"] > 4000 and out["direct_blocks"] > 10 and out["quads"] > 100000, r.stderr[-2000:]


def test_default_bedgraph_round_trips(emu):
    got = render(emu, "bedGraph", bedgraph_rows("extract_cg_q2.out_CpG.bedGraph"), "--prefix", "out", "--context", "CpG")
    assert got == (EXPECTED / "extract_cg_q2.out_CpG.bedGraph").read_bytes() and got.count(b"\n") > 10


def test_fraction_equals_the_fraction_golden(emu):
    """the same command line apart from --fraction (tests/golden/make_expected.py): the q2 rows rendered as fractions are that file"""
    got = render(emu, "fraction", bedgraph_rows("extract_cg_q2.out_CpG.bedGraph"), "--prefix", "out", "--context", "CpG")
    assert got == (EXPECTED / "extract_cg_fraction.out_CpG.meth.bedGraph").read_bytes()


def test_cytosine_report_round_trips(emu):
    want = (EXPECTED / "extract_cg_cytosine_report.out.cytosine_report.txt").read_bytes()
    assert render(emu, "cytosine_report", want) == want and want.count(b"\n") > 50
    assert {l.split(b"\t")[5] for l in want.splitlines()} == {b"CG", b"CHH"}          # (the fixture's reference has no CHG)
    chg = b"chr1\t1000000\t-\t12\t345\tCHG\tCTG\nchr1\t1000003\t+\t0\t0\tCHG\tCNG\n"
    assert render(emu, "cytosine_report", chg) == chg


@pytest.mark.parametrize("ctx", ["CpG", "CHG", "CHH"])
def test_all_contexts_round_trip(emu, ctx):
    """the CHG file is header-only: no rows give the header alone"""
    name = f"extract_cg_all_contexts.out_{ctx}.bedGraph"
    assert render(emu, "bedGraph", bedgraph_rows(name), "--prefix", "out", "--context", ctx) == (EXPECTED / name).read_bytes()


@pytest.mark.parametrize("ctx", ["CpG", "CHG", "CHH"])
def test_methylkit_round_trips(emu, ctx):
    """the fields of the methylKit golden back through the %6.2f layout: base - 1 is the start, coverage and freqC give the counts"""
    want = (EXPECTED / f"extract_cg_methylkit.out_{ctx}.methylKit").read_bytes()
    rows = []
    for t in (l.split(b"\t") for l in want.splitlines()[1:]):
        cov = int(t[4]); m = round(float(t[5]) * cov / 100.0)
        rows.append(b"%s\t%d\t%d\t%d\t%d\t%s\n" % (t[1], int(t[2]) - 1, int(t[2]), m, cov - m, b"+" if t[3] == b"F" else b"-"))
    assert render(emu, "methylKit", b"".join(rows), "--prefix", "out", "--context", ctx) == want


def test_merged_header_and_rows_without_coverage(emu):
    got = render(emu, "counts", b"chrA\t5\t7\t3\t4\nchrA\t9\t11\t0\t0\n", "--prefix", "p/q", "--context", "CHG", "--merged")
    assert got == b'track type="bedGraph" description="p/q CHG merged methylation counts"\nchrA\t5\t7\t7\n'
    r = subprocess.run([str(emu), "--render", "methylKit"], input=b"chrA\t5\t7\t3\t4\t.\n", capture_output=True)
    assert r.returncode != 0 and b"strand" in r.stderr          # a merged row has no methylKit line


def test_render_refusals_need_no_device():
    """--logit is refused with rc -23, an unknown format and CPU tensors with MdkError: there is no CPU path"""
    import torch
    import methyldackel_amd as mdk
    cols = {n: torch.zeros(2, dtype=getattr(torch, dt)) for n, dt in mdk.CALL_COLUMNS}
    c = mdk.Calls(["chrA"], cols)
    assert c.merged is False and c.contexts_on == (0, 1, 2)
    with pytest.raises(mdk.MdkError) as e:
        c.render(fmt="logit", prefix="out")
    assert e.value.rc == mdk.RC_UNSUPPORTED == -23
    with pytest.raises(mdk.MdkError) as e:
        c.write("out", fmt="logit")
    assert e.value.rc == -23
    with pytest.raises(mdk.MdkError):
        c.render(fmt="bigWig", prefix="out")
    with pytest.raises(mdk.MdkError, match="no CPU path"):
        c.render(prefix="out")
    y = mdk.Cytosines(["chrA"], {n: torch.zeros((2, 3) if n == "trinucleotide" else 2, dtype=getattr(torch, dt)) for n, dt in mdk.CYTOSINE_COLUMNS})
    with pytest.raises(mdk.MdkError, match="no CPU path"):
        y.render()
    assert c.header("bedGraph", 1, "a b") == b'track type="bedGraph" description="a b CHG methylation levels"\n'
    assert c.header("methylKit", 0, None) == b"chrBase\tchr\tbase\tstrand\tcoverage\tfreqC\tfreqT\n"


DRIVER = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import methyldackel_amd as mdk
res = []
with mdk.Session(0) as s:
    for args in json.loads(sys.argv[2]):
        c = s.extract(args, device_tensors=False)
        y = s.cytosine_report([a for a in args if not a.startswith("--mergeC")], device_tensors=False)
        res.append([c.merged, list(c.contexts_on), list(y.contexts_on)])
print("RESULT " + json.dumps(res))
"""


def test_results_know_their_command_line(tmp_path):
    """Calls.merged / Calls.contexts_on / Cytosines.contexts_on come from the parsed options (getopt abbreviations included), not from the rows"""
    if not STANDIN.exists():
        subprocess.run(["make", "-C", str(REPO), "tools/_build/libmdk_dev_standin.so"], check=True, capture_output=True)
    base = [str(GOLDEN / "cg100.fa"), str(GOLDEN / "cg_aln.bam"), "-q", "2"]
    jobs = [base, base + ["--CHG", "--CHH"], base + ["--mergeContext", "--CHG"], base + ["--noCpG", "--CHH"], base + ["--mergeC", "--noC", "--CHG"]]
    e = dict(os.environ)
    e.update({"LD_PRELOAD": str(STANDIN), "MDK_STANDIN_DUMP": str(tmp_path / "none.tsv")})
    r = subprocess.run([sys.executable, "-c", DRIVER, str(REPO), json.dumps(jobs)], cwd=tmp_path, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert res == [[False, [0], [0]], [False, [0, 1, 2], [0, 1, 2]], [True, [0, 1], [0, 1]], [False, [2], [2]], [True, [1], [1]]]
