"""CPU: the resident session's perRead (mdk_session_perread, methyldackel_amd.Session.perread) without a GPU.  tools/dev_standin.c is preloaded
in front of libmdk_hip.so, as in test_calls_cpu.py: a chunk's reads are selected from its records as the device selects them, each kept read's
name and position are checked against the oracle's next `perRead` line and its counts are taken from that line (MDK_STANDIN_PERREAD), and the
stand-in's md_dev_reads_* keep the rows.  What runs here is the product's own host code: option parsing, the chunk loop with two chunks in
flight, the session's sink (device-selected chunks, chunks of a contig the FASTA lacks), the reset between runs and the Python API down to CPU
tensors.  Rows rendered as the command renders them must equal the oracle's output byte for byte."""
import json
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, REPO, run_oracle
from test_perread import BAD, FIX, SYN, oracle_perread

STANDIN = REPO / "tools" / "_build" / "libmdk_dev_standin.so"

# runs the session in a fresh process (the stand-in must be preloaded before libmdk_hip.so is loaded): per job its rc, or its rows as text
DRIVER = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import methyldackel_amd as mdk
jobs = json.loads(sys.argv[2]); res = []

def render(r):
    out = []
    for name, chrom, pos, m, u in r.rows():
        out.append("%s\t%s\t%d\t%f\t%u\n" % (name, chrom, pos, 100.0 * m / (m + u), m + u) if m + u else "%s\t%s\t%d\t0.0\t%u\n" % (name, chrom, pos, m + u))
    return "".join(out)

with mdk.Session(0) as s:
    for cmd, args in jobs:
        try:
            if cmd == "perRead":
                r = s.perread(args, device_tensors=False)
            else:
                c = s.extract(args, device_tensors=False)
        except mdk.MdkError as e:
            res.append({"rc": e.rc}); continue
        if cmd == "perRead":
            assert r.pos.device.type == "cpu" and str(r.pos.dtype) == "torch.int32" and str(r.name_offsets.dtype) == "torch.int64" and str(r.name_bytes.dtype) == "torch.uint8"
            assert r.name_offsets.shape[0] == len(r) + 1 and int(r.name_offsets[0]) == 0 and int(r.name_offsets[-1]) == r.name_bytes.shape[0]
            res.append({"rc": 0, "text": render(r), "n": len(r)})
        else:
            res.append({"rc": 0, "rows": [[list(x) for x in c.rows(k)] for k in range(3)]})
print("RESULT " + json.dumps(res))
"""


def run_session(jobs, cwd, perread=None, dump=None, preload=True):
    if not STANDIN.exists():
        subprocess.run(["make", "-C", str(REPO), "tools/_build/libmdk_dev_standin.so"], check=True, capture_output=True)
    e = dict(os.environ)
    if preload:
        e.update({"LD_PRELOAD": str(STANDIN), "MDK_STANDIN_DUMP": str(dump or cwd / "no_dump.tsv"), "MDK_STANDIN_PERREAD": str(perread or cwd / "no_perread.txt")})
    r = subprocess.run([sys.executable, "-c", DRIVER, str(REPO), json.dumps([[c, [str(a) for a in j]] for c, j in jobs])], cwd=cwd, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:]), r.stderr


def oracle_text(args, tmp, name="o"):
    """the oracle's perRead output for args, and the file it was saved to (the stand-in's counts)"""
    o = oracle_perread(list(args), cwd=tmp)
    assert o.returncode == 0, o.stderr[-500:]
    f = tmp / f"{name}_perread.txt"
    f.write_text(o.stdout)
    return o.stdout, f


def parity(tmp_path, args, **kw):
    want, f = oracle_text(args, tmp_path)
    res, _ = run_session([("perRead", args)], tmp_path, perread=f, **kw)
    assert res[0]["rc"] == 0, res
    assert res[0]["text"] == want
    assert res[0]["n"] == want.count("\n")
    return want


@pytest.mark.parametrize("args,rc", BAD, ids=[" ".join(str(a).replace(str(GOLDEN) + "/", "") for a in b[0]) or "no arguments" for b in BAD])
def test_option_errors_give_the_commands_codes(tmp_path, args, rc):
    """the codes perRead_main returns, before any device is asked for (no stand-in: on a box without a GPU the device could not be opened);
    -o is ignored by a session, so the command line that only fails to open it gives the reads"""
    res, err = run_session([("perRead", args)], tmp_path, preload=False)
    if "-o" in [str(a) for a in args]:
        assert res[0]["rc"] in (0, -20), res           # (-20: no device on this box -- the -o was not what stopped it)
        assert "Couldn't open" not in err and not (tmp_path / "x").exists()
        return
    want = rc if rc < 128 else rc - 256
    assert res[0]["rc"] == want, (res, err[-500:])
    if want == 0:
        assert res[0]["n"] == 0 and res[0]["text"] == ""


def test_help_and_version_give_empty_reads(tmp_path):
    res, err = run_session([("perRead", ["-h"]), ("perRead", ["--version"])], tmp_path, preload=False)
    assert [r["rc"] for r in res] == [0, 0] and [r["n"] for r in res] == [0, 0]


def test_output_option_is_ignored(tmp_path):
    args = [GOLDEN / "cg100.fa", GOLDEN / "cg_aln.bam", "-q", "2"]
    want, f = oracle_text(args, tmp_path)
    res, err = run_session([("perRead", args + ["-o", "/nonexistent/dir/x"]), ("perRead", args + ["-o", tmp_path / "y.txt"])], tmp_path, perread=f)
    assert [r["rc"] for r in res] == [0, 0] and res[0]["text"] == want == res[1]["text"]
    assert not (tmp_path / "y.txt").exists()


@pytest.mark.parametrize("args", FIX, ids=[" ".join(a[1:]).replace(str(GOLDEN) + "/", "") for a in FIX])
def test_fixtures_equal_oracle(tmp_path, args):
    assert parity(tmp_path, args)


@pytest.mark.parametrize("which,extra", SYN, ids=[f"{w}:{' '.join(e)}" for w, e in SYN])
def test_synthetic_equal_oracle(tmp_path, small_synth, which, extra):
    text = parity(tmp_path, [small_synth / f"{which}.fa", small_synth / f"{which}.bam"] + extra)
    assert text.count("\n") > 100


def test_bed_with_small_chunks_equals_oracle(tmp_path, small_synth):
    """-l only passes over whole chunks; 2000-base chunks"""
    bed = tmp_path / "b.bed"
    bed.write_text("chrS1\t5000\t5100\nchrS2\t100\t200\n")
    text = parity(tmp_path, [small_synth / "pe.fa", small_synth / "pe.bam", "-l", bed, "--chunkSize", "2000"])
    assert 20 < text.count("\n") < 2000


def test_contig_missing_from_fasta_equals_oracle(tmp_path, small_synth):
    """the reads of a contig the FASTA lacks come out with no calls, listed by the host"""
    fa = tmp_path / "one.fa"
    txt = (small_synth / "pe.fa").read_text()
    fa.write_text(txt[: txt.index(">", 1)])
    text = parity(tmp_path, [fa, small_synth / "pe.bam", "--chunkSize", "7000"])
    assert any(l.split("\t")[1] == "chrS2" and l.endswith("\t0.0\t0") for l in text.splitlines())


def test_alternating_with_extract_equals_fresh_sessions(tmp_path, small_synth):
    """extract, perRead, extract, perRead on one session (the handle is reset between commands) give what fresh sessions give"""
    xa = [small_synth / "pe.fa", small_synth / "pe.bam", "--chunkSize", "6000"]
    pa = [small_synth / "pe.fa", small_synth / "pe.bam", "--chunkSize", "5000", "-p", "20"]
    od = tmp_path / "o"; od.mkdir()
    dump = tmp_path / "dump.tsv"
    assert run_oracle(xa + ["-o", "out"], cwd=od, dump=dump).returncode == 0
    want, f = oracle_text(pa, tmp_path)
    jobs = [("extract", xa), ("perRead", pa), ("extract", xa), ("perRead", pa)]
    res, _ = run_session(jobs, tmp_path, perread=f, dump=dump)
    fresh = [run_session([j], tmp_path, perread=f, dump=dump)[0][0] for j in jobs[:2]]
    assert [r["rc"] for r in res] == [0, 0, 0, 0]
    assert res[0] == res[2] == fresh[0] and sum(len(x) for x in res[0]["rows"]) > 100
    assert res[1] == res[3] == fresh[1] and res[1]["text"] == want
