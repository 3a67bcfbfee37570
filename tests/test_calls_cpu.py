"""CPU: the resident extract session (mdk_session_*, methyldackel_amd.Session) without a GPU.  tools/dev_standin.c is preloaded in front of
libmdk_hip.so, as in test_ranks_cpu.py: a slot's sites come from the oracle's per-column dump, and the stand-in's md_dev_calls_* restate
k_calls_compact's rules over them.  What runs here is the product's own host code: the session, extract_main's pipeline with the calls sink
(groups in flight, chunks handed back to the host preparation), the reset between runs and the Python API down to CPU tensors.  Every row
must equal the oracle's bedGraph line (columns 1, 2, 3, 5, 6 of each context file)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, REPO, run_oracle, synth

STANDIN = REPO / "tools" / "_build" / "libmdk_dev_standin.so"
CTX = ("CpG", "CHG", "CHH")

# runs the session in a fresh process (the stand-in must be preloaded before libmdk_hip.so is loaded): every job's rows per context, or its rc
DRIVER = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import methyldackel_amd as mdk
jobs = json.loads(sys.argv[2]); res = []
with mdk.Session(0) as s:
    for args in jobs:
        try:
            c = s.extract(args, device_tensors=False)
        except mdk.MdkError as e:
            res.append({"rc": e.rc}); continue
        assert c.start.device.type == "cpu" and str(c.start.dtype) == "torch.int32" and str(c.context.dtype) == "torch.uint8" and str(c.strand.dtype) == "torch.int8"
        assert (c.end > c.start).all() and ((c.strand == 0) | (c.strand == 1) | (c.strand == -1)).all()
        res.append({"rc": 0, "rows": [[list(r) for r in c.rows(k)] for k in range(3)], "strand": c.strand.tolist(), "width": (c.end - c.start).tolist()})
print("RESULT " + json.dumps(res))
"""


def run_session(jobs, dump, cwd, **env):
    if not STANDIN.exists():
        subprocess.run(["make", "-C", str(REPO), "tools/_build/libmdk_dev_standin.so"], check=True, capture_output=True)
    e = dict(os.environ)
    e.update({"LD_PRELOAD": str(STANDIN), "MDK_STANDIN_DUMP": str(dump)})
    e.update({k: str(v) for k, v in env.items()})
    r = subprocess.run([sys.executable, "-c", DRIVER, str(REPO), json.dumps([[str(a) for a in j] for j in jobs])], cwd=cwd, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:]), r.stderr


def oracle_rows(args, tmp, name="o"):
    """the oracle's bedGraph rows per context (None where the context was not written) and the dump its counters went to"""
    od = tmp / name; od.mkdir()
    dump = tmp / (name + "_dump.tsv")
    r = run_oracle(list(args) + ["-o", "out"], cwd=od, dump=dump)
    assert r.returncode == 0, r.stderr[-500:]
    rows = []
    for k in CTX:
        f = od / f"out_{k}.bedGraph"
        if not f.exists():
            rows.append(None); continue
        rows.append([[t[0], int(t[1]), int(t[2]), int(t[4]), int(t[5])] for t in (l.split("\t") for l in f.read_text().splitlines()[1:])])
    return rows, dump


def same_rows(got, want):
    seen = 0
    for k in range(3):
        if want[k] is None:
            assert got["rows"][k] == [], CTX[k]
            continue
        seen += len(want[k])
        assert got["rows"][k] == want[k], (CTX[k], len(got["rows"][k]), len(want[k]))
    assert seen > 0


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("calls_cpu")
    synth(d / "s", "-L", "60000,25000", "-c", "18", "-s", "43", "--extras")
    return d


@pytest.mark.parametrize("extra,env", [([], {}), (["--chunkSize", "3"], {}), (["--chunkSize", "2500", "--CHG", "--CHH"], {}),
                                       (["--chunkSize", "2500"], {"MDK_STANDIN_HANDBACK": 2}), (["--chunkSize", "4000", "--CHG"], {"MDK_GROUPS_IN_FLIGHT": 2}),
                                       (["--chunkSize", "3000", "--mergeContext", "--CHG", "--CHH", "-d", "3"], {}), (["--chunkSize", "5000"], {"MDK_HOST_PREP": 1})])
def test_session_rows_equal_oracle(data, tmp_path, extra, env):
    """chunk sizes 3 (chunks of a few positions, most of them empty), 2500 and the default; every second chunk handed back to the host
    preparation; two groups in flight; merged contexts with a depth threshold; chunks prepared on the host"""
    if extra[:2] == ["--chunkSize", "3"]:
        args = [data / "s.fa", data / "s.bam", "-r", "chrS1:1000-1600"] + extra     # (3-base chunks over a short region: the schedule walks every one)
    else:
        args = [data / "s.fa", data / "s.bam", "-@", "3"] + extra
    want, dump = oracle_rows(args, tmp_path)
    res, err = run_session([args], dump, tmp_path, **env)
    same_rows(res[0], want)
    assert not list(tmp_path.glob("*.bedGraph")) and not list(tmp_path.glob("s_*"))      # nothing was written next to the caller
    if "--mergeContext" in extra:
        assert set(res[0]["strand"]) <= {0, -1, 1} and any(w in (2, 3) for w in res[0]["width"])
        assert all(s == 0 for s, w in zip(res[0]["strand"], res[0]["width"]) if w > 1)


def test_session_merge_with_variants_equals_oracle(tmp_path):
    """--mergeContext with the variant filter on cg_with_variants.bam: a G dropped as a variant zeroes the counts of its C (mdk_emit.c:86-88)"""
    for extra in ([], ["--chunkSize", "30"]):
        args = [GOLDEN / "cg100.fa", GOLDEN / "cg_with_variants.bam", "--mergeContext", "-p", "1", "-q", "0", "--minOppositeDepth", "3", "--maxVariantFrac", "0.25"] + extra
        want, dump = oracle_rows(args, tmp_path, "o" + str(len(extra)))
        res, _ = run_session([args], dump, tmp_path)
        same_rows(res[0], want)


def test_session_refuses_text_options(data, tmp_path):
    """options that only shape text: the same return code for each, no file written; a run after a refused one still works"""
    base = [data / "s.fa", data / "s.bam"]
    want, dump = oracle_rows(base, tmp_path)
    jobs = [base + [o, "-o", "x"] for o in ("--fraction", "--counts", "--logit", "--methylKit", "--cytosine_report")] + [base + ["-o", "x"]]
    res, err = run_session(jobs, dump, tmp_path)
    assert [r["rc"] for r in res[:5]] == [-23] * 5, res
    assert err.count("only shape text output") == 5
    same_rows(res[5], want)
    assert not list(tmp_path.glob("x*")) and not list(tmp_path.glob("s_*"))


def test_session_errors_match_the_command(data, tmp_path):
    """a bad command line gives the return code extract_main gives"""
    import methyldackel_amd as mdk
    for bad in (["-d", "0"], ["--noCpG"], ["--mergeContext", "--methylKit"], ["-r", "nochrom:1-5"]):
        args = [data / "s.fa", data / "s.bam"] + bad
        cli = mdk.run_cli(args + ["-o", "y"], cwd=tmp_path)
        res, _ = run_session([args], tmp_path / "none.tsv", tmp_path)
        assert res[0]["rc"] == cli.returncode - 256 if cli.returncode > 127 else res[0]["rc"] == cli.returncode, (bad, res, cli.returncode)


def test_session_reuse_does_not_carry_state(data, tmp_path):
    """one session, runs with different options one after the other: contexts, merging and the depth threshold of one run do not reach the
    next (the device-side state -- -l runs, mappability -- is the GPU suite's: the stand-in counts every column)"""
    base = [data / "s.fa", data / "s.bam", "--chunkSize", "6000"]
    jobs = [base + ["--CHG", "--CHH", "--mergeContext"], base, base + ["--noCpG", "--CHG"], base + ["-d", "4"], base]
    wants = [oracle_rows(j, tmp_path, f"o{i}")[0] for i, j in enumerate(jobs)]
    # one dump holds every column any of the runs counts (the stand-in looks a slot's interval up in it): the widest run's
    _, dump = oracle_rows(base + ["--CHG", "--CHH"], tmp_path, "all")
    res, _ = run_session(jobs, dump, tmp_path)
    for r, w in zip(res, wants):
        same_rows(r, w)
    assert res[1] == res[4]
