"""CPU: Session.cytosine_report (mdk_session_cytosines) without a GPU.  tools/dev_standin.c is preloaded in front of libmdk_hip.so, as in
test_calls_cpu.py: a slot's sites come from the oracle's per-column dump, the contigs' bases are the ones the host uploaded, and the
stand-in's md_dev_cytosines_* restate the rules of csrc/mdk_cytosines.hip over them.  What runs here is the product's own host code: the
session's option hook, extract_main's pipeline with the cytosine sink (groups in flight, chunks handed back to the host preparation, chunks
without reads), the reset between runs and the Python API down to CPU tensors.  Every row -- all seven fields, in order -- must equal the
line of the oracle's <prefix>.cytosine_report.txt."""
import json
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, REPO, run_oracle, synth

STANDIN = REPO / "tools" / "_build" / "libmdk_dev_standin.so"

# runs the session in a fresh process (the stand-in must be preloaded before libmdk_hip.so is loaded): every job's rows, or its rc.
# A job is [kind, args]: kind "cyto" -> Session.cytosine_report, "extract" -> Session.extract (only its return code is kept)
DRIVER = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import methyldackel_amd as mdk
jobs = json.loads(sys.argv[2]); res = []
with mdk.Session(0) as s:
    for kind, args in jobs:
        try:
            c = s.cytosine_report(args, device_tensors=False) if kind == "cyto" else s.extract(args, device_tensors=False)
        except mdk.MdkError as e:
            res.append({"rc": e.rc}); continue
        if kind != "cyto":
            res.append({"rc": 0, "n": len(c)}); continue
        assert c.pos.device.type == "cpu" and [str(getattr(c, n).dtype) for n, _ in c.COLUMNS] == ["torch.int32", "torch.int32", "torch.int8", "torch.int32", "torch.int32", "torch.uint8", "torch.uint8"]
        assert tuple(c.trinucleotide.shape) == (len(c), 3) and ((c.strand == 1) | (c.strand == -1)).all() and (c.context <= 2).all() and (c.pos >= 1).all()
        res.append({"rc": 0, "rows": [list(r) for r in c.rows()], "contigs": c.contigs})
print("RESULT " + json.dumps(res))
"""


def run_session(jobs, dump, cwd, **env):
    if not STANDIN.exists():
        subprocess.run(["make", "-C", str(REPO), "tools/_build/libmdk_dev_standin.so"], check=True, capture_output=True)
    e = dict(os.environ)
    e.update({"LD_PRELOAD": str(STANDIN), "MDK_STANDIN_DUMP": str(dump)})
    e.update({k: str(v) for k, v in env.items()})
    jobs = [[k, [str(a) for a in j]] for k, j in jobs]
    r = subprocess.run([sys.executable, "-c", DRIVER, str(REPO), json.dumps(jobs)], cwd=cwd, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:]), r.stderr


def report_rows(path):
    """the seven fields of every line of a cytosine report"""
    rows = []
    for l in path.read_text().splitlines():
        t = l.split("\t")
        assert len(t) == 7, l
        rows.append([t[0], int(t[1]), t[2], int(t[3]), int(t[4]), t[5], t[6]])
    return rows


def oracle_report(args, tmp, name="o"):
    """the oracle's report for `args` + --cytosine_report, and the dump its counters went to"""
    od = tmp / name; od.mkdir()
    dump = tmp / (name + "_dump.tsv")
    r = run_oracle(list(args) + ["--cytosine_report", "-o", "out"], cwd=od, dump=dump)
    assert r.returncode == 0, r.stderr[-500:]
    return report_rows(od / "out.cytosine_report.txt"), dump


def same(got, want):
    assert got["rc"] == 0, got
    assert len(got["rows"]) == len(want), (len(got["rows"]), len(want))
    assert got["rows"] == want, next((i, a, b) for i, (a, b) in enumerate(zip(got["rows"], want)) if a != b)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("cyto_cpu")
    synth(d / "s", "-L", "60000,25000", "-c", "18", "-s", "43", "--extras")
    return d


@pytest.mark.parametrize("extra,env", [([], {}), (["--chunkSize", "3"], {}), (["--chunkSize", "2500", "--CHG", "--CHH"], {}),
                                       (["--chunkSize", "2500"], {"MDK_STANDIN_HANDBACK": 2}), (["--chunkSize", "4000", "--CHG"], {"MDK_GROUPS_IN_FLIGHT": 2}),
                                       (["--chunkSize", "5000"], {"MDK_HOST_PREP": 1})])
def test_rows_equal_oracle(data, tmp_path, extra, env):
    """the default schedule; 3-base chunks over a short region (most of them without a site); 2500-base chunks with every context; every
    second chunk handed back to the host preparation; two groups in flight; chunks prepared on the host"""
    if extra[:2] == ["--chunkSize", "3"]:
        args = [data / "s.fa", data / "s.bam", "-r", "chrS1:1000-1600"] + extra
    else:
        args = [data / "s.fa", data / "s.bam", "-@", "3"] + extra
    want, dump = oracle_report(args, tmp_path)
    assert any(r[3] + r[4] > 0 for r in want) and ("-r" in [str(a) for a in args] or any(r[3] + r[4] == 0 for r in want))      # (the short region is covered throughout)
    res, err = run_session([("cyto", args)], dump, tmp_path, **env)
    same(res[0], want)
    assert not list(tmp_path.glob("*.cytosine_report.txt")) and not list(tmp_path.glob("*.bedGraph")) and not list(tmp_path.glob("s_*")) and not list(tmp_path.glob("s.*"))      # nothing was written next to the caller


def test_flag_given_and_depth_do_not_change_the_rows(data, tmp_path):
    """--cytosine_report may be given; -o is ignored; -d does not apply to this format"""
    args = [data / "s.fa", data / "s.bam", "--chunkSize", "9000", "--CHG"]
    want, dump = oracle_report(args, tmp_path)
    res, _ = run_session([("cyto", args), ("cyto", args + ["--cytosine_report", "-o", "x"]), ("cyto", args + ["-d", "5"])], dump, tmp_path)
    for r in res:
        same(r, want)
    assert not list(tmp_path.glob("x*"))


def test_variant_fixture_equals_oracle(tmp_path):
    """cg_with_variants.bam with the variant filter: a dropped site comes back as a 0 0 row"""
    for k, extra in enumerate(([], ["--chunkSize", "30"])):
        args = [GOLDEN / "cg100.fa", GOLDEN / "cg_with_variants.bam", "-p", "1", "-q", "0", "--minOppositeDepth", "3", "--maxVariantFrac", "0.25"] + extra
        want, dump = oracle_report(args, tmp_path, f"o{k}")
        plain, _ = oracle_report(args[:6], tmp_path, f"p{k}")
        assert want != plain and [r[:3] for r in want] == [r[:3] for r in plain]       # the filter changes counts, never the row set
        res, _ = run_session([("cyto", args)], dump, tmp_path)
        same(res[0], want)


def test_golden_report(tmp_path):
    """the committed expected output of the command: 99 rows, 50 of them 0 0"""
    args = [GOLDEN / "cg100.fa", GOLDEN / "cg_aln.bam", "-q", "2", "--CHG", "--CHH"]
    want, dump = oracle_report(args, tmp_path)
    assert want == report_rows(GOLDEN / "expected" / "extract_cg_cytosine_report.out.cytosine_report.txt")
    assert len(want) == 99 and sum(1 for r in want if r[3] + r[4] == 0) == 50
    res, _ = run_session([("cyto", args)], dump, tmp_path)
    same(res[0], want)


def test_refusals(data, tmp_path):
    """the formats that are arithmetic on columns: rc -23, no file; --mergeContext and other bad command lines: what the command returns;
    Session.extract keeps refusing --cytosine_report; the session works afterwards"""
    import methyldackel_amd as mdk
    base = [data / "s.fa", data / "s.bam"]
    want, dump = oracle_report(base, tmp_path)
    jobs = [("cyto", base + [o, "-o", "x"]) for o in ("--fraction", "--counts", "--logit", "--methylKit")]
    bad = (["--mergeContext"], ["--mergeContext", "--cytosine_report"], ["-d", "0"], ["--noCpG"], ["-r", "nochrom:1-5"], ["--fraction", "--cytosine_report"])
    jobs += [("cyto", base + b) for b in bad] + [("extract", base + ["--cytosine_report"]), ("cyto", base)]
    res, err = run_session(jobs, dump, tmp_path)
    assert [r["rc"] for r in res[:4]] == [-23] * 4, res[:4]
    for b, r in zip(bad, res[4:4 + len(bad)]):
        cli = mdk.run_cli(base + [x for x in b if x != "--cytosine_report"] + ["--cytosine_report", "-o", "y"], cwd=tmp_path)
        assert r["rc"] == (cli.returncode - 256 if cli.returncode > 127 else cli.returncode) and r["rc"] != 0, (b, r, cli.returncode)
    assert res[-2]["rc"] == -23 and "--cytosine_report only shape text output" in err
    same(res[-1], want)
    assert not list(tmp_path.glob("x*")) and not list(tmp_path.glob("s_*"))


def test_reuse_does_not_carry_state(data, tmp_path):
    """one session, reports with different options one after the other with an extract run in between: contexts, the region and the
    chunk size of one run do not reach the next"""
    base = [data / "s.fa", data / "s.bam", "--chunkSize", "6000"]
    jobs = [base + ["--CHG", "--CHH"], base, base + ["--noCpG", "--CHG"], base + ["-r", "chrS2:2000-9000"], base]
    wants = [oracle_report(j, tmp_path, f"o{i}")[0] for i, j in enumerate(jobs)]
    # one dump holds every column any of the runs counts (the stand-in looks a slot's interval up in it): the widest run's
    _, dump = oracle_report(base + ["--CHG", "--CHH"], tmp_path, "all")
    mixed = [("cyto", j) for j in jobs]
    mixed.insert(2, ("extract", base))
    res, _ = run_session(mixed, dump, tmp_path)
    assert res[2]["rc"] == 0 and res[2]["n"] > 0
    got = res[:2] + res[3:]
    for r, w in zip(got, wants):
        same(r, w)
    assert got[1] == got[4] and len(wants[0]) > len(wants[1]) > len(wants[3])
