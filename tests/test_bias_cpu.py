"""CPU: the session's mbias (mdk_session_mbias, methyldackel_amd.Session.mbias -> Bias) and the exported bounds (mdk_mbias_suggest) without
a GPU.  tools/dev_standin.c is preloaded in front of libmdk_hip.so as in test_calls_cpu.py.  The stand-in CANNOT COUNT: the oracle has no
per-chunk histogram dump, so the histogram of a run is GIVEN to it -- the oracle's --noSVG table of the same command line
($MDK_STANDIN_MBIAS/<run>.txt), added when the run's first chunk is submitted.  What runs here is therefore the product's host code and
nothing else: parsing and return codes, the group pipeline with the histogram sink ending cleanly (groups in flight, chunks handed back to
the host preparation, chunks prepared on the host), the reset between runs, the bounds, the order of the rows, the Python class, and that no
file is written.  The counting itself -- k_mbias_multi, k_bias_rows -- is the GPU suite's (tests/test_gpu_bias.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import methyldackel_amd as mdk
from conftest import GOLDEN, ORACLE, REPO
from test_mbias import FIX, REPORTS, SYN, STRANDS, _report, _table, oracle_mbias, parse_txt

STANDIN = REPO / "tools" / "_build" / "libmdk_dev_standin.so"
NAMES = ("OT", "OB", "CTOT", "CTOB")


def suggestion(stderr):
    """{"OT": (a, b, c, d), ...} from the "Suggested inclusion options:" line of a report's stderr ({} when there is none)"""
    out = {}
    for line in stderr.splitlines():
        if line.startswith("Suggested inclusion options:"):
            t = line.split()[3:]
            for k, v in zip(t[0::2], t[1::2]):
                out[k[2:]] = tuple(int(x) for x in v.split(","))
    return out


def hist_of(rows):
    """the oracle's table {(strand 1..4, read, q): [m, u]} as rows [q][16]"""
    n = max((q for (_, _, q) in rows), default=-1) + 1
    a = np.zeros((n, 4, 2, 2), dtype=np.uint32)
    for (s, r, q), (m, u) in rows.items():
        a[q, s - 1, r - 1] = (m, u)
    return a


def oracle_table(args, cwd, name="o"):
    """the oracle's run WITH a prefix and --txt: (table lines in print order as tuples, parsed table, suggestion).  The SVGs go to cwd/name"""
    d = cwd / name; d.mkdir()
    o = oracle_mbias(list(args) + ["out", "--txt"], cwd=d)
    assert o.returncode == 0, o.stderr[-500:]
    lines = [tuple(l.split("\t")) for l in o.stdout.splitlines()[1:]]
    return [(s, int(r), int(q), int(m), int(u)) for s, r, q, m, u in lines], parse_txt(o.stdout), suggestion(o.stderr), o.stdout


def all_lines(small_synth):
    return [list(a) for a in FIX] + [[small_synth / f"{w}.fa", small_synth / f"{w}.bam"] + e for w, e in SYN] + \
           [[small_synth / f"{w}.fa", small_synth / f"{w}.bam"] + e for w, e, _ in REPORTS] + [[small_synth / "bis.fa", small_synth / "bis.bam", "--CHG", "--CHH"]]


def test_suggest_equals_the_oracles_line(tmp_path, small_synth):
    """mdk_mbias_suggest over the oracle's own histogram gives the strands and numbers of the oracle's "Suggested inclusion options:" line,
    for every command line of test_mbias.FIX, SYN and REPORTS, and for the Bismark-style sample with all contexts, whose bounds are not zero"""
    nonzero = 0
    for i, args in enumerate(all_lines(small_synth)):
        _, table, want, _ = oracle_table(args, tmp_path, f"o{i}")
        got = mdk.mbias_suggest(hist_of(table))
        assert got == want and list(got) == [k for k in NAMES if k in want], (args, got, want)
        nonzero += any(any(v) for v in got.values())
    _, table, want, _ = oracle_table([small_synth / "bis.fa", small_synth / "bis.bam", "--CHG", "--CHH"], tmp_path, "bis")
    assert want == {"OT": (0, 0, 0, 0), "OB": (0, 0, 41, 142), "CTOT": (50, 0, 0, 0), "CTOB": (46, 0, 0, 0)} and len(table) == 1200
    assert mdk.mbias_suggest(hist_of(table)) == want
    assert nonzero >= 1


def test_suggest_on_skewed_profiles(tmp_path):
    """the hand-made histograms of test_mbias.test_report_on_skewed_profiles: the exported bounds are the ones mdk_mbias_report prints"""
    rng = np.random.default_rng(5)
    for case, L in enumerate((32, 64, 100, 128, 151)):
        rows = {}
        for q in range(L):
            n = int(rng.integers(200, 400))
            f1 = 0.75 - (0.5 if q < 6 else 0) + (0.2 if q > L - 5 else 0)
            f2 = 0.75 + (0.2 if q < 3 else 0) - (0.6 if q > L - 9 else 0)
            rows[(1, 1, q)] = [int(n * f1), n - int(n * f1)]
            rows[(1, 2, q)] = [int(n * f2), n - int(n * f2)]
            if q % 3:
                rows[(2, 2, q)] = [int(n * 0.1), n - int(n * 0.1)]
            if q > 10:
                rows[(4, 1, q)] = [n, 0]
        d = tmp_path / f"c{case}"; d.mkdir()
        g = _report(rows, "out", 1, 0, 7, d)
        assert g.returncode == 0, g.stderr
        want = suggestion(g.stderr)
        assert set(want) == {"OT", "OB", "CTOB"} and any(want["OT"])
        assert mdk.mbias_suggest(hist_of(rows)) == want
        o = subprocess.run([str(ORACLE), "mbias-report", "out", "7"], cwd=d, input=_table(rows), capture_output=True, text=True)
        assert o.returncode == 0 and suggestion(o.stderr) == want


# runs the session in a fresh process (the stand-in must be preloaded before libmdk_hip.so is loaded): per job {"cmd": "mbias" | "extract" | "perread", "args": [...]}
DRIVER = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import methyldackel_amd as mdk
jobs = json.loads(sys.argv[2]); res = []
with mdk.Session(0) as s:
    for job in jobs:
        try:
            r = getattr(s, job["cmd"])(job["args"], device_tensors=False)
        except mdk.MdkError as e:
            res.append({"rc": e.rc}); continue
        if job["cmd"] != "mbias":
            res.append({"rc": 0, "rows": [list(x) for x in r.rows()]}); continue
        assert isinstance(r, mdk.Bias) and not hasattr(r, "contigs")
        dt = {n: str(getattr(r, n).dtype) for n, _ in mdk.BIAS_COLUMNS}
        assert dt == {n: "torch." + t for n, t in mdk.BIAS_COLUMNS}, dt
        assert all(getattr(r, n).device.type == "cpu" for n, _ in mdk.BIAS_COLUMNS)
        assert r.counts.dim() == 4 and tuple(r.counts.shape[1:]) == (4, 2, 2) and len(r) == r.strand.shape[0]
        res.append({"rc": 0, "rows": [list(x) for x in r.rows()], "counts": r.counts.tolist(), "suggested": {k: list(v) for k, v in r.suggested.items()},
                    "order": list(r.suggested), "options": r.options(), "resubmitted": r.resubmitted})
print("RESULT " + json.dumps(res))
"""


def run_session(jobs, tables, cwd, **env):
    """jobs in one fresh process over the stand-in; tables[i] = the oracle's --noSVG table text of the i-th mbias run that reaches the device"""
    if not STANDIN.exists():
        subprocess.run(["make", "-C", str(REPO), "tools/_build/libmdk_dev_standin.so"], check=True, capture_output=True)
    given = cwd / f"given{len(list(cwd.glob('given*')))}"; given.mkdir()
    for i, t in enumerate(tables):
        (given / f"{i}.txt").write_text(t)
    e = dict(os.environ)
    e.update({"LD_PRELOAD": str(STANDIN), "MDK_STANDIN_DUMP": str(cwd / "none.tsv"), "MDK_STANDIN_MBIAS": str(given)})
    e.update({k: str(v) for k, v in env.items()})
    jobs = [{"cmd": j[0], "args": [str(a) for a in j[1]]} for j in jobs]
    r = subprocess.run([sys.executable, "-c", DRIVER, str(REPO), json.dumps(jobs)], cwd=cwd, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    head = r.stdout[: r.stdout.index("RESULT ")]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:]), head, r.stderr


def same_as_oracle(got, lines, table, want):
    assert got["rc"] == 0
    assert [tuple(x) for x in got["rows"]] == lines                        # line by line, in the command's order
    dense = hist_of(table).astype(np.int64)
    assert np.array_equal(np.asarray(got["counts"], dtype=np.int64).reshape(dense.shape), dense)
    assert {k: tuple(v) for k, v in got["suggested"].items()} == want and got["order"] == [k for k in NAMES if k in want]
    assert got["options"] == [t for k in NAMES if k in want for t in ("--" + k, ",".join(str(x) for x in want[k]))]


@pytest.mark.parametrize("extra,env", [(["--CHG", "--CHH"], {}), (["--CHG", "--CHH", "--chunkSize", "2500"], {"MDK_STANDIN_HANDBACK": 2}),
                                       (["--chunkSize", "4000", "--CHH"], {"MDK_GROUPS_IN_FLIGHT": 2}), (["--chunkSize", "5000"], {"MDK_HOST_PREP": 1})])
def test_session_over_the_standin(tmp_path, small_synth, extra, env):
    """the default chunks; every second chunk handed back to the host preparation; two groups in flight; chunks prepared on the host.  A
    prefix is given and --txt asked for: no file appears next to the caller and nothing is printed"""
    args = [small_synth / "bis.fa", small_synth / "bis.bam"] + extra
    lines, table, want, text = oracle_table(args, tmp_path)
    before = sorted(p.name for p in tmp_path.iterdir())
    res, out, err = run_session([("mbias", args + ["prefix_ignored", "--txt"])], [text], tmp_path, **env)
    same_as_oracle(res[0], lines, table, want)
    assert len(lines) > 100
    assert out == "" and "Suggested inclusion" not in err
    assert sorted(p.name for p in tmp_path.iterdir() if not p.name.startswith("given")) == before and not list(tmp_path.glob("**/prefix_ignored*"))
    if extra == ["--CHG", "--CHH"]:
        assert any(any(v) for v in want.values())                          # (not a comparison of zeros)


def test_session_errors_match_the_command(tmp_path, small_synth):
    """a bad command line gives the return code mbias_main gives, and -h an empty result"""
    base = [small_synth / "se.fa", small_synth / "se.bam"]
    bad = [base, base + ["p", "--noCpG"], base + ["p", "--chunkSize", "0"], base + ["p", "--bogus"], base + ["p", "-r", "nochrom:1-5"], base + ["--noSVG", "--noCpG"]]
    res, _, _ = run_session([("mbias", b) for b in bad] + [("mbias", ["-h"])], [], tmp_path)
    want = []
    for b in bad:
        cli = mdk.run_cli([str(a) for a in b], cwd=tmp_path, command="mbias")
        want.append(cli.returncode - 256 if cli.returncode > 127 else cli.returncode)
    assert [r["rc"] for r in res[:-1]] == want and want[:4] == [-1, -1, 1, 1] and want[4] != 0, (res, want)
    assert res[-1]["rc"] == 0 and res[-1]["rows"] == [] and res[-1]["counts"] == [] and res[-1]["suggested"] == {}


def test_session_reuse_does_not_carry_state(tmp_path, small_synth):
    """mbias, extract, mbias with other options, perRead, mbias on one session: each result equals a fresh session's, and the second mbias
    run holds none of the first run's counts (the extract and perRead legs get the oracle's dump and lines, as in their own CPU tests)"""
    from conftest import run_oracle
    a1 = [small_synth / "bis.fa", small_synth / "bis.bam", "--CHG", "--CHH", "--noSVG"]
    a2 = [small_synth / "se.fa", small_synth / "se.bam", "--CHG", "--noSVG"]
    o1, o2 = oracle_table(a1[:-1], tmp_path, "o1"), oracle_table(a2[:-1], tmp_path, "o2")
    xa = [small_synth / "se.fa", small_synth / "se.bam"]
    (tmp_path / "x").mkdir()
    assert run_oracle([str(a) for a in xa] + ["-o", "out"], cwd=tmp_path / "x", dump=tmp_path / "dump.tsv").returncode == 0
    pr = subprocess.run([str(ORACLE), "perRead"] + [str(a) for a in xa], cwd=tmp_path, capture_output=True, text=True)
    assert pr.returncode == 0
    (tmp_path / "perread.txt").write_text(pr.stdout)
    env = {"MDK_STANDIN_DUMP": tmp_path / "dump.tsv", "MDK_STANDIN_PERREAD": tmp_path / "perread.txt"}
    res, _, _ = run_session([("mbias", a1), ("extract", xa), ("mbias", a2), ("perread", xa), ("mbias", a1)], [o1[3], o2[3], o1[3]], tmp_path, **env)
    fresh1, _, _ = run_session([("mbias", a1)], [o1[3]], tmp_path)
    fresh2, _, _ = run_session([("mbias", a2)], [o2[3]], tmp_path)
    freshx, _, _ = run_session([("extract", xa)], [], tmp_path, **env)
    freshp, _, _ = run_session([("perread", xa)], [], tmp_path, **env)
    same_as_oracle(res[0], *o1[:3]); same_as_oracle(res[2], *o2[:3]); same_as_oracle(res[4], *o1[:3])
    assert res[0] == fresh1[0] == res[4] and res[2] == fresh2[0]
    want_x = sorted(tuple(t[i] for i in (0, 1, 2, 4, 5)) for t in (l.split("\t") for l in (tmp_path / "x" / "out_CpG.bedGraph").read_text().splitlines()[1:]))
    assert res[1] == freshx[0] and res[1]["rc"] == 0 and len(res[1]["rows"]) == len(want_x) > 100
    assert sorted((r[0], str(r[1]), str(r[2]), str(r[3]), str(r[4])) for r in res[1]["rows"]) == want_x
    assert res[3] == freshp[0] and res[3]["rc"] == 0 and len(res[3]["rows"]) == len(pr.stdout.splitlines()) > 100
    assert [r[0] for r in res[3]["rows"]] == [l.split("\t")[0] for l in pr.stdout.splitlines()]
    assert res[2]["rows"] != res[0]["rows"]
    assert sum(r[3] + r[4] for r in res[2]["rows"]) == sum(m + u for m, u in o2[1].values())       # none of the first run's counts
