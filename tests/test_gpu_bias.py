"""GPU: the session's mbias (Session.mbias -> Bias) against the oracle's table and suggestion line, and the group launch of the histogram
(md_dev_mbias_group, k_mbias_multi) against the single-chunk path at the C ABI.  The table must match row for row IN ORDER, as tensors on the
device; the paths on which a chunk of a group launch must add nothing and be counted by a launch of its own afterwards (a read longer than the
histogram, more segments than reserved) are checked to have been taken (Bias.resubmitted)."""
import os
import random

import numpy as np
import pytest

import methyldackel_amd as mdk
from bamwriter import record, write_bam, write_fasta
from bedgen import random_bed
from conftest import GOLDEN, run_oracle, synth
from test_bias_cpu import NAMES, hist_of, oracle_table
from test_gpu_edge_cases import bs_read, ref_with_cpgs
from test_mbias import FIX, SYN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def session():
    with mdk.Session(0) as s:
        yield s


def same_as_oracle(b, lines, table, want):
    import torch
    for name, dt in mdk.BIAS_COLUMNS:
        t = getattr(b, name)
        assert t.device == torch.device("cuda", 0) and str(t.dtype) == "torch." + dt, name
    assert b.rows() == lines                                               # row for row, in the command's order
    dense = hist_of(table).astype(np.int64)
    got = b.counts.cpu().numpy()                                           # len = the longest admitted read: rows past the last call are zero
    assert got.shape[1:] == (4, 2, 2) and got.shape[0] >= dense.shape[0]
    assert np.array_equal(got[:dense.shape[0]], dense) and not got[dense.shape[0]:].any()
    assert b.suggested == want and list(b.suggested) == [k for k in NAMES if k in want]
    assert len(b) == len(lines)


def compare(session, tmp_path, args, name="o", env=None, fresh=False):
    """the oracle's table, rows in order and suggestion against Session.mbias of the same command line; env / fresh: on a session of its own
    (MDK_TILE is read when a handle is opened; a fresh handle's histogram has its first capacity)"""
    lines, table, want, _ = oracle_table(args, tmp_path, name)
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        if env or fresh:
            with mdk.Session(0) as s:
                b = s.mbias(list(args) + ["--noSVG"])
        else:
            b = session.mbias(list(args) + ["--noSVG"])
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    same_as_oracle(b, lines, table, want)
    return b, lines, want


@pytest.mark.parametrize("args", FIX, ids=[" ".join(a[1:]).replace(str(GOLDEN) + "/", "") for a in FIX])
def test_fixtures(session, tmp_path, args):
    compare(session, tmp_path, args)


@pytest.mark.parametrize("which,extra", SYN, ids=[f"{w}:{' '.join(e)}" for w, e in SYN])
@pytest.mark.parametrize("env", [None, {"MDK_TILE": "512"}], ids=["tile-default", "tile-512"])
def test_synthetic(session, tmp_path, small_synth, which, extra, env):
    b, lines, _ = compare(session, tmp_path, [small_synth / f"{which}.fa", small_synth / f"{which}.bam"] + extra, env=env)
    assert len(lines) > 50


def test_bed_keepstrand_and_threads(session, tmp_path, small_synth):
    bed = random_bed(tmp_path / "r.bed", [("chrS1", 40000), ("chrS2", 20000)], n=60, seed=61)
    compare(session, tmp_path, [small_synth / "pe.fa", small_synth / "pe.bam", "-l", bed, "--keepStrand", "--CHG", "--chunkSize", "2500", "-@", "4"])


def test_host_prep_mode(session, tmp_path, small_synth):
    compare(session, tmp_path, [small_synth / "pe.fa", small_synth / "pe.bam", "--CHG", "--chunkSize", "7000"], env={"MDK_HOST_PREP": "1"})


def test_s1(session, tmp_path):
    synth(tmp_path / "S1", "-L", "1000000", "-c", "30", "-s", "0x5EED0001")
    compare(session, tmp_path, [tmp_path / "S1.fa", tmp_path / "S1.bam", "-@", "8"], "a")
    compare(session, tmp_path, [tmp_path / "S1.fa", tmp_path / "S1.bam", "-@", "8", "--CHG", "--CHH", "--nOT", "6,6,6,6", "--nOB", "6,6,6,6"], "b")


def abi_hist(args, group):
    """the histogram of a plan's chunks: group = 0 through md_dev_mbias_submit_raw chunk by chunk (the yardstick), else through
    md_dev_mbias_group, `group` chunks per launch; -> (histogram, chunks, chunks sent through the single-chunk path)"""
    plan = mdk.Plan(args, command="mbias")
    plan.set_prep(1)
    cfg = plan.dev_cfg(); cfg.n_slots = 8
    dev = mdk.Device(cfg)
    dev.set_prep(plan.prep_cfg())
    n, redone, pend = 0, 0, []
    while True:
        if not group:
            dev.slot_sync(n & 1)
        c = plan.next_chunk()
        if c is not None and c.skipped:
            continue
        if c is not None:
            assert c.prep == 1
            plan.ensure_reference(dev, c.tid)
            if group:
                dev.upload_raw(len(pend), c.raw)
                assert dev.L.md_dev_upload_wait(dev.h, len(pend)) == 0     # (the plan recycles the records two chunks on)
                pend.append(len(pend))
            else:
                dev.mbias_submit_raw(n & 1, c.raw)
            n += 1
        if pend and (c is None or len(pend) == group):
            rcs, redone = dev.mbias_group(pend)
            assert rcs == [0] * len(pend)
            pend = []
        if c is None:
            break
    h = dev.mbias_read()
    dev.close(); plan.close()
    return h, n, redone


@pytest.mark.parametrize("extra", [["--CHG", "--CHH", "--chunkSize", "997"], ["--CHG", "--CHH", "--chunkSize", "333", "--nOT", "2,3,4,5", "-p", "20"]], ids=["997", "333_trim"])
def test_abi_group_equals_single_chunk_path(small_synth, extra):
    """groups of 1, 2, 3 and 8 chunks, all contexts, small chunks (many chunk edges: window-relative contexts)"""
    args = [str(small_synth / "pe.fa"), str(small_synth / "pe.bam")] + extra + ["--noSVG"]
    want, n, _ = abi_hist(args, 0)
    assert want.sum() > 1000 and n > 40
    for g in (1, 2, 3, 8):
        got, m, redone = abi_hist(args, g)
        assert m == n and redone == 0
        assert got.shape == want.shape and (got == want).all(), g


def test_reads_longer_than_the_lds_rows(session, tmp_path):
    """reads of 700 bases: rows beyond the 512 a workgroup keeps in LDS go to the global histogram directly"""
    synth(tmp_path / "L", "-L", "60000", "-c", "12", "-l", "700", "-s", "91", "--single")
    b, lines, _ = compare(session, tmp_path, [tmp_path / "L.fa", tmp_path / "L.bam", "--CHG", "--CHH"])
    assert b.counts.shape[0] == 700 and b.resubmitted == 0 and max(l[2] for l in lines) == 700


def test_reads_longer_than_the_histogram_are_counted_exactly_once(session, tmp_path):
    """reads of 1,500 bases, longer than the histogram's first capacity (1,024 rows, hist_reserve): the group's kernel adds nothing for the
    chunk and flags it, the collector grows the histogram with the device drained and counts the chunk through the single-chunk path"""
    synth(tmp_path / "X", "-L", "60000", "-c", "12", "-l", "1500", "-s", "91", "--single")
    b, lines, want = compare(session, tmp_path, [tmp_path / "X.fa", tmp_path / "X.bam", "--CHG", "--CHH"], fresh=True)
    assert len(lines) == 3000 and want == {"OT": (611, 763, 0, 0), "OB": (645, 1114, 0, 0)}
    assert b.resubmitted >= 1
    # and on a warm handle whose histogram was dropped by the reset between runs, with small chunks: several flagged chunks, several groups
    b2, _, _ = compare(session, tmp_path, [tmp_path / "X.fa", tmp_path / "X.bam", "--CHG", "--CHH", "--chunkSize", "7000"], "o2")
    assert b2.resubmitted >= 1


def test_more_segments_than_reserved_are_counted_exactly_once(session, tmp_path):
    """the records of test_gpu_edge_cases.py::test_many_cigar_operations_far_skips_and_a_crowd_of_pairs: reads of ten gapless runs, so many
    that the chunk's segment array has to grow and its preparation runs again -- after the group's histogram kernel has left the chunk out"""
    rng = random.Random(11)
    L = 260000
    ref = ref_with_cpgs(L, 9)
    R = []

    def add(pos, flag, cig, qname, mpos=0):
        import re
        seq, p = [], pos
        for n, op in re.findall(r"(\d+)([MIDNS])", cig):
            n = int(n)
            if op == "M":
                seq.append(bs_read(ref, p, n, bool(flag & 0x40) != bool(flag & 0x10), rng)); p += n
            elif op in "IS":
                seq.append("".join(rng.choice("ACGT") for _ in range(n)))
            else:
                p += n
        s = "".join(seq)
        R.append((pos, len(R), record(0, pos, flag, cig, s, [rng.choice([12, 23, 37, 41]) for _ in range(len(s))], qname=qname, mpos=mpos)))

    many = "8M1D" * 9 + "8M"
    for k in range(1200):
        pos = 1000 + 15 * k
        add(pos, 99, many, f"m{k}", pos + 40); add(pos + 40, 147, many, f"m{k}", pos)
    for k in range(40):
        pos = 30000 + 50 * k
        add(pos, 99, f"30M{1000 + 3000 * k}N30M", f"n{k}", pos + 10); add(pos + 10, 147, "50M", f"n{k}", pos)
    for k in range(300):
        pos = 150000 + 20 * k
        add(pos, 99, "60M", f"f{k}", pos + 14000)
        add(pos + 14000, 147, "60M", f"f{k}", pos)
        if k % 10 == 0:
            add(pos + 7000, 99 | 0x800, "40M", f"f{k}", pos)
    for k in range(700):
        add(150010 + 20 * k, 0, "70M", f"s{k}")
    R.sort(key=lambda x: (x[0], x[1]))
    write_bam(tmp_path / "m.bam", [("c1", L)], [r for _, _, r in R])
    write_fasta(tmp_path / "m.fa", [("c1", ref)])
    b, lines, _ = compare(session, tmp_path, [tmp_path / "m.fa", tmp_path / "m.bam", "--CHG", "--CHH", "-q", "0"])
    assert b.resubmitted >= 1 and len(lines) > 100
    b, _, _ = compare(session, tmp_path, [tmp_path / "m.fa", tmp_path / "m.bam", "-F", "0", "--keepSingleton", "--keepDiscordant", "--chunkSize", "100000", "-q", "0"], "o2")
    assert b.resubmitted >= 1


def test_workflow_bounds_into_extract(session, tmp_path, small_synth):
    """mbias, then extract with the suggested bounds, in one session: equal to the oracle's extract with the oracle's own suggestion"""
    args = [small_synth / "bis.fa", small_synth / "bis.bam", "--CHG", "--CHH"]
    b, _, want = compare(session, tmp_path, args)
    assert any(any(v) for v in want.values())
    opts = [t for k in NAMES if k in want for t in ("--" + k, ",".join(str(x) for x in want[k]))]
    assert b.options() == opts
    calls = session.extract(args + b.options())
    od = tmp_path / "x"; od.mkdir()
    r = run_oracle([str(a) for a in args] + opts + ["-o", "out"], cwd=od)
    assert r.returncode == 0, r.stderr[-500:]
    plain = session.extract(args)
    seen = 0
    for k, ctx in enumerate(("CpG", "CHG", "CHH")):
        rows = [[t[0], int(t[1]), int(t[2]), int(t[4]), int(t[5])] for t in (l.split("\t") for l in (od / f"out_{ctx}.bedGraph").read_text().splitlines()[1:])]
        assert [list(x) for x in calls.rows(k)] == rows, ctx
        seen += len(rows)
    assert seen > 1000 and calls.rows() != plain.rows()                    # (the bounds trimmed something)


def test_contig_missing_from_fasta_ends_the_run_as_the_command(session, tmp_path, small_synth):
    """a chunk whose contig the FASTA lacks: the command's return code (-4), after groups of the first contig were launched -- the run waits
    for the handle before its plan gives the slabs back -- and the next runs on the same session are right"""
    fa = tmp_path / "one.fa"
    txt = (small_synth / "pe.fa").read_text()
    fa.write_text(txt[: txt.index(">", 1)])
    args = [fa, small_synth / "pe.bam", "--chunkSize", "3000", "--noSVG"]
    cli = mdk.run_cli([str(a) for a in args], cwd=tmp_path, command="mbias", timeout=300)
    assert cli.returncode == (-4 & 255)
    with pytest.raises(mdk.MdkError) as e:
        session.mbias(args)
    assert e.value.rc == -4
    compare(session, tmp_path, [small_synth / "pe.fa", small_synth / "pe.bam", "--CHG"])
    xa = [small_synth / "se.fa", small_synth / "se.bam"]
    with mdk.Session(0) as f:
        want = f.extract(xa).rows()
    assert session.extract(xa).rows() == want and len(want) > 100


def test_bias_outlives_the_session(small_synth, tmp_path):
    args = [small_synth / "se.fa", small_synth / "se.bam", "--CHG", "--noSVG"]
    s = mdk.Session(0)
    b = s.mbias(args)
    want, dense = b.rows(), b.counts.clone()
    s.close()
    import torch
    assert b.rows() == want and len(b) > 50 and torch.equal(b.counts, dense)
    with pytest.raises(mdk.MdkError):
        s.mbias(args)


def test_no_leak_over_ten_calls(session, small_synth):
    """ten alternating calls, one of them failing: free HBM and the resident set stay within 64 MiB of their values after the first"""
    import torch
    ma = [small_synth / "pe.fa", small_synth / "pe.bam", "--chunkSize", "8000", "--noSVG"]
    xa = [small_synth / "pe.fa", small_synth / "pe.bam", "--chunkSize", "8000"]
    with mdk.Session(0) as f:                                              # what extract and perRead give on a handle that never ran mbias
        want_x, want_p = f.extract(xa).rows(), f.perread(xa).rows()
    assert len(want_x) > 100 and len(want_p) > 100
    ref = session.mbias(ma)
    assert session.extract(xa).rows() == want_x and session.perread(xa).rows() == want_p
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    cur0 = int(open("/proc/self/statm").read().split()[1]) * os.sysconf("SC_PAGE_SIZE")
    for i in range(10):
        if i == 4:
            with pytest.raises(mdk.MdkError):
                session.mbias(ma + ["-r", "nochrom:1-5"])
        elif i % 3 == 1:
            x = session.extract(xa)
            assert x.rows() == want_x
            del x
        elif i % 3 == 2:
            x = session.perread(xa)
            assert x.rows() == want_p
            del x
        else:
            b = session.mbias(ma)
            assert b.rows() == ref.rows()
            del b
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    cur1 = int(open("/proc/self/statm").read().split()[1]) * os.sysconf("SC_PAGE_SIZE")
    assert free0 - free1 <= 64 << 20, (free0, free1)
    assert cur1 - cur0 <= 64 << 20, (cur0, cur1)


def test_growing_tables_on_another_session_after_mbias_runs(session, tmp_path, small_synth):
    """mbias runs -- one of them with chunks re-submitted and the histogram grown -- and then, in the same process on another session, the
    perRead and extract runs whose tables grow past their floors (the samples of test_tables_grow_with_rows_in_them in test_gpu_reads.py and
    test_gpu_calls.py): nothing an mbias run leaves in the process (staging blocks known to the runtime, carved memory, the host copy of the
    histogram) may reach a later run.  Each twice with equal columns"""
    import torch
    synth(tmp_path / "X", "-L", "60000", "-c", "12", "-l", "1500", "-s", "91", "--single")
    assert session.mbias([tmp_path / "X.fa", tmp_path / "X.bam", "--CHG", "--CHH", "--chunkSize", "7000", "--noSVG"]).resubmitted >= 1
    ref = session.mbias([small_synth / "pe.fa", small_synth / "pe.bam", "--noSVG"])
    synth(tmp_path / "g", "-L", "3000000", "-c", "30", "-s", "7")
    synth(tmp_path / "h", "-L", "9000000", "-c", "4", "-s", "7")
    with mdk.Session(0) as other:
        r, again = other.perread([tmp_path / "g.fa", tmp_path / "g.bam"]), other.perread([tmp_path / "g.fa", tmp_path / "g.bam"])
        assert len(r) > 1 << 18 and all(torch.equal(getattr(r, n), getattr(again, n)) for n, _ in mdk.READ_COLUMNS)
        os.environ["MDK_TILE"] = "512"
        try:
            xa = [tmp_path / "h.fa", tmp_path / "h.bam", "-@", "4", "--CHG", "--CHH"]
            c, again = other.extract(xa), other.extract(xa)
        finally:
            os.environ.pop("MDK_TILE")
        assert len(c) > 1 << 20 and all(torch.equal(getattr(c, n), getattr(again, n)) for n, _ in mdk.CALL_COLUMNS)
    assert session.mbias([small_synth / "pe.fa", small_synth / "pe.bam", "--noSVG"]).rows() == ref.rows()


def test_torch_first(tmp_path, small_synth):
    """torch has initialised the device before the session opens (a fresh process)"""
    import subprocess
    import sys
    from conftest import REPO
    args = [str(small_synth / "bis.fa"), str(small_synth / "bis.bam"), "--CHG", "--CHH"]
    lines, _, want, _ = oracle_table(args, tmp_path)
    code = ("import sys, json, torch; x = torch.ones(1024, device='cuda:0') * 2; torch.cuda.synchronize(); sys.path.insert(0, %r)\n"
            "import methyldackel_amd as mdk\n"
            "with mdk.Session(0) as s:\n    b = s.mbias(sys.argv[1:] + ['--noSVG'])\n"
            "assert b.counts.device == x.device and int((b.nmeth + b.nunmeth).sum()) == int(b.counts.sum())\n"
            "print('RESULT ' + json.dumps({'rows': [list(r) for r in b.rows()], 'opts': b.options()}))\n" % str(REPO))
    r = subprocess.run([sys.executable, "-c", code] + args, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    import json
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert [tuple(x) for x in got["rows"]] == lines
    assert got["opts"] == [t for k in NAMES if k in want for t in ("--" + k, ",".join(str(x) for x in want[k]))]
