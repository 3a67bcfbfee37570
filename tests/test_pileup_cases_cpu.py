"""CPU-only: the hand-built cases of tests/batchgen.py that tests/test_gpu_pileup_kernel.py runs on the device.
  * every case still reaches the edge it is named for (its `reaches` predicate), at every tile size it runs at, and stays within the
    evaluator's budget: a case that stops hitting its edge after an edit fails here, without a GPU;
  * the references of the carpet, saturated-list, deep-pile and tile-edge cases, written as FASTA + BAM with the reads of those cases,
    go through the oracle and through the host preparation + evaluator (tests/test_host_logic.py check): the evaluator's context and
    counting rules are pinned to the oracle at exactly these extremes."""
import numpy as np
import pytest

import batchgen as bg
from bamwriter import record, write_bam, write_fasta
from test_host_logic import check


@pytest.mark.parametrize("name", [n for n, _ in bg.CASES])
def test_case_reaches_its_edge(name):
    ref, fields, regions, batch, reaches = bg.build(name)
    assert bg.evaluated_bases(batch) <= bg.BUDGET
    S = bg.seg_array(batch)
    if batch.n_segs:        # the contract the evaluator asserts; everything else may vary freely
        assert (S["len"] >= 1).all() and (S["q0"].astype(np.int64) + S["len"] <= S["l_qseq"]).all()
        P = S[(S["sf"] & 32) != 0]
        assert (P["m_q0"].astype(np.int64) + P["len"] <= P["m_l_qseq"]).all()
    result = bg.expected(name, (1, 1, 1), 1)
    for tile in bg.tiles_for(name):
        assert reaches(batch, tile, result), f"case {name} no longer reaches its edge at tile {tile}"
    # the keep masks the kernels run under give an answer too (the strand-0 abort included), and fewer contexts never give more sites
    for keep in ((1, 0, 0),) + tuple(fields.get("keeps", ())):
        sub = bg.expected(name, keep, 1)
        assert type(sub) is type(result) or result == bg.ERR_STRAND0
        if isinstance(sub, dict) and isinstance(result, dict):
            assert all(result[p] == v for p, v in sub.items())


@pytest.mark.parametrize("name", [n for n, _ in bg.MBIAS_CASES])
def test_mbias_case_reaches_its_edge(name):
    ref, fields, _, batch, reaches = bg.build_mbias(name)
    assert bg.evaluated_bases(batch) <= bg.BUDGET
    assert not (bg.seg_array(batch)["sf"] & 32).any()
    assert reaches(batch, 512, bg.expected_mbias(name, (1, 1, 1)))


def test_group_tile_counts():
    """the group launch test's eight intervals have the tile counts it is about, at both tile sizes"""
    import test_gpu_pileup_kernel as gk
    for tile in (512, 2048):
        got = [(b.end - b.beg + tile - 1) // tile for _, b in gk.group_batches(tile)]
        assert got == list(gk.GROUP_TILES)


# ---- the same references through the oracle ----
def records_of(tid, ref, batch, tag):
    """the case's segments as unpaired BAM records (OT/CTOT -> forward = OT, OB/CTOB -> reverse = OB), clipped to the contig"""
    out = []
    for i, s in enumerate(bg.seg_array(batch)):
        pos, n = int(s["rpos"]), int(s["len"])
        seq, qual = bg.seg_payload(batch, s)
        if pos < 0:
            seq, qual, n, pos = seq[-pos:], qual[-pos:], n + pos, 0
        n = min(n, len(ref) - pos)
        if n < 1 or not (s["sf"] & 7):
            continue
        out.append((pos, i, record(tid, pos, 0 if s["sf"] & 1 else 16, f"{n}M", seq[:n].replace("=", "N"), qual[:n], qname=f"{tag}{i}")))
    return out


def write_cases(tmp_path, names):
    contigs, seqs, recs = [], [], []
    for tid, name in enumerate(names):
        ref, _, _, batch, _ = bg.build(name)
        contigs.append((name, len(ref)))
        seqs.append((name, ref.decode()))
        recs += [(tid,) + r for r in records_of(tid, ref, batch, name)]
    recs.sort(key=lambda r: r[:3])
    write_fasta(tmp_path / "c.fa", seqs)
    write_bam(tmp_path / "c.bam", contigs, [r[3] for r in recs])
    return [str(tmp_path / "c.fa"), str(tmp_path / "c.bam")]


ORACLE_SETS = {
    "carpet": [n for n, _ in bg.CASES if n.startswith("carpet_")],
    "lists": [n for n, _ in bg.CASES if n.startswith("lists_")],
    "edges": ["edges_points", "edges_span", "edges_contig_end", "edges_gap"],
    "deep": ["deep_ob", "deep_opposite"],          # (deep_ot is deep_ob on the other base; one command line: 200,000 records take seconds)
}
ORACLE_ARGS = [[], ["--CHG", "--CHH", "--minOppositeDepth", "1", "-p", "5"], ["--noCpG", "--CHG"], ["--noCpG", "--CHH", "--chunkSize", "512"]]


@pytest.mark.parametrize("which", list(ORACLE_SETS))
def test_oracle_agrees_with_evaluator_on_the_case_references(tmp_path, which):
    args = write_cases(tmp_path, ORACLE_SETS[which])
    for k, extra in enumerate(ORACLE_ARGS if which != "deep" else ORACLE_ARGS[1:2]):
        d = tmp_path / f"run{k}"
        d.mkdir()
        check(d, args + extra, variant="--minOppositeDepth" in extra)
