"""CPU-only: the united table as text and back (csrc/mdk_cohort_core.h), driven through tools/cohort_emu -- the host build of the header in
the kernels' blocking: one hand-written table against its text as a literal, the emulator against the restatement with str.join /
bytes.split (tests/cohort_rule.py) for both formats under several blockings, the way back, every refusal of the parser, and the argument
checks of Cohort.write / Cohort.read that need no device."""
import subprocess

import pytest

import cohort_rule as rule
from conftest import REPO

EMU = REPO / "tools" / "_build" / "cohort_emu"
FORMATS = {"cohort": 0, "methylBase": 1}
WRITE_CODES = {1: "position", 2: "contig", 3: "end", 4: "context", 5: "negative"}
BLOCKINGS = ((64, 32), (64, 2))            # (tile_sites, sample_block): the defaults, and the GPU test's limits


def emu_render(t, fmt, tile=64, sblock=32, lead=0):
    """the table's lines by the emulator, `lead` bytes behind a 16-byte boundary; a refused table: (reason, site, sample)"""
    S, n = len(t["m"]), len(t["sites"])
    lines = ["R %d %d %d %d %d %d %d" % (FORMATS[fmt], tile, sblock, S, n, len(t["contigs"]), lead)] + list(t["contigs"])
    lines += ["%d %d %d %d %d %d" % s for s in t["sites"]]
    for j in range(S):
        lines += ["%d %d" % e for e in zip(t["m"][j], t["u"][j])]
    r = subprocess.run([str(EMU)], input=("\n".join(lines) + "\n").encode("latin-1"), capture_output=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    head, _, rest = r.stdout.partition(b"\n")
    f = head.split()
    if f[0] == b"ERR":
        return WRITE_CODES[int(f[1])], int(f[2]), int(f[3])
    assert len(rest) == int(f[1])
    return rest


def emu_parse(text, S, contigs, tile=64, begin=0, prev=None):
    """(sites, m, u) of text[begin:] by the emulator, or (refusal, row, offset of the row's first byte)"""
    head = "P %d %d %d %d %d %d %d %d\n" % (tile, S, len(contigs), len(text), begin, int(prev is not None), *(prev or (0, 0)))
    r = subprocess.run([str(EMU)], input=(head + "".join(c + "\n" for c in contigs)).encode("latin-1") + text, capture_output=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    lines = r.stdout.decode().splitlines()
    f = lines[0].split()
    if f[0] == "ERR":
        return f[1], int(f[2]), int(f[3])
    rows = [[int(v) for v in ln.split()] for ln in lines[1:]]
    assert len(rows) == int(f[1])
    return [tuple(r[:6]) for r in rows], [[r[6 + 2 * j] for r in rows] for j in range(S)], [[r[7 + 2 * j] for r in rows] for j in range(S)]


def table_of(t):
    return [tuple(s) for s in t["sites"]], [list(x) for x in t["m"]], [list(x) for x in t["u"]]


HAND = {"contigs": ["chr1", "chrM"], "names": ["ctl", "kd.1", "kd.2"], "merged": True, "contexts_on": (0, 2), "n_union": 7,
        "sites": [(0, 10, 12, 0, 0, 3), (0, 99, 100, 2, 1, 1), (1, 0, 1, 1, -1, 2)],
        "m": [[5, 0, 2147483647], [1, 0, 0], [12, 7, 3]], "u": [[0, 0, 1], [2, 0, 0], [30, 0, 2147483647]]}
HAND_COHORT = ("#methyldackel_amd cohort 1\tsamples=3\tmerged=1\tcontexts=0,2\tn_union=7\n"
               "#chrom\tstart\tend\tcontext\tstrand\tnsamples\tctl.nmeth\tctl.nunmeth\tkd.1.nmeth\tkd.1.nunmeth\tkd.2.nmeth\tkd.2.nunmeth\n"
               "chr1\t10\t12\tCG\t.\t3\t5\t0\t1\t2\t12\t30\n"
               "chr1\t99\t100\tCHH\t+\t1\t0\t0\t0\t0\t7\t0\n"
               "chrM\t0\t1\tCHG\t-\t2\t2147483647\t1\t0\t0\t3\t2147483647\n")
HAND_METHYLBASE = ("chr\tstart\tend\tstrand\tcoverage1\tnumCs1\tnumTs1\tcoverage2\tnumCs2\tnumTs2\tcoverage3\tnumCs3\tnumTs3\n"
                   "chr1\t11\t11\t+\t5\t5\t0\t3\t1\t2\t42\t12\t30\n"
                   "chr1\t100\t100\t+\t0\t0\t0\t0\t0\t0\t7\t7\t0\n"
                   "chrM\t1\t1\t-\t2147483648\t2147483647\t1\t0\t0\t0\t2147483650\t3\t2147483647\n")


def test_hand_table_is_its_literal():
    """3 samples, 2 contigs, a merged row with `.`, `0 0` cells, 10-digit counts: the rule, the emulator and the package's header all give
    the text written out here -- so rule and code cannot agree on something else"""
    import methyldackel_amd as mdk
    for fmt, want in (("cohort", HAND_COHORT), ("methylBase", HAND_METHYLBASE)):
        want = want.encode()
        assert rule.render(fmt, HAND) == want
        head = mdk._cohort_header(fmt, HAND["names"], HAND["merged"], HAND["contexts_on"], HAND["n_union"])
        assert head == rule.header(fmt, HAND).encode()
        for tile, sblock in BLOCKINGS:
            assert head + emu_render(HAND, fmt, tile, sblock, lead=len(head)) == want


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 257, 513))
def test_emulator_renders_the_rule(n):
    """seeded tables, both formats, every S on both sides of a sample block and of a wavefront, under the default blocking and the GPU
    test's; the text lies behind its real header, so the destination's alignment is whatever the header's length makes it"""
    for S in (1, 2, 31, 32, 33, 65):
        t = rule.shared_table(n, S, merged=bool(S & 1))
        for fmt in FORMATS:
            want, lead = rule.body(fmt, t), len(rule.header(fmt, t))
            for tile, sblock in BLOCKINGS:
                assert emu_render(t, fmt, tile, sblock, lead) == want, (n, S, fmt, tile, sblock)


def test_emulator_renders_1024_samples():
    t = rule.shared_table(3, 1024)
    for fmt in FORMATS:
        for tile, sblock in BLOCKINGS:
            assert emu_render(t, fmt, tile, sblock, 5) == rule.body(fmt, t)


def test_names_and_alignments():
    """names of 1 and of 255 bytes in the header; and name lengths that walk the first line's destination through all 16 alignments"""
    import methyldackel_amd as mdk
    t = rule.shared_table(65, 3)
    seen = set()
    for length, n_union in [(1, 70), (255, 70)] + [(k, u) for k in range(2, 10) for u in (70, 700)]:           # (a name stands in the header twice)
        tn = dict(rule.with_names(t, rule.sample_names(3, length)), n_union=n_union)
        head = rule.header("cohort", tn).encode("latin-1")
        assert mdk._cohort_header("cohort", tn["names"], tn["merged"], tn["contexts_on"], tn["n_union"]) == head
        seen.add(len(head) & 15)
        assert head + emu_render(tn, "cohort", 64, 2, len(head)) == rule.render("cohort", tn)
    assert len(seen) == 16
    for lead in range(16):
        assert emu_render(t, "methylBase", 64, 32, lead) == rule.body("methylBase", t)


@pytest.mark.parametrize("n,S", ((0, 2), (1, 1), (65, 3), (257, 33), (513, 2), (3, 1024), (70, 130)))
def test_parse_gives_the_table_back(n, S):
    """emulator parse of emulator render, and of the rule's text, under a full tile and a shrunk one; the rule's parser agrees"""
    t = rule.shared_table(n, S, merged=True)
    text = rule.render("cohort", t)
    hdr = len(rule.header("cohort", t))
    assert text[hdr:] == emu_render(t, "cohort", 64, 32, hdr)
    assert rule.parse(text[hdr:], S, t["contigs"]) == table_of(t)
    for tile in (64, 3):
        assert emu_parse(text, S, t["contigs"], tile, begin=hdr) == table_of(t)


def refusal_cases():
    """(name, the lines of a body, the refusal, its 1-based line in a file with two header lines) for S = 2 and contigs chr1, chr2"""
    ok = [b"chr1\t5\t6\tCG\t+\t2\t1\t2\t3\t4", b"chr1\t9\t11\tCHG\t.\t1\t0\t0\t7\t8", b"chr2\t1\t2\tCHH\t-\t0\t0\t0\t0\t0"]
    def at(k, ln):
        out = list(ok); out[k] = ln
        return out
    big = b"chr1\t9\t11\tCG\t+\t1\t0\t0\t7\t" + b"8" * 32760
    return [
        ("long", at(1, big), "long", 4),
        ("hash", at(2, b"#chrom\tstart"), "hash", 5),
        ("empty", at(1, b""), "empty", 4),
        ("few", at(0, b"chr1\t5\t6\tCG\t+\t2\t1\t2\t3"), "few", 3),
        ("many", at(2, b"chr2\t1\t2\tCHH\t-\t0\t0\t0\t0\t0\t0"), "many", 5),
        ("field", at(1, b"chr1\t9\t11\tCHG\t.\t1\t\t0\t7\t8"), "field", 4),
        ("field_last", at(1, b"chr1\t9\t11\tCHG\t.\t1\t0\t0\t7\t"), "field", 4),
        ("contig", at(1, b"chr3\t9\t11\tCHG\t.\t1\t0\t0\t7\t8"), "contig", 4),
        ("contig_long", at(1, b"c" * 300 + b"\t9\t11\tCHG\t.\t1\t0\t0\t7\t8"), "contig", 4),
        ("digit", at(1, b"chr1\t9\t11\tCHG\t.\t1\t0\t-1\t7\t8"), "digit", 4),
        ("digit_start", at(0, b"chr1\t+5\t6\tCG\t+\t2\t1\t2\t3\t4"), "digit", 3),
        ("overflow", at(1, b"chr1\t9\t11\tCHG\t.\t1\t0\t0\t2147483648\t8"), "overflow", 4),
        ("overflow_len", at(1, b"chr1\t9\t11\tCHG\t.\t1\t0\t0\t00000000001\t8"), "overflow", 4),
        ("context", at(1, b"chr1\t9\t11\tCHGG\t.\t1\t0\t0\t7\t8"), "context", 4),
        ("context_short", at(1, b"chr1\t9\t11\tC\t.\t1\t0\t0\t7\t8"), "context", 4),
        ("strand", at(1, b"chr1\t9\t11\tCHG\t*\t1\t0\t0\t7\t8"), "strand", 4),
        ("strand_long", at(1, b"chr1\t9\t11\tCHG\t+-\t1\t0\t0\t7\t8"), "strand", 4),
        ("end", at(1, b"chr1\t9\t9\tCHG\t.\t1\t0\t0\t7\t8"), "end", 4),
        ("nsamples", at(1, b"chr1\t9\t11\tCHG\t.\t3\t0\t0\t7\t8"), "nsamples", 4),
        ("order_equal", at(1, b"chr1\t5\t7\tCHG\t.\t1\t0\t0\t7\t8"), "order", 4),
        ("order_contig", [ok[2], ok[0]], "order", 4),
        # two refusals on one line: the earlier in the fixed order
        ("many_before_field", at(1, b"chr1\t9\t11\tCHG\t.\t1\t\t0\t7\t8\t9"), "many", 4),
        ("contig_before_digit", at(1, b"chr3\t9\tx\tCHG\t.\t1\t0\t0\t7\t8"), "contig", 4),
        ("digit_before_overflow", at(1, b"chr1\t9\t11\tCHG\t.\t1\t0\tx\t2147483648\t8"), "digit", 4),
        ("overflow_before_digit", at(1, b"chr1\t9\t11\tCHG\t.\t1\t2147483648\tx\t7\t8"), "overflow", 4),
        ("context_before_strand", at(1, b"chr1\t9\t11\tcg\t?\t1\t0\t0\t7\t8"), "context", 4),
        ("digit_before_end", at(1, b"chr1\t9\t9\tCHG\t.\t1\t0\tx\t7\t8"), "digit", 4),
        ("end_before_nsamples", at(1, b"chr1\t9\t9\tCHG\t.\t3\t0\t0\t7\t8"), "end", 4),
        ("format_before_order", at(1, b"chr1\t5\t6\tCHG\t.\t3\t0\t0\t7\t8"), "nsamples", 4),
        ("first_line_wins", [ok[0], b"chr1\t9\t9\tCHG\t.\t1\t0\t0\t7\t8", b"", ok[2]], "end", 4),
    ]


REFUSALS = refusal_cases()


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_parser_refusals(case):
    _, lines, want, lineno = case
    text = b"\n".join(lines) + b"\n"
    assert rule.parse(text, 2, ["chr1", "chr2"]) == (want, lineno)
    for tile in (64, 2):
        got = emu_parse(text, 2, ["chr1", "chr2"], tile)
        assert got[0] == want and got[1] + 3 == lineno and got[2] == sum(len(x) + 1 for x in lines[:got[1]]), got
    assert want in rule.MESSAGES


def test_crlf_and_a_last_line_without_newline():
    t = rule.shared_table(65, 2)
    body = rule.body("cohort", t)
    for text in (body.replace(b"\n", b"\r\n"), body[:-1], body.replace(b"\n", b"\r\n")[:-2], body.replace(b"\n", b"\r\n")[:-1]):
        assert rule.parse(text, 2, t["contigs"]) == table_of(t)
        assert emu_parse(text, 2, t["contigs"]) == table_of(t)
    assert emu_parse(body + b"\n", 2, t["contigs"])[0] == "empty"
    assert emu_parse(body.replace(b"\n", b"\r\r\n"), 2, t["contigs"])[0] == "digit"


def test_a_file_cut_at_every_offset():
    """a 3-line file in two pieces, cut the way the reader cuts (behind the piece's last newline), at every offset: the pieces' rows are the
    file's, and a row out of order across the cut is refused in the second piece's first line"""
    t = rule.shared_table(3, 2)
    text = rule.render("cohort", t)
    hdr = len(rule.header("cohort", t))
    swapped = text[:hdr] + b"".join(reversed(text[hdr:].splitlines(keepends=True)))
    for k in range(hdr + 1, len(text)):
        cut = text.rfind(b"\n", 0, k) + 1
        first = emu_parse(text[:cut], 2, t["contigs"], begin=hdr)
        prev = first[0][-1][:2] if first[0] else None
        second = emu_parse(text[cut:], 2, t["contigs"], prev=prev)
        assert first[0] + second[0] == table_of(t)[0]
        assert [a + b for a, b in zip(first[1], second[1])] == t["m"] and [a + b for a, b in zip(first[2], second[2])] == t["u"]
        cut = swapped.rfind(b"\n", 0, k) + 1
        first = emu_parse(swapped[:cut], 2, t["contigs"], begin=hdr)
        if first[0] == "order":
            continue
        second = emu_parse(swapped[cut:], 2, t["contigs"], prev=first[0][-1][:2] if first[0] else None)
        assert second[0] == "order" and second[1] == (1 if not first[0] else 0)


def test_emulator_write_refusals():
    base = rule.shared_table(70, 3)
    def changed(site=None, count=None):
        t = dict(base, sites=list(base["sites"]), m=[list(x) for x in base["m"]], u=[list(x) for x in base["u"]])
        if site:
            t["sites"][site[0]] = site[1]
        if count:
            t[count[0]][count[1]][count[2]] = -1
        return t
    c, a, b, x, s, k = base["sites"][66]
    cases = [changed(site=(66, (c, -1, b, x, s, k))), changed(site=(66, (-1, a, b, x, s, k))), changed(site=(66, (3, a, b, x, s, k))),
             changed(site=(66, (c, a, a, x, s, k))), changed(site=(66, (c, a, b, 3, s, k))), changed(count=("u", 2, 66)), changed(count=("m", 1, 5))]
    two = changed(site=(66, (c, a, a, 3, s, k)), count=("m", 0, 66))
    two["u"][1][3] = -1
    for t, want in zip(cases + [two], ["position", "position", "contig", "end", "context", "negative", "negative", "negative"]):
        got = rule.write_refusal(t)
        assert got[0] == want
        for fmt in FORMATS:
            for tile, sblock in BLOCKINGS:
                r = emu_render(t, fmt, tile, sblock)
                assert r[:2] == got[:2] and (got[2] is None or r[2] == got[2]), (r, got)


# ---- argument checks that need no device ----
def cpu_cohort(names=None):
    import torch
    import methyldackel_amd as mdk
    t = HAND
    cols = {name: torch.tensor([s[k] for s in t["sites"]], dtype=getattr(torch, dt)) for k, (name, dt) in enumerate(rule.SITE_COLUMNS)}
    return mdk.Cohort(t["contigs"], cols, torch.tensor(t["m"], dtype=torch.int32), torch.tensor(t["u"], dtype=torch.int32), True, (0, 2), 7, names=names)


def test_cpu_tensors_are_refused(tmp_path):
    import methyldackel_amd as mdk
    c = cpu_cohort()
    assert c.names is None and c.select(slice(0, 2)).names is None
    for call in (lambda: c.write(tmp_path / "x.tsv"), lambda: c.render(), lambda: c.render("methylBase", compress=True)):
        with pytest.raises(mdk.MdkError, match="no CPU path"):
            call()
    assert not (tmp_path / "x.tsv").exists()


def test_names_and_format_are_checked(tmp_path):
    import methyldackel_amd as mdk
    c = cpu_cohort(names=["a", "b", "c"])
    assert c.names == ("a", "b", "c") and c.select(slice(1, 3)).names == ("a", "b", "c")
    for bad, what in ((["a", "", "c"], "not 1 to 255 bytes"), (["a", "b\tx", "c"], "not 1 to 255 bytes"), (["a", "b", "a"], "the same name"), (["a", "b"], "2 names for 3 samples"),
                      (["a", "b", "x" * 256], "not 1 to 255 bytes"), (["a", "b", "c d"], "not 1 to 255 bytes"), ("abc", "a sequence of sample names")):
        with pytest.raises(mdk.MdkError, match=what):
            c.write(tmp_path / "x.tsv", names=bad)
        with pytest.raises(mdk.MdkError, match=what):
            cpu_cohort(names=bad)
    with pytest.raises(mdk.MdkError, match="unknown format"):
        c.write(tmp_path / "x.tsv", fmt="bedGraph")
    with pytest.raises(mdk.MdkError, match="piece_bytes"):
        c.write(tmp_path / "x.tsv", piece_bytes=-1)
    assert not (tmp_path / "x.tsv").exists()


def test_read_checks_the_header_first(tmp_path):
    import methyldackel_amd as mdk
    good = HAND_COHORT.encode()
    first, second, rest = good.split(b"\n", 2)
    cases = [(b"#methyldackel_amd cohort 2" + first[26:], second, "line 1"), (first.replace(b"samples=3", b"samples=0"), second, "line 1"),
             (first.replace(b"\tmerged=1", b""), second, "line 1"), (b"chr1\t1\t2", second, "line 1"), (b"", b"", "line 1"),
             (first, second + b"\textra", "line 2"), (first, second.rsplit(b"\t", 1)[0], "line 2"), (first, second.replace(b"kd.1.nunmeth", b"kd.2.nunmeth"), "line 2"),
             (first, second.replace(b"kd.1", b"ctl"), "line 2"), (first, second.replace(b"#chrom", b"chrom"), "line 2")]
    for k, (a, b, what) in enumerate(cases):
        p = tmp_path / f"bad{k}.tsv"
        p.write_bytes(a + b"\n" + b + b"\n" + rest)
        with pytest.raises(mdk.MdkError, match=what):
            mdk.Cohort.read(p, HAND["contigs"])
    got = mdk._cohort_read_header(_write(tmp_path / "good.tsv", good), "plain")
    assert got == (3, True, (0, 2), 7, ("ctl", "kd.1", "kd.2"), len(first) + len(second) + 2)
    import gzip
    with pytest.raises(mdk.MdkError, match="not BGZF"):
        mdk.Cohort.read(_write(tmp_path / "plain.gz", gzip.compress(good)), HAND["contigs"])


def _write(path, data):
    path.write_bytes(data)
    return path
