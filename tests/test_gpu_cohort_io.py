"""GPU: the united table written as text and read back on the device (k_ctext_len, k_ctext_fill, k_cparse_len, k_cparse_fill of
csrc/mdk_cohort.hip, libmdk_cohort.so) -- Cohort.write, Cohort.render, Cohort.read, Cohort.names and mdk.cohort_limits.  Every comparison
is byte for byte, or torch.equal on every column plus the dtype, against the restatement with str.join / bytes.split
(tests/cohort_rule.py), which tests/test_cohort_io_cpu.py holds against the host build of the same header.  The tables are hand-made; no
BAM is used."""
import gzip
import re

import pytest

import cohort_rule as rule
from test_cohort_io_cpu import HAND, HAND_COHORT, REFUSALS

pytestmark = pytest.mark.gpu
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 513, 4100)
SAMPLES = (1, 3, 33, 130)
FORMATS = ("cohort", "methylBase")


def cohort_of(t, names="table"):
    """the table dict as a Cohort on the device"""
    import torch
    import methyldackel_amd as mdk
    S, n = len(t["m"]), len(t["sites"])
    cols = {name: torch.tensor([s[k] for s in t["sites"]], dtype=getattr(torch, dt)).cuda() for k, (name, dt) in enumerate(rule.SITE_COLUMNS)}
    m, u = (torch.tensor(t[w], dtype=torch.int32).reshape(S, n).cuda() for w in ("m", "u"))
    return mdk.Cohort(list(t["contigs"]), cols, m, u, t["merged"], t["contexts_on"], t["n_union"], names=t["names"] if names == "table" else names)


def tensors(c):
    return [getattr(c, name) for name, _ in rule.SITE_COLUMNS] + [c.nmeth, c.nunmeth]


def same(a, b):
    """two Cohorts equal in every column and its dtype, in names, merged, contexts_on and n_union"""
    import torch
    return (all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(tensors(a), tensors(b)))
            and a.names == b.names and a.merged == b.merged and a.contexts_on == b.contexts_on and a.n_union == b.n_union and list(a.contigs) == list(b.contigs))


def text_of(t):
    return bytes(t.cpu().numpy())


# first in the file: the kernels' first execution
@pytest.mark.parametrize("n", SIZES)
def test_render_and_write_are_the_rule(n, tmp_path):
    """both formats at every size, S taking turns over the sizes; a second run gives the same bytes, and the inputs are as they were"""
    import torch
    S = SAMPLES[SIZES.index(n) % len(SAMPLES)]
    t = rule.shared_table(n, S, merged=bool(n & 1))
    c = cohort_of(t)
    before = [x.clone() for x in tensors(c)]
    for fmt in FORMATS:
        want = rule.render(fmt, t)
        got = c.render(fmt)
        assert got.dtype == torch.uint8 and got.device == c.nmeth.device and text_of(got) == want, (n, S, fmt)
        path = tmp_path / f"t.{fmt}"
        assert c.write(path, fmt) == path and path.read_bytes() == want
        assert text_of(c.render(fmt)) == want
    assert all(torch.equal(a, b) for a, b in zip(tensors(c), before))


def test_1024_samples():
    t = rule.shared_table(3, 1024)
    c = cohort_of(t)
    for fmt in FORMATS:
        assert text_of(c.render(fmt)) == rule.render(fmt, t)
    assert same(type(c).read(_file(rule.render("cohort", t)), t["contigs"]), c)


_files = []


def _file(data, suffix=".tsv"):
    import tempfile
    f = tempfile.NamedTemporaryFile(suffix=suffix, delete=False)
    f.write(data); f.close()
    _files.append(f.name)
    return f.name


@pytest.fixture(scope="module", autouse=True)
def _cleanup():
    import os
    yield
    for f in _files:
        if os.path.exists(f):
            os.unlink(f)


def test_limits_do_not_change_a_byte():
    """tile_sites 64, sample_block 2, at most 3 workgroups: the bytes and the columns of the defaults"""
    import methyldackel_amd as mdk
    cases = [(n, S, rule.shared_table(n, S, merged=True)) for n, S in ((513, 3), (257, 33), (65, 130))]
    try:
        mdk.cohort_limits(tile_sites=64, sample_block=2, max_workgroups=3)
        for n, S, t in cases:
            c = cohort_of(t)
            for fmt in FORMATS:
                assert text_of(c.render(fmt)) == rule.render(fmt, t), (n, S, fmt)
            assert same(mdk.Cohort.read(_file(rule.render("cohort", t)), t["contigs"]), c)
        with pytest.raises(mdk.MdkError, match="tile_sites a multiple of 64"):
            mdk.cohort_limits(tile_sites=100)
    finally:
        mdk.cohort_limits()


def test_pieces(tmp_path):
    """piece_bytes small enough for many blocks, and smaller than one line (blocks of one row): the plain file is the single-block one, and
    gzip.decompress of the compressed file is it too"""
    t = rule.shared_table(513, 3)
    c = cohort_of(t)
    for fmt in FORMATS:
        want = rule.render(fmt, t)
        for piece in (4096, 7):
            assert c.write(tmp_path / "p.tsv", fmt, piece_bytes=piece).read_bytes() == want
        for piece in (None, 4096, 300):
            z = c.write(tmp_path / "p.tsv.gz", fmt, compress=True, piece_bytes=piece).read_bytes()
            assert gzip.decompress(z) == want and z.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
            assert text_of(c.render(fmt, compress=True, piece_bytes=piece)) == z


@pytest.mark.parametrize("n,S", ((0, 2), (1, 1), (513, 3), (4100, 3), (257, 33)))
def test_read_of_write_is_the_table(n, S, tmp_path):
    """every column, names, merged, contexts_on and n_union, from plain text and from BGZF, whole and in pieces so small that lines straddle
    pieces and BGZF members"""
    import methyldackel_amd as mdk
    t = rule.with_names(rule.shared_table(n, S, merged=bool(n & 1)), rule.sample_names(S, 5))
    c = cohort_of(t)
    plain, packed = c.write(tmp_path / "c.tsv"), c.write(tmp_path / "c.tsv.gz", compress=True, piece_bytes=100000)
    longest = max(len(x) for x in plain.read_bytes().splitlines()) + 1
    for path, blocks in ((plain, (None, longest + 40)), (packed, (None, 65536))):
        for block_bytes in blocks:
            got = mdk.Cohort.read(path, t["contigs"], block_bytes=block_bytes)
            assert same(got, c), (n, S, path, block_bytes)
            assert got.names == tuple(t["names"]) and got.nmeth.is_contiguous()
    sub = c.select(slice(0, n // 2))
    assert sub.names == c.names and text_of(sub.render()) == rule.render("cohort", dict(t, sites=t["sites"][:n // 2], m=[x[:n // 2] for x in t["m"]], u=[x[:n // 2] for x in t["u"]]))


def test_read_of_a_file_the_device_never_wrote(tmp_path):
    """the rule's own text, with CRLF line ends and without the last newline too; unite-less names default to s0 ..."""
    import methyldackel_amd as mdk
    t = rule.shared_table(257, 3, merged=True)
    c = cohort_of(t)
    text = rule.render("cohort", t)
    hdr = len(rule.header("cohort", t))
    for k, data in enumerate((text, text[:hdr] + text[hdr:].replace(b"\n", b"\r\n"), text[:-1])):
        p = tmp_path / f"r{k}.tsv"
        p.write_bytes(data)
        assert same(mdk.Cohort.read(p, t["contigs"]), c)
        assert same(mdk.Cohort.read(p, t["contigs"], block_bytes=400), c)
    assert text_of(cohort_of(t, names=None).render()) == rule.render("cohort", rule.with_names(t, ["s0", "s1", "s2"]))
    hand = mdk.Cohort.read(_file(HAND_COHORT.encode()), HAND["contigs"])
    assert same(hand, cohort_of(HAND)) and hand.names == ("ctl", "kd.1", "kd.2") and hand.merged and hand.contexts_on == (0, 2) and hand.n_union == 7


HEAD = b"#methyldackel_amd cohort 1\tsamples=2\tmerged=0\tcontexts=0,1,2\tn_union=3\n#chrom\tstart\tend\tcontext\tstrand\tnsamples\ta.nmeth\ta.nunmeth\tb.nmeth\tb.nunmeth\n"


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_parser_refusals(case, tmp_path):
    """every refusal through the API with the path, the line's number and the message; the next call is unharmed"""
    import methyldackel_amd as mdk
    _, lines, want, lineno = case
    p = tmp_path / "bad.tsv"
    p.write_bytes(HEAD + b"\n".join(lines) + b"\n")
    with pytest.raises(mdk.MdkError, match=re.escape(f"{p}, line {lineno}: {rule.MESSAGES[want]}")) as e:
        mdk.Cohort.read(p, ["chr1", "chr2"])
    assert e.value.rc == -3
    assert same(mdk.Cohort.read(_file(HAND_COHORT.encode()), HAND["contigs"]), cohort_of(HAND))


def test_rows_out_of_order_across_a_piece_boundary(tmp_path):
    import methyldackel_amd as mdk
    rows = [b"chr1\t9\t11\tCHG\t.\t1\t0\t0\t7\t8\n", b"chr1\t5\t6\tCG\t+\t2\t1\t2\t3\t4\n", b"chr2\t1\t2\tCHH\t-\t0\t0\t0\t0\t0\n"]
    p = tmp_path / "o.tsv"
    p.write_bytes(HEAD + b"".join(rows))
    for block_bytes in (None, len(HEAD) + len(rows[0]) + 5):             # the second row in the first piece, and as the first of the second
        with pytest.raises(mdk.MdkError, match=re.escape(f"{p}, line 4: {rule.MESSAGES['order']}")):
            mdk.Cohort.read(p, ["chr1", "chr2"], block_bytes=block_bytes)
    z = tmp_path / "o.tsv.gz"
    z.write_bytes(bytes(mdk.bgzf_compress(_cuda_bytes(HEAD + b"".join(rows))).cpu().numpy()))
    with pytest.raises(mdk.MdkError, match=re.escape(f"{z}, line 4: {rule.MESSAGES['order']}")):
        mdk.Cohort.read(z, ["chr1", "chr2"])
    good = z.read_bytes()
    for at, what in ((-36, "CRC32"), (-32, None)):          # the data member's trailer, in front of the 28-byte EOF member
        bad = bytearray(good); bad[at] ^= 1
        z.write_bytes(bytes(bad))
        with pytest.raises(mdk.MdkError, match=what):
            mdk.Cohort.read(z, ["chr1", "chr2"])
    z.write_bytes(good[:-40])
    with pytest.raises(mdk.MdkError, match="cut short"):
        mdk.Cohort.read(z, ["chr1", "chr2"])
    g = tmp_path / "g.tsv.gz"
    g.write_bytes(gzip.compress(HEAD + b"".join(rows)))
    with pytest.raises(mdk.MdkError, match="not BGZF"):
        mdk.Cohort.read(g, ["chr1", "chr2"])


def _cuda_bytes(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def test_write_refusals_leave_no_file(tmp_path):
    """each refusal names the site (and the sample), is rc -3, and no file is opened"""
    import methyldackel_amd as mdk
    base = rule.shared_table(70, 3)
    c0, a, b, x, s, k = base["sites"][66]

    def changed(site=None, counts=()):
        t = dict(base, sites=list(base["sites"]), m=[list(v) for v in base["m"]], u=[list(v) for v in base["u"]])
        if site:
            t["sites"][66] = site
        for w, j, i in counts:
            t[w][j][i] = -1
        return t
    cases = [changed((c0, -1, b, x, s, k)), changed((-1, a, b, x, s, k)), changed((3, a, b, x, s, k)), changed((c0, a, a, x, s, k)), changed((c0, a, b, 3, s, k)),
             changed(counts=[("u", 2, 66)]), changed(counts=[("m", 1, 5), ("m", 2, 5), ("u", 0, 69)]), changed((c0, a, a, 3, s, k), counts=[("m", 0, 66), ("u", 1, 3)])]
    for t in cases:
        what, site, sample = rule.write_refusal(t)
        where = f"(site {site}, sample {sample})" if sample is not None else f"(site {site})"
        for fmt in FORMATS:
            with pytest.raises(mdk.MdkError, match=re.escape(f"{rule.WRITE_MESSAGES[what]} {where}")) as e:
                cohort_of(t).write(tmp_path / "no.tsv", fmt, compress=fmt == "cohort")
            assert e.value.rc == -3 and not (tmp_path / "no.tsv").exists()
    # rows need not ascend to be written
    t = rule.shared_table(70, 3)
    back = dict(t, sites=t["sites"][::-1], m=[v[::-1] for v in t["m"]], u=[v[::-1] for v in t["u"]])
    assert text_of(cohort_of(back).render()) == rule.render("cohort", back)


def test_tabix_index_takes_the_file(tmp_path):
    """a 3-sample .gz is a BED-like BGZF file to mdk.tabix_index as it is"""
    import methyldackel_amd as mdk
    t = rule.shared_table(3, 3)
    path = cohort_of(t).write(tmp_path / "c.tsv.gz", compress=True)
    assert mdk.tabix_index(path) == str(path) + ".tbi"
    assert gzip.decompress((tmp_path / "c.tsv.gz.tbi").read_bytes())[:4] == b"TBI\x01"


def test_unite_write_read_diff(tmp_path):
    """unite -> write -> read -> diff gives the Diff bits of diff on the original"""
    import random
    import torch
    import methyldackel_amd as mdk
    rng = random.Random(5)
    contigs, samples = ["chr1", "chr2"], []
    sites = [(c, 10 * i + 3, rng.randrange(3), rng.choice((1, -1))) for c in (0, 1) for i in range(150)]
    for _ in range(4):
        rows = [(c, x, x + 1, rng.randrange(40), rng.randrange(40), ctx, s) for c, x, ctx, s in sites if rng.random() < 0.9]
        cols = {name: torch.tensor([r[k] for r in rows], dtype=getattr(torch, dt)).cuda() for k, (name, dt) in enumerate(mdk.CALL_COLUMNS)}
        samples.append(mdk.Calls(contigs, cols))
    co = mdk.unite(samples, min_samples=2)
    assert co.names is None
    back = mdk.Cohort.read(co.write(tmp_path / "u.tsv.gz", names=["a1", "a2", "b1", "b2"], compress=True), contigs)
    assert back.names == ("a1", "a2", "b1", "b2") and back.n_union == co.n_union and same(back, mdk.Cohort(co.contigs, {k: getattr(co, k) for k, _ in rule.SITE_COLUMNS},
                                                                                                       co.nmeth, co.nunmeth, co.merged, co.contexts_on, co.n_union, names=back.names))
    d0, d1 = co.diff([0, 1], [2, 3]), back.diff([0, 1], [2, 3])
    for name, _ in mdk.DIFF_SITE_COLUMNS + mdk.DIFF_RESULT_COLUMNS:
        a, b = getattr(d0, name), getattr(d1, name)
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b), name
