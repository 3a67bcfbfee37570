"""The colliding read names of tests/name_hash.py, and the collision cases of tests/test_gpu_prep_cases.py built from them, checked without
a GPU: the literal pairs collide under the restated hash (the probe of test_gpu_prep_cases.py ties the restatement to the device), and
every collision case is SENSITIVE -- with the two colliding names replaced by one shared name, which is what the device would compute if
it took the two for one, the oracle's output differs.  A case for which it does not would prove nothing on the device."""
import pytest

import name_hash as nh
import test_gpu_prep_cases as cases
from conftest import run_oracle


def test_restated_hash_properties():
    """the name as strcmp sees it; 16-byte blocks, of which one with fewer than 16 letters is the last; never 0; length enters"""
    assert nh.name_hash("same") == nh.name_hash(b"same\0junk") != nh.name_hash("same\1")
    assert nh.name_hash("a" * 16) != nh.name_hash("a" * 16 + "\1") != nh.name_hash("a" * 17)
    assert nh.name_hash("") == (((nh.SEED ^ 0) * nh.MUL_LEN) & nh.M64) ^ ((((nh.SEED ^ 0) * nh.MUL_LEN) & nh.M64) >> 32)
    assert all(0 < nh.name_hash(f"r{k}") < 1 << 64 for k in range(1000))
    assert nh.table_key("x") == nh.name_hash("x") >> 32 and nh.home_slot("x", 4095) == nh.name_hash("x") & 4095


@pytest.mark.parametrize("a,b,ctl", nh.ALL_PAIRS, ids=[p[0] for p in nh.ALL_PAIRS])
def test_literal_pairs_collide_and_controls_do_not(a, b, ctl):
    assert nh.collide(a, b) and nh.table_key(a) == nh.table_key(b)
    for hmask in (1023, 2047, 4095):
        assert nh.home_slot(a, hmask) == nh.home_slot(b, hmask)
    assert nh.unrelated(a, ctl) and nh.unrelated(b, ctl)
    assert not nh.collide(a, ctl) and not nh.collide(b, ctl)


def test_pair_kinds():
    assert len(nh.SHORT_PAIRS) >= 6 and len(nh.TAIL_PAIRS) >= 2 and len(nh.LENGTH_PAIRS) >= 3
    assert len({n for p in nh.ALL_PAIRS for n in p}) == 3 * len(nh.ALL_PAIRS)
    for a, b, _ in nh.SHORT_PAIRS:
        assert len(a) <= 16 and len(b) <= 16
    for a, b, _ in nh.TAIL_PAIRS:
        assert len(a) == len(b) == 24 and a[:16] == b[:16] and a[16:] != b[16:]
    for a, b, _ in nh.LENGTH_PAIRS:
        assert a[:16] == b[:16] and len(a) != len(b) and min(len(a), len(b)) > 16
    assert {len(a) < len(b) for a, b, _ in nh.LENGTH_PAIRS} == {True, False}          # the longer name first, and second


def test_vectorised_hash_is_the_restatement():
    """what find_collisions hashes with (numpy, 64-bit wrap-around) against the Python integers"""
    for prefix, slen in ((b"rd", 8), (b"HWI-ST1234:C0ABC", 8), (b"A00123:45:HXYZ7:", 7), (b"0123456789abcde", 1), (b"", 3)):
        rows = nh._names(prefix, slen, 12345, 50)
        h = nh._hash_rows(rows, len(prefix) + slen)
        for k in range(50):
            assert int(h[k]) == nh.name_hash(bytes(rows[k, :len(prefix) + slen]))


def oracle_output(d, args):
    r = run_oracle(args + ["-o", "out"], cwd=d)
    assert r.returncode == 0, r.stderr
    return (d / "out_CpG.bedGraph").read_bytes()


# (every entry but the one in order A A B B: with A's two reads before B's two, one name or two pair the same reads -- that placement is
# there for the links across workgroups, and its sensitive form, "swept", stands beside it)
SENSITIVE = [(case, k) for case, entries in cases.COLLISION_CASES.items() for k in range(len(entries)) if entries[k][0] != "AABB"]


@pytest.mark.parametrize("case,k", SENSITIVE, ids=[f"{c}-{cases.COLLISION_CASES[c][k][0]}{k}" for c, k in SENSITIVE])
def test_collision_case_is_sensitive(tmp_path, case, k):
    """the same records with the k-th entry's two names made one: the oracle must count differently"""
    (tmp_path / "two").mkdir(), (tmp_path / "one").mkdir()
    args2, lay2 = cases.collision_bam(tmp_path / "two", case)
    args1, lay1 = cases.collision_bam(tmp_path / "one", case, merged=k)
    assert [r[1:] for r in lay1.recs] == [r[1:] for r in lay2.recs] and sum(a[0] != b[0] for a, b in zip(lay1.recs, lay2.recs)) in (1, 2)
    two, one = oracle_output(tmp_path / "two", args2 + cases.Q10), oracle_output(tmp_path / "one", args1 + cases.Q10)
    assert two.count(b"\n") > 20
    assert two != one, f"{case}[{k}]: the oracle counts the same whether or not the two names are one: the case proves nothing"
