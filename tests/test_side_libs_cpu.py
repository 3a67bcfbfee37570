"""CPU: what the five side libraries -- libmdk_index/stats/smooth/cohort/track.so, one .hip file and one code object each, loaded at the
first call that needs them -- have in common, as far as it goes without a device: lib_X() binds what include/mdk_X.h declares and
nothing else, a library that was not built is named with what builds it, and a library loads without a device with no error text."""
import re
import threading

import pytest

from conftest import REPO

NOUNS = {"index": "index", "stats": "statistics", "smooth": "smoothing", "cohort": "cohort text", "track": "track"}
LIBS = list(NOUNS)


def fresh(mdk, monkeypatch, name):
    """lib_<name>() with its cache emptied: a CDLL that holds what this load bound, and no more"""
    monkeypatch.setattr(mdk, f"_{name}", None)
    return getattr(mdk, f"lib_{name}")()


@pytest.mark.parametrize("name", LIBS)
def test_the_loader_binds_what_the_header_declares(monkeypatch, name):
    import methyldackel_amd as mdk
    header = (REPO / "include" / f"mdk_{name}.h").read_text()
    declared = set(re.findall(rf"\b(md_{name}_\w+)\s*\(", header))
    assert {f"md_{name}_open", f"md_{name}_close", f"md_{name}_last_error"} < declared
    L = fresh(mdk, monkeypatch, name)
    bound = {f for f in vars(L) if f.startswith("md_")}
    assert bound == declared, bound ^ declared
    # every function that returns a code takes arguments, as many as its declaration
    for f in declared - {f"md_{name}_last_error"}:
        decl = re.search(rf"\b{f}\s*\((.*?)\);", header, re.S).group(1)
        assert len(getattr(L, f).argtypes) == len(decl.split(",")), f


@pytest.mark.parametrize("name", LIBS)
def test_a_missing_library_names_make(tmp_path, monkeypatch, name):
    import methyldackel_amd as mdk
    missing = tmp_path / f"libmdk_{name}.so"
    monkeypatch.setattr(mdk, f"_{name}", None)
    monkeypatch.setattr(mdk, f"LIB_{name.upper()}", missing)
    with pytest.raises(mdk.MdkError) as e:
        getattr(mdk, f"lib_{name}")()
    assert str(e.value) == f"{missing} is missing: the {NOUNS[name]} library was not built (run `make` / __graft_entry__.build()); there is no fallback"
    assert getattr(mdk, f"_{name}") is None                        # and nothing was kept


@pytest.mark.parametrize("name", LIBS)
def test_a_library_loads_without_a_device_and_a_fresh_thread_has_no_error(monkeypatch, name):
    import methyldackel_amd as mdk
    L = fresh(mdk, monkeypatch, name)
    got = []
    t = threading.Thread(target=lambda: got.append(getattr(L, f"md_{name}_last_error")()))
    t.start(); t.join()
    assert got == [b""]
    assert getattr(mdk, f"lib_{name}")() is L                      # kept: the second call loads nothing
