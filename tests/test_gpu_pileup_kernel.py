"""GPU: the pileup and mbias kernels (csrc/mdk_hip.hip k_pileup, k_pileup_multi, k_mbias, with k_classify and k_mask_regions) on
hand-built segment batches (tests/batchgen.py), against the slow evaluator (tests/batch_eval.py).  Every batch goes through the
public C ABI (md_dev_submit / md_dev_launch_group / md_dev_mbias_submit); none comes from the product's chunk preparation.

Every case runs on the three kernels -- CpG only (a lane per segment), all contexts (a quarter of a wavefront per segment), all
contexts with MDK_NO_QW (a lane per segment over dense lists) -- with minOppositeDepth 0 and 1 and at tiles 512 and 2048; the list,
edge and fuzz cases at 1024 and 1536 too.  Bar: the whole dictionary of sites equal to the evaluator's."""
import ctypes as C
import os
import random

import pytest

import methyldackel_amd as mdk
import batchgen as bg

pytestmark = pytest.mark.gpu

KERNELS = {"cpg": ((1, 0, 0), False), "qw": ((1, 1, 1), False), "lane_dense": ((1, 1, 1), True),
           "qw_chg": ((0, 1, 0), False), "qw_chh": ((0, 0, 1), False)}
MAIN_KERNELS = ("cpg", "qw", "lane_dense")


class Dev:
    """one md_dev per (kernel, minOppositeDepth, tile), shared by the cases; what a case sets of the cfg (minPhred, bounds) goes in
    through md_dev_reset, which keeps the handle, its slots and its streams"""

    def __init__(self, kernel, mod, tile, n_slots=2, keep=None):
        self.kernel, self.mod, self.tile, self.n_slots = kernel, mod, tile, n_slots
        self.keep, self.noqw = KERNELS[kernel] if keep is None else (keep, False)
        self.fields = {}
        self._env(lambda: setattr(self, "dev", mdk.Device(bg.make_cfg({}, self.keep, mod, tile, n_slots))))
        assert mdk.lib_hip().md_dev_tile(self.dev.h) == tile

    def _env(self, fn):
        if self.noqw:
            os.environ["MDK_NO_QW"] = "1"
        try:
            return fn()
        finally:
            os.environ.pop("MDK_NO_QW", None)

    def use(self, fields, ref, regions=None, tid=0):
        f = {k: fields[k] for k in ("minPhred", "bounds", "absoluteBounds") if k in fields}
        if f != self.fields:
            cfg = bg.make_cfg(f, self.keep, self.mod, self.tile, self.n_slots)
            rc = self._env(lambda: self.dev.L.md_dev_reset(self.dev.h, C.byref(cfg)))
            stop_on_hip_error(rc, "md_dev_reset")
            assert rc == 0, self.dev.L.md_dev_last_error()
            self.fields = f
        stop_on_hip_error(self.dev.L.md_dev_set_reference(self.dev.h, tid, ref, len(ref)), "md_dev_set_reference")
        if regions is not None:
            self.dev.set_regions(tid, regions)

    def __str__(self):
        return f"kernel {self.kernel} minOppositeDepth {self.mod} tile {self.tile}"


def applies(name, kernel, mod):
    fields = bg.build(name)[1]
    if mod not in fields.get("mod", (0, 1)):
        return False
    return kernel in MAIN_KERNELS or KERNELS[kernel][0] in fields.get("keeps", ())


CONFIGS = [(k, mod, tile) for k in KERNELS for mod in (0, 1) for tile in bg.TILES if k in MAIN_KERNELS or tile in (512, 2048)]
PAIRS = [(c, name) for c in CONFIGS for name, _ in bg.CASES if c[2] in bg.tiles_for(name) and applies(name, c[0], c[1])]


@pytest.fixture(scope="module")
def dev(request):
    d = Dev(*request.param)
    yield d
    d.dev.close()


def stop_on_hip_error(rc, what):
    """a failed HIP call leaves the process's device context unusable: nothing more is started on it"""
    if rc == -1:
        pytest.exit(f"{what}: HIP error ({mdk.lib_hip().md_dev_last_error().decode()}); the session ends here", returncode=3)


def compare(d, name, got, want):
    stop_on_hip_error(got, f"case {name}, {d}")
    assert got == want, f"case {name}, {d}: {bg.first_difference(got, want)}"


@pytest.mark.parametrize("dev,name", PAIRS, indirect=["dev"], ids=[f"{c[0]}-mod{c[1]}-tile{c[2]}-{n}" for c, n in PAIRS])
def test_case_equals_evaluator(dev, name):
    ref, fields, regions, batch, _ = bg.build(name)
    dev.use(fields, ref, regions)
    want = bg.expected(name, dev.keep, dev.mod)
    compare(dev, name, bg.device_sites(dev.dev, 0, batch), want)
    if want == bg.ERR_STRAND0:
        # the error is the launch's, not the slot's: the next clean submit on the same slot answers 0 and the right sites
        ref, fields, regions, batch, _ = bg.build("strand0_over_c")
        dev.use(fields, ref, regions)
        compare(dev, "strand0_over_c after " + name, bg.device_sites(dev.dev, 0, batch), bg.expected("strand0_over_c", dev.keep, dev.mod))


GROUP_TILES = (0, 1, 1, 2, 3, 7, 8, 9)


def group_batches(tile):
    """eight intervals of 0, 1, 1, 2, 3, 7, 8 and 9 tiles, each on a contig of its own, over one set of reads (what lies outside an
    interval is dropped by the library), built as the list, edge and partner cases are"""
    rng = random.Random(500 + tile)
    n = 9 * tile + 200
    refs = [bg.rand_ref(random.Random(600 + k), n, (0.05, 0.5, 1.0)[k % 3], letters="ATatNn", cg="CGCGcg") for k in range(8)]
    B = bg.Builder()
    bg.sprinkle(B, rng, refs[1], 100 + 12 * 9 * tile // 512, 20, 150, partner_frac=0.4)
    rng.shuffle(B.segs)
    out = []
    for k, nt in enumerate(GROUP_TILES):
        beg = 3 + 11 * k
        end = beg if nt == 0 else beg + (nt - 1) * tile + (tile if k % 2 else 1 + 37 * k)
        out.append((refs[k], B.batch(k, beg, end)))
    return out


_group = {}


@pytest.mark.parametrize("tile", (512, 2048))
@pytest.mark.parametrize("mod", (0, 1))
@pytest.mark.parametrize("kernel", MAIN_KERNELS)
def test_group_launch_equals_evaluator(kernel, mod, tile):
    """k_pileup_multi: eight slots of 0 to 9 tiles launched as groups of 8, 3 and 1; every slot equals the evaluator (the XCD dealing of
    the tiles of all slots together must give each slot its own tiles, parameters and site counter)"""
    d = Dev(kernel, mod, tile, n_slots=8)
    try:
        if (tile, d.keep) not in _group:
            batches = group_batches(tile)
            _group[(tile, d.keep)] = batches, [bg.expected_sites(ref, {}, None, b, d.keep, 1) for ref, b in batches]
        batches, want = _group[(tile, d.keep)]
        want = [bg.without_opposite(w, mod) for w in want]
        for k, (ref, b) in enumerate(batches):
            assert (b.end - b.beg + tile - 1) // tile == GROUP_TILES[k]
            d.dev.set_reference(k, ref)
        assert sum(len(w) for w in want) > 500
        for group in ([0, 1, 2, 3, 4, 5, 6, 7], [7, 3, 5], [2]):
            for k in group:
                d.dev.upload(k, batches[k][1])
            d.dev.launch_group(group)
            for k in group:
                s = mdk.md_sites()
                rc = d.dev.L.md_dev_download(d.dev.h, k, C.byref(s))
                stop_on_hip_error(rc, f"group {group} slot {k}, {d}")
                assert rc == 0, (group, k, rc)
                compare(d, f"group {group} slot {k}", bg.sites_dict(s, batches[k][1].beg, batches[k][1].end), want[k])
    finally:
        d.dev.close()


MBIAS_KEEPS = {"cpg": (1, 0, 0), "chg": (0, 1, 0), "chh": (0, 0, 1), "all": (1, 1, 1)}
MBIAS_PAIRS = [((k, tile), name) for k in MBIAS_KEEPS for tile in (512, 2048) for name, _ in bg.MBIAS_CASES
               if k in ("cpg", "all") or MBIAS_KEEPS[k] in bg.build_mbias(name)[1].get("keeps", ())]


@pytest.fixture(scope="module")
def mdev(request):
    k, tile = request.param
    d = Dev("mbias", 0, tile, keep=MBIAS_KEEPS[k])
    yield d
    d.dev.close()


@pytest.mark.parametrize("mdev,name", MBIAS_PAIRS, indirect=["mdev"], ids=[f"{c[0]}-tile{c[1]}-{n}" for c, n in MBIAS_PAIRS])
def test_mbias_equals_evaluator(mdev, name):
    """k_mbias through md_dev_mbias_submit: the histogram equals eval_mbias, rows kept in LDS and rows past them alike"""
    mbias_once(mdev, name)
    if name == "mbias_strand0":             # reported once, and the handle works on
        mbias_once(mdev, "mbias_edges_a")


def mbias_once(mdev, name):
    ref, fields, _, batch, _ = bg.build_mbias(name)
    mdev.fields = None                      # md_dev_reset every time: it also drops the histogram of the case before
    mdev.use(fields, ref)
    want = bg.expected_mbias(name, mdev.keep)
    mdev.dev.mbias_submit(0, batch)
    got = bg.device_hist(mdev.dev)
    stop_on_hip_error(got, f"case {name}, keep {mdev.keep} tile {mdev.tile}")
    assert got == want, f"case {name}, keep {mdev.keep} tile {mdev.tile}: {bg.first_difference(got, want)}"
