"""GPU: the one table of handles under the side libraries (methyldackel_amd._side_handles): a small table goes through libmdk_smooth,
libmdk_stats, libmdk_cohort and libmdk_track twice and once more from another thread; every result is the first one's, and each
library has one handle on device 0 throughout.  What the kernels compute is test_gpu_smooth / _qdiff / _cohort_io / _track's."""
import threading

import pytest

pytestmark = pytest.mark.gpu
N = 65                                                              # a wavefront's 64 sites and one more
HANDLED = ("stats", "smooth", "cohort", "track")


def table():
    """65 sites of one contig, 2 samples, every site covered in both"""
    import torch
    import methyldackel_amd as mdk
    i = torch.arange(N, dtype=torch.int32)
    cols = {"contig": torch.zeros(N, dtype=torch.int32), "start": 10 * i, "end": 10 * i + 1, "context": torch.zeros(N, dtype=torch.uint8),
            "strand": torch.ones(N, dtype=torch.int8), "nsamples": torch.full((N,), 2, dtype=torch.int32)}
    m = torch.stack([1 + i % 7, 2 + i % 5]).to(torch.int32)
    u = torch.stack([3 + i % 4, 1 + i % 9]).to(torch.int32)
    return mdk.Cohort(["chr1"], {k: v.cuda() for k, v in cols.items()}, m.cuda().contiguous(), u.cuda().contiguous())


def results(co):
    import methyldackel_amd as mdk
    out = list(mdk.smooth_counts(co.contig, co.start, co.nmeth, co.nunmeth, 100, 5)) + list(mdk.diff_replicates(co.nmeth, co.nunmeth, [0], [1]))
    out += [co.render(), co.sample(0).render_bigwig([1000])]
    return [t.cpu() for t in out]


def handles(mdk):
    """library -> the address of its handle on device 0"""
    return {name: h.value for (name, device), h in mdk._side_handles.items() if device == 0}


def test_two_calls_and_a_second_thread_share_one_handle_per_library():
    import torch
    import methyldackel_amd as mdk
    co = table()
    first = results(co)
    mine = handles(mdk)
    assert sorted(mine) == sorted(HANDLED) and all(mine.values())
    assert all(t.numel() for t in first) and not any(torch.isnan(t).any() for t in first[:2])
    second = results(co)
    assert len(second) == len(first) and all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(first, second))
    assert handles(mdk) == mine
    got = []
    t = threading.Thread(target=lambda: got.append(results(co)))
    t.start(); t.join()
    assert len(got) == 1 and all(torch.equal(a, b) for a, b in zip(first, got[0]))
    assert handles(mdk) == mine                                     # the other thread opened none of its own
