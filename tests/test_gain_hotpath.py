"""Which launches' gain statistics reach the run's rows (core/hotpath.py), on the host: the asynchronous schedules attach a
launch's table to its buffers (``HotPath._filtered``) and ``finish_sampled`` decides, per launch, whether it is kept - kept with the
launch's points, dropped with them.  A reference whose selection is refused (upstream's ordinary "no candidates" error, raised by
``collect``) must not cost the references behind it their statistics, with ``min_support_views`` off as well as on; a chained call that is
void as a whole, and a call whose statistics the caller cleared because it drops the result, leave nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import colour_scene as cs
import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd.core import hip_backend as hb
from lichtfeld_densification_plugin_amd.core.hotpath import HotPath

MATCH, H, W, K = 96, 12, 16, 3
REFS = (5, 13, 21, 29)


@pytest.fixture(scope="module")
def scenes():
    return [cs.make(r, K, H, W, match=MATCH, noise_px=0.6, gains=(1.0, 0.9, 1.1, 1.0)) for r in REFS]


def hot_for(min_support):
    exp = {"gain_compensation": "luma"}
    if min_support:
        exp["min_support_views"] = min_support
    cfg = lfd.DensePipelineConfig(output_path="a.ply", backend="host", experimental=exp)
    return HotPath(cs.cameras(), cfg, 1.0, MATCH, MATCH, torch.device("cpu"), None)


def launch(hot, scene):
    """What launch_sampled does behind its kernel, with the twin's dense points in the buffers: the stages of ``_filtered``, the gain
    statistics among them, attached to the buffers that ``finish_sampled`` will collect."""
    batch = hb.PreparedBatch([scene.inputs], MATCH, MATCH)
    out = hot._take_buffers(H * W, 1, K)
    assert hot.dens._lib.lfd_triangulate_dense_host(hot.dens._ctx, C.byref(batch.c), C.byref(cs.params()), C.byref(out.c), out.ref_offsets.data_ptr(),
                                                    out.seg_counts.data_ptr()) == 0
    out = hot._filtered(batch, out)
    assert out.gain_pending is not None
    return batch, out


def refuse(handle):
    """The handle of a reference whose selection is refused: ``collect`` raises upstream's error."""
    def collect(*a, **kw):
        del handle[1].collect                    # (the buffers are recycled: the next launch that takes them collects as usual)
        raise ValueError("a must be non-empty")
    handle[1].collect = collect
    return handle


def uids(rows):
    return sorted(set(int(u) for u in rows.ref_uid))


@pytest.mark.parametrize("min_support", [0, 1])
def test_a_refused_reference_does_not_cost_the_later_ones_their_statistics(scenes, min_support):
    hot = hot_for(min_support)
    try:
        cams = cs.cameras()
        first = hot.finish_sampled(launch(hot, scenes[0]))
        assert first is not None and first.count > 100
        # two references in flight; the older one is refused, the one launched behind it is fine and its points are kept
        bad, good = refuse(launch(hot, scenes[1])), launch(hot, scenes[2])
        with pytest.raises(ValueError, match="non-empty"):
            hot.finish_sampled(bad)
        kept = hot.finish_sampled(good)
        last = hot.finish_sampled(launch(hot, scenes[3]))
        assert kept is not None and kept.count > 100 and last is not None and last.count > 100
        rows = hot.gain_rows()
        assert uids(rows) == sorted(int(cams[r].uid) for r in (REFS[0], REFS[2], REFS[3]))          # the refused reference alone is missing
        assert rows.table.shape == (3 * K, 7) and rows.table.dtype == np.uint64 and (rows.table[:, 0] > 0).all()
        for sc in (scenes[0], scenes[2], scenes[3]):                                              # every row names its own pair
            mine = rows.ref_uid == int(cams[sc.ref].uid)
            assert rows.nbr_uid[mine].tolist() == [int(cams[n].uid) for n in sc.nbrs]
    finally:
        hot.close()


def test_a_void_chain_and_a_discarded_call_leave_nothing(scenes):
    hot = hot_for(0)
    try:
        handle = launch(hot, scenes[0])
        plain = handle[1].collect

        def void(*a, **kw):
            del handle[1].collect                # (the buffers are recycled: the next launch that takes them collects as usual)
            res = plain(*a, **kw)
            res.sel_status[0] = sorted(hb.SELECT_VOIDS_STREAM)[0]
            return res
        handle[1].collect = void
        assert hot.finish_sampled(handle, check_selection=False) is not None                      # (the caller reads the status and redoes it)
        assert hot.gain_rows().table.shape[0] == 0
        behind = launch(hot, scenes[1])
        behind[1].gain_pending = None                                                             # launched behind a failed call: SampledLoop._recover
        hot.finish_sampled(behind, check_selection=False)                                         # drops its statistics with its results
        assert hot.gain_rows().table.shape[0] == 0
        hot.finish_sampled(launch(hot, scenes[2]), check_selection=False)                         # the redone reference: kept
        assert uids(hot.gain_rows()) == [int(cs.cameras()[REFS[2]].uid)]
    finally:
        hot.close()
