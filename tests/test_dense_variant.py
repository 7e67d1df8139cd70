"""lfd_dense_variant (include/lfd_densify.h): the host predicate that decides whether lfd_triangulate_dense may launch the production-shape
instantiation of the fused kernel (lfd_dense_prod_kernel) - 1 - or launches the generic kernel - 0.  A pure function of the launch's arguments:
no context, no device.  The kernel it guards TESTS NONE of these conditions again, so every one of them must switch it off on its own.
(It never reads through the device pointers of the tables; the addresses below are made up.)"""
import ctypes as C

import pytest

import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd.core import hip_backend as hb


class Launch:
    """The arguments of one lfd_triangulate_dense call as ctypes structures; the defaults are the benchmark's headline shape."""

    def __init__(self, n_refs=64, k=3, H=512, W=512, channels=2, mask_a=None, mask_b=None, axes=False, with_cell=False, with_slot=False,
                 with_segments=False, n_slots=None, **config):
        vp = C.POINTER(C.c_void_p)
        self.n_slots = (C.c_int32 * n_refs)(*([k] * n_refs if n_slots is None else n_slots))
        self.ref_cam = (C.c_int32 * n_refs)()
        self.nbr_cam = (C.c_int32 * (n_refs * k))()
        self.cert = (C.c_void_p * (n_refs * k))(*[0x1000] * (n_refs * k))
        self.warp = (C.c_void_p * (n_refs * k))(*[0x2000] * (n_refs * k))
        self.image = (C.c_void_p * n_refs)(*[0x3000] * n_refs)
        self.mask_a = (C.c_void_p * n_refs)(*mask_a) if mask_a is not None else None
        self.mask_b = (C.c_void_p * (n_refs * k))(*mask_b) if mask_b is not None else None
        self.batch = hb.lfd_batch(
            n_refs=n_refs, k=k, H=H, W=W, w_match=512, h_match=512, warp_channels=channels, reserved=0, fundamental=None,
            ref_cam=C.cast(self.ref_cam, C.POINTER(C.c_int32)), n_slots=C.cast(self.n_slots, C.POINTER(C.c_int32)),
            nbr_cam=C.cast(self.nbr_cam, C.POINTER(C.c_int32)), cert=C.cast(self.cert, vp), warp=C.cast(self.warp, vp), image=C.cast(self.image, vp),
            mask_a=C.cast(self.mask_a, vp) if self.mask_a is not None else None, mask_b=C.cast(self.mask_b, vp) if self.mask_b is not None else None,
            axis_x=0x4000 if axes else None, axis_y=0x5000 if axes else None)
        exact = config.pop("exact_colour", False)
        self.params = hb.make_params(lfd.DensePipelineConfig(output_path="", nns_per_ref=k, **config), exact_colour=exact)
        self.out = hb.lfd_points(xyz=0x6000, rgb=0x7000, err=0x8000, cell=0x9000 if with_cell else None, slot=0xa000 if with_slot else None,
                                 capacity=n_refs * H * W)
        self.seg_counts = 0xb000 if with_segments else None

    def variant(self):
        return hb.dense_variant(self.batch, self.params, self.out, self.seg_counts)


def test_headline_shape_runs_the_production_kernel():
    assert Launch().variant() == 1
    assert Launch(n_refs=2, H=4, W=256).variant() == 1                  # one tile per reference
    assert Launch(n_refs=1, k=1, H=4, W=512).variant() == 1
    assert Launch(k=4, n_slots=[4] * 63 + [2]).variant() == 1           # a ragged reference is no violation


def test_null_tables_of_masks_are_no_masks():
    assert Launch(n_refs=2, mask_a=[0, 0], mask_b=[0] * 6).variant() == 1
    # a mask on a slot beyond the reference's n_slots is never uploaded (and never read)
    assert Launch(n_refs=2, n_slots=[3, 2], mask_b=[0, 0, 0, 0, 0, 0xc000]).variant() == 1


# one case per row of the table the production kernel assumes (and per single condition inside a row)
VIOLATIONS = {
    "grid_not_whole_tiles": dict(H=6, W=256),
    "grid_of_half_a_tile": dict(H=2, W=256),
    "width_not_a_multiple_of_4": dict(H=1024, W=5),
    "mask_a_on_one_reference": dict(n_refs=2, mask_a=[0, 0xc000]),
    "mask_b_on_one_slot": dict(n_refs=2, mask_b=[0, 0, 0, 0, 0xc000, 0]),
    "certainty_floor_of_zero": dict(certainty_thresh=0.0),
    "negative_certainty_floor": dict(certainty_thresh=-1.0),
    "four_channel_warps": dict(channels=4),
    "explicit_axes": dict(axes=True),
    "exact_colour": dict(exact_colour=True),
    "no_filter": dict(no_filter=True),
    "sampson_gate_off": dict(sampson_thresh=0.0),
    "parallax_gate_off": dict(min_parallax_deg=0.0),
    "seg_counts": dict(with_segments=True),
    "cell_output": dict(with_cell=True),
    "slot_output": dict(with_slot=True),
}


@pytest.mark.parametrize("name", list(VIOLATIONS))
def test_a_single_violation_selects_the_generic_kernel(name):
    assert Launch(**VIOLATIONS[name]).variant() == 0


def test_nan_thresholds_and_null_arguments_select_the_generic_kernel():
    lib = hb.load_library()
    a = Launch()
    assert lib.lfd_dense_variant(None, C.byref(a.params), C.byref(a.out), None) == 0
    assert lib.lfd_dense_variant(C.byref(a.batch), None, C.byref(a.out), None) == 0
    assert lib.lfd_dense_variant(C.byref(a.batch), C.byref(a.params), None, None) == 0
    for field in ("certainty_thresh", "sampson_thresh", "min_parallax_deg"):
        b = Launch()
        setattr(b.params, field, float("nan"))
        assert b.variant() == 0, field
