"""ctypes binding of the C-ABI in ``include/lfd_densify.h`` (the HIP library is the only backend).

Torch is used for what it is good at here - owning device memory and streams; every tensor is
handed to the library as a raw device pointer.  If ``liblfd_densify.so`` is missing or no GPU is
present the constructors raise: there is deliberately no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import threading
import dataclasses
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .types import CameraRecord, DensePipelineConfig

LFD_MAX_SLOTS = 16
LFD_ABI_VERSION = 9
LFD_CONSENSUS_CAP = 8        # lfd_consensus_filter: min_refs is in 1 .. this, and the counts stop there
LFD_FLAG_EXACT_COLOUR = 1     # lfd_params.flags: dense mode blends colours with upstream's f64 arithmetic (bit-identical rgb)
LFD_FLAG_TILE_SEGMENTS = 2    # informational: the caller takes the unordered-retirement route (lfd_triangulate_dense_segments)
_LIB_NAME = "liblfd_densify.so"
_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class HipBackendError(RuntimeError):
    """Raised for any non-zero status of the HIP library (message from ``lfd_last_error``)."""


class SelectionInexact(HipBackendError):
    """The device selection met a normalised weight below 2^-29 (LFD_SELECT_INEXACT): its exact parallel cumulative sum
    is not guaranteed for such input, so it refused - WITHOUT consuming the MT19937 stream.  The caller runs the host
    stage (core/sampling.py) on the same map with the device's stream state instead (core/pipeline.py does)."""


class VoxelInputRefused(HipBackendError):
    """lfd_voxel_downsample refused its input - a non-finite coordinate, or a linear voxel key beyond 63 bits - before sorting anything.
    The caller filters on the host instead (densify.dense_init_from_lfs does)."""


class ConsensusInputRefused(HipBackendError):
    """lfd_consensus_filter refused the cloud for its key range - so wide for the radius that an axis has more than 2^30 cells or the linear
    cell key leaves 63 bits - before sorting anything.  Nothing stands in for it: the caller reports the radius (densify.py does)."""


class FuseInputRefused(HipBackendError):
    """lfd_fuse_oriented refused its input - a non-finite coordinate, or a linear voxel key beyond 63 bits - before sorting anything.  Nothing
    stands in for it: the caller reports the voxel size (densify.py does)."""


class KnnInputRefused(HipBackendError):
    """lfd_knn_dist2 refused the cloud - fewer than four points, a non-finite coordinate, or a cell key range beyond the grid's limits - before
    sorting anything.  Nothing was written."""


class CapInputRefused(HipBackendError):
    """lfd_cap_spatial refused the cloud - a non-finite coordinate - before sorting anything.  Nothing stands in for it: the caller reports the
    knob (densify.py does)."""


class ThinInputRefused(HipBackendError):
    """lfd_thin_footprint refused the cloud - a non-finite coordinate - before sorting anything.  Nothing stands in for it: the caller reports the
    knob (densify.py does)."""


class lfd_params(C.Structure):
    _fields_ = [("sampson_thresh", C.c_double), ("certainty_thresh", C.c_float), ("sample_cap", C.c_float),
                ("reproj_thresh", C.c_float), ("min_parallax_deg", C.c_float), ("no_filter", C.c_int32),
                ("flags", C.c_int32)]


class lfd_batch(C.Structure):
    _fields_ = [("n_refs", C.c_int32), ("k", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("w_match", C.c_int32), ("h_match", C.c_int32), ("warp_channels", C.c_int32), ("reserved", C.c_int32),
                ("ref_cam", C.POINTER(C.c_int32)), ("n_slots", C.POINTER(C.c_int32)), ("nbr_cam", C.POINTER(C.c_int32)),
                ("cert", C.POINTER(C.c_void_p)), ("warp", C.POINTER(C.c_void_p)), ("image", C.POINTER(C.c_void_p)),
                ("mask_a", C.POINTER(C.c_void_p)), ("mask_b", C.POINTER(C.c_void_p)),
                ("axis_x", C.c_void_p), ("axis_y", C.c_void_p), ("fundamental", C.POINTER(C.c_float))]


class lfd_points(C.Structure):
    _fields_ = [("xyz", C.c_void_p), ("rgb", C.c_void_p), ("err", C.c_void_p), ("cell", C.c_void_p),
                ("slot", C.c_void_p), ("capacity", C.c_int64)]


class lfd_tile_segment(C.Structure):
    """one row of the tile table of lfd_triangulate_dense_segments (handled as an (n, 2) int32 tensor on this side)"""
    _fields_ = [("offset", C.c_int32), ("count", C.c_int32)]


class lfd_copy_segment(C.Structure):
    """one copy of lfd_copy_segments (handled as an (n, 3) int64 array on this side)"""
    _fields_ = [("src_offset", C.c_int64), ("dst_offset", C.c_int64), ("nbytes", C.c_int64)]


ABI_STRUCTS = (lfd_params, lfd_batch, lfd_points, lfd_tile_segment, lfd_copy_segment)     # the order lfd_struct_layout reports them in


def check_struct_layout(lib, structs=ABI_STRUCTS) -> None:
    """The ctypes mirrors above against what the COMPILER made of include/lfd_densify.h (lfd_struct_layout: sizeof, field count and every
    field's offset and size per structure; lfd_struct_fields: their names): a field added, dropped, reordered or retyped on one side only is an import error here, not a corrupted
    launch later."""
    lib.lfd_struct_layout.argtypes = [C.POINTER(C.c_int32), C.c_int32]
    lib.lfd_struct_layout.restype = C.c_int
    n = int(lib.lfd_struct_layout(None, 0))
    table = (C.c_int32 * n)()
    lib.lfd_struct_layout(table, n)
    lib.lfd_struct_fields.restype = C.c_char_p
    names = dict(part.split(":") for part in lib.lfd_struct_fields().decode().split(";"))
    vals, at = list(table), 0
    for cls in structs:
        theirs = names.get(cls.__name__, "").split(",")
        if [name for name, *_ in cls._fields_] != theirs:
            raise HipBackendError(f"ctypes mirror of {cls.__name__} lists the fields {[name for name, *_ in cls._fields_]}, the library's header has "
                                  f"{theirs} (include/lfd_densify.h and core/hip_backend.py disagree)")
        if at + 2 > len(vals):
            raise HipBackendError(f"lfd_struct_layout ends before {cls.__name__}: the library is older than this binding")
        size, n_fields = vals[at], vals[at + 1]
        offsets = list(zip(vals[at + 2:at + 2 + 2 * n_fields:2], vals[at + 3:at + 2 + 2 * n_fields:2]))       # (offset, size) per field
        at += 2 + 2 * n_fields
        mine = [(name, getattr(cls, name).offset, getattr(cls, name).size) for name, *_ in cls._fields_]
        if C.sizeof(cls) != size or [(o, z) for _n, o, z in mine] != offsets:
            raise HipBackendError(f"ctypes mirror of {cls.__name__} does not match the library's layout: here sizeof {C.sizeof(cls)} with offsets "
                                  f"(name, offset, size) {mine}, the library has sizeof {size} with (offset, size) {offsets} (include/lfd_densify.h and core/hip_backend.py disagree)")
    if at != len(vals):
        raise HipBackendError("lfd_struct_layout reports structures this binding does not mirror")


_lib = None


def library_path() -> str:
    """In-tree library; ``LFD_DENSIFY_LIB`` overrides it (used to A/B kernel builds while profiling)."""
    return os.environ.get("LFD_DENSIFY_LIB") or os.path.join(_PKG_DIR, _LIB_NAME)


def load_library() -> C.CDLL:
    """dlopen the in-tree HIP library and declare its prototypes (works without a GPU: the host
    helpers and symbol table are usable, every compute entry point then returns LFD_ERR_HIP)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise HipBackendError(
            f"{path} not found: build it with `python {os.path.join(_PKG_DIR, 'csrc', 'build.py')}` "
            "(hipcc, --offload-arch=gfx950). There is no CPU fallback for the dense-initialisation path.")
    lib = C.CDLL(path)
    ctxp = C.c_void_p
    lib.lfd_abi_version.restype = C.c_int
    if int(lib.lfd_abi_version()) != LFD_ABI_VERSION:
        raise HipBackendError(f"{path} implements ABI {int(lib.lfd_abi_version())}, this binding ABI {LFD_ABI_VERSION}: rebuild the library "
                              f"(python {os.path.join(_PKG_DIR, 'csrc', 'build.py')})")
    check_struct_layout(lib)
    lib.lfd_create.argtypes = [C.c_int, C.c_void_p, C.POINTER(ctxp)]
    lib.lfd_destroy.argtypes = [ctxp]
    lib.lfd_destroy.restype = None
    lib.lfd_set_stream.argtypes = [ctxp, C.c_void_p]
    lib.lfd_reload_env.argtypes = [ctxp]
    lib.lfd_kernel_timing.argtypes = [ctxp, C.c_int32]
    lib.lfd_kernel_timing_read.argtypes = [ctxp, C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_int32)]
    lib.lfd_last_error.argtypes = [ctxp]
    lib.lfd_last_error.restype = C.c_char_p
    fptr = C.POINTER(C.c_float)
    lib.lfd_upload_cameras.argtypes = [ctxp, C.c_int32, fptr, fptr, fptr, fptr, fptr, C.POINTER(C.c_int32)]
    lib.lfd_prepare_batch.argtypes = [ctxp, C.POINTER(lfd_batch), C.POINTER(lfd_params)]
    lib.lfd_aggregate.argtypes = [ctxp, C.POINTER(lfd_batch), C.POINTER(lfd_params), C.c_void_p, C.c_void_p]
    lib.lfd_triangulate_dense.argtypes = [ctxp, C.POINTER(lfd_batch), C.POINTER(lfd_params), C.POINTER(lfd_points),
                                          C.c_void_p, C.c_void_p]
    lib.lfd_triangulate_dense_ply.argtypes = [ctxp, C.POINTER(lfd_batch), C.POINTER(lfd_params), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]
    lib.lfd_dense_tiles_per_ref.argtypes = [C.c_int32, C.c_int32]
    lib.lfd_dense_variant.argtypes = [C.POINTER(lfd_batch), C.POINTER(lfd_params), C.POINTER(lfd_points), C.c_void_p]
    lib.lfd_dense_variant.restype = C.c_int
    lib.lfd_triangulate_dense_segments.argtypes = [ctxp, C.POINTER(lfd_batch), C.POINTER(lfd_params), C.POINTER(lfd_points),
                                                   C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lfd_triangulate_dense_ply_segments.argtypes = [ctxp, C.POINTER(lfd_batch), C.POINTER(lfd_params), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lfd_order_segments.argtypes = [ctxp, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(lfd_points), C.POINTER(lfd_points), C.c_void_p]
    lib.lfd_pack_ply_segments.argtypes = [ctxp, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.lfd_pack_points3d_segments.argtypes = [ctxp, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                               C.c_uint64, C.c_void_p, C.c_void_p]
    lib.lfd_triangulate_indexed.argtypes = [ctxp, C.POINTER(lfd_batch), C.POINTER(lfd_params), C.c_void_p,
                                            C.POINTER(C.c_int64), C.POINTER(lfd_points), C.c_void_p, C.c_void_p,
                                            C.c_void_p]
    lib.lfd_triangulate_sampled.argtypes = [ctxp, C.POINTER(lfd_batch), C.POINTER(lfd_params), C.c_int32, C.c_float, C.c_int32,
                                            C.c_int32, C.c_float, C.POINTER(lfd_points), C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]
    lib.lfd_triangulate_sampled_multi.argtypes = [ctxp, C.POINTER(lfd_batch), C.POINTER(lfd_params), C.c_int32, C.c_float, C.c_int32,
                                                  C.c_int32, C.POINTER(C.c_uint32), C.POINTER(lfd_points), C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]
    lib.lfd_triangulate_sampled_chain.argtypes = [ctxp, C.POINTER(lfd_batch), C.POINTER(lfd_params), C.c_int32, C.c_float, C.c_int32,
                                                  C.c_int32, C.POINTER(C.c_float), C.POINTER(lfd_points), C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]
    lib.lfd_select_top_m.argtypes = [ctxp, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int64,
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.lfd_pack_ply.argtypes = [ctxp, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.lfd_pack_points3d.argtypes = [ctxp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p]
    lib.lfd_voxel_downsample.argtypes = [ctxp, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    lib.lfd_quantise_rgb.argtypes = [ctxp, C.c_void_p, C.c_int64, C.c_void_p]
    lib.lfd_local_corr.argtypes = [ctxp, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int32] * 6 + [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p]
    lib.lfd_local_corr_host.argtypes = list(lib.lfd_local_corr.argtypes)
    lib.lfd_refiner_block.argtypes = [ctxp, C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p] * 6
    lib.lfd_refiner_block_host.argtypes = list(lib.lfd_refiner_block.argtypes)
    lib.lfd_refiner_head.argtypes = ([ctxp, C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p,
                                     C.POINTER(C.c_int64), C.c_int32, C.c_float, C.c_void_p, C.c_void_p])
    lib.lfd_refiner_head_host.argtypes = list(lib.lfd_refiner_head.argtypes)
    lib.lfd_cycle_gate.argtypes = ([ctxp, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                   C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p])
    lib.lfd_cycle_gate_host.argtypes = list(lib.lfd_cycle_gate.argtypes)
    lib.lfd_support_filter.argtypes = [ctxp, C.POINTER(lfd_batch), C.POINTER(lfd_points), C.c_void_p, C.c_int32, C.c_float, C.POINTER(lfd_points),
                                       C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lfd_support_filter_host.argtypes = list(lib.lfd_support_filter.argtypes)
    lib.lfd_refine_multiview.argtypes = [ctxp, C.POINTER(lfd_batch), C.POINTER(lfd_points), C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]
    lib.lfd_refine_multiview_host.argtypes = list(lib.lfd_refine_multiview.argtypes)
    lib.lfd_refine_multiview_weighted.argtypes = list(lib.lfd_refine_multiview.argtypes) + [C.c_void_p]
    lib.lfd_refine_multiview_weighted_host.argtypes = list(lib.lfd_refine_multiview_weighted.argtypes)
    lib.lfd_depth_sigma_filter.argtypes = [ctxp, C.POINTER(lfd_batch), C.POINTER(lfd_points), C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_float,
                                           C.c_float, C.POINTER(lfd_points), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lfd_depth_sigma_filter_host.argtypes = list(lib.lfd_depth_sigma_filter.argtypes)
    lib.lfd_estimate_normals.argtypes = [ctxp, C.POINTER(lfd_batch), C.POINTER(lfd_points), C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_void_p,
                                         C.c_void_p, C.c_void_p]
    lib.lfd_estimate_normals_host.argtypes = list(lib.lfd_estimate_normals.argtypes)
    lib.lfd_colour_multiview.argtypes = [ctxp, C.POINTER(lfd_batch), C.POINTER(lfd_points), C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_void_p,
                                         C.c_void_p, C.c_void_p]
    lib.lfd_colour_multiview_host.argtypes = list(lib.lfd_colour_multiview.argtypes)
    lib.lfd_photo_gate.argtypes = [ctxp, C.POINTER(lfd_batch), C.POINTER(lfd_points), C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_float,
                                   C.POINTER(lfd_points), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lfd_photo_gate_host.argtypes = list(lib.lfd_photo_gate.argtypes)
    lib.lfd_gain_accumulate.argtypes = [ctxp, C.POINTER(lfd_batch), C.POINTER(lfd_points), C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    lib.lfd_gain_accumulate_host.argtypes = list(lib.lfd_gain_accumulate.argtypes)
    lib.lfd_gain_apply.argtypes = [ctxp, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.lfd_gain_apply_host.argtypes = list(lib.lfd_gain_apply.argtypes)
    lib.lfd_far_accumulate.argtypes = [ctxp, C.POINTER(lfd_batch), C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.lfd_far_accumulate_host.argtypes = list(lib.lfd_far_accumulate.argtypes)
    lib.lfd_far_accumulate_flags.argtypes = list(lib.lfd_far_accumulate.argtypes) + [C.c_void_p]
    lib.lfd_far_accumulate_flags_host.argtypes = list(lib.lfd_far_accumulate_flags.argtypes)
    lib.lfd_epipolar_audit.argtypes = [ctxp, C.POINTER(lfd_batch), C.c_float, C.c_void_p, C.c_void_p]
    lib.lfd_epipolar_audit_host.argtypes = list(lib.lfd_epipolar_audit.argtypes)
    lib.lfd_pose_accumulate.argtypes = [ctxp, C.POINTER(lfd_batch), C.c_float, C.c_float, C.c_void_p]
    lib.lfd_pose_accumulate_host.argtypes = list(lib.lfd_pose_accumulate.argtypes)
    lib.lfd_far_emit.argtypes = [ctxp, C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_double), C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    lib.lfd_far_emit_host.argtypes = list(lib.lfd_far_emit.argtypes)
    lib.lfd_pack_ply_normals.argtypes = [ctxp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.lfd_consensus_filter.argtypes = [ctxp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_int32, C.c_float, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_int64)]
    lib.lfd_consensus_filter_host.argtypes = list(lib.lfd_consensus_filter.argtypes)
    lib.lfd_component_filter.argtypes = [ctxp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_int32, C.c_float, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.POINTER(C.c_int64),
                                         C.POINTER(C.c_int64)]
    lib.lfd_component_filter_host.argtypes = list(lib.lfd_component_filter.argtypes)
    lib.lfd_component_filter.restype = lib.lfd_component_filter_host.restype = C.c_int
    lib.lfd_freespace_filter.argtypes = [ctxp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_float),
                                         C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    lib.lfd_freespace_filter_host.argtypes = list(lib.lfd_freespace_filter.argtypes)
    lib.lfd_render_depth.argtypes = [ctxp, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lfd_render_depth_host.argtypes = list(lib.lfd_render_depth.argtypes)
    lib.lfd_fuse_oriented.argtypes = [ctxp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.lfd_fuse_oriented_host.argtypes = list(lib.lfd_fuse_oriented.argtypes)
    lib.lfd_knn_dist2.argtypes = [ctxp, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.POINTER(C.c_double)]
    lib.lfd_knn_dist2_host.argtypes = list(lib.lfd_knn_dist2.argtypes)
    lib.lfd_pack_gaussians.argtypes = [ctxp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_double, C.c_double, C.c_void_p]
    lib.lfd_pack_gaussians_host.argtypes = list(lib.lfd_pack_gaussians.argtypes)
    lib.lfd_cap_spatial.argtypes = [ctxp, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    lib.lfd_cap_spatial_host.argtypes = list(lib.lfd_cap_spatial.argtypes)
    lib.lfd_thin_footprint.argtypes = [ctxp, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_double), C.c_double,
                                       C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    lib.lfd_thin_footprint_host.argtypes = list(lib.lfd_thin_footprint.argtypes)
    lib.lfd_copy_segments.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    lib.lfd_launch_status.argtypes = [ctxp, C.POINTER(C.c_int32)]
    lib.lfd_get_pair_fundamental.argtypes = [ctxp, C.c_int32, C.POINTER(C.c_double)]
    lib.lfd_rng_seed.argtypes = [ctxp, C.c_uint32]
    lib.lfd_rng_get_state.argtypes = [ctxp, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
    lib.lfd_rng_set_state.argtypes = [ctxp, C.POINTER(C.c_uint32), C.c_int32]
    lib.lfd_rng_checkpoint.argtypes = [ctxp, C.c_int32]
    lib.lfd_rng_rollback.argtypes = [ctxp, C.c_int32]
    lib.lfd_select_samples.argtypes = [ctxp, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32,
                                       C.c_float, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.lfd_create_host.argtypes = [C.c_int32, C.POINTER(ctxp)]
    lib.lfd_host_threads.argtypes = [ctxp]
    lib.lfd_host_threads.restype = C.c_int
    lib.lfd_aggregate_host.argtypes = [ctxp, C.POINTER(lfd_batch), C.POINTER(lfd_params), C.c_void_p, C.c_void_p]
    lib.lfd_triangulate_dense_host.argtypes = [ctxp, C.POINTER(lfd_batch), C.POINTER(lfd_params), C.POINTER(lfd_points),
                                               C.c_void_p, C.c_void_p]
    lib.lfd_triangulate_indexed_host.argtypes = [ctxp, C.POINTER(lfd_batch), C.POINTER(lfd_params), C.c_void_p,
                                                 C.POINTER(C.c_int64), C.POINTER(lfd_points), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lfd_prepare_image.argtypes = [ctxp, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.lfd_prepare_mask.argtypes = [ctxp, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p]
    dptr = C.POINTER(C.c_double)
    lib.lfd_undistort_image.argtypes = [ctxp, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, dptr, dptr, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    lib.lfd_host_undistort_image.argtypes = list(lib.lfd_undistort_image.argtypes[1:])
    lib.lfd_host_resize_tables.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32)]
    lib.lfd_host_nearest_indices.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    lib.lfd_identity_axis.argtypes = [C.c_int32, fptr]
    lib.lfd_parallax_dot_threshold.argtypes = [C.c_float]
    lib.lfd_parallax_dot_threshold.restype = C.c_float
    lib.lfd_host_fundamental.argtypes = [fptr] * 7
    lib.lfd_host_null_vector.argtypes = [fptr, C.POINTER(C.c_double)]
    lib.lfd_host_null_vector.restype = C.c_int
    lib.lfd_host_null_vector_sym.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.lfd_host_null_vector_sym.restype = C.c_int
    lib.lfd_host_eval_correspondence.argtypes = [fptr, fptr, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32,
                                                 C.c_int32, C.POINTER(lfd_params), fptr]
    for name in ("lfd_create", "lfd_set_stream", "lfd_reload_env", "lfd_kernel_timing", "lfd_kernel_timing_read", "lfd_upload_cameras", "lfd_prepare_batch", "lfd_aggregate", "lfd_triangulate_dense",
                 "lfd_triangulate_dense_ply", "lfd_triangulate_dense_ply_segments", "lfd_dense_tiles_per_ref", "lfd_triangulate_dense_segments", "lfd_order_segments", "lfd_pack_ply_segments", "lfd_pack_points3d_segments",
                 "lfd_triangulate_indexed", "lfd_triangulate_sampled", "lfd_triangulate_sampled_multi", "lfd_triangulate_sampled_chain", "lfd_launch_status", "lfd_rng_seed", "lfd_rng_get_state", "lfd_rng_set_state",
                 "lfd_rng_checkpoint", "lfd_rng_rollback",
                 "lfd_select_samples", "lfd_select_top_m", "lfd_pack_ply", "lfd_pack_points3d", "lfd_voxel_downsample", "lfd_local_corr", "lfd_local_corr_host", "lfd_refiner_block", "lfd_refiner_block_host", "lfd_refiner_head", "lfd_refiner_head_host", "lfd_cycle_gate", "lfd_cycle_gate_host", "lfd_support_filter", "lfd_support_filter_host", "lfd_refine_multiview", "lfd_refine_multiview_host", "lfd_refine_multiview_weighted", "lfd_refine_multiview_weighted_host", "lfd_depth_sigma_filter", "lfd_depth_sigma_filter_host", "lfd_estimate_normals", "lfd_estimate_normals_host", "lfd_colour_multiview", "lfd_photo_gate", "lfd_photo_gate_host", "lfd_colour_multiview_host", "lfd_gain_accumulate", "lfd_gain_accumulate_host", "lfd_gain_apply", "lfd_gain_apply_host", "lfd_far_accumulate", "lfd_far_accumulate_host", "lfd_far_accumulate_flags", "lfd_far_accumulate_flags_host", "lfd_far_emit", "lfd_far_emit_host", "lfd_pack_ply_normals", "lfd_consensus_filter", "lfd_consensus_filter_host", "lfd_freespace_filter", "lfd_freespace_filter_host", "lfd_render_depth", "lfd_render_depth_host", "lfd_fuse_oriented", "lfd_fuse_oriented_host", "lfd_knn_dist2", "lfd_knn_dist2_host", "lfd_pack_gaussians", "lfd_pack_gaussians_host", "lfd_cap_spatial", "lfd_cap_spatial_host", "lfd_thin_footprint", "lfd_thin_footprint_host", "lfd_quantise_rgb", "lfd_copy_segments", "lfd_identity_axis",
                 "lfd_host_fundamental", "lfd_get_pair_fundamental", "lfd_create_host", "lfd_aggregate_host",
                 "lfd_triangulate_dense_host", "lfd_triangulate_indexed_host", "lfd_prepare_image", "lfd_prepare_mask",
                 "lfd_host_resize_tables", "lfd_host_nearest_indices",
                 "lfd_host_eval_correspondence"):
        getattr(lib, name).restype = C.c_int
    _lib = lib
    return lib


def make_params(config: DensePipelineConfig, sample_cap: float = 0.9, exact_colour: Optional[bool] = None) -> lfd_params:
    """``exact_colour``: dense mode blends colours in f64 like upstream (bit-identical rgb) instead of f32 (within 2.5e-7);
    default: the configuration's ``exact_colour`` field (False).
    With ``experimental['cycle_thresh_px']`` > 0 the certainty planes reach the kernels GATED (lfd_cycle_gate): they carry the floor already
    and a rejected cell is exactly 0, so the kernels' own floor is min(thresh, 0) - it leaves every value of a gated plane (>= thresh, 0, NaN)
    as it is, and a rejected cell behaves like one that mask_b masks out."""
    if exact_colour is None:
        exact_colour = bool(config.exact_colour)
    floor = float(config.certainty_thresh)
    if float(config.exp("cycle_thresh_px")) > 0.0:
        floor = min(floor, 0.0)
    return lfd_params(sampson_thresh=float(config.sampson_thresh), certainty_thresh=floor,
                      sample_cap=float(sample_cap), reproj_thresh=float(config.reproj_thresh),
                      min_parallax_deg=float(config.min_parallax_deg), no_filter=1 if config.no_filter else 0,
                      flags=LFD_FLAG_EXACT_COLOUR if exact_colour else 0)


def dense_variant(batch: lfd_batch, params: lfd_params, out: lfd_points, seg_counts: Optional[int] = None) -> int:
    """lfd_dense_variant: which instantiation of the fused kernel lfd_triangulate_dense runs for these ctypes structures (``PreparedBatch.c``,
    ``make_params``, ``OutputBuffers.c``) and this ``seg_counts`` address - 1 the production-shape kernel, 0 the generic one.  A host
    function: needs no context and no GPU.  (LFD_DENSE_GENERIC=1 in the environment of a context forces the generic kernel regardless.)"""
    return int(load_library().lfd_dense_variant(C.byref(batch), C.byref(params), C.byref(out), seg_counts))


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, np.float32))


def _fp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


# ---- host helpers (usable without a GPU) --------------------------------------------------------
def identity_axis(n: int) -> np.ndarray:
    out = np.empty(n, np.float32)
    rc = load_library().lfd_identity_axis(n, _fp(out))
    if rc != 0:
        raise HipBackendError("lfd_identity_axis failed")
    return out


def copy_segments(src: torch.Tensor, dst: torch.Tensor, segments, stream: Optional["torch.cuda.Stream"] = None) -> None:
    """lfd_copy_segments: ``dst.bytes[d : d + n] = src.bytes[s : s + n]`` for every row ``(s, d, n)`` of ``segments`` (int64, byte offsets into the two
    contiguous device tensors' storage views) in ONE launch on ``stream`` (default: torch's current stream of that device).  Asynchronous."""
    segs = np.ascontiguousarray(np.asarray(segments, np.int64).reshape(-1, 3))
    if segs.shape[0] == 0:
        return
    if not (src.is_cuda and dst.is_cuda and src.device == dst.device and src.is_contiguous() and dst.is_contiguous()):
        raise ValueError("copy_segments needs two contiguous tensors on one GPU")
    sb, db = src.numel() * src.element_size(), dst.numel() * dst.element_size()
    if segs.min() < 0 or int((segs[:, 0] + segs[:, 2]).max()) > sb or int((segs[:, 1] + segs[:, 2]).max()) > db:
        raise ValueError("copy_segments: a segment leaves its tensor")
    st = stream if stream is not None else torch.cuda.current_stream(src.device)
    rc = load_library().lfd_copy_segments(C.c_void_p(st.cuda_stream), int(src.device.index or 0), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
                                          segs.ctypes.data_as(C.c_void_p), int(segs.shape[0]))
    if rc != 0:
        raise HipBackendError(f"lfd_copy_segments failed ({rc})")


def parallax_dot_threshold(min_deg: float) -> float:
    return float(load_library().lfd_parallax_dot_threshold(C.c_float(min_deg)))


def host_fundamental(K1, R1, t1, K2, R2, t2) -> np.ndarray:
    a = [_f32(x).reshape(-1) for x in (K1, R1, t1, K2, R2, t2)]
    out = np.empty(9, np.float32)
    rc = load_library().lfd_host_fundamental(*[_fp(x) for x in a], _fp(out))
    if rc != 0:
        raise HipBackendError("lfd_host_fundamental failed")
    return out.reshape(3, 3)


def host_resize_tables(in_size: int, out_size: int):
    """(bounds (out,2), kk (out,ksize)) of the BILINEAR resampling exactly as the device kernel uses them (Pillow's tables)."""
    lib = load_library()
    ks = C.c_int32(0)
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((1,), np.int32)
    lib.lfd_host_resize_tables(in_size, out_size, bounds.ctypes.data_as(C.POINTER(C.c_int32)), kk.ctypes.data_as(C.POINTER(C.c_int32)), 0, C.byref(ks))
    kk = np.zeros((out_size, int(ks.value)), np.int32)
    rc = lib.lfd_host_resize_tables(in_size, out_size, bounds.ctypes.data_as(C.POINTER(C.c_int32)), kk.ctypes.data_as(C.POINTER(C.c_int32)),
                                    int(kk.size), C.byref(ks))
    if rc != 0:
        raise HipBackendError("lfd_host_resize_tables failed")
    return bounds, kk


def host_nearest_indices(in_size: int, out_size: int) -> np.ndarray:
    idx = np.zeros((out_size,), np.int32)
    if load_library().lfd_host_nearest_indices(in_size, out_size, idx.ctypes.data_as(C.POINTER(C.c_int32))) != 0:
        raise HipBackendError("lfd_host_nearest_indices failed")
    return idx


def _undistort_parameters(distortion):
    """(intr, dist) as the C arrays of lfd_undistort_image from the twelve f64 values (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6)."""
    d = [float(v) for v in distortion]
    if len(d) != 12:
        raise ValueError("distortion must hold twelve values: fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6")
    return (C.c_double * 4)(*d[:4]), (C.c_double * 8)(*d[4:])


def host_undistort_image(src, distortion, nearest: bool = False, with_valid: bool = False):
    """The context-free CPU twin of ``HipDensifier.undistort_image`` (lfd_host_undistort_image): ``src`` a (h, w) or
    (h, w, 3) u8 array, ``distortion`` the twelve f64 parameters.  Returns ``(dst, valid255 or None, n_invalid)``; ``valid255`` (h, w) u8 is
    255 where the photograph covers the pixel and 0 elsewhere.  Callable from several threads at once."""
    a = np.ascontiguousarray(src, dtype=np.uint8)
    if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise ValueError("src must be a (h, w) or (h, w, 3) uint8 array")
    h, w = int(a.shape[0]), int(a.shape[1])
    intr, dist = _undistort_parameters(distortion)
    dst = np.empty_like(a)
    valid = np.empty((h, w), np.uint8) if with_valid else None
    n_bad = C.c_int64(-1)
    rc = load_library().lfd_host_undistort_image(a.ctypes.data, w, h, 1 if a.ndim == 2 else 3, 1 if nearest else 0, intr, dist, dst.ctypes.data,
                                                 valid.ctypes.data if with_valid else None, C.byref(n_bad))
    if rc != 0:
        raise HipBackendError(f"lfd_host_undistort_image refused its arguments ({rc}): {w} x {h}, parameters {tuple(float(v) for v in distortion)}")
    return dst, valid, int(n_bad.value)


def fundamental_from_world2cam(K1, R1, t1, K2, R2, t2) -> np.ndarray:
    """Upstream's ``fundamental_from_world2cam`` (core/geometry.py:122-130 with ``skew`` :53-55): the same NumPy
    calls in the same order on the same f32 arrays (``np.linalg.inv`` is LAPACK sgetrf/sgetri), so the result is
    upstream's F bit for bit on the same machine.  Handed to the kernels through ``lfd_batch.fundamental``."""
    K1, R1, K2, R2 = (np.asarray(a, np.float32) for a in (K1, R1, K2, R2))
    t1, t2 = np.asarray(t1, np.float32).reshape(3, 1), np.asarray(t2, np.float32).reshape(3, 1)
    R = R2 @ R1.T
    t = (t2 - R @ t1).reshape(3)
    tx, ty, tz = t
    cross = np.array([[0, -tz, ty], [tz, 0, -tx], [-ty, tx, 0]], dtype=np.float32)
    E = cross @ R
    return _inv_intrinsics(K2).T @ E @ _inv_intrinsics(K1)


_KINV_CACHE: dict = {}


def _inv_intrinsics(K: np.ndarray) -> np.ndarray:
    """``np.linalg.inv(K)`` (upstream's call, LAPACK sgetrf/sgetri), remembered by the matrix's bytes: a run has a few hundred cameras and every
    pair asks for both inverses - the same LAPACK call on the same bytes gives the same bytes, so the cache changes no result, only the count
    of LAPACK calls in the per-reference loop (six per reference of three neighbours otherwise)."""
    key = K.tobytes()
    inv = _KINV_CACHE.get(key)
    if inv is None:
        if len(_KINV_CACHE) > 4096:
            _KINV_CACHE.clear()
        inv = _KINV_CACHE[key] = np.linalg.inv(K)
    return inv


def host_null_vector(A) -> "tuple[np.ndarray, int]":
    """Smallest right singular vector (un-normalised, f64) of a 4x4 f32 matrix through the routine the kernels
    triangulate with (host build of csrc/lfd_geometry.hpp), and the number of solves it made."""
    a = _f32(A).reshape(16)
    out = np.zeros(4, np.float64)
    it = load_library().lfd_host_null_vector(_fp(a), out.ctypes.data_as(C.POINTER(C.c_double)))
    if it < 0:
        raise HipBackendError("lfd_host_null_vector failed")
    return out, int(it)


def host_null_vector_sym(M) -> "tuple[np.ndarray, int]":
    """Smallest eigenvector (un-normalised, f64) of a symmetric positive semi-definite 4x4 matrix through the routine the multi-view
    re-triangulation solves with (host build of csrc/lfd_refine.hpp::lfd_null_vector_sym), and the number of solves it made."""
    M = np.asarray(M, np.float64).reshape(4, 4)
    m = np.ascontiguousarray(M[np.triu_indices(4)], np.float64)
    out = np.zeros(4, np.float64)
    it = load_library().lfd_host_null_vector_sym(m.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double)))
    if it < 0:
        raise HipBackendError("lfd_host_null_vector_sym failed")
    return out, int(it)


def pack_camera(cam: CameraRecord) -> np.ndarray:
    return np.concatenate([_f32(cam.K).reshape(-1), _f32(cam.R).reshape(-1), _f32(cam.t).reshape(-1),
                           _f32(cam.P).reshape(-1), _f32(cam.C).reshape(-1),
                           np.array([cam.width, cam.height], np.float32)]).astype(np.float32)


def host_eval_correspondence(cam1: CameraRecord, cam2: CameraRecord, xa, ya, xb, yb, w_match, h_match,
                             params: lfd_params) -> np.ndarray:
    """The per-cell routine (host build of the kernels' source) on one correspondence: a debugging /
    unit-test aid, not a code path of the pipeline.  Returns [x,y,z,_,_,_,err,keep]."""
    out = np.zeros(8, np.float32)
    c1, c2 = pack_camera(cam1), pack_camera(cam2)
    rc = load_library().lfd_host_eval_correspondence(_fp(c1), _fp(c2), C.c_float(xa), C.c_float(ya), C.c_float(xb),
                                                     C.c_float(yb), int(w_match), int(h_match), C.byref(params), _fp(out))
    if rc != 0:
        raise HipBackendError("lfd_host_eval_correspondence failed")
    return out


# ---- device path ---------------------------------------------------------------------------------
@dataclasses.dataclass
class ReferenceInputs:
    """Device-resident inputs of one reference view (what RoMa produced for it)."""
    ref_cam: int                              # index into the uploaded camera table
    nbr_cams: List[int]                       # one per neighbour slot
    cert: List[torch.Tensor]                  # per slot (H,W) f32, raw certainty
    warp: List[torch.Tensor]                  # per slot (H,W,2|4) f32
    image: torch.Tensor                       # (h_match,w_match,3) u8
    mask_a: Optional[torch.Tensor] = None     # (h_match,w_match) u8 {0,1}
    mask_b: Optional[List[Optional[torch.Tensor]]] = None
    fundamental: Optional[Sequence[np.ndarray]] = None   # per slot (3,3) f32: upstream's F for the pair (see PreparedBatch)
    precision: Optional[List[torch.Tensor]] = None   # per slot (H,W,3) f32: RoMa-v2's precision (q00, q01, q11), match px^-2
    nbr_images: Optional[List[torch.Tensor]] = None  # per slot (h_match,w_match,3) u8: the neighbour's match-size image (lfd_colour_multiview)


@dataclasses.dataclass
class TriangulationOutput:
    xyz: torch.Tensor            # (n,3) f32
    rgb: torch.Tensor            # (n,3) f32 in [0,1]
    err: torch.Tensor            # (n,)  f32
    cell: Optional[torch.Tensor]  # (n,) i32
    slot: Optional[torch.Tensor]  # (n,) u8
    ref_offsets: np.ndarray      # (n_refs+1,) i64 host
    seg_counts: np.ndarray       # (n_refs,k) i32 host
    seg_order: Optional[np.ndarray] = None   # indexed mode: slot of the g-th emitted group, -1 = none
    n_selected: Optional[int] = None         # sampled call: cells the selection stage picked
    launch_status: int = 0                   # sampled call: look-back status of the launch (0 = ok)
    sel_status: Optional[np.ndarray] = None  # sampled calls: selection status per reference (0 = ok, else what upstream would have raised for)
    support_in: Optional[int] = None         # buffers lfd_support_filter filled: the points that reached the filter (``count`` of them were kept)
    sigma_in: Optional[int] = None           # buffers lfd_depth_sigma_filter filled: the points that reached the gate (``count`` of them were kept;
                                             # with both, the support filter kept ``sigma_in``)
    photo_in: Optional[int] = None           # buffers lfd_photo_gate filled: the points that reached it (``count`` of them were kept; the stage in
                                             # front of it kept ``photo_in``)
    _packed: Optional[torch.Tensor] = None   # the one float buffer xyz / rgb / err are views of
    _cap: int = 0
    normals: Optional[torch.Tensor] = None   # (n,3) f32 where the points live: what estimate_normals wrote for these points

    def host_arrays(self):
        """(xyz, rgb, err) as NumPy arrays.  When the buffers are small (sampled mode) the whole packed buffer crosses in
        one copy instead of three."""
        n = int(self.xyz.shape[0])
        if self._packed is None or self._cap * 7 > (1 << 20) or n == 0:
            return self.xyz.cpu().numpy(), self.rgb.cpu().numpy(), self.err.cpu().numpy()
        h = self._packed.cpu().numpy()
        c = self._cap
        return h[:3 * c].reshape(c, 3)[:n].copy(), h[3 * c:6 * c].reshape(c, 3)[:n].copy(), h[6 * c:6 * c + n].copy()

    @property
    def count(self) -> int:
        return int(self.ref_offsets[-1])


@dataclasses.dataclass
class SegmentedOutput:
    """What lfd_triangulate_dense_segments leaves on the device: reference r's survivors in rows [r*H*W, r*H*W + ref_counts[r]) of the
    buffers, tile after tile in the order the tiles retired; ``table[r * tiles_per_ref + t] = (offset, count)`` of every tile.  The ordered
    result / the file payload come out of ``HipDensifier.order_segments`` / ``pack_ply_segments`` / ``pack_points3d_segments``."""
    buffers: "OutputBuffers"
    table: torch.Tensor          # (n_refs * tiles_per_ref, 2) i32
    ref_counts: torch.Tensor     # (n_refs,) i64, device
    n_refs: int
    H: int
    W: int
    k: int


class PreparedBatch:
    """ctypes view of a list of ReferenceInputs; keeps the tensors alive."""

    def __init__(self, refs: Sequence[ReferenceInputs], w_match: int, h_match: int,
                 axes: Optional[Sequence[torch.Tensor]] = None, cameras: Optional[Sequence[CameraRecord]] = None):
        """``cameras``: the run's camera records; when given, every pair's fundamental matrix is computed on the host
        with upstream's own NumPy calls (``fundamental_from_world2cam``) and handed to the library, so the Sampson gate
        sees upstream's F bit for bit.  A reference that carries its own ``fundamental`` list keeps it."""
        if not refs:
            raise ValueError("empty batch")
        self.refs = list(refs)
        n = len(self.refs)
        k = max(len(r.cert) for r in self.refs)
        if k < 1 or k > LFD_MAX_SLOTS:
            raise ValueError(f"neighbour slots per reference must be in [1,{LFD_MAX_SLOTS}]")
        H, W = self.refs[0].cert[0].shape
        ch = int(self.refs[0].warp[0].shape[-1])
        dev = self.refs[0].cert[0].device
        self.n_refs, self.k, self.H, self.W, self.channels, self.device = n, k, int(H), int(W), ch, dev
        self.ref_cam = (C.c_int32 * n)(*[int(r.ref_cam) for r in self.refs])
        self.n_slots = (C.c_int32 * n)(*[len(r.cert) for r in self.refs])
        self.nbr_cam = (C.c_int32 * (n * k))()
        self.cert = (C.c_void_p * (n * k))()
        self.warp = (C.c_void_p * (n * k))()
        self.image = (C.c_void_p * n)()
        any_ma = any(r.mask_a is not None for r in self.refs)
        any_mb = any(r.mask_b is not None and any(m is not None for m in r.mask_b) for r in self.refs)
        self.mask_a = (C.c_void_p * n)() if any_ma else None
        self.mask_b = (C.c_void_p * (n * k))() if any_mb else None
        self._keep = []
        for i, r in enumerate(self.refs):
            if not (len(r.cert) == len(r.warp) == len(r.nbr_cams)):
                raise ValueError("cert / warp / nbr_cams length mismatch")
            img = self._chk(r.image, torch.uint8, (h_match, w_match, 3), "image")
            self.image[i] = img.data_ptr()
            if r.mask_a is not None:
                self.mask_a[i] = self._chk(r.mask_a, torch.uint8, (h_match, w_match), "mask_a").data_ptr()
            for j in range(len(r.cert)):
                s = i * k + j
                self.nbr_cam[s] = int(r.nbr_cams[j])
                self.cert[s] = self._chk(r.cert[j], torch.float32, (H, W), "cert").data_ptr()
                self.warp[s] = self._chk(r.warp[j], torch.float32, (H, W, ch), "warp").data_ptr()
                if r.mask_b is not None and r.mask_b[j] is not None:
                    self.mask_b[s] = self._chk(r.mask_b[j], torch.uint8, (h_match, w_match), "mask_b").data_ptr()
        # the precision planes of lfd_refine_multiview_weighted: a table of its own (lfd_batch is pinned), present when EVERY reference has them
        self.precision = None
        if all(r.precision is not None for r in self.refs):
            self.precision = (C.c_void_p * (n * k))()
            for i, r in enumerate(self.refs):
                if len(r.precision) != len(r.cert):
                    raise ValueError("precision / cert length mismatch")
                for j in range(len(r.cert)):
                    self.precision[i * k + j] = self._chk(r.precision[j], torch.float32, (H, W, 3), "precision").data_ptr()
        elif any(r.precision is not None for r in self.refs):
            raise ValueError("precision planes must be given for every reference of a batch or for none")
        # the neighbours' images of lfd_colour_multiview: a table of its own like the precision planes', present when EVERY reference has them
        self.nbr_images = None
        if all(r.nbr_images is not None for r in self.refs):
            self.nbr_images = (C.c_void_p * (n * k))()
            for i, r in enumerate(self.refs):
                if len(r.nbr_images) != len(r.cert):
                    raise ValueError("nbr_images / cert length mismatch")
                for j in range(len(r.cert)):
                    self.nbr_images[i * k + j] = self._chk(r.nbr_images[j], torch.uint8, (h_match, w_match, 3), "nbr_images").data_ptr()
        elif any(r.nbr_images is not None for r in self.refs):
            raise ValueError("neighbour images must be given for every reference of a batch or for none")
        self.fundamental = None
        if cameras is not None or any(r.fundamental is not None for r in self.refs):
            fund = np.zeros((n * k, 9), np.float32)
            for i, r in enumerate(self.refs):
                for j in range(len(r.cert)):
                    if r.fundamental is not None:
                        F = np.asarray(r.fundamental[j], np.float32)
                    elif cameras is not None:
                        a, b = cameras[int(r.ref_cam)], cameras[int(r.nbr_cams[j])]
                        F = fundamental_from_world2cam(a.K, a.R, a.t, b.K, b.R, b.t)
                    else:
                        raise ValueError("fundamental matrices must be given for every reference of a batch or for none")
                    fund[i * k + j] = np.asarray(F, np.float32).reshape(9)
            self.fundamental = np.ascontiguousarray(fund)
        self.axes = None
        if axes is not None:
            ax = self._chk(axes[0], torch.float32, (W,), "axis_x")
            ay = self._chk(axes[1], torch.float32, (H,), "axis_y")
            self.axes = (ax, ay)
        vp = C.POINTER(C.c_void_p)
        self.c = lfd_batch(
            n_refs=n, k=k, H=int(H), W=int(W), w_match=int(w_match), h_match=int(h_match), warp_channels=ch, reserved=0,
            fundamental=self.fundamental.ctypes.data_as(C.POINTER(C.c_float)) if self.fundamental is not None else None,
            ref_cam=C.cast(self.ref_cam, C.POINTER(C.c_int32)), n_slots=C.cast(self.n_slots, C.POINTER(C.c_int32)),
            nbr_cam=C.cast(self.nbr_cam, C.POINTER(C.c_int32)), cert=C.cast(self.cert, vp), warp=C.cast(self.warp, vp),
            image=C.cast(self.image, vp), mask_a=C.cast(self.mask_a, vp) if self.mask_a is not None else None,
            mask_b=C.cast(self.mask_b, vp) if self.mask_b is not None else None,
            axis_x=self.axes[0].data_ptr() if self.axes else None, axis_y=self.axes[1].data_ptr() if self.axes else None)

    def _chk(self, t: torch.Tensor, dtype, shape, what: str) -> torch.Tensor:
        if not isinstance(t, torch.Tensor) or t.device != self.device:
            raise ValueError(f"{what} must be a tensor on {self.device} (the path consumes RoMa's outputs in place, "
                             "all tensors of a batch on one device)")
        if t.dtype != dtype or tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what}: expected {dtype} {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
        if not t.is_contiguous():
            t = t.contiguous()
        self._keep.append(t)
        return t


_tls = threading.local()
# 1-3: what upstream's np.random.choice raises for (the reference drew nothing, there as here).  4-7: this implementation's own refusals -
# the reference did NOT do what upstream would have done with the stream, so a fused call of several references that reports one of them
# is void from that reference on (SELECT_VOIDS_STREAM; core/strategies.py::SampledLoop rolls the stream back and redoes the references).
_SELECT_ERRORS = {1: "probabilities contain NaN", 2: "probabilities are not non-negative", 3: "Fewer non-zero entries in p than size",
                  4: "selection: a weight is below 2^-29 (exact parallel cumsum not guaranteed)",
                  5: "selection made no progress (a bounded wait between its workgroups expired; nothing was committed to the random stream)",
                  6: "selection: too many coverage bins for the device stage",
                  7: "selection: more cells than the output has room for"}
SELECT_VOIDS_STREAM = frozenset((4, 5, 6, 7))
RNG_CHECKPOINTS = 4            # LFD_RNG_CHECKPOINTS of the header


def selection_error(status: int) -> str:
    """What upstream's sampling stage says (np.random.choice's ValueError texts) for a selection status of the fused calls."""
    return _SELECT_ERRORS.get(int(status), f"selection failed with status {int(status)}")


def _read_back_i32(t: torch.Tensor) -> np.ndarray:
    """Small int32 device tensor -> NumPy copy, staged through a per-thread pinned buffer (a pageable ``.cpu()`` costs
    ~2x as much and pinning a fresh buffer per call far more)."""
    n = int(t.numel())
    if not t.is_cuda:
        return t.numpy().copy()
    buf = getattr(_tls, "pinned_i32", None)
    if buf is None or buf.numel() < n:
        buf = torch.empty((max(n, 4096),), dtype=torch.int32).pin_memory()
        _tls.pinned_i32 = buf
    buf[:n].copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return buf[:n].numpy().copy()


class OutputBuffers:
    """Caller-owned survivor buffers (device).  Allocate once, reuse across launches."""

    def __init__(self, capacity: int, n_refs: int, k: int, device, with_cell: bool = True, with_segments: bool = True):
        """``with_cell``: also return the grid cell / neighbour slot of every survivor (debug previews);
        ``with_segments``: also count survivors per (reference, neighbour) - upstream's group sizes.  Both are
        optional outputs of the C-ABI; upstream's own result is xyz, rgb, err."""
        self.capacity = int(capacity)
        self.with_segments = with_segments
        cap = max(self.capacity, 1)
        # one allocation for the three float outputs (views below): the sampled mode's few thousand points then reach the
        # host in ONE copy (TriangulationOutput.host_arrays)
        self._f = torch.empty((cap * 7,), dtype=torch.float32, device=device)
        self.xyz = self._f[:cap * 3].view(cap, 3)
        self.rgb = self._f[cap * 3:cap * 6].view(cap, 3)
        self.err = self._f[cap * 6:]
        self.cell = torch.empty((cap,), dtype=torch.int32, device=device) if with_cell else None
        self.slot = torch.empty((cap,), dtype=torch.uint8, device=device) if with_cell else None
        # the small integer outputs share ONE buffer so that collect() needs a single device-to-host copy:
        # [ref_offsets i64 x (R+1)] [seg_counts i32 x R*k] [seg_order i32 x R*k]
        n_off, n_seg = 2 * (n_refs + 1), n_refs * k
        # ... [sel_info i32 x 2R+1] [pad to 8 bytes] [support_in i64]: the points that reached lfd_support_filter, written by HipDensifier.support_filter
        n_info = 2 * n_refs + 2
        # ... [sigma_in i64]: the points that reached lfd_depth_sigma_filter, written by HipDensifier.depth_sigma_filter
        # ... [photo_in i64]: the points that reached lfd_photo_gate, written by HipDensifier.photo_gate
        self._meta = torch.zeros((n_off + 2 * n_seg + n_info + 6,), dtype=torch.int32, device=device)
        self._meta[n_off + n_seg:n_off + 2 * n_seg].fill_(-1)
        self.ref_offsets = self._meta[:n_off].view(torch.int64)
        self.seg_counts = self._meta[n_off:n_off + n_seg].view(n_refs, k)
        self.seg_order = self._meta[n_off + n_seg:n_off + 2 * n_seg].view(n_refs, k)
        self.support_in = self._meta[n_off + 2 * n_seg + n_info:n_off + 2 * n_seg + n_info + 2].view(torch.int64)
        self.sigma_in = self._meta[n_off + 2 * n_seg + n_info + 2:n_off + 2 * n_seg + n_info + 4].view(torch.int64)
        self.photo_in = self._meta[n_off + 2 * n_seg + n_info + 4:].view(torch.int64)
        self.normals: Optional[torch.Tensor] = None              # (cap,3) f32, allocated by the first estimate_normals over these buffers
        self.normals_valid = False                               # True: ``normals`` was written for the points the buffers hold NOW (collect
                                                                 # hands them out); whatever refills the buffers or moves their points clears it
        self.filtered = False                                    # True: these buffers are a support filter's destination (collect reports support_in)
        self.sigma_filtered = False                              # True: ... a depth-uncertainty gate's (collect reports sigma_in)
        self.photo_filtered = False                              # True: ... a photo-consistency gate's (collect reports photo_in)
        self.sel_info = self._meta[n_off + 2 * n_seg:n_off + 2 * n_seg + 2 * n_refs + 1]           # lfd_triangulate_sampled[_multi]: {cells selected, selection status} per reference, then the launch status
        self._n_refs, self._k = n_refs, k
        self.c = lfd_points(xyz=self.xyz.data_ptr(), rgb=self.rgb.data_ptr(), err=self.err.data_ptr(),
                            cell=self.cell.data_ptr() if with_cell else None,
                            slot=self.slot.data_ptr() if with_cell else None, capacity=self.capacity)

    def begin_collect(self, stream: Optional["torch.cuda.Stream"] = None) -> None:
        """Enqueue the read-back of the small integer outputs (counts, selection / launch status) into this buffer's own pinned
        landing area and record an event behind it: ``collect`` then waits for THAT event only, not for whatever has been
        launched on the stream since (the next reference's kernels)."""
        if not self._meta.is_cuda:
            return
        if getattr(self, "_pinned_meta", None) is None:
            self._pinned_meta = torch.empty((int(self._meta.numel()),), dtype=torch.int32).pin_memory()
            self._meta_event = torch.cuda.Event()
        st = stream if stream is not None else torch.cuda.current_stream(self._meta.device)
        with torch.cuda.stream(st):
            self._pinned_meta.copy_(self._meta, non_blocking=True)
            self._meta_event.record(st)
        self._meta_pending = True

    def select_status(self, meta: np.ndarray) -> int:
        """Worst selection status over the references of a fused sampled call (0 = every selection went through)."""
        base = 2 * (self._n_refs + 1) + 2 * self._n_refs * self._k
        st = meta[base + 1:base + 2 * self._n_refs:2]
        bad = st[st != 0]
        return int(bad[0]) if bad.size else 0

    def collect(self, indexed: bool = False, check_selection: bool = False) -> TriangulationOutput:
        """Synchronise and trim to the number of survivors.  ``check_selection``: raise what upstream's sampling stage
        would have raised if the fused call's selection refused its input (any reference's; without it the caller reads
        ``sel_status`` reference by reference)."""
        if getattr(self, "_meta_pending", False):             # begin_collect() was called: wait for that copy alone
            self._meta_event.synchronize()
            self._meta_pending = False
            meta = self._pinned_meta.numpy().copy()
        else:
            meta = _read_back_i32(self._meta)                 # one copy through a cached pinned buffer (synchronises)
        if check_selection:
            st = self.select_status(meta)
            if st in (1, 2, 3):
                raise ValueError(_SELECT_ERRORS[st])
            if st == 4:
                raise SelectionInexact(_SELECT_ERRORS[4])
            if st != 0:
                raise HipBackendError(selection_error(st))
        n_off, n_seg = 2 * (self._n_refs + 1), self._n_refs * self._k
        offs = meta[:n_off].view(np.int64).copy()
        n = int(offs[-1])
        if n > self.capacity:
            raise HipBackendError(f"output capacity {self.capacity} too small for {n} survivors")
        return TriangulationOutput(
            xyz=self.xyz[:n], rgb=self.rgb[:n], err=self.err[:n],
            cell=self.cell[:n] if self.cell is not None else None, slot=self.slot[:n] if self.slot is not None else None,
            ref_offsets=offs, seg_counts=meta[n_off:n_off + n_seg].reshape(self._n_refs, self._k).copy(),
            seg_order=meta[n_off + n_seg:n_off + 2 * n_seg].reshape(self._n_refs, self._k).copy() if indexed else None,
            n_selected=int(meta[n_off + 2 * n_seg:n_off + 2 * n_seg + 2 * self._n_refs:2].sum()),
            sel_status=meta[n_off + 2 * n_seg + 1:n_off + 2 * n_seg + 2 * self._n_refs:2].copy(),
            launch_status=int(meta[n_off + 2 * n_seg + 2 * self._n_refs]),
            support_in=int(meta[n_off + 2 * n_seg + 2 * self._n_refs + 2:].view(np.int64)[0]) if self.filtered else None,
            sigma_in=int(meta[n_off + 2 * n_seg + 2 * self._n_refs + 2:].view(np.int64)[1]) if self.sigma_filtered else None,
            photo_in=int(meta[n_off + 2 * n_seg + 2 * self._n_refs + 2:].view(np.int64)[2]) if self.photo_filtered else None, _packed=self._f,
            _cap=max(self.capacity, 1), normals=self.normals[:n] if (self.normals is not None and self.normals_valid) else None)



def _local_corr_arguments(a, bf, warp, device):
    """Shapes, dtype and device of a local_corr call checked; (a, bf, warp, (B, N, C, K, H1, W1)) with ``warp`` contiguous and ``a`` / ``bf``
    in a layout the library reads well (see HipDensifier.local_corr)."""
    for name, t, nd in (("a", a, 3), ("bf", bf, 4), ("warp", warp, 4)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != nd:
            raise ValueError(f"local_corr: {name} must be a float32 tensor of {nd} dimensions")
        if t.device != device:
            raise ValueError(f"local_corr: {name} lives on {t.device}, this context computes on {device}")
    B, N, Cc = (int(v) for v in a.shape)
    H1, W1 = int(bf.shape[1]), int(bf.shape[2])
    K = int(warp.shape[2])
    if tuple(bf.shape) != (B, H1, W1, Cc) or tuple(warp.shape) != (B, N, K, 2):
        raise ValueError(f"local_corr: a {tuple(a.shape)}, bf {tuple(bf.shape)}, warp {tuple(warp.shape)} are not (B, N, C), (B, H1, W1, C), (B, N, K, 2)")
    if Cc % 4 == 0:
        # the vector kernel's layout: channels adjacent, rows of channels 16-byte aligned
        if a.stride(2) != 1 or any(s % 4 for s in a.stride()[:2]) or a.data_ptr() % 16:
            a = a.contiguous()
        if bf.stride(3) != 1 or any(s % 4 for s in bf.stride()[:3]) or bf.data_ptr() % 16:
            bf = bf.contiguous()
    return a.detach(), bf.detach(), warp.detach().contiguous(), (B, N, Cc, K, H1, W1)


def _refiner_block_call(fn, ctx, x, dw_w, scale, shift, pw_wt, pw_b, device):
    """Shapes, dtypes and device of a refiner_block call checked, the entry point ``fn`` called; (rc, out).  ``x`` (B, C, H, W) bf16 or f32 - a
    non-contiguous one is copied to contiguous NCHW first, same values -, ``dw_w`` (C, 25) or (C, 1, 5, 5), ``scale`` / ``shift`` (C), and
    either both or neither of ``pw_wt`` (C, C) and ``pw_b`` (C): f32.  Everything else is the library's to refuse."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("refiner_block: x must be a bfloat16 or float32 tensor of 4 dimensions (B, C, H, W)")
    B, Cc, H, W = (int(v) for v in x.shape)
    small = {"dw_w": (dw_w, Cc * 25), "scale": (scale, Cc), "shift": (shift, Cc)}
    if (pw_wt is None) != (pw_b is None):
        raise ValueError("refiner_block: pw_wt and pw_b must both be given or both be None")
    if pw_wt is not None:
        small.update(pw_wt=(pw_wt, Cc * Cc), pw_b=(pw_b, Cc))
    held = {}
    for name, (t, n) in small.items():
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != n:
            raise ValueError(f"refiner_block: {name} must be a float32 tensor of {n} elements for C = {Cc}")
        held[name] = t.detach().contiguous()
    for name, t in [("x", x)] + list(held.items()):
        if t.device != device:
            raise ValueError(f"refiner_block: {name} lives on {t.device}, this context computes on {device}")
    x = x.detach().contiguous()
    out = torch.empty((B, Cc, H, W), dtype=torch.bfloat16, device=device)
    ptr = lambda name: held[name].data_ptr() if name in held else None      # noqa: E731
    rc = fn(ctx, x.data_ptr(), int(x.dtype == torch.float32), B, Cc, H, W, ptr("dw_w"), ptr("scale"), ptr("shift"), ptr("pw_wt"), ptr("pw_b"),
            out.data_ptr())
    return rc, out


def _refiner_head_call(fn, ctx, z, head_w, head_b, prev_warp, prev_conf, refine_init, device):
    """Dtypes, devices and layout of a refiner_head call checked, the entry point ``fn`` called; (rc, warp, conf).  ``z`` (B, C, H, W) bf16 or
    f32, contiguous NCHW - the call exists to read z once, so another layout is refused, not copied -, ``head_w`` (6, C) and ``head_b`` (6) f32, ``prev_warp`` (B, H, W, 2)
    and ``prev_conf`` (B, H, W, 1 or 4; or None) f32 in ANY layout: they are handed over with their own strides, nothing is copied.  Shapes
    and values are the library's to refuse."""
    if not isinstance(z, torch.Tensor) or z.dim() != 4 or z.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("refiner_head: z must be a bfloat16 or float32 tensor of 4 dimensions (B, C, H, W)")
    if not z.is_contiguous():
        raise ValueError(f"refiner_head: z must be contiguous NCHW, got strides {tuple(z.stride())} for shape {tuple(z.shape)}")
    B, Cc, H, W = (int(v) for v in z.shape)
    for name, t, shape in (("head_w", head_w, (6, Cc)), ("head_b", head_b, (6,))):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise ValueError(f"refiner_head: {name} must be a float32 tensor of shape {shape} for C = {Cc}")
    for name, t in (("prev_warp", prev_warp), ("prev_conf", prev_conf)):
        if t is None and name == "prev_conf":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4 or tuple(t.shape[:3]) != (B, H, W):
            raise ValueError(f"refiner_head: {name} must be a float32 tensor of shape ({B}, {H}, {W}, D)")
    if int(prev_warp.shape[3]) != 2:
        raise ValueError(f"refiner_head: prev_warp must have 2 channels, got {int(prev_warp.shape[3])}")
    for name, t in (("z", z), ("head_w", head_w), ("head_b", head_b), ("prev_warp", prev_warp), ("prev_conf", prev_conf)):
        if t is not None and t.device != device:
            raise ValueError(f"refiner_head: {name} lives on {t.device}, this context computes on {device}")
    z, head_w, head_b, prev_warp = z.detach(), head_w.detach().contiguous(), head_b.detach().contiguous(), prev_warp.detach()
    prev_dim, pc_ptr, pc_strides = 0, None, None
    if prev_conf is not None:
        prev_conf = prev_conf.detach()
        prev_dim, pc_ptr, pc_strides = int(prev_conf.shape[3]), prev_conf.data_ptr(), (C.c_int64 * 4)(*prev_conf.stride())
    warp = torch.empty((B, H, W, 2), dtype=torch.float32, device=device)
    conf = torch.empty((B, H, W, 4), dtype=torch.float32, device=device)
    rc = fn(ctx, z.data_ptr(), int(z.dtype == torch.float32), B, Cc, H, W, head_w.data_ptr(), head_b.data_ptr(), prev_warp.data_ptr(),
            (C.c_int64 * 4)(*prev_warp.stride()), pc_ptr, pc_strides, prev_dim, float(refine_init), warp.data_ptr(), conf.data_ptr())
    return rc, warp, conf


def _cycle_gate_arguments(cert, warp_ab, warp_ba, axes, device):
    """Shapes, dtype and device of a cycle_gate call checked; (n_pairs, H, W, C, Hb, Wb, axis_x, axis_y).  The planes are handed to the library
    as they are - nothing is copied, ``cert`` may be written in place - so every one has to be a contiguous f32 tensor of ``device``."""
    cert, warp_ab, warp_ba = list(cert), list(warp_ab), list(warp_ba)
    n = len(cert)
    if n < 1 or len(warp_ab) != n or len(warp_ba) != n:
        raise ValueError("cycle_gate: one certainty, one forward and one backward warp per pair, at least one pair")
    for name, ts in (("cert", cert), ("warp_ab", warp_ab), ("warp_ba", warp_ba)):
        for t in ts:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"cycle_gate: {name} must hold contiguous float32 tensors")
            if t.device != device:
                raise ValueError(f"cycle_gate: {name} lives on {t.device}, this context computes on {device}")
    if cert[0].dim() != 2 or warp_ab[0].dim() != 3 or warp_ba[0].dim() != 3:
        raise ValueError("cycle_gate: cert (H, W), warp_ab (H, W, C), warp_ba (Hb, Wb, 2)")
    H, W = (int(v) for v in cert[0].shape)
    Cc = int(warp_ab[0].shape[-1])
    Hb, Wb = int(warp_ba[0].shape[0]), int(warp_ba[0].shape[1])
    for c, wa, wb in zip(cert, warp_ab, warp_ba):
        if tuple(c.shape) != (H, W) or tuple(wa.shape) != (H, W, Cc) or tuple(wb.shape) != (Hb, Wb, 2):
            raise ValueError(f"cycle_gate: cert {tuple(c.shape)}, warp_ab {tuple(wa.shape)}, warp_ba {tuple(wb.shape)} are not (H, W), (H, W, C), (Hb, Wb, 2) "
                             "of one size for all pairs")
    ax = ay = None
    if axes is not None:
        ax, ay = (torch.as_tensor(a).to(device, torch.float32).contiguous() for a in axes)
        if tuple(ax.shape) != (W,) or tuple(ay.shape) != (H,):
            raise ValueError("cycle_gate: axes must be (axis_x [W], axis_y [H])")
    return n, H, W, Cc, Hb, Wb, ax, ay


def _cycle_gate_call(fn, ctx, cert, warp_ab, warp_ba, w_match, h_match, certainty_thresh, cycle_thresh_px, axes, inplace, with_err, rejected, device):
    n, H, W, Cc, Hb, Wb, ax, ay = _cycle_gate_arguments(cert, warp_ab, warp_ba, axes, device)
    if rejected is not None and (not isinstance(rejected, torch.Tensor) or rejected.dtype != torch.int32 or rejected.device != device
                                 or not rejected.is_contiguous() or rejected.numel() < n):
        raise ValueError("cycle_gate: rejected must be a contiguous int32 tensor of this context's device with one element per pair")
    outs = list(cert) if inplace else [torch.empty_like(c) for c in cert]
    errs = [torch.empty_like(c) for c in cert] if with_err else None
    table = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    rc = fn(ctx, n, table(cert), table(warp_ab), table(warp_ba), H, W, Cc, Hb, Wb, ax.data_ptr() if ax is not None else None,
            ay.data_ptr() if ay is not None else None, int(w_match), int(h_match), float(certainty_thresh), float(cycle_thresh_px), table(outs),
            table(errs) if errs is not None else None, rejected.data_ptr() if rejected is not None else None)
    return rc, outs, errs


def _support_filter_call(fn, ctx, batch, src, min_support, support_thresh_px, with_support, into, device):
    """One lfd_support_filter[_host] call.  ``src``: the OutputBuffers a triangulation launch wrote for ``batch`` (asynchronous: the result is
    another OutputBuffers - ``into``, or a new one - whose small integer outputs are the source's with the offsets and counts replaced), or a
    collected TriangulationOutput (the result is collected as well).  Returns (rc, result or None, support or None)."""
    if not isinstance(min_support, (int, np.integer)) or isinstance(min_support, bool):
        raise ValueError("support_filter: min_support must be an integer")
    collected = isinstance(src, TriangulationOutput)
    if src.cell is None or src.slot is None:
        raise ValueError("support_filter: the source buffers need the cell / slot outputs (with_cell=True)")
    if collected:
        n = int(src.xyz.shape[0])
        keep = [src.xyz.contiguous(), src.rgb.contiguous(), src.err.contiguous(), src.cell.contiguous(), src.slot.contiguous()]
        if n == 0:                            # (an empty tensor may have no address at all; the library wants its arrays)
            keep = [torch.zeros((1, 3) if t.dim() == 2 else (1,), dtype=t.dtype, device=t.device) for t in keep]
        if any(t.device != device for t in keep):
            raise ValueError(f"support_filter: the points live on {keep[0].device}, this context computes on {device}")
        offs_in = torch.from_numpy(np.ascontiguousarray(src.ref_offsets, np.int64)).to(device)
        pts_in = lfd_points(xyz=keep[0].data_ptr(), rgb=keep[1].data_ptr(), err=keep[2].data_ptr(), cell=keep[3].data_ptr(), slot=keep[4].data_ptr(),
                            capacity=n)
        n_refs, k, cap = int(len(src.ref_offsets)) - 1, int(src.seg_counts.shape[1]), n
    else:
        if src.xyz.device != device:
            raise ValueError(f"support_filter: the points live on {src.xyz.device}, this context computes on {device}")
        keep, offs_in, pts_in, n_refs, k, cap = [], src.ref_offsets, src.c, src._n_refs, src._k, src.capacity
    if n_refs != batch.n_refs or k != batch.k:
        raise ValueError(f"support_filter: the points were made for {n_refs} references x {k} slots, the batch has {batch.n_refs} x {batch.k}")
    dst = into if into is not None else OutputBuffers(cap, n_refs, k, device, True, True if collected else src.with_segments)
    if dst.capacity < cap or dst._n_refs != n_refs or dst._k != k or dst.xyz.device != device:
        raise ValueError("support_filter: `into` must have the source's capacity, references and slots, on this context's device")
    dst.normals_valid = False                 # (refilled: normals an earlier estimate wrote there belong to other points)
    if not collected:
        dst._meta.copy_(src._meta)            # group order, selection and launch status travel with the points
        dst.support_in.copy_(src.ref_offsets[-1:])
        dst.filtered = True
    support = torch.empty((max(cap, 1),), dtype=torch.uint8, device=device) if with_support else None
    rc = fn(ctx, C.byref(batch.c), C.byref(pts_in), offs_in.data_ptr(), int(min_support), C.c_float(float(support_thresh_px)), C.byref(dst.c),
            dst.ref_offsets.data_ptr(), dst.seg_counts.data_ptr() if dst.with_segments else None, support.data_ptr() if with_support else None)
    if rc != 0:
        return rc, None, None
    if with_support:
        support = support[:cap]
    if not collected:
        return rc, dst, support
    res = dst.collect()
    res.support_in = n
    res.seg_order = None
    res.n_selected, res.sel_status, res.launch_status = src.n_selected, src.sel_status, src.launch_status
    return rc, res, support


def _refine_call(fn, ctx, batch, src, support_thresh_px, reproj_thresh, with_status, counters, device, precision=False):
    """One lfd_refine_multiview[_host] call.  ``src``: the OutputBuffers a triangulation launch (or the support filter) wrote for ``batch`` -
    refined IN PLACE, asynchronously, and returned - or a collected TriangulationOutput (the result is a copy with new xyz / err tensors).
    ``counters``: None, or an int64 [2] tensor on the context's device that is added to ([3] with ``precision``: fn is then
    lfd_refine_multiview_weighted[_host] and the batch's precision table its last argument).  Returns (rc, result or None, status or None)."""
    collected = isinstance(src, TriangulationOutput)
    n_counters = 3 if precision else 2
    if precision and batch.precision is None:
        raise ValueError("refine_multiview: precision=True needs a batch whose references carry precision planes (ReferenceInputs.precision)")
    if src.cell is None or src.slot is None:
        raise ValueError("refine_multiview: the source buffers need the cell / slot outputs (with_cell=True)")
    if counters is not None and (counters.dtype != torch.int64 or counters.numel() != n_counters or counters.device != device or not counters.is_contiguous()):
        raise ValueError(f"refine_multiview: counters must be a contiguous int64 tensor of {'three' if precision else 'two'} elements on {device}")
    if collected:
        n = int(src.xyz.shape[0])
        keep = [src.xyz.contiguous(), src.err.contiguous(), src.cell.contiguous(), src.slot.contiguous()]
        if n == 0:                            # (an empty tensor may have no address at all; the library wants its arrays)
            keep = [torch.zeros((1, 3) if t.dim() == 2 else (1,), dtype=t.dtype, device=t.device) for t in keep]
        if any(t.device != device for t in keep):
            raise ValueError(f"refine_multiview: the points live on {keep[0].device}, this context computes on {device}")
        offs = torch.from_numpy(np.ascontiguousarray(src.ref_offsets, np.int64)).to(device)
        pts = lfd_points(xyz=keep[0].data_ptr(), rgb=None, err=keep[1].data_ptr(), cell=keep[2].data_ptr(), slot=keep[3].data_ptr(), capacity=n)
        n_refs, k, cap = int(len(src.ref_offsets)) - 1, int(src.seg_counts.shape[1]), n
        xyz_out = torch.empty((max(n, 1), 3), dtype=torch.float32, device=device)
        err_out = torch.empty((max(n, 1),), dtype=torch.float32, device=device)
    else:
        if src.xyz.device != device:
            raise ValueError(f"refine_multiview: the points live on {src.xyz.device}, this context computes on {device}")
        keep, offs, pts, n_refs, k, cap = [], src.ref_offsets, src.c, src._n_refs, src._k, src.capacity
        xyz_out, err_out = src.xyz, src.err
        src.normals_valid = False             # (the points move: normals estimated before belong to the old positions)
    if n_refs != batch.n_refs or k != batch.k:
        raise ValueError(f"refine_multiview: the points were made for {n_refs} references x {k} slots, the batch has {batch.n_refs} x {batch.k}")
    status = torch.zeros((max(cap, 1),), dtype=torch.uint8, device=device) if with_status else None
    rc = fn(ctx, C.byref(batch.c), C.byref(pts), offs.data_ptr(), C.c_float(float(support_thresh_px)), C.c_float(float(reproj_thresh)),
            xyz_out.data_ptr(), err_out.data_ptr(), status.data_ptr() if with_status else None, counters.data_ptr() if counters is not None else None,
            *((C.cast(batch.precision, C.c_void_p),) if precision else ()))
    if rc != 0:
        return rc, None, None
    if with_status:
        status = status[:cap]
    if not collected:
        return rc, src, status
    return rc, dataclasses.replace(src, xyz=xyz_out[:cap], err=err_out[:cap], _packed=None), status


def _normals_call(fn, ctx, batch, src, radius, depth_step_rel, reproj_thresh, with_status, counters, device):
    """One lfd_estimate_normals[_host] call.  ``src``: the OutputBuffers a triangulation launch or a post-stage wrote for ``batch`` - their
    ``normals`` tensor is allocated on first use and written asynchronously, the buffers are returned - or a collected TriangulationOutput (the
    result is a copy that carries ``normals``).  ``counters``: None, or an int64 [2] tensor on the context's device that is added to (fitted,
    fell back).  Returns (rc, result or None, status or None)."""
    if not isinstance(radius, (int, np.integer)) or isinstance(radius, bool):
        raise ValueError("estimate_normals: radius must be an integer")
    collected = isinstance(src, TriangulationOutput)
    if src.cell is None or src.slot is None:
        raise ValueError("estimate_normals: the source buffers need the cell / slot outputs (with_cell=True)")
    if counters is not None and (counters.dtype != torch.int64 or counters.numel() != 2 or counters.device != device or not counters.is_contiguous()):
        raise ValueError(f"estimate_normals: counters must be a contiguous int64 tensor of two elements on {device}")
    if collected:
        n = int(src.xyz.shape[0])
        keep = [src.xyz.contiguous(), src.cell.contiguous(), src.slot.contiguous()]
        if n == 0:                            # (an empty tensor may have no address at all; the library wants its arrays)
            keep = [torch.zeros((1, 3) if t.dim() == 2 else (1,), dtype=t.dtype, device=t.device) for t in keep]
        if any(t.device != device for t in keep):
            raise ValueError(f"estimate_normals: the points live on {keep[0].device}, this context computes on {device}")
        offs = torch.from_numpy(np.ascontiguousarray(src.ref_offsets, np.int64)).to(device)
        pts = lfd_points(xyz=keep[0].data_ptr(), rgb=None, err=None, cell=keep[1].data_ptr(), slot=keep[2].data_ptr(), capacity=n)
        n_refs, k, cap = int(len(src.ref_offsets)) - 1, int(src.seg_counts.shape[1]), n
        normals = torch.empty((max(n, 1), 3), dtype=torch.float32, device=device)
    else:
        if src.xyz.device != device:
            raise ValueError(f"estimate_normals: the points live on {src.xyz.device}, this context computes on {device}")
        keep, offs, pts, n_refs, k, cap = [], src.ref_offsets, src.c, src._n_refs, src._k, src.capacity
        if src.normals is None:
            src.normals = torch.empty((max(cap, 1), 3), dtype=torch.float32, device=device)
        normals = src.normals
        src.normals_valid = False
    if n_refs != batch.n_refs or k != batch.k:
        raise ValueError(f"estimate_normals: the points were made for {n_refs} references x {k} slots, the batch has {batch.n_refs} x {batch.k}")
    status = torch.zeros((max(cap, 1),), dtype=torch.uint8, device=device) if with_status else None
    rc = fn(ctx, C.byref(batch.c), C.byref(pts), offs.data_ptr(), int(radius), C.c_float(float(depth_step_rel)), C.c_float(float(reproj_thresh)),
            normals.data_ptr(), status.data_ptr() if with_status else None, counters.data_ptr() if counters is not None else None)
    if rc != 0:
        return rc, None, None
    if with_status:
        status = status[:cap]
    if not collected:
        src.normals_valid = True
        return rc, src, status
    return rc, dataclasses.replace(src, normals=normals[:cap]), status


COLOUR_MODES = {"mean": 1, "median": 2}      # LFD_COLOUR_MEAN, LFD_COLOUR_MEDIAN of include/lfd_densify.h


def _colour_call(fn, ctx, batch, src, support_thresh_px, mode, with_status, counters, device):
    """One lfd_colour_multiview[_host] call.  ``src``: the OutputBuffers a triangulation launch or a post-stage wrote for ``batch`` - their
    ``rgb`` is rewritten IN PLACE, asynchronously, and the buffers are returned - or a collected TriangulationOutput (the result is a copy
    with a new rgb tensor).  ``mode``: "mean" or "median".  ``counters``: None, or an int64 [2] tensor on the context's device that is added
    to (points blended, the sum of their views).  Returns (rc, result or None, status or None)."""
    if mode not in COLOUR_MODES:
        raise ValueError("colour_multiview: mode must be 'mean' or 'median'")
    if batch.nbr_images is None:
        raise ValueError("colour_multiview: the batch's references carry no neighbour images (ReferenceInputs.nbr_images)")
    collected = isinstance(src, TriangulationOutput)
    if src.cell is None or src.slot is None:
        raise ValueError("colour_multiview: the source buffers need the cell / slot outputs (with_cell=True)")
    if counters is not None and (counters.dtype != torch.int64 or counters.numel() != 2 or counters.device != device or not counters.is_contiguous()):
        raise ValueError(f"colour_multiview: counters must be a contiguous int64 tensor of two elements on {device}")
    if collected:
        n = int(src.xyz.shape[0])
        keep = [src.xyz.contiguous(), src.rgb.contiguous(), src.cell.contiguous(), src.slot.contiguous()]
        if n == 0:                            # (an empty tensor may have no address at all; the library wants its arrays)
            keep = [torch.zeros((1, 3) if t.dim() == 2 else (1,), dtype=t.dtype, device=t.device) for t in keep]
        if any(t.device != device for t in keep):
            raise ValueError(f"colour_multiview: the points live on {keep[0].device}, this context computes on {device}")
        offs = torch.from_numpy(np.ascontiguousarray(src.ref_offsets, np.int64)).to(device)
        pts = lfd_points(xyz=keep[0].data_ptr(), rgb=keep[1].data_ptr(), err=None, cell=keep[2].data_ptr(), slot=keep[3].data_ptr(), capacity=n)
        n_refs, k, cap = int(len(src.ref_offsets)) - 1, int(src.seg_counts.shape[1]), n
        rgb_out = torch.empty((max(n, 1), 3), dtype=torch.float32, device=device)
    else:
        if src.xyz.device != device:
            raise ValueError(f"colour_multiview: the points live on {src.xyz.device}, this context computes on {device}")
        keep, offs, pts, n_refs, k, cap = [], src.ref_offsets, src.c, src._n_refs, src._k, src.capacity
        rgb_out = src.rgb
    if n_refs != batch.n_refs or k != batch.k:
        raise ValueError(f"colour_multiview: the points were made for {n_refs} references x {k} slots, the batch has {batch.n_refs} x {batch.k}")
    status = torch.zeros((max(cap, 1),), dtype=torch.uint8, device=device) if with_status else None
    rc = fn(ctx, C.byref(batch.c), C.byref(pts), offs.data_ptr(), C.cast(batch.nbr_images, C.c_void_p), C.c_float(float(support_thresh_px)),
            int(COLOUR_MODES[mode]), rgb_out.data_ptr(), status.data_ptr() if with_status else None,
            counters.data_ptr() if counters is not None else None)
    if rc != 0:
        return rc, None, None
    if with_status:
        status = status[:cap]
    if not collected:
        return rc, src, status
    return rc, dataclasses.replace(src, rgb=rgb_out[:cap], _packed=None), status


GAIN_QUANTITIES = 7                          # LFD_GAIN_QUANTITIES of csrc/lfd_gain.hpp: N, Sref[3], Snbr[3] per (reference, slot)


def _gain_accumulate_call(fn, ctx, batch, src, support_thresh_px, table, device):
    """One lfd_gain_accumulate[_host] call.  ``src``: the OutputBuffers a launch or a post-stage wrote for ``batch``, or a collected
    TriangulationOutput; nothing of it changes.  ``table``: None (a zeroed one is made) or a contiguous int64 (n_refs * k, 7) tensor on the
    context's device - the library's u64 sums, far below 2^63 - that is ADDED to.  Returns (rc, table)."""
    if batch.nbr_images is None:
        raise ValueError("gain_accumulate: the batch's references carry no neighbour images (ReferenceInputs.nbr_images)")
    if src.cell is None or src.slot is None:
        raise ValueError("gain_accumulate: the source buffers need the cell / slot outputs (with_cell=True)")
    rows = batch.n_refs * batch.k
    if table is None:
        table = torch.zeros((rows, GAIN_QUANTITIES), dtype=torch.int64, device=device)
    elif table.dtype != torch.int64 or tuple(table.shape) != (rows, GAIN_QUANTITIES) or table.device != device or not table.is_contiguous():
        raise ValueError(f"gain_accumulate: table must be a contiguous int64 ({rows}, {GAIN_QUANTITIES}) tensor on {device}")
    if isinstance(src, TriangulationOutput):
        n = int(src.xyz.shape[0])
        keep = [src.xyz.contiguous(), src.rgb.contiguous(), src.cell.contiguous(), src.slot.contiguous()]
        if n == 0:                            # (an empty tensor may have no address at all; the library wants its arrays)
            keep = [torch.zeros((1, 3) if t.dim() == 2 else (1,), dtype=t.dtype, device=t.device) for t in keep]
        if any(t.device != device for t in keep):
            raise ValueError(f"gain_accumulate: the points live on {keep[0].device}, this context computes on {device}")
        offs = torch.from_numpy(np.ascontiguousarray(src.ref_offsets, np.int64)).to(device)
        pts = lfd_points(xyz=keep[0].data_ptr(), rgb=keep[1].data_ptr(), err=None, cell=keep[2].data_ptr(), slot=keep[3].data_ptr(), capacity=n)
        n_refs, k = int(len(src.ref_offsets)) - 1, int(src.seg_counts.shape[1])
    else:
        if src.xyz.device != device:
            raise ValueError(f"gain_accumulate: the points live on {src.xyz.device}, this context computes on {device}")
        keep, offs, pts, n_refs, k = [], src.ref_offsets, src.c, src._n_refs, src._k
    if n_refs != batch.n_refs or k != batch.k:
        raise ValueError(f"gain_accumulate: the points were made for {n_refs} references x {k} slots, the batch has {batch.n_refs} x {batch.k}")
    rc = fn(ctx, C.byref(batch.c), C.byref(pts), offs.data_ptr(), C.cast(batch.nbr_images, C.c_void_p), C.c_float(float(support_thresh_px)),
            table.data_ptr())
    del keep
    return rc, table


FAR_QUANTITIES = 7                           # LFD_FAR_QUANTITIES of csrc/lfd_far.hpp: direction sum [3], colour sum [3], count per direction cell


def far_table(shell_cells: int, device) -> torch.Tensor:
    """A zeroed table of the far-field shell: int64 (6 * S * S, 7) - the library's u64 sums, the direction columns two's complement."""
    return torch.zeros((6 * int(shell_cells) * int(shell_cells), FAR_QUANTITIES), dtype=torch.int64, device=device)


def _far_accumulate_call(fn, ctx, batch, far_thresh_px, far_certainty, far_min_views, shell_cells, table, counters, device, flags=None):
    """One lfd_far_accumulate[_flags][_host] call.  ``table``: None (a zeroed one is made) or a contiguous int64 (6 S S, 7) tensor where the
    context computes, ADDED to; ``counters``: None or a contiguous int64 (n_refs,) tensor there, added to; ``flags`` (the _flags calls): a
    contiguous uint8 (n_refs, H * W) tensor there, written.  Returns (rc, table)."""
    S = int(shell_cells)
    rows = 6 * S * S
    if table is None:
        table = far_table(S, device)
    elif table.dtype != torch.int64 or tuple(table.shape) != (rows, FAR_QUANTITIES) or table.device != device or not table.is_contiguous():
        raise ValueError(f"far_accumulate: table must be a contiguous int64 ({rows}, {FAR_QUANTITIES}) tensor on {device}")
    if counters is not None and (counters.dtype != torch.int64 or tuple(counters.shape) != (batch.n_refs,) or counters.device != device
                                 or not counters.is_contiguous()):
        raise ValueError(f"far_accumulate: counters must be a contiguous int64 ({batch.n_refs},) tensor on {device}")
    args = [ctx, C.byref(batch.c), C.c_float(float(far_thresh_px)), C.c_float(float(far_certainty)), int(far_min_views), S, table.data_ptr(),
            counters.data_ptr() if counters is not None else None]
    if flags is not None:
        if flags.dtype != torch.uint8 or tuple(flags.shape) != (batch.n_refs, batch.H * batch.W) or flags.device != device or not flags.is_contiguous():
            raise ValueError(f"far_accumulate: flags must be a contiguous uint8 ({batch.n_refs}, {batch.H * batch.W}) tensor on {device}")
        args.append(flags.data_ptr())
    rc = fn(*args)
    return rc, table


AUDIT_QUANTITIES = 66                        # LFD_AUDIT_QUANTITIES of csrc/lfd_audit.hpp: usable, degenerate, 64 bins of 1/8 px per (reference, slot)
AUDIT_NONE = 255                             # the cell map's "no usable confident slot"


def audit_table(n_refs: int, k: int, device) -> torch.Tensor:
    """A zeroed table of the epipolar audit: int64 (n_refs * k, 66) - the library's u64 counts, far below 2^63."""
    return torch.zeros((int(n_refs) * int(k), AUDIT_QUANTITIES), dtype=torch.int64, device=device)


def _epipolar_audit_call(fn, ctx, batch, audit_certainty, table, best, device):
    """One lfd_epipolar_audit[_host] call.  ``table``: None (a zeroed one is made) or a contiguous int64 (n_refs * k, 66) tensor where the
    context computes, ADDED to; ``best``: None or a contiguous uint8 (n_refs, H * W) tensor there, written.  Returns (rc, table)."""
    rows = batch.n_refs * batch.k
    if table is None:
        table = audit_table(batch.n_refs, batch.k, device)
    elif table.dtype != torch.int64 or tuple(table.shape) != (rows, AUDIT_QUANTITIES) or table.device != device or not table.is_contiguous():
        raise ValueError(f"epipolar_audit: table must be a contiguous int64 ({rows}, {AUDIT_QUANTITIES}) tensor on {device}")
    if best is not None and (best.dtype != torch.uint8 or tuple(best.shape) != (batch.n_refs, batch.H * batch.W) or best.device != device
                             or not best.is_contiguous()):
        raise ValueError(f"epipolar_audit: best must be a contiguous uint8 ({batch.n_refs}, {batch.H * batch.W}) tensor on {device}")
    rc = fn(ctx, C.byref(batch.c), C.c_float(float(audit_certainty)), table.data_ptr(), best.data_ptr() if best is not None else None)
    return rc, table


POSE_QUANTITIES = 32                         # LFD_POSE_QUANTITIES of csrc/lfd_pose.hpp: inliers, outliers, degenerate, 28 signed sums, one unused, per (reference, slot)


def pose_table(n_refs: int, k: int, device) -> torch.Tensor:
    """A zeroed table of the pose refinement: int64 (n_refs * k, 32) - the normal equations of one Gauss-Newton step per pair, as integers."""
    return torch.zeros((int(n_refs) * int(k), POSE_QUANTITIES), dtype=torch.int64, device=device)


def _pose_accumulate_call(fn, ctx, batch, pose_certainty, pose_inlier_px, table, device):
    """One lfd_pose_accumulate[_host] call.  ``table``: None (a zeroed one is made) or a contiguous int64 (n_refs * k, 32) tensor where the
    context computes, ADDED to.  Returns (rc, table)."""
    rows = batch.n_refs * batch.k
    if table is None:
        table = pose_table(batch.n_refs, batch.k, device)
    elif table.dtype != torch.int64 or tuple(table.shape) != (rows, POSE_QUANTITIES) or table.device != device or not table.is_contiguous():
        raise ValueError(f"pose_accumulate: table must be a contiguous int64 ({rows}, {POSE_QUANTITIES}) tensor on {device}")
    rc = fn(ctx, C.byref(batch.c), C.c_float(float(pose_certainty)), C.c_float(float(pose_inlier_px)), table.data_ptr())
    return rc, table


def _far_emit_call(fn, ctx, table, shell_cells, min_samples, centre, radius, with_normals, capacity, device):
    """One lfd_far_emit[_host] call.  Returns (rc, n_out, xyz, rgb, normals or None, samples): the tensors hold min(n_out, capacity) records.
    ``capacity`` None: the number of direction cells that reach ``min_samples`` (an upper bound of what is emitted)."""
    S = int(shell_cells)
    if table.dtype != torch.int64 or tuple(table.shape) != (6 * S * S, FAR_QUANTITIES) or table.device != device or not table.is_contiguous():
        raise ValueError(f"far_emit: table must be a contiguous int64 ({6 * S * S}, {FAR_QUANTITIES}) tensor on {device}")
    cap = int((table[:, 6] >= int(min_samples)).sum().item()) if capacity is None else int(capacity)
    alloc = max(cap, 1)
    xyz = torch.empty((alloc, 3), dtype=torch.float32, device=device)
    rgb = torch.empty((alloc, 3), dtype=torch.float32, device=device)
    nrm = torch.empty((alloc, 3), dtype=torch.float32, device=device) if with_normals else None
    smp = torch.empty((alloc,), dtype=torch.int32, device=device)
    c3 = (C.c_double * 3)(*[float(v) for v in np.asarray(centre, np.float64).reshape(3)])
    n_out = C.c_int64(0)
    rc = fn(ctx, table.data_ptr(), S, int(min_samples), c3, C.c_double(float(radius)), xyz.data_ptr(), rgb.data_ptr(),
            nrm.data_ptr() if nrm is not None else None, smp.data_ptr(), cap, C.byref(n_out))
    n = min(int(n_out.value), cap)
    return rc, int(n_out.value), xyz[:n], rgb[:n], (nrm[:n] if nrm is not None else None), smp[:n]


def _gain_apply_call(fn, ctx, rgb, ref_counts, factors, device):
    """One lfd_gain_apply[_host] call.  ``rgb`` (n, 3) float32 where the context computes; ``ref_counts``: points per reference, in the order
    of the cloud; ``factors`` (n_refs, 3) float32 (array or tensor).  Returns (rc, a new (n, 3) tensor)."""
    counts = np.ascontiguousarray(np.asarray(ref_counts, np.int64).reshape(-1))
    n = int(rgb.shape[0])
    if rgb.dtype != torch.float32 or rgb.dim() != 2 or rgb.shape[1] != 3 or rgb.device != device:
        raise ValueError(f"gain_apply: rgb must be a float32 (n, 3) tensor on {device}")
    if counts.size < 1 or (counts < 0).any() or int(counts.sum()) != n:
        raise ValueError(f"gain_apply: ref_counts must be non-negative counts, one per reference, that add up to the {n} points")
    f = torch.as_tensor(np.ascontiguousarray(np.asarray(factors.cpu() if isinstance(factors, torch.Tensor) else factors, np.float32)))
    if tuple(f.shape) != (counts.size, 3):
        raise ValueError(f"gain_apply: factors must be ({counts.size}, 3) float32, one row per reference")
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to(device)
    f = f.to(device)
    src = rgb.contiguous()
    out = torch.empty((max(n, 1), 3), dtype=torch.float32, device=device)
    if n == 0:
        return 0, out[:0]
    rc = fn(ctx, src.data_ptr(), n, offs.data_ptr(), int(counts.size), f.data_ptr(), out.data_ptr())
    return rc, out[:n]


def _depth_sigma_call(fn, ctx, batch, src, max_rel_sigma, iso_sigma_px, refine_status, support_thresh_px, with_sigma, into, device):
    """One lfd_depth_sigma_filter[_host] call.  ``src``, ``into`` and the result: as in ``_support_filter_call``.  ``iso_sigma_px`` > 0: the
    isotropic form; 0: the batch's precision planes.  ``refine_status``: None (the winner alone places a point) or the uint8 status tensor of
    the re-triangulation that just ran over ``src``.  Returns (rc, result or None, sigma_rel of the input points or None, compacted sigma_rel
    or None)."""
    collected = isinstance(src, TriangulationOutput)
    iso_sigma_px = float(iso_sigma_px)
    if iso_sigma_px == 0.0 and batch.precision is None:
        raise ValueError("depth_sigma_filter: iso_sigma_px=0 needs a batch whose references carry precision planes (ReferenceInputs.precision)")
    if src.cell is None or src.slot is None:
        raise ValueError("depth_sigma_filter: the source buffers need the cell / slot outputs (with_cell=True)")
    if collected:
        n = int(src.xyz.shape[0])
        keep = [src.xyz.contiguous(), src.rgb.contiguous(), src.err.contiguous(), src.cell.contiguous(), src.slot.contiguous()]
        if n == 0:                            # (an empty tensor may have no address at all; the library wants its arrays)
            keep = [torch.zeros((1, 3) if t.dim() == 2 else (1,), dtype=t.dtype, device=t.device) for t in keep]
        if any(t.device != device for t in keep):
            raise ValueError(f"depth_sigma_filter: the points live on {keep[0].device}, this context computes on {device}")
        offs_in = torch.from_numpy(np.ascontiguousarray(src.ref_offsets, np.int64)).to(device)
        pts_in = lfd_points(xyz=keep[0].data_ptr(), rgb=keep[1].data_ptr(), err=keep[2].data_ptr(), cell=keep[3].data_ptr(), slot=keep[4].data_ptr(),
                            capacity=n)
        n_refs, k, cap = int(len(src.ref_offsets)) - 1, int(src.seg_counts.shape[1]), n
    else:
        if src.xyz.device != device:
            raise ValueError(f"depth_sigma_filter: the points live on {src.xyz.device}, this context computes on {device}")
        keep, offs_in, pts_in, n_refs, k, cap = [], src.ref_offsets, src.c, src._n_refs, src._k, src.capacity
    if n_refs != batch.n_refs or k != batch.k:
        raise ValueError(f"depth_sigma_filter: the points were made for {n_refs} references x {k} slots, the batch has {batch.n_refs} x {batch.k}")
    if refine_status is not None and (refine_status.dtype != torch.uint8 or refine_status.device != device or not refine_status.is_contiguous()
                                      or int(refine_status.numel()) < cap):
        raise ValueError(f"depth_sigma_filter: refine_status must be a contiguous uint8 tensor of at least {cap} elements on {device}")
    dst = into if into is not None else OutputBuffers(cap, n_refs, k, device, True, True if collected else src.with_segments)
    if dst.capacity < cap or dst._n_refs != n_refs or dst._k != k or dst.xyz.device != device:
        raise ValueError("depth_sigma_filter: `into` must have the source's capacity, references and slots, on this context's device")
    dst.normals_valid = False                 # (refilled: normals an earlier estimate wrote there belong to other points)
    if not collected:
        dst._meta.copy_(src._meta)            # group order, selection and launch status (and the support filter's count) travel with the points
        dst.sigma_in.copy_(src.ref_offsets[-1:])
        dst.filtered, dst.sigma_filtered = bool(src.filtered), True
    sigma = torch.empty((max(cap, 1),), dtype=torch.float32, device=device) if with_sigma else None
    sigma_out = torch.empty((max(dst.capacity, 1),), dtype=torch.float32, device=device) if with_sigma else None
    rc = fn(ctx, C.byref(batch.c), C.byref(pts_in), offs_in.data_ptr(), C.cast(batch.precision, C.c_void_p) if iso_sigma_px == 0.0 else None,
            C.c_float(iso_sigma_px), refine_status.data_ptr() if refine_status is not None else None, C.c_float(float(support_thresh_px)),
            C.c_float(float(max_rel_sigma)), C.byref(dst.c), dst.ref_offsets.data_ptr(), dst.seg_counts.data_ptr() if dst.with_segments else None,
            sigma.data_ptr() if with_sigma else None, sigma_out.data_ptr() if with_sigma else None)
    if rc != 0:
        return rc, None, None, None
    if with_sigma:
        sigma = sigma[:cap]
    if not collected:
        return rc, dst, sigma, sigma_out
    res = dst.collect()
    res.sigma_in = n
    res.seg_order = None
    res.n_selected, res.sel_status, res.launch_status = src.n_selected, src.sel_status, src.launch_status
    return rc, res, sigma, (sigma_out[:res.count] if with_sigma else None)


PHOTO_STATUSES = 5                           # LFD_PHOTO_STATUSES of csrc/lfd_photo.hpp: guarded, sparse window, untextured, consistent, refuted


def _photo_gate_call(fn, ctx, batch, src, window_cells, min_ncc, min_texture, with_status, with_ncc, counters, into, device):
    """One lfd_photo_gate[_host] call.  ``src``, ``into`` and the result: as in ``_support_filter_call``.  ``counters``: None, or an int64 [5]
    tensor on the context's device that is added to (points per status 0..4).  Returns (rc, result or None, uint8 status of the input points
    or None, f32 ncc of the input points or None)."""
    if not isinstance(window_cells, (int, np.integer)) or isinstance(window_cells, bool):
        raise ValueError("photo_gate: window_cells must be an integer")
    if batch.nbr_images is None:
        raise ValueError("photo_gate: the batch's references carry no neighbour images (ReferenceInputs.nbr_images)")
    collected = isinstance(src, TriangulationOutput)
    if src.cell is None or src.slot is None:
        raise ValueError("photo_gate: the source buffers need the cell / slot outputs (with_cell=True)")
    if counters is not None and (counters.dtype != torch.int64 or counters.numel() != PHOTO_STATUSES or counters.device != device
                                 or not counters.is_contiguous()):
        raise ValueError(f"photo_gate: counters must be a contiguous int64 tensor of five elements on {device}")
    if collected:
        n = int(src.xyz.shape[0])
        keep = [src.xyz.contiguous(), src.rgb.contiguous(), src.err.contiguous(), src.cell.contiguous(), src.slot.contiguous()]
        if n == 0:                            # (an empty tensor may have no address at all; the library wants its arrays)
            keep = [torch.zeros((1, 3) if t.dim() == 2 else (1,), dtype=t.dtype, device=t.device) for t in keep]
        if any(t.device != device for t in keep):
            raise ValueError(f"photo_gate: the points live on {keep[0].device}, this context computes on {device}")
        offs_in = torch.from_numpy(np.ascontiguousarray(src.ref_offsets, np.int64)).to(device)
        pts_in = lfd_points(xyz=keep[0].data_ptr(), rgb=keep[1].data_ptr(), err=keep[2].data_ptr(), cell=keep[3].data_ptr(), slot=keep[4].data_ptr(),
                            capacity=n)
        n_refs, k, cap = int(len(src.ref_offsets)) - 1, int(src.seg_counts.shape[1]), n
    else:
        if src.xyz.device != device:
            raise ValueError(f"photo_gate: the points live on {src.xyz.device}, this context computes on {device}")
        keep, offs_in, pts_in, n_refs, k, cap = [], src.ref_offsets, src.c, src._n_refs, src._k, src.capacity
    if n_refs != batch.n_refs or k != batch.k:
        raise ValueError(f"photo_gate: the points were made for {n_refs} references x {k} slots, the batch has {batch.n_refs} x {batch.k}")
    dst = into if into is not None else OutputBuffers(cap, n_refs, k, device, True, True if collected else src.with_segments)
    if dst.capacity < cap or dst._n_refs != n_refs or dst._k != k or dst.xyz.device != device:
        raise ValueError("photo_gate: `into` must have the source's capacity, references and slots, on this context's device")
    dst.normals_valid = False                 # (refilled: normals an earlier estimate wrote there belong to other points)
    if not collected:
        dst._meta.copy_(src._meta)            # group order, selection and launch status and the earlier filters' counts travel with the points
        dst.photo_in.copy_(src.ref_offsets[-1:])
        dst.filtered, dst.sigma_filtered, dst.photo_filtered = bool(src.filtered), bool(src.sigma_filtered), True
    status = torch.zeros((max(cap, 1),), dtype=torch.uint8, device=device) if with_status else None
    ncc = torch.full((max(cap, 1),), float("nan"), dtype=torch.float32, device=device) if with_ncc else None
    rc = fn(ctx, C.byref(batch.c), C.byref(pts_in), offs_in.data_ptr(), C.cast(batch.nbr_images, C.c_void_p), int(window_cells),
            C.c_float(float(min_ncc)), C.c_float(float(min_texture)), C.byref(dst.c), dst.ref_offsets.data_ptr(),
            dst.seg_counts.data_ptr() if dst.with_segments else None, status.data_ptr() if with_status else None,
            ncc.data_ptr() if with_ncc else None, counters.data_ptr() if counters is not None else None)
    del keep
    if rc != 0:
        return rc, None, None, None
    if with_status:
        status = status[:cap]
    if with_ncc:
        ncc = ncc[:cap]
    if not collected:
        return rc, dst, status, ncc
    res = dst.collect()
    res.support_in, res.sigma_in, res.photo_in = src.support_in, src.sigma_in, n
    res.seg_order = None
    res.n_selected, res.sel_status, res.launch_status = src.n_selected, src.sel_status, src.launch_status
    return rc, res, status, ncc


def _consensus_call(fn, ctx, what, xyz, rgb, err, ref_counts, radius, min_refs, with_consensus, device, last_error):
    """One lfd_consensus_filter[_host] call.  ``xyz`` (n, 3), ``rgb`` (n, 3) or None, ``err`` (n,) or None: float32 tensors on ``device``;
    ``ref_counts``: points per reference, in the order of the cloud.  Returns ``(xyz, rgb, err, counts, consensus)``: the kept points in input
    order (views of n-row tensors; rgb / err None when not given), the kept points per reference (int64 array) and - ``with_consensus`` - the
    uint8 count of every INPUT point, else None.  Raises ``ConsensusInputRefused`` for the key-range refusal."""
    counts = np.ascontiguousarray(np.asarray(ref_counts, np.int64).reshape(-1))
    n = int(xyz.shape[0])
    if counts.size < 1 or (counts < 0).any() or int(counts.sum()) != n:
        raise ValueError(f"{what}: ref_counts must be non-negative counts, one per reference, that add up to the {n} points")
    tensors = []
    for t, cols, name in ((xyz, 3, "xyz"), (rgb, 3, "rgb"), (err, 0, "err")):
        if t is None:
            tensors.append(None)
            continue
        if t.dtype != torch.float32 or t.device != device or int(t.shape[0]) != n or (cols and (t.dim() != 2 or t.shape[1] != cols)) or (not cols and t.dim() != 1):
            raise ValueError(f"{what}: {name} must be a float32 tensor of {n} rows{' x 3' if cols else ''} on {device}")
        tensors.append(t.contiguous())
    xyz, rgb, err = tensors
    offs = np.zeros(counts.size + 1, np.int64)
    np.cumsum(counts, out=offs[1:])
    offs_out = np.zeros_like(offs)
    outs = [torch.empty((max(n, 1),) + tuple(t.shape[1:]), dtype=torch.float32, device=device) if t is not None else None for t in tensors]
    cons = torch.empty((max(n, 1),), dtype=torch.uint8, device=device) if with_consensus else None
    n_out = C.c_int64(0)
    ptr = lambda t: t.data_ptr() if t is not None and n > 0 else None       # noqa: E731  (an empty tensor may have no address at all)
    i64p = C.POINTER(C.c_int64)
    rc = fn(ctx, ptr(xyz), ptr(rgb), ptr(err), n, offs.ctypes.data_as(i64p), int(counts.size), C.c_float(float(radius)), int(min_refs),
            ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), offs_out.ctypes.data_as(i64p), ptr(cons), C.byref(n_out))
    if rc != 0:
        msg = last_error()
        if "key range" in msg:
            raise ConsensusInputRefused(f"{what} refused its input ({rc}): {msg}")
        raise HipBackendError(f"{what} failed ({rc}): {msg}")
    k = int(n_out.value)
    kept = [o[:k] if o is not None else None for o in outs]
    return kept[0], kept[1], kept[2], np.diff(offs_out), (cons[:n] if with_consensus else None)


COMPONENT_SUMMARY_WORDS = 66     # lfd_component_filter's summary: n_components, largest size, 32 bins of components, 32 bins of their points


def _component_call(fn, ctx, what, xyz, rgb, err, ref_counts, radius, min_points, with_sizes, with_labels, device, last_error):
    """One lfd_component_filter[_host] call.  ``xyz`` (n, 3), ``rgb`` (n, 3) or None, ``err`` (n,) or None: float32 tensors on ``device``;
    ``ref_counts``: points per reference, in the order of the cloud.  Returns ``(xyz, rgb, err, kept_counts, sizes, labels, summary)``: the kept
    points in input order (views of n-row tensors; rgb / err None when not given), the kept points per reference (int64 array), - ``with_sizes``
    / ``with_labels``, else None - every INPUT point's component size and label (the smallest input index of its component) as int32 tensors
    on ``device`` holding the library's u32 values (both are below 2^31), and the 66 summary words (int64 array).  Raises
    ``ConsensusInputRefused`` for the key-range refusal, which is the consensus filter's."""
    counts = np.ascontiguousarray(np.asarray(ref_counts, np.int64).reshape(-1))
    n = int(xyz.shape[0])
    if counts.size < 1 or (counts < 0).any() or int(counts.sum()) != n:
        raise ValueError(f"{what}: ref_counts must be non-negative counts, one per reference, that add up to the {n} points")
    tensors = []
    for t, cols, name in ((xyz, 3, "xyz"), (rgb, 3, "rgb"), (err, 0, "err")):
        if t is None:
            tensors.append(None)
            continue
        if t.dtype != torch.float32 or t.device != device or int(t.shape[0]) != n or (cols and (t.dim() != 2 or t.shape[1] != cols)) or (not cols and t.dim() != 1):
            raise ValueError(f"{what}: {name} must be a float32 tensor of {n} rows{' x 3' if cols else ''} on {device}")
        tensors.append(t.contiguous())
    xyz, rgb, err = tensors
    offs = np.zeros(counts.size + 1, np.int64)
    np.cumsum(counts, out=offs[1:])
    offs_out = np.zeros_like(offs)
    outs = [torch.empty((max(n, 1),) + tuple(t.shape[1:]), dtype=torch.float32, device=device) if t is not None else None for t in tensors]
    sizes = torch.empty((max(n, 1),), dtype=torch.int32, device=device) if with_sizes else None
    labels = torch.empty((max(n, 1),), dtype=torch.int32, device=device) if with_labels else None
    summary = np.zeros(COMPONENT_SUMMARY_WORDS, np.int64)
    n_out = C.c_int64(0)
    ptr = lambda t: t.data_ptr() if t is not None and n > 0 else None       # noqa: E731  (an empty tensor may have no address at all)
    i64p = C.POINTER(C.c_int64)
    rc = fn(ctx, ptr(xyz), ptr(rgb), ptr(err), n, offs.ctypes.data_as(i64p), int(counts.size), C.c_float(float(radius)), int(min_points),
            ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), offs_out.ctypes.data_as(i64p), ptr(sizes), ptr(labels), summary.ctypes.data_as(i64p),
            C.byref(n_out))
    if rc != 0:
        msg = last_error()
        if "key range" in msg:
            raise ConsensusInputRefused(f"{what} refused its input ({rc}): {msg}")
        raise HipBackendError(f"{what} failed ({rc}): {msg}")
    k = int(n_out.value)
    kept = [o[:k] if o is not None else None for o in outs]
    return (kept[0], kept[1], kept[2], np.diff(offs_out), (sizes[:n] if with_sizes else None), (labels[:n] if with_labels else None), summary)


def _fuse_call(fn, ctx, what, xyz, normals, rgb, voxel_size, with_counts, device, last_error):
    """One lfd_fuse_oriented[_host] call.  ``xyz``, ``normals``, ``rgb``: (n, 3) float32 tensors on ``device``.  Returns
    ``((xyz, normals, rgb[, counts]), n_voxels)``: the rows - views of n-row tensors, voxels in key order, side 0 before side 1 -, with
    ``with_counts`` the int32 number of points merged into each row, and the number of occupied voxels.  Raises ``FuseInputRefused`` for a
    non-finite coordinate or a voxel key range beyond 63 bits."""
    n = int(xyz.shape[0])
    tensors = []
    for t, name in ((xyz, "xyz"), (normals, "normals"), (rgb, "rgb")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != device or t.dim() != 2 or t.shape[1] != 3 or int(t.shape[0]) != n:
            raise ValueError(f"{what}: {name} must be a float32 tensor of {n} rows x 3 on {device}")
        tensors.append(t.contiguous())
    outs = [torch.empty((max(n, 1), 3), dtype=torch.float32, device=device) for _ in range(3)]
    cnt = torch.empty((max(n, 1),), dtype=torch.int32, device=device) if with_counts else None
    n_rows, n_vox = C.c_int64(0), C.c_int64(0)
    ptr = lambda t: t.data_ptr() if t is not None and n > 0 else None       # noqa: E731  (an empty tensor may have no address at all)
    rc = fn(ctx, ptr(tensors[0]), ptr(tensors[1]), ptr(tensors[2]), n, C.c_double(float(voxel_size)), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
            ptr(cnt), C.byref(n_rows), C.byref(n_vox))
    if rc != 0:
        msg = last_error()
        if "non-finite coordinate" in msg or "key range" in msg:
            raise FuseInputRefused(f"{what} refused its input ({rc}): {msg}")
        raise HipBackendError(f"{what} failed ({rc}): {msg}")
    k = int(n_rows.value)
    rows = tuple(o[:k] for o in outs)
    return (rows + (cnt[:k],) if with_counts else rows), int(n_vox.value)


def _knn_call(fn, ctx, what, xyz, cell_size, device, last_error):
    """One lfd_knn_dist2[_host] call.  ``xyz``: (n, 3) float32 tensor on ``device``.  Returns ``(dist2, stats)``: the (n,) float32 mean squared
    distance of every point to its three nearest neighbours, and ``(cell size used, occupied cells, points in the fullest cell, points finished by
    the brute-force pass)``.  Raises ``KnnInputRefused`` for fewer than four points, a non-finite coordinate or a cell key range beyond the limits."""
    if not isinstance(xyz, torch.Tensor) or xyz.dtype != torch.float32 or xyz.device != device or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{what}: xyz must be a float32 tensor of n rows x 3 on {device}")
    n = int(xyz.shape[0])
    xyz = xyz.contiguous()
    out = torch.empty((max(n, 1),), dtype=torch.float32, device=device)
    stats = (C.c_double * 4)()
    rc = fn(ctx, xyz.data_ptr() if n > 0 else None, n, C.c_double(float(cell_size)), out.data_ptr() if n > 0 else None, stats)
    if rc != 0:
        msg = last_error()
        if "fewer than four points" in msg or "non-finite coordinate" in msg or "key range" in msg:
            raise KnnInputRefused(f"{what} refused its input ({rc}): {msg}")
        raise HipBackendError(f"{what} failed ({rc}): {msg}")
    return out[:n], (float(stats[0]), int(stats[1]), int(stats[2]), int(stats[3]))


def _cap_call(fn, ctx, what, xyz, err, budget, device, last_error):
    """One lfd_cap_spatial[_host] call.  ``xyz``: (n, 3) float32 tensor on ``device``; ``err``: (n,) float32 tensor there, or None.  Returns
    ``(keep, stats)``: the int64 tensor of the kept input indices, ascending, on ``device``, and ``(level, cells at that level, cells one level
    up, longest side of the bounding box)``.  Raises ``CapInputRefused`` for a non-finite coordinate."""
    if not isinstance(xyz, torch.Tensor) or xyz.dtype != torch.float32 or xyz.device != device or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{what}: xyz must be a float32 tensor of n rows x 3 on {device}")
    n = int(xyz.shape[0])
    if err is not None and (not isinstance(err, torch.Tensor) or err.dtype != torch.float32 or err.device != device or err.dim() != 1
                            or int(err.shape[0]) != n):
        raise ValueError(f"{what}: err must be None or a float32 tensor of {n} values on {device}")
    budget = int(budget)
    xyz = xyz.contiguous()
    err = err.contiguous() if err is not None else None
    keep = torch.empty((max(min(budget, n), 1),), dtype=torch.int64, device=device)
    n_keep = C.c_int64(0)
    stats = (C.c_double * 4)()
    rc = fn(ctx, xyz.data_ptr() if n > 0 else None, err.data_ptr() if err is not None and n > 0 else None, n, budget,
            keep.data_ptr() if n > 0 else None, C.byref(n_keep), stats)
    if rc != 0:
        msg = last_error()
        if "non-finite coordinate" in msg:
            raise CapInputRefused(f"{what} refused its input ({rc}): {msg}")
        raise HipBackendError(f"{what} failed ({rc}): {msg}")
    return keep[:int(n_keep.value)], (int(stats[0]), int(stats[1]), int(stats[2]), float(stats[3]))


THIN_LEVELS = 21     # octree levels 0 .. 20 of lfd_thin_footprint (csrc/lfd_thin.hpp)


def _thin_call(fn, ctx, what, xyz, err, ref_counts, ref_rows, thin_cells, device, last_error):
    """One lfd_thin_footprint[_host] call.  ``xyz``: (n, 3) float32 tensor on ``device``; ``err``: (n,) float32 tensor there, or None;
    ``ref_counts``: points per reference, in the order of the cloud; ``ref_rows``: (n_refs, 5) float64 host array, per reference the third row of
    its world-to-camera [R | t] and the tangent of one match-grid cell.  Returns ``(keep, counts, stats)``: the int64 tensor of the kept input
    indices, ascending, on ``device``, the kept points per reference (int64 array) and ``(points per level, cells per level, longest side of the
    bounding box)`` with two int64 arrays of THIN_LEVELS entries.  Raises ``ThinInputRefused`` for a non-finite coordinate."""
    if not isinstance(xyz, torch.Tensor) or xyz.dtype != torch.float32 or xyz.device != device or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{what}: xyz must be a float32 tensor of n rows x 3 on {device}")
    n = int(xyz.shape[0])
    if err is not None and (not isinstance(err, torch.Tensor) or err.dtype != torch.float32 or err.device != device or err.dim() != 1
                            or int(err.shape[0]) != n):
        raise ValueError(f"{what}: err must be None or a float32 tensor of {n} values on {device}")
    counts = np.ascontiguousarray(np.asarray(ref_counts, np.int64).reshape(-1))
    if counts.size < 1 or (counts < 0).any() or int(counts.sum()) != n:
        raise ValueError(f"{what}: ref_counts must be non-negative counts, one per reference, that add up to the {n} points")
    rows = np.ascontiguousarray(np.asarray(ref_rows, np.float64).reshape(-1, 5))
    if rows.shape[0] != counts.size:
        raise ValueError(f"{what}: ref_rows must hold five values per reference ({counts.size}), not {rows.shape[0]} rows")
    xyz = xyz.contiguous()
    err = err.contiguous() if err is not None else None
    offs = np.zeros(counts.size + 1, np.int64)
    np.cumsum(counts, out=offs[1:])
    offs_out = np.zeros_like(offs)
    keep = torch.empty((max(n, 1),), dtype=torch.int64, device=device)
    n_keep = C.c_int64(0)
    stats = (C.c_double * (2 * THIN_LEVELS + 1))()
    i64p = C.POINTER(C.c_int64)
    rc = fn(ctx, xyz.data_ptr() if n > 0 else None, err.data_ptr() if err is not None and n > 0 else None, n, offs.ctypes.data_as(i64p),
            int(counts.size), rows.ctypes.data_as(C.POINTER(C.c_double)), C.c_double(float(thin_cells)), keep.data_ptr() if n > 0 else None,
            C.byref(n_keep), offs_out.ctypes.data_as(i64p), stats)
    if rc != 0:
        msg = last_error()
        if "non-finite coordinate" in msg:
            raise ThinInputRefused(f"{what} refused its input ({rc}): {msg}")
        raise HipBackendError(f"{what} failed ({rc}): {msg}")
    values = np.asarray(list(stats), np.float64)
    return (keep[:int(n_keep.value)], np.diff(offs_out),
            (values[:THIN_LEVELS].astype(np.int64), values[THIN_LEVELS:2 * THIN_LEVELS].astype(np.int64), float(values[2 * THIN_LEVELS])))


def gaussian_pack_arguments(opacity: float, flatten: float, max_scale: float):
    """``(opacity_logit, log_flatten, max_scale)`` as lfd_pack_gaussians takes them: the f32 logit of the initial opacity and log(flatten), each
    computed once in f64."""
    import math
    opacity, flatten, max_scale = float(opacity), float(flatten), float(max_scale)
    if not (0.0 < opacity < 1.0) or not (0.0 < flatten <= 1.0) or not (0.0 <= max_scale < float("inf")):
        raise ValueError("pack_gaussians: opacity must be in (0, 1), flatten in (0, 1], max_scale finite and >= 0")
    return float(np.float32(math.log(opacity / (1.0 - opacity)))), math.log(flatten), max_scale


def _pack_gaussians_call(fn, ctx, what, xyz, normals, rgb, dist2, opacity, flatten, max_scale, device, last_error):
    """One lfd_pack_gaussians[_host] call: the (n*68,) u8 tensor on ``device`` - the body of a PLY whose header is ``writers.gaussian_ply_header``."""
    n = int(xyz.shape[0])
    tensors = []
    for t, cols, name in ((xyz, 3, "xyz"), (normals, 3, "normals"), (rgb, 3, "rgb"), (dist2, 0, "dist2")):
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != device or int(t.shape[0]) != n
                or (cols and (t.dim() != 2 or t.shape[1] != cols)) or (not cols and t.dim() != 1)):
            raise ValueError(f"{what}: {name} must be a float32 tensor of {n} rows{' x 3' if cols else ''} on {device}")
        tensors.append(t.contiguous())
    logit, log_flatten, max_scale = gaussian_pack_arguments(opacity, flatten, max_scale)
    out = torch.empty((max(n * 68, 4),), dtype=torch.uint8, device=device)
    ptr = lambda t: t.data_ptr() if n > 0 else None       # noqa: E731  (an empty tensor may have no address at all)
    rc = fn(ctx, ptr(tensors[0]), ptr(tensors[1]), ptr(tensors[2]), ptr(tensors[3]), n, C.c_float(logit), C.c_double(log_flatten),
            C.c_double(max_scale), out.data_ptr())
    if rc != 0:
        raise HipBackendError(f"{what} failed ({rc}): {last_error()}")
    return out[:n * 68]


def _freespace_call(fn, ctx, what, xyz, rgb, err, ref_counts, cam_P, cam_wh, plane, tol, min_violations, with_counts, device, last_error):
    """One lfd_freespace_filter[_host] call.  ``xyz`` (n, 3), ``rgb`` (n, 3) or None, ``err`` (n,) or None: float32 tensors on ``device``;
    ``ref_counts``: points per reference, in the order of the cloud; ``cam_P`` (n_refs, 3, 4) or (n_refs, 12) float32 and ``cam_wh`` (n_refs, 2)
    int32: every reference's projection and image size (host arrays); ``plane`` = (pw, ph), the z-buffer size.  Returns
    ``(xyz, rgb, err, counts, violations, supports)``: the kept points in input order (views of n-row tensors; rgb / err None when not given), the
    kept points per reference (int64 array) and - ``with_counts`` - the two uint8 counts of every INPUT point, else None."""
    counts = np.ascontiguousarray(np.asarray(ref_counts, np.int64).reshape(-1))
    n = int(xyz.shape[0])
    if counts.size < 1 or (counts < 0).any() or int(counts.sum()) != n:
        raise ValueError(f"{what}: ref_counts must be non-negative counts, one per reference, that add up to the {n} points")
    P = np.ascontiguousarray(np.asarray(cam_P, np.float32).reshape(-1, 12))
    wh = np.ascontiguousarray(np.asarray(cam_wh, np.int32).reshape(-1, 2))
    if P.shape[0] != counts.size or wh.shape[0] != counts.size:
        raise ValueError(f"{what}: cam_P and cam_wh must hold one camera per reference ({counts.size}), not {P.shape[0]} and {wh.shape[0]}")
    tensors = []
    for t, cols, name in ((xyz, 3, "xyz"), (rgb, 3, "rgb"), (err, 0, "err")):
        if t is None:
            tensors.append(None)
            continue
        if t.dtype != torch.float32 or t.device != device or int(t.shape[0]) != n or (cols and (t.dim() != 2 or t.shape[1] != cols)) or (not cols and t.dim() != 1):
            raise ValueError(f"{what}: {name} must be a float32 tensor of {n} rows{' x 3' if cols else ''} on {device}")
        tensors.append(t.contiguous())
    xyz, rgb, err = tensors
    offs = np.zeros(counts.size + 1, np.int64)
    np.cumsum(counts, out=offs[1:])
    offs_out = np.zeros_like(offs)
    outs = [torch.empty((max(n, 1),) + tuple(t.shape[1:]), dtype=torch.float32, device=device) if t is not None else None for t in tensors]
    viol = torch.empty((max(n, 1),), dtype=torch.uint8, device=device) if with_counts else None
    supp = torch.empty((max(n, 1),), dtype=torch.uint8, device=device) if with_counts else None
    n_out = C.c_int64(0)
    ptr = lambda t: t.data_ptr() if t is not None and n > 0 else None       # noqa: E731  (an empty tensor may have no address at all)
    i64p = C.POINTER(C.c_int64)
    rc = fn(ctx, ptr(xyz), ptr(rgb), ptr(err), n, offs.ctypes.data_as(i64p), int(counts.size), P.ctypes.data_as(C.POINTER(C.c_float)),
            wh.ctypes.data_as(C.POINTER(C.c_int32)), int(plane[0]), int(plane[1]), C.c_float(float(tol)), int(min_violations),
            ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), offs_out.ctypes.data_as(i64p), ptr(viol), ptr(supp), C.byref(n_out))
    if rc != 0:
        raise HipBackendError(f"{what} failed ({rc}): {last_error()}")
    k = int(n_out.value)
    kept = [o[:k] if o is not None else None for o in outs]
    return kept[0], kept[1], kept[2], np.diff(offs_out), (viol[:n] if with_counts else None), (supp[:n] if with_counts else None)


def _depth_call(fn, ctx, what, xyz, normals, cam_P, cam_wh, plane, splat_cells, window_cells, tol, with_index, cams_per_batch, device, last_error):
    """One lfd_render_depth[_host] call.  ``xyz`` (n, 3) and ``normals`` (n, 3) or None: float32 tensors on ``device``, or arrays (then the
    results are arrays too); ``cam_P`` (n_cams, 3, 4) or (n_cams, 12) float32 and ``cam_wh`` (n_cams, 2) int32: every camera's projection and
    image size (host arrays); ``plane`` = (pw, ph).  Returns ``(depth, index, normal)``: float32 (n_cams, ph, pw) with 0 for no data, int32 of
    the same shape with -1 for no data (None without ``with_index``), float32 (n_cams, ph, pw, 3) (None without ``normals``)."""
    as_arrays = not torch.is_tensor(xyz)
    if as_arrays:
        xyz = torch.from_numpy(np.ascontiguousarray(np.asarray(xyz, np.float32))).to(device)
        normals = None if normals is None else torch.from_numpy(np.ascontiguousarray(np.asarray(normals, np.float32))).to(device)
    n = int(xyz.shape[0])
    for t, name in ((xyz, "xyz"), (normals, "normals")):
        if t is not None and (t.dtype != torch.float32 or t.device != device or t.dim() != 2 or tuple(t.shape) != (n, 3)):
            raise ValueError(f"{what}: {name} must be a float32 tensor of {n} rows x 3 on {device}")
    xyz = xyz.contiguous()
    normals = None if normals is None else normals.contiguous()
    P = np.ascontiguousarray(np.asarray(cam_P, np.float32).reshape(-1, 12))
    wh = np.ascontiguousarray(np.asarray(cam_wh, np.int32).reshape(-1, 2))
    n_cams, pw, ph = int(P.shape[0]), int(plane[0]), int(plane[1])
    if wh.shape[0] != n_cams:
        raise ValueError(f"{what}: cam_P and cam_wh must hold one camera each, not {n_cams} and {wh.shape[0]}")
    if n_cams < 1 or pw < 1 or ph < 1 or n_cams * pw * ph > 0x7fffffff:
        raise ValueError(f"{what}: {n_cams} cameras on a {pw} x {ph} plane: at least one camera and one cell, at most 2^31 - 1 cells")
    depth = torch.empty((n_cams, ph, pw), dtype=torch.float32, device=device)
    index = torch.empty((n_cams, ph, pw), dtype=torch.int32, device=device) if with_index else None
    normal = torch.empty((n_cams, ph, pw, 3), dtype=torch.float32, device=device) if normals is not None else None
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() > 0 else None       # noqa: E731  (an empty tensor may have no address at all)
    # normals of no points: the call wants a non-null address next to normal_out and reads nothing through it
    nptr = None if normals is None else (normals.data_ptr() if n > 0 else normal.data_ptr())
    rc = fn(ctx, ptr(xyz), n, nptr, P.ctypes.data_as(C.POINTER(C.c_float)), wh.ctypes.data_as(C.POINTER(C.c_int32)), n_cams, pw, ph, int(splat_cells), int(window_cells),
            C.c_float(float(tol)), int(cams_per_batch), ptr(depth), ptr(index), ptr(normal))
    if rc != 0:
        raise HipBackendError(f"{what} failed ({rc}): {last_error()}")
    if as_arrays:
        return tuple(None if t is None else t.cpu().numpy() for t in (depth, index, normal))
    return depth, index, normal


class HipDensifier:
    """One context = one GPU + one stream (``torch.cuda.current_stream`` of the device at creation,
    unless a stream is given).  Not thread-safe: use one per thread, as the C-ABI requires."""

    def __init__(self, device: Optional[torch.device] = None, stream: Optional[torch.cuda.Stream] = None):
        self._lib = load_library()
        self._ctx = C.c_void_p()
        self._undistort_ws: dict = {}           # undistort_image's named workspaces: (name, part) -> u8 buffer
        if not torch.cuda.is_available():
            raise HipBackendError("no GPU visible: the dense-initialisation hot path has no CPU fallback")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        if self.device.type != "cuda":
            raise HipBackendError(f"HipDensifier needs a cuda (HIP) device, got {self.device}")
        index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", index)
        self.stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        rc = self._lib.lfd_create(index, C.c_void_p(self.stream.cuda_stream), C.byref(self._ctx))
        if rc != 0:
            raise HipBackendError(f"lfd_create failed ({rc}): {self._lib.lfd_last_error(None).decode()}")
        self.n_cams = 0
        self.fuse_voxels = 0           # occupied voxels of the last fuse_oriented call
        self.knn_stats = (0.0, 0, 0, 0)       # (cell size, occupied cells, fullest cell, brute-forced points) of the last knn_dist2 call
        self.cap_stats = (0, 0, 0, 0.0)       # (level, cells at it, cells one level up, longest side of the box) of the last cap_spatial call
        self.thin_stats = (np.zeros(THIN_LEVELS, np.int64), np.zeros(THIN_LEVELS, np.int64), 0.0)   # (points, cells per level, box side) of the last thin_footprint call

    def close(self) -> None:
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self._lib.lfd_destroy(self._ctx)
            self._ctx = C.c_void_p()
        self._undistort_ws = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str) -> None:
        if rc != 0:
            raise HipBackendError(f"{what} failed ({rc}): {self._lib.lfd_last_error(self._ctx).decode()}")

    def _same_device(self, batch: "PreparedBatch", out: Optional["OutputBuffers"] = None, *tensors) -> None:
        """Every pointer handed to the library must live where this context computes: a CPU batch (or one of another GPU) given
        to a device context would be a memory fault inside a kernel, a device batch given to the CPU twin a host segfault."""
        if torch.device(batch.device) != self.device:
            raise ValueError(f"batch lives on {batch.device}, this context computes on {self.device}")
        if out is not None and out.xyz.device != self.device:
            raise ValueError(f"output buffers live on {out.xyz.device}, this context computes on {self.device}")
        for t in tensors:
            if t is not None and t.device != self.device:
                raise ValueError(f"tensor on {t.device} handed to a context that computes on {self.device}")

    def upload_cameras(self, cams: Sequence[CameraRecord]) -> None:
        K = _f32(np.stack([np.asarray(c.K, np.float32).reshape(9) for c in cams]))
        R = _f32(np.stack([np.asarray(c.R, np.float32).reshape(9) for c in cams]))
        t = _f32(np.stack([np.asarray(c.t, np.float32).reshape(3) for c in cams]))
        P = _f32(np.stack([np.asarray(c.P, np.float32).reshape(12) for c in cams]))
        Cc = _f32(np.stack([np.asarray(c.C, np.float32).reshape(3) for c in cams]))
        wh = np.ascontiguousarray(np.array([[c.width, c.height] for c in cams], np.int32))
        self._check(self._lib.lfd_upload_cameras(self._ctx, len(cams), _fp(K), _fp(R), _fp(t), _fp(P), _fp(Cc),
                                                 wh.ctypes.data_as(C.POINTER(C.c_int32))), "lfd_upload_cameras")
        self.n_cams = len(cams)

    def pair_fundamentals(self, n_refs: int, k: int) -> np.ndarray:
        """(n_refs, k, 3, 3) f64: the fundamental matrices the kernels of the last prepared batch used (debug read-back)."""
        out = np.zeros((n_refs * k, 9), np.float64)
        self._check(self._lib.lfd_get_pair_fundamental(self._ctx, n_refs * k, out.ctypes.data_as(C.POINTER(C.c_double))),
                    "lfd_get_pair_fundamental")
        return out.reshape(n_refs, k, 3, 3)

    def reload_env(self) -> None:
        """Re-read the profiling switches of the environment (they are read at creation only, lfd_reload_env)."""
        self._check(self._lib.lfd_reload_env(self._ctx), "lfd_reload_env")

    def time_dense_kernels(self, n_launches: int) -> None:
        """The next ``n_launches`` dense launches carry start / stop events of their own (lfd_kernel_timing): the kernel's device-side
        duration, as a kernel trace reports it.  0 switches the timing off."""
        self._check(self._lib.lfd_kernel_timing(self._ctx, int(n_launches)), "lfd_kernel_timing")

    def dense_kernel_times_ms(self) -> np.ndarray:
        """Durations (ms, launch order) of the dense launches timed since ``time_dense_kernels`` / the last read; waits for the last one."""
        cap = 1 << 20
        n = C.c_int32(0)
        buf = np.zeros(cap, np.float32)
        self._check(self._lib.lfd_kernel_timing_read(self._ctx, buf.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(n)), "lfd_kernel_timing_read")
        return buf[:n.value].astype(np.float64)

    def check_launches(self) -> None:
        """Synchronise and raise if a kernel reported a look-back timeout."""
        st = C.c_int32(0)
        self._check(self._lib.lfd_launch_status(self._ctx, C.byref(st)), "lfd_launch_status")

    # -- N1: file payloads packed on the device ------------------------------------------------------------
    @staticmethod
    def _pts(t: torch.Tensor, cols: int, what: str) -> torch.Tensor:
        if t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError(f"{what} must be a float32 device tensor")
        t = t.contiguous()
        if cols and (t.dim() != 2 or t.shape[1] != cols):
            raise ValueError(f"{what} must have shape (n,{cols})")
        return t

    def pack_ply(self, xyz: torch.Tensor, rgb: torch.Tensor) -> torch.Tensor:
        """(n*15,) u8 device tensor: the PLY body upstream's write_ply emits after its header."""
        xyz, rgb = self._pts(xyz, 3, "xyz"), self._pts(rgb, 3, "rgb")
        n = int(xyz.shape[0])
        out = torch.empty((max(n * 15, 4),), dtype=torch.uint8, device=xyz.device)
        self._check(self._lib.lfd_pack_ply(self._ctx, xyz.data_ptr(), rgb.data_ptr(), n, out.data_ptr()), "lfd_pack_ply")
        return out[:n * 15]

    def pack_points3d(self, xyz: torch.Tensor, rgb: torch.Tensor, err: Optional[torch.Tensor] = None,
                      id_base: int = 0) -> torch.Tensor:
        """(n*43,) u8 device tensor: upstream's points3D.bin body (without the leading u64 count)."""
        xyz, rgb = self._pts(xyz, 3, "xyz"), self._pts(rgb, 3, "rgb")
        e = self._pts(err, 0, "err") if err is not None else None
        n = int(xyz.shape[0])
        out = torch.empty((max(n * 43, 4),), dtype=torch.uint8, device=xyz.device)
        self._check(self._lib.lfd_pack_points3d(self._ctx, xyz.data_ptr(), rgb.data_ptr(), e.data_ptr() if e is not None else None,
                                                n, int(id_base), out.data_ptr()), "lfd_pack_points3d")
        return out[:n * 43]

    def voxel_downsample(self, xyz: torch.Tensor, rgb: torch.Tensor, voxel_size: float) -> Tuple[torch.Tensor, torch.Tensor]:
        """The distance filter on the device (lfd_voxel_downsample): (xyz_v, rgb_v), f32 device tensors of one row per occupied voxel, bit for bit
        and in the order of the NumPy branch of ``densify._voxel_downsample``.  Synchronous.  Raises ``VoxelInputRefused`` for a non-finite
        coordinate or a voxel key range beyond 63 bits."""
        xyz, rgb = self._pts(xyz, 3, "xyz"), self._pts(rgb, 3, "rgb")
        n = int(xyz.shape[0])
        if int(rgb.shape[0]) != n:
            raise ValueError("xyz and rgb must have the same number of rows")
        xo = torch.empty((max(n, 1), 3), dtype=torch.float32, device=xyz.device)
        ro = torch.empty((max(n, 1), 3), dtype=torch.float32, device=xyz.device)
        nv = C.c_int64(0)
        rc = self._lib.lfd_voxel_downsample(self._ctx, xyz.data_ptr(), rgb.data_ptr(), n, float(voxel_size), xo.data_ptr(), ro.data_ptr(), C.byref(nv))
        if rc != 0:
            msg = self._lib.lfd_last_error(self._ctx).decode()
            if "non-finite coordinate" in msg or "key range" in msg:
                raise VoxelInputRefused(f"lfd_voxel_downsample refused its input ({rc}): {msg}")
            self._check(rc, "lfd_voxel_downsample")
        return xo[:nv.value], ro[:nv.value]

    def consensus_filter(self, xyz: torch.Tensor, rgb: Optional[torch.Tensor], err: Optional[torch.Tensor], ref_counts, radius: float, min_refs: int,
                         with_consensus: bool = False):
        """Cross-reference consensus filter on the device (lfd_consensus_filter): a point of the cloud - the concatenation of the
        references' points, ``ref_counts`` each - is kept iff at least ``min_refs`` OTHER references own a point within ``radius`` of it.
        Returns ``(xyz, rgb, err, counts, consensus)`` as ``_consensus_call`` describes.  Synchronous."""
        return _consensus_call(self._lib.lfd_consensus_filter, self._ctx, "lfd_consensus_filter", xyz, rgb, err, ref_counts, radius, min_refs,
                               with_consensus, self.device, lambda: self._lib.lfd_last_error(self._ctx).decode())

    def component_filter(self, xyz: torch.Tensor, rgb: Optional[torch.Tensor], err: Optional[torch.Tensor], ref_counts, radius: float,
                         min_points: int, with_sizes: bool = False, with_labels: bool = False):
        """Connected-component filter on the device (lfd_component_filter): a point of the cloud is kept iff the connected
        component of the radius graph it belongs to has at least ``min_points`` points.  The points never leave the GPU.  Returns
        ``(xyz, rgb, err, kept_counts, sizes, labels, summary)`` as ``_component_call`` describes.  Synchronous."""
        return _component_call(self._lib.lfd_component_filter, self._ctx, "lfd_component_filter", xyz, rgb, err, ref_counts, radius, min_points,
                               with_sizes, with_labels, self.device, lambda: self._lib.lfd_last_error(self._ctx).decode())

    def freespace_filter(self, xyz: torch.Tensor, rgb: Optional[torch.Tensor], err: Optional[torch.Tensor], ref_counts, cam_P, cam_wh, plane,
                         tol: float, min_violations: int, with_counts: bool = False):
        """Free-space filter on the device (lfd_freespace_filter): a point of the cloud - the concatenation of the references'
        points, ``ref_counts`` each - is dropped when at least ``min_violations`` OTHER references triangulated a surface behind it on the same
        ray (they looked through it) and more refute than support it.  Returns ``(xyz, rgb, err, counts, violations, supports)`` as
        ``_freespace_call`` describes.  Synchronous."""
        return _freespace_call(self._lib.lfd_freespace_filter, self._ctx, "lfd_freespace_filter", xyz, rgb, err, ref_counts, cam_P, cam_wh, plane, tol,
                               min_violations, with_counts, self.device, lambda: self._lib.lfd_last_error(self._ctx).decode())

    def render_depth(self, xyz, normals, cam_P, cam_wh, plane, splat_cells: int = 1, window_cells: int = 3, tol: float = 0.02,
                     with_index: bool = False, cams_per_batch: int = 0):
        """Depth and normal maps of a cloud on the device (lfd_render_depth): every camera's nearest point per cell of its
        ``plane``, splatted over ``2 splat_cells + 1`` cells, and dropped where something nearer by more than ``tol`` lies within
        ``window_cells``.  Returns ``(depth, index, normal)`` as ``_depth_call`` describes.  Synchronous."""
        return _depth_call(self._lib.lfd_render_depth, self._ctx, "lfd_render_depth", xyz, normals, cam_P, cam_wh, plane, splat_cells, window_cells,
                           tol, with_index, cams_per_batch, self.device, lambda: self._lib.lfd_last_error(self._ctx).decode())

    def fuse_oriented(self, xyz: torch.Tensor, normals: torch.Tensor, rgb: torch.Tensor, voxel_size: float, with_counts: bool = False):
        """Oriented voxel fusion on the device (lfd_fuse_oriented): the points of every occupied voxel merged per side their
        normals face - positions and colours averaged, normals summed and renormalised -, one row per visible face.  Returns
        ``(xyz, normals, rgb)``, with ``with_counts`` also the points per row; ``self.fuse_voxels`` then holds the number of occupied voxels
        of this call.  Synchronous.  Raises ``FuseInputRefused`` as ``_fuse_call`` describes."""
        rows, self.fuse_voxels = _fuse_call(self._lib.lfd_fuse_oriented, self._ctx, "lfd_fuse_oriented", xyz, normals, rgb, voxel_size, with_counts,
                                            self.device, lambda: self._lib.lfd_last_error(self._ctx).decode())
        return rows

    def set_stream(self, stream: "torch.cuda.Stream") -> None:
        """Later calls are issued on ``stream`` (lfd_set_stream: what was issued on the previous one is waited for first).  A call with the
        stream the context already uses does nothing."""
        if int(stream.cuda_stream) == int(self.stream.cuda_stream):
            return
        self._check(self._lib.lfd_set_stream(self._ctx, C.c_void_p(stream.cuda_stream)), "lfd_set_stream")
        self.stream = stream

    def local_corr(self, a: torch.Tensor, bf: torch.Tensor, warp: torch.Tensor) -> torch.Tensor:
        """RoMa-v2's local correlation (lfd_local_corr): ``out[b, n, k] = sum_c a[b, n, c] * bilinear(bf[b, :, :, c]; warp[b, n, k])``
        for f32 tensors ``a`` (B, N, C), ``bf`` (B, H1, W1, C), ``warp`` (B, N, K, 2) of this context's device; (B, N, K) f32.  One launch on
        the context's stream, no temporary of the size of the sampled features.  ``a`` and ``bf`` are read through their strides; when
        C % 4 == 0 and the channels of one of them are not adjacent in memory, a channel-last copy of that tensor is made first so that the
        vector kernel (16-byte loads) serves the call - same bits as for a contiguous input."""
        a, bf, warp, dims = _local_corr_arguments(a, bf, warp, self.device)
        out = torch.empty((dims[0], dims[1], dims[3]), dtype=torch.float32, device=self.device)
        sa, sb = (C.c_int64 * 3)(*a.stride()), (C.c_int64 * 4)(*bf.stride())
        self._check(self._lib.lfd_local_corr(self._ctx, a.data_ptr(), bf.data_ptr(), warp.data_ptr(), *dims, sa, sb, out.data_ptr()), "lfd_local_corr")
        return out

    def refiner_block(self, x: torch.Tensor, dw_w: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, pw_wt: Optional[torch.Tensor] = None,
                      pw_b: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One conv block of RoMa-v2's refiners (lfd_refiner_block): depthwise 5x5 with the weights ``dw_w`` (C, 25) on ``x``
        (B, C, H, W; bf16, or f32 that is rounded to bf16 on load), the folded BatchNorm ``scale`` / ``shift`` (C), ReLU, rounded to bf16; with
        ``pw_wt`` (C, C; the 1x1 weights TRANSPOSED) and ``pw_b`` (C) the 1x1 convolution as well - C == 32 only.  (B, C, H, W) bf16.  One
        launch on the context's stream; a non-contiguous ``x`` is copied to contiguous NCHW first."""
        rc, out = _refiner_block_call(self._lib.lfd_refiner_block, self._ctx, x, dw_w, scale, shift, pw_wt, pw_b, self.device)
        self._check(rc, "lfd_refiner_block")
        return out

    def refiner_head(self, z: torch.Tensor, head_w: torch.Tensor, head_b: torch.Tensor, prev_warp: torch.Tensor,
                     prev_conf: Optional[torch.Tensor] = None, refine_init: float = 4.0) -> Tuple[torch.Tensor, torch.Tensor]:
        """The output head of RoMa-v2's refiners (lfd_refiner_head): the two 1x1 convolutions ``head_w`` (6, C; rows 0..1 the warp
        head, 2..5 the confidence head) / ``head_b`` (6) on ``z`` (B, C, H, W; bf16 or f32, used as given), the warp update
        ``prev_warp + a[0:2] / (refine_init (W, H))``, softplus and the Cholesky-to-precision conversion, and the addition of ``prev_conf``
        (B, H, W, 1 or 4; None: nothing is added).  (warp (B, H, W, 2), conf (B, H, W, 4)) f32.  One launch on the context's stream;
        ``prev_warp`` and ``prev_conf`` are read through their own strides; a ``z`` that is not contiguous NCHW raises ValueError."""
        rc, warp, conf = _refiner_head_call(self._lib.lfd_refiner_head, self._ctx, z, head_w, head_b, prev_warp, prev_conf, refine_init, self.device)
        self._check(rc, "lfd_refiner_head")
        return warp, conf

    def cycle_gate(self, cert, warp_ab, warp_ba, w_match: int, h_match: int, certainty_thresh: float, cycle_thresh_px: float, axes=None,
                   inplace: bool = False, with_err: bool = False, rejected: Optional[torch.Tensor] = None):
        """Forward-backward consistency gate (lfd_cycle_gate) over up to 16 pairs in one launch on the context's stream.
        ``cert`` [(H, W)], ``warp_ab`` [(H, W, 2 | 4)], ``warp_ba`` [(Hb, Wb, 2)]: one contiguous f32 tensor of this device per pair, read in
        place.  A cell keeps its certainty, floored at ``certainty_thresh``, iff following ``warp_ab`` and coming back with ``warp_ba`` lands
        within ``cycle_thresh_px`` pixels of the match image (``w_match`` x ``h_match``) of where it started; else it becomes exactly 0.
        ``axes``: (axis_x, axis_y) of the reference grid for 2-channel warps (None: the identity axes).  ``inplace``: the planes of ``cert`` are
        overwritten.  ``rejected``: int32 [n_pairs] on this device, the rejected cells of every pair are ADDED to it.
        Returns (gated planes, error planes in px or None)."""
        rc, outs, errs = _cycle_gate_call(self._lib.lfd_cycle_gate, self._ctx, cert, warp_ab, warp_ba, w_match, h_match, certainty_thresh,
                                          cycle_thresh_px, axes, inplace, with_err, rejected, self.device)
        self._check(rc, "lfd_cycle_gate")
        return outs, errs

    def support_filter(self, batch: PreparedBatch, out_buffers, min_support: int, support_thresh_px: float, with_support: bool = False,
                       into: Optional[OutputBuffers] = None):
        """Multi-view support filter behind a triangulation call (lfd_support_filter): of the points ``out_buffers`` holds for
        ``batch`` (an OutputBuffers a launch wrote, or a collected TriangulationOutput; with_cell=True), those that at least ``min_support``
        OTHER neighbours of their reference confirm within ``support_thresh_px`` (px of the neighbour's camera image), compacted in order.
        Returns buffers of the same kind (asynchronous on the context's stream for OutputBuffers; ``into``: the buffers to fill instead of new
        ones); with ``with_support`` a pair (result, uint8 support count of every INPUT point)."""
        self._same_device(batch)
        with torch.cuda.stream(self.stream):
            rc, res, support = _support_filter_call(self._lib.lfd_support_filter, self._ctx, batch, out_buffers, min_support, support_thresh_px,
                                                    with_support, into, self.device)
        self._check(rc, "lfd_support_filter")
        return (res, support) if with_support else res

    def refine_multiview(self, batch: PreparedBatch, out_buffers, support_thresh_px: float, reproj_thresh: float, with_status: bool = False,
                         counters: Optional[torch.Tensor] = None, precision: bool = False):
        """Multi-view re-triangulation of supported points (lfd_refine_multiview): every point ``out_buffers`` holds for ``batch``
        (an OutputBuffers a launch wrote - refined in place, asynchronously on the context's stream - or a collected TriangulationOutput, which
        is copied) that OTHER neighbours of its reference confirm within ``support_thresh_px`` is triangulated again from all those views and
        replaced when the result passes the two-view tests at ``reproj_thresh`` and every confirming view still agrees.  Order, counts, rgb,
        cell and slot never change.  ``counters``: int64 [2] on the device, added to (refined, kept their two-view position although confirmed).
        With ``with_status`` a pair (result, uint8 per point: confirming views | 0x80 if replaced).  ``precision``: the rows are weighted by
        the batch's precision planes (lfd_refine_multiview_weighted); ``counters`` is then int64 [3] (+ points solved with
        weighted rows) and the status carries 0x40 where they were."""
        self._same_device(batch)
        name = "lfd_refine_multiview_weighted" if precision else "lfd_refine_multiview"
        with torch.cuda.stream(self.stream):
            rc, res, status = _refine_call(getattr(self._lib, name), self._ctx, batch, out_buffers, support_thresh_px, reproj_thresh,
                                           with_status, counters, self.device, precision)
        self._check(rc, name)
        return (res, status) if with_status else res

    def depth_sigma_filter(self, batch: PreparedBatch, out_buffers, max_rel_sigma: float, iso_sigma_px: float = 0.0,
                           refine_status: Optional[torch.Tensor] = None, support_thresh_px: float = 0.0, with_sigma: bool = False,
                           into: Optional[OutputBuffers] = None):
        """Depth-uncertainty gate behind a triangulation call (lfd_depth_sigma_filter): of the points ``out_buffers`` holds for
        ``batch`` (an OutputBuffers a launch wrote, or a collected TriangulationOutput; with_cell=True), those whose sigma_rel - the 1-sigma
        Cramer-Rao bound on the relative depth error along the reference's ray, from the views that placed the point - is at most
        ``max_rel_sigma`` (0: all of them), compacted in order.  ``iso_sigma_px`` > 0: every match has that isotropic noise (camera px); 0: the
        batch's precision planes.  ``refine_status``: the status tensor of the ``refine_multiview`` call that just ran over the points (its
        candidates at ``support_thresh_px`` then count for the points it replaced), or None: the winning slot alone.  Returns buffers of the
        same kind (asynchronous on the context's stream for OutputBuffers; ``into``: the buffers to fill instead of new ones); with
        ``with_sigma`` a triple (result, f32 sigma_rel of every INPUT point, f32 sigma_rel compacted with the points)."""
        self._same_device(batch)
        with torch.cuda.stream(self.stream):
            rc, res, sigma, sigma_out = _depth_sigma_call(self._lib.lfd_depth_sigma_filter, self._ctx, batch, out_buffers, max_rel_sigma,
                                                          iso_sigma_px, refine_status, support_thresh_px, with_sigma, into, self.device)
        self._check(rc, "lfd_depth_sigma_filter")
        return (res, sigma, sigma_out) if with_sigma else res

    def photo_gate(self, batch: PreparedBatch, out_buffers, window_cells: int, min_ncc: float, min_texture: float, with_status: bool = False,
                   with_ncc: bool = False, counters: Optional[torch.Tensor] = None, into: Optional[OutputBuffers] = None):
        """Photo-consistency gate behind a triangulation call (lfd_photo_gate): of the points ``out_buffers`` holds for ``batch``
        (an OutputBuffers a launch or a post-stage wrote, or a collected TriangulationOutput; with_cell=True), those whose MATCH the images do
        not refute, compacted in order.  The test is the ZNCC of the reference's patch - the (2 ``window_cells`` + 1)^2 grid cells around the
        point's cell - and the winning neighbour's patch where the dense warp sends those cells, sampled from ``ReferenceInputs.nbr_images``;
        a point is dropped only where at least half the window takes part, both patches have a standard deviation of ``min_texture`` grey
        levels (8-bit) and the ZNCC is below ``min_ncc``.  ``counters``: int64 [5] on the device, added to (points guarded, with a sparse
        window, untextured, consistent, refuted).  Returns buffers of the same kind (asynchronous on the context's stream for OutputBuffers;
        ``into``: the buffers to fill instead of new ones); with ``with_status`` and / or ``with_ncc`` a tuple (result[, uint8 status of every
        INPUT point][, f32 ZNCC of every INPUT point, NaN where none was decided on])."""
        self._same_device(batch)
        with torch.cuda.stream(self.stream):
            rc, res, status, ncc = _photo_gate_call(self._lib.lfd_photo_gate, self._ctx, batch, out_buffers, window_cells, min_ncc, min_texture,
                                                    with_status, with_ncc, counters, into, self.device)
        self._check(rc, "lfd_photo_gate")
        extra = ((status,) if with_status else ()) + ((ncc,) if with_ncc else ())
        return (res,) + extra if extra else res

    def estimate_normals(self, batch: PreparedBatch, out_buffers, radius: int, depth_step_rel: float, reproj_thresh: float,
                         with_status: bool = False, counters: Optional[torch.Tensor] = None):
        """Per-point surface normals from the resident warps (lfd_estimate_normals): for every point ``out_buffers`` holds for
        ``batch`` (an OutputBuffers a launch or a post-stage wrote - their ``normals`` tensor is written asynchronously on the context's
        stream - or a collected TriangulationOutput, whose copy carries ``normals``) the unit normal of the plane fitted to the winning
        neighbour's warp in the (2 ``radius`` + 1)^2 window of grid cells around the point's cell, oriented towards the reference's centre;
        the unit view vector where no plane can be fitted.  The points themselves are not touched.  ``counters``: int64 [2] on the device,
        added to (fitted, fell back).  With ``with_status`` a pair (result, uint8 per point: window cells that took part | 0x80 if fitted)."""
        self._same_device(batch)
        with torch.cuda.stream(self.stream):
            rc, res, status = _normals_call(self._lib.lfd_estimate_normals, self._ctx, batch, out_buffers, radius, depth_step_rel, reproj_thresh,
                                            with_status, counters, self.device)
        self._check(rc, "lfd_estimate_normals")
        return (res, status) if with_status else res

    def colour_multiview(self, batch: PreparedBatch, out_buffers, support_thresh_px: float, mode: str, with_status: bool = False,
                         counters: Optional[torch.Tensor] = None):
        """Multi-view point colour (lfd_colour_multiview): the colour of every point ``out_buffers`` holds for ``batch`` (an
        OutputBuffers a launch or a post-stage wrote - rewritten in place, asynchronously on the context's stream - or a collected
        TriangulationOutput, whose copy carries the new ``rgb``) becomes the ``mode`` ("mean" / "median") over the views that see it: its
        reference (the colour it has), the neighbour that won it and every other neighbour the support filter's test confirms within
        ``support_thresh_px``, each sampled from ``ReferenceInputs.nbr_images``.  Points, counts and order are untouched.  ``counters``: int64
        [2] on the device, added to (points blended, the sum of their views).  With ``with_status`` a pair (result, uint8 per point: views
        blended, 0 = left as it was)."""
        self._same_device(batch)
        with torch.cuda.stream(self.stream):
            rc, res, status = _colour_call(self._lib.lfd_colour_multiview, self._ctx, batch, out_buffers, support_thresh_px, mode, with_status,
                                           counters, self.device)
        self._check(rc, "lfd_colour_multiview")
        return (res, status) if with_status else res

    def gain_accumulate(self, batch: PreparedBatch, out_buffers, support_thresh_px: float, table: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The exposure statistics of per-image gain compensation (lfd_gain_accumulate): for every point ``out_buffers`` holds for
        ``batch`` (an OutputBuffers on the context's stream, or a collected TriangulationOutput; nothing of it changes) and every neighbour
        slot that confirms it - the multi-view colour's views - the reference's and the neighbour's colour are added, as exact integers, to row
        ``ref * k + slot`` of ``table``: int64 (n_refs * k, 7) on the device, columns N, Sref[3], Snbr[3], ADDED to (None: a zeroed one is
        made).  Asynchronous; returns the table."""
        self._same_device(batch)
        with torch.cuda.stream(self.stream):
            rc, table = _gain_accumulate_call(self._lib.lfd_gain_accumulate, self._ctx, batch, out_buffers, support_thresh_px, table, self.device)
        self._check(rc, "lfd_gain_accumulate")
        return table

    def gain_apply(self, rgb: torch.Tensor, ref_counts, factors) -> torch.Tensor:
        """Gain compensation of a cloud's colours (lfd_gain_apply): a new (n, 3) tensor min(rgb * f, 1) per channel, f the row
        of ``factors`` (n_refs, 3) of the point's reference - the cloud is the concatenation of ``ref_counts`` points per reference."""
        with torch.cuda.stream(self.stream):
            rc, out = _gain_apply_call(self._lib.lfd_gain_apply, self._ctx, rgb, ref_counts, factors, self.device)
        self._check(rc, "lfd_gain_apply")
        return out

    def far_accumulate(self, batch: PreparedBatch, far_thresh_px: float, far_certainty: float, far_min_views: int, shell_cells: int,
                       table: Optional[torch.Tensor] = None, counters: Optional[torch.Tensor] = None,
                       flags: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The statistics of the far-field shell (lfd_far_accumulate): every grid cell of ``batch`` that all its confident
        neighbours see at infinity adds its direction, its colour and a count to its direction cell's row of ``table``: int64 (6 S S, 7) on
        the device, ADDED to (None: a zeroed one is made); ``counters``: int64 (n_refs,) far cells per reference, added to; ``flags``: uint8
        (n_refs, H * W), written 1 for the far cells (lfd_far_accumulate_flags).  One launch on the context's stream, asynchronous; returns
        the table."""
        self._same_device(batch, None, table, counters, flags)
        with torch.cuda.stream(self.stream):
            fn = self._lib.lfd_far_accumulate if flags is None else self._lib.lfd_far_accumulate_flags
            rc, table = _far_accumulate_call(fn, self._ctx, batch, far_thresh_px, far_certainty, far_min_views, shell_cells, table, counters,
                                             self.device, flags)
        self._check(rc, "lfd_far_accumulate")
        return table

    def epipolar_audit(self, batch: PreparedBatch, audit_certainty: float, table: Optional[torch.Tensor] = None,
                       best: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The epipolar audit's statistics (lfd_epipolar_audit): every confident match of ``batch`` is measured against its pair's
        epipolar line and counted in row ``r * k + j`` of ``table``: int64 (n_refs * k, 66) on the device - usable, degenerate, 64 bins of an
        eighth of a neighbour's camera pixel - ADDED to (None: a zeroed one is made); ``best``: uint8 (n_refs, H * W), written with the smallest
        bin of each cell (255: none).  One launch on the context's stream, asynchronous; returns the table."""
        self._same_device(batch, None, table, best)
        with torch.cuda.stream(self.stream):
            rc, table = _epipolar_audit_call(self._lib.lfd_epipolar_audit, self._ctx, batch, audit_certainty, table, best, self.device)
        self._check(rc, "lfd_epipolar_audit")
        return table

    def pose_accumulate(self, batch: PreparedBatch, pose_certainty: float, pose_inlier_px: float,
                        table: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The pose refinement's statistics (lfd_pose_accumulate): every confident match of ``batch`` adds its row of the
        Gauss-Newton normal equations of the epipolar error, as quantised integers, to row ``r * k + j`` of ``table``: int64 (n_refs * k, 32) on
        the device, ADDED to (None: a zeroed one is made).  One launch on the context's stream, asynchronous; returns the table."""
        self._same_device(batch, None, table)
        with torch.cuda.stream(self.stream):
            rc, table = _pose_accumulate_call(self._lib.lfd_pose_accumulate, self._ctx, batch, pose_certainty, pose_inlier_px, table, self.device)
        self._check(rc, "lfd_pose_accumulate")
        return table

    def far_emit(self, table: torch.Tensor, shell_cells: int, min_samples: int, centre, radius: float, with_normals: bool = False):
        """The shell's points (lfd_far_emit) from ``table``: (xyz, rgb, normals or None, samples) device tensors, one record per
        direction cell with at least ``min_samples`` samples, in key order, at ``centre + radius * d_hat``.  Synchronous."""
        with torch.cuda.stream(self.stream):
            rc, _n, xyz, rgb, nrm, smp = _far_emit_call(self._lib.lfd_far_emit, self._ctx, table, shell_cells, min_samples, centre, radius,
                                                        with_normals, None, self.device)
        self._check(rc, "lfd_far_emit")
        return xyz, rgb, nrm, smp

    def pack_ply_normals(self, xyz: torch.Tensor, normals: torch.Tensor, rgb: torch.Tensor) -> torch.Tensor:
        """(n*27,) u8 device tensor: the body of a PLY whose header lists x y z nx ny nz red green blue."""
        xyz, normals, rgb = self._pts(xyz, 3, "xyz"), self._pts(normals, 3, "normals"), self._pts(rgb, 3, "rgb")
        n = int(xyz.shape[0])
        if int(normals.shape[0]) != n or int(rgb.shape[0]) != n:
            raise ValueError("pack_ply_normals: xyz, normals and rgb must have the same number of rows")
        out = torch.empty((max(n * 27, 4),), dtype=torch.uint8, device=xyz.device)
        self._check(self._lib.lfd_pack_ply_normals(self._ctx, xyz.data_ptr(), normals.data_ptr(), rgb.data_ptr(), n, out.data_ptr()),
                    "lfd_pack_ply_normals")
        return out[:n * 27]

    def knn_dist2(self, xyz: torch.Tensor, cell_size: float = 0.0) -> torch.Tensor:
        """The exact mean squared distance of every point to its three nearest neighbours (lfd_knn_dist2): (n,) float32 on the
        device, bit for bit what a brute-force loop over all pairs gives, whatever ``cell_size`` (the side of the search grid's cells; 0 =
        automatic).  ``self.knn_stats`` then holds (cell size used, occupied cells, points in the fullest cell, points finished by the brute-force
        pass).  Synchronous.  Raises ``KnnInputRefused`` as ``_knn_call`` describes."""
        with torch.cuda.stream(self.stream):
            out, self.knn_stats = _knn_call(self._lib.lfd_knn_dist2, self._ctx, "lfd_knn_dist2", xyz, cell_size, self.device,
                                            lambda: self._lib.lfd_last_error(self._ctx).decode())
        return out

    def cap_spatial(self, xyz: torch.Tensor, err: Optional[torch.Tensor], budget: int) -> torch.Tensor:
        """The spatial point cap (lfd_cap_spatial): the int64 device tensor of the input indices of at most ``budget`` points, one
        per cell of the coarsest Morton level with ``budget`` occupied cells, picked evenly along the curve, each cell's point of smallest ``err``
        (lowest index on ties and with ``err`` None); ascending, so ``xyz[keep]`` is the input under a mask.  ``self.cap_stats`` then holds
        (level, cells at that level, cells one level up, longest side of the bounding box).  Synchronous.  Raises ``CapInputRefused`` for a
        non-finite coordinate."""
        with torch.cuda.stream(self.stream):
            keep, self.cap_stats = _cap_call(self._lib.lfd_cap_spatial, self._ctx, "lfd_cap_spatial", xyz, err, budget, self.device,
                                             lambda: self._lib.lfd_last_error(self._ctx).decode())
        return keep

    def thin_footprint(self, xyz: torch.Tensor, err: Optional[torch.Tensor], ref_counts, ref_rows, thin_cells: float):
        """Footprint-adaptive thinning (lfd_thin_footprint): one point per cell of an octree over the cloud, every point at the
        level whose cell is ``thin_cells`` match-grid cells of its own reference camera at its depth, each cell's point of smallest ``err``
        (lowest index on ties and with ``err`` None).  Returns ``(keep, counts)``: the int64 device tensor of the kept input indices, ascending,
        so ``xyz[keep]`` is the input under a mask, and the kept points per reference.  ``self.thin_stats`` then holds (points per level, cells
        per level, longest side of the bounding box).  Synchronous.  Raises ``ThinInputRefused`` for a non-finite coordinate."""
        with torch.cuda.stream(self.stream):
            keep, counts, self.thin_stats = _thin_call(self._lib.lfd_thin_footprint, self._ctx, "lfd_thin_footprint", xyz, err, ref_counts, ref_rows,
                                                       thin_cells, self.device, lambda: self._lib.lfd_last_error(self._ctx).decode())
        return keep, counts

    def pack_gaussians(self, xyz: torch.Tensor, normals: torch.Tensor, rgb: torch.Tensor, dist2: torch.Tensor, opacity: float = 0.1,
                       flatten: float = 1.0, max_scale: float = 0.0) -> torch.Tensor:
        """(n*68,) u8 device tensor: the body of a 3DGS point_cloud.ply at SH degree 0 (lfd_pack_gaussians; ``writers.gaussian_ply_header``)."""
        with torch.cuda.stream(self.stream):
            return _pack_gaussians_call(self._lib.lfd_pack_gaussians, self._ctx, "lfd_pack_gaussians", xyz, normals, rgb, dist2, opacity, flatten,
                                        max_scale, self.device, lambda: self._lib.lfd_last_error(self._ctx).decode())

    def quantise_rgb(self, rgb: torch.Tensor) -> torch.Tensor:
        rgb = self._pts(rgb, 3, "rgb")
        out = torch.empty(rgb.shape, dtype=torch.uint8, device=rgb.device)
        self._check(self._lib.lfd_quantise_rgb(self._ctx, rgb.data_ptr(), int(rgb.shape[0]), out.data_ptr()), "lfd_quantise_rgb")
        return out

    # -- N3: image preparation on the device -----------------------------------------------------------------
    def prepare_image(self, rgb: torch.Tensor, size_wh, mask01: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``Image.resize(size_wh, BILINEAR)`` of a decoded (h, w, 3) u8 device image, then masked pixels black
        (upstream core/image_utils.py:69-91), bit for bit like Pillow.  Returns a (h_out, w_out, 3) u8 device tensor."""
        if rgb.dtype != torch.uint8 or not rgb.is_cuda or rgb.dim() != 3 or rgb.shape[2] != 3:
            raise ValueError("rgb must be a (h, w, 3) uint8 device tensor")
        rgb = rgb.contiguous()
        w_out, h_out = int(size_wh[0]), int(size_wh[1])
        if mask01 is not None:
            if mask01.dtype != torch.uint8 or not mask01.is_cuda or tuple(mask01.shape) != (h_out, w_out):
                raise ValueError("mask01 must be a (h_out, w_out) uint8 device tensor")
            mask01 = mask01.contiguous()
        out = torch.empty((h_out, w_out, 3), dtype=torch.uint8, device=rgb.device)
        self._check(self._lib.lfd_prepare_image(self._ctx, rgb.data_ptr(), int(rgb.shape[1]), int(rgb.shape[0]), w_out, h_out,
                                                mask01.data_ptr() if mask01 is not None else None, out.data_ptr()), "lfd_prepare_image")
        return out

    def prepare_mask(self, mask_l: torch.Tensor, size_wh, threshold: float = 0.5, invert: bool = False) -> torch.Tensor:
        """``load_mask_resized_np`` after the "L" conversion: NEAREST resize + threshold (core/image_utils.py:40-66)."""
        if mask_l.dtype != torch.uint8 or not mask_l.is_cuda or mask_l.dim() != 2:
            raise ValueError("mask_l must be a (h, w) uint8 device tensor")
        mask_l = mask_l.contiguous()
        w_out, h_out = int(size_wh[0]), int(size_wh[1])
        out = torch.empty((h_out, w_out), dtype=torch.uint8, device=mask_l.device)
        self._check(self._lib.lfd_prepare_mask(self._ctx, mask_l.data_ptr(), int(mask_l.shape[1]), int(mask_l.shape[0]), w_out, h_out,
                                               C.c_float(threshold), 1 if invert else 0, out.data_ptr()), "lfd_prepare_mask")
        return out

    def undistort_image(self, src: torch.Tensor, distortion, nearest: bool = False, with_valid: bool = False, count: bool = False,
                        workspace: Optional[str] = None):
        """A decoded (h, w, 3) or (h, w) u8 device image resampled through the camera's distortion model into the pinhole image of the same
        intrinsics (lfd_undistort_image); ``distortion``: the twelve f64 parameters of ``CameraRecord.distortion``;
        ``nearest``: one tap per pixel (mask planes).  Returns ``(dst, valid255 or None, n_invalid or None)``: ``valid255`` (h, w) u8, 255
        where the photograph covers the pixel; ``count``: the call synchronises and reports the invalid pixels, else it is asynchronous on
        the context's stream.  ``workspace``: a name - the outputs are then views of buffers this context owns under that name and reuses
        (valid until the next call with the same name: everything runs in stream order) instead of fresh tensors."""
        if src.dtype != torch.uint8 or src.device != self.device or src.dim() not in (2, 3) or (src.dim() == 3 and src.shape[2] != 3):
            raise ValueError("src must be a (h, w) or (h, w, 3) uint8 tensor on this context's device")
        src = src.contiguous()
        h, w = int(src.shape[0]), int(src.shape[1])
        intr, dist = _undistort_parameters(distortion)
        dst = self._undistort_buffer(workspace, "dst", src.numel()).view(src.shape)
        valid = self._undistort_buffer(workspace, "valid", h * w).view(h, w) if with_valid else None
        n_bad = C.c_int64(-1)
        self._check(self._lib.lfd_undistort_image(self._ctx, src.data_ptr(), w, h, 1 if src.dim() == 2 else 3, 1 if nearest else 0, intr, dist,
                                                  dst.data_ptr(), valid.data_ptr() if with_valid else None, C.byref(n_bad) if count else None),
                    "lfd_undistort_image")
        return dst, valid, (int(n_bad.value) if count else None)

    def _undistort_buffer(self, workspace: Optional[str], part: str, nbytes: int) -> torch.Tensor:
        if workspace is None:
            return torch.empty((int(nbytes),), dtype=torch.uint8, device=self.device)
        buf = self._undistort_ws.get((workspace, part))
        if buf is None or buf.numel() < nbytes:
            buf = self._undistort_ws[(workspace, part)] = torch.empty((int(nbytes),), dtype=torch.uint8, device=self.device)
        return buf[:int(nbytes)]

    # -- S: selection stage on the device ----------------------------------------------------------------
    def seed_rng(self, seed: int) -> None:
        """Seed the context's legacy MT19937 stream like ``np.random.seed(seed)``."""
        self._check(self._lib.lfd_rng_seed(self._ctx, C.c_uint32(int(seed) & 0xFFFFFFFF)), "lfd_rng_seed")

    def rng_state(self):
        key = (C.c_uint32 * 624)()
        pos = C.c_int32(0)
        self._check(self._lib.lfd_rng_get_state(self._ctx, key, C.byref(pos)), "lfd_rng_get_state")
        return np.frombuffer(key, dtype=np.uint32).copy(), int(pos.value)

    def set_rng_state(self, key: np.ndarray, pos: int) -> None:
        k = np.ascontiguousarray(key, dtype=np.uint32)
        self._check(self._lib.lfd_rng_set_state(self._ctx, k.ctypes.data_as(C.POINTER(C.c_uint32)), int(pos)),
                    "lfd_rng_set_state")

    def checkpoint_rng(self, place: int) -> None:
        """The stream put aside on the device, in stream order (no host wait): lfd_rng_checkpoint."""
        self._check(self._lib.lfd_rng_checkpoint(self._ctx, int(place)), "lfd_rng_checkpoint")

    def rollback_rng(self, place: int) -> None:
        """... and taken back: the stream continues from where ``checkpoint_rng(place)`` saw it."""
        self._check(self._lib.lfd_rng_rollback(self._ctx, int(place)), "lfd_rng_rollback")

    def select_samples(self, best_cert: torch.Tensor, M: int, cap: float = 0.9, border: int = 2, tiles: int = 24,
                       s_override: float = 0.0) -> torch.Tensor:
        """Coverage sampling (filter mode) of one reference's aggregated certainty map on the device;
        returns the selected cells (int64 device tensor, ascending).  Raises ValueError in the cases
        upstream's ``np.random.choice`` does."""
        if best_cert.dtype != torch.float32 or not best_cert.is_cuda or best_cert.dim() != 2:
            raise ValueError("best_cert must be a 2-D float32 device tensor")
        bc = best_cert.contiguous()
        H, W = bc.shape
        cap_n = int(M) + int(tiles) * int(tiles) + 64
        out = torch.empty((cap_n,), dtype=torch.int64, device=bc.device)
        n = C.c_int32(0)
        st = C.c_int32(0)
        rc = self._lib.lfd_select_samples(self._ctx, bc.data_ptr(), H, W, int(M), C.c_float(cap), int(border), int(tiles),
                                          C.c_float(s_override), out.data_ptr(), cap_n, C.byref(n), C.byref(st))
        if rc != 0 and st.value in (1, 2, 3):
            raise ValueError(self._lib.lfd_last_error(self._ctx).decode().replace("selection: ", ""))
        if rc != 0 and st.value == 4:
            raise SelectionInexact(self._lib.lfd_last_error(self._ctx).decode())
        self._check(rc, "lfd_select_samples")
        return out[:int(n.value)]

    TOP_M_MAX = 16384

    def select_top_m(self, best_cert: torch.Tensor, M: int, cap: float = 0.9) -> torch.Tensor:
        """no_filter selection: the M largest capped certainties, descending (ties by cell index)."""
        if best_cert.dtype != torch.float32 or not best_cert.is_cuda or best_cert.dim() != 2:
            raise ValueError("best_cert must be a 2-D float32 device tensor")
        bc = best_cert.contiguous()
        H, W = bc.shape
        cap_n = max(min(int(M), H * W), 1)
        out = torch.empty((cap_n,), dtype=torch.int64, device=bc.device)
        n, st = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.lfd_select_top_m(self._ctx, bc.data_ptr(), H, W, int(M), C.c_float(cap), out.data_ptr(), cap_n,
                                               C.byref(n), C.byref(st)), "lfd_select_top_m")
        return out[:int(n.value)]

    # -- launches (asynchronous on self.stream) -------------------------------------------------------
    def prepare(self, batch: PreparedBatch, params: lfd_params) -> None:
        """Upload the batch's descriptor tables and derive its per-pair constants now (lfd_prepare_batch); the launch that follows
        for the same batch then finds them in place."""
        self._same_device(batch)
        self._check(self._lib.lfd_prepare_batch(self._ctx, C.byref(batch.c), C.byref(params)), "lfd_prepare_batch")

    def launch_aggregate(self, batch: PreparedBatch, params: lfd_params, best_cert: torch.Tensor,
                         best_slot: Optional[torch.Tensor]) -> None:
        self._same_device(batch, None, best_cert, best_slot)
        self._check(self._lib.lfd_aggregate(self._ctx, C.byref(batch.c), C.byref(params), best_cert.data_ptr(),
                                            best_slot.data_ptr() if best_slot is not None else None), "lfd_aggregate")

    def launch_dense(self, batch: PreparedBatch, params: lfd_params, out: OutputBuffers) -> None:
        self._same_device(batch, out)
        out.normals_valid = False             # (refilled)
        self._check(self._lib.lfd_triangulate_dense(self._ctx, C.byref(batch.c), C.byref(params), C.byref(out.c),
                                                    out.ref_offsets.data_ptr(),
                                                    out.seg_counts.data_ptr() if out.with_segments else None),
                    "lfd_triangulate_dense")

    # -- the file payload straight from the kernel ----------------------------------------------------------------------------------------
    def launch_dense_ply(self, batch: PreparedBatch, params: lfd_params, records: torch.Tensor, ref_offsets: torch.Tensor,
                         seg_counts: Optional[torch.Tensor] = None) -> None:
        """lfd_triangulate_dense_ply: ``records`` (uint8, capacity * 15) receives the 15-byte PLY vertex records of the survivors in raster
        order per reference; ``ref_offsets`` (int64, n_refs + 1) their exclusive prefix.  Asynchronous."""
        self._same_device(batch, None, records, ref_offsets, seg_counts)
        if records.dtype != torch.uint8 or ref_offsets.dtype != torch.int64 or not records.is_contiguous():
            raise ValueError("records must be a contiguous uint8 tensor, ref_offsets int64")
        self._check(self._lib.lfd_triangulate_dense_ply(self._ctx, C.byref(batch.c), C.byref(params), records.data_ptr(), int(records.numel()) // 15,
                                                        ref_offsets.data_ptr(), seg_counts.data_ptr() if seg_counts is not None else None, None, None),
                    "lfd_triangulate_dense_ply")

    def triangulate_dense_ply(self, batch: PreparedBatch, params: lfd_params):
        """(PLY body as a uint8 device tensor, ref_offsets host int64): what pack_ply makes of triangulate_dense's result, from one kernel."""
        cap = batch.n_refs * batch.H * batch.W
        rec = torch.empty((max(cap * 15, 4),), dtype=torch.uint8, device=self.device)
        offs = torch.zeros((batch.n_refs + 1,), dtype=torch.int64, device=self.device)
        self.launch_dense_ply(batch, params, rec, offs)
        self.check_launches()
        h = offs.cpu().numpy()
        return rec[:int(h[-1]) * 15], h

    def launch_dense_ply_segments(self, batch: PreparedBatch, params: lfd_params, records: torch.Tensor, ref_counts: torch.Tensor, table: torch.Tensor,
                                  seg_counts: Optional[torch.Tensor] = None) -> None:
        """lfd_triangulate_dense_ply_segments: the PLY records without a look-back - reference r's ``ref_counts[r]`` records start at byte
        ``15 * r * H * W`` of ``records`` (uint8, n_refs * H * W * 15), tile after tile in retirement order; ``table`` (int32 (n_tiles, 2)) says where
        each tile went.  Asynchronous."""
        self._same_device(batch, None, records, ref_counts, table, seg_counts)
        if records.dtype != torch.uint8 or ref_counts.dtype != torch.int64 or table.dtype != torch.int32 or not records.is_contiguous() or not table.is_contiguous():
            raise ValueError("records must be a contiguous uint8 tensor, ref_counts int64, table a contiguous int32 (n_tiles, 2) tensor")
        self._check(self._lib.lfd_triangulate_dense_ply_segments(self._ctx, C.byref(batch.c), C.byref(params), records.data_ptr(), int(records.numel()) // 15,
                                                                 ref_counts.data_ptr(), seg_counts.data_ptr() if seg_counts is not None else None, table.data_ptr()),
                    "lfd_triangulate_dense_ply_segments")

    def tiles_per_ref(self, H: int, W: int) -> int:
        return int(self._lib.lfd_dense_tiles_per_ref(int(H), int(W)))

    # -- unordered retirement (opt-in): tiles claim room with one atomic, the consumers restore raster order from the tile table ------------
    def launch_dense_segments(self, batch: PreparedBatch, params: lfd_params, out: OutputBuffers, table: torch.Tensor,
                              ref_counts: torch.Tensor) -> None:
        self._same_device(batch, out, table, ref_counts)
        out.normals_valid = False             # (refilled)
        if table.dtype != torch.int32 or ref_counts.dtype != torch.int64 or not table.is_contiguous():
            raise ValueError("table must be a contiguous int32 (n_tiles, 2) tensor, ref_counts int64 (n_refs,)")
        self._check(self._lib.lfd_triangulate_dense_segments(self._ctx, C.byref(batch.c), C.byref(params), C.byref(out.c), ref_counts.data_ptr(),
                                                             out.seg_counts.data_ptr() if out.with_segments else None, table.data_ptr()),
                    "lfd_triangulate_dense_segments")

    def triangulate_dense_segments(self, batch: PreparedBatch, params: lfd_params, with_cell: bool = True) -> SegmentedOutput:
        out = OutputBuffers(batch.n_refs * batch.H * batch.W, batch.n_refs, batch.k, self.device, with_cell)
        tpr = int(self._lib.lfd_dense_tiles_per_ref(batch.H, batch.W))
        table = torch.zeros((batch.n_refs * tpr, 2), dtype=torch.int32, device=self.device)
        counts = torch.zeros((batch.n_refs,), dtype=torch.int64, device=self.device)
        self.launch_dense_segments(batch, params, out, table, counts)
        self.check_launches()
        return SegmentedOutput(out, table, counts, batch.n_refs, batch.H, batch.W, batch.k)

    def order_segments(self, seg: SegmentedOutput, into: Optional[OutputBuffers] = None) -> TriangulationOutput:
        """The ordered structure-of-arrays result of a segmented launch: what lfd_triangulate_dense would have returned, bit for bit."""
        src = seg.buffers
        dst = into if into is not None else OutputBuffers(src.capacity, seg.n_refs, seg.k, self.device, with_cell=src.cell is not None)
        self._check(self._lib.lfd_order_segments(self._ctx, seg.n_refs, seg.H, seg.W, seg.table.data_ptr(), C.byref(src.c), C.byref(dst.c),
                                                 dst.ref_offsets.data_ptr()), "lfd_order_segments")
        dst.seg_counts.copy_(src.seg_counts)
        return dst.collect()

    def pack_ply_segments(self, seg: SegmentedOutput):
        """(PLY body in raster order as a u8 device tensor, ref_offsets (n_refs + 1,) host i64) straight from the unordered buffers."""
        cap = seg.buffers.capacity
        out = torch.empty((max(cap * 15, 4),), dtype=torch.uint8, device=self.device)
        offs = torch.zeros((seg.n_refs + 1,), dtype=torch.int64, device=self.device)
        self._check(self._lib.lfd_pack_ply_segments(self._ctx, seg.n_refs, seg.H, seg.W, seg.table.data_ptr(), seg.buffers.xyz.data_ptr(),
                                                    seg.buffers.rgb.data_ptr(), cap, out.data_ptr(), offs.data_ptr()), "lfd_pack_ply_segments")
        h = offs.cpu().numpy()
        return out[:int(h[-1]) * 15], h

    def pack_points3d_segments(self, seg: SegmentedOutput, id_base: int = 0):
        cap = seg.buffers.capacity
        out = torch.empty((max(cap * 43, 4),), dtype=torch.uint8, device=self.device)
        offs = torch.zeros((seg.n_refs + 1,), dtype=torch.int64, device=self.device)
        self._check(self._lib.lfd_pack_points3d_segments(self._ctx, seg.n_refs, seg.H, seg.W, seg.table.data_ptr(), seg.buffers.xyz.data_ptr(),
                                                         seg.buffers.rgb.data_ptr(), seg.buffers.err.data_ptr(), cap, int(id_base), out.data_ptr(),
                                                         offs.data_ptr()), "lfd_pack_points3d_segments")
        h = offs.cpu().numpy()
        return out[:int(h[-1]) * 43], h

    def launch_indexed(self, batch: PreparedBatch, params: lfd_params, sel_idx: torch.Tensor,
                       sel_offsets: Sequence[int], out: OutputBuffers) -> None:
        if sel_idx.dtype != torch.int64 or not sel_idx.is_cuda or not sel_idx.is_contiguous():
            raise ValueError("sel_idx must be a contiguous int64 device tensor")
        self._same_device(batch, out, sel_idx)
        offs = (C.c_int64 * (batch.n_refs + 1))(*[int(v) for v in sel_offsets])
        self._check(self._lib.lfd_triangulate_indexed(self._ctx, C.byref(batch.c), C.byref(params), sel_idx.data_ptr(),
                                                      offs, C.byref(out.c), out.ref_offsets.data_ptr(),
                                                      out.seg_counts.data_ptr(), out.seg_order.data_ptr()),
                    "lfd_triangulate_indexed")

    def launch_sampled(self, batch: PreparedBatch, params: lfd_params, M: int, out: OutputBuffers, cap: float = 0.9,
                       border: int = 2, tiles: int = 24, s_override: float = 0.0, sel_cells: Optional[torch.Tensor] = None) -> None:
        """One reference view through aggregate -> selection -> indexed triangulation in one asynchronous call
        (lfd_triangulate_sampled): no read-back in between, the selection count stays on the device."""
        self._same_device(batch, out, sel_cells)
        out.normals_valid = False             # (refilled)
        self._check(self._lib.lfd_triangulate_sampled(self._ctx, C.byref(batch.c), C.byref(params), int(M), C.c_float(cap), int(border),
                                                      int(tiles), C.c_float(s_override), C.byref(out.c), out.ref_offsets.data_ptr(),
                                                      out.seg_counts.data_ptr(), out.seg_order.data_ptr(), out.sel_info.data_ptr(),
                                                      sel_cells.data_ptr() if sel_cells is not None else None),
                    "lfd_triangulate_sampled")

    def launch_sampled_multi(self, batch: PreparedBatch, params: lfd_params, M: int, out: OutputBuffers, seeds: Sequence[int],
                             cap: float = 0.9, border: int = 2, tiles: int = 24) -> None:
        """Several reference views through the fused call at once, each on its own MT19937 stream (``seeds[r]``, like
        ``np.random.seed``): lfd_triangulate_sampled_multi.  ``out`` needs capacity n_refs * (M + tiles*tiles + 64)."""
        if len(seeds) != batch.n_refs:
            raise ValueError("one seed per reference")
        self._same_device(batch, out)
        out.normals_valid = False             # (refilled)
        arr = (C.c_uint32 * batch.n_refs)(*[int(v) & 0xFFFFFFFF for v in seeds])
        self._check(self._lib.lfd_triangulate_sampled_multi(self._ctx, C.byref(batch.c), C.byref(params), int(M), C.c_float(cap), int(border),
                                                            int(tiles), arr, C.byref(out.c), out.ref_offsets.data_ptr(),
                                                            out.seg_counts.data_ptr(), out.seg_order.data_ptr(), out.sel_info.data_ptr(), None),
                    "lfd_triangulate_sampled_multi")

    def launch_sampled_chain(self, batch: PreparedBatch, params: lfd_params, M: int, out: OutputBuffers,
                             s_overrides: Optional[Sequence[float]] = None, cap: float = 0.9, border: int = 2, tiles: int = 24,
                             sel_cells: Optional[torch.Tensor] = None) -> None:
        """Several reference views through the fused call at once on the context's ONE MT19937 stream, consumed in batch order
        (lfd_triangulate_sampled_chain): the results and the stream afterwards are those of ``n_refs`` successive ``launch_sampled`` calls.
        ``s_overrides[r]`` > 0: upstream's own normaliser of reference r.  ``out`` needs capacity n_refs * (M + tiles*tiles + 64)."""
        if s_overrides is not None and len(s_overrides) != batch.n_refs:
            raise ValueError("one normaliser per reference")
        self._same_device(batch, out, sel_cells)
        out.normals_valid = False             # (refilled)
        arr = (C.c_float * batch.n_refs)(*[float(v) for v in s_overrides]) if s_overrides is not None else None
        self._check(self._lib.lfd_triangulate_sampled_chain(self._ctx, C.byref(batch.c), C.byref(params), int(M), C.c_float(cap), int(border),
                                                            int(tiles), arr, C.byref(out.c), out.ref_offsets.data_ptr(),
                                                            out.seg_counts.data_ptr(), out.seg_order.data_ptr(), out.sel_info.data_ptr(),
                                                            sel_cells.data_ptr() if sel_cells is not None else None),
                    "lfd_triangulate_sampled_chain")

    def triangulate_sampled(self, batch: PreparedBatch, params: lfd_params, M: int, cap: float = 0.9, border: int = 2,
                            tiles: int = 24, s_override: float = 0.0, with_cell: bool = True) -> TriangulationOutput:
        out = OutputBuffers(int(M) + int(tiles) * int(tiles) + 64, 1, batch.k, self.device, with_cell)
        self.launch_sampled(batch, params, M, out, cap, border, tiles, s_override)
        with torch.cuda.stream(self.stream):                       # the read-back is ordered after the launch on ITS stream
            res = out.collect(indexed=True, check_selection=True)  # one copy: counts, selection status, launch status
        if res.launch_status != 0:
            self.check_launches()                                  # resets the device word and raises
        return res

    # -- convenience wrappers (synchronising) -------------------------------------------------------------
    def aggregate(self, batch: PreparedBatch, params: lfd_params):
        best = torch.empty((batch.n_refs, batch.H, batch.W), dtype=torch.float32, device=self.device)
        slot = torch.empty((batch.n_refs, batch.H, batch.W), dtype=torch.uint8, device=self.device)
        self.launch_aggregate(batch, params, best, slot)
        return best, slot

    def triangulate_dense(self, batch: PreparedBatch, params: lfd_params, capacity: Optional[int] = None,
                          with_cell: bool = True) -> TriangulationOutput:
        cap = batch.n_refs * batch.H * batch.W if capacity is None else int(capacity)
        out = OutputBuffers(cap, batch.n_refs, batch.k, self.device, with_cell)
        self.launch_dense(batch, params, out)
        self.check_launches()
        return out.collect()

    def triangulate_indexed(self, batch: PreparedBatch, params: lfd_params, sel_idx: torch.Tensor,
                            sel_offsets: Sequence[int], with_cell: bool = True) -> TriangulationOutput:
        out = OutputBuffers(int(sel_offsets[-1]), batch.n_refs, batch.k, self.device, with_cell)
        self.launch_indexed(batch, params, sel_idx, sel_offsets, out)
        self.check_launches()
        return out.collect(indexed=True)


class HostDensifier:
    """The CPU twin of :class:`HipDensifier` (``lfd_create_host`` + the ``*_host`` entry points of the C-ABI): the host
    build of the kernels' per-cell source over CPU tensors, on ``n_threads`` threads.  Explicitly chosen - for upstream's
    CPU-only configuration, for the CPU baseline of the benchmark and for parity checks - never a fallback: a
    :class:`HipDensifier` does not turn into one when the GPU is missing."""

    def __init__(self, n_threads: int = 0):
        self._lib = load_library()
        self._ctx = C.c_void_p()
        rc = self._lib.lfd_create_host(int(n_threads), C.byref(self._ctx))
        if rc != 0:
            raise HipBackendError(f"lfd_create_host failed ({rc}): {self._lib.lfd_last_error(None).decode()}")
        self.device = torch.device("cpu")
        self.n_threads = int(self._lib.lfd_host_threads(self._ctx))
        self.n_cams = 0
        self.fuse_voxels = 0           # occupied voxels of the last fuse_oriented call
        self.knn_stats = (0.0, 0, 0, 0)       # (cell size, occupied cells, fullest cell, brute-forced points) of the last knn_dist2 call
        self.cap_stats = (0, 0, 0, 0.0)       # (level, cells at it, cells one level up, longest side of the box) of the last cap_spatial call
        self.thin_stats = (np.zeros(THIN_LEVELS, np.int64), np.zeros(THIN_LEVELS, np.int64), 0.0)   # (points, cells per level, box side) of the last thin_footprint call

    close = HipDensifier.close
    __del__ = HipDensifier.__del__
    _check = HipDensifier._check
    _same_device = HipDensifier._same_device
    upload_cameras = HipDensifier.upload_cameras

    def check_launches(self) -> None:
        pass

    def local_corr(self, a: torch.Tensor, bf: torch.Tensor, warp: torch.Tensor) -> torch.Tensor:
        """HipDensifier.local_corr over CPU tensors (lfd_local_corr_host: the general kernel's routine on this context's threads)."""
        a, bf, warp, dims = _local_corr_arguments(a, bf, warp, self.device)
        out = torch.empty((dims[0], dims[1], dims[3]), dtype=torch.float32)
        sa, sb = (C.c_int64 * 3)(*a.stride()), (C.c_int64 * 4)(*bf.stride())
        self._check(self._lib.lfd_local_corr_host(self._ctx, a.data_ptr(), bf.data_ptr(), warp.data_ptr(), *dims, sa, sb, out.data_ptr()),
                    "lfd_local_corr_host")
        return out

    def refiner_block(self, x: torch.Tensor, dw_w: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, pw_wt: Optional[torch.Tensor] = None,
                      pw_b: Optional[torch.Tensor] = None) -> torch.Tensor:
        """HipDensifier.refiner_block over CPU tensors (lfd_refiner_block_host): the same routine, the same bits, whatever the thread count."""
        rc, out = _refiner_block_call(self._lib.lfd_refiner_block_host, self._ctx, x, dw_w, scale, shift, pw_wt, pw_b, self.device)
        self._check(rc, "lfd_refiner_block_host")
        return out

    def refiner_head(self, z: torch.Tensor, head_w: torch.Tensor, head_b: torch.Tensor, prev_warp: torch.Tensor,
                     prev_conf: Optional[torch.Tensor] = None, refine_init: float = 4.0) -> Tuple[torch.Tensor, torch.Tensor]:
        """HipDensifier.refiner_head over CPU tensors (lfd_refiner_head_host): the same routine, the same bits, whatever the thread count."""
        rc, warp, conf = _refiner_head_call(self._lib.lfd_refiner_head_host, self._ctx, z, head_w, head_b, prev_warp, prev_conf, refine_init,
                                            self.device)
        self._check(rc, "lfd_refiner_head_host")
        return warp, conf

    def cycle_gate(self, cert, warp_ab, warp_ba, w_match: int, h_match: int, certainty_thresh: float, cycle_thresh_px: float, axes=None,
                   inplace: bool = False, with_err: bool = False, rejected: Optional[torch.Tensor] = None):
        """HipDensifier.cycle_gate over CPU tensors (lfd_cycle_gate_host): the same per-cell routine, the same bits in the gated planes and counters."""
        rc, outs, errs = _cycle_gate_call(self._lib.lfd_cycle_gate_host, self._ctx, cert, warp_ab, warp_ba, w_match, h_match, certainty_thresh,
                                          cycle_thresh_px, axes, inplace, with_err, rejected, self.device)
        self._check(rc, "lfd_cycle_gate_host")
        return outs, errs

    def support_filter(self, batch: PreparedBatch, out_buffers, min_support: int, support_thresh_px: float, with_support: bool = False,
                       into: Optional[OutputBuffers] = None):
        """HipDensifier.support_filter over CPU tensors (lfd_support_filter_host): the same per-(point, slot) routine, the same bits in every output."""
        self._same_device(batch)
        rc, res, support = _support_filter_call(self._lib.lfd_support_filter_host, self._ctx, batch, out_buffers, min_support, support_thresh_px,
                                                with_support, into, self.device)
        self._check(rc, "lfd_support_filter_host")
        return (res, support) if with_support else res

    def refine_multiview(self, batch: PreparedBatch, out_buffers, support_thresh_px: float, reproj_thresh: float, with_status: bool = False,
                         counters: Optional[torch.Tensor] = None, precision: bool = False):
        """HipDensifier.refine_multiview over CPU tensors (lfd_refine_multiview[_weighted]_host): the same per-point routine, host build."""
        self._same_device(batch)
        name = "lfd_refine_multiview_weighted_host" if precision else "lfd_refine_multiview_host"
        rc, res, status = _refine_call(getattr(self._lib, name), self._ctx, batch, out_buffers, support_thresh_px, reproj_thresh,
                                       with_status, counters, self.device, precision)
        self._check(rc, name)
        return (res, status) if with_status else res

    def depth_sigma_filter(self, batch: PreparedBatch, out_buffers, max_rel_sigma: float, iso_sigma_px: float = 0.0,
                           refine_status: Optional[torch.Tensor] = None, support_thresh_px: float = 0.0, with_sigma: bool = False,
                           into: Optional[OutputBuffers] = None):
        """HipDensifier.depth_sigma_filter over CPU tensors (lfd_depth_sigma_filter_host): the same per-point routine, host build."""
        self._same_device(batch)
        rc, res, sigma, sigma_out = _depth_sigma_call(self._lib.lfd_depth_sigma_filter_host, self._ctx, batch, out_buffers, max_rel_sigma,
                                                      iso_sigma_px, refine_status, support_thresh_px, with_sigma, into, self.device)
        self._check(rc, "lfd_depth_sigma_filter_host")
        return (res, sigma, sigma_out) if with_sigma else res

    def photo_gate(self, batch: PreparedBatch, out_buffers, window_cells: int, min_ncc: float, min_texture: float, with_status: bool = False,
                   with_ncc: bool = False, counters: Optional[torch.Tensor] = None, into: Optional[OutputBuffers] = None):
        """HipDensifier.photo_gate over CPU tensors (lfd_photo_gate_host): the same per-point routine, the same decisions."""
        self._same_device(batch)
        rc, res, status, ncc = _photo_gate_call(self._lib.lfd_photo_gate_host, self._ctx, batch, out_buffers, window_cells, min_ncc, min_texture,
                                                with_status, with_ncc, counters, into, self.device)
        self._check(rc, "lfd_photo_gate_host")
        extra = ((status,) if with_status else ()) + ((ncc,) if with_ncc else ())
        return (res,) + extra if extra else res

    def estimate_normals(self, batch: PreparedBatch, out_buffers, radius: int, depth_step_rel: float, reproj_thresh: float,
                         with_status: bool = False, counters: Optional[torch.Tensor] = None):
        """HipDensifier.estimate_normals over CPU tensors (lfd_estimate_normals_host): the same per-point routine, host build."""
        self._same_device(batch)
        rc, res, status = _normals_call(self._lib.lfd_estimate_normals_host, self._ctx, batch, out_buffers, radius, depth_step_rel, reproj_thresh,
                                        with_status, counters, self.device)
        self._check(rc, "lfd_estimate_normals_host")
        return (res, status) if with_status else res

    def colour_multiview(self, batch: PreparedBatch, out_buffers, support_thresh_px: float, mode: str, with_status: bool = False,
                         counters: Optional[torch.Tensor] = None):
        """HipDensifier.colour_multiview over CPU tensors (lfd_colour_multiview_host): the same per-point routine, the same bits."""
        self._same_device(batch)
        rc, res, status = _colour_call(self._lib.lfd_colour_multiview_host, self._ctx, batch, out_buffers, support_thresh_px, mode, with_status,
                                       counters, self.device)
        self._check(rc, "lfd_colour_multiview_host")
        return (res, status) if with_status else res

    def gain_accumulate(self, batch: PreparedBatch, out_buffers, support_thresh_px: float, table: Optional[torch.Tensor] = None) -> torch.Tensor:
        """HipDensifier.gain_accumulate over CPU tensors (lfd_gain_accumulate_host): the same routine, the same integers."""
        self._same_device(batch)
        rc, table = _gain_accumulate_call(self._lib.lfd_gain_accumulate_host, self._ctx, batch, out_buffers, support_thresh_px, table, self.device)
        self._check(rc, "lfd_gain_accumulate_host")
        return table

    def gain_apply(self, rgb: torch.Tensor, ref_counts, factors) -> torch.Tensor:
        """HipDensifier.gain_apply over CPU tensors (lfd_gain_apply_host): the same bits."""
        rc, out = _gain_apply_call(self._lib.lfd_gain_apply_host, self._ctx, rgb, ref_counts, factors, self.device)
        self._check(rc, "lfd_gain_apply_host")
        return out

    def far_accumulate(self, batch: PreparedBatch, far_thresh_px: float, far_certainty: float, far_min_views: int, shell_cells: int,
                       table: Optional[torch.Tensor] = None, counters: Optional[torch.Tensor] = None,
                       flags: Optional[torch.Tensor] = None) -> torch.Tensor:
        """HipDensifier.far_accumulate over CPU tensors (lfd_far_accumulate[_flags]_host): the same routines, the same integers."""
        self._same_device(batch, None, table, counters, flags)
        fn = self._lib.lfd_far_accumulate_host if flags is None else self._lib.lfd_far_accumulate_flags_host
        rc, table = _far_accumulate_call(fn, self._ctx, batch, far_thresh_px, far_certainty, far_min_views, shell_cells, table, counters,
                                         self.device, flags)
        self._check(rc, "lfd_far_accumulate_host")
        return table

    def epipolar_audit(self, batch: PreparedBatch, audit_certainty: float, table: Optional[torch.Tensor] = None,
                       best: Optional[torch.Tensor] = None) -> torch.Tensor:
        """HipDensifier.epipolar_audit over CPU tensors (lfd_epipolar_audit_host): the same routine, the same integers."""
        self._same_device(batch, None, table, best)
        rc, table = _epipolar_audit_call(self._lib.lfd_epipolar_audit_host, self._ctx, batch, audit_certainty, table, best, self.device)
        self._check(rc, "lfd_epipolar_audit_host")
        return table

    def pose_accumulate(self, batch: PreparedBatch, pose_certainty: float, pose_inlier_px: float,
                        table: Optional[torch.Tensor] = None) -> torch.Tensor:
        """HipDensifier.pose_accumulate over CPU tensors (lfd_pose_accumulate_host): the same routine, the same integers."""
        self._same_device(batch, None, table)
        rc, table = _pose_accumulate_call(self._lib.lfd_pose_accumulate_host, self._ctx, batch, pose_certainty, pose_inlier_px, table, self.device)
        self._check(rc, "lfd_pose_accumulate_host")
        return table

    def far_emit(self, table: torch.Tensor, shell_cells: int, min_samples: int, centre, radius: float, with_normals: bool = False):
        """HipDensifier.far_emit over CPU tensors (lfd_far_emit_host): the same bits."""
        rc, _n, xyz, rgb, nrm, smp = _far_emit_call(self._lib.lfd_far_emit_host, self._ctx, table, shell_cells, min_samples, centre, radius,
                                                    with_normals, None, self.device)
        self._check(rc, "lfd_far_emit_host")
        return xyz, rgb, nrm, smp

    def pack_ply_normals(self, xyz: torch.Tensor, normals: torch.Tensor, rgb: torch.Tensor) -> torch.Tensor:
        """HipDensifier.pack_ply_normals over CPU tensors: the host writer's records (core/writers.py), the same bytes."""
        from .image_io import to_uint8_rgb
        from .writers import ply_records
        rec = ply_records(xyz.numpy(), to_uint8_rgb(rgb.numpy()), normals=normals.numpy())
        return torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())

    def consensus_filter(self, xyz: torch.Tensor, rgb: Optional[torch.Tensor], err: Optional[torch.Tensor], ref_counts, radius: float, min_refs: int,
                         with_consensus: bool = False):
        """HipDensifier.consensus_filter over CPU tensors (lfd_consensus_filter_host): the same per-point routine, the same bits in every output."""
        return _consensus_call(self._lib.lfd_consensus_filter_host, self._ctx, "lfd_consensus_filter_host", xyz, rgb, err, ref_counts, radius,
                               min_refs, with_consensus, self.device, lambda: self._lib.lfd_last_error(self._ctx).decode())

    def component_filter(self, xyz: torch.Tensor, rgb: Optional[torch.Tensor], err: Optional[torch.Tensor], ref_counts, radius: float,
                         min_points: int, with_sizes: bool = False, with_labels: bool = False):
        """HipDensifier.component_filter over CPU tensors (lfd_component_filter_host): a sequential union-find over the same links, the same bits
        in every output."""
        return _component_call(self._lib.lfd_component_filter_host, self._ctx, "lfd_component_filter_host", xyz, rgb, err, ref_counts, radius,
                               min_points, with_sizes, with_labels, self.device, lambda: self._lib.lfd_last_error(self._ctx).decode())

    def freespace_filter(self, xyz: torch.Tensor, rgb: Optional[torch.Tensor], err: Optional[torch.Tensor], ref_counts, cam_P, cam_wh, plane,
                         tol: float, min_violations: int, with_counts: bool = False):
        """HipDensifier.freespace_filter over CPU tensors (lfd_freespace_filter_host): the same per-point routine, the same bits in every output."""
        return _freespace_call(self._lib.lfd_freespace_filter_host, self._ctx, "lfd_freespace_filter_host", xyz, rgb, err, ref_counts, cam_P, cam_wh,
                               plane, tol, min_violations, with_counts, self.device, lambda: self._lib.lfd_last_error(self._ctx).decode())

    def render_depth(self, xyz, normals, cam_P, cam_wh, plane, splat_cells: int = 1, window_cells: int = 3, tol: float = 0.02,
                     with_index: bool = False, cams_per_batch: int = 0):
        """HipDensifier.render_depth over CPU tensors or arrays (lfd_render_depth_host): the rule by its definition, the same bits in every output."""
        return _depth_call(self._lib.lfd_render_depth_host, self._ctx, "lfd_render_depth_host", xyz, normals, cam_P, cam_wh, plane, splat_cells,
                           window_cells, tol, with_index, cams_per_batch, self.device, lambda: self._lib.lfd_last_error(self._ctx).decode())

    def fuse_oriented(self, xyz: torch.Tensor, normals: torch.Tensor, rgb: torch.Tensor, voxel_size: float, with_counts: bool = False):
        """HipDensifier.fuse_oriented over CPU tensors (lfd_fuse_oriented_host): the same rule, with IEEE sqrt and divide in the normals' last step."""
        rows, self.fuse_voxels = _fuse_call(self._lib.lfd_fuse_oriented_host, self._ctx, "lfd_fuse_oriented_host", xyz, normals, rgb, voxel_size,
                                            with_counts, self.device, lambda: self._lib.lfd_last_error(self._ctx).decode())
        return rows

    def knn_dist2(self, xyz: torch.Tensor, cell_size: float = 0.0) -> torch.Tensor:
        """HipDensifier.knn_dist2 over CPU tensors (lfd_knn_dist2_host): the same bits, the same ``knn_stats``."""
        out, self.knn_stats = _knn_call(self._lib.lfd_knn_dist2_host, self._ctx, "lfd_knn_dist2_host", xyz, cell_size, self.device,
                                        lambda: self._lib.lfd_last_error(self._ctx).decode())
        return out

    def cap_spatial(self, xyz: torch.Tensor, err: Optional[torch.Tensor], budget: int) -> torch.Tensor:
        """HipDensifier.cap_spatial over CPU tensors (lfd_cap_spatial_host): the same indices, the same ``cap_stats``, whatever the thread count."""
        keep, self.cap_stats = _cap_call(self._lib.lfd_cap_spatial_host, self._ctx, "lfd_cap_spatial_host", xyz, err, budget, self.device,
                                         lambda: self._lib.lfd_last_error(self._ctx).decode())
        return keep

    def thin_footprint(self, xyz: torch.Tensor, err: Optional[torch.Tensor], ref_counts, ref_rows, thin_cells: float):
        """HipDensifier.thin_footprint over CPU tensors (lfd_thin_footprint_host): the same indices, counts and ``thin_stats``, whatever the thread
        count."""
        keep, counts, self.thin_stats = _thin_call(self._lib.lfd_thin_footprint_host, self._ctx, "lfd_thin_footprint_host", xyz, err, ref_counts,
                                                   ref_rows, thin_cells, self.device, lambda: self._lib.lfd_last_error(self._ctx).decode())
        return keep, counts

    def pack_gaussians(self, xyz: torch.Tensor, normals: torch.Tensor, rgb: torch.Tensor, dist2: torch.Tensor, opacity: float = 0.1,
                       flatten: float = 1.0, max_scale: float = 0.0) -> torch.Tensor:
        """HipDensifier.pack_gaussians over CPU tensors (lfd_pack_gaussians_host): IEEE sqrt and divide, the C library's log."""
        return _pack_gaussians_call(self._lib.lfd_pack_gaussians_host, self._ctx, "lfd_pack_gaussians_host", xyz, normals, rgb, dist2, opacity,
                                    flatten, max_scale, self.device, lambda: self._lib.lfd_last_error(self._ctx).decode())

    def aggregate(self, batch: PreparedBatch, params: lfd_params):
        self._same_device(batch)
        best = torch.empty((batch.n_refs, batch.H, batch.W), dtype=torch.float32)
        slot = torch.empty((batch.n_refs, batch.H, batch.W), dtype=torch.uint8)
        self._check(self._lib.lfd_aggregate_host(self._ctx, C.byref(batch.c), C.byref(params), best.data_ptr(), slot.data_ptr()),
                    "lfd_aggregate_host")
        return best, slot

    def triangulate_dense(self, batch: PreparedBatch, params: lfd_params, capacity: Optional[int] = None,
                          with_cell: bool = True) -> TriangulationOutput:
        self._same_device(batch)
        cap = batch.n_refs * batch.H * batch.W if capacity is None else int(capacity)
        out = OutputBuffers(cap, batch.n_refs, batch.k, self.device, with_cell)
        self._check(self._lib.lfd_triangulate_dense_host(self._ctx, C.byref(batch.c), C.byref(params), C.byref(out.c),
                                                         out.ref_offsets.data_ptr(), out.seg_counts.data_ptr()),
                    "lfd_triangulate_dense_host")
        return out.collect()

    def triangulate_indexed(self, batch: PreparedBatch, params: lfd_params, sel_idx: torch.Tensor,
                            sel_offsets: Sequence[int], with_cell: bool = True) -> TriangulationOutput:
        if sel_idx.dtype != torch.int64 or sel_idx.is_cuda or not sel_idx.is_contiguous():
            raise ValueError("sel_idx must be a contiguous int64 CPU tensor")
        self._same_device(batch)
        out = OutputBuffers(int(sel_offsets[-1]), batch.n_refs, batch.k, self.device, with_cell)
        offs = (C.c_int64 * (batch.n_refs + 1))(*[int(v) for v in sel_offsets])
        self._check(self._lib.lfd_triangulate_indexed_host(self._ctx, C.byref(batch.c), C.byref(params), sel_idx.data_ptr(), offs,
                                                           C.byref(out.c), out.ref_offsets.data_ptr(), out.seg_counts.data_ptr(),
                                                           out.seg_order.data_ptr()), "lfd_triangulate_indexed_host")
        return out.collect(indexed=True)
