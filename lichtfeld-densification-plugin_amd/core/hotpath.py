"""Per-run state of the per-reference hot path: the context of the C-ABI, the camera table, the prepared-image cache, and the ways of
triangulating a reference (the fused sampled call, its pipelined forms, the unfused three calls, the dense launch).

Replaces upstream core/pipeline.py:405-442 (``_collect_reference_matches`` epilogue) + :602-780 (``_triangulate_ref``): what those do on
the CPU per reference happens here through ``core/hip_backend.py`` (device) or the CPU twin (``backend="host"``)."""
from __future__ import annotations

import collections
import dataclasses
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip_backend as hb
from .image_io import to_uint8_rgb
from .packing import PackedReference
from .sampling import select_samples_with_coverage, upstream_weight_sum
from .stages import NULL_CLOCK
from .types import CameraRecord, DensePipelineConfig
from .writers import ply_records

# device_image_prep: bytes of prepared match-size images / masks kept on the device per run (LFD_PREPARED_CACHE_MB; 0 = keep none)
PREPARED_CACHE_BYTES = int(os.environ.get("LFD_PREPARED_CACHE_MB", "4096")) << 20


def _upload_u8(a, dev) -> torch.Tensor:
    """A u8 array to where the kernels run, without a host copy in between.  The loaders' caches hand out READ-ONLY arrays (a cached image must not be
    written to); torch warns when it wraps one - the wrapper here is only ever read (uploaded, or handed to the CPU twin, which takes const pointers)."""
    import warnings
    arr = np.ascontiguousarray(a, dtype=np.uint8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        t = torch.from_numpy(arr)
    return t if torch.device(dev).type == "cpu" else t.to(dev)


def _pool_kind(out: hb.OutputBuffers) -> int:
    """Which of the recycled buffers ``out`` belongs to: 0 a launch's own, 1 a support filter's destination, 2 / 3 a depth-uncertainty gate's
    (behind no / a support filter), + 4 a photo-consistency gate's - ``collect`` reports the points that went into a stage only for that
    stage's destinations."""
    return int(bool(out.filtered)) | (2 if getattr(out, "sigma_filtered", False) else 0) | (4 if getattr(out, "photo_filtered", False) else 0)


class HotPath:
    """Per-run state of the hot path: context, camera table, and the ways of triangulating a reference."""

    def __init__(self, cams: Sequence[CameraRecord], config: DensePipelineConfig, sample_cap: float, w_match: int,
                 h_match: int, dev: torch.device, densifier: Optional[hb.HipDensifier], clock=NULL_CLOCK):
        self.dev = dev
        self.clock = clock
        self.config = config
        self.sample_cap = float(sample_cap)
        self.w_match, self.h_match = int(w_match), int(h_match)
        self.on_host = dev.type == "cpu"          # config.backend == "host": the CPU twin, chosen by the caller
        if densifier is not None:
            self.dens = densifier
        else:
            self.dens = hb.HostDensifier(int(config.exp("host_threads"))) if self.on_host else hb.HipDensifier(dev)
        if self.dens.device.type != dev.type:
            raise ValueError(f"backend runs on {dev} but the densifier handed in lives on {self.dens.device}")
        self._own = densifier is None
        self._prepared: "collections.OrderedDict" = collections.OrderedDict()      # device_image_prep: camera -> (image, mask) at match size
        self._prepared_bytes = 0
        self._buf_pool: dict = {}              # recycled survivor buffers of the fused sampled calls
        self._norm_side = None                 # upstream's normaliser: side stream, free slots, border masks (begin_normaliser)
        self._norm_free: list = []
        self._norm_group, self._norm_grid = 1, None
        self._norm_masks: dict = {}
        self.dens.upload_cameras(cams)
        self.cams = list(cams) if bool(config.exp("upstream_fundamental")) else None
        # the kernels' floor is min(thresh, 0) when the planes arrive gated (hb.make_params); everything on the host that reasons about the
        # floor - the exactness checks below - keeps reading the CONFIGURED threshold
        self.params = hb.make_params(config, sample_cap)
        self.cycle_thresh_px = float(config.exp("cycle_thresh_px"))
        self._cycle_counter: Optional[torch.Tensor] = None      # int32 [LFD_MAX_SLOTS] where the kernels run: rejected cells per slot, added to
        self._cycle_pending = 0                                 # cells per slot gated since the counter was last read (it must not wrap)
        self.cycle_cells = self.cycle_rejected = 0
        self.min_support = int(config.exp("min_support_views"))
        self.support_thresh_px = float(config.support_threshold())
        self.support_in = self.support_kept = 0                 # points that reached the filter / that it kept, over the results the run used
        self._support_void = False                              # a grouped call failed as a whole: what is collected until the next launch is dropped
        self.refine = bool(config.exp("multiview_refine"))
        self.refine_weighted = bool(config.exp("precision_weighted_refine"))     # lfd_refine_multiview_weighted in its place
        # int64 [2] where the kernels run: points refined / confirmed but left alone ([3] weighted: + solved with weighted rows), added to
        self._refine_counter: Optional[torch.Tensor] = None
        # depth-uncertainty gate (lfd_depth_sigma_filter): the last stage behind support filter and re-triangulation
        self.max_sigma = float(config.exp("max_depth_sigma_rel"))
        self.iso_sigma_px = float(config.exp("match_sigma_px"))
        self.sigma_planes = self.max_sigma > 0.0 and self.iso_sigma_px == 0.0     # the gate reads the matcher's precision planes
        self.sigma_in = self.sigma_kept = 0                     # points that reached the gate / that it kept, over the results the run used
        # experimental['undistort_images']: per camera, the twelve parameters its decoded image is undistorted with in
        # prepare_on_device, or None (knob off, or a camera without distortion coefficients: no new code runs for it)
        # per-point normals (lfd_estimate_normals): the last stage, behind everything that moves or drops points
        self.normals = bool(config.exp("estimate_normals"))
        self.normal_radius = int(config.exp("normal_radius_cells"))
        self.normal_depth_step = float(config.exp("normal_depth_step_rel"))
        self._normal_counter: Optional[torch.Tensor] = None     # int64 [2] where the kernels run: points fitted / fallen back, added to
        # multi-view point colour (lfd_colour_multiview): a column rewrite behind the stages that move or drop points
        self.colour_mode = str(config.exp("multiview_colour"))
        self.colour = self.colour_mode != "off"
        self._colour_counter: Optional[torch.Tensor] = None     # int64 [2] where the kernels run: points blended / the sum of their views, added to
        # per-image exposure gains (lfd_gain_accumulate): statistics where the colour stage would run; reads only
        self.gain_mode = str(config.exp("gain_compensation"))
        self.gain = self.gain_mode != "off"
        # photo-consistency gate (lfd_photo_gate): behind the depth-uncertainty gate - it then sees the fewest points - and in
        # front of everything that reads the survivors' colours or cells
        self.photo_ncc = float(config.exp("min_photo_ncc"))
        self.photo = self.photo_ncc > 0.0
        self.photo_window = int(config.exp("photo_window_cells"))
        self.photo_texture = float(config.exp("photo_min_texture"))
        self._photo_counter: Optional[torch.Tensor] = None      # int64 [5] where the kernels run: points per status, added to
        self.nbr_images = self.colour or self.gain or self.photo   # the neighbours' match-size images travel with the reference's
        # far-field shell (lfd_far_accumulate): once per launch on the stream that holds the batch, beside the point stages
        self.far_mode = str(config.exp("far_shell"))
        self.far = self.far_mode != "off"
        self.far_thresh_px = float(config.far_threshold())
        self.far_certainty = float(config.exp("far_certainty"))
        self.far_min_views = int(config.exp("far_min_views"))
        self.far_cells = int(config.exp("far_shell_cells"))
        self._far_table: Optional[torch.Tensor] = None          # the run's table, int64 (6 S S, 7) where the kernels run
        self._far_parts: list = []                              # (far cells per reference, reference uids, overlap or None) per launch the run used
        # epipolar audit (lfd_epipolar_audit): once per launch on the stream that holds the batch, where the far shell's launch is
        self.audit = str(config.exp("epipolar_audit")) != "off"
        self.audit_certainty = float(config.exp("audit_certainty"))
        self.audit_maps = self.audit and str(config.exp("audit_maps_dir")) != ""
        self._audit_parts: list = []                            # (table, (reference uid, neighbour uid) or None per row, cell map or None, reference uids, (H, W)) per launch the run used
        # pose refinement (lfd_pose_accumulate): once per launch beside the audit's, with the audit's pending / commit rule
        self.pose = str(config.exp("pose_refine")) != "off"
        self.pose_certainty = float(config.exp("pose_certainty"))
        self.pose_inlier_px = float(config.exp("pose_inlier_px"))
        self._pose_parts: list = []                             # (table, (reference uid, neighbour uid) or None per row) per launch the run used
        self._uids = [int(c.uid) for c in cams]
        self._gain_parts: list = []                             # (table where the kernels run, reference uids, neighbour uids) per launch the run used
        on = bool(config.exp("undistort_images"))
        self._distortion = [c.active_distortion() if on else None for c in cams]

    # -- forward-backward consistency filter (lfd_cycle_gate) -------------------------------------------------------------------
    def cycle_gate(self, warps, certs, backs, axes) -> None:
        """The certainty planes of one reference's pairs gated IN PLACE, one launch per 16 pairs on the densifier's stream - the stream the
        matcher left them on - with nothing read back: the counters stay where the kernels run until ``cycle_totals``."""
        if self._cycle_counter is None:
            self._cycle_counter = torch.zeros(hb.LFD_MAX_SLOTS, dtype=torch.int32, device=self.dev)
        hw = int(certs[0].numel())
        if self._cycle_pending + hw > 0x7fffffff:
            self._cycle_flush()
        with self.clock.stage("kernel", sync=False):
            for j0 in range(0, len(certs), hb.LFD_MAX_SLOTS):
                j1 = min(len(certs), j0 + hb.LFD_MAX_SLOTS)
                self.dens.cycle_gate(certs[j0:j1], warps[j0:j1], backs[j0:j1], self.w_match, self.h_match, float(self.config.certainty_thresh),
                                     self.cycle_thresh_px, axes=axes, inplace=True, rejected=self._cycle_counter)
        self._cycle_pending += hw
        self.cycle_cells += hw * len(certs)

    def _cycle_flush(self) -> None:
        if self._cycle_counter is not None and self._cycle_pending:
            self.cycle_rejected += int(self._cycle_counter.to(torch.int64).sum().item())
            self._cycle_counter.zero_()
            self._cycle_pending = 0

    def cycle_totals(self) -> Tuple[int, int]:
        """(cells gated, cells rejected) of the run so far: the one read of the device counters."""
        self._cycle_flush()
        return self.cycle_cells, self.cycle_rejected

    # -- multi-view support filter (lfd_support_filter) --------------------------------------------------------------------------
    def support_filter_collected(self, batch: hb.PreparedBatch, res: hb.TriangulationOutput) -> hb.TriangulationOutput:
        """A collected result through the filter (the synchronous schedules, the host backend)."""
        far_part = None
        if self.far:
            with self.clock.stage("kernel"):
                far_part = self._far_launch(batch, pending=False)
        if self.audit:
            with self.clock.stage("kernel"):
                self._audit_commit(self._audit_launch(batch))
        if self.pose:
            with self.clock.stage("kernel"):
                self._pose_commit(self._pose_launch(batch))
        if res is None:
            self._far_commit(far_part, None)
            return res
        if self.min_support > 0:
            self._support_void = False
            with self.clock.stage("kernel"):
                out = self.dens.support_filter(batch, res, self.min_support, self.support_thresh_px)
            self._support_count(out)
            res = out
        status = None
        if self.refine:
            with self.clock.stage("kernel"):
                res, status = self._refined(batch, res, self.max_sigma > 0.0)
        if self.max_sigma > 0.0:
            with self.clock.stage("kernel"):
                res = self._sigma_gated(batch, res, status)
            self._support_count(res)
        if self.photo:
            with self.clock.stage("kernel"):
                res = self._photo_gated(batch, res)
        if self.colour:
            with self.clock.stage("kernel"):
                res = self._recoloured(batch, res)
        if self.gain:
            with self.clock.stage("kernel"):
                self._gain_commit(self._gain_launch(batch, res))
        if self.normals:
            with self.clock.stage("kernel"):
                res = self._with_normals(batch, res)
        self._far_commit(far_part, res)
        return res

    # -- far-field shell (lfd_far_accumulate) ------------------------------------------------------------------------------------
    def _far_launch(self, batch: hb.PreparedBatch, pending: bool):
        """One launch of lfd_far_accumulate over ``batch`` on the stream that holds it; nothing is read back here.  ``pending``: into a zeroed
        table of the launch's own, which ``_far_commit`` adds to the run's when the launch's result is one the run uses (``finish_sampled``) and
        drops otherwise - the gain statistics' rule: a grouped call that is void as a whole and redone reference by reference counts once.
        Otherwise straight into the run's table.  Returns (pending table or None, far cells per reference, reference uids, far flags)."""
        if self._far_table is None:
            self._far_table = hb.far_table(self.far_cells, self.dev)
        table = hb.far_table(self.far_cells, self.dev) if pending else self._far_table
        counters = torch.zeros(batch.n_refs, dtype=torch.int64, device=self.dev)
        flags = torch.empty((batch.n_refs, batch.H * batch.W), dtype=torch.uint8, device=self.dev)
        self.dens.far_accumulate(batch, self.far_thresh_px, self.far_certainty, self.far_min_views, self.far_cells, table=table, counters=counters,
                                 flags=flags)
        uids = np.array([self._uids[int(r.ref_cam)] for r in batch.refs], np.int64)
        return (table if pending else None), counters, uids, flags

    def _far_commit(self, part, res) -> None:
        """The launch's statistics join the run's.  ``res``: the launch's collected result (or None): the far cells that also produced one of
        its points are counted where the flags are."""
        if part is None:
            return
        table, counters, uids, flags = part
        if table is not None:
            self._far_table += table
        overlap = None
        if res is not None and getattr(res, "cell", None) is not None and int(res.count) > 0:
            per_ref = torch.from_numpy(np.diff(np.asarray(res.ref_offsets, np.int64))).to(flags.device)
            ref_of = torch.repeat_interleave(torch.arange(per_ref.numel(), device=flags.device), per_ref)
            cell = res.cell.to(flags.device).long()
            ok = (cell >= 0) & (cell < flags.shape[1])
            overlap = flags.reshape(-1)[(ref_of * flags.shape[1] + cell.clamp(0, flags.shape[1] - 1))[ok]].sum()
        self._far_parts.append((counters, uids, overlap))

    def far_result(self) -> dict:
        """The run's far-field statistics: ``table`` (where the kernels run), ``far_cells`` {camera uid: far cells of its references},
        ``overlap`` (far cells that also produced a point of their launch's result)."""
        table = self._far_table if self._far_table is not None else hb.far_table(self.far_cells, self.dev)
        cells: dict = {}
        overlap = 0
        for counters, uids, ov in self._far_parts:
            for uid, n in zip(uids.tolist(), counters.cpu().tolist()):
                cells[int(uid)] = cells.get(int(uid), 0) + int(n)
            overlap += int(ov.item()) if ov is not None else 0
        return dict(table=table, far_cells=cells, overlap=overlap)

    # -- epipolar audit (lfd_epipolar_audit) --------------------------------------------------------------------------------------
    def _audit_launch(self, batch: hb.PreparedBatch):
        """One launch of lfd_epipolar_audit over ``batch`` on the stream that holds it, into a zeroed table of the launch's own (its rows are
        the batch's (reference, slot) pairs); nothing is read back here.  ``_audit_commit`` makes it part of the run - at once where the
        launch's result is the run's, in ``finish_sampled`` for a grouped sampled call (the far shell's rule: a call that is void as a whole
        and redone reference by reference counts once).  With experimental['audit_maps_dir'] the launch also writes the cell map."""
        best = torch.empty((batch.n_refs, batch.H * batch.W), dtype=torch.uint8, device=self.dev) if self.audit_maps else None
        table = self.dens.epipolar_audit(batch, self.audit_certainty, best=best)
        pairs = []
        for r in batch.refs:
            row = [(self._uids[int(r.ref_cam)], self._uids[int(n)]) for n in r.nbr_cams]
            pairs.extend(row + [None] * (batch.k - len(row)))
        return table, pairs, best, [self._uids[int(r.ref_cam)] for r in batch.refs], (batch.H, batch.W)

    def _audit_commit(self, part) -> None:
        if part is not None:
            self._audit_parts.append(part)

    def audit_result(self) -> dict:
        """The run's audit: ``rows`` {(reference uid, neighbour uid): the pair's 66 integers summed over the run} and ``maps`` {reference uid:
        uint8 (H, W) cell map} (None without experimental['audit_maps_dir']).  The one read of the tables."""
        rows: dict = {}
        maps = {} if self.audit_maps else None
        for table, pairs, best, ref_uids, grid in self._audit_parts:
            for pair, row in zip(pairs, table.cpu().tolist()):
                if pair is not None:
                    have = rows.get(pair)
                    rows[pair] = row if have is None else [a + b for a, b in zip(have, row)]
            if maps is not None and best is not None:
                for uid, m in zip(ref_uids, best.cpu().numpy()):
                    maps[int(uid)] = m.reshape(grid)
        return dict(rows=rows, maps=maps)

    # -- pose refinement (lfd_pose_accumulate) ---------------------------------------------------------------------------------------
    def _pose_launch(self, batch: hb.PreparedBatch):
        """One launch of lfd_pose_accumulate over ``batch`` on the stream that holds it, into a zeroed table of the launch's own; nothing is
        read back here.  ``_pose_commit`` makes it part of the run, by the audit's rule."""
        table = self.dens.pose_accumulate(batch, self.pose_certainty, self.pose_inlier_px)
        pairs = []
        for r in batch.refs:
            row = [(self._uids[int(r.ref_cam)], self._uids[int(n)]) for n in r.nbr_cams]
            pairs.extend(row + [None] * (batch.k - len(row)))
        return table, pairs

    def _pose_commit(self, part) -> None:
        if part is not None:
            self._pose_parts.append(part)

    def pose_result(self) -> dict:
        """The run's normal equations: ``rows`` {(reference uid, neighbour uid): the pair's 32 integers summed over the run}.  The one read of
        the tables."""
        rows: dict = {}
        for table, pairs in self._pose_parts:
            for pair, row in zip(pairs, table.cpu().tolist()):
                if pair is not None:
                    have = rows.get(pair)
                    rows[pair] = row if have is None else [a + b for a, b in zip(have, row)]
        return dict(rows=rows)

    # -- per-image exposure gains (lfd_gain_accumulate) -------------------------------------------------------------------------
    def _gain_launch(self, batch: hb.PreparedBatch, out):
        """One launch of lfd_gain_accumulate over the points ``out`` holds NOW (buffers on the stream, or a collected result), behind every
        stage that moves or drops them, into a zeroed table of the launch's own: (table, reference uids, neighbour uids) with a row per
        (reference, slot) of the batch.  Nothing is read back here.  A launch has a table of its own so that a grouped call that is redone,
        or dropped as a whole, leaves no trace: only what ``_gain_commit`` is given reaches the run's statistics - decided per launch where
        its result is collected (``finish_sampled``), never by a flag that outlives the launch."""
        table = self.dens.gain_accumulate(batch, out, self.support_thresh_px)
        ref_uid = np.zeros(batch.n_refs * batch.k, np.int64)
        nbr_uid = np.full(batch.n_refs * batch.k, -1, np.int64)           # (-1: a slot the reference does not use; dropped in gain_rows)
        for i, r in enumerate(batch.refs):
            ref_uid[i * batch.k:(i + 1) * batch.k] = self._uids[int(r.ref_cam)]
            for j, c in enumerate(r.nbr_cams):
                nbr_uid[i * batch.k + j] = self._uids[int(c)]
        return table, ref_uid, nbr_uid

    def _gain_commit(self, part) -> None:
        if part is not None:
            self._gain_parts.append(part)

    def gain_rows(self):
        """The run's statistics as core.gains.GainRows on the host: the tables are concatenated where they are and read with one copy."""
        from .gains import GainRows
        if not self._gain_parts:
            return GainRows.empty()
        table = torch.cat([t for t, _r, _n in self._gain_parts], 0).cpu().numpy().view(np.uint64)
        ref_uid = np.concatenate([r for _t, r, _n in self._gain_parts])
        nbr_uid = np.concatenate([n for _t, _r, n in self._gain_parts])
        live = nbr_uid >= 0
        return GainRows(ref_uid[live], nbr_uid[live], table[live])

    def _recoloured(self, batch: hb.PreparedBatch, out):
        """``out`` (buffers on the stream: in place; or a collected result: a copy) with the colour of every point blended over the views that
        see it: one launch of lfd_colour_multiview on the stream that made the points, behind every stage that moves or drops them.  The
        counters stay where the kernels run until ``colour_totals``; like the re-triangulation's they count every launch issued."""
        if self._colour_counter is None:
            self._colour_counter = torch.zeros(2, dtype=torch.int64, device=self.dev)
        return self.dens.colour_multiview(batch, out, self.support_thresh_px, self.colour_mode, counters=self._colour_counter)

    def colour_totals(self) -> Tuple[int, int]:
        """(points whose colour was blended, the sum of the views blended into them) over the launches of the run: the one read of the counters."""
        if self._colour_counter is None:
            return 0, 0
        return tuple(int(v) for v in self._colour_counter.cpu())

    def _with_normals(self, batch: hb.PreparedBatch, out):
        """``out`` (buffers on the stream, or a collected result) with the normals of the points it holds NOW: one launch of
        lfd_estimate_normals on the stream that made them, behind every stage that moves or drops points and before anything is read back.
        The counters stay where the kernels run until ``normal_totals``; like the re-triangulation's they count every launch issued."""
        if self._normal_counter is None:
            self._normal_counter = torch.zeros(2, dtype=torch.int64, device=self.dev)
        return self.dens.estimate_normals(batch, out, self.normal_radius, self.normal_depth_step, float(self.config.reproj_thresh),
                                          counters=self._normal_counter)

    def normal_totals(self) -> Tuple[int, int]:
        """(points whose normal was fitted, points that got the view vector) over the launches of the run: the one read of the counters."""
        if self._normal_counter is None:
            return 0, 0
        return tuple(int(v) for v in self._normal_counter.cpu())

    def _support_count(self, res: hb.TriangulationOutput) -> None:
        """The run's totals, from the integers a result brings along anyway (no read-back of their own)."""
        if res is None or self._support_void:
            return
        # (what a stage kept is what reached the stage behind it: the depth gate behind the filter, the photo-consistency gate behind both)
        behind = int(res.count if getattr(res, "photo_in", None) is None else res.photo_in)
        if res.support_in is not None:
            self.support_in += int(res.support_in)
            self.support_kept += int(behind if res.sigma_in is None else res.sigma_in)
        if res.sigma_in is not None:
            self.sigma_in += int(res.sigma_in)
            self.sigma_kept += behind

    def sigma_totals(self) -> Tuple[int, int]:
        """(points that reached the depth-uncertainty gate, points it kept) of the run so far."""
        return self.sigma_in, self.sigma_kept

    def _sigma_gated(self, batch: hb.PreparedBatch, out, status, into=None):
        """``out`` (buffers on the stream, or a collected result) through lfd_depth_sigma_filter.  ``status``: the status of the re-triangulation
        that just ran over ``out`` on the same stream, or None: the winning slot alone placed every point."""
        return self.dens.depth_sigma_filter(batch, out, self.max_sigma, iso_sigma_px=self.iso_sigma_px, refine_status=status,
                                            support_thresh_px=self.support_thresh_px if status is not None else 0.0, into=into)

    # -- photo-consistency gate (lfd_photo_gate) ---------------------------------------------------------------------------------
    def _photo_gated(self, batch: hb.PreparedBatch, out, into=None):
        """``out`` (buffers on the stream, or a collected result) through lfd_photo_gate: one call on the stream that made the points.  The five
        counters stay where the kernels run until ``photo_totals``; like the re-triangulation's they count every launch issued."""
        if self._photo_counter is None:
            self._photo_counter = torch.zeros(hb.PHOTO_STATUSES, dtype=torch.int64, device=self.dev)
        return self.dens.photo_gate(batch, out, self.photo_window, self.photo_ncc, self.photo_texture, counters=self._photo_counter, into=into)

    def photo_totals(self) -> Tuple[int, int, int, int, int]:
        """Points per verdict of the photo-consistency gate over the launches of the run - guarded, under half a window, untextured, consistent,
        refuted (the dropped ones): the one read of the counters."""
        if self._photo_counter is None:
            return 0, 0, 0, 0, 0
        return tuple(int(v) for v in self._photo_counter.cpu())

    def support_totals(self) -> Tuple[int, int]:
        """(points that reached the filter, points it dropped) of the run so far."""
        return self.support_in, self.support_in - self.support_kept

    def _filtered(self, batch: hb.PreparedBatch, out: hb.OutputBuffers) -> hb.OutputBuffers:
        """``out`` as the launch left it, or - with the filter on - the buffers the filter compacts it into: one launch behind the one that
        filled ``out``, on the same stream, before anything is read back (``out`` goes back to the pool: whatever uses it next follows in the
        same stream).  Destination buffers are recycled among themselves: ``collect`` reports the points that went in only for them."""
        if self.min_support > 0:
            self._support_void = False             # (a new launch: whatever a failed grouped call left behind has been dealt with)
            into = self._take_buffers(out.capacity, out._n_refs, out._k, filtered=True)
            try:
                self.dens.support_filter(batch, out, self.min_support, self.support_thresh_px, into=into)
            finally:
                self._buf_pool.setdefault((out.capacity, out._n_refs, out._k, False), []).append(out)
            out = into
        status = None
        if self.refine:
            out, status = self._refined(batch, out, self.max_sigma > 0.0)
        if self.max_sigma > 0.0:
            into = self._take_buffers(out.capacity, out._n_refs, out._k, filtered=_pool_kind(out) | 2)
            try:
                self._sigma_gated(batch, out, status, into=into)
            finally:
                self._buf_pool.setdefault((out.capacity, out._n_refs, out._k, _pool_kind(out)), []).append(out)
            out = into
        if self.photo:
            into = self._take_buffers(out.capacity, out._n_refs, out._k, filtered=_pool_kind(out) | 4)  # (the source's counts travel along)
            try:
                self._photo_gated(batch, out, into=into)
            finally:
                self._buf_pool.setdefault((out.capacity, out._n_refs, out._k, _pool_kind(out)), []).append(out)
            out = into
        if self.colour:
            out = self._recoloured(batch, out)
        if self.gain:
            out.gain_pending = self._gain_launch(batch, out)       # (committed in finish_sampled, when the result is one the run uses)
        if self.normals:
            out = self._with_normals(batch, out)
        if self.far:
            out.far_pending = self._far_launch(batch, pending=True)    # (committed in finish_sampled, like the gain statistics)
        if self.audit:
            out.audit_pending = self._audit_launch(batch)              # (likewise)
        if self.pose:
            out.pose_pending = self._pose_launch(batch)                # (likewise)
        return out

    # -- multi-view re-triangulation of supported points (lfd_refine_multiview) ---------------------------------------------------
    def _refined(self, batch: hb.PreparedBatch, out, with_status: bool = False):
        """The points of ``out`` (buffers a launch or the support filter just filled: in place; or a collected result: a copy) through
        lfd_refine_multiview - or, with experimental['precision_weighted_refine'], lfd_refine_multiview_weighted on the batch's precision
        planes: one launch on the stream that made them, before anything reads them.  The counters stay where the kernels run until
        ``refine_totals``; they count every launch issued (a grouped call that is redone is counted twice).  Returns (result, status): the
        per-point status tensor, where the kernels run, when ``with_status`` (the depth-uncertainty gate behind it reads it), else None."""
        if self._refine_counter is None:
            self._refine_counter = torch.zeros(3 if self.refine_weighted else 2, dtype=torch.int64, device=self.dev)
        kw = {"precision": True} if self.refine_weighted else {}
        if with_status:
            return self.dens.refine_multiview(batch, out, self.support_thresh_px, float(self.config.reproj_thresh), with_status=True,
                                              counters=self._refine_counter, **kw)
        return self.dens.refine_multiview(batch, out, self.support_thresh_px, float(self.config.reproj_thresh), counters=self._refine_counter, **kw), None

    def refine_totals(self) -> Tuple[int, ...]:
        """(points refined, points other views confirmed that kept their two-view position[, points solved with weighted rows]) of the run:
        the one read of the device counters."""
        if self._refine_counter is None:
            return (0, 0, 0) if self.refine_weighted else (0, 0)
        return tuple(int(v) for v in self._refine_counter.cpu())

    def close(self) -> None:
        self._prepared.clear()
        self._prepared_bytes = 0
        if self._own:
            self.dens.close()

    def stage_decoded(self, cam_index: int, size_wh: Tuple[int, int], img, mask_l):
        """Called on a PACK thread with a freshly decoded view (device_image_prep): unless the camera's prepared tensors are already on the device,
        the decoded bytes start their way there now - a 3-4 MB pageable copy per image that would otherwise sit on the driver's thread between
        two matcher calls.  (Two packages that need the same new camera at the same moment both upload it: harmless.)"""
        if (int(cam_index), int(size_wh[0]), int(size_wh[1]), mask_l is not None) in self._prepared:
            return img, mask_l
        with self.clock.stage("prepare", sync=False):
            return _upload_u8(img, self.dev), (_upload_u8(mask_l, self.dev) if mask_l is not None else None)

    def prepare_on_device(self, packed: PackedReference, size_wh: Tuple[int, int], need_host: bool) -> PackedReference:
        """device_image_prep: the decoded arrays of ``packed`` are uploaded and resized / thresholded / blacked out by
        lfd_prepare_mask + lfd_prepare_image (Pillow's arithmetic, bit for bit); the result replaces the host-prepared arrays
        (``need_host``: also as NumPy copies, for a matcher that wants PIL images or for debug previews)."""
        dev = self.dev

        def up(a):
            return a if isinstance(a, torch.Tensor) else _upload_u8(a, dev)          # (a pack thread may have uploaded it already: stage_decoded)

        def one(cam_index, img, mask_l):
            # A camera is prepared the same way whether it is the reference or a neighbour, and it appears in ~k + 1 packages of a
            # run: the prepared match-size tensors (0.8 MB + 0.26 MB at 512^2) stay on the device, least recently used first out
            # beyond PREPARED_CACHE_BYTES - upstream keeps its resized images the same way (core/image_utils.py lru caches) - so a
            # decoded full-resolution image (36-72 MB at 12-24 MP) is uploaded and resized once per run, not once per appearance.
            key = (int(cam_index), int(size_wh[0]), int(size_wh[1]), mask_l is not None)
            hit = self._prepared.get(key)
            if hit is not None:
                self._prepared.move_to_end(key)
                return hit
            dist = self._distortion[int(cam_index)]
            if dist is None:
                m01 = self.dens.prepare_mask(up(mask_l), size_wh) if mask_l is not None else None
                entry = (self.dens.prepare_image(up(img), size_wh, m01), m01)
            else:
                entry = undistorted(up(img), up(mask_l) if mask_l is not None else None, dist)
                m01 = entry[1]
            nbytes = entry[0].numel() + (m01.numel() if m01 is not None else 0)
            if nbytes <= PREPARED_CACHE_BYTES:
                self._prepared[key] = entry
                self._prepared_bytes += nbytes
                while self._prepared_bytes > PREPARED_CACHE_BYTES:
                    _k, old = self._prepared.popitem(last=False)
                    self._prepared_bytes -= old[0].numel() + (old[1].numel() if old[1] is not None else 0)
            return entry

        def undistorted(img_t, mask_t, dist):
            # lfd_undistort_image into the context's full-resolution workspaces, in front of the two preparation kernels, all in stream order.
            # The one read-back - the number of pixels the photograph does not cover - decides whether the camera gets a mask of its own: with
            # ordinary barrel distortion there is none, and the dense kernel keeps its no-mask fast path.
            pin, valid, n_invalid = self.dens.undistort_image(img_t, dist, with_valid=True, count=True, workspace="image")
            m01 = None
            if mask_t is not None:
                m01 = self.dens.prepare_mask(self.dens.undistort_image(mask_t, dist, nearest=True, workspace="mask")[0], size_wh)
            if n_invalid:
                v01 = self.dens.prepare_mask(valid, size_wh)
                if m01 is None:
                    m01 = v01
                else:
                    with torch.cuda.stream(self.dens.stream):
                        m01 &= v01
            return self.dens.prepare_image(pin, size_wh, m01), m01

        with self.clock.stage("prepare"):
            img_a, mask_a = one(packed.ref_index, packed.image, packed.mask_a)
            nbrs = [one(ci, im, mk) for ci, im, mk in zip(packed.nbr_indices, packed.nbr_images, packed.nbr_masks)]
        out = dataclasses.replace(packed, raw=False, dev={"image": img_a, "mask_a": mask_a, "nbr_images": [n[0] for n in nbrs],
                                                          "nbr_masks": [n[1] for n in nbrs]})
        if need_host:
            out.image = img_a.cpu().numpy()
            out.mask_a = mask_a.cpu().numpy() if mask_a is not None else None
            out.nbr_images = [n[0].cpu().numpy() for n in nbrs]
            out.nbr_masks = [n[1].cpu().numpy() if n[1] is not None else None for n in nbrs]
        else:
            out.mask_a = True if mask_a is not None else None           # only "is there a mask" is asked of these below
            out.nbr_masks = [True if n[1] is not None else None for n in nbrs]
        return out

    def inputs(self, packed: PackedReference, warps, certs, precision=None) -> hb.ReferenceInputs:
        """``precision``: the matcher's precision planes of the pairs (experimental['precision_weighted_refine'], the depth-uncertainty gate
        without experimental['match_sigma_px']), or None."""
        dev = self.dev
        if packed.dev is not None:                 # prepared on the device: nothing to upload
            d = packed.dev
            use_masks = d["mask_a"] is not None or any(m is not None for m in d["nbr_masks"])
            return hb.ReferenceInputs(ref_cam=packed.ref_index, nbr_cams=list(packed.nbr_indices), cert=certs, warp=warps,
                                      image=d["image"], mask_a=d["mask_a"], mask_b=list(d["nbr_masks"]) if use_masks else None,
                                      precision=precision, nbr_images=list(d["nbr_images"]) if self.nbr_images else None)
        use_masks = packed.mask_a is not None or any(m is not None for m in packed.nbr_masks)
        mask_b = None
        with self.clock.stage("prepare"):        # the host-prepared image and masks cross to where the kernels run
            if use_masks:
                mask_b = [_upload_u8(m, dev) if m is not None else None for m in packed.nbr_masks]
            image = _upload_u8(packed.image, dev)
            mask_a = _upload_u8(packed.mask_a, dev) if packed.mask_a is not None else None
            # (multi-view colour: the neighbours' match-size images cross beside the reference's)
            nbr_images = [_upload_u8(im, dev) for im in packed.nbr_images] if self.nbr_images else None
        return hb.ReferenceInputs(ref_cam=packed.ref_index, nbr_cams=list(packed.nbr_indices), cert=certs, warp=warps, image=image,
                                  mask_a=mask_a, mask_b=mask_b, precision=precision, nbr_images=nbr_images)

    def sampled(self, ref: hb.ReferenceInputs, axes, rng, device_seed: Optional[int], need_best: bool = False
                ) -> Tuple[Optional[hb.TriangulationOutput], Optional[torch.Tensor]]:
        """aggregate kernel -> coverage sampling -> indexed kernel.  The sampling stage runs on the
        device (lfd_select_samples consuming the context's MT19937 stream; lfd_select_top_m for
        no_filter) unless the configuration asks for the host stage (core/sampling.py).  With the device
        stage and no debug preview to feed (``need_best``), the three steps are ONE asynchronous call
        (lfd_triangulate_sampled): the selection count never visits the host."""
        batch = hb.PreparedBatch([ref], self.w_match, self.h_match, axes=axes, cameras=self.cams)
        on_device = self.config.selection_backend == "device" and not self.on_host
        fusable = on_device and (not self.config.no_filter or self.config.matches_per_ref <= self.dens.TOP_M_MAX)
        # upstream's own normaliser (torch's f32 sum of the weights, on this host) for the single-stream, filtered selection
        torch_sum = on_device and not self.config.no_filter and device_seed is None and bool(self.config.upstream_normaliser)
        if fusable and not need_best and not torch_sum:
            if device_seed is not None and not self.config.no_filter:
                self.dens.seed_rng(device_seed)
            try:
                with self.clock.stage("kernel"):
                    out = self.dens.triangulate_sampled(batch, self.params, self.config.matches_per_ref, cap=self.sample_cap, border=2, tiles=24)
                out = self.support_filter_collected(batch, out)
                return (out if out.count else None), None
            except hb.SelectionInexact:
                pass         # weights below 2^-29 (certainty_thresh ~ 0): the host stage below, on the device's RNG stream
        with self.clock.stage("select"):
            best, _ = self.dens.aggregate(batch, self.params)
            sel_t = self._select(best, rng, device_seed, on_device, torch_sum)
        if sel_t.numel() == 0:
            return None, best[0]
        with self.clock.stage("kernel"):
            out = self.dens.triangulate_indexed(batch, self.params, sel_t, [0, int(sel_t.numel())])
        out = self.support_filter_collected(batch, out)
        return (out if out.count else None), best[0]

    def _select(self, best: torch.Tensor, rng, device_seed: Optional[int], on_device: bool, torch_sum: bool) -> torch.Tensor:
        """The cells of one reference's aggregated map the sampling stage picks (int64, where the kernels run)."""
        sel_t = None
        if on_device and self.config.no_filter and self.config.matches_per_ref <= self.dens.TOP_M_MAX:
            sel_t = self.dens.select_top_m(best[0], self.config.matches_per_ref, cap=self.sample_cap)
        elif on_device and not self.config.no_filter:
            if device_seed is not None:
                self.dens.seed_rng(device_seed)
            try:
                s_up = upstream_weight_sum(best[0], cap=self.sample_cap, border=2) if torch_sum else 0.0
                # (a sum <= 0 is upstream's "nothing to sample" case, which the device stage reports itself from its exact sum)
                sel_t = self.dens.select_samples(best[0], self.config.matches_per_ref, cap=self.sample_cap, border=2, tiles=24,
                                                 s_override=s_up if s_up > 0.0 else 0.0)
            except hb.SelectionInexact:
                # upstream handles such maps normally (core/sampling.py:27-32): run its host stage on the stream the device
                # holds (the refused call consumed nothing) and hand the advanced stream back
                key, pos = self.dens.rng_state()
                rs = np.random.RandomState()
                rs.set_state(("MT19937", key, pos, 0, 0.0))
                sel = select_samples_with_coverage(best[0], self.config.matches_per_ref, cap=self.sample_cap, border=2,
                                                   tiles=24, no_filter=False, rng=rs)
                st = rs.get_state()
                self.dens.set_rng_state(st[1], int(st[2]))
                sel_t = torch.from_numpy(np.ascontiguousarray(sel, dtype=np.int64)).to(self.dev)
        if sel_t is None:        # host stage by configuration (selection_backend="host", or no_filter beyond the device's top-M limit)
            sel = select_samples_with_coverage(best[0], self.config.matches_per_ref, cap=self.sample_cap, border=2,
                                               tiles=24, no_filter=self.config.no_filter, rng=rng)
            sel_t = torch.from_numpy(np.ascontiguousarray(sel, dtype=np.int64)).to(self.dev)
        return sel_t

    def can_launch_ahead(self, need_best: bool, per_ref_rng: bool, H: int, W: int) -> bool:
        """The fused sampled call of reference i+1 may be launched before reference i is read back when nothing on the host
        depends on i's result: the selection runs on the device, no debug preview wants the aggregated map, and the device
        selection cannot refuse its input (every weight >= 2^-29 or 0, i.e. certainty_thresh >= 2^-29 * H*W*cap; a refused
        call consumes no random numbers and falls back to the host stage, which would then see the stream AFTER i+1's draws) -
        or every reference has its own stream anyway."""
        cfg = self.config
        if self.on_host:
            return False
        if cfg.selection_backend == "device" and not cfg.no_filter and not per_ref_rng and bool(cfg.upstream_normaliser):
            return False         # the normaliser comes from the host: one reference at a time
        fusable = cfg.selection_backend == "device" and (not cfg.no_filter or cfg.matches_per_ref <= self.dens.TOP_M_MAX)
        exact_ok = cfg.no_filter or per_ref_rng or float(cfg.certainty_thresh) >= 2.0 ** -29 * H * W * max(self.sample_cap, 1e-6)
        return fusable and not need_best and exact_ok

    def launch_sampled(self, ref: hb.ReferenceInputs, axes, device_seed: Optional[int], s_override: float = 0.0, batch=None):
        """Enqueue one reference's fused call and the read-back of its counts; returns what ``finish_sampled`` needs."""
        if batch is None:
            batch = hb.PreparedBatch([ref], self.w_match, self.h_match, axes=axes, cameras=self.cams)
        if device_seed is not None and not self.config.no_filter:
            self.dens.seed_rng(device_seed)
        M = self.config.matches_per_ref
        with self.clock.stage("kernel"):
            out = self._take_buffers(int(M) + 24 * 24 + 64, 1, batch.k)
            self.dens.launch_sampled(batch, self.params, M, out, cap=self.sample_cap, border=2, tiles=24, s_override=float(s_override))
            out = self._filtered(batch, out)
            out.begin_collect(self.dens.stream)
        return batch, out

    def _take_buffers(self, capacity: int, n_refs: int, k: int, filtered: int = 0) -> hb.OutputBuffers:
        """Survivor buffers of the fused sampled calls, recycled: a fresh OutputBuffers costs two device allocations and - on its first
        read-back - a pinned host allocation (hipHostMalloc: milliseconds), per reference; ``finish_sampled`` hands a buffer back once the
        reference's survivors have been copied out of it."""
        free = self._buf_pool.setdefault((int(capacity), int(n_refs), int(k), int(filtered)), [])
        out = free.pop() if free else hb.OutputBuffers(int(capacity), int(n_refs), int(k), self.dev)
        out.normals_valid = False              # (whatever fills them next has not had its normals estimated)
        out.gain_pending = None
        out.far_pending = None
        out.audit_pending = None
        out.pose_pending = None
        return out

    # -- upstream's normaliser without stalling the launch stream ---------------------------------------------------------------
    def can_pipeline_normaliser(self, need_best: bool, per_ref_rng: bool, H: int, W: int) -> bool:
        """The default single-stream sampled mode (``upstream_normaliser``): the aggregated map of reference i is copied to the host on
        a SIDE stream while the host is busy with reference i - 1 (its torch sum, its fused launch) and the matcher with reference
        i + 1; the launch stream never waits for the host.  Same preconditions as the launch-ahead (the device selection must not be
        able to refuse its input), plus: one RNG stream, filter mode."""
        cfg = self.config
        if self.on_host or cfg.selection_backend != "device" or cfg.no_filter or per_ref_rng or need_best:
            return False
        if not bool(cfg.upstream_normaliser):
            return False
        return float(cfg.certainty_thresh) >= 2.0 ** -29 * H * W * max(self.sample_cap, 1e-6)

    def _normaliser_slot(self, R: int, H: int, W: int) -> dict:
        """Buffers of a group's weight maps on their way to the host: aggregated map, weights, pinned landing area, two events.  A slot is
        allocated for the run's group size and SLICED for whatever is smaller (a last short group, a single reference between groups): a run
        allocates two of them - hipHostMalloc of tens of MB costs milliseconds - and a slot of another grid is dropped, not kept."""
        for i, cand in enumerate(self._norm_free):
            if cand["grid"] == (H, W) and cand["cap"] >= R:
                slot = self._norm_free.pop(i)
                break
        else:
            self._norm_free.clear()            # a stale grid's - or too small - slots go back to the driver
            cap = self._norm_group = max(int(R), self._norm_group if self._norm_grid == (H, W) else 1)       # the largest group this grid has seen
            self._norm_grid = (H, W)
            slot = {"grid": (H, W), "cap": cap,
                    "best": torch.empty((cap, H, W), dtype=torch.float32, device=self.dev), "w": torch.empty((cap, H, W), dtype=torch.float32, device=self.dev),
                    "host": torch.empty((cap, H, W), dtype=torch.float32).pin_memory(), "agg_done": torch.cuda.Event(), "copied": torch.cuda.Event()}
        slot["n"] = int(R)
        return slot

    def _border_mask(self, H: int, W: int) -> torch.Tensor:
        mask = self._norm_masks.get((H, W))
        if mask is None:
            ys = torch.arange(H, device=self.dev).view(H, 1)
            xs = torch.arange(W, device=self.dev).view(1, W)
            mask = ((xs >= 2) & (xs <= W - 1 - 2) & (ys >= 2) & (ys <= H - 1 - 2)).to(torch.float32)          # border = 2 (core/pipeline.py:642-649 upstream)
            self._norm_masks = {(H, W): mask}
        return mask

    def _start_normalisers(self, batch: hb.PreparedBatch, slot: dict) -> None:
        """Aggregate on the launch stream; the capped, border-masked WEIGHTS (upstream's ``clamp(max=cap) * inside.float()``: exactly rounded
        element by element, so the device gives the host's values) right behind it; then the weight maps to pinned host memory on the side
        stream, an event behind them.  What is left for the host is upstream's one library-dependent step: torch's f32 ``sum``."""
        if self._norm_side is None:
            self._norm_side = torch.cuda.Stream(device=self.dev)
        n = slot["n"]
        best, w, host = slot["best"][:n], slot["w"][:n], slot["host"][:n]
        self.dens.launch_aggregate(batch, self.params, best, None)
        with torch.cuda.stream(self.dens.stream):
            torch.clamp(best, max=self.sample_cap, out=w)
            w.mul_(self._border_mask(batch.H, batch.W))
            slot["agg_done"].record(self.dens.stream)
        with torch.cuda.stream(self._norm_side):
            self._norm_side.wait_event(slot["agg_done"])
            host.copy_(w, non_blocking=True)
            slot["copied"].record(self._norm_side)

    def begin_normaliser(self, ref: hb.ReferenceInputs, axes):
        """One reference's weight map on its way to the host (``_start_normalisers``); returns what ``finish_normaliser`` needs."""
        batch = hb.PreparedBatch([ref], self.w_match, self.h_match, axes=axes, cameras=self.cams)
        slot = self._normaliser_slot(1, batch.H, batch.W)
        with self.clock.stage("select", sync=False):
            self._start_normalisers(batch, slot)
        return batch, slot

    def finish_normaliser(self, handle) -> float:
        """upstream's torch f32 sum (core/sampling.py:27 there) of the weight map that has arrived; the slot goes back to the pool"""
        _batch, slot = handle
        return self.finish_chain_normalisers(slot)[0]

    def launch_sampled_multi(self, refs: List[hb.ReferenceInputs], axes, seeds: List[int]):
        """``refs_per_launch`` references through ONE fused call, each on its own stream (per_reference_rng)."""
        batch = hb.PreparedBatch(refs, self.w_match, self.h_match, axes=axes, cameras=self.cams)
        M = self.config.matches_per_ref
        with self.clock.stage("kernel"):
            out = self._take_buffers(len(refs) * (int(M) + 24 * 24 + 64), len(refs), batch.k)
            self.dens.launch_sampled_multi(batch, self.params, M, out, seeds, cap=self.sample_cap, border=2, tiles=24)
            out = self._filtered(batch, out)
            out.begin_collect(self.dens.stream)
        return batch, out

    # -- several references per fused call on upstream's ONE stream ------------------------------------------------------------------
    def can_chain(self, need_best: bool, H: int, W: int) -> bool:
        """``refs_per_launch`` references of the single-stream sampled mode may share one fused call (lfd_triangulate_sampled_chain: they draw one
        after the other from the context's MT19937 stream, everything else runs side by side) under the launch-ahead's preconditions: device
        selection that cannot refuse its input for inexactness, no debug preview that wants the aggregated map."""
        cfg = self.config
        if self.on_host or cfg.selection_backend != "device" or need_best:
            return False
        if cfg.no_filter:
            return cfg.matches_per_ref <= self.dens.TOP_M_MAX
        return float(cfg.certainty_thresh) >= 2.0 ** -29 * H * W * max(self.sample_cap, 1e-6)

    def chain_uses_upstream_normaliser(self) -> bool:
        return bool(self.config.upstream_normaliser) and not self.config.no_filter

    def prepare_chain(self, refs: List[hb.ReferenceInputs], axes) -> hb.PreparedBatch:
        """(separate from the launch: a reference that cannot be batched fails HERE, before anything has drawn from the stream)"""
        return hb.PreparedBatch(refs, self.w_match, self.h_match, axes=axes, cameras=self.cams)

    def begin_chain_normalisers(self, batch: hb.PreparedBatch):
        """``begin_normaliser`` for a whole group: ONE aggregate launch, the capped, border-masked weights of all its references in one pass, one
        copy to pinned host memory on the side stream.  The caller launches the group BEFORE this one next (its sums have long arrived), so that
        the copy and torch's sums of this group hide under that group's kernels."""
        slot = self._normaliser_slot(batch.n_refs, batch.H, batch.W)
        with self.clock.stage("select", sync=False):
            self._start_normalisers(batch, slot)
        return slot

    def finish_chain_normalisers(self, slot) -> List[float]:
        """upstream's torch f32 sum (core/sampling.py:27 there) of every reference's weight map, each over its own contiguous (H, W) block"""
        try:
            with self.clock.stage("select", sync=False):
                slot["copied"].synchronize()
                sums = [float(slot["host"][r].reshape(-1).sum()) for r in range(slot["n"])]
        finally:
            self._norm_free.append(slot)
        # (a sum <= 0 is upstream's "nothing to sample" case, which the device stage reports itself from its exact sum)
        return [v if v > 0.0 else 0.0 for v in sums]

    def checkpoint_rng(self, place: int) -> None:
        """The device's random stream put aside in stream order, before a fused call of several references (core/strategies.py::SampledLoop)."""
        self.dens.checkpoint_rng(place)

    def rollback_rng(self, place: int) -> None:
        self._support_void = False             # (the failed grouped call and what was launched behind it have been collected and dropped)
        self.dens.rollback_rng(place)

    def launch_sampled_chain(self, batch: hb.PreparedBatch, s_overrides: Optional[List[float]]):
        M = self.config.matches_per_ref
        with self.clock.stage("kernel"):
            out = self._take_buffers(batch.n_refs * (int(M) + 24 * 24 + 64), batch.n_refs, batch.k)
            self.dens.launch_sampled_chain(batch, self.params, M, out, s_overrides=s_overrides, cap=self.sample_cap, border=2, tiles=24)
            out = self._filtered(batch, out)
            out.begin_collect(self.dens.stream)
        return batch, out

    def finish_sampled(self, handle, check_selection: bool = True) -> Optional[hb.TriangulationOutput]:
        """Wait for the reference's counts, copy its survivors out of the (recycled) buffers: the result owns trimmed tensors.
        ``check_selection=False``: the caller reads ``sel_status`` reference by reference (a chained group: a refused reference is that
        reference's error, not the group's)."""
        _batch, out = handle
        try:
            try:
                with self.clock.stage("d2h"):          # the counts: whatever the device still had to do for this reference shows here
                    res = out.collect(indexed=True, check_selection=check_selection)
                if res.launch_status != 0:
                    self.dens.check_launches()
            except Exception:
                self._support_void = True              # (the caller redoes the call, and drops what was launched behind it)
                raise
            void = not check_selection and any(int(st) in hb.SELECT_VOIDS_STREAM for st in res.sel_status)
            if void:
                self._support_void = True              # (a chained call that is void as a whole: core/strategies.py::SampledLoop._recover)
            self._support_count(res)
            # the gain statistics of THIS call follow its points: kept unless the call is void as a whole (the caller redoes its references);
            # an exception above keeps nothing, and a caller that drops the result clears ``gain_pending`` first (SampledLoop._recover)
            if not void:
                self._gain_commit(getattr(out, "gain_pending", None))
                self._far_commit(getattr(out, "far_pending", None), res)
                self._audit_commit(getattr(out, "audit_pending", None))
                self._pose_commit(getattr(out, "pose_pending", None))
            if not res.count and check_selection:
                return None
            return dataclasses.replace(res, xyz=res.xyz.clone(), rgb=res.rgb.clone(), err=res.err.clone(),
                                       cell=res.cell.clone() if res.cell is not None else None,
                                       slot=res.slot.clone() if res.slot is not None else None, _packed=None,
                                       normals=res.normals.clone() if res.normals is not None else None)
        finally:
            out.gain_pending = None
            out.far_pending = None
            out.audit_pending = None
            out.pose_pending = None
            self._buf_pool.setdefault((out.capacity, out._n_refs, out._k, _pool_kind(out)), []).append(out)

    def pack_ply_tensor(self, xyz: torch.Tensor, rgb: torch.Tensor) -> torch.Tensor:
        """The same records as a uint8 tensor that stays where the points are (what a sharded run sends to the writer rank)."""
        if self.on_host:
            return torch.from_numpy(ply_records(xyz.numpy(), to_uint8_rgb(rgb.numpy())).view(np.uint8).reshape(-1).copy())
        return self.dens.pack_ply(xyz, rgb)

    def pack_ply_bytes(self, xyz: torch.Tensor, rgb: torch.Tensor) -> bytes:
        """The survivors' 15-byte PLY records, quantised and packed on the device (only file payload crosses PCIe)."""
        if self.on_host:
            return ply_records(xyz.numpy(), to_uint8_rgb(rgb.numpy())).tobytes()
        with self.clock.stage("d2h"):
            return self.dens.pack_ply(xyz, rgb).cpu().numpy().tobytes()

    def dense(self, refs: List[hb.ReferenceInputs], axes) -> hb.TriangulationOutput:
        batch = hb.PreparedBatch(refs, self.w_match, self.h_match, axes=axes, cameras=self.cams)
        with self.clock.stage("kernel"):
            if bool(self.config.exp("dense_tile_segments")):
                # unordered retirement (no look-back), raster order restored from the tile table: the same result, bit for bit
                return self.dens.order_segments(self.dens.triangulate_dense_segments(batch, self.params))
            if (self.min_support > 0 or self.refine or self.max_sigma > 0.0 or self.photo or self.colour or self.gain or self.normals) and not self.on_host:
                # the launch, the filter, the re-triangulation and / or the gate behind it on the same stream, then the one read-back of the offsets
                cap = batch.n_refs * batch.H * batch.W
                out = hb.OutputBuffers(cap, batch.n_refs, batch.k, self.dev)
                self.dens.launch_dense(batch, self.params, out)
                if self.min_support > 0:
                    out = self.dens.support_filter(batch, out, self.min_support, self.support_thresh_px)
                status = None
                if self.refine:
                    out, status = self._refined(batch, out, self.max_sigma > 0.0)
                if self.max_sigma > 0.0:
                    out = self._sigma_gated(batch, out, status)
                if self.photo:
                    out = self._photo_gated(batch, out)
                if self.colour:
                    out = self._recoloured(batch, out)
                if self.gain:
                    self._gain_commit(self._gain_launch(batch, out))
                if self.normals:
                    out = self._with_normals(batch, out)
                far_part = self._far_launch(batch, pending=False) if self.far else None
                if self.audit:
                    self._audit_commit(self._audit_launch(batch))
                if self.pose:
                    self._pose_commit(self._pose_launch(batch))
                self.dens.check_launches()
                res = out.collect()
                self._support_void = False
                self._support_count(res)
                self._far_commit(far_part, res)
                return res
            res = self.dens.triangulate_dense(batch, self.params)
        return self.support_filter_collected(batch, res)

    def launch_dense_ply(self, refs: List[hb.ReferenceInputs], axes, records: torch.Tensor, ref_offsets: torch.Tensor,
                         table: Optional[torch.Tensor] = None) -> hb.PreparedBatch:
        """The dense kernel writing the 15-byte PLY records itself (lfd_triangulate_dense_ply), asynchronously, into the caller's buffers
        (the streamed output of a dense run: core/strategies.py::DensePlyStreamer).  ``table``: the form without the look-back
        (lfd_triangulate_dense_ply_segments) - ``ref_offsets[:n]`` then receives the references' COUNTS and reference r's records start at
        byte 15 * r * H * W.  Returns the batch, which keeps the inputs alive."""
        batch = hb.PreparedBatch(refs, self.w_match, self.h_match, axes=axes, cameras=self.cams)
        with self.clock.stage("kernel"):
            if table is not None:
                self.dens.launch_dense_ply_segments(batch, self.params, records, ref_offsets, table)
            else:
                self.dens.launch_dense_ply(batch, self.params, records, ref_offsets)
        return batch

    def debug_matches(self, ref: hb.ReferenceInputs, out_cell: torch.Tensor, out_slot: torch.Tensor, axes,
                      best_cert: Optional[torch.Tensor]):
        """Per neighbour slot: clipped [xA,yA,xB,yB] in match pixels + certainty/cap of the survivors
        (upstream core/pipeline.py:761-769), gathered on the GPU from the maps the kernel consumed."""
        res = {}
        H, W = ref.cert[0].shape
        wm1, hm1 = float(self.w_match - 1), float(self.h_match - 1)
        cells = out_cell.long()
        for j in range(len(ref.cert)):
            sel = cells[out_slot == j]
            if sel.numel() == 0:
                continue
            wp = ref.warp[j].reshape(H * W, -1)[sel]
            if wp.shape[1] == 4:
                xan, yan, xbn, ybn = wp[:, 0], wp[:, 1], wp[:, 2], wp[:, 3]
            else:
                ax, ay = axes if axes is not None else (torch.from_numpy(hb.identity_axis(W)).to(self.dev),
                                                        torch.from_numpy(hb.identity_axis(H)).to(self.dev))
                xan, yan, xbn, ybn = ax[sel % W], ay[sel // W], wp[:, 0], wp[:, 1]
            m = torch.stack([((xan + 1.0) * 0.5 * wm1).clamp(0.0, wm1), ((yan + 1.0) * 0.5 * hm1).clamp(0.0, hm1),
                             ((xbn + 1.0) * 0.5 * wm1).clamp(0.0, wm1), ((ybn + 1.0) * 0.5 * hm1).clamp(0.0, hm1)], dim=1)
            denom = self.sample_cap if self.sample_cap > 1e-6 else 1.0
            if best_cert is not None:
                # gathered on the device, divided on the host with NumPy like upstream (core/pipeline.py:766-768): the GPU's f32
                # division may differ from IEEE by an ulp, and these few thousand values are a preview, not a hot path
                cn = np.clip(best_cert.reshape(-1)[sel].cpu().numpy() / denom, 0.0, 1.0).astype(np.float32)
            else:
                cn = np.ones(int(sel.numel()), np.float32)
            res[j] = (m.cpu().numpy().astype(np.float32), cn)
        return res

