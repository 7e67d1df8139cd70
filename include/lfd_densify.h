/*
 * lfd_densify.h -- C ABI of the MI355X-native dense-initialisation hot path.
 *
 * The upstream plugin (shadygm/Lichtfeld-Densification-Plugin) has no FFI: its boundary is a set of
 * Python call signatures inside one interpreter.  This header is the C-ABI a maintainer would bind
 * (ctypes / cffi / pybind) to replace, per reference view, the CPU stage
 *
 *     core/pipeline.py:405-442   _collect_reference_matches epilogue (certainty floor, masks, D2H)
 *     core/pipeline.py:602-780   _triangulate_ref
 *     core/geometry.py:53-141    skew / DLT / reprojection / cheirality / parallax / F / Sampson
 *     core/sampling.py:8-53      select_samples_with_coverage        (lfd_select_*: see below)
 *     core/writers.py:15-46      write_ply / write_points3D_bin      (lfd_pack_*)
 *
 * with hand-written HIP kernels for gfx950.  All tensor arguments are raw DEVICE pointers unless the
 * comment says "host"; nothing here depends on torch.  Every function returns LFD_OK (0) or an
 * error code and records a message retrievable with lfd_last_error(); nothing aborts.  A context is
 * bound to one HIP device and one stream; use one context per thread (no hidden globals).
 *
 * Every entry point that computes needs a GPU and fails with LFD_ERR_HIP when none is present; nothing falls back to
 * the host.  The CPU twin at the end of this header (lfd_create_host + the *_host entry points: the host build of
 * the same per-cell source over host arrays) is a separate, explicitly chosen interface for upstream's CPU-only
 * configuration, for timing a CPU baseline and for parity checks.
 */
#ifndef LFD_DENSIFY_H
#define LFD_DENSIFY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LFD_ABI_VERSION 9
#define LFD_MAX_SLOTS 16 /* neighbours per reference handled by one launch */

enum lfd_status {
    LFD_OK = 0,
    LFD_ERR_INVALID = 1,  /* bad argument */
    LFD_ERR_HIP = 2,      /* HIP runtime error / no device */
    LFD_ERR_CAPACITY = 3, /* output buffers too small (counts are still valid) */
    LFD_ERR_STATE = 4     /* call order (e.g. cameras not uploaded) */
};

typedef struct lfd_context lfd_context;

/* Thresholds of DensePipelineConfig that reach the kernels (core/config.py:7-26).  Comparison
 * dtypes follow upstream: Sampson f64 `<`, reprojection f32 `<=`, depth f32 `> 0`, parallax f32 `>=`. */
typedef struct lfd_params {
    double sampson_thresh;  /* px^2; <= 0 disables the Sampson gate (core/pipeline.py:708)          */
    float certainty_thresh; /* FLOOR applied to certainty, not a reject (core/pipeline.py:407)       */
    float sample_cap;       /* RomaMatcher.sample_thresh = 0.9 (core/matcher.py:92)                  */
    float reproj_thresh;    /* px (core/pipeline.py:745)                                             */
    float min_parallax_deg; /* degrees; <= 0 disables (core/pipeline.py:748)                         */
    int32_t no_filter;      /* keep every finite point (core/pipeline.py:739-743)                    */
    int32_t flags;          /* LFD_FLAG_* below, 0 = defaults                                        */
} lfd_params;

/* lfd_triangulate_dense blends the four colour taps in f32 by default (same taps, weights and order as upstream
 * core/pipeline.py:661-679, within 2.5e-7 of upstream's f64 blend).  With this flag it runs upstream's f64
 * arithmetic: rgb is then bit-identical to upstream's, at ~6 % more kernel time.  The upstream-equivalent entry
 * points (lfd_triangulate_indexed / _sampled) always use the f64 form. */
#define LFD_FLAG_EXACT_COLOUR 1

/* One launch = n_refs reference views, each with up to k neighbour slots (slots [0, n_slots[r]) are
 * valid, in the order upstream's `nn_ids` lists the loaded neighbours).  Arrays marked "host" are
 * host arrays whose ELEMENTS are device pointers. */
typedef struct lfd_batch {
    int32_t n_refs;
    int32_t k;                    /* slot stride of the per-slot arrays, 1..LFD_MAX_SLOTS            */
    int32_t H, W;                 /* RoMa output grid                                                */
    int32_t w_match, h_match;     /* matcher.w_resized / h_resized (pixel conversion, image, masks)  */
    int32_t warp_channels;        /* 4: [xA,yA,xB,yB] as upstream's matcher emits; 2: [xB,yB] only   */
    int32_t reserved;
    const int32_t* ref_cam;       /* host [n_refs]      index into the uploaded camera table         */
    const int32_t* n_slots;       /* host [n_refs]      valid slots of each reference (<= k)         */
    const int32_t* nbr_cam;       /* host [n_refs*k]    camera index of every slot                   */
    const float* const* cert;     /* host [n_refs*k] -> device f32 [H*W]   raw certainty (pre-floor) */
    const float* const* warp;     /* host [n_refs*k] -> device f32 [H*W*warp_channels], normalised   */
    const uint8_t* const* image;  /* host [n_refs]   -> device u8 [h_match*w_match*3] (RGB, resized) */
    const uint8_t* const* mask_a; /* NULL, or host [n_refs]   -> device u8 {0,1} [h_match*w_match] or NULL */
    const uint8_t* const* mask_b; /* NULL, or host [n_refs*k] -> device u8 {0,1} [h_match*w_match] or NULL */
    const float* axis_x;          /* device f32 [W]: A-grid x of column j (torch.linspace(-1+1/W,1-1/W,W)); */
    const float* axis_y;          /* device f32 [H]; both NULL -> lfd_identity_axis() values. Used when warp_channels==2 */
    const float* fundamental;     /* NULL, or host f32 [n_refs*k*9]: F of every (reference, slot) pair as upstream's
                                   * fundamental_from_world2cam returns it (core/geometry.py:122-130, row-major), used instead of
                                   * the F the library derives from the camera table.  The library's own F is built with the
                                   * closed-form inverse of K (exactly 1/fx, -cx/fx ...) where upstream calls np.linalg.inv
                                   * (LAPACK sgetrf/sgetri); the two agree to ~2e-6 relative, not bit for bit, which moves a
                                   * Sampson value next to the threshold by ~1e-5.  A caller that already holds upstream's F
                                   * (integration path B in INTEGRATION.md) passes it here and gets upstream's Sampson decisions. */
} lfd_batch;

/* Survivors.  Capacity is in points.  cell / slot are optional (NULL to skip). */
typedef struct lfd_points {
    float* xyz;     /* [capacity*3]                                                                  */
    float* rgb;     /* [capacity*3]  f32 in [0,1] (quantised only by the writers, as upstream)       */
    float* err;     /* [capacity]    max reprojection error of the two views, px                     */
    int32_t* cell;  /* [capacity]    flat grid index y*W+x                                            */
    uint8_t* slot;  /* [capacity]    neighbour slot that won the arg-max                              */
    int64_t capacity;
} lfd_points;

/* ---- lifecycle ------------------------------------------------------------------------------ */
int lfd_abi_version(void);
int lfd_create(int device_index, void* hip_stream, lfd_context** out);
void lfd_destroy(lfd_context* ctx);
int lfd_set_stream(lfd_context* ctx, void* hip_stream);
/* The profiling / A-B switches of the environment (LFD_DENSE_EXTRA_LDS, LFD_DENSE_GENERIC, LFD_INDEXED_SPLIT, LFD_SELECT_WORKGROUPS, LFD_SELECT_TIMING,
 * LFD_DENSE_TIMING) are read when a context is created, never on a launch path; a test or profiling script that changes them for a
 * live context calls this to have them read again. */
int lfd_reload_env(lfd_context* ctx);
/* Measurement: the device-side duration of the dense kernel's launches.  lfd_kernel_timing(ctx, n) makes the next n launches of
 * lfd_triangulate_dense carry a start and a stop event of their own (recorded by the command processor where the kernel begins and
 * ends: the figure a kernel trace reports, without the dispatch gaps that events recorded around the call include); n = 0 switches it
 * off.  lfd_kernel_timing_read waits for the last timed launch and writes the durations in launch order (milliseconds; at most
 * `capacity`, *n_out = how many), then starts a new series.  Asynchronous launches stay asynchronous. */
int lfd_kernel_timing(lfd_context* ctx, int32_t n_launches);
int lfd_kernel_timing_read(lfd_context* ctx, float* ms, int32_t capacity, int32_t* n_out);
const char* lfd_last_error(const lfd_context* ctx); /* ctx may be NULL: last creation error */
/* How THIS build of the library lays out the structures of this header, so that a binding that mirrors them by hand (ctypes, cffi ABI mode,
 * JNA ...) can check itself at load time instead of trusting a transcription: for lfd_params, lfd_batch, lfd_points, lfd_tile_segment and
 * lfd_copy_segment, in that order, {sizeof, number of fields, then offsetof(field), sizeof(field) for every field in declaration order}.  Writes at most `capacity`
 * values to `out` (host int32; may be NULL with capacity 0) and returns how many values the table has.  The Python mirror compares its
 * ctypes `_fields_` with it when it loads the library (core/hip_backend.py::check_struct_layout). */
int lfd_struct_layout(int32_t* out, int32_t capacity);
/* ... and the names behind those numbers: "lfd_params:sampson_thresh,certainty_thresh,...;lfd_batch:n_refs,...;..." - the same structures and
 * fields in the same order (two neighbouring fields of one type swapped in a mirror keep every offset; their names tell). */
const char* lfd_struct_fields(void);

/* Camera table, all host f32 row-major as upstream's CameraRecord holds them
 * (core/camera_models.py:10-28): K[n][9] R[n][9] t[n][3] P[n][12] C[n][3], wh[n][2] = width,height. */
int lfd_upload_cameras(lfd_context* ctx, int32_t n, const float* K, const float* R, const float* t,
                       const float* P, const float* C, const int32_t* wh);

/* ---- the hot path ------------------------------------------------------------------------------ */
/* Optional: the batch-dependent preparation of a launch on its own - validation, upload of the descriptor tables (skipped when the
 * device already holds the same tables) and the per-(reference, neighbour) constants (F5: fundamental matrices, projection blocks,
 * core/geometry.py:53-55,122-130) - stream-ordered, asynchronous.  Every compute entry point below does the same itself when the
 * batch differs from the last one it saw; calling this first only moves that work (a driver can issue it for reference i+1 while
 * reference i computes, and a benchmark can time the kernels apart from it). */
int lfd_prepare_batch(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params);

/* P1+F1: certainty floor, masks, per-cell arg-max over the neighbours (first maximum wins).
 * best_cert: device f32 [n_refs*H*W]; best_slot: device u8 [n_refs*H*W] or NULL. */
int lfd_aggregate(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params,
                  float* best_cert, uint8_t* best_slot);

/* Fused dense kernel: every grid cell -> floor/masks/arg-max -> Sampson -> DLT -> reprojection,
 * cheirality, parallax -> colour -> ordered compaction.  Survivors are emitted per reference in
 * raster order.  Candidates are the cells upstream's sampler could draw (core/sampling.py:24-27, 41-43:
 * a cell whose best certainty after floor and masks is <= 0 - masked out - has weight 0 there) plus the
 * two-cell border upstream keeps out of its draw; a masked-out cell is never triangulated.  ref_offsets: device i64 [n_refs+1] (exclusive prefix of survivors per reference;
 * last = total); seg_counts: device i32 [n_refs*k] survivors per (reference, slot) or NULL. */
int lfd_triangulate_dense(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params,
                          const lfd_points* out, int64_t* ref_offsets, int32_t* seg_counts);

/* Host helper, no context and no device: which instantiation of the fused kernel lfd_triangulate_dense runs for these arguments.  1: the
 * production-shape kernel - the same code compiled for H*W a multiple of the 1024-cell tile and W % 4 == 0, no masks, certainty_thresh > 0,
 * warp_channels == 2 on the default axes (axis_x == axis_y == NULL), the default f32 colour, no_filter off with sampson_thresh > 0 and
 * min_parallax_deg > 0, and seg_counts, out->cell and out->slot all NULL; 0: the generic kernel (any violated condition, and every launch of a
 * context created with LFD_DENSE_GENERIC=1 in the environment).  The two produce the same bytes (tests/test_gpu_dense_prod.py). */
int lfd_dense_variant(const lfd_batch* batch, const lfd_params* params, const lfd_points* out, const int32_t* seg_counts);

/* The same kernel writing the FILE PAYLOAD itself: survivors leave as 15-byte PLY vertex records (x y z f32 LE, r g b u8 quantised like
 * upstream's to_uint8_rgb - what lfd_pack_ply makes of lfd_triangulate_dense's arrays, byte for byte) in raster order per reference, so a run
 * whose consumer is the PLY writer (streamed output, the exchange of a sharded run) needs no packing pass and writes 15 instead of 28 bytes
 * per survivor.  records: device u8 [capacity * 15]; the reprojection error is not part of a PLY vertex and is not produced; cell / slot:
 * optional as in the lfd_points structure - NULL to skip.  Replaces core/pipeline.py:753-780 + core/writers.py:29-46 for that consumer. */
int lfd_triangulate_dense_ply(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params, uint8_t* records, int64_t capacity,
                              int64_t* ref_offsets, int32_t* seg_counts, int32_t* cell, uint8_t* slot);

/* The same kernel with UNORDERED RETIREMENT (opt-in; the default entry point above stays ordered).  The ordered kernel makes a tile wait
 * for the survivor counts of every tile before it (a decoupled look-back: a fifth of a tile's life on the benchmark shape); here a tile
 * claims room with ONE atomic on its reference's cursor and records where it went:
 *   - reference r owns the region [r*H*W, (r+1)*H*W) of out (out->capacity >= n_refs*H*W, else LFD_ERR_CAPACITY); its survivors fill
 *     [r*H*W, r*H*W + ref_counts[r]) tile after tile in the order the tiles RETIRED, raster order inside a tile;
 *   - table[r * lfd_dense_tiles_per_ref(H, W) + t] = {offset inside the reference's region, survivors} of the reference's t-th tile
 *     (tile t covers grid cells [1024 t, 1024 t + 1024));
 *   - ref_counts: device i64 [n_refs] survivors per reference (it is the cursor array: zeroed by the launch itself).
 * Raster order is tile order, so the consumers below restore upstream's sequence from the table: lfd_order_segments writes the ordered
 * structure-of-arrays result (bit-identical to lfd_triangulate_dense's), lfd_pack_ply_segments / lfd_pack_points3d_segments write the
 * file payload in raster order straight from the unordered buffers.  The reference interface both forms replace is the per-group
 * concatenation of core/pipeline.py:753-780,917-919. */
typedef struct lfd_tile_segment { int32_t offset; int32_t count; } lfd_tile_segment;
#define LFD_FLAG_TILE_SEGMENTS 2 /* informational: set in lfd_params.flags by callers that take the unordered route (the entry point decides) */
int lfd_dense_tiles_per_ref(int32_t H, int32_t W); /* host helper: rows of the tile table per reference */
int lfd_triangulate_dense_segments(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params, const lfd_points* out,
                                   int64_t* ref_counts, int32_t* seg_counts, lfd_tile_segment* table);
/* Both at once: the 15-byte PLY vertex records of lfd_triangulate_dense_ply with the unordered retirement of lfd_triangulate_dense_segments, for a
 * consumer that wants every reference's point SET as file payload and does not care about its raster order (a point cloud has none; the streamed
 * output of a run that does not have to reproduce upstream's byte sequence).  records: device u8 [capacity * 15], capacity >= n_refs*H*W;
 * reference r's records fill [15*r*H*W, 15*(r*H*W + ref_counts[r])) tile after tile in retirement order, raster order inside a tile; table and
 * ref_counts as above.  The same points, byte for byte per record, as lfd_triangulate_dense_ply emits (tests/test_gpu_segments.py). */
int lfd_triangulate_dense_ply_segments(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params, uint8_t* records, int64_t capacity,
                                       int64_t* ref_counts, int32_t* seg_counts, lfd_tile_segment* table);
/* src: the unordered buffers of lfd_triangulate_dense_segments (capacity ignored); dst: ordered result, at most dst->capacity records
 * (cell / slot copied when both sides give them); ref_offsets: device i64 [n_refs + 1] or NULL.  Asynchronous on the context's stream. */
int lfd_order_segments(lfd_context* ctx, int32_t n_refs, int32_t H, int32_t W, const lfd_tile_segment* table, const lfd_points* src,
                       const lfd_points* dst, int64_t* ref_offsets);
/* lfd_pack_ply / lfd_pack_points3d through the table: out receives min(total, capacity) records in raster order (ids count from
 * id_base + 1 in that order); ref_offsets as above (the caller reads the total there). */
int lfd_pack_ply_segments(lfd_context* ctx, int32_t n_refs, int32_t H, int32_t W, const lfd_tile_segment* table, const float* xyz,
                          const float* rgb, int64_t capacity, uint8_t* out, int64_t* ref_offsets);
int lfd_pack_points3d_segments(lfd_context* ctx, int32_t n_refs, int32_t H, int32_t W, const lfd_tile_segment* table, const float* xyz,
                               const float* rgb, const float* err, int64_t capacity, uint64_t id_base, uint8_t* out, int64_t* ref_offsets);

/* Upstream-equivalent mode: only the selected cells (sel_idx: device i64, concatenated per
 * reference; sel_offsets: host i64 [n_refs+1]) are triangulated, and survivors are emitted in
 * upstream's order: per reference, neighbour groups in order of first appearance while scanning
 * sel_idx, members in sel_idx order (core/pipeline.py:685-780).  seg_order: device i32 [n_refs*k]
 * or NULL: the slot of the g-th group (or -1). */
int lfd_triangulate_indexed(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params,
                            const int64_t* sel_idx, const int64_t* sel_offsets, const lfd_points* out,
                            int64_t* ref_offsets, int32_t* seg_counts, int32_t* seg_order);

/* One reference view (batch->n_refs == 1) through upstream's whole per-reference stage (core/pipeline.py:602-780,
 * `_triangulate_ref`) in ONE stream-ordered call with nothing read back in between: lfd_aggregate -> selection (coverage
 * sampling on the context's MT19937 stream, or the top-M of the no_filter mode when params->no_filter) ->
 * lfd_triangulate_indexed on the cells selected.  Equivalent to the three calls, bit for bit.
 * out->capacity >= M + tiles*tiles + 64.  sel_info: device i32 [3] = {cells selected, selection status (0 = ok, else
 * the LFD_SELECT_* code upstream would have raised for), launch status (what lfd_launch_status would report: 0 = ok)};
 * with a non-zero selection status or an empty selection no point is emitted (ref_offsets = {0, 0}).  sel_cells: device i64 [M + tiles*tiles + 64] receiving the selected cells, or NULL. */
int lfd_triangulate_sampled(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params, int32_t M, float cap,
                            int32_t border, int32_t tiles, float s_override, const lfd_points* out, int64_t* ref_offsets,
                            int32_t* seg_counts, int32_t* seg_order, int32_t* sel_info, int64_t* sel_cells);

/* The same for SEVERAL reference views per call, each drawing from its own MT19937 stream seeded with seeds[r] (host u32
 * [n_refs]) like np.random.seed(seeds[r]) - the per-reference streams of the multi-GPU / per_reference_rng mode, where no
 * reference depends on another one's draws.  One aggregate launch and one pair of indexed launches serve the whole batch; the
 * selections run one after the other.  out->capacity >= n_refs * (M + tiles*tiles + 64).  sel_info: device i32 [2*n_refs + 1] =
 * {cells selected, selection status} per reference, then the launch status.  sel_cells: device i64 [n_refs * (M + tiles*tiles +
 * 64)] (reference r's cells start at r * (M + tiles*tiles + 64)) or NULL.  The context's own stream is left seeded with the last
 * reference's seed. */
int lfd_triangulate_sampled_multi(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params, int32_t M, float cap,
                                  int32_t border, int32_t tiles, const uint32_t* seeds, const lfd_points* out,
                                  int64_t* ref_offsets, int32_t* seg_counts, int32_t* seg_order, int32_t* sel_info,
                                  int64_t* sel_cells);

/* SEVERAL reference views per call on the CONTEXT's one MT19937 stream - upstream's single global stream (np.random.seed(config.seed) once,
 * core/pipeline.py:793; every reference's np.random.choice continues where the one before it stopped, core/sampling.py:32) - consumed in
 * batch order: the points, the cells selected and the position the stream is left at are those of n_refs successive
 * lfd_triangulate_sampled calls, bit for bit.  What does not depend on the stream (weights, probabilities, the first cumulative sum of every
 * reference) runs side by side; a reference starts drawing where the one before it stopped.  A reference whose selection refuses its input
 * (selection status 1-3: upstream raises before it draws) consumes nothing and emits nothing, the others are not affected.  A status of 4-7 on
 * any reference is THIS implementation's refusal, not upstream's: the call is VOID as a whole (a chain whose bounded waits expire - 5 - commits
 * nothing to the stream although its first references have drawn; a reference refused for inexactness - 4 - draws nothing although upstream would
 * have).  Callers that read the status behind further launches take lfd_rng_checkpoint before the call and, on such a status, roll back and redo
 * the references with lfd_triangulate_sampled one at a time (core/strategies.py::SampledLoop._recover does).
 * s_overrides: host f32 [n_refs] or NULL - the normaliser of reference r (> 0: upstream's own torch sum, handed in; else the exact device sum).
 * out->capacity, sel_info, sel_cells: as lfd_triangulate_sampled_multi.  lfd_rng_seed / lfd_rng_set_state first. */
int lfd_triangulate_sampled_chain(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params, int32_t M, float cap,
                                  int32_t border, int32_t tiles, const float* s_overrides, const lfd_points* out,
                                  int64_t* ref_offsets, int32_t* seg_counts, int32_t* seg_order, int32_t* sel_info,
                                  int64_t* sel_cells);

/* S: coverage sampling on the device (core/sampling.py:8-53, filter mode).  The context owns a legacy
 * MT19937 stream seeded like np.random.seed(seed); every call consumes it exactly as upstream's
 * np.random.choice does, so successive references see the same stream upstream would.
 * best_cert: device f32 [H*W] (one reference, from lfd_aggregate).  sel_out: device i64 [capacity],
 * ascending cell indices (capacity >= M + tiles*tiles is always enough).  Synchronises; the count and
 * a status (0 ok; 1 NaN, 2 negative, 3 "Fewer non-zero entries in p than size" - the conditions
 * under which upstream's np.random.choice raises ValueError; 4.. internal) are returned on the host.
 * s_override > 0 replaces the normaliser sum(weights) (upstream's is a torch f32 reduction whose
 * rounding depends on the host's thread count; the device uses the correctly rounded exact sum).
 * Limit: the coverage pass holds at most 2304 tiles (tile = max(1, W / tiles) cells per side, ceil(W / tile) * ceil(H / tile) of
 * them): every square grid fits (47 x 47 has the most, 2209; RoMa's grids of 320 ... 1280 cells per side have 576 ... 625); a grid
 * beyond the limit (much taller than wide: 24 x 200) is refused with LFD_ERR_INVALID and a message that says so - the host
 * selection stage has no such limit. */
int lfd_rng_seed(lfd_context* ctx, uint32_t seed);
int lfd_rng_get_state(lfd_context* ctx, uint32_t* key624_host, int32_t* pos_host);
int lfd_rng_set_state(lfd_context* ctx, const uint32_t* key624_host, int32_t pos);
/* The stream put aside and taken back ON THE DEVICE, in stream order, without a host wait: lfd_rng_checkpoint copies the context's MT19937
 * state (key + position) into one of LFD_RNG_CHECKPOINTS places, lfd_rng_rollback copies it back.  A caller that launches fused calls AHEAD
 * of reading their status (lfd_triangulate_sampled_chain: a chain whose bounded spins expire commits nothing, a reference refused for
 * inexactness draws nothing although upstream would have) takes a checkpoint before every call and, on such a status, rolls back to the
 * first affected call's checkpoint and redoes the references one at a time - the stream then continues exactly where upstream's would. */
#define LFD_RNG_CHECKPOINTS 4
int lfd_rng_checkpoint(lfd_context* ctx, int32_t place);
int lfd_rng_rollback(lfd_context* ctx, int32_t place);
int lfd_select_samples(lfd_context* ctx, const float* best_cert, int32_t H, int32_t W, int32_t M, float cap,
                       int32_t border, int32_t tiles, float s_override, int64_t* sel_out, int64_t capacity,
                       int32_t* n_sel_host, int32_t* status_host);

/* no_filter branch of the selection (core/sampling.py:15-21): the min(M, H*W) largest capped
 * certainties in descending order (ties: ascending cell index; NumPy leaves tie order unspecified;
 * NaN last).  M <= 16384.  Does not touch the RNG stream.  Synchronises like lfd_select_samples. */
int lfd_select_top_m(lfd_context* ctx, const float* best_cert, int32_t H, int32_t W, int32_t M, float cap,
                     int64_t* sel_out, int64_t capacity, int32_t* n_sel_host, int32_t* status_host);

/* N1: file payloads on the device (core/writers.py:15-46, core/image_utils.py:24-26).  Colours are
 * quantised like upstream's to_uint8_rgb: clip(round_half_even(c * 255), 0, 255).
 * lfd_pack_ply:      out[n*15] = per point x y z (f32 LE) r g b (u8): the PLY body after upstream's header.
 * lfd_pack_points3d: out[n*43] = per point u64 id (id_base + i + 1), xyz as f64, rgb u8, error f64
 *                    (err may be NULL -> 0.0): upstream's points3D.bin body after the u64 count.
 * lfd_pack_ply_normals: out[n*27] = per point x y z nx ny nz (f32 LE) r g b (u8): the body of a PLY whose header lists
 *                    x y z nx ny nz red green blue (normals: lfd_estimate_normals' f32 [3*n]).
 * out must be 4-byte aligned.  Asynchronous on the context's stream. */
int lfd_pack_ply(lfd_context* ctx, const float* xyz, const float* rgb, int64_t n, uint8_t* out);
int lfd_pack_ply_normals(lfd_context* ctx, const float* xyz, const float* normals, const float* rgb, int64_t n, uint8_t* out);
int lfd_pack_points3d(lfd_context* ctx, const float* xyz, const float* rgb, const float* err, int64_t n,
                      uint64_t id_base, uint8_t* out);
int lfd_quantise_rgb(lfd_context* ctx, const float* rgb, int64_t n, uint8_t* out);

/* The GUI's distance filter (densify._voxel_downsample, NumPy branch; upstream densify.py:29-50 with Open3D): one point per occupied voxel,
 * bit for bit and in the same order as the NumPy branch for the same arrays.  xyz, rgb: n x 3 f32 on the device.
 *   origin_c = (f64) min_c x - 0.5 voxel_size;  key_c = floor(((f64) x_c - origin_c) / voxel_size)  (IEEE f64 subtract and divide)
 *   voxels in ascending lexicographic (k0, k1, k2) - np.unique(axis=0)'s row order
 *   per voxel, in f64 from 0.0 over its points in ascending index (np.add.at's order): the sum of (f64) xyz and of (f64) rgb / s, where
 *   s = 255 if max(rgb) > 1 else 1 (a NaN colour makes the max NaN: s = 1); xyz_out / rgb_out = (f32) (sum / count), round to nearest even.
 * xyz_out and rgb_out hold n rows (there are never more voxels than points); *n_out_host receives the voxel count (n = 0 gives 0).
 * Synchronous.  The workspace lives on the context (grown on demand, freed by lfd_destroy).
 * LFD_ERR_INVALID: a null pointer, n < 0 or n > 2^31 - 1, a voxel_size <= 0 or not finite, and - decided in the min / max pass, before
 * anything is sorted - "non-finite coordinate" (an inf / NaN in xyz) or "key range" (the linear key k0 E1 E2 + k1 E2 + k2, E_c = max key_c + 1,
 * does not fit 63 bits); lfd_last_error names which. */
int lfd_voxel_downsample(lfd_context* ctx, const float* xyz, const float* rgb, int64_t n, double voxel_size,
                         float* xyz_out, float* rgb_out, int64_t* n_out_host);

/* Local correlation of RoMa-v2's conv refiners (RoMaV2/src/romav2/local_correlation.py looks for a CUDA-only extension `local_corr` and, without
 * it, materialises the sampled neighbour features as a (C, h, w, K) tensor):
 *
 *   out[b, n, k] = sum_c A[b, n, c] * bilinear(Bf[b, :, :, c]; warp[b, n, k])
 *
 * A (B, N, C) f32, Bf (B, H1, W1, C) f32, warp (B, N, K, 2) f32 contiguous, (x, y) normalised as F.grid_sample(mode="bilinear",
 * padding_mode="zeros", align_corners=False) reads them: ix = ((x + 1) W1 - 1) / 2 in f32, the four texels round (ix, iy), texels outside the
 * map count as 0.  out (B, N, K) f32 contiguous.  a_strides[3] / bf_strides[4]: element strides of A / Bf in the order of their dimensions
 * (NULL: contiguous); channels adjacent (stride 1), C % 4 == 0 and 16-byte aligned rows take the vector kernel, anything else the general one.
 * Departure from grid_sample: a coordinate that is inf, NaN or beyond the map by any amount contributes exactly 0 - no address is formed from it.
 * Deterministic (no atomics).  One launch on the context's stream, asynchronous.  LFD_ERR_INVALID: a null pointer, B, N, K < 0, C, H1, W1 < 1,
 * H1 or W1 > 32768, B N > 2^26 - 1, B N K > 2^31 - 1, a negative stride.  lfd_local_corr_host: the same routine over host pointers on a host
 * context's threads (the general kernel's summation order). */
int lfd_local_corr(lfd_context* ctx, const float* A, const float* Bf, const float* warp, int32_t B, int32_t N, int32_t C, int32_t K,
                   int32_t H1, int32_t W1, const int64_t* a_strides, const int64_t* bf_strides, float* out);
int lfd_local_corr_host(lfd_context* ctx, const float* A, const float* Bf, const float* warp, int32_t B, int32_t N, int32_t C, int32_t K,
                        int32_t H1, int32_t W1, const int64_t* a_strides, const int64_t* bf_strides, float* out);

/* One conv block of RoMa-v2's refiners in one pass (RoMaV2/src/romav2/refiner.py: each of the three ConvRefiners runs nine blocks of depthwise 5x5
 * convolution, eval-mode BatchNorm, ReLU and 1x1 convolution under bf16 autocast).  x (B, C, H, W) contiguous NCHW, bf16 (16-bit
 * words) or, with x_is_f32 != 0, f32 that is rounded to bf16 on load; dw_w (C, 25) the depthwise weights as stored (f32, not rounded); scale /
 * shift (C) the folded affine s = gamma / sqrt(var + eps), t = beta + (bias_dw - mean) s; out (B, C, H, W) bf16 as 16-bit words.  In f32 with
 * IEEE fmaf, every rounding written out (csrc/lfd_block.hpp):
 *   a = 0; for ky = 0..4, kx = 0..4: a = fmaf(w[c][5 ky + kx], x[y + ky - 2][x + kx - 2], a), a tap outside the plane skipped
 *   h = relu(fmaf(s[c], a, t[c])) rounded to bf16 (nearest even; a NaN stays a quiet NaN, -0 becomes +0)
 * pw_wT == NULL: out = h.  Otherwise pw_wT (C, C) holds the 1x1 weights TRANSPOSED - row c the weights that multiply hidden channel c - and
 * pw_b (C) its bias: z = pw_b[o]; for c = 0..C-1: z = fmaf(pw_wT[c][o], h[c], z); out = z rounded to bf16.  Implemented for C == 32 only.
 * One launch on the context's stream, asynchronous, no atomics.  LFD_ERR_INVALID: a null required pointer, exactly one of pw_wT / pw_b,
 * B, C, H or W < 1, pw_wT with C != 32, H or W > 32768, B C H W > 2^31 - 1, out overlapping x.  lfd_refiner_block_host: the same routine
 * over host pointers on a host context's threads - the same bits, whatever the thread count. */
int lfd_refiner_block(lfd_context* ctx, const void* x, int32_t x_is_f32, int32_t B, int32_t C, int32_t H, int32_t W,
                      const float* dw_w, const float* scale, const float* shift, const float* pw_wT, const float* pw_b, uint16_t* out);
int lfd_refiner_block_host(lfd_context* ctx, const void* x, int32_t x_is_f32, int32_t B, int32_t C, int32_t H, int32_t W,
                           const float* dw_w, const float* scale, const float* shift, const float* pw_wT, const float* pw_b, uint16_t* out);

/* The output head of RoMa-v2's refiners in one pass (RoMaV2/src/romav2/refiner.py: behind its nine blocks each ConvRefiner casts z to f32, runs two
 * 1x1 convolutions, hidden -> 2 and hidden -> 4, and about a dozen element-wise kernels).  z (B, C, H, W) contiguous NCHW, bf16 (16-bit
 * words) or, with z_is_f32 != 0, f32 - used as given, nothing is rounded on load; head_w (6, C) f32, rows 0..1 the warp head's weights, rows 2..5
 * the confidence head's; head_b (6) f32 (zeros for a convolution without bias); prev_warp (B, H, W, 2) f32 read through prev_warp_strides[4],
 * element strides in the order b, y, x, c (NULL: contiguous); prev_conf (B, H, W, prev_dim) f32 through prev_conf_strides[4], prev_dim 0 (prev_conf
 * NULL), 1 or 4; refine_init the model's 4.0.  warp (B, H, W, 2) and conf (B, H, W, 4) f32 contiguous.  In f32 with IEEE fmaf and division, every
 * rounding written out (csrc/lfd_head.hpp):
 *   a[o] = head_b[o]; for c = 0..C-1: a[o] = fmaf(head_w[o][c], z[c], a[o])
 *   warp.x = prev_warp.x + a[0] / (refine_init * (float)W), warp.y = prev_warp.y + a[1] / (refine_init * (float)H)
 *   sp(v) = v > 20 ? v : (float)log1p(exp((double)v)); l00 = sp(a[3]) + 1e-6f, l10 = a[4], l11 = sp(a[5]) + 1e-6f
 *   d = (a[2], l00 l00, l00 l10, l10 l10 + l11 l11); conf = prev + d (prev_dim 1: channels 1..3 of prev are +0; prev_dim 0: conf = d)
 * warp and conf[..., 0] are the same bits on device and host; conf[..., 1:4] pass through the libraries' exp and log1p and may differ by
 * 2^-21 of d plus the rounding of the last addition.  One launch on the context's stream, asynchronous, no atomics, no address formed
 * from data.  LFD_ERR_INVALID: a null required pointer, prev_dim not 0, 1 or 4, prev_conf given or missing contrary to prev_dim, B, C, H or W < 1,
 * H or W > 32768, B C H W > 2^31 - 1, a negative stride or one above 2^31 - 1, refine_init not finite or <= 0, an output overlapping an input or
 * the other output.  lfd_refiner_head_host: the same routine over host pointers on a host context's threads - the same bits, whatever the thread
 * count. */
int lfd_refiner_head(lfd_context* ctx, const void* z, int32_t z_is_f32, int32_t B, int32_t C, int32_t H, int32_t W, const float* head_w,
                     const float* head_b, const float* prev_warp, const int64_t* prev_warp_strides, const float* prev_conf,
                     const int64_t* prev_conf_strides, int32_t prev_dim, float refine_init, float* warp, float* conf);
int lfd_refiner_head_host(lfd_context* ctx, const void* z, int32_t z_is_f32, int32_t B, int32_t C, int32_t H, int32_t W, const float* head_w,
                          const float* head_b, const float* prev_warp, const int64_t* prev_warp_strides, const float* prev_conf,
                          const int64_t* prev_conf_strides, int32_t prev_dim, float refine_init, float* warp, float* conf);

/* Forward-backward consistency gate on RoMa-v2's two warps (upstream has no counterpart: it reads warp_AB / overlap_AB only and its
 * "certainty threshold" is a floor, so a match that slid along its epipolar line - what a dense matcher produces at occlusions and depth steps -
 * passes every two-view test).  For each of n_pairs (reference, neighbour) pairs (1..LFD_MAX_SLOTS; the tables are HOST arrays of n_pairs DEVICE
 * pointers, read before the call returns: they travel in the kernel arguments, nothing is uploaded and nothing synchronises) and each cell of the
 * H x W grid, in f32 with every rounding written out (csrc/lfd_cycle.hpp):
 *   c        = certainty floored at certainty_thresh (the floor of lfd_params.certainty_thresh, NaN stays NaN)
 *   (xb, yb) = channels C-2, C-1 of warp_ab (C = warp_channels: 4 [xA,yA,xB,yB] or 2 [xB,yB]); (xa, ya) = channels 0, 1, or axis_x / axis_y
 *              as in lfd_batch when C == 2 (both NULL: lfd_identity_axis values)
 *   not (-1 <= xb <= 1 and -1 <= yb <= 1), NaN included: REJECTED, error +inf; no address is formed from such a coordinate
 *   ix = ((xb + 1) Wb - 1) / 2, iy likewise; (xa', ya') = bilinear blend of warp_ba (f32 [Hb*Wb*2]: normalised A-coordinates on B's grid) with
 *              the taps clamped to the grid (F.grid_sample(padding_mode="border", align_corners=False))
 *   dx = (xa' - xa) 0.5 (w_match - 1), dy = (ya' - ya) 0.5 (h_match - 1), d2 = dx dx + dy dy   (upstream's pixel conversion)
 *   kept iff d2 <= tau2, tau2 = the f32 square of cycle_thresh_px formed once on the host (a NaN rejects)
 *   cert_out = kept ? c : 0.0f;   err_out = sqrtf(d2)
 * cert_out[i] may be cert[i] (in place).  err_out: NULL, or a table of n_pairs planes f32 [H*W].  rejected: NULL, or device i32 [n_pairs] that the
 * number of rejected cells of every pair is ADDED to (zero it once, read it once per run).  A gated plane already carries the floor: hand it to
 * the entry points above with lfd_params.certainty_thresh = min(thresh, 0) and a rejected cell behaves like one that mask_b masks out.
 * One launch on the context's stream, asynchronous, deterministic.  LFD_ERR_INVALID: a null pointer (table or element), n_pairs outside
 * 1..LFD_MAX_SLOTS, H, W, Hb, Wb outside 1..32768, w_match or h_match < 1, warp_channels not 2 or 4, only one of the axes, a cycle_thresh_px that is
 * <= 0 or not finite.  lfd_cycle_gate_host: the same routine over host pointers (rejected: host i32 [n_pairs]) on a host context's threads; its
 * cert_out and counters equal the device's bit for bit. */
int lfd_cycle_gate(lfd_context* ctx, int32_t n_pairs, const float* const* cert, const float* const* warp_ab, const float* const* warp_ba, int32_t H,
                   int32_t W, int32_t warp_channels, int32_t Hb, int32_t Wb, const float* axis_x, const float* axis_y, int32_t w_match,
                   int32_t h_match, float certainty_thresh, float cycle_thresh_px, float* const* cert_out, float* const* err_out,
                   int32_t* rejected);
int lfd_cycle_gate_host(lfd_context* ctx, int32_t n_pairs, const float* const* cert, const float* const* warp_ab, const float* const* warp_ba,
                        int32_t H, int32_t W, int32_t warp_channels, int32_t Hb, int32_t Wb, const float* axis_x, const float* axis_y,
                        int32_t w_match, int32_t h_match, float certainty_thresh, float cycle_thresh_px, float* const* cert_out,
                        float* const* err_out, int32_t* rejected);

/* Multi-view support filter BEHIND triangulation (upstream has no counterpart: it loads nns_per_ref neighbours per reference, keeps the
 * most certain one per cell and never looks at the others again, so nothing checks a triangulated point against a third view - the only thing that
 * can refute a match that slid along its epipolar line and triangulated cleanly to the wrong depth).  "Keep a point only if at least m other views
 * agree with it", the fusion rule of multi-view stereo, on data that is resident anyway: `in` is what lfd_triangulate_dense / _indexed /
 * _sampled* wrote for `batch` (in->cell and in->slot required), reference r's points are [ref_offsets_in[r], ref_offsets_in[r+1]) (device i64
 * [n_refs + 1]; offsets beyond in->capacity count as in->capacity).  Per input point i of reference r with s = slot[i], cell = cell[i], X = xyz[i],
 * for every slot j != s, j < n_slots[r], in f32 with every rounding written out (csrc/lfd_support.hpp):
 *   live(j)      cert[r,j][cell] > 0 (the RAW plane: a NaN, and the exact 0 lfd_cycle_gate leaves, are not live) and, where mask_b[r,j] is given, the
 *                mask pixel the slot's warp points at is non-zero - looked up as the kernels' certainty prologue does (lfd_grid_nearest, a
 *                coordinate outside the grid: not live).  mask_a plays no part: the point exists.
 *   (ub, vb)     = ((xb + 1) 0.5 (w_match - 1)) sx_j, ((yb + 1) 0.5 (h_match - 1)) sy_j - the pixel conversion and the camera-pixel scale of the
 *                  triangulation kernels; (xb, yb) = channels C-2, C-1 of warp[r,j][cell]
 *   (px, py, pz) = the rows of P_j applied to (X, 1): the FMA chain of the reprojection test, so a point projects to the same f32 everywhere
 *   agree(j)     du = px - ub pz, dv = py - vb pz, d2 = du du + dv dv, t = support_thresh_px pz: pz > 0 and d2 <= t t   (a NaN rejects)
 *   support_i    = the number of j that are live and agree; the point is KEPT iff support_i >= min_support
 * A cell outside the grid has support 0 (no address is formed from it).  The kept points are compacted STABLY into `out` (input order inside and
 * across references: dense raster order and the sampled mode's slot groups survive), every given array copied bit for bit; out->cell / out->slot
 * optional.  ref_offsets_out: device i64 [n_refs + 1], always written (the counts stay on the device).  seg_counts_out: NULL, or device i32
 * [n_refs*k], the kept points per (reference, winning slot), overwritten.  support: NULL, or device u8 [in->capacity], support_i of every INPUT point.
 * Three launches on the context's stream, asynchronous, deterministic (integer atomics only).  The batch is prepared like the compute entry points
 * above prepare it (only when it differs from the last one seen).  LFD_ERR_INVALID: a null required pointer, missing cell / slot, in->capacity
 * > 2^31 - 1, min_support outside 1..LFD_MAX_SLOTS-1, a support_thresh_px that is <= 0 or not finite, overlapping in / out arrays;
 * LFD_ERR_CAPACITY: out->capacity < in->capacity.  lfd_support_filter_host: the same routine over host pointers on a host context's threads; every
 * output equals the device's bit for bit. */
int lfd_support_filter(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets_in, int32_t min_support,
                       float support_thresh_px, const lfd_points* out, int64_t* ref_offsets_out, int32_t* seg_counts_out, uint8_t* support);
int lfd_support_filter_host(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets_in, int32_t min_support,
                            float support_thresh_px, const lfd_points* out, int64_t* ref_offsets_out, int32_t* seg_counts_out, uint8_t* support);

/* Multi-view re-triangulation of supported points (no upstream counterpart).  lfd_support_filter uses the other neighbours that agree
 * with a two-view point for a vote only; here their observations place the point.  `in` / ref_offsets: what a triangulation call (or
 * lfd_support_filter) wrote for `batch` (in->cell and in->slot required, in->rgb unused; offsets beyond in->capacity count as in->capacity).  Per
 * input point of reference r with s = slot[i], cell = cell[i], X = xyz[i] (csrc/lfd_refine.hpp, every rounding written out):
 *   candidates   every slot j != s, j < n_slots[r], that lfd_support_filter would count for X at support_thresh_px (live and agree, the same
 *                routines: the same set bit for bit); n_extra their number.  n_extra == 0, a cell outside the grid or s >= n_slots[r]: the point is
 *                copied bit for bit
 *   rows         per view the DLT rows u p2 - p0, v p2 - p1 in f32 as the triangulation kernels form them; the reference's observation is warp
 *                channels 0, 1 of slot s (four channels) or the A-grid axes (two), every other view's the last two channels of its own warp
 *   solve        M = sum row row^T in f64 (one fma chain; reference, slot s, candidates by ascending j), smallest eigenvector by the kernels'
 *                scheme (LDL^T, inverse iteration, Rayleigh-shifted passes), X' = c[0..2] / c[3] rounded to f32
 *   acceptance   X' replaces X iff it is finite, the two-view test of the triangulation kernels holds in the reference and in slot s (depth > 0,
 *                max reprojection error <= reproj_thresh) and every candidate still agrees with X' at support_thresh_px; err' = that max
 *                reprojection error.  Otherwise (a NaN anywhere included) the two-view point and its err are emitted bit for bit.  The parallax
 *                test is not repeated.
 * xyz_out / err_out: exactly in->xyz and in->err (in place: every point is independent) or arrays [3 * capacity] / [capacity] that overlap nothing
 * of `in`; points beyond the last offset are not touched.  status: NULL, or u8 [capacity]: n_extra | (accepted ? 0x80 : 0) per input point.
 * counters: NULL, or device i64 [2] that is ADDED to: points refined, points with a candidate that kept their two-view position.  One launch on the
 * context's stream, asynchronous, deterministic; the batch is prepared as lfd_support_filter prepares it.  LFD_ERR_INVALID: a null required
 * pointer, missing cell / slot, a threshold that is <= 0 or not finite, partial overlap, in->capacity > 2^31 - 1.  lfd_refine_multiview_host: the
 * same routine over host pointers on a host context's threads; the candidate sets are the device's bit for bit, X' agrees to the last bits (the
 * host divides where the device refines a reciprocal). */
int lfd_refine_multiview(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets, float support_thresh_px,
                         float reproj_thresh, float* xyz_out, float* err_out, uint8_t* status, int64_t* counters);
int lfd_refine_multiview_host(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets, float support_thresh_px,
                              float reproj_thresh, float* xyz_out, float* err_out, uint8_t* status, int64_t* counters);

/* Precision-weighted multi-view re-triangulation (no upstream counterpart).  RoMa-v2 predicts a 2x2 precision matrix (inverse error
 * covariance, px^-2) per match in every preset and nothing uses it; lfd_refine_multiview gives every view's two algebraic rows the same weight, so a
 * blurry, oblique neighbour pulls a point as hard as a sharp one.  The arguments, the candidates, the rows, the solver, the acceptance, the fallback,
 * the refusals and the launch are lfd_refine_multiview's; what differs (csrc/lfd_refine.hpp, every rounding written out):
 *   precision    HOST array [n_refs * k] of DEVICE planes [H*W*3] f32 (host planes for the twin), (q00, q01, q11) per cell: the neighbour's
 *                precision in px^-2 of its MATCH image, in the pixel convention of the warps.  Entries at j >= n_slots[r] are ignored
 *   valid(j)     all three values finite, q00 > 0, q11 > 0, q00 q11 - q01 q01 > 0 (f64: exact products, one rounding)
 *   weights      per participating neighbour j (slot s, the candidates): p = (q00 / (sx sx), q01 / (sx sy), q11 / (sy sy)) in camera px^-2 and
 *                w2 = 1 / (pz pz), pz the f32 depth of the two-view X in view j, both in f64; the view adds w2 (p00 ru ru^T + p01 (ru rv^T +
 *                rv ru^T) + p11 rv rv^T) to M, order slot s, candidates by ascending j.  The reference - a cell centre, no matching noise - is
 *                added last as lamA w2_A (ru ru^T + rv rv^T), lamA = sum_j (p00_j + p11_j) / 2: the result does not depend on a common scale
 *                of the planes.  ANY participating view invalid: the point is solved with lfd_refine_multiview's unweighted rows, bit for bit
 * status: n_extra | (weighted rows used ? 0x40 : 0) | (accepted ? 0x80 : 0).  counters: NULL, or device i64 [3] that is ADDED to: points refined,
 * points with a candidate that kept their two-view position, points solved with weighted rows.  The table of plane pointers reaches the device
 * as the batch's descriptor tables do: compared with what the device holds, uploaded on the context's stream when it differs, no synchronisation.
 * One launch, asynchronous, deterministic.  LFD_ERR_INVALID: what lfd_refine_multiview refuses, a null `precision`, a null plane in a valid slot.
 * lfd_refine_multiview_weighted_host: the same routine over host pointers on a host context's threads. */
int lfd_refine_multiview_weighted(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets,
                                  float support_thresh_px, float reproj_thresh, float* xyz_out, float* err_out, uint8_t* status, int64_t* counters,
                                  const float* const* precision);
int lfd_refine_multiview_weighted_host(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets,
                                       float support_thresh_px, float reproj_thresh, float* xyz_out, float* err_out, uint8_t* status,
                                       int64_t* counters, const float* const* precision);

/* Depth-uncertainty gate on triangulated points (no upstream counterpart - upstream's only depth-conditioning test is the fixed
 * parallax angle).  Per point X of reference r made by winning slot s: X(l) = C_A + l D, D = X - C_A; sigma_rel is the 1-sigma Cramer-Rao
 * bound on l, the relative depth error, from the views that placed the point (csrc/lfd_sigma.hpp, every rounding written out, f64 from the f32
 * inputs, rounded to f32 once):
 *   view j       (px, py, pz) = P_j (X, 1), h = P_j[:, :3] D, g = (hx / pz - px hz / pz^2, hy / pz - py hz / pz^2) camera px per unit l,
 *                I_j = p00 gx^2 + 2 p01 gx gy + p11 gy^2 with the view's precision p in camera px^-2; sigma_rel = 1 / sqrt(sum_j I_j).
 *                A view with pz <= 0 or a non-finite I_j is skipped.  +inf: sum not finite or <= 0, no view, X not finite, a cell outside the
 *                grid, a slot the reference does not have (no address is formed from either)
 *   views        the winning slot; with refine_status non-null (the status of lfd_refine_multiview[_weighted]) and 0x80 set for the point
 *                also every slot j != s that lfd_support_filter's candidate test accepts at X and support_thresh_px, by ascending j.  With
 *                refine_status NULL no other slot's certainty, warp or precision is read and support_thresh_px is ignored
 *   precision    exactly one of: `precision` (the table of lfd_refine_multiview_weighted: p = q / (s s), a view whose entry is not valid
 *                there is skipped) or iso_sigma_px > 0 (every view p00 = p11 = 1 / iso_sigma_px^2, p01 = 0; camera px, reproj_thresh's unit)
 *   gate         max_rel_sigma > 0: kept iff sigma_rel <= max_rel_sigma (NaN and +inf drop); 0: every point is kept (annotate only)
 * Compaction, `out`, ref_offsets_out (always written, stays on the device), seg_counts_out (optional), the batch preparation and the three
 * launches are lfd_support_filter's.  sigma_rel: NULL, or f32 [in->capacity], one value per INPUT point; sigma_rel_out: NULL, or f32
 * [out->capacity], compacted with the points.  LFD_ERR_INVALID: a null required pointer, missing cell / slot, both or neither of precision and
 * iso_sigma_px > 0, a null plane in a valid slot, max_rel_sigma negative or not finite, refine_status with support_thresh_px not finite or
 * <= 0, in and out overlapping, a capacity beyond 2^31 - 1; LFD_ERR_CAPACITY: out->capacity < in->capacity.  lfd_depth_sigma_filter_host: the
 * same routine over host pointers on a host context's threads; the participating sets are the device's bit for bit, sigma_rel agrees within
 * one f32 ulp (the host divides and takes an IEEE root where the device refines v_rcp_f64 / v_rsq_f64). */
int lfd_depth_sigma_filter(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets_in,
                           const float* const* precision, float iso_sigma_px, const uint8_t* refine_status, float support_thresh_px,
                           float max_rel_sigma, const lfd_points* out, int64_t* ref_offsets_out, int32_t* seg_counts_out, float* sigma_rel,
                           float* sigma_rel_out);
int lfd_depth_sigma_filter_host(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets_in,
                                const float* const* precision, float iso_sigma_px, const uint8_t* refine_status, float support_thresh_px,
                                float max_rel_sigma, const lfd_points* out, int64_t* ref_offsets_out, int32_t* seg_counts_out,
                                float* sigma_rel, float* sigma_rel_out);

/* Per-point surface normals from the resident warps (no upstream counterpart - upstream writes x y z r g b).  Per input point X
 * of reference r made by winning slot s on cell (x, y): the winning slot's warp in the (2 radius_cells + 1)^2 window of grid cells around the
 * cell gives the neighbouring surface samples, and the normal is the cross product of the two regression slopes of those samples on the cell
 * offsets, oriented towards the reference's centre C_A (csrc/lfd_normals.hpp, every rounding written out):
 *   fallback     Vw / |Vw|, Vw = C_A - X in f64, rounded to f32; (0, 0, 0) where |Vw| is zero or not finite
 *   guard        the fallback with status 0 where X is not finite, the cell lies outside the grid, s >= n_slots[r] or X's depth in the
 *                reference (row 2 of P_A applied to (X, 1)) is not > 0 (no address is formed from the cell or the slot)
 *   window       cells q = (x + dx, y + dy) inside the grid, dy outer, dx inner, the centre included.  q takes part iff it is live in slot
 *                s as lfd_support_filter defines it (raw certainty > 0, the mask_b pixel its warp points at non-zero), the reference's
 *                mask_a pixel of q is non-zero, its own two-view point Y_q (the routine of lfd_triangulate_dense, Sampson and parallax
 *                gates off) passes that routine's test at reproj_thresh, and |pz(Y_q) - pz(X)| <= depth_step_rel * pz(X) in f32
 *   fit          n, sum dx, sum dy, sum dx^2, sum dx dy, sum dy^2 in integers; sum D, sum dx D, sum dy D, D = Y_q - X, in f64 in the visiting
 *                order; U = n sum dx D - sum dx sum D, V likewise with dy, N = U x V, negated when N . Vw < 0.  The fallback with status n
 *                where the cells are fewer than three or collinear or N . N is not finite or not > 0; otherwise N / |N| rounded to f32
 *                and status n | 0x80
 * `in` and ref_offsets are what a triangulation call or any post-stage wrote (cell and slot required, rgb and err unused); nothing of `in`
 * is written and points beyond the last offset are not touched.  normals_out: f32 [3 * in->capacity]; status: NULL or u8 [in->capacity];
 * counters: NULL or device i64 [2], ADDED to: points fitted, points that fell back (integer adds only).  One launch on the context's
 * stream, asynchronous and deterministic; the batch is prepared as lfd_support_filter prepares it.  LFD_ERR_INVALID: a null required
 * pointer, missing cell / slot, radius_cells outside 1..4, depth_step_rel or reproj_thresh <= 0 or not finite, normals_out or status
 * overlapping any array of `in` (or each other), a capacity beyond 2^31 - 1.  lfd_estimate_normals_host: the same routine over host pointers
 * on a host context's threads (counters: host i64 [2]); the statuses are the device's wherever the window's points are, the components agree
 * within one f32 ulp (the host divides by an IEEE root where the device refines v_rcp_f64 / v_rsq_f64).  A host context is served by
 * _host only, a device context refuses _host (LFD_ERR_STATE). */
int lfd_estimate_normals(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets, int32_t radius_cells,
                         float depth_step_rel, float reproj_thresh, float* normals_out, uint8_t* status, int64_t* counters);
int lfd_estimate_normals_host(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets, int32_t radius_cells,
                              float depth_step_rel, float reproj_thresh, float* normals_out, uint8_t* status, int64_t* counters);

/* Multi-view point colour (no upstream counterpart - upstream's colour is the bilinear sample of the reference image alone).  A
 * column rewrite, not a filter: no point, count or order changes.  Per input point X of reference r made by winning slot s on cell c, all in
 * f32 with every rounding written out (csrc/lfd_colour.hpp):
 *   guard        the three rgb values are copied bit for bit with status 0 where X or in->rgb[i] is not finite, the cell lies outside the grid
 *                or s >= n_slots[r] (no address is formed from the cell or the slot)
 *   views        in this order: the reference, whose colour is in->rgb[i] as it stands; the winning slot s unless its observation (the last
 *                two channels of warp[r, s][c]) is not finite; every slot j != s, j < n_slots[r], ascending, that lfd_support_filter's
 *                candidate test accepts for X at support_thresh_px - the same routine, hence the same set
 *   colour       of neighbour j: the four-tap f32 blend lfd_triangulate_* use for the reference image, applied to nbr_image[r * k + j] at
 *                the match pixel ((xb + 1) * 0.5) * (w_match - 1), ((yb + 1) * 0.5) * (h_match - 1) of its observation (xb, yb)
 *   mode 1       mean: per channel sum = c_ref; sum = sum + c_s; sum = sum + c_j ...; the result is sum * RN_f32(1 / n), the factor from
 *                a table (1 / n in f64, rounded once)
 *   mode 2       median: per channel the middle one of the n values in ascending order, (lo + hi) * 0.5f of the two middle ones for even n
 * nbr_image: HOST array [n_refs * k] of DEVICE images u8 [h_match * w_match * 3] (entries at j >= n_slots[r] are ignored); the table is kept on
 * the device, compared with what it holds and uploaded on the context's stream when it differs, without synchronising.  `in` and ref_offsets
 * are what a triangulation call or any post-stage wrote (cell, slot and rgb required, err unused).  rgb_out: exactly in->rgb (in place), or
 * f32 [3 * in->capacity] overlapping nothing of `in`; status: NULL or u8 [in->capacity], the number of views n blended (0: guarded); points
 * beyond the last offset are not touched.  counters: NULL or device i64 [2], ADDED to: points blended, the sum of their n (integer adds only).
 * One launch on the context's stream, asynchronous and deterministic; the batch is prepared as lfd_support_filter prepares it.
 * LFD_ERR_INVALID: a null required pointer, missing cell / slot / rgb, a null image in a valid slot, mode outside {1, 2}, support_thresh_px
 * <= 0 or not finite, rgb_out or status partially overlapping `in` or each other, a capacity beyond 2^31 - 1.  lfd_colour_multiview_host: the
 * same routine over host pointers (host images, counters: host i64 [2]) on a host context's threads, the same bits.  A host context is served
 * by _host only, a device context refuses _host (LFD_ERR_STATE). */
#define LFD_COLOUR_MEAN 1
#define LFD_COLOUR_MEDIAN 2
int lfd_colour_multiview(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets,
                         const uint8_t* const* nbr_image, float support_thresh_px, int32_t mode, float* rgb_out, uint8_t* status,
                         int64_t* counters);
int lfd_colour_multiview_host(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets,
                              const uint8_t* const* nbr_image, float support_thresh_px, int32_t mode, float* rgb_out, uint8_t* status,
                              int64_t* counters);

/* Per-image exposure gains, the statistics (no upstream counterpart).  Reads only: no point, colour, count or order changes.
 * The views of a point are lfd_colour_multiview's, by the same routines (csrc/lfd_colour.hpp): the reference, whose colour is in->rgb[i]; the
 * winning slot unless its observation is not finite; every other slot lfd_support_filter's candidate test accepts at support_thresh_px; a
 * guarded point (see there) has none.  For each (point of reference r, confirming slot j) the neighbour's colour is sampled as there, and
 *   the sample counts iff all six values - the reference's r, g, b and the neighbour's - lie in [0.05f, 0.95f] (f32 comparisons);
 *   each value is quantised as (uint32_t)(c * 16777216.0f): exact, a power of two and a truncation;
 *   row [r * k + j] of table, u64 [n_refs * k][7], receives N += 1, Sref[0..3) += q_ref, Snbr[0..3) += q_nbr (columns 0, 1..3, 4..6).
 * The table is ADDED to, never cleared; integer additions only, so its content does not depend on launch geometry or thread count and the
 * device and the twin agree on every element.  nbr_image, `in`, ref_offsets: as lfd_colour_multiview.  table: device u64 [n_refs * k * 7],
 * overlapping nothing of `in`.  One launch on the context's stream, asynchronous; at most one global atomic per (workgroup, reference, slot,
 * quantity).  LFD_ERR_INVALID: a null required pointer, missing cell / slot / rgb, a null image in a valid slot, support_thresh_px <= 0 or not
 * finite, a table overlapping `in`, a capacity beyond 2^31 - 1.  lfd_gain_accumulate_host: the same routine over host pointers on a host
 * context's threads, the same integers.  A host context is served by _host only, a device context refuses _host (LFD_ERR_STATE). */
int lfd_gain_accumulate(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets,
                        const uint8_t* const* nbr_image, float support_thresh_px, uint64_t* table);
int lfd_gain_accumulate_host(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets,
                             const uint8_t* const* nbr_image, float support_thresh_px, uint64_t* table);

/* Per-image exposure gains, the compensation.  The cloud is the concatenation of n_refs references' points, reference r's in
 * [ref_offsets[r], ref_offsets[r + 1]) (i64 [n_refs + 1], clamped to [0, n]); per point i of reference r and channel ch, in f32 with one
 * rounding: rgb_out[3 i + ch] = min(rgb[3 i + ch] * factors[3 r + ch], 1.0f); a value that is not finite is copied bit for bit.  Points at
 * and beyond ref_offsets[n_refs] are not touched.  rgb, rgb_out: f32 [3 * n], rgb_out exactly rgb (in place) or overlapping nothing of it;
 * factors: f32 [n_refs * 3], used as they stand.  All four arrays where the context computes (device memory / host memory for _host).  One
 * launch on the context's stream, asynchronous.  LFD_ERR_INVALID: a null pointer, n outside [0, 2^31 - 1], n_refs <= 0, a partial overlap.
 * LFD_ERR_STATE: the other kind of context. */
int lfd_gain_apply(lfd_context* ctx, const float* rgb, int64_t n, const int64_t* ref_offsets, int32_t n_refs, const float* factors,
                   float* rgb_out);
int lfd_gain_apply_host(lfd_context* ctx, const float* rgb, int64_t n, const int64_t* ref_offsets, int32_t n_refs, const float* factors,
                        float* rgb_out);

/* Far-field shell, the statistics (no upstream counterpart).  Reads the batch only; independent of the point stages.  Per grid cell
 * c of reference r (csrc/lfd_far.hpp, every rounding written out):
 *   d        the f32 world direction of the cell's ray: M (u, v, 1), M = R^T K^-1 of the reference's camera as forward fused chains, (u, v) the
 *            cell's A-coordinate in camera px - warp channels 0 / 1 of slot 0 with four-channel warps, axis_x / axis_y (or the matcher's grid)
 *            with two;
 *   slot s < n_slots[r] is CONFIDENT iff its raw certainty is >= far_certainty (a NaN is not), its observation lies inside the neighbour's grid
 *            (lfd_grid_nearest >= 0 on both axes) and mask_b, where present, is set at the pixel the support filter looks at; it AGREES with
 *            infinity iff lfd_support_filter's comparison, with the homogeneous point (d, 0) in place of (X, 1), holds at far_thresh_px [px of
 *            the neighbour's camera image]: pz > 0 and d2 <= (tau pz)^2, a NaN anywhere rejects;
 *   the cell is FAR iff mask_a, where present, is set at the cell, n_conf >= min(far_min_views, n_slots[r]), n_agree == n_conf, and d is finite
 *            and not zero.
 * A far cell adds to row `key` of table, u64 [6 S S][7], S = shell_cells: in f64 with IEEE division and root, face = 2 m + (d_m < 0), m the
 * index of the largest |d_i| (lowest on ties); (u, v) the two other components, ascending, over |d_m|; cell = floor((u + 1) / 2 S) clamped to
 * [0, S - 1]; key = (face S + cell_v) S + cell_u.  Columns 0..2 += rint(d_i / |d| 2^30) as i64 (two's complement), 3..5 += the reference image's
 * colour at the cell (the dense kernel's f32 four-tap blend, quantised as the writers do), 6 += 1.  counters: NULL or i64 [n_refs], far cells per
 * reference.  Both are ADDED to, never cleared; integer additions only (no-return 64-bit atomics behind a reduction over runs of equal keys
 * inside a wave), so the content does not depend on launch geometry and the device and the twin agree on every element.  A column overflows
 * after 2^33 samples in one direction cell.  One launch on the context's stream, asynchronous.  LFD_ERR_INVALID: a null table, far_thresh_px or
 * far_certainty not finite or <= 0, far_min_views outside [1, 8], shell_cells outside [8, 512], a table or counters overlapping the batch's
 * planes or each other, more than 65535 references.  lfd_far_accumulate_host: the same routines over host pointers on a host context's threads.
 * A host context is served by _host only, a device context refuses _host (LFD_ERR_STATE). */
int lfd_far_accumulate(lfd_context* ctx, const lfd_batch* batch, float far_thresh_px, float far_certainty, int32_t far_min_views,
                       int32_t shell_cells, uint64_t* table, int64_t* counters);
int lfd_far_accumulate_host(lfd_context* ctx, const lfd_batch* batch, float far_thresh_px, float far_certainty, int32_t far_min_views,
                            int32_t shell_cells, uint64_t* table, int64_t* counters);

/* lfd_far_accumulate that also reports WHICH cells were far: flags, u8 [n_refs * H * W] where the context computes (NULL: lfd_far_accumulate
 * itself), is written - not added to - 1 at [r * H * W + cell] for every far cell and 0 elsewhere.  It must overlap neither the table, the
 * counters nor the batch (LFD_ERR_INVALID).  What the driver counts the far cells that also produced a point with. */
int lfd_far_accumulate_flags(lfd_context* ctx, const lfd_batch* batch, float far_thresh_px, float far_certainty, int32_t far_min_views,
                             int32_t shell_cells, uint64_t* table, int64_t* counters, uint8_t* flags);
int lfd_far_accumulate_flags_host(lfd_context* ctx, const lfd_batch* batch, float far_thresh_px, float far_certainty, int32_t far_min_views,
                                  int32_t shell_cells, uint64_t* table, int64_t* counters, uint8_t* flags);

/* Far-field shell, the points.  The direction cells of `table` with count >= min_samples and a non-zero direction sum, in key
 * order; per cell in f64: d_hat = sum / |sum|, xyz = (float)(centre + radius d_hat), rgb = (float)(sum_c / (255 count)), normal = (float)(-d_hat)
 * (NULL: not written), samples = count saturated to i32 (NULL: not written).  table and the outputs where the context computes; centre (f64 [3],
 * finite) and n_out on the host.  Synchronous.  *n_out is the number of cells that qualify; at most `capacity` records are written, and
 * LFD_ERR_CAPACITY is returned when there are more.  LFD_ERR_INVALID: a null required pointer, shell_cells outside [8, 512], min_samples < 1,
 * radius not finite or <= 0, capacity outside [0, 2^31 - 1], outputs overlapping the table or each other. */
int lfd_far_emit(lfd_context* ctx, const uint64_t* table, int32_t shell_cells, int64_t min_samples, const double* centre, double radius,
                 float* xyz, float* rgb, float* normal, int32_t* samples, int64_t capacity, int64_t* n_out);
int lfd_far_emit_host(lfd_context* ctx, const uint64_t* table, int32_t shell_cells, int64_t min_samples, const double* centre, double radius,
                      float* xyz, float* rgb, float* normal, int32_t* samples, int64_t capacity, int64_t* n_out);

/* Epipolar audit: pose health from the matches (no upstream counterpart).  Reads the batch only; independent of the point stages.
 * Per reference r, per grid cell c whose mask_a, where present, is set, and per slot j < n_slots[r] (csrc/lfd_audit.hpp, every rounding
 * written out):
 *   the slot is CONFIDENT exactly as lfd_far_accumulate's is, at audit_certainty: its raw certainty is >= audit_certainty (a NaN is not), its
 *            observation lies inside the neighbour's grid, and mask_b, where present, is set at the pixel the support filter looks at;
 *   (ua, va), (ub, vb)  the match in camera px as the dense kernel forms it, f32: ((x + 1) * 0.5) * (w_match - 1) * sx and so on, the A-coordinate
 *            from warp channels 0 / 1 of slot 0 with four-channel warps, from axis_x / axis_y (or the matcher's grid) with two;
 *   in f64 from the widened f32 values, every product and sum rounded separately, F the pair's fundamental matrix (f32 values):
 *            l_i = (F_3i ua + F_3i+1 va) + F_3i+2,  num = (ub l0 + vb l1) + l2,  n2 = l0 l0 + l1 l1,  num2 = num num;
 *   the sample is USABLE iff num2 and n2 are finite and n2 > 0, else DEGENERATE;
 *   bin      the number of b in 0 .. 62 with num2 >= RN(((b + 1)^2 / 64) n2): no division, no root.  bin b < 63: the observation lies
 *            [b / 8, (b + 1) / 8) px of the NEIGHBOUR's camera image (reproj_thresh's unit) off its epipolar line; bin 63: >= 7.875 px.
 * Row r * k + j of table, u64 [n_refs * k][66]: column 0 += 1 per usable sample, column 1 += 1 per degenerate one, column 2 + bin += 1.  The
 * table is ADDED to, never cleared; rows of slots >= n_slots[r] are not touched.  Integer additions only (an aggregation inside the wave, one
 * table per workgroup, then at most one no-return 64-bit atomic per workgroup, slot and non-zero quantity), so the content does not depend on
 * launch geometry and the device and the twin agree on every element.  best: NULL, or u8 [n_refs * H * W] where the context computes, WRITTEN,
 * not added to: the smallest bin over the cell's usable confident slots, 255 where there is none or mask_a is unset - the best that any
 * confident neighbour says about the cell, in the winning slot's camera px.  One launch on the context's stream, asynchronous.
 * LFD_ERR_INVALID: a null table, audit_certainty not finite or <= 0, a table or best overlapping the batch's planes or each other, more than
 * 65535 references.  lfd_epipolar_audit_host: the same routine over host pointers on a host context's threads.  A host context is served by
 * _host only, a device context refuses _host (LFD_ERR_STATE). */
int lfd_epipolar_audit(lfd_context* ctx, const lfd_batch* batch, float audit_certainty, uint64_t* table, uint8_t* best);
int lfd_epipolar_audit_host(lfd_context* ctx, const lfd_batch* batch, float audit_certainty, uint64_t* table, uint8_t* best);

/* Pose corrections from the matches: the normal equations of one Gauss-Newton step on the epipolar error (no upstream
 * counterpart).  Reads the batch and the uploaded camera table only; batch->fundamental is NOT used (a caller's F says nothing about R and t).
 * Per pair (reference A = ref_cam[r], neighbour B = nbr_cam[r * k + j]), once per launch on the host, in f64 from the table's f32 values with
 * every operation rounded separately:  R = R_B R_A^T,  t = t_B - R t_A,  tn = |t|,  th = t / tn (tn not finite or 0: every sample of the pair
 * is degenerate),  K_A^-1 and K_B^-1 the closed-form inverses the library's own F uses.
 * Per grid cell whose mask_a, where present, is set and per slot that is CONFIDENT exactly as lfd_epipolar_audit's is, at pose_certainty, with
 * (ua, va), (ub, vb) the match in camera px formed as there (csrc/lfd_pose.hpp, f64, IEEE division and root, no contraction):
 *   yA = K_A^-1 (ua, va, 1),  p = R yA,  n = th x p,  l = K_B^-T n,  num = (ub l0 + vb l1) + l2,  d2 = l0 l0 + l1 l1,  d = sqrt(d2),
 *   r = num / d  (the signed distance from the epipolar line in px of B's camera image);
 *   the foot point  ub' = ub - (r l0) / d,  vb' = vb - (r l1) / d,  yB = K_B^-1 (ub', vb', 1);
 *   J[0..2] = (n x yB) / d,  J[3..5] = (p x yB) / d:  the derivative of r with respect to a left twist (omega, tau) of the RELATIVE pose
 *   T_B T_A^-1, tau in units of tn, in px per radian;
 *   DEGENERATE iff num, d2, num num or any later value is not finite, or d2 <= 0, or some |J_i| >= 2^16; otherwise OUTLIER iff
 *   num num >= (c c) d2, c = pose_inlier_px (no division in the decision); otherwise INLIER with Jq_i = rint(8 J_i), rq = rint(1024 r).
 * Row r * k + j of table, i64 [n_refs * k][32], is ADDED to (two's complement), never cleared: column 0 inliers, 1 outliers, 2 degenerate,
 * 3 the sum of rq rq, 4..9 of Jq_i rq, 10..30 of Jq_i Jq_j for i <= j row-major; column 31 and rows of slots >= n_slots[r] are not touched.
 * |Jq| <= 2^19, |rq| <= 2^16 and H W <= 2^24, so a launch adds less than 2^63 to a column.  Integer additions only (sums inside the wave, one
 * table per workgroup, then at most one no-return 64-bit atomic per workgroup, slot and non-zero quantity): the content does not depend on
 * launch geometry, and the device and the twin agree on every element.  One launch on the context's stream, asynchronous.
 * LFD_ERR_INVALID: a null table, pose_certainty not in (0, 3.4e38], pose_inlier_px not in (0, 64], a table overlapping the batch's planes,
 * more than 65535 references, H W > 2^24.  lfd_pose_accumulate_host: the same routine over host pointers on a host context's threads.  A host
 * context is served by _host only, a device context refuses _host (LFD_ERR_STATE). */
int lfd_pose_accumulate(lfd_context* ctx, const lfd_batch* batch, float pose_certainty, float pose_inlier_px, int64_t* table);
int lfd_pose_accumulate_host(lfd_context* ctx, const lfd_batch* batch, float pose_certainty, float pose_inlier_px, int64_t* table);

/* Photo-consistency gate on triangulated points (no upstream counterpart - every other gate is geometric).  The test concerns
 * the MATCH that made a point, not X: xyz is carried along and never read.  Per input point of reference r made by winning slot s on cell
 * (y, x) of the H x W grid (csrc/lfd_photo.hpp, exact integers, every rounding written out):
 *   guard        kept with status 0 where the cell lies outside the grid or s >= n_slots[r] (no address is formed from the cell or the slot)
 *   window       the cells (y + dy, x + dx), |dy|, |dx| <= window_cells (1..3), inside the grid.  A window cell PARTICIPATES iff it is live
 *                in slot s as lfd_support_filter defines it (raw certainty > 0, the mask_b pixel its warp points at non-zero), its
 *                observation (xb, yb) - the last two warp channels of slot s there - is finite and -1 <= xb, yb <= 1, and the reference's
 *                mask_a pixel of the cell is non-zero
 *   samples      reference: the four-tap f32 blend lfd_triangulate_* use, of batch->image[r] at the match pixel of the cell's reference
 *                position (warp channels 0, 1 of a 4-channel warp, else axis_x / axis_y); neighbour: lfd_colour_multiview's sample of
 *                nbr_image[r * k + s] at (xb, yb).  Each channel c, clamped to [0, 1] (NaN -> 0), is quantised as (uint32_t)(c * 4096.0f);
 *                a, b: the sums of the three channels
 *   sums         n, Sa, Sb, Saa, Sbb, Sab over the participating cells; va = n Saa - Sa Sa, vb = n Sbb - Sb Sb, cov = n Sab - Sa Sb in i64
 *   verdict      in this order - status 1, kept: 2 n < (2 window_cells + 1)^2 + 1; status 2, kept: va < n n T or vb < n n T with the
 *                integer T = ceil((min_texture * 12288 / 255)^2) (min_texture: a standard deviation in 8-bit grey levels); status 3, kept:
 *                cov > 0 and (double)cov * (double)cov >= ((double)min_ncc * (double)min_ncc) * ((double)va * (double)vb); status 4, DROPPED
 *                otherwise.  No division and no root takes part: the device and the twin agree on every decision
 * Compaction, `in`, `out`, ref_offsets_in, ref_offsets_out (always written, stays on the device), seg_counts_out (optional), the batch
 * preparation and the two launches behind the gate's own are lfd_support_filter's.  nbr_image and its table: as lfd_colour_multiview.
 * status: NULL or u8 [in->capacity]; ncc: NULL or f32 [in->capacity], (float)(cov / sqrt(va vb)) for status 3 or 4 and NaN otherwise, within
 * one f32 ulp of the twin's (the host divides and takes an IEEE root where the device refines its reciprocal instructions); both hold one
 * value per INPUT point.  counters: NULL or device i64 [5], ADDED to: the number of points per status 0..4.  LFD_ERR_INVALID: what the two
 * siblings refuse, window_cells outside [1, 3], min_ncc outside (0, 1], min_texture negative or not finite, a null image in a valid slot, a
 * null batch->image[r], status / ncc / counters overlapping `in`, `out` or each other; LFD_ERR_CAPACITY: out->capacity < in->capacity.
 * lfd_photo_gate_host: the same routine over host pointers (host images, counters: host i64 [5]) on a host context's threads, the same
 * decisions.  A host context is served by _host only, a device context refuses _host (LFD_ERR_STATE). */
int lfd_photo_gate(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets_in,
                   const uint8_t* const* nbr_image, int32_t window_cells, float min_ncc, float min_texture, const lfd_points* out,
                   int64_t* ref_offsets_out, int32_t* seg_counts_out, uint8_t* status, float* ncc, int64_t* counters);
int lfd_photo_gate_host(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets_in,
                        const uint8_t* const* nbr_image, int32_t window_cells, float min_ncc, float min_texture, const lfd_points* out,
                        int64_t* ref_offsets_out, int32_t* seg_counts_out, uint8_t* status, float* ncc, int64_t* counters);

/* Cross-reference consensus filter on the final cloud (no upstream counterpart - the cloud upstream writes is the plain union of what
 * every reference triangulated on its own).  The cloud is the concatenation of n_refs references' points; a point is kept iff at least min_refs
 * OTHER references own a point within `radius` of it - the fusion rule of multi-view stereo, one level above lfd_support_filter, which only sees
 * the neighbours one reference loaded (csrc/lfd_consensus.hpp, every rounding written out, no FMA):
 *   agree(i, j)  f32: dx = x_i - x_j, dy, dz likewise; d2 = (dx dx + dy dy) + dz dz; r2 = radius radius; d2 <= r2.  Symmetric bit for bit; a NaN
 *                never agrees
 *   c_i          the number of DISTINCT references g != ref(i) that own at least one point agreeing with i, capped at LFD_CONSENSUS_CAP.  A point
 *                with a non-finite coordinate agrees with nothing and vouches for nothing: c = 0, dropped; it takes no part in the min / max and
 *                forms no address
 *   kept         iff c_i >= min_refs.  Neighbours are found through a sorted grid of cells of side 1.000001 radius; neither the kept set nor the
 *                counts depend on it
 * xyz: f32 [n][3]; rgb (f32 [n][3]) and err (f32 [n]) travel along when given (NULL together with their output: not copied).  ref_offsets_host:
 * HOST i64 [n_refs + 1], starts at 0, does not decrease, ends at n; reference g owns the points [off[g], off[g + 1]).  min_refs in
 * 1 .. LFD_CONSENSUS_CAP.  The compaction is stable and copies bit for bit; xyz_out / rgb_out / err_out hold n points.  ref_offsets_out_host
 * (HOST i64 [n_refs + 1]) and *n_out_host are always written; consensus: NULL, or u8 [n], c_i per INPUT point (without it the count stops at
 * min_refs).  Synchronous, deterministic; the workspace belongs to the context and is reused.  LFD_ERR_INVALID: a null required pointer, n < 0 or
 * > 2^31 - 1, n_refs < 1, malformed offsets, a radius that is <= 0 or not finite (or whose f32 square is below 2^-102 or overflows), min_refs out
 * of range, in and out arrays that overlap, and - decided before anything is sorted, message "... key range ..." - a cloud so wide for the radius
 * that an axis has more than 2^30 cells or the linear cell key leaves 63 bits.  n == 0 is valid.  lfd_consensus_filter_host: the same over host
 * pointers on a host context's threads; every output equals the device's bit for bit. */
#define LFD_CONSENSUS_CAP 8
int lfd_consensus_filter(lfd_context* ctx, const float* xyz, const float* rgb, const float* err, int64_t n, const int64_t* ref_offsets_host,
                         int32_t n_refs, float radius, int32_t min_refs, float* xyz_out, float* rgb_out, float* err_out,
                         int64_t* ref_offsets_out_host, uint8_t* consensus, int64_t* n_out_host);
int lfd_consensus_filter_host(lfd_context* ctx, const float* xyz, const float* rgb, const float* err, int64_t n, const int64_t* ref_offsets_host,
                              int32_t n_refs, float radius, int32_t min_refs, float* xyz_out, float* rgb_out, float* err_out,
                              int64_t* ref_offsets_out_host, uint8_t* consensus, int64_t* n_out_host);

/* Connected-component filter on the final cloud (no upstream counterpart): the floater rule that needs no second witness.  The cloud
 * is the concatenation of n_refs references' points, as for lfd_consensus_filter (csrc/lfd_component.hpp):
 *   linked(i, j) iff lfd_consensus_filter's agree(i, j) holds at the same r2 = radius radius - that routine itself: f32, every rounding written
 *                out, symmetric bit for bit, a NaN never agrees
 *   component    a class of the transitive closure of the links.  A point with a non-finite coordinate links to nothing: a component of size 1
 *   size(i)      the number of points in i's component;  label(i): the smallest INPUT index in it
 *   kept         iff size(i) >= min_points.  The kept cloud is the input under that mask, in input order, with the same bits; ref_offsets_out_host
 *                is rebuilt as lfd_consensus_filter rebuilds it
 * The partition does not depend on the order in which links are found, nor on the grid that finds them (lfd_consensus_filter's cells of side
 * 1.000001 radius), so every output is exact: device, twin and an all-pairs reference agree element for element.
 * xyz, rgb, err, ref_offsets_host, the outputs xyz_out / rgb_out / err_out / ref_offsets_out_host / *n_out_host: as for lfd_consensus_filter.
 * min_points in 2 .. 2^31 - 1.  Optional outputs (NULL: not written): size, label: u32 [n] at the point's ORIGINAL index (device pointers for
 * lfd_component_filter); summary_host: HOST i64 [66]: [0] the number of components, [1] the size of the largest, [2 + b] for b = 0 .. 31 the
 * components with 2^b <= size < 2^(b + 1), [34 + b] the points in those components.  Synchronous, deterministic; the workspace belongs to the
 * context and is reused.  LFD_ERR_INVALID: lfd_consensus_filter's refusals of cloud, offsets and radius (the "... key range ..." one included),
 * min_points < 2, any input array overlapping any output array.  n == 0 is valid (the summary is all zero).  The union-find of the device call
 * cannot hang: no loop in it waits for another workgroup's store (csrc/lfd_component.hpp, TERMINATION).  lfd_component_filter_host: the same over
 * host pointers with a sequential union-find on a host context; every output equals the device's bit for bit. */
int lfd_component_filter(lfd_context* ctx, const float* xyz, const float* rgb, const float* err, int64_t n, const int64_t* ref_offsets_host,
                         int32_t n_refs, float radius, int32_t min_points, float* xyz_out, float* rgb_out, float* err_out,
                         int64_t* ref_offsets_out_host, uint32_t* size, uint32_t* label, int64_t* summary_host, int64_t* n_out_host);
int lfd_component_filter_host(lfd_context* ctx, const float* xyz, const float* rgb, const float* err, int64_t n, const int64_t* ref_offsets_host,
                              int32_t n_refs, float radius, int32_t min_points, float* xyz_out, float* rgb_out, float* err_out,
                              int64_t* ref_offsets_out_host, uint32_t* size, uint32_t* label, int64_t* summary_host, int64_t* n_out_host);

/* Free-space filter on the final cloud (no upstream counterpart).  Every reference's own points are a sparse depth map of what it
 * saw; a point of ANOTHER reference that lies in front of that depth map on the same ray cannot exist - the reference looked through it.  The
 * cloud is the concatenation of n_refs references' points (ref_offsets_host as for lfd_consensus_filter); cam_P_host: HOST f32 [n_refs][12], the
 * row-major 3 x 4 projection of each reference (pixels of its image); cam_wh_host: HOST i32 [n_refs][2], its image size w, h; pw x ph: the size of
 * every reference's z-buffer plane (csrc/lfd_freespace.hpp, every rounding written out, no FMA):
 *   projection   f64 from the f32 inputs: p_r = ((P[r][0] x + P[r][1] y) + P[r][2] z) + P[r][3]; u = p_0 / p_2, v = p_1 / p_2; d = (float) p_2;
 *                inside iff p_0, p_1, p_2 finite, p_2 > 0, 0 <= u < w, 0 <= v < h, d finite and > 0;
 *                cx = min(pw - 1, floor((u pw) / w)), cy = min(ph - 1, floor((v ph) / h))
 *   Z_r[cy][cx]  the smallest d over reference r's OWN points inside its own camera, +inf where there are none
 *   test         point i of reference r against every j != r it is inside of, d_i its depth there, over the cells of the 3 x 3 window around its
 *                cell that lie in the plane; for a finite D = Z_j[cell], f32: t = tol D, lo = D - t, hi = D + t.  j SUPPORTS i iff some cell has
 *                lo <= d_i <= hi; else j REFUTES i iff the window has a finite cell and d_i < lo(D_min), D_min its smallest; else j says nothing
 *   dropped      iff v_i >= min_violations and v_i > s_i, the numbers of refuting and supporting references (unsaturated)
 * rgb (f32 [n][3]) and err (f32 [n]) travel along when given (NULL together with their output).  tol in (0, 1), min_violations in 1 .. 255.  The
 * compaction is stable and copies bit for bit; xyz_out / rgb_out / err_out hold n points.  ref_offsets_out_host (HOST i64 [n_refs + 1]) and
 * *n_out_host are always written; violations / supports: each NULL, or u8 [n], min(v_i, 255) / min(s_i, 255) per INPUT point.  Synchronous,
 * deterministic; the workspace (the z-buffers among it, refilled on every call) belongs to the context and is reused.  LFD_ERR_INVALID: a null
 * required pointer or half of an optional pair, n < 0 or > 2^31 - 1, n_refs < 1, malformed offsets, pw, ph, w or h below 1,
 * n_refs pw ph > 2^31 - 1, an entry of P that is not finite, tol outside (0, 1), min_violations out of range, in and out arrays that overlap.
 * n == 0 is valid.  lfd_freespace_filter_host: the same over host pointers on a host context's threads; every output equals the device's bit for
 * bit. */
int lfd_freespace_filter(lfd_context* ctx, const float* xyz, const float* rgb, const float* err, int64_t n, const int64_t* ref_offsets_host,
                         int32_t n_refs, const float* cam_P_host, const int32_t* cam_wh_host, int32_t pw, int32_t ph, float tol,
                         int32_t min_violations, float* xyz_out, float* rgb_out, float* err_out, int64_t* ref_offsets_out_host,
                         uint8_t* violations, uint8_t* supports, int64_t* n_out_host);
int lfd_freespace_filter_host(lfd_context* ctx, const float* xyz, const float* rgb, const float* err, int64_t n, const int64_t* ref_offsets_host,
                              int32_t n_refs, const float* cam_P_host, const int32_t* cam_wh_host, int32_t pw, int32_t ph, float tol,
                              int32_t min_violations, float* xyz_out, float* rgb_out, float* err_out, int64_t* ref_offsets_out_host,
                              uint8_t* violations, uint8_t* supports, int64_t* n_out_host);

/* Depth and normal maps of the final cloud, one per camera (no upstream counterpart).  A point cloud is not watertight: a plain
 * z-buffer shows the back wall through the gaps of the front wall, so a cell is kept only when nothing clearly nearer lies around it.  xyz: f32
 * [n][3]; normals: NULL or f32 [n][3]; cam_P_host / cam_wh_host: HOST f32 [n_cams][12] / i32 [n_cams][2] as for lfd_freespace_filter, whose
 * projection decides "inside", cell and depth d of a point in a camera; all cameras share one pw x ph plane (csrc/lfd_depth.hpp):
 *   key          ((u64) bits(d) << 32) | (u32) i for point i: positive finite f32 order like their bits, so the smallest key is the nearest point,
 *                the lowest index at equal depth; empty is (0x7f800000 << 32) | 0xffffffff
 *   splat        K[c][cell] = the smallest key of the points inside camera c whose cell lies within Chebyshev distance splat_cells (0 .. 3) of
 *                `cell` (the part of the window inside the plane)
 *   visibility   D the depth of K[c][cell], m the smallest finite depth of K[c] within distance window_cells (0 .. 8; 0: every cell with data is
 *                kept) of `cell`; kept iff D <= hi, f32: t = tol m, hi = m + t.  tol in (0, 1)
 *   outputs      depth_out f32 [n_cams][ph][pw]: D, 0 where there is no data or the cell was not kept; index_out: NULL, or i32 of the same shape,
 *                the winner's index, -1 for no data; normal_out: NULL iff normals is NULL, else f32 [n_cams][ph][pw][3], a copy of the winner's
 *                three values, 0 0 0 for no data
 * The result does not depend on the order of the points' arrival.  Cameras are rendered in batches whose u64 planes live in the context's
 * workspace: cams_per_batch cameras when non-zero, else as many as keep them at or below 256 MiB; the outputs do not depend on it.  Synchronous on
 * the context's stream.  n == 0 is valid: every cell is "no data".  LFD_ERR_INVALID: a null required pointer or half of normals / normal_out,
 * n < 0 or > 2^31 - 1, n_cams < 1, pw, ph, w or h below 1, n_cams pw ph > 2^31 - 1, an entry of P that is not finite, splat_cells, window_cells
 * or tol out of range, cams_per_batch < 0, arrays that overlap; nothing is written then.  lfd_render_depth_host: the same over host pointers on a
 * host context's threads, by the definition; every output equals the device's bit for bit. */
int lfd_render_depth(lfd_context* ctx, const float* xyz, int64_t n, const float* normals, const float* cam_P_host, const int32_t* cam_wh_host,
                     int32_t n_cams, int32_t pw, int32_t ph, int32_t splat_cells, int32_t window_cells, float tol, int32_t cams_per_batch,
                     float* depth_out, int32_t* index_out, float* normal_out);
int lfd_render_depth_host(lfd_context* ctx, const float* xyz, int64_t n, const float* normals, const float* cam_P_host, const int32_t* cam_wh_host,
                          int32_t n_cams, int32_t pw, int32_t ph, int32_t splat_cells, int32_t window_cells, float tol, int32_t cams_per_batch,
                          float* depth_out, int32_t* index_out, float* normal_out);

/* Oriented voxel fusion on the final cloud (no upstream counterpart): the merge step behind lfd_estimate_normals.  The points of a
 * voxel are merged per SIDE their normals face, so an occupied voxel gives one oriented point per visible face: 1 or 2 rows.  Grid, keys, voxel
 * order, colour scale and the two data refusals are lfd_voxel_downsample's, word for word.  xyz, normals, rgb: f32 [n][3] (csrc/lfd_fuse.hpp,
 * every rounding written out, no FMA):
 *   usable    a normal whose components are finite and, in f64, (n0 n0 + n1 n1) + n2 n2 > 0
 *   pivot     of a voxel: the usable normal of its point with the lowest input index (a voxel may have none)
 *   side      1 iff the normal is usable and d < 0, d = (n0 p0 + n1 p1) + n2 p2 in f64 (the products are exact); else 0.  Side 0 is never empty
 *   per side  f64 sums from 0.0 over its points in ascending input index: xyz and rgb / s over all of them, N over the usable normals;
 *             xyz_out, rgb_out = (f32)(sum / count); q = (N0 N0 + N1 N1) + N2 N2; normal = (f32)(N_c / sqrt(q)) if q is finite and > 0, else 0
 *   rows      voxels in ascending (k0, k1, k2), side 0 before side 1: V .. 2 V rows for V occupied voxels, never more than n
 * The pivot depends on the input order: one that is a gross outlier can split a voxel into two rows of similar normals (a density blip, not a wrong
 * point).  xyz_out / normals_out / rgb_out hold n rows; count_out: NULL, or u32 [n], the points merged into each row.  *n_rows_host and
 * *n_voxels_host are always written.  Synchronous, deterministic; the workspace belongs to the context and is reused.  On the device the normal's
 * final division goes through a refined reciprocal: its components are within one f32 ulp of the twin's, everything else is equal bit for bit.
 * LFD_ERR_INVALID: a null required pointer, n < 0 or > 2^31 - 1, voxel_size <= 0 or not finite, outputs that overlap inputs or each other, a
 * "non-finite coordinate" in the input, a "key range" whose linear voxel key does not fit 63 bits (both decided before anything is sorted).
 * n == 0 is valid.  lfd_fuse_oriented_host: the same over host pointers on a host context. */
int lfd_fuse_oriented(lfd_context* ctx, const float* xyz, const float* normals, const float* rgb, int64_t n, double voxel_size, float* xyz_out,
                      float* normals_out, float* rgb_out, uint32_t* count_out, int64_t* n_rows_host, int64_t* n_voxels_host);
int lfd_fuse_oriented_host(lfd_context* ctx, const float* xyz, const float* normals, const float* rgb, int64_t n, double voxel_size, float* xyz_out,
                           float* normals_out, float* rgb_out, uint32_t* count_out, int64_t* n_rows_host, int64_t* n_voxels_host);

/* Gaussian-ready output (no upstream counterpart): what a 3DGS trainer computes from a point file before it can start, computed where
 * the cloud is.  lfd_knn_dist2: the mean squared distance of every point to its three nearest neighbours (distCUDA2 of the 3DGS code), EXACT.
 * xyz: f32 [n][3]; dist2_out: f32 [n] (csrc/lfd_knn.hpp, every rounding written out, no FMA):
 *   d2(i, j)   = (dx dx + dy dy) + dz dz in f32 for i != j, taken by INDEX: a duplicate of a point counts with distance 0
 *   dist2[i]   = ((a + b) + c) / 3.0f, a <= b <= c the three smallest d2(i, .), in f32.  Only values enter: ties need no rule
 * The output does not depend on the grid: it equals the brute-force evaluation over all pairs bit for bit, for every cell size, on device and twin.
 * No search cap changes a result: an isolated point gets its true three neighbours.  cell_size: the side of the search grid's cells in scene
 * units, 0 = automatic (from 2 L / ceil(sqrt(n)), L the longest side of the bounding box, divided by 4 while points / occupied cells > 16, at
 * most 8 times and inside the key limits; computed on the host in f64, the same on device and twin); it changes the time a call takes, nothing
 * else.  stats_host: NULL, or f64 [4] = {cell size used, occupied cells, points in the fullest cell, points finished by the brute-force pass}.
 * Synchronous, deterministic; the workspace belongs to the context and is reused.
 * LFD_ERR_INVALID: a null required pointer, n < 0 or > 2^31 - 1, cell_size negative or not finite, dist2_out overlapping xyz, "fewer than four
 * points" for 1 <= n <= 3, a "non-finite coordinate" in the input, a "key range" with more than 2^30 cells along an axis or a linear cell key
 * beyond 63 bits (the last three decided before anything is sorted).  n == 0 is valid.  lfd_knn_dist2_host: the same over host pointers on a host
 * context.
 *
 * lfd_pack_gaussians: out[n*68] = per point 17 f32 LE in the property order of a 3DGS point_cloud.ply at SH degree 0:
 *   x y z nx ny nz   copied bit for bit (normals: lfd_estimate_normals' / lfd_fuse_oriented's f32 [n][3])
 *   f_dc_0..2        (q / 255.0f - 0.5f) / 0.28209479177387814f in f32, q the u8 lfd_pack_ply_normals stores for the colour
 *   opacity          opacity_logit as given (the f32 logit of the initial opacity)
 *   scale_0, scale_1 (f32)(0.5 log((f64) m)), m = max(dist2, 1e-7f), then min(m, (f32) max_scale^2) if max_scale > 0
 *   scale_2          (f32)(0.5 log((f64) m) + log_flatten), log_flatten = log(flatten) <= 0: thinner along the normal
 *   rot_0..3         (w, x, y, z) of the shortest arc from +z onto the normal: (1 + nz, -ny, nx, 0) normalised in f32 (IEEE sqrt and divide);
 *                    (0, 1, 0, 0) where 1 + nz < 2^-23; the identity (1, 0, 0, 0) for a normal that is zero or not finite
 * The device's log is its math library's and its division may not be correctly rounded: the three scales and the four rot values are within one
 * f32 ulp of the twin's, every other column is equal bit for bit.  out must be 4-byte aligned.  Asynchronous on the context's stream.
 * lfd_pack_gaussians_host: the same over host pointers on a host context (synchronous). */
int lfd_knn_dist2(lfd_context* ctx, const float* xyz, int64_t n, double cell_size, float* dist2_out, double* stats_host);
int lfd_knn_dist2_host(lfd_context* ctx, const float* xyz, int64_t n, double cell_size, float* dist2_out, double* stats_host);
int lfd_pack_gaussians(lfd_context* ctx, const float* xyz, const float* normals, const float* rgb, const float* dist2, int64_t n, float opacity_logit,
                       double log_flatten, double max_scale, uint8_t* out);
int lfd_pack_gaussians_host(lfd_context* ctx, const float* xyz, const float* normals, const float* rgb, const float* dist2, int64_t n,
                            float opacity_logit, double log_flatten, double max_scale, uint8_t* out);

/* Spatial point cap (no upstream counterpart - upstream caps by a uniform random draw, which keeps the cloud's density contrast): of n
 * points keep at most `budget`, spread over the occupied space.  xyz: f32 [n][3]; err: f32 [n] or NULL; keep_out: i64 [min(budget, n)], the kept
 * INPUT INDICES in ascending order - the kept cloud is the input under a mask, in input order.  The rule (csrc/lfd_cap.hpp; integers and single
 * IEEE f64 operations, no FMA), exact: device, twin and a reference written from these lines agree element for element.
 *   box        o_c = the f32 minimum per axis; L = the longest side of the bounding box, f64 from the f32 min and max
 *   key        q_c = min(2^21 - 1, floor((((f64) x_c - o_c) / L) * 2^21)) (0 where L = 0); 63-bit Morton interleave, axis 0 the high bit of a triple
 *   cells(l)   the number of distinct key >> 3 (21 - l), l = 0 .. 21
 *   lev        the smallest l with cells(l) >= budget, 21 if there is none; c = cells(lev)
 *   picked     cell k of c in key order iff floor((k + 1) budget / c) > floor(k budget / c): exactly `budget` cells; all cells when c < budget
 *   kept       of a picked cell the point of smallest error by the monotone integer image of its f32 bits (-0 < +0, NaNs by their bits), the
 *              lowest input index on ties and with err NULL
 * *n_keep_host = min(budget, c), or n when n <= budget (every point is kept).  stats_host: NULL, or f64 [4] = {lev, cells(lev), cells(lev - 1)
 * (0 at level 0), L}.  Synchronous, deterministic; the workspace belongs to the context and is reused.
 * LFD_ERR_INVALID: a null required pointer, n < 0 or > 2^31 - 1, budget < 1, keep_out overlapping xyz or err, a "non-finite coordinate" in the input
 * (decided before anything is sorted).  n == 0 is valid.  lfd_cap_spatial_host: the same over host pointers on a host context, whatever its
 * thread count. */
int lfd_cap_spatial(lfd_context* ctx, const float* xyz, const float* err, int64_t n, int64_t budget, int64_t* keep_out, int64_t* n_keep_host,
                    double* stats_host);
int lfd_cap_spatial_host(lfd_context* ctx, const float* xyz, const float* err, int64_t n, int64_t budget, int64_t* keep_out, int64_t* n_keep_host,
                         double* stats_host);

/* Footprint-adaptive thinning (no upstream counterpart): keep at most one point per cell of a linear octree over the cloud, every
 * point at the level that the footprint of its own reference camera selects, so the kept density is constant in that camera's image and not in
 * world space.  xyz: f32 [n][3]; err: f32 [n] or NULL; ref_offsets_host: i64 [n_refs + 1], ascending from 0 to n (point i belongs to the
 * reference r with offsets[r] <= i < offsets[r + 1]); ref_rows_host: f64 [n_refs][5] = r3x r3y r3z t3 (the third row of the reference's
 * world-to-camera [R | t]) and tan_cell (the tangent of one match-grid cell, max(cam_w / (fx grid_w), cam_h / (fy grid_h))); keep_out: i64 [n],
 * the kept INPUT INDICES in ascending order - the kept cloud is the input under a mask, in input order.  The rule (csrc/lfd_thin.hpp; integers
 * and single IEEE f64 operations, no FMA), exact: device, twin and a reference written from these lines agree element for element.
 *   box, key   lfd_cap_spatial's: o_c the f32 minimum per axis, L the longest side, the 63-bit Morton key of 21 bits per axis
 *   depth      z = ((r3x x + r3y y) + r3z z_c) + t3 in f64 from the f32 coordinates
 *   footprint  g = (z tan_cell) thin_cells
 *   level      20 where !(g > 0), g is infinite or !(L > 0); else with q = L / g: 0 where q < 1, else min(the unbiased binary exponent of q, 20) -
 *              the cell side L / 2^level is at least g and, unless clamped, below 2 g
 *   code       (1 << 3 level) | (key >> 3 (21 - level)): unique across levels, below 2^61
 *   kept       of the points of equal code the one of smallest error by the monotone integer image of its f32 bits (-0 < +0, NaNs by their
 *              bits), the lowest input index on ties and with err NULL
 * There is no suppression across levels: a surface seen from two distances keeps a point per cell of each level.
 * *n_keep_host: the number of kept points; ref_offsets_out_host: i64 [n_refs + 1], the offsets of the kept cloud; stats_host: NULL, or f64 [43] =
 * points per level 0 .. 20, cells per level 0 .. 20, L.  Synchronous, deterministic; the workspace belongs to the context and is reused.
 * LFD_ERR_INVALID: a null required pointer, n < 0 or > 2^31 - 1, n_refs < 1, offsets that do not start at 0, end at n or that decrease, thin_cells
 * or a tan_cell that is not finite and > 0, keep_out overlapping xyz or err, a "non-finite coordinate" in the input (decided before anything is
 * sorted).  n == 0 is valid: zero outputs.  lfd_thin_footprint_host: the same over host pointers on a host context, whatever its thread count. */
int lfd_thin_footprint(lfd_context* ctx, const float* xyz, const float* err, int64_t n, const int64_t* ref_offsets_host, int32_t n_refs,
                       const double* ref_rows_host, double thin_cells, int64_t* keep_out, int64_t* n_keep_host, int64_t* ref_offsets_out_host,
                       double* stats_host);
int lfd_thin_footprint_host(lfd_context* ctx, const float* xyz, const float* err, int64_t n, const int64_t* ref_offsets_host, int32_t n_refs,
                            const double* ref_rows_host, double thin_cells, int64_t* keep_out, int64_t* n_keep_host, int64_t* ref_offsets_out_host,
                            double* stats_host);

/* (e) multi-GPU exchange, placement step (no upstream counterpart - upstream has no multi-GPU code): n copies
 * dst[dst_offset .. +nbytes) = src[src_offset .. +nbytes) in ONE launch on `hip_stream` of device `device_index` (offsets and lengths in
 * bytes, no alignment required: 15-byte PLY records).  The overlapped exchange receives every rank's records of a round as one padded block
 * per rank; this puts each reference's records at its place in the ordered cloud (core/distributed.py::OverlappedExchange).  Needs no
 * context; segments must not overlap each other's destination.  Asynchronous. */
typedef struct lfd_copy_segment {
    int64_t src_offset, dst_offset, nbytes;
} lfd_copy_segment;
int lfd_copy_segments(void* hip_stream, int32_t device_index, const void* src, void* dst, const lfd_copy_segment* segs, int32_t n);

/* Debug / test read-back: the f64-widened fundamental matrices the kernels of the LAST prepared batch used, one
 * row-major 3x3 per (reference, slot) pair (n_pairs = n_refs * k of that batch; rows of unused slots are unspecified).
 * Synchronises the stream. */
int lfd_get_pair_fundamental(lfd_context* ctx, int32_t n_pairs, double* F_out_host);

/* ---- N3: image preparation on the device (core/image_utils.py:40-91, core/pipeline.py:163-171) ------------------- */
/* Decoding stays on the host (PIL); the decoded u8 arrays are uploaded and prepared here, bit for bit like Pillow 12:
 * lfd_prepare_image:  dst = Image.resize((w_out, h_out), BILINEAR) of the (h_in, w_in, 3) u8 image src (8-bit two-pass
 *                     fixed-point convolution, horizontal first - vertical first where Pillow's Image.resize does that: an
 *                     image more than 100 times taller than wide that shrinks vertically), then masked pixels black (mask01: device u8 {0,1}
 *                     [h_out*w_out] or NULL) as apply_mask_to_rgb does.  dst: device u8 [h_out*w_out*3].
 * lfd_prepare_mask:   dst01 = load_mask_resized_np after the "L" conversion: Image.resize(NEAREST) of the (h_in, w_in) u8
 *                     mask, then (v / 255 as f32) > threshold, optionally inverted; dst01: device u8 {0,1} [h_out*w_out].
 * Asynchronous on the context's stream (the tables of a new size pair are built on the host and uploaded first). */
int lfd_prepare_image(lfd_context* ctx, const uint8_t* src_rgb, int32_t w_in, int32_t h_in, int32_t w_out, int32_t h_out,
                      const uint8_t* mask01, uint8_t* dst_rgb);
int lfd_prepare_mask(lfd_context* ctx, const uint8_t* src_l, int32_t w_in, int32_t h_in, int32_t w_out, int32_t h_out,
                     float threshold, int32_t invert, uint8_t* dst01);
/* Image undistortion in front of everything else (no upstream counterpart - upstream reads (fx, fy, cx, cy) of a COLMAP camera and
 * ignores the rest).  dst is the pinhole image of the same (fx, fy, cx, cy), width and height: output pixel (i, j) is sent through the camera
 * model and sampled from the photograph src.  COLMAP's SIMPLE_RADIAL, RADIAL, OPENCV and FULL_OPENCV are one formula with the eight
 * coefficients dist = (k1, k2, p1, p2, k3, k4, k5, k6); all in f64, every rounding written out, no FMA (csrc/lfd_undistort.hpp), pixel
 * centres at +0.5:
 *   x = ((j + 0.5) - cx) / fx, y likewise;  r2 = x x + y y;  rad = (((1 + k1 r2) + k2 r4) + k3 r6) / (((1 + k4 r2) + k5 r4) + k6 r6)
 *   xd = (x rad + (2 p1) x y) + p2 (r2 + 2 x x), yd = (y rad + (2 p2) x y) + p1 (r2 + 2 y y);  su = (fx xd + cx) - 0.5, sv likewise
 *   valid  iff -0.5 <= su <= w - 0.5 and -0.5 <= sv <= h - 0.5 (a NaN or an infinity, a zero denominator included, is not)
 *   valid pixels: bilinear blend of the four u8 taps around (su, sv), indices clamped to the image (edge replication inside the half-pixel
 *   border), top = p00 + ax (p01 - p00), bot likewise, val = top + ay (bot - top), out = floor(val + 0.5); with `nearest` (mask planes) the
 *   one tap at floor(su + 0.5), floor(sv + 0.5), clamped.  Invalid pixels: every channel 0.
 * With all-zero coefficients dst equals src byte for byte.  src, dst: u8 [h][w][channels], channels 1 or 3; valid255: NULL, or u8 [h*w],
 * 255 where valid and 0 elsewhere (an "L" mask as it stands); intr = (fx, fy, cx, cy) and dist: HOST f64.  Asynchronous on the context's
 * stream unless n_invalid_host is given: the call then synchronises and reports the number of invalid pixels (counted per wave, one atomic
 * add per workgroup into a counter of the context).  LFD_ERR_INVALID: a null required pointer, w or h < 1 or w*h beyond 2^31 - 1, channels
 * not 1 or 3, fx or fy not finite or <= 0, any other parameter not finite, src / dst / valid255 overlapping; LFD_ERR_STATE: a host context.
 * lfd_host_undistort_image: the same routine over host pointers on the caller's thread; no context, no global state (callable from several
 * threads at once; an error is its return code alone); every output equals the device's byte for byte. */
int lfd_undistort_image(lfd_context* ctx, const uint8_t* src, int32_t w, int32_t h, int32_t channels, int32_t nearest, const double intr[4],
                        const double dist[8], uint8_t* dst, uint8_t* valid255, int64_t* n_invalid_host);
int lfd_host_undistort_image(const uint8_t* src, int32_t w, int32_t h, int32_t channels, int32_t nearest, const double intr[4],
                             const double dist[8], uint8_t* dst, uint8_t* valid255, int64_t* n_invalid_host);
/* host helpers (CPU tests): the resampling tables exactly as the kernels use them. bounds: [out_size*2] = {first, count};
 * kk: [out_size * *ksize_out] 22-bit fixed-point coefficients (LFD_ERR_CAPACITY if kk_capacity is too small, *ksize_out is
 * still set); idx: [out_size] NEAREST source indices. */
int lfd_host_resize_tables(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* kk, int32_t kk_capacity, int32_t* ksize_out);
int lfd_host_nearest_indices(int32_t in_size, int32_t out_size, int32_t* idx);

/* Synchronise the context's stream and report whether the last launches completed normally.
 * *status_out = 0, or 1 when a bounded look-back spin gave up (results invalid; returns LFD_ERR_HIP). */
int lfd_launch_status(lfd_context* ctx, int32_t* status_out);

/* ---- host-side helpers (no GPU needed; used by the CPU test-suite) -------------------------------- */
/* A-grid axis used when axis_x/axis_y are NULL: start + step*j below the midpoint,
 * end - step*(n-1-j) from it on, f32 (the per-element form of torch.linspace, core/matcher.py:132-133). */
int lfd_identity_axis(int32_t n, float* out_host);
/* Largest f32 d with degrees(acosf(d)) >= min_deg: the kernels test `dot <= d` instead of calling
 * acos per cell (core/geometry.py:113-119). */
float lfd_parallax_dot_threshold(float min_deg);
/* F (f32, row-major 9) for one camera pair, the same routine the kernels run in their prologue
 * (core/geometry.py:122-130). */
int lfd_host_fundamental(const float* K1, const float* R1, const float* t1, const float* K2,
                         const float* R2, const float* t2, float* F_out);
/* Smallest right singular vector of a row-major 4x4 f32 matrix, the routine the kernels triangulate with
 * (f64 inverse iteration on A^T A), on the HOST build of the same source; out4 is un-normalised.  Returns the
 * number of solves made (>= 3) or a negative lfd_status.  CPU unit tests compare it with an f64 SVD. */
int lfd_host_null_vector(const float* A16, double* out4);
/* The same for the re-triangulation's solver (lfd_refine_multiview[_weighted], any number of views): the smallest eigenvector of the
 * symmetric 4x4 matrix whose upper triangle is M10 (m00 m01 m02 m03 m11 m12 m13 m22 m23 m33, f64), HOST build; out4 is un-normalised.
 * Returns the number of solves made (>= 3) or a negative lfd_status. */
int lfd_host_null_vector_sym(const double* M10, double* out4);
/* One correspondence through the per-cell routine on the HOST build of the same source (debug /
 * CPU unit tests of the arithmetic; not a fallback: no batch entry point uses it).
 * cam1/cam2: K[9] R[9] t[3] P[12] C[3] w h (as floats, 38 values).  out: x y z r g b err keep. */
int lfd_host_eval_correspondence(const float* cam1, const float* cam2, float xa_norm, float ya_norm,
                                 float xb_norm, float yb_norm, int32_t w_match, int32_t h_match,
                                 const lfd_params* params, float* out8);

/* ---- CPU twin ------------------------------------------------------------------ */
/* The same three steps on the host: EVERY pointer of lfd_batch / lfd_points / the arguments below is a HOST pointer.
 * The per-cell arithmetic is the host build of the very source the kernels compile (csrc/lfd_geometry.hpp; IEEE
 * division / square root where the device uses the 1-ulp v_rcp / v_sqrt), spread over n_threads std::threads
 * (<= 0: all hardware threads).  A host context accepts lfd_upload_cameras, lfd_last_error, lfd_destroy and the
 * *_host calls (the three below, lfd_local_corr_host, lfd_refiner_block_host, lfd_refiner_head_host, lfd_cycle_gate_host, lfd_support_filter_host, lfd_refine_multiview_host, lfd_refine_multiview_weighted_host, lfd_depth_sigma_filter_host, lfd_consensus_filter_host, lfd_freespace_filter_host, lfd_render_depth_host, lfd_fuse_oriented_host, lfd_knn_dist2_host, lfd_pack_gaussians_host, lfd_cap_spatial_host and lfd_photo_gate_host); every device entry point refuses it with LFD_ERR_STATE, and the *_host calls refuse a device
 * context: neither side ever stands in for the other.  Semantics (orders, counts, optional outputs, LFD_ERR_CAPACITY
 * with valid counts) are those of lfd_aggregate / lfd_triangulate_dense / lfd_triangulate_indexed. */
int lfd_create_host(int32_t n_threads, lfd_context** out);
int lfd_host_threads(const lfd_context* ctx); /* threads a host context uses (0 for a device context) */
int lfd_aggregate_host(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params, float* best_cert,
                       uint8_t* best_slot);
int lfd_triangulate_dense_host(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params,
                               const lfd_points* out, int64_t* ref_offsets, int32_t* seg_counts);
int lfd_triangulate_indexed_host(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params,
                                 const int64_t* sel_idx, const int64_t* sel_offsets, const lfd_points* out,
                                 int64_t* ref_offsets, int32_t* seg_counts, int32_t* seg_order);

#ifdef __cplusplus
}
#endif
#endif /* LFD_DENSIFY_H */
