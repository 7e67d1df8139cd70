// Host side of the C-ABI declared in include/lfd_densify.h: context, tables, launches.
// No compute happens on the host here except the tiny helpers the header lists as host-side.
#include <cstddef>
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "lfd_context.hpp"
#include "lfd_corr.hpp"
#include "lfd_block.hpp"
#include "lfd_head.hpp"
#include "lfd_cycle.hpp"
#include "lfd_support.hpp"
#include "lfd_refine.hpp"
#include "lfd_normals.hpp"
#include "lfd_colour.hpp"
#include "lfd_photo.hpp"
#include "lfd_gain.hpp"
#include "lfd_far.hpp"
#include "lfd_audit.hpp"
#include "lfd_pose.hpp"
#include "lfd_sigma.hpp"
#include "lfd_consensus.hpp"
#include "lfd_component.hpp"
#include "lfd_undistort.hpp"
#include "lfd_freespace.hpp"
#include "lfd_depth.hpp"
#include "lfd_fuse.hpp"
#include "lfd_knn.hpp"
#include "lfd_cap.hpp"
#include "lfd_thin.hpp"

extern "C" __global__ void lfd_aggregate_kernel(LfdLaunch L, float* best_cert, uint8_t* best_slot);
extern "C" __global__ void lfd_dense_kernel(LfdLaunch L);
extern "C" __global__ void lfd_dense_exact_kernel(LfdLaunch L);
extern "C" __global__ void lfd_dense_prod_kernel(LfdLaunch L);
extern "C" __global__ void lfd_dense_ply_kernel(LfdLaunch L);
extern "C" __global__ void lfd_dense_ply_exact_kernel(LfdLaunch L);
extern "C" __global__ void lfd_dense_segments_kernel(LfdLaunch L);
extern "C" __global__ void lfd_dense_segments_exact_kernel(LfdLaunch L);
extern "C" __global__ void lfd_dense_ply_segments_kernel(LfdLaunch L);
extern "C" __global__ void lfd_dense_ply_segments_exact_kernel(LfdLaunch L);
extern "C" __global__ void lfd_segment_scan_kernel(const LfdTileSeg* table, int n_tiles, int tiles_per_ref, int n_refs, long long* tile_dst, long long* ref_offsets);
extern "C" __global__ void lfd_order_segments_kernel(const long long* tile_dst, const LfdTileSeg* table, long long hw, int tiles_per_ref, int n_tiles,
                                                     const float* sxyz, const float* srgb, const float* serr, const int* scell, const unsigned char* sslot,
                                                     float* dxyz, float* drgb, float* derr, int* dcell, unsigned char* dslot, long long capacity);
extern "C" __global__ void lfd_pack_ply_segments_kernel(const long long* tile_dst, const LfdTileSeg* table, long long hw, int tiles_per_ref, int n_tiles,
                                                        const float* xyz, const float* rgb, long long capacity, unsigned char* out);
extern "C" __global__ void lfd_pack_points3d_segments_kernel(const long long* tile_dst, const LfdTileSeg* table, long long hw, int tiles_per_ref, int n_tiles,
                                                             const float* xyz, const float* rgb, const float* err, long long capacity,
                                                             unsigned long long id_base, unsigned char* out);
extern "C" __global__ void lfd_pair_setup_kernel(LfdLaunch L, LfdRefConst* ref_out, LfdPairConst* pair_out);
extern "C" __global__ void lfd_select_filter_kernel(LfdSelectArgs A);
extern "C" __global__ void lfd_pack_ply_kernel(const float* xyz, const float* rgb, long long n, unsigned char* out);
extern "C" __global__ void lfd_pack_points3d_kernel(const float* xyz, const float* rgb, const float* err, long long n,
                                                    unsigned long long id_base, unsigned char* out);
extern "C" __global__ void lfd_copy_segments_kernel(LfdCopyArgs A, const unsigned char* src, unsigned char* dst);
extern "C" __global__ void lfd_quantise_rgb_kernel(const float* rgb, long long n3, unsigned char* out);
extern "C" __global__ void lfd_voxel_minmax_kernel(const float* xyz, const float* rgb, long long n, LfdVoxStats* part);
extern "C" __global__ void lfd_voxel_final_kernel(const LfdVoxStats* part, int n_part, LfdVoxStats* out);
extern "C" __global__ void lfd_voxel_keys_kernel(const float* xyz, long long n, double o0, double o1, double o2, double vs, unsigned long long e1,
                                                 unsigned long long e2, unsigned long long* keys, unsigned* idx);
extern "C" __global__ void lfd_voxel_hist_kernel(const unsigned long long* keys, long long n, long long chunk, int shift, unsigned* counts);
extern "C" __global__ void lfd_voxel_scan_kernel(unsigned* v, int m, unsigned* total);
extern "C" __global__ void lfd_voxel_scatter_kernel(const unsigned long long* kin, const unsigned* iin, long long n, long long chunk, int shift,
                                                    const unsigned* counts, unsigned long long* kout, unsigned* iout);
extern "C" __global__ void lfd_voxel_head_count_kernel(const unsigned long long* keys, long long n, long long chunk, unsigned* counts);
extern "C" __global__ void lfd_voxel_head_scatter_kernel(const unsigned long long* keys, long long n, long long chunk, const unsigned* counts,
                                                         unsigned* vstart);
extern "C" __global__ void lfd_voxel_sums_kernel(const float* xyz, const float* rgb, long long n, const unsigned* sorted_idx, const unsigned* vstart,
                                                 const unsigned* nv_p, double cscale, float* xyz_out, float* rgb_out, unsigned* big, unsigned* n_big);
extern "C" __global__ void lfd_voxel_sums_big_kernel(const float* xyz, const float* rgb, long long n, const unsigned* sorted_idx, const unsigned* vstart,
                                                     const unsigned* nv_p, double cscale, const unsigned* big, const unsigned* n_big, float* xyz_out,
                                                     float* rgb_out);
hipError_t lfd_undistort_launch(const LfdUndistortArgs& p, unsigned long long* n_invalid, hipStream_t stream);
extern "C" __global__ void lfd_consensus_minmax_kernel(const float* xyz, long long n, LfdVoxStats* part);
extern "C" __global__ void lfd_consensus_keys_kernel(const float* xyz, long long n, double o0, double o1, double o2, double h, unsigned long long e1,
                                                     unsigned long long e2, unsigned long long sentinel, unsigned long long* keys, unsigned* idx);
extern "C" __global__ void lfd_consensus_gather_kernel(const float* xyz, const unsigned* sorted_idx, const long long* offs, int n_refs, long long n,
                                                       LfdConsensusPt* spt);
extern "C" __global__ void lfd_consensus_count_kernel(const unsigned long long* skey, const LfdConsensusPt* spt, const unsigned* sorted_idx, long long n,
                                                      unsigned long long e1, unsigned long long e2, unsigned long long sentinel, float r2, int min_refs,
                                                      int bound, uint8_t* keep, uint8_t* consensus);
extern "C" __global__ void lfd_consensus_wgcount_kernel(const uint8_t* keep, long long n, unsigned* wg_kept);
extern "C" __global__ void lfd_consensus_offsets_kernel(const long long* offs, int n_refs, const uint8_t* keep, const unsigned* wg_kept, long long* offs_out);
extern "C" __global__ void lfd_consensus_scatter_kernel(const float* xyz, const float* rgb, const float* err, long long n, const uint8_t* keep,
                                                        const unsigned* wg_kept, float* o_xyz, float* o_rgb, float* o_err);
extern "C" __global__ void lfd_component_gather_kernel(const float* xyz, const unsigned* sorted_idx, long long n, LfdComponentPt* spt, uint32_t* parent,
                                                       uint32_t* count, uint32_t* first, unsigned long long* summary);
extern "C" __global__ void lfd_component_link_kernel(const unsigned long long* skey, const LfdComponentPt* spt, long long n, unsigned long long e1,
                                                     unsigned long long e2, unsigned long long sentinel, float r2, uint32_t* parent);
extern "C" __global__ void lfd_component_flatten_kernel(const uint32_t* parent, long long n, uint32_t* root);
extern "C" __global__ void lfd_component_size_kernel(const uint32_t* root, const LfdComponentPt* spt, long long n, int aggregate, uint32_t* count,
                                                     uint32_t* first);
extern "C" __global__ void lfd_component_mark_kernel(const uint32_t* root, const LfdComponentPt* spt, const uint32_t* count, const uint32_t* first,
                                                     long long n, uint32_t min_points, uint8_t* keep, uint32_t* size, uint32_t* label,
                                                     unsigned long long* summary);
extern "C" __global__ void lfd_fuse_side_kernel(const float* normals, long long n, const unsigned* sorted_idx, const unsigned* vstart, const unsigned* nv_p,
                                                uint8_t* flag, unsigned* rows, unsigned* big, unsigned* n_big);
extern "C" __global__ void lfd_fuse_side_big_kernel(const float* normals, long long n, const unsigned* sorted_idx, const unsigned* vstart, const unsigned* nv_p,
                                                    const unsigned* big, const unsigned* n_big, uint8_t* flag, unsigned* rows);
extern "C" __global__ void lfd_fuse_rowsum_kernel(const unsigned* rows, const unsigned* nv_p, long long chunk, unsigned* counts);
extern "C" __global__ void lfd_fuse_rowstart_kernel(unsigned* rows, const unsigned* nv_p, long long chunk, const unsigned* counts);
extern "C" __global__ void lfd_fuse_sums_kernel(const float* xyz, const float* normals, const float* rgb, long long n, const unsigned* sorted_idx,
                                                const unsigned* vstart, const unsigned* nv_p, const uint8_t* flag, const unsigned* rowstart, double cscale,
                                                float* xyz_out, float* normals_out, float* rgb_out, unsigned* count_out);
extern "C" __global__ void lfd_fuse_sums_big_kernel(const float* xyz, const float* normals, const float* rgb, long long n, const unsigned* sorted_idx,
                                                    const unsigned* vstart, const unsigned* nv_p, const uint8_t* flag, const unsigned* rowstart, double cscale,
                                                    const unsigned* big, const unsigned* n_big, float* xyz_out, float* normals_out, float* rgb_out,
                                                    unsigned* count_out);
extern "C" __global__ void lfd_knn_keys_kernel(const float* xyz, long long n, LfdKnnGrid g, unsigned long long* keys, unsigned* idx);
extern "C" __global__ void lfd_knn_cellmax_kernel(const unsigned* vstart, const unsigned* nv_p, long long n, unsigned* max_out);
extern "C" __global__ void lfd_knn_gather_kernel(const float* xyz, const unsigned* sorted_idx, long long n, LfdKnnPt* spt);
extern "C" __global__ void lfd_knn_scan_kernel(const unsigned long long* skey, const LfdKnnPt* spt, long long n, LfdKnnGrid g, float* dist2, unsigned* list,
                                               unsigned* n_list);
extern "C" __global__ void lfd_knn_brute_kernel(const LfdKnnPt* spt, long long n, const unsigned* list, const unsigned* n_list, float* dist2);
extern "C" __global__ void lfd_pack_gaussians_kernel(const float* xyz, const float* normals, const float* rgb, const float* dist2, long long n, float opacity,
                                                     double log_flatten, float max_m, float* out);
extern "C" __global__ void lfd_cap_keys_kernel(const float* xyz, long long n, LfdCapBox box, unsigned long long* keys, unsigned* idx);
extern "C" __global__ void lfd_cap_levels_kernel(const unsigned long long* keys, long long n, unsigned* hist);
extern "C" __global__ void lfd_cap_coarsen_kernel(unsigned long long* keys, long long n, int shift);
extern "C" __global__ void lfd_cap_rep_kernel(const unsigned* sorted_idx, const unsigned* vstart, const unsigned* nc_p, const float* err, long long n,
                                              unsigned long long budget, unsigned long long* rep);
extern "C" __global__ void lfd_cap_mark_kernel(const unsigned long long* rep, const unsigned* nc_p, long long n, unsigned long long budget, uint8_t* keep);
extern "C" __global__ void lfd_cap_index_kernel(const uint8_t* keep, const unsigned* wg_kept, long long n, long long capacity, long long* keep_out);
extern "C" __global__ void lfd_thin_keys_kernel(const float* xyz, long long n, const long long* offs, int n_refs, const double* rows, double thin_cells,
                                                LfdCapBox box, unsigned long long* keys, unsigned* idx, unsigned* hist);
extern "C" __global__ void lfd_thin_cells_kernel(const unsigned long long* keys, const unsigned* vstart, const unsigned* nc_p, long long n, unsigned* hist);
extern "C" __global__ void lfd_freespace_fill_kernel(uint32_t* zbuf, long long n_words);
extern "C" __global__ void lfd_freespace_splat_kernel(const float* xyz, long long n, const long long* offs, int n_refs, const LfdFreespaceCam* cams, int pw,
                                                      int ph, uint32_t* zbuf);
extern "C" __global__ void lfd_freespace_count_kernel(const float* xyz, long long n, const long long* offs, int n_refs, const LfdFreespaceCam* cams,
                                                      const uint32_t* zbuf, int pw, int ph, float tol, int min_violations, uint8_t* keep,
                                                      uint8_t* violations, uint8_t* supports);
extern "C" __global__ void lfd_depth_fill_kernel(unsigned long long* keys, long long n_words);
extern "C" __global__ void lfd_depth_splat_kernel(const float* xyz, long long n, const LfdFreespaceCam* cams, int n_batch, int pw, int ph,
                                                  unsigned long long* keys);
extern "C" __global__ void lfd_depth_resolve_kernel(const unsigned long long* keys, int pw, int ph, int tiles_x, int tiles_y, int r, int R, float tol,
                                                    const float* normals, float* depth_out, int* index_out, float* normal_out);
hipError_t lfd_corr_launch(const LfdCorrArgs& p, hipStream_t stream);     // lfd_corr.hip
hipError_t lfd_block_launch(const LfdBlockArgs& p, hipStream_t stream);   // lfd_block.hip
hipError_t lfd_head_launch(const LfdHeadArgs& p, hipStream_t stream);     // lfd_head.hip
hipError_t lfd_cycle_launch(const LfdCycleArgs& p, hipStream_t stream);   // lfd_cycle.hip
hipError_t lfd_support_launch(const LfdSupportArgs& p, const LfdCompactArgs& tail, hipStream_t stream);   // lfd_support.hip
hipError_t lfd_refine_launch(const LfdRefineArgs& p, hipStream_t stream);     // lfd_refine.hip
hipError_t lfd_sigma_launch(const LfdSigmaArgs& p, const LfdCompactArgs& tail, hipStream_t stream);   // lfd_sigma.hip
hipError_t lfd_normals_launch(const LfdNormalArgs& p, hipStream_t stream);    // lfd_normals.hip
hipError_t lfd_colour_launch(const LfdColourArgs& p, hipStream_t stream);     // lfd_colour.hip
hipError_t lfd_photo_launch(const LfdPhotoArgs& p, const LfdCompactArgs& tail, hipStream_t stream);   // lfd_photo.hip
hipError_t lfd_gain_launch(const LfdGainArgs& p, hipStream_t stream);         // lfd_gain.hip
hipError_t lfd_gain_apply_launch(const LfdGainApplyArgs& p, hipStream_t stream);
hipError_t lfd_far_launch(const LfdFarArgs& p, bool reduce, hipStream_t stream);   // lfd_far.hip
hipError_t lfd_far_mark_launch(const unsigned long long* table, long long n_cells, long long min_samples, uint8_t* keep, hipStream_t stream);
hipError_t lfd_far_emit_launch(const LfdFarEmitArgs& p, hipStream_t stream);
hipError_t lfd_audit_launch(const LfdAuditArgs& p, bool aggregate, hipStream_t stream);   // lfd_audit.hip
hipError_t lfd_pose_launch(const LfdPoseArgs& p, hipStream_t stream);   // lfd_pose.hip
extern "C" __global__ void lfd_pack_ply_normals_kernel(const float* xyz, const float* normals, const float* rgb, long long n, unsigned char* out);
extern "C" __global__ void lfd_select_topm_kernel(LfdSelectArgs A);
extern "C" __global__ void lfd_select_filter_mw_kernel(LfdSelectArgs A, LfdSelectNorms norms);
extern "C" __global__ void lfd_select_begins_kernel(long long* pairs, long long stride, int n);
extern "C" __global__ void lfd_mt_seed_kernel(unsigned* mt, unsigned seed);
extern "C" __global__ void lfd_mt_seed_batch_kernel(unsigned* mt_base, LfdSeedBatch seeds);
extern "C" __global__ void lfd_indexed_eval_kernel(LfdLaunch L, const long long* sel_idx, const long long* sel_offsets, float* scratch,
                                                   uint8_t* codes, unsigned* tab, int off_pairs);
extern "C" __global__ void lfd_indexed_kernel(LfdLaunch L, const long long* sel_idx, const long long* sel_offsets,
                                              float* scratch, uint8_t* codes, int32_t* seg_order, const unsigned* tab, int off_pairs);

namespace {

// the one piece of process-wide state: the message of the last lfd_create() that failed (there is no context to hold it).
// Written under a mutex; lfd_last_error(NULL) hands out a per-thread copy, so concurrent creators cannot tear it.
std::mutex g_create_mutex;
std::string g_create_error;
thread_local std::string t_create_error_copy;

}  // namespace

namespace {

int fail(lfd_context* ctx, int code, const std::string& msg) { return lfd_fail(ctx, code, msg); }

#define LFD_HIP(ctx, expr)                                                                         \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail((ctx), LFD_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));    \
    } while (0)

int ensure(lfd_context* ctx, DeviceBuffer& b, size_t bytes, bool zero = false) {
    if (b.bytes >= bytes && b.ptr) return LFD_OK;
    if (b.ptr) {
        LFD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->prep_stream) LFD_HIP(ctx, hipStreamSynchronize(ctx->prep_stream));
        LFD_HIP(ctx, hipFree(b.ptr));
        b.ptr = nullptr; b.bytes = 0;
    }
    size_t want = std::max<size_t>(bytes, 256);
    want = (want + 255) & ~size_t(255);
    LFD_HIP(ctx, hipMalloc(&b.ptr, want));
    b.bytes = want;
    if (zero) LFD_HIP(ctx, hipMemsetAsync(b.ptr, 0, want, ctx->stream));
    return LFD_OK;
}

int validate_batch(lfd_context* ctx, const lfd_batch* b, const lfd_params* p) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "this context was made by lfd_create_host: it serves the *_host entry points only");
    if (!b || !p) return fail(ctx, LFD_ERR_INVALID, "null batch/params");
    if (ctx->n_cams <= 0) return fail(ctx, LFD_ERR_STATE, "lfd_upload_cameras must be called first");
    if (b->n_refs <= 0) return fail(ctx, LFD_ERR_INVALID, "n_refs must be > 0");
    if (b->k <= 0 || b->k > LFD_MAX_SLOTS) return fail(ctx, LFD_ERR_INVALID, "k must be in [1, LFD_MAX_SLOTS]");
    if (b->H <= 0 || b->W <= 0 || b->w_match <= 1 || b->h_match <= 1) return fail(ctx, LFD_ERR_INVALID, "bad grid / match size");
    // byte offsets into the match-size image are 32-bit, its rows and columns 24-bit multiplicands (lfd_bilinear_fetch)
    if (b->w_match >= (1 << 24) || b->h_match >= (1 << 24) || (long long)b->w_match * b->h_match * 3 > 0x7fffffffLL)
        return fail(ctx, LFD_ERR_INVALID, "match-size image too large");
    if ((long long)b->H * b->W > 0x7fffffffLL) return fail(ctx, LFD_ERR_INVALID, "grid too large");
    if (b->warp_channels != 2 && b->warp_channels != 4) return fail(ctx, LFD_ERR_INVALID, "warp_channels must be 2 or 4");
    if (!b->ref_cam || !b->n_slots || !b->nbr_cam || !b->cert || !b->warp || !b->image)
        return fail(ctx, LFD_ERR_INVALID, "null table in batch");
    if ((b->axis_x == nullptr) != (b->axis_y == nullptr)) return fail(ctx, LFD_ERR_INVALID, "axis_x and axis_y must both be given or both be null");
    for (int r = 0; r < b->n_refs; ++r) {
        if (b->ref_cam[r] < 0 || b->ref_cam[r] >= ctx->n_cams) return fail(ctx, LFD_ERR_INVALID, "ref_cam out of range");
        if (b->n_slots[r] < 1 || b->n_slots[r] > b->k) return fail(ctx, LFD_ERR_INVALID, "n_slots must be in [1, k]");
        if (!b->image[r]) return fail(ctx, LFD_ERR_INVALID, "null image pointer");
        for (int j = 0; j < b->n_slots[r]; ++j) {
            const size_t s = (size_t)r * b->k + j;
            if (b->nbr_cam[s] < 0 || b->nbr_cam[s] >= ctx->n_cams) return fail(ctx, LFD_ERR_INVALID, "nbr_cam out of range");
            if (!b->cert[s] || !b->warp[s]) return fail(ctx, LFD_ERR_INVALID, "null cert/warp pointer in a valid slot");
            if ((reinterpret_cast<uintptr_t>(b->cert[s]) & 15u) || (reinterpret_cast<uintptr_t>(b->warp[s]) & 15u))
                return fail(ctx, LFD_ERR_INVALID, "cert/warp planes must be 16-byte aligned");
        }
    }
    return LFD_OK;
}

// The events of this file order work on ONE device; none of them publishes device writes to the host, so none needs the release to system
// scope that an event carries by default (after the dense kernel: behind 400 MB of stores).  A host read of results goes through a copy or a
// stream synchronisation of the caller's, which release on their own.
constexpr unsigned kOrderOnly = hipEventDisableTiming | hipEventDisableSystemFence;

int slot_events(lfd_context* ctx, LfdBatchSlot& sl) {
    // pinned_free: the host waits on it (hipEventSynchronize) before it overwrites `pinned`, host memory the device only READS
    if (!sl.pinned_free) LFD_HIP(ctx, hipEventCreateWithFlags(&sl.pinned_free, kOrderOnly));
    // ready: the launch stream waits on it (hipStreamWaitEvent) and then reads the tables and constants the preparation stream wrote - same device
    if (!sl.ready) LFD_HIP(ctx, hipEventCreateWithFlags(&sl.ready, kOrderOnly));
    // idle: the preparation stream waits on it (hipStreamWaitEvent) before it OVERWRITES the slot's tables - same device, nothing is read
    if (!sl.idle) LFD_HIP(ctx, hipEventCreateWithFlags(&sl.idle, kOrderOnly));
    return LFD_OK;
}

// Build refs|slots|fundamental matrices into one blob and find it a slot: a slot that already holds these tables is reused as it is;
// otherwise the blob is uploaded - by a launch into the slot of the last launch, on the launch stream (stream order protects the kernels
// still reading it); by lfd_prepare_batch (`ahead`) into the OTHER slot, on the preparation stream, behind the event that marks the end
// of that slot's last user - so that it runs beside the kernels of the batch before it.
// `extra` (the selection offsets of lfd_triangulate_indexed) is NOT part of what is cached and compared: it sits behind the tables and
// is uploaded on its own, on the launch stream, by the launch that brings it - so a batch staged by lfd_prepare_batch serves the indexed
// entry point as well (round 3 kept the offsets inside the blob: a staged batch then never matched).
int upload_tables(lfd_context* ctx, const lfd_batch* b, const long long* extra, size_t n_extra, bool ahead, int* slot_out, hipStream_t* stream_out,
                  const LfdRefDesc** d_refs, const LfdSlotDesc** d_slots, const long long** d_extra, const float** d_fund) {
    const size_t nr = (size_t)b->n_refs, ns = nr * (size_t)b->k;
    const size_t off_slots = (nr * sizeof(LfdRefDesc) + 15) & ~size_t(15);
    const size_t off_fund = (off_slots + ns * sizeof(LfdSlotDesc) + 15) & ~size_t(15);
    const size_t total = (off_fund + (b->fundamental ? ns * 9 * sizeof(float) : 0) + 15) & ~size_t(15);       // what is cached
    const size_t off_extra = total;
    const size_t extra_room = ((nr + 1) * sizeof(long long) + 15) & ~size_t(15);                              // always reserved: [n_refs + 1] offsets
    std::vector<unsigned char> blob(total, 0);
    LfdRefDesc* refs = reinterpret_cast<LfdRefDesc*>(blob.data());
    LfdSlotDesc* slots = reinterpret_cast<LfdSlotDesc*>(blob.data() + off_slots);
    for (size_t r = 0; r < nr; ++r) {
        refs[r].image = b->image[r];
        refs[r].mask_a = b->mask_a ? b->mask_a[r] : nullptr;
        refs[r].cam = b->ref_cam[r];
        refs[r].n_slots = b->n_slots[r];
        refs[r].any_mask = refs[r].mask_a ? 1 : 0;
        refs[r].pad = 0;
        for (int j = 0; j < b->k; ++j) {
            LfdSlotDesc& s = slots[r * b->k + j];
            const bool valid = j < b->n_slots[r];
            s.cert = valid ? b->cert[r * b->k + j] : nullptr;
            s.warp = valid ? b->warp[r * b->k + j] : nullptr;
            s.mask_b = (valid && b->mask_b) ? b->mask_b[r * b->k + j] : nullptr;
            s.cam = valid ? b->nbr_cam[r * b->k + j] : 0;
            s.pad = 0;
            if (s.mask_b) refs[r].any_mask = 1;
        }
    }
    if (b->fundamental) std::memcpy(blob.data() + off_fund, b->fundamental, ns * 9 * sizeof(float));
    if (n_extra * sizeof(long long) > extra_room) return fail(ctx, LFD_ERR_INVALID, "internal: selection offsets beyond the reserved room");

    int si = -1;
    for (int c = 0; c < 2; ++c) {
        const int i = c == 0 ? ctx->cur : 1 - ctx->cur;
        if (ctx->slot[i].desc.ptr && ctx->slot[i].cache == blob) { si = i; break; }
    }
    hipStream_t st = ctx->stream;
    if (si >= 0) {                                   // the tables are (or are about to be) in place
        LfdBatchSlot& sl = ctx->slot[si];
        if (!ahead && sl.ready_pending) {            // staged ahead on the preparation stream: the launch stream waits for that, once
#if !defined(LFD_EXPERIMENT_NO_READY_WAIT)           // (measurement only, UNSAFE: what the wait packet costs a step - profiles/r4/ab_ready_wait.txt)
            LFD_HIP(ctx, hipStreamWaitEvent(ctx->stream, sl.ready, 0));
#endif
            sl.ready_pending = false;
        }
        if (ahead && sl.ready_pending) st = ctx->prep_stream;      // (a second lfd_prepare_batch of the same batch: stay behind the first)
    } else {
        if (ahead) {
            if (!ctx->prep_stream) LFD_HIP(ctx, hipStreamCreateWithFlags(&ctx->prep_stream, hipStreamNonBlocking));
            si = ctx->last_used < 0 ? ctx->cur : 1 - ctx->cur;
            st = ctx->prep_stream;
        } else {
            si = ctx->cur;
        }
        LfdBatchSlot& sl = ctx->slot[si];
        int rc = slot_events(ctx, sl);
        if (rc != LFD_OK) return rc;
        if (ahead) {
            // the kernels of this slot's last user must be through (the event sits where the launch after it began), and so must
            // whatever a launch issued for the slot in the launch stream since (si == cur only before the first launch)
            if (sl.used) LFD_HIP(ctx, hipStreamWaitEvent(st, sl.idle_attached ? sl.idle_ext : sl.idle, 0));
        } else if (sl.ready_pending) {               // an unused staging of another batch is still on its way into this slot
            LFD_HIP(ctx, hipStreamWaitEvent(ctx->stream, sl.ready, 0));
            sl.ready_pending = false;
        }
        rc = ensure(ctx, sl.desc, total + extra_room);
        if (rc != LFD_OK) return rc;
        if (sl.pinned_bytes < total + extra_room) {
            if (sl.pinned_in_flight) { LFD_HIP(ctx, hipEventSynchronize(sl.pinned_free)); sl.pinned_in_flight = false; }
            if (sl.pinned) LFD_HIP(ctx, hipHostFree(sl.pinned));
            sl.pinned = nullptr;
            sl.pinned_bytes = std::max<size_t>((total + extra_room) * 2, 1 << 16);
            LFD_HIP(ctx, hipHostMalloc(&sl.pinned, sl.pinned_bytes, hipHostMallocDefault));
        }
        if (sl.pinned_in_flight) { LFD_HIP(ctx, hipEventSynchronize(sl.pinned_free)); sl.pinned_in_flight = false; }
        std::memcpy(sl.pinned, blob.data(), total);
        LFD_HIP(ctx, hipMemcpyAsync(sl.desc.ptr, sl.pinned, total, hipMemcpyHostToDevice, st));
        LFD_HIP(ctx, hipEventRecord(sl.pinned_free, st));
        sl.pinned_in_flight = true;
        sl.cache.swap(blob);
        sl.consts_valid = false;
    }
    LfdBatchSlot& sl = ctx->slot[si];
    if (n_extra) {
        // this launch's selection offsets, behind the tables: a few dozen bytes, on the launch stream (the launch that reads them follows
        // in the same stream; an earlier launch that read the previous offsets precedes the copy in it)
        if (sl.desc.bytes < total + extra_room) return fail(ctx, LFD_ERR_STATE, "internal: batch slot without room for the selection offsets");
        if (sl.x_in_flight) { LFD_HIP(ctx, hipEventSynchronize(sl.x_free)); sl.x_in_flight = false; }      // (the previous indexed launch into this slot: long through)
        if (sl.pinned_x_bytes < extra_room) {
            if (sl.pinned_x) LFD_HIP(ctx, hipHostFree(sl.pinned_x));
            sl.pinned_x = nullptr;
            sl.pinned_x_bytes = std::max<size_t>(extra_room * 2, 4096);
            LFD_HIP(ctx, hipHostMalloc(&sl.pinned_x, sl.pinned_x_bytes, hipHostMallocDefault));
        }
        // x_free: the host waits on it before it overwrites `pinned_x`, host memory the device only reads
        if (!sl.x_free) LFD_HIP(ctx, hipEventCreateWithFlags(&sl.x_free, kOrderOnly));
        std::memcpy(sl.pinned_x, extra, n_extra * sizeof(long long));
        LFD_HIP(ctx, hipMemcpyAsync(static_cast<unsigned char*>(sl.desc.ptr) + off_extra, sl.pinned_x, n_extra * sizeof(long long), hipMemcpyHostToDevice,
                                    ctx->stream));
        LFD_HIP(ctx, hipEventRecord(sl.x_free, ctx->stream));
        sl.x_in_flight = true;
    }
    *slot_out = si;
    *stream_out = st;
    *d_refs = reinterpret_cast<const LfdRefDesc*>(sl.desc.ptr);
    *d_slots = reinterpret_cast<const LfdSlotDesc*>(static_cast<unsigned char*>(sl.desc.ptr) + off_slots);
    if (d_extra) *d_extra = reinterpret_cast<const long long*>(static_cast<unsigned char*>(sl.desc.ptr) + off_extra);
    *d_fund = b->fundamental ? reinterpret_cast<const float*>(static_cast<unsigned char*>(sl.desc.ptr) + off_fund) : nullptr;
    return LFD_OK;
}

int default_axes(lfd_context* ctx, int W, int H, const float** ax, const float** ay) {
    if (ctx->axes_w != W || ctx->axes_h != H || !ctx->axes.ptr) {
        int rc = ensure(ctx, ctx->axes, sizeof(float) * (size_t)(W + H));
        if (rc != LFD_OK) return rc;
        std::vector<float> host((size_t)W + H);
        lfd_identity_axis(W, host.data());
        lfd_identity_axis(H, host.data() + W);
        LFD_HIP(ctx, hipMemcpyAsync(ctx->axes.ptr, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        LFD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->axes_w = W; ctx->axes_h = H;
    }
    *ax = static_cast<const float*>(ctx->axes.ptr);
    *ay = *ax + W;
    return LFD_OK;
}

// dense mode's colour tables for the analytic A-grid (lfd_geometry.hpp): built on the host with the per-cell arithmetic itself,
// once per (grid, match size)
int colour_tables(lfd_context* ctx, int W, int H, int wm, int hm, const LfdColourCol** cols, const LfdColourRow** rows) {
    const int key[4] = {W, H, wm, hm};
    if (!ctx->colour_tab.ptr || std::memcmp(key, ctx->colour_key, sizeof(key)) != 0) {
        static_assert(sizeof(LfdColourCol) == 16 && sizeof(LfdColourRow) == 16, "colour table entries are 16 bytes");
        int rc = ensure(ctx, ctx->colour_tab, sizeof(LfdColourCol) * (size_t)W + sizeof(LfdColourRow) * (size_t)H);
        if (rc != LFD_OK) return rc;
        std::vector<unsigned char> host(sizeof(LfdColourCol) * (size_t)W + sizeof(LfdColourRow) * (size_t)H);
        LfdColourCol* hc = reinterpret_cast<LfdColourCol*>(host.data());
        LfdColourRow* hr = reinterpret_cast<LfdColourRow*>(host.data() + sizeof(LfdColourCol) * (size_t)W);
        const LfdAxis ax = lfd_make_axis(W), ay = lfd_make_axis(H);
        for (int x = 0; x < W; ++x) hc[x] = lfd_colour_col(lfd_match_px(lfd_axis_value(ax, x), (float)(wm - 1)), wm);
        for (int y = 0; y < H; ++y) hr[y] = lfd_colour_row(lfd_match_px(lfd_axis_value(ay, y), (float)(hm - 1)), wm, hm);
        LFD_HIP(ctx, hipMemcpyAsync(ctx->colour_tab.ptr, host.data(), host.size(), hipMemcpyHostToDevice, ctx->stream));
        LFD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        std::memcpy(ctx->colour_key, key, sizeof(key));
    }
    *cols = static_cast<const LfdColourCol*>(ctx->colour_tab.ptr);
    *rows = reinterpret_cast<const LfdColourRow*>(static_cast<const unsigned char*>(ctx->colour_tab.ptr) + sizeof(LfdColourCol) * (size_t)W);
    return LFD_OK;
}

}  // namespace

void lfd_fill_kernel_params(const lfd_batch* b, const lfd_params* p, LfdKernelParams& kp) {
    kp.sampson_thresh = p->sampson_thresh;
    kp.certainty_thresh = p->certainty_thresh;
    kp.reproj_thresh = p->reproj_thresh;
    kp.no_filter = p->no_filter ? 1 : 0;
    (void)LFD_FLAG_EXACT_COLOUR;     // consumed by lfd_triangulate_dense (kernel choice), not by the per-cell routine
    kp.use_sampson = (!p->no_filter && p->sampson_thresh > 0.0) ? 1 : 0;
    kp.use_parallax = (!p->no_filter && p->min_parallax_deg > 0.0f) ? 1 : 0;
    kp.dot_thresh = kp.use_parallax ? lfd_parallax_dot_threshold(p->min_parallax_deg) : 2.0f;
    kp.wm1 = (float)(b->w_match - 1);
    kp.hm1 = (float)(b->h_match - 1);
}

namespace {

int prepare_launch(lfd_context* ctx, const lfd_batch* b, const lfd_params* p, const long long* extra, size_t n_extra,
                   LfdLaunch& L, const long long** d_extra, bool ahead = false) {
    int rc = validate_batch(ctx, b, p);
    if (rc != LFD_OK) return rc;
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    std::memset(&L, 0, sizeof(L));
    if (!ahead && ctx->last_used >= 0) {
        // the kernels of the previous launch end here in the launch stream: from this point on its slot may be refilled ahead
        LfdBatchSlot& prev = ctx->slot[ctx->last_used];
        rc = slot_events(ctx, prev);
        if (rc != LFD_OK) return rc;
        if (!prev.idle_attached) LFD_HIP(ctx, hipEventRecord(prev.idle, ctx->stream));     // (a dense launch carried its own marker)
        prev.used = true;
    }
    int si = 0;
    hipStream_t st = ctx->stream;
    rc = upload_tables(ctx, b, extra, n_extra, ahead, &si, &st, &L.refs, &L.slots, d_extra, &L.fund_override);
    if (rc != LFD_OK) return rc;
    LfdBatchSlot& sl = ctx->slot[si];
    L.cams = static_cast<const LfdCam*>(ctx->cams.ptr);
    if (b->axis_x) { L.axis_x = b->axis_x; L.axis_y = b->axis_y; }
    else {
        rc = default_axes(ctx, b->W, b->H, &L.axis_x, &L.axis_y);
        if (rc != LFD_OK) return rc;
        L.axis_identity = 1;
    }
    L.ax = lfd_make_axis(b->W);
    L.ay = lfd_make_axis(b->H);
    L.n_refs = b->n_refs; L.k = b->k; L.H = b->H; L.W = b->W;
    L.w_match = b->w_match; L.h_match = b->h_match; L.warp_channels = b->warp_channels;
    const long long HW = (long long)b->H * b->W;
    const int tile = LFD_DENSE_BLOCK * LFD_DENSE_CPT;
    L.tiles_per_ref = (int)((HW + tile - 1) / tile);
    L.mask_sx = (float)b->w_match / (float)b->W;
    L.mask_sy = (float)b->h_match / (float)b->H;
    L.inv_w = 1.0f / (float)b->W;
    L.w_log2 = -1;
    if ((b->W & (b->W - 1)) == 0) { int l = 0; while ((1 << l) < b->W) ++l; L.w_log2 = l; }
    lfd_fill_kernel_params(b, p, L.kp);
    // per-pair constants: (re)derive when the batch tables, the cameras or the match size changed
    const size_t ref_bytes = ((size_t)b->n_refs * sizeof(LfdRefConst) + 15) & ~size_t(15);
    const size_t need = ref_bytes + (size_t)b->n_refs * b->k * sizeof(LfdPairConst);
    if (sl.consts.bytes < need) sl.consts_valid = false;
    rc = ensure(ctx, sl.consts, need);
    if (rc != LFD_OK) return rc;
    LfdRefConst* d_rc = static_cast<LfdRefConst*>(sl.consts.ptr);
    LfdPairConst* d_pc = reinterpret_cast<LfdPairConst*>(static_cast<unsigned char*>(sl.consts.ptr) + ref_bytes);
    L.ref_const = d_rc;
    L.pair_const = d_pc;
    if (!sl.consts_valid || sl.wm != b->w_match || sl.hm != b->h_match) {
        const int n = b->n_refs * b->k + b->n_refs;
        hipLaunchKernelGGL(lfd_pair_setup_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, L, d_rc, d_pc);
        LFD_HIP(ctx, hipGetLastError());
        sl.consts_valid = true;
        sl.refs = b->n_refs; sl.k = b->k;
        sl.wm = b->w_match;
        sl.hm = b->h_match;
        if (st != ctx->stream) {                 // issued ahead: the launch that uses the slot waits for this
            LFD_HIP(ctx, hipEventRecord(sl.ready, st));
            sl.ready_pending = true;
        }
    }
    if (!ahead) {
        ctx->cur = si; ctx->last_used = si;
        sl.idle_attached = false;          // this launch becomes the slot's last user: its end is marked by the launch itself or by the next one
    }
    return LFD_OK;
}

// ticket counter + tile states.  Tickets are never reset: each launch is given the value the
// counter holds when it starts; tile-state words carry a launch epoch, so stale words of earlier
// launches read as "empty" and no per-launch memset is needed.
// workspace: [0] u64 ticket counter, [8] u32 launch status, [16..] tile states
// workspace: [0] u64 ticket counter (indexed kernel), [8] u32 launch status, [16] u32 seg_ready, [128 + 128*s] u64 ticket counter of
// sequence s (dense kernel), [kWsHeader..] tile states
constexpr size_t kWsHeader = 128 + 128 * LFD_TICKET_LANES;

int prepare_lookback(lfd_context* ctx, size_t n_tiles, size_t n_tickets, bool lanes, LfdLaunch& L) {
    const size_t need = kWsHeader + n_tiles * sizeof(unsigned long long);
    const bool fresh = ctx->ws.bytes < need || !ctx->ws.ptr;
    int rc = ensure(ctx, ctx->ws, need, true);
    if (rc != LFD_OK) return rc;
    if (fresh) {
        ctx->tickets_issued = 0; ctx->epoch = 0;
        for (int s = 0; s < LFD_TICKET_LANES; ++s) ctx->lane_issued[s] = 0;
    }
    ctx->epoch = (ctx->epoch + 1) & LFD_EPOCH_MASK;
    if (ctx->epoch == 0) {   // epoch wrapped: clear stale words once
        LFD_HIP(ctx, hipMemsetAsync(static_cast<unsigned char*>(ctx->ws.ptr) + kWsHeader, 0, ctx->ws.bytes - kWsHeader, ctx->stream));
        LFD_HIP(ctx, hipMemsetAsync(static_cast<unsigned char*>(ctx->ws.ptr) + 16, 0, 4, ctx->stream));   // seg_ready
        ctx->epoch = 1;
    }
    unsigned char* base = static_cast<unsigned char*>(ctx->ws.ptr);
    L.ticket = reinterpret_cast<unsigned long long*>(base);
    L.ticket_lanes = reinterpret_cast<unsigned long long*>(base + 128);
    L.tile_state = reinterpret_cast<unsigned long long*>(base + kWsHeader);
    L.status = reinterpret_cast<unsigned int*>(base + 8);
    L.seg_ready = reinterpret_cast<unsigned int*>(base + 16);
    L.ticket_base = ctx->tickets_issued;
    L.epoch = ctx->epoch;
    if (lanes) {             // n_tickets workgroups, workgroup b draws from sequence b % LANES
        for (int s = 0; s < LFD_TICKET_LANES; ++s) {
            L.ticket_base_lane[s] = ctx->lane_issued[s];
            if ((size_t)s < n_tickets) ctx->lane_issued[s] += (n_tickets - (size_t)s + LFD_TICKET_LANES - 1) / LFD_TICKET_LANES;
        }
    } else {
        ctx->tickets_issued += n_tickets;
    }
    return LFD_OK;
}

void read_env_switches(lfd_context* ctx) {
    ctx->env = LfdEnvSwitches();
    if (const char* e = std::getenv("LFD_DENSE_EXTRA_LDS")) ctx->env.dense_extra_lds = (size_t)std::atol(e);
    if (const char* e = std::getenv("LFD_DENSE_TIMING")) ctx->env.dense_timing_path = e;
    if (const char* e = std::getenv("LFD_DENSE_GENERIC")) ctx->env.dense_generic = std::atoi(e) != 0;
    if (const char* e = std::getenv("LFD_INDEXED_SPLIT")) ctx->env.indexed_split = std::atoi(e) != 0;
    if (const char* e = std::getenv("LFD_SELECT_TIMING")) ctx->env.select_timing = std::max(1, std::atoi(e));
    if (const char* e = std::getenv("LFD_SELECT_WORKGROUPS")) ctx->env.select_workgroups = std::atoi(e);
    if (const char* e = std::getenv("LFD_COMPONENT_PLAIN_SIZE")) ctx->env.component_plain_size = std::atoi(e) != 0;
}

int check_points(lfd_context* ctx, const lfd_points* out, const long long* ref_offsets) {
    if (!out || !out->xyz || !out->rgb || !out->err) return fail(ctx, LFD_ERR_INVALID, "null output buffers");
    if (out->capacity < 0) return fail(ctx, LFD_ERR_INVALID, "negative capacity");
    if (!ref_offsets) return fail(ctx, LFD_ERR_INVALID, "ref_offsets is required");
    return LFD_OK;
}

// The LfdLaunch of a batch for the calls that only read it (support, refine, normals, sigma): the batch's tables and per-pair constants, derived
// again only when the batch differs from the last one seen (no threshold reaches them).
int batch_launch(lfd_context* ctx, const lfd_batch* batch, LfdLaunch& L) {
    lfd_params none;
    std::memset(&none, 0, sizeof(none));
    return prepare_launch(ctx, batch, &none, nullptr, 0, L, nullptr);
}

// ---- what the stages on the final cloud share (voxel, consensus, free-space, fuse, kNN): plan, workspace, statistics, sort, heads, compaction -------
// All of them are synchronous and run on the context's stream, so they carve one workspace, ctx->cloud_ws; each writes or clears what it reads.
struct CloudPlan {
    long long n;
    long long G, chunk;          // radix passes: workgroup b of G owns the items [b * chunk, (b + 1) * chunk); chunk is a multiple of the scatter's 512-item round
    int n_part;                  // workgroups (= partial results) of the min / max pass
    long long n_wg;              // workgroups of the kernels that give a thread to every point
    unsigned grid;               // ... and of those that stride over the points
};

CloudPlan cloud_plan(int64_t n) {
    CloudPlan p;
    p.n = n;
    p.G = std::min<long long>(1024, (n + 4095) / 4096);
    p.chunk = (((n + p.G - 1) / p.G) + 511) / 512 * 512;
    p.G = (n + p.chunk - 1) / p.chunk;
    p.n_part = (int)std::min<long long>(1024, (n + 255) / 256);
    p.n_wg = (n + 255) / 256;
    p.grid = (unsigned)std::min<long long>(p.n_wg, 4096);
    return p;
}

// Bump allocator over the workspace: every region starts on a 256-byte boundary.  A layout is run twice (carve_cloud_ws): without a buffer for
// the size, then over the buffer.
struct Bump {
    unsigned char* base;         // null: sizing only, every region comes back null
    size_t at = 0;
    template <class T>
    T* take(size_t count, size_t extra_bytes = 0) {
        const size_t o = at;
        at = (at + count * sizeof(T) + extra_bytes + 255) & ~size_t(255);
        return base ? reinterpret_cast<T*>(base + o) : nullptr;
    }
};

template <class Layout>
int carve_cloud_ws(lfd_context* ctx, Layout&& layout) {
    Bump size{nullptr};
    layout(size);
    if (int rc = ensure(ctx, ctx->cloud_ws, size.at)) return rc;
    Bump b{static_cast<unsigned char*>(ctx->cloud_ws.ptr)};
    layout(b);
    return LFD_OK;
}

struct CloudSort {               // partials | stats + counters | digit counts | keys x 2 | indices x 2 | cell starts
    LfdVoxStats *part, *stats;
    unsigned* counters;          // the stage's few words behind the statistics; [0] is the number of occupied cells where there are heads
    unsigned* counts;
    unsigned long long* keys[2];
    unsigned* idx[2];
    unsigned* vstart;            // null for a stage without heads
};

CloudSort carve_sort(Bump& b, long long n, int n_counters, bool heads) {
    CloudSort w;
    w.part = b.take<LfdVoxStats>(1024);
    w.stats = b.take<LfdVoxStats>(1, (size_t)n_counters * sizeof(unsigned));
    w.counters = w.stats ? reinterpret_cast<unsigned*>(w.stats + 1) : nullptr;
    w.counts = b.take<unsigned>(256 * 1024);
    for (int i = 0; i < 2; ++i) w.keys[i] = b.take<unsigned long long>((size_t)n);
    for (int i = 0; i < 2; ++i) w.idx[i] = b.take<unsigned>((size_t)n);
    w.vstart = heads ? b.take<unsigned>((size_t)n) : nullptr;
    return w;
}

// min / max pass (with rgb: lfd_voxel_minmax_kernel, colour maximum and NaN flag too; without: lfd_consensus_minmax_kernel) and its read-back.
// The stream is idle when this returns: a stage decides its refusals on `s` before anything is sorted.
int cloud_stats(lfd_context* ctx, const CloudPlan& p, const CloudSort& w, const float* xyz, const float* rgb, LfdVoxStats& s) {
    hipStream_t st = ctx->stream;
    if (rgb) hipLaunchKernelGGL(lfd_voxel_minmax_kernel, dim3(p.n_part), dim3(256), 0, st, xyz, rgb, p.n, w.part);
    else hipLaunchKernelGGL(lfd_consensus_minmax_kernel, dim3(p.n_part), dim3(256), 0, st, xyz, p.n, w.part);
    hipLaunchKernelGGL(lfd_voxel_final_kernel, dim3(1), dim3(256), 0, st, w.part, p.n_part, w.stats);
    LFD_HIP(ctx, hipGetLastError());
    LFD_HIP(ctx, hipMemcpyAsync(ctx->pinned_words, w.stats, sizeof(LfdVoxStats), hipMemcpyDeviceToHost, st));
    LFD_HIP(ctx, hipStreamSynchronize(st));
    std::memcpy(&s, ctx->pinned_words, sizeof(s));
    return LFD_OK;
}

// stable LSD radix sort of (keys[0], idx[0]) over the low `bits` bits, 8 at a time; returns which of the two buffers holds the result
int cloud_sort(hipStream_t st, const CloudPlan& p, const CloudSort& w, int bits) {
    int cur = 0;
    for (int shift = 0; shift < bits; shift += 8, cur ^= 1) {
        hipLaunchKernelGGL(lfd_voxel_hist_kernel, dim3((unsigned)p.G), dim3(256), 0, st, w.keys[cur], p.n, p.chunk, shift, w.counts);
        hipLaunchKernelGGL(lfd_voxel_scan_kernel, dim3(1), dim3(1024), 0, st, w.counts, (int)(256 * p.G), (unsigned*)nullptr);
        hipLaunchKernelGGL(lfd_voxel_scatter_kernel, dim3((unsigned)p.G), dim3(512), 0, st, w.keys[cur], w.idx[cur], p.n, p.chunk, shift, w.counts,
                           w.keys[cur ^ 1], w.idx[cur ^ 1]);
    }
    return cur;
}

// heads of the sorted keys: the number of occupied cells goes to counters[0] ...
void cloud_heads_count(hipStream_t st, const CloudPlan& p, const CloudSort& w, int cur) {
    hipLaunchKernelGGL(lfd_voxel_head_count_kernel, dim3((unsigned)p.G), dim3(256), 0, st, w.keys[cur], p.n, p.chunk, w.counts);
    hipLaunchKernelGGL(lfd_voxel_scan_kernel, dim3(1), dim3(1024), 0, st, w.counts, (int)p.G, w.counters);
}

// ... and the first sorted position of every cell to vstart
void cloud_heads_scatter(hipStream_t st, const CloudPlan& p, const CloudSort& w, int cur) {
    hipLaunchKernelGGL(lfd_voxel_head_scatter_kernel, dim3((unsigned)p.G), dim3(512), 0, st, w.keys[cur], p.n, p.chunk, w.counts, w.vstart);
}

struct CloudCompact {            // offsets in, out | keep bytes | kept per workgroup
    long long *offs, *offs_out;
    uint8_t* keep;
    unsigned* wg_kept;
};

CloudCompact carve_compact(Bump& b, const CloudPlan& p, int32_t n_refs) {
    CloudCompact c;
    c.offs = b.take<long long>((size_t)n_refs + 1);
    c.offs_out = b.take<long long>((size_t)n_refs + 1);
    c.keep = b.take<uint8_t>((size_t)p.n_wg * 256);
    c.wg_kept = b.take<unsigned>((size_t)p.n_wg + 1);
    return c;
}

// kept points in front of every 256 input points (wg_kept[b]) and in all (wg_kept[n_wg]) from the keep bytes
void cloud_compact_prefix(hipStream_t st, const CloudPlan& p, const CloudCompact& c) {
    hipLaunchKernelGGL(lfd_consensus_wgcount_kernel, dim3((unsigned)p.n_wg), dim3(256), 0, st, c.keep, p.n, c.wg_kept);
    hipLaunchKernelGGL(lfd_voxel_scan_kernel, dim3(1), dim3(1024), 0, st, c.wg_kept, (int)p.n_wg, c.wg_kept + p.n_wg);
}

// From the keep bytes to the compacted cloud, its reference offsets and its size on the host.  The stream is idle when this returns.
int cloud_compact(lfd_context* ctx, const CloudPlan& p, const CloudCompact& c, const float* xyz, const float* rgb, const float* err, int32_t n_refs,
                  float* xyz_out, float* rgb_out, float* err_out, int64_t* ref_offsets_out_host, int64_t* n_out_host) {
    hipStream_t st = ctx->stream;
    cloud_compact_prefix(st, p, c);
    hipLaunchKernelGGL(lfd_consensus_offsets_kernel, dim3((unsigned)std::min<long long>(((long long)n_refs + 256) / 256, 1024)), dim3(256), 0, st, c.offs,
                       (int)n_refs, c.keep, c.wg_kept, c.offs_out);
    hipLaunchKernelGGL(lfd_consensus_scatter_kernel, dim3((unsigned)p.n_wg), dim3(256), 0, st, xyz, rgb, err, p.n, c.keep, c.wg_kept, xyz_out, rgb_out,
                       err_out);
    LFD_HIP(ctx, hipGetLastError());
    LFD_HIP(ctx, hipMemcpyAsync(ref_offsets_out_host, c.offs_out, ((size_t)n_refs + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
    LFD_HIP(ctx, hipStreamSynchronize(st));
    *n_out_host = ref_offsets_out_host[n_refs];
    return LFD_OK;
}

}  // namespace

int lfd_fail(lfd_context* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg;
    else { std::lock_guard<std::mutex> lock(g_create_mutex); g_create_error = msg; }
    return code;
}

// =================================================================================================
extern "C" {

int lfd_abi_version(void) { return LFD_ABI_VERSION; }

int lfd_struct_layout(int32_t* out, int32_t capacity) {
#define LFD_OFF(T, f) (int32_t)offsetof(T, f), (int32_t)sizeof(((T*)nullptr)->f)
    const int32_t table[] = {
        (int32_t)sizeof(lfd_params), 7, LFD_OFF(lfd_params, sampson_thresh), LFD_OFF(lfd_params, certainty_thresh), LFD_OFF(lfd_params, sample_cap),
        LFD_OFF(lfd_params, reproj_thresh), LFD_OFF(lfd_params, min_parallax_deg), LFD_OFF(lfd_params, no_filter), LFD_OFF(lfd_params, flags),
        (int32_t)sizeof(lfd_batch), 19, LFD_OFF(lfd_batch, n_refs), LFD_OFF(lfd_batch, k), LFD_OFF(lfd_batch, H), LFD_OFF(lfd_batch, W),
        LFD_OFF(lfd_batch, w_match), LFD_OFF(lfd_batch, h_match), LFD_OFF(lfd_batch, warp_channels), LFD_OFF(lfd_batch, reserved),
        LFD_OFF(lfd_batch, ref_cam), LFD_OFF(lfd_batch, n_slots), LFD_OFF(lfd_batch, nbr_cam), LFD_OFF(lfd_batch, cert), LFD_OFF(lfd_batch, warp),
        LFD_OFF(lfd_batch, image), LFD_OFF(lfd_batch, mask_a), LFD_OFF(lfd_batch, mask_b), LFD_OFF(lfd_batch, axis_x), LFD_OFF(lfd_batch, axis_y),
        LFD_OFF(lfd_batch, fundamental),
        (int32_t)sizeof(lfd_points), 6, LFD_OFF(lfd_points, xyz), LFD_OFF(lfd_points, rgb), LFD_OFF(lfd_points, err), LFD_OFF(lfd_points, cell),
        LFD_OFF(lfd_points, slot), LFD_OFF(lfd_points, capacity),
        (int32_t)sizeof(lfd_tile_segment), 2, LFD_OFF(lfd_tile_segment, offset), LFD_OFF(lfd_tile_segment, count),
        (int32_t)sizeof(lfd_copy_segment), 3, LFD_OFF(lfd_copy_segment, src_offset), LFD_OFF(lfd_copy_segment, dst_offset), LFD_OFF(lfd_copy_segment, nbytes),
    };
#undef LFD_OFF
    const int32_t n = (int32_t)(sizeof(table) / sizeof(table[0]));
    for (int32_t i = 0; out != nullptr && i < n && i < capacity; ++i) out[i] = table[i];
    return n;
}

const char* lfd_struct_fields(void) {
    return "lfd_params:sampson_thresh,certainty_thresh,sample_cap,reproj_thresh,min_parallax_deg,no_filter,flags;"
           "lfd_batch:n_refs,k,H,W,w_match,h_match,warp_channels,reserved,ref_cam,n_slots,nbr_cam,cert,warp,image,mask_a,mask_b,axis_x,axis_y,fundamental;"
           "lfd_points:xyz,rgb,err,cell,slot,capacity;"
           "lfd_tile_segment:offset,count;"
           "lfd_copy_segment:src_offset,dst_offset,nbytes";
}

const char* lfd_last_error(const lfd_context* ctx) {
    if (ctx) return ctx->err.c_str();
    std::lock_guard<std::mutex> lock(g_create_mutex);
    t_create_error_copy = g_create_error;
    return t_create_error_copy.c_str();
}

int lfd_create(int device_index, void* hip_stream, lfd_context** out) {
    if (!out) return fail(nullptr, LFD_ERR_INVALID, "out is null");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, LFD_ERR_HIP, std::string("no HIP device available: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
    if (device_index < 0 || device_index >= n) return fail(nullptr, LFD_ERR_INVALID, "device index out of range");
    lfd_context* ctx = new lfd_context();
    ctx->device = device_index;
    ctx->stream = static_cast<hipStream_t>(hip_stream);
    read_env_switches(ctx);      // profiling / A-B switches: read ONCE here, never on a launch path
    e = hipSetDevice(device_index);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&ctx->n_cus, hipDeviceAttributeMultiprocessorCount, device_index);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&ctx->pinned_words), 32 * sizeof(int), hipHostMallocDefault);
    if (e != hipSuccess) {
        std::string m = std::string("context init: ") + hipGetErrorString(e);
        delete ctx;
        return fail(nullptr, LFD_ERR_HIP, m);
    }
    *out = ctx;
    return LFD_OK;
}

void lfd_destroy(lfd_context* ctx) {
    if (!ctx) return;
    if (ctx->is_host) { lfd_host_pool_destroy(ctx->host_pool); delete ctx; return; }
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->prep_stream) { (void)hipStreamSynchronize(ctx->prep_stream); (void)hipStreamDestroy(ctx->prep_stream); }
    for (LfdBatchSlot& sl : ctx->slot) {
        if (sl.desc.ptr) (void)hipFree(sl.desc.ptr);
        if (sl.consts.ptr) (void)hipFree(sl.consts.ptr);
        if (sl.pinned) (void)hipHostFree(sl.pinned);
        if (sl.pinned_x) (void)hipHostFree(sl.pinned_x);
        for (hipEvent_t ev : {sl.pinned_free, sl.ready, sl.idle, sl.x_free}) if (ev) (void)hipEventDestroy(ev);
    }
    for (hipEvent_t ev : ctx->kt_start) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : ctx->kt_stop) (void)hipEventDestroy(ev);
    for (DeviceBuffer* b : {&ctx->cams, &ctx->ws, &ctx->axes, &ctx->scratch, &ctx->codes, &ctx->idx_tab, &ctx->agg, &ctx->sel_buf, &ctx->colour_tab, &ctx->mt, &ctx->mt_ckpt, &ctx->mt_batch, &ctx->sel_scratch, &ctx->sel_chain, &ctx->stamps, &ctx->img_tab, &ctx->msk_tab, &ctx->seg_scan, &ctx->cloud_ws, &ctx->support_ws, &ctx->prec.tab, &ctx->colour_img.tab, &ctx->pose_const.tab, &ctx->undist_cnt})
        if (b->ptr) (void)hipFree(b->ptr);
    if (ctx->pinned_words) (void)hipHostFree(ctx->pinned_words);
    for (lfd_context::PointerTable* t : {&ctx->prec, &ctx->colour_img, &ctx->pose_const}) {
        if (t->pinned) (void)hipHostFree(t->pinned);
        if (t->free_ev) (void)hipEventDestroy(t->free_ev);
    }
    delete ctx;
}

int lfd_kernel_timing(lfd_context* ctx, int32_t n_launches) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (n_launches < 0 || n_launches > (1 << 20)) return fail(ctx, LFD_ERR_INVALID, "lfd_kernel_timing: n_launches must be in [0, 2^20]");
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    LFD_HIP(ctx, hipStreamSynchronize(ctx->stream));           // no launch is still using the events that go
    if (ctx->prep_stream) LFD_HIP(ctx, hipStreamSynchronize(ctx->prep_stream));
    for (LfdBatchSlot& sl : ctx->slot) { sl.idle_attached = false; sl.idle_ext = nullptr; sl.used = false; }      // (nor is a slot waiting on one)
    while (ctx->kt_start.size() > (size_t)n_launches) {
        (void)hipEventDestroy(ctx->kt_start.back()); (void)hipEventDestroy(ctx->kt_stop.back());
        ctx->kt_start.pop_back(); ctx->kt_stop.pop_back();
    }
    while (ctx->kt_start.size() < (size_t)n_launches) {
        // kt_start / kt_stop: read for their time stamps (hipEventElapsedTime; lfd_kernel_timing_read waits for the last stop only to know the
        // stamps are there), and a stop event doubles as the slot's `idle` marker above - nobody reads device results on their strength
        hipEvent_t a = nullptr, b = nullptr;
        LFD_HIP(ctx, hipEventCreateWithFlags(&a, hipEventDisableSystemFence));
        hipError_t e = hipEventCreateWithFlags(&b, hipEventDisableSystemFence);
        if (e != hipSuccess) { (void)hipEventDestroy(a); return fail(ctx, LFD_ERR_HIP, std::string("hipEventCreate: ") + hipGetErrorString(e)); }
        ctx->kt_start.push_back(a); ctx->kt_stop.push_back(b);
    }
    ctx->kt_used = 0;
    return LFD_OK;
}

int lfd_kernel_timing_read(lfd_context* ctx, float* ms, int32_t capacity, int32_t* n_out) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (!n_out || capacity < 0 || (capacity > 0 && !ms)) return fail(ctx, LFD_ERR_INVALID, "lfd_kernel_timing_read: bad arguments");
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = std::min(ctx->kt_used, (size_t)capacity);
    if (ctx->kt_used) LFD_HIP(ctx, hipEventSynchronize(ctx->kt_stop[ctx->kt_used - 1]));
    for (size_t i = 0; i < n; ++i) LFD_HIP(ctx, hipEventElapsedTime(ms + i, ctx->kt_start[i], ctx->kt_stop[i]));
    *n_out = (int32_t)n;
    ctx->kt_used = 0;
    return LFD_OK;
}

int lfd_reload_env(lfd_context* ctx) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    read_env_switches(ctx);
    return LFD_OK;
}

int lfd_set_stream(lfd_context* ctx, void* hip_stream) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    LFD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->prep_stream) LFD_HIP(ctx, hipStreamSynchronize(ctx->prep_stream));
    for (LfdBatchSlot& sl : ctx->slot) { sl.ready_pending = false; sl.used = false; sl.idle_attached = false; }      // everything issued so far has completed
    ctx->last_used = -1;
    ctx->stream = static_cast<hipStream_t>(hip_stream);
    return LFD_OK;
}

int lfd_launch_status(lfd_context* ctx, int32_t* status_out) {
    if (!ctx || !status_out) return fail(ctx, LFD_ERR_INVALID, "null argument");
    *status_out = 0;
    if (ctx->is_host) return LFD_OK;
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->ws.ptr) { LFD_HIP(ctx, hipStreamSynchronize(ctx->stream)); return LFD_OK; }
    LFD_HIP(ctx, hipMemcpyAsync(ctx->pinned_words, static_cast<unsigned char*>(ctx->ws.ptr) + 8, sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
    LFD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const unsigned int st = (unsigned int)ctx->pinned_words[0];
    if (st != 0) {
        LFD_HIP(ctx, hipMemset(static_cast<unsigned char*>(ctx->ws.ptr) + 8, 0, sizeof(st)));
        *status_out = (int32_t)st;
        return fail(ctx, LFD_ERR_HIP, "a look-back spin timed out (workgroups of the persistent grid were not co-resident); results of the last launch are invalid");
    }
    return LFD_OK;
}

int lfd_get_pair_fundamental(lfd_context* ctx, int32_t n_pairs, double* F_out_host) {
    if (!ctx || !F_out_host || n_pairs <= 0) return fail(ctx, LFD_ERR_INVALID, "bad arguments");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    const LfdBatchSlot& sl = ctx->slot[ctx->cur];        // the batch of the last launch
    if (ctx->last_used < 0 || !sl.consts_valid || !sl.consts.ptr) return fail(ctx, LFD_ERR_STATE, "no batch has been launched on this context yet");
    if (n_pairs != sl.refs * sl.k) return fail(ctx, LFD_ERR_INVALID, "n_pairs must be n_refs * k of the last batch");
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ref_bytes = ((size_t)sl.refs * sizeof(LfdRefConst) + 15) & ~size_t(15);
    std::vector<LfdPairConst> host((size_t)n_pairs);
    LFD_HIP(ctx, hipMemcpyAsync(host.data(), static_cast<unsigned char*>(sl.consts.ptr) + ref_bytes, host.size() * sizeof(LfdPairConst),
                                hipMemcpyDeviceToHost, ctx->stream));
    LFD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n_pairs; ++i)
        for (int j = 0; j < 9; ++j) F_out_host[(size_t)i * 9 + j] = host[(size_t)i].F[j];
    return LFD_OK;
}

int lfd_upload_cameras(lfd_context* ctx, int32_t n, const float* K, const float* R, const float* t, const float* P,
                       const float* C, const int32_t* wh) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (n <= 0 || !K || !R || !t || !P || !C || !wh) return fail(ctx, LFD_ERR_INVALID, "bad camera arrays");
    std::vector<LfdCam> cams((size_t)n);
    for (int i = 0; i < n; ++i) {
        LfdCam& c = cams[i];
        std::memcpy(c.K, K + (size_t)i * 9, sizeof(c.K));
        std::memcpy(c.R, R + (size_t)i * 9, sizeof(c.R));
        std::memcpy(c.t, t + (size_t)i * 3, sizeof(c.t));
        std::memcpy(c.P, P + (size_t)i * 12, sizeof(c.P));
        std::memcpy(c.C, C + (size_t)i * 3, sizeof(c.C));
        c.w = wh[i * 2 + 0]; c.h = wh[i * 2 + 1];
        c.pad[0] = c.pad[1] = 0;
        if (c.w <= 0 || c.h <= 0) return fail(ctx, LFD_ERR_INVALID, "camera width/height must be positive");
    }
    if (ctx->is_host) { ctx->host_cams.swap(cams); ctx->n_cams = n; return LFD_OK; }
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    int rc = ensure(ctx, ctx->cams, cams.size() * sizeof(LfdCam));
    if (rc != LFD_OK) return rc;
    LFD_HIP(ctx, hipMemcpyAsync(ctx->cams.ptr, cams.data(), cams.size() * sizeof(LfdCam), hipMemcpyHostToDevice, ctx->stream));
    LFD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->prep_stream) LFD_HIP(ctx, hipStreamSynchronize(ctx->prep_stream));
    ctx->host_cams.swap(cams);
    ctx->n_cams = n;
    for (LfdBatchSlot& sl : ctx->slot) sl.consts_valid = false;      // every constant block derives from the camera table
    return LFD_OK;
}

int lfd_prepare_batch(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params) {
    LfdLaunch L;
    return prepare_launch(ctx, batch, params, nullptr, 0, L, nullptr, /*ahead=*/true);
}

int lfd_aggregate(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params, float* best_cert, uint8_t* best_slot) {
    LfdLaunch L;
    int rc = prepare_launch(ctx, batch, params, nullptr, 0, L, nullptr);
    if (rc != LFD_OK) return rc;
    if (!best_cert) return fail(ctx, LFD_ERR_INVALID, "best_cert is null");
    const long long HW = (long long)batch->H * batch->W;
    const int per_block = 256 * 4;
    int gx = (int)std::min<long long>((HW + per_block - 1) / per_block, 2048);
    dim3 grid((unsigned)gx, (unsigned)batch->n_refs, 1);
    hipLaunchKernelGGL(lfd_aggregate_kernel, grid, dim3(256), 0, ctx->stream, L, best_cert, best_slot);
    LFD_HIP(ctx, hipGetLastError());
    return LFD_OK;
}

// Which instantiation of the ordered dense kernel a launch of lfd_triangulate_dense may run: 1 = the production-shape one (lfd_dense_prod_kernel,
// lfd_kernels.hip: every question below is compiled into it as answered), 0 = the generic one.  A pure function of its arguments - no context, no
// device - and the ONLY place the conditions are written down: every line is an assumption the kernel makes and does not test again.
int lfd_dense_variant(const lfd_batch* b, const lfd_params* p, const lfd_points* out, const int32_t* seg_counts) {
    if (!b || !p || !out) return 0;
    const long long tile = LFD_DENSE_BLOCK * LFD_DENSE_CPT;
    if (b->n_refs <= 0 || b->H <= 0 || b->W <= 0 || (b->W & 3) != 0 || ((long long)b->H * b->W) % tile != 0) return 0;      // whole tiles, rows of whole threads
    if (b->warp_channels != 2 || b->axis_x || b->axis_y) return 0;                     // [xB, yB] warps on the identity axes (and with them the colour tables)
    if ((p->flags & LFD_FLAG_EXACT_COLOUR) != 0) return 0;                             // f32 colour blend
    if (!(p->certainty_thresh > 0.0f)) return 0;                                       // a positive floor: no cell of an unmasked reference is dead
    if (p->no_filter || !(p->sampson_thresh > 0.0) || !(p->min_parallax_deg > 0.0f)) return 0;      // all three gates on
    if (seg_counts || out->cell || out->slot) return 0;                                // xyz / rgb / err / ref_offsets only
    if (b->mask_a || b->mask_b) {                                                      // no mask on any reference (what upload_tables calls any_mask)
        if (!b->n_slots) return 0;
        for (int r = 0; r < b->n_refs; ++r) {
            if (b->mask_a && b->mask_a[r]) return 0;
            for (int j = 0; b->mask_b && j < b->n_slots[r] && j < b->k; ++j)
                if (b->mask_b[(size_t)r * b->k + j]) return 0;
        }
    }
    return 1;
}

// the dense launch in its two forms: ordered (ref_offsets; ref_counts / table null) and unordered retirement (ref_counts + table)
static int dense_launch(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params, const lfd_points* out,
                        int64_t* ref_offsets, int32_t* seg_counts, int64_t* ref_counts, lfd_tile_segment* table, uint8_t* ply = nullptr) {
    const bool unordered = table != nullptr;
    LfdLaunch L;
    int rc = prepare_launch(ctx, batch, params, nullptr, 0, L, nullptr);
    if (rc != LFD_OK) return rc;
    if (ply) {                         // file-payload output: the records go to `ply`; out carries the capacity (and optionally cell / slot)
        if (!out || out->capacity < 0 || !(unordered ? (void*)ref_counts : (void*)ref_offsets))
            return fail(ctx, LFD_ERR_INVALID, "lfd_triangulate_dense_ply[_segments]: the capacity and ref_offsets (ordered) / ref_counts (unordered) are required");
    } else {
        rc = check_points(ctx, out, reinterpret_cast<long long*>(unordered ? ref_counts : ref_offsets));
        if (rc != LFD_OK) return rc;
    }
    if (unordered && out->capacity < (int64_t)batch->n_refs * batch->H * batch->W)
        return fail(ctx, LFD_ERR_CAPACITY, "lfd_triangulate_dense_segments: capacity must be n_refs * H * W (every reference owns a region of H * W records)");
    const size_t n_tiles = (size_t)batch->n_refs * (size_t)L.tiles_per_ref;
    if (n_tiles > 0x7fffffffu) return fail(ctx, LFD_ERR_INVALID, "too many tiles in one launch");
    const size_t grid = n_tiles;              // one workgroup per tile, numbered by ticket
    rc = prepare_lookback(ctx, n_tiles, grid, true, L);
    if (rc != LFD_OK) return rc;
    L.xyz = out->xyz; L.rgb = out->rgb; L.err = out->err; L.cell = out->cell; L.slot = out->slot;
    L.capacity = out->capacity;
    L.ref_offsets = reinterpret_cast<long long*>(ref_offsets);
    L.seg_counts = seg_counts;                // zeroed inside the kernel (tile 0), no memset launch
    static_assert(sizeof(lfd_tile_segment) == sizeof(LfdTileSeg), "lfd_tile_segment is the kernels' LfdTileSeg");
    L.ref_cursor = reinterpret_cast<unsigned long long*>(ref_counts);      // (zeroed the same way)
    L.tile_table = reinterpret_cast<LfdTileSeg*>(table);
    L.ply = ply;
    size_t extra_lds = 0;                     // profiling switch: dynamic LDS lowers the number of resident workgroups
    extra_lds = ctx->env.dense_extra_lds;
#if defined(LFD_DENSE_TIMING)            // profiling builds: per-tile phase stamps, dumped to the file named by LFD_DENSE_TIMING
    const char* stamp_path = ctx->env.dense_timing_path.empty() ? nullptr : ctx->env.dense_timing_path.c_str();
    if (stamp_path) {
        rc = ensure(ctx, ctx->stamps, n_tiles * 2 * 12 * sizeof(unsigned long long));
        if (rc != LFD_OK) return rc;
        LFD_HIP(ctx, hipMemsetAsync(ctx->stamps.ptr, 0, n_tiles * 2 * 12 * sizeof(unsigned long long), ctx->stream));
        L.phase_stamps = static_cast<unsigned long long*>(ctx->stamps.ptr);
    }
#endif
#if defined(LFD_FORCE_EXACT_COLOUR)      // profiling builds: what the f64 colour costs on the bench workload
    const bool exact_colour = true;
#else
    const bool exact_colour = (params->flags & LFD_FLAG_EXACT_COLOUR) != 0;
#endif
    if (!exact_colour && L.axis_identity && batch->warp_channels == 2) {      // the f32 blend reads its positions and weights from tables
        rc = colour_tables(ctx, batch->W, batch->H, batch->w_match, batch->h_match, &L.colour_cols, &L.colour_rows);
        if (rc != LFD_OK) return rc;
    }
    // The launch carries its own stop event (hipExtLaunchKernelGGL): it marks the end of this batch slot's last user - what the staging
    // of a later batch into the slot waits for - without a marker packet of its own in the stream; with lfd_kernel_timing switched on
    // the pair of events is the next of its ring and doubles as that marker.
    LfdBatchSlot& used_slot = ctx->slot[ctx->cur];
    rc = slot_events(ctx, used_slot);
    if (rc != LFD_OK) return rc;
    hipEvent_t t_start = nullptr, t_stop = used_slot.idle;
    if (ctx->kt_used < ctx->kt_start.size()) { t_start = ctx->kt_start[ctx->kt_used]; t_stop = ctx->kt_stop[ctx->kt_used]; ++ctx->kt_used; }
    // (the colour tables exist whenever the predicate holds; LFD_DENSE_GENERIC=1 keeps the generic kernel for tests and A/B runs)
    const bool prod = !ply && !unordered && !exact_colour && !ctx->env.dense_generic && L.colour_cols && lfd_dense_variant(batch, params, out, seg_counts) == 1;
    auto kernel = prod ? lfd_dense_prod_kernel
                : (ply && unordered) ? (exact_colour ? lfd_dense_ply_segments_exact_kernel : lfd_dense_ply_segments_kernel)
                : ply ? (exact_colour ? lfd_dense_ply_exact_kernel : lfd_dense_ply_kernel)
                : unordered ? (exact_colour ? lfd_dense_segments_exact_kernel : lfd_dense_segments_kernel)
                            : (exact_colour ? lfd_dense_exact_kernel : lfd_dense_kernel);
    hipExtLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(LFD_DENSE_BLOCK), (unsigned)extra_lds, ctx->stream, t_start, t_stop, 0, L);
    LFD_HIP(ctx, hipGetLastError());
    used_slot.idle_ext = t_stop;          // (only behind a launch that went out: a later staging into the slot waits for THIS event)
    used_slot.idle_attached = true;
#if defined(LFD_DENSE_TIMING)
    if (stamp_path) {
        std::vector<unsigned long long> host(n_tiles * 2 * 12);
        LFD_HIP(ctx, hipMemcpyAsync(host.data(), ctx->stamps.ptr, host.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        LFD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (FILE* f = std::fopen(stamp_path, "wb")) { std::fwrite(host.data(), sizeof(unsigned long long), host.size(), f); std::fclose(f); }
    }
#endif
    return LFD_OK;
}

int lfd_triangulate_dense(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params, const lfd_points* out,
                          int64_t* ref_offsets, int32_t* seg_counts) {
    return dense_launch(ctx, batch, params, out, ref_offsets, seg_counts, nullptr, nullptr);
}

int lfd_triangulate_dense_ply(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params, uint8_t* records, int64_t capacity,
                              int64_t* ref_offsets, int32_t* seg_counts, int32_t* cell, uint8_t* slot) {
    if (ctx && !records) return fail(ctx, LFD_ERR_INVALID, "lfd_triangulate_dense_ply: records is null");
    lfd_points out;
    std::memset(&out, 0, sizeof(out));
    out.capacity = capacity;
    out.cell = cell;
    out.slot = slot;
    return dense_launch(ctx, batch, params, &out, ref_offsets, seg_counts, nullptr, nullptr, records);
}

int lfd_dense_tiles_per_ref(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0) return 0;
    const long long tile = LFD_DENSE_BLOCK * LFD_DENSE_CPT;
    return (int)(((long long)H * W + tile - 1) / tile);
}

int lfd_triangulate_dense_segments(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params, const lfd_points* out,
                                   int64_t* ref_counts, int32_t* seg_counts, lfd_tile_segment* table) {
    if (ctx && !table) return fail(ctx, LFD_ERR_INVALID, "lfd_triangulate_dense_segments: the tile table is required");
    return dense_launch(ctx, batch, params, out, nullptr, seg_counts, ref_counts, table);
}

int lfd_triangulate_dense_ply_segments(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params, uint8_t* records, int64_t capacity,
                                       int64_t* ref_counts, int32_t* seg_counts, lfd_tile_segment* table) {
    if (ctx && (!records || !table)) return fail(ctx, LFD_ERR_INVALID, "lfd_triangulate_dense_ply_segments: records and the tile table are required");
    lfd_points out;
    std::memset(&out, 0, sizeof(out));
    out.capacity = capacity;
    return dense_launch(ctx, batch, params, &out, nullptr, seg_counts, ref_counts, table, records);
}

// exclusive prefix of the table in tile order into the context's scratch (tile_dst[n_tiles + 1]); the launches that follow read it
static int segment_scan(lfd_context* ctx, int32_t n_refs, int32_t H, int32_t W, const lfd_tile_segment* table, int64_t* ref_offsets,
                        const long long** tile_dst, int* tpr_out, int* n_tiles_out) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (n_refs <= 0 || H <= 0 || W <= 0 || !table) return fail(ctx, LFD_ERR_INVALID, "bad segment arguments");
    const int tpr = lfd_dense_tiles_per_ref(H, W);
    const long long n_tiles = (long long)n_refs * tpr;
    if (n_tiles > 0x7fffffffLL) return fail(ctx, LFD_ERR_INVALID, "too many tiles");
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    int rc = ensure(ctx, ctx->seg_scan, ((size_t)n_tiles + 1) * sizeof(long long) + ((size_t)n_tiles + 2) * sizeof(int));      // prefix + chunk index
    if (rc != LFD_OK) return rc;
    long long* dst = static_cast<long long*>(ctx->seg_scan.ptr);
    hipLaunchKernelGGL(lfd_segment_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, reinterpret_cast<const LfdTileSeg*>(table), (int)n_tiles, tpr,
                       (int)n_refs, dst, reinterpret_cast<long long*>(ref_offsets));
    LFD_HIP(ctx, hipGetLastError());
    *tile_dst = dst; *tpr_out = tpr; *n_tiles_out = (int)n_tiles;
    return LFD_OK;
}

int lfd_order_segments(lfd_context* ctx, int32_t n_refs, int32_t H, int32_t W, const lfd_tile_segment* table, const lfd_points* src,
                       const lfd_points* dst, int64_t* ref_offsets) {
    const long long* tile_dst = nullptr; int tpr = 0, n_tiles = 0;
    int rc = segment_scan(ctx, n_refs, H, W, table, ref_offsets, &tile_dst, &tpr, &n_tiles);
    if (rc != LFD_OK) return rc;
    if (!src || !dst || !src->xyz || !src->rgb || !src->err || !dst->xyz || !dst->rgb || !dst->err) return fail(ctx, LFD_ERR_INVALID, "null point buffers");
    if (dst->capacity <= 0) return LFD_OK;
    const unsigned grid = (unsigned)std::min<int64_t>((dst->capacity + 1023) / 1024, 8192);
    hipLaunchKernelGGL(lfd_order_segments_kernel, dim3(grid), dim3(256), 0, ctx->stream, tile_dst, reinterpret_cast<const LfdTileSeg*>(table),
                       (long long)H * W, tpr, n_tiles, src->xyz, src->rgb, src->err, src->cell, src->slot, dst->xyz, dst->rgb, dst->err, dst->cell,
                       dst->slot, (long long)dst->capacity);
    LFD_HIP(ctx, hipGetLastError());
    return LFD_OK;
}

int lfd_pack_ply_segments(lfd_context* ctx, int32_t n_refs, int32_t H, int32_t W, const lfd_tile_segment* table, const float* xyz,
                          const float* rgb, int64_t capacity, uint8_t* out, int64_t* ref_offsets) {
    const long long* tile_dst = nullptr; int tpr = 0, n_tiles = 0;
    int rc = segment_scan(ctx, n_refs, H, W, table, ref_offsets, &tile_dst, &tpr, &n_tiles);
    if (rc != LFD_OK) return rc;
    if (capacity < 0 || (capacity > 0 && (!xyz || !rgb || !out))) return fail(ctx, LFD_ERR_INVALID, "bad arguments");
    if (reinterpret_cast<uintptr_t>(out) & 3u) return fail(ctx, LFD_ERR_INVALID, "out must be 4-byte aligned");
    if (capacity == 0) return LFD_OK;
    const unsigned grid = (unsigned)std::min<int64_t>((capacity + 255) / 256, 4096);
    hipLaunchKernelGGL(lfd_pack_ply_segments_kernel, dim3(grid), dim3(256), 0, ctx->stream, tile_dst, reinterpret_cast<const LfdTileSeg*>(table),
                       (long long)H * W, tpr, n_tiles, xyz, rgb, (long long)capacity, out);
    LFD_HIP(ctx, hipGetLastError());
    return LFD_OK;
}

int lfd_pack_points3d_segments(lfd_context* ctx, int32_t n_refs, int32_t H, int32_t W, const lfd_tile_segment* table, const float* xyz,
                               const float* rgb, const float* err, int64_t capacity, uint64_t id_base, uint8_t* out, int64_t* ref_offsets) {
    const long long* tile_dst = nullptr; int tpr = 0, n_tiles = 0;
    int rc = segment_scan(ctx, n_refs, H, W, table, ref_offsets, &tile_dst, &tpr, &n_tiles);
    if (rc != LFD_OK) return rc;
    if (capacity < 0 || (capacity > 0 && (!xyz || !rgb || !err || !out))) return fail(ctx, LFD_ERR_INVALID, "bad arguments");
    if (reinterpret_cast<uintptr_t>(out) & 3u) return fail(ctx, LFD_ERR_INVALID, "out must be 4-byte aligned");
    if (capacity == 0) return LFD_OK;
    const unsigned grid = (unsigned)std::min<int64_t>((capacity + 255) / 256, 4096);
    hipLaunchKernelGGL(lfd_pack_points3d_segments_kernel, dim3(grid), dim3(256), 0, ctx->stream, tile_dst, reinterpret_cast<const LfdTileSeg*>(table),
                       (long long)H * W, tpr, n_tiles, xyz, rgb, err, (long long)capacity, (unsigned long long)id_base, out);
    LFD_HIP(ctx, hipGetLastError());
    return LFD_OK;
}

int lfd_triangulate_indexed(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params, const int64_t* sel_idx,
                            const int64_t* sel_offsets, const lfd_points* out, int64_t* ref_offsets, int32_t* seg_counts,
                            int32_t* seg_order) {
    if (ctx && (!sel_idx || !sel_offsets)) return fail(ctx, LFD_ERR_INVALID, "sel_idx / sel_offsets are required");
    if (ctx && batch && batch->n_refs > 0) {
        if (sel_offsets[0] != 0) return fail(ctx, LFD_ERR_INVALID, "sel_offsets[0] must be 0");
        for (int r = 0; r < batch->n_refs; ++r)
            if (sel_offsets[r + 1] < sel_offsets[r]) return fail(ctx, LFD_ERR_INVALID, "sel_offsets must be non-decreasing");
    }
    LfdLaunch L;
    const long long* d_off = nullptr;
    int rc = prepare_launch(ctx, batch, params, reinterpret_cast<const long long*>(sel_offsets),
                            batch ? (size_t)std::max(batch->n_refs, 0) + 1 : 0, L, &d_off);
    if (rc != LFD_OK) return rc;
    rc = check_points(ctx, out, reinterpret_cast<long long*>(ref_offsets));
    if (rc != LFD_OK) return rc;
    const size_t n_sel = (size_t)sel_offsets[batch->n_refs];
    rc = prepare_lookback(ctx, (size_t)batch->n_refs, (size_t)batch->n_refs, false, L);
    if (rc != LFD_OK) return rc;
    rc = ensure(ctx, ctx->scratch, std::max<size_t>(n_sel, 1) * 8 * sizeof(float));
    if (rc != LFD_OK) return rc;
    rc = ensure(ctx, ctx->codes, std::max<size_t>(n_sel, 1));
    if (rc != LFD_OK) return rc;
    L.xyz = out->xyz; L.rgb = out->rgb; L.err = out->err; L.cell = out->cell; L.slot = out->slot;
    L.capacity = out->capacity;
    L.ref_offsets = reinterpret_cast<long long*>(ref_offsets);
    L.seg_counts = seg_counts;
    // pass A (the per-cell arithmetic) runs on the whole chip, one thread per selected cell; the per-reference workgroups
    // of lfd_indexed_kernel then only order and scatter.  LFD_INDEXED_SPLIT=0 keeps everything in the one kernel.
    bool split = true;
    split = ctx->env.indexed_split;
    long long max_sel = 0;
    for (int r = 0; r < batch->n_refs; ++r) max_sel = std::max<long long>(max_sel, sel_offsets[r + 1] - sel_offsets[r]);
    unsigned* tab = nullptr;
    if (split && max_sel > 0) {
        const size_t tab_bytes = (size_t)batch->n_refs * LFD_MAX_SLOTS * 2 * sizeof(unsigned);
        rc = ensure(ctx, ctx->idx_tab, tab_bytes);
        if (rc != LFD_OK) return rc;
        tab = static_cast<unsigned*>(ctx->idx_tab.ptr);
        LFD_HIP(ctx, hipMemsetAsync(tab, 0, tab_bytes, ctx->stream));
        const unsigned chunks = (unsigned)((max_sel + LFD_INDEXED_EVAL_BLOCK - 1) / LFD_INDEXED_EVAL_BLOCK);
        hipLaunchKernelGGL(lfd_indexed_eval_kernel, dim3(chunks, (unsigned)batch->n_refs), dim3(LFD_INDEXED_EVAL_BLOCK), 0, ctx->stream, L,
                           reinterpret_cast<const long long*>(sel_idx), d_off, static_cast<float*>(ctx->scratch.ptr),
                           static_cast<uint8_t*>(ctx->codes.ptr), tab, 0);
        LFD_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(lfd_indexed_kernel, dim3((unsigned)batch->n_refs), dim3(LFD_INDEXED_BLOCK), 0, ctx->stream, L,
                       reinterpret_cast<const long long*>(sel_idx), d_off, static_cast<float*>(ctx->scratch.ptr),
                       static_cast<uint8_t*>(ctx->codes.ptr), seg_order, static_cast<const unsigned*>(tab), 0);
    LFD_HIP(ctx, hipGetLastError());
    return LFD_OK;
}

// ---- S: selection ---------------------------------------------------------------------------------
int lfd_rng_seed(lfd_context* ctx, uint32_t seed) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    int rc = ensure(ctx, ctx->mt, 625 * sizeof(unsigned));
    if (rc != LFD_OK) return rc;
    hipLaunchKernelGGL(lfd_mt_seed_kernel, dim3(1), dim3(64), 0, ctx->stream, static_cast<unsigned*>(ctx->mt.ptr), seed);
    LFD_HIP(ctx, hipGetLastError());
    ctx->mt_seeded = true;
    return LFD_OK;
}

int lfd_rng_get_state(lfd_context* ctx, uint32_t* key624, int32_t* pos) {
    if (!ctx || !key624 || !pos) return fail(ctx, LFD_ERR_INVALID, "null argument");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (!ctx->mt_seeded) return fail(ctx, LFD_ERR_STATE, "lfd_rng_seed / lfd_rng_set_state must be called first");
    unsigned host[625];
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    LFD_HIP(ctx, hipMemcpyAsync(host, ctx->mt.ptr, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    LFD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(key624, host, 624 * sizeof(unsigned));
    *pos = (int32_t)host[624];
    return LFD_OK;
}

int lfd_rng_set_state(lfd_context* ctx, const uint32_t* key624, int32_t pos) {
    if (!ctx || !key624 || pos < 0 || pos > 624) return fail(ctx, LFD_ERR_INVALID, "bad MT19937 state");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    int rc = ensure(ctx, ctx->mt, 625 * sizeof(unsigned));
    if (rc != LFD_OK) return rc;
    unsigned host[625];
    std::memcpy(host, key624, 624 * sizeof(unsigned));
    host[624] = (unsigned)pos;
    LFD_HIP(ctx, hipMemcpyAsync(ctx->mt.ptr, host, sizeof(host), hipMemcpyHostToDevice, ctx->stream));
    LFD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->mt_seeded = true;
    return LFD_OK;
}

// The stream put aside / taken back in stream order (device-to-device, 2.5 KB): see the header.
static int rng_checkpoint_copy(lfd_context* ctx, int32_t place, bool take_back) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (place < 0 || place >= LFD_RNG_CHECKPOINTS) return fail(ctx, LFD_ERR_INVALID, "checkpoint place out of range");
    if (!ctx->mt_seeded) return fail(ctx, LFD_ERR_STATE, "lfd_rng_seed / lfd_rng_set_state must be called first");
    if (take_back && !(ctx->mt_ckpt_taken & (1u << place))) return fail(ctx, LFD_ERR_STATE, "no checkpoint was taken at this place");
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    int rc = ensure(ctx, ctx->mt_ckpt, (size_t)LFD_RNG_CHECKPOINTS * 640 * sizeof(unsigned));
    if (rc != LFD_OK) return rc;
    unsigned* slot = static_cast<unsigned*>(ctx->mt_ckpt.ptr) + (size_t)place * 640;
    if (take_back) LFD_HIP(ctx, hipMemcpyAsync(ctx->mt.ptr, slot, 625 * sizeof(unsigned), hipMemcpyDeviceToDevice, ctx->stream));
    else LFD_HIP(ctx, hipMemcpyAsync(slot, ctx->mt.ptr, 625 * sizeof(unsigned), hipMemcpyDeviceToDevice, ctx->stream));
    if (!take_back) ctx->mt_ckpt_taken |= 1u << place;
    return LFD_OK;
}

int lfd_rng_checkpoint(lfd_context* ctx, int32_t place) { return rng_checkpoint_copy(ctx, place, false); }
int lfd_rng_rollback(lfd_context* ctx, int32_t place) { return rng_checkpoint_copy(ctx, place, true); }

// whether a filtered selection of an N-cell map runs on the multi-workgroup kernel (the only one that can chain references on one stream)
static bool select_runs_on_several_workgroups(lfd_context* ctx, long long N) {
    int n_wg = LFD_SELECT_DEFAULT_WG;
    if (ctx->env.select_workgroups >= 0) n_wg = ctx->env.select_workgroups;
    n_wg = std::min(std::min(n_wg, (int)LFD_SELECT_MAX_WG), (int)(N / 8192));
    return n_wg >= 2 && ctx->env.select_timing == 0;
}

// launches the selection of one reference; *d_info = device {n_out, status}; nothing is read back here.
// n_batch > 1 (or info_batch set): n_batch references in ONE launch (blockIdx.y = reference) - maps best_cert + r*H*W, cells
// sel_out + r*capacity, {begin, end} pairs sel_offsets_dev + 2r, MT19937 states mt_batch + r*LFD_MT_STATE_STRIDE, results at
// info_batch + 2r; every reference has its own scratch block and barrier words, so they run side by side (a selection
// occupies 17 of the 256 CUs).
static int select_launch(lfd_context* ctx, bool topm, const float* best_cert, int32_t H, int32_t W, int32_t M, float cap,
                         int32_t border, int32_t tiles, float s_override, int64_t* sel_out, int64_t capacity,
                         long long* sel_offsets_dev, int** d_info, unsigned char** d_time, int n_batch = 1,
                         unsigned* mt_batch = nullptr, int* info_batch = nullptr, const float* s_batch = nullptr) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!best_cert || !sel_out) return fail(ctx, LFD_ERR_INVALID, "null argument");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL || M < 0 || tiles <= 0 || border < 0 || capacity < 0)
        return fail(ctx, LFD_ERR_INVALID, "bad selection arguments");
    if (!topm && !mt_batch && !ctx->mt_seeded) return fail(ctx, LFD_ERR_STATE, "lfd_rng_seed must be called before lfd_select_samples");
    if (n_batch < 1 || n_batch > LFD_SELECT_BATCH_MAX) return fail(ctx, LFD_ERR_INVALID, "bad selection batch");
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->mt.ptr) { int rc0 = ensure(ctx, ctx->mt, 625 * sizeof(unsigned)); if (rc0 != LFD_OK) return rc0; }
    const size_t N = (size_t)H * W, Mz = (size_t)std::max(M, 1);
    auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
    const size_t o_w = 0, o_p = o_w + up(N * 4), o_cdf = o_p + up(N * 8), o_first = o_cdf + up(N * 8), o_mark = o_first + up(N * 4),
                 o_draws = o_mark + up(N), o_cand = o_draws + up(Mz * 8), o_found = o_cand + up(Mz * 4), o_out = o_found + up(Mz * 4),
                 o_time = o_out + 256, o_coop = o_time + 256, total = o_coop + up(LFD_SELECT_COOP_BYTES);
    int rc = ensure(ctx, ctx->sel_scratch, total * (size_t)n_batch);
    if (rc != LFD_OK) return rc;
    unsigned char* base = static_cast<unsigned char*>(ctx->sel_scratch.ptr);
    LfdSelectArgs A;
    std::memset(&A, 0, sizeof(A));
    A.best_cert = best_cert;
    A.weights = reinterpret_cast<float*>(base + o_w);
    A.p = reinterpret_cast<double*>(base + o_p);
    A.cdf = reinterpret_cast<double*>(base + o_cdf);
    A.first = reinterpret_cast<int*>(base + o_first);
    A.mark = base + o_mark;
    A.draws = reinterpret_cast<double*>(base + o_draws);
    A.cand = reinterpret_cast<int*>(base + o_cand);
    A.found = reinterpret_cast<int*>(base + o_found);
    A.mt = mt_batch ? mt_batch : static_cast<unsigned*>(ctx->mt.ptr);
    A.batch_scratch_stride = (long long)total;
    A.batch_cert_stride = (long long)N;
    A.batch_out_stride = (long long)capacity;
    A.batch_mt_stride = mt_batch ? LFD_MT_STATE_STRIDE : 0;
    A.batch_info = info_batch;
    A.sel_out = reinterpret_cast<long long*>(sel_out);
    A.n_out = reinterpret_cast<int*>(base + o_out);
    A.status = reinterpret_cast<int*>(base + o_out + 4);
    A.capacity = capacity;
    A.H = H; A.W = W; A.M = M; A.border = border; A.tiles = tiles; A.cap = cap; A.s_override = s_override;
    A.sel_offsets_out = sel_offsets_dev;
    LfdSelectNorms norms;
    std::memset(&norms, 0, sizeof(norms));
    if (s_batch) {
        norms.use = 1;
        for (int i = 0; i < n_batch; ++i) norms.s[i] = s_batch[i];
    }
    *d_info = reinterpret_cast<int*>(base + o_out);
    *d_time = nullptr;
    const bool timing = !topm && n_batch == 1 && ctx->env.select_timing != 0;
    if (timing) {
        A.timing = reinterpret_cast<unsigned long long*>(base + o_time);
        LFD_HIP(ctx, hipMemsetAsync(base + o_time, 0, 256, ctx->stream));
        *d_time = base + o_time;
    }
    if (topm) {
        const size_t lds = (size_t)LFD_SELECT_TOPM_MAX * sizeof(unsigned long long);
        if (!ctx->topm_lds_attr_set) {     // after hipSetDevice(ctx->device) above: the attribute belongs to this context's device
            LFD_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(lfd_select_topm_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            ctx->topm_lds_attr_set = true;
        }
        hipLaunchKernelGGL(lfd_select_topm_kernel, dim3(1, (unsigned)n_batch), dim3(LFD_SELECT_BLOCK), lds, ctx->stream, A);
    } else {
        // several workgroups (one per CU) when the map is large enough to share out; LFD_SELECT_WORKGROUPS=0 keeps the
        // single-workgroup kernel (both produce the same selection)
        int n_wg = LFD_SELECT_DEFAULT_WG;
        if (ctx->env.select_workgroups >= 0) n_wg = ctx->env.select_workgroups;
        n_wg = std::min(std::min(n_wg, (int)LFD_SELECT_MAX_WG), (int)(N / 8192));
        {
            const int tile = std::max(1, W / tiles);
            const long long nbins = (long long)((W - 1) / tile + 1) * ((H - 1) / tile + 1);
            if (nbins > LFD_SELECT_MAX_BINS)
                return fail(ctx, LFD_ERR_INVALID, "selection: too many coverage bins: a " + std::to_string(H) + " x " + std::to_string(W) + " grid with " +
                            std::to_string(tiles) + " tiles per side has " + std::to_string(nbins) + " coverage tiles, the device stage holds " +
                            std::to_string((int)LFD_SELECT_MAX_BINS) + " (every square grid fits; RoMa's, 320 ... 1280 cells per side, have 576 ... 625); the host selection "
                            "stage (selection_backend=\"host\" in the Python mirror: upstream's own library calls) has no such limit");
        }
        const bool timing_mw = timing && ctx->env.select_timing == 2;     // 2: stamps of workgroup 0 of the multi-workgroup kernel
        const bool several_wg = n_wg >= 2 && (!timing || timing_mw);
        const bool one_stream = mt_batch == nullptr;              // the references of the launch share the context's stream, in batch order
        if (one_stream && n_batch > 1 && !several_wg)
            return fail(ctx, LFD_ERR_STATE, "selection: several references on one stream need the multi-workgroup kernel");
        if (several_wg) {
            // the stream as an array (lfd_select.hip, mt_stream_producer): a ring of doubles four first rounds long (later rounds are shorter than
            // the first, the producer stays at most one first round ahead) and the key of every twist the producer can be ahead by - one set for
            // the launch when its references share a stream, one per reference when every reference has its own
            const long long first_round = std::max<long long>(std::min<long long>((long long)((double)M * 0.85), (long long)N), 1);
            long long ring_cap = 4096;
            while (ring_cap < 4 * first_round) ring_cap *= 2;
            const int snap_slots = (int)(2 * ring_cap / 624) + 8;
            const size_t o_ring = LFD_CHAIN_BYTES, o_snaps = o_ring + (size_t)ring_cap * 8,
                         chain_total = (o_snaps + (size_t)snap_slots * 624 * 4 + 255) & ~size_t(255);
            const int n_chains = one_stream ? 1 : n_batch;
            rc = ensure(ctx, ctx->sel_chain, chain_total * (size_t)n_chains);
            if (rc != LFD_OK) return rc;
            unsigned char* cb = static_cast<unsigned char*>(ctx->sel_chain.ptr);
            if (n_chains == 1) LFD_HIP(ctx, hipMemsetAsync(cb, 0, LFD_CHAIN_BYTES, ctx->stream));
            else LFD_HIP(ctx, hipMemset2DAsync(cb, chain_total, 0, LFD_CHAIN_BYTES, (size_t)n_chains, ctx->stream));
            A.chain = cb;
            A.ring = reinterpret_cast<double*>(cb + o_ring);
            A.snaps = reinterpret_cast<unsigned*>(cb + o_snaps);
            A.ring_cap = ring_cap;
            A.snap_slots = snap_slots;
            A.chain_refs = one_stream ? n_batch : 1;
            A.batch_chain_stride = one_stream ? 0 : (long long)chain_total;
        }
        if (several_wg) {
            A.coop = base + o_coop;
            A.n_wg = n_wg;
            // barrier words, flags and the coverage bins (everything in front of LFD_COOP_MT)
            if (n_batch == 1) LFD_HIP(ctx, hipMemsetAsync(base + o_coop, 0, LFD_COOP_MT, ctx->stream));
            else LFD_HIP(ctx, hipMemset2DAsync(base + o_coop, total, 0, LFD_COOP_MT, (size_t)n_batch, ctx->stream));
            hipLaunchKernelGGL(lfd_select_filter_mw_kernel, dim3((unsigned)n_wg + 1u, (unsigned)n_batch), dim3(LFD_SELECT_BLOCK), 0, ctx->stream, A, norms);
        } else {
            hipLaunchKernelGGL(lfd_select_filter_kernel, dim3(1, (unsigned)n_batch), dim3(LFD_SELECT_BLOCK), 0, ctx->stream, A);
        }
    }
    LFD_HIP(ctx, hipGetLastError());
    return LFD_OK;
}

static const char* select_status_name(int st) {
    static const char* names[] = {"ok", "probabilities contain NaN", "probabilities are not non-negative",
                                  "Fewer non-zero entries in p than size", "weight below 2^-29: exact parallel cumsum not guaranteed",
                                  "no progress", "too many coverage bins", "sel_out capacity too small"};
    return names[std::min(std::max(st, 0), 7)];
}

static int select_impl(lfd_context* ctx, bool topm, const float* best_cert, int32_t H, int32_t W, int32_t M, float cap,
                       int32_t border, int32_t tiles, float s_override, int64_t* sel_out, int64_t capacity,
                       int32_t* n_sel_host, int32_t* status_host) {
    if (ctx && (!n_sel_host || !status_host)) return fail(ctx, LFD_ERR_INVALID, "null argument");
    int* d_info = nullptr;
    unsigned char* d_time = nullptr;
    int rc = select_launch(ctx, topm, best_cert, H, W, M, cap, border, tiles, s_override, sel_out, capacity, nullptr, &d_info, &d_time);
    if (rc != LFD_OK) return rc;
    int* host = ctx->pinned_words + 4;
    LFD_HIP(ctx, hipMemcpyAsync(host, d_info, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    LFD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_sel_host = host[0];
    *status_host = host[1];
    if (d_time) {   // phase times of the filter kernel (100 MHz wall clock), profiling only
        unsigned long long t[32];
        LFD_HIP(ctx, hipMemcpy(t, d_time, sizeof(t), hipMemcpyDeviceToHost));
        fprintf(stderr, "[lfd] select phases (us):");
        for (int i = 1; i < 30 && t[i]; ++i) fprintf(stderr, " %.1f", (double)(t[i] - t[i - 1]) * 0.01);
        if (t[30]) fprintf(stderr, " | stream workgroup: start +%.1f, first draws ready +%.1f", (double)((long long)t[30] - (long long)t[0]) * 0.01, (double)((long long)t[31] - (long long)t[0]) * 0.01);
        fprintf(stderr, "\n");
    }
    if (host[1] != LFD_SELECT_OK)
        return fail(ctx, host[1] == LFD_SELECT_CAPACITY ? LFD_ERR_CAPACITY : LFD_ERR_INVALID,
                    std::string("selection: ") + select_status_name(host[1]));
    return LFD_OK;
}

// seeds: one MT19937 stream per reference (lfd_triangulate_sampled_multi).  chain: all references on the CONTEXT's stream, consumed in batch order
// (lfd_triangulate_sampled_chain; s_chain: their normalisers, or null).  Neither: one reference on the context's stream.
static int sampled_impl(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params, int32_t M, float cap, int32_t border, int32_t tiles,
                        float s_override, const uint32_t* seeds, const lfd_points* out, int64_t* ref_offsets, int32_t* seg_counts,
                        int32_t* seg_order, int32_t* sel_info, int64_t* sel_cells, bool chain = false, const float* s_chain = nullptr) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (!batch || !params || !sel_info) return fail(ctx, LFD_ERR_INVALID, "null argument");
    const int R = batch->n_refs;
    if (R != 1 && !seeds && !chain) return fail(ctx, LFD_ERR_INVALID, "lfd_triangulate_sampled takes one reference view per call (several: lfd_triangulate_sampled_chain on the context's stream, lfd_triangulate_sampled_multi on per-reference streams)");
    if (R < 1) return fail(ctx, LFD_ERR_INVALID, "no reference view");
    if (M < 0 || tiles <= 0 || border < 0) return fail(ctx, LFD_ERR_INVALID, "bad selection arguments");
    const bool topm = params->no_filter != 0;
    if (topm && M > LFD_SELECT_TOPM_MAX) return fail(ctx, LFD_ERR_INVALID, "no_filter selection is limited to 16384 matches per reference");
    LfdLaunch L;
    int rc = prepare_launch(ctx, batch, params, nullptr, 0, L, nullptr);
    if (rc != LFD_OK) return rc;
    rc = check_points(ctx, out, reinterpret_cast<long long*>(ref_offsets));
    if (rc != LFD_OK) return rc;
    const long long HW = (long long)batch->H * batch->W;
    const long long cap_sel = topm ? std::max<long long>(std::min<long long>(M, HW), 1) : (long long)M + (long long)tiles * tiles + 64;
    if (out->capacity < cap_sel * R) return fail(ctx, LFD_ERR_CAPACITY, "output capacity below (M + tiles*tiles + 64) per reference");
    // P1 + F1 for every reference of the batch in one launch
    rc = ensure(ctx, ctx->agg, (size_t)HW * (size_t)R * sizeof(float));
    if (rc != LFD_OK) return rc;
    float* best = static_cast<float*>(ctx->agg.ptr);
    {
        const int per_block = 256 * 4;
        const int gx = (int)std::min<long long>((HW + per_block - 1) / per_block, 2048);
        hipLaunchKernelGGL(lfd_aggregate_kernel, dim3((unsigned)gx, (unsigned)R, 1u), dim3(256), 0, ctx->stream, L, best, static_cast<uint8_t*>(nullptr));
        LFD_HIP(ctx, hipGetLastError());
    }
    // S, reference after reference (the selection kernels share one scratch area): the counts stay on the device as {begin, end}
    // pairs for the kernels below; every reference's cells sit at a fixed stride
    rc = ensure(ctx, ctx->sel_buf, (size_t)R * 16 + (size_t)cap_sel * (size_t)R * sizeof(long long));
    if (rc != LFD_OK) return rc;
    long long* sel_pairs = static_cast<long long*>(ctx->sel_buf.ptr);
    long long* cells = sel_cells ? reinterpret_cast<long long*>(sel_cells) : sel_pairs + 2 * (size_t)R;
    if (R == 1) {
        LFD_HIP(ctx, hipMemsetAsync(sel_pairs, 0, 16, ctx->stream));
    } else {
        // (written on the device: a copy from a host vector had to be waited for - a drain of the stream inside every grouped call, which kept the
        // caller from running ahead of the device)
        hipLaunchKernelGGL(lfd_select_begins_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, ctx->stream, sel_pairs, (long long)cap_sel, R);
        LFD_HIP(ctx, hipGetLastError());
    }
    if (!seeds && (topm || select_runs_on_several_workgroups(ctx, HW)) && R > 1) {
        // the context's stream, R references in ONE launch per LFD_SELECT_BATCH_MAX of them: everything that does not depend on the stream runs
        // side by side, a reference starts drawing where the one before it stopped (no_filter draws nothing: plain side by side)
        if (!topm && !ctx->mt_seeded) return fail(ctx, LFD_ERR_STATE, "lfd_rng_seed must be called before lfd_triangulate_sampled_chain");
        for (int r0 = 0; r0 < R; r0 += LFD_SELECT_BATCH_MAX) {
            const int nb = std::min(R - r0, (int)LFD_SELECT_BATCH_MAX);
            int* d_info = nullptr;
            unsigned char* d_time = nullptr;
            rc = select_launch(ctx, topm, best + (size_t)r0 * HW, batch->H, batch->W, M, cap, topm ? 0 : border, topm ? 1 : tiles, 0.0f,
                               reinterpret_cast<int64_t*>(cells + (size_t)r0 * cap_sel), cap_sel, sel_pairs + 2 * (size_t)r0, &d_info, &d_time,
                               nb, nullptr, sel_info + 2 * (size_t)r0, (s_chain && !topm) ? s_chain + r0 : nullptr);
            if (rc != LFD_OK) return rc;
        }
    } else if (!seeds) {     // the context's MT19937 stream (upstream's single global stream), reference after reference
        for (int r = 0; r < R; ++r) {
            int* d_info = nullptr;
            unsigned char* d_time = nullptr;
            const float s_r = topm ? 0.0f : (s_chain ? s_chain[r] : s_override);
            rc = select_launch(ctx, topm, best + (size_t)r * HW, batch->H, batch->W, M, cap, topm ? 0 : border, topm ? 1 : tiles, s_r,
                               reinterpret_cast<int64_t*>(cells + (size_t)r * cap_sel), cap_sel, sel_pairs + 2 * (size_t)r, &d_info, &d_time);
            if (rc != LFD_OK) return rc;
            LFD_HIP(ctx, hipMemcpyAsync(sel_info + 2 * (size_t)r, d_info, 2 * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
        }
    } else {                 // every reference on its own stream: up to LFD_SELECT_BATCH_MAX selections side by side per launch
        rc = ensure(ctx, ctx->mt_batch, (size_t)LFD_SELECT_BATCH_MAX * LFD_MT_STATE_STRIDE * sizeof(unsigned));
        if (rc != LFD_OK) return rc;
        unsigned* mtb = static_cast<unsigned*>(ctx->mt_batch.ptr);
        for (int r0 = 0; r0 < R; r0 += LFD_SELECT_BATCH_MAX) {
            const int nb = std::min(R - r0, (int)LFD_SELECT_BATCH_MAX);
            if (!topm) {
                LfdSeedBatch sb;
                std::memset(&sb, 0, sizeof(sb));
                for (int i = 0; i < nb; ++i) sb.seed[i] = seeds[r0 + i];
                hipLaunchKernelGGL(lfd_mt_seed_batch_kernel, dim3((unsigned)nb), dim3(64), 0, ctx->stream, mtb, sb);
                LFD_HIP(ctx, hipGetLastError());
            }
            int* d_info = nullptr;
            unsigned char* d_time = nullptr;
            rc = select_launch(ctx, topm, best + (size_t)r0 * HW, batch->H, batch->W, M, cap, topm ? 0 : border, topm ? 1 : tiles, 0.0f,
                               reinterpret_cast<int64_t*>(cells + (size_t)r0 * cap_sel), cap_sel, sel_pairs + 2 * (size_t)r0, &d_info, &d_time,
                               nb, mtb, sel_info + 2 * (size_t)r0);
            if (rc != LFD_OK) return rc;
        }
    }
    // F2..F10 on the selected cells of all references
    rc = prepare_lookback(ctx, (size_t)R, (size_t)R, false, L);
    if (rc != LFD_OK) return rc;
    rc = ensure(ctx, ctx->scratch, (size_t)cap_sel * (size_t)R * 8 * sizeof(float));
    if (rc != LFD_OK) return rc;
    rc = ensure(ctx, ctx->codes, (size_t)cap_sel * (size_t)R);
    if (rc != LFD_OK) return rc;
    const size_t tab_bytes = (size_t)R * LFD_MAX_SLOTS * 2 * sizeof(unsigned);
    rc = ensure(ctx, ctx->idx_tab, tab_bytes);
    if (rc != LFD_OK) return rc;
    unsigned* tab = static_cast<unsigned*>(ctx->idx_tab.ptr);
    LFD_HIP(ctx, hipMemsetAsync(tab, 0, tab_bytes, ctx->stream));
    L.xyz = out->xyz; L.rgb = out->rgb; L.err = out->err; L.cell = out->cell; L.slot = out->slot;
    L.capacity = out->capacity;
    L.ref_offsets = reinterpret_cast<long long*>(ref_offsets);
    L.seg_counts = seg_counts;
    const unsigned chunks = (unsigned)((cap_sel + LFD_INDEXED_EVAL_BLOCK - 1) / LFD_INDEXED_EVAL_BLOCK);
    hipLaunchKernelGGL(lfd_indexed_eval_kernel, dim3(chunks, (unsigned)R), dim3(LFD_INDEXED_EVAL_BLOCK), 0, ctx->stream, L,
                       static_cast<const long long*>(cells), static_cast<const long long*>(sel_pairs), static_cast<float*>(ctx->scratch.ptr),
                       static_cast<uint8_t*>(ctx->codes.ptr), tab, 1);
    LFD_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(lfd_indexed_kernel, dim3((unsigned)R), dim3(LFD_INDEXED_BLOCK), 0, ctx->stream, L,
                       static_cast<const long long*>(cells), static_cast<const long long*>(sel_pairs), static_cast<float*>(ctx->scratch.ptr),
                       static_cast<uint8_t*>(ctx->codes.ptr), seg_order, static_cast<const unsigned*>(tab), 1);
    LFD_HIP(ctx, hipGetLastError());
    // the look-back status word of this launch rides along with the counts: one read-back tells the caller everything
    LFD_HIP(ctx, hipMemcpyAsync(sel_info + 2 * (size_t)R, static_cast<unsigned char*>(ctx->ws.ptr) + 8, sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
    return LFD_OK;
}

int lfd_triangulate_sampled(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params, int32_t M, float cap,
                            int32_t border, int32_t tiles, float s_override, const lfd_points* out, int64_t* ref_offsets,
                            int32_t* seg_counts, int32_t* seg_order, int32_t* sel_info, int64_t* sel_cells) {
    if (ctx && batch && batch->n_refs != 1) return fail(ctx, LFD_ERR_INVALID, "lfd_triangulate_sampled takes one reference view per call");
    return sampled_impl(ctx, batch, params, M, cap, border, tiles, s_override, nullptr, out, ref_offsets, seg_counts, seg_order, sel_info, sel_cells);
}

int lfd_triangulate_sampled_chain(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params, int32_t M, float cap,
                                  int32_t border, int32_t tiles, const float* s_overrides, const lfd_points* out, int64_t* ref_offsets,
                                  int32_t* seg_counts, int32_t* seg_order, int32_t* sel_info, int64_t* sel_cells) {
    return sampled_impl(ctx, batch, params, M, cap, border, tiles, 0.0f, nullptr, out, ref_offsets, seg_counts, seg_order, sel_info, sel_cells, true, s_overrides);
}

int lfd_triangulate_sampled_multi(lfd_context* ctx, const lfd_batch* batch, const lfd_params* params, int32_t M, float cap,
                                  int32_t border, int32_t tiles, const uint32_t* seeds, const lfd_points* out, int64_t* ref_offsets,
                                  int32_t* seg_counts, int32_t* seg_order, int32_t* sel_info, int64_t* sel_cells) {
    if (ctx && !seeds) return fail(ctx, LFD_ERR_INVALID, "seeds is required: every reference draws from its own MT19937 stream");
    return sampled_impl(ctx, batch, params, M, cap, border, tiles, 0.0f, seeds, out, ref_offsets, seg_counts, seg_order, sel_info, sel_cells);
}

int lfd_select_samples(lfd_context* ctx, const float* best_cert, int32_t H, int32_t W, int32_t M, float cap,
                       int32_t border, int32_t tiles, float s_override, int64_t* sel_out, int64_t capacity,
                       int32_t* n_sel_host, int32_t* status_host) {
    return select_impl(ctx, false, best_cert, H, W, M, cap, border, tiles, s_override, sel_out, capacity, n_sel_host, status_host);
}

int lfd_select_top_m(lfd_context* ctx, const float* best_cert, int32_t H, int32_t W, int32_t M, float cap,
                     int64_t* sel_out, int64_t capacity, int32_t* n_sel_host, int32_t* status_host) {
    return select_impl(ctx, true, best_cert, H, W, M, cap, 0, 1, 0.0f, sel_out, capacity, n_sel_host, status_host);
}

// ---- N1: writers ----------------------------------------------------------------------------------
int lfd_pack_ply(lfd_context* ctx, const float* xyz, const float* rgb, int64_t n, uint8_t* out) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (n < 0 || (n > 0 && (!xyz || !rgb || !out))) return fail(ctx, LFD_ERR_INVALID, "bad arguments");
    if (reinterpret_cast<uintptr_t>(out) & 3u) return fail(ctx, LFD_ERR_INVALID, "out must be 4-byte aligned");
    if (n == 0) return LFD_OK;
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(lfd_pack_ply_kernel, dim3(grid), dim3(256), 0, ctx->stream, xyz, rgb, (long long)n, out);
    LFD_HIP(ctx, hipGetLastError());
    return LFD_OK;
}

int lfd_pack_ply_normals(lfd_context* ctx, const float* xyz, const float* normals, const float* rgb, int64_t n, uint8_t* out) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (n < 0 || (n > 0 && (!xyz || !normals || !rgb || !out))) return fail(ctx, LFD_ERR_INVALID, "bad arguments");
    if (reinterpret_cast<uintptr_t>(out) & 3u) return fail(ctx, LFD_ERR_INVALID, "out must be 4-byte aligned");
    if (n == 0) return LFD_OK;
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(lfd_pack_ply_normals_kernel, dim3(grid), dim3(256), 0, ctx->stream, xyz, normals, rgb, (long long)n, out);
    LFD_HIP(ctx, hipGetLastError());
    return LFD_OK;
}

int lfd_pack_points3d(lfd_context* ctx, const float* xyz, const float* rgb, const float* err, int64_t n, uint64_t id_base,
                      uint8_t* out) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (n < 0 || (n > 0 && (!xyz || !rgb || !out))) return fail(ctx, LFD_ERR_INVALID, "bad arguments");
    if (reinterpret_cast<uintptr_t>(out) & 3u) return fail(ctx, LFD_ERR_INVALID, "out must be 4-byte aligned");
    if (n == 0) return LFD_OK;
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(lfd_pack_points3d_kernel, dim3(grid), dim3(256), 0, ctx->stream, xyz, rgb, err, (long long)n,
                       (unsigned long long)id_base, out);
    LFD_HIP(ctx, hipGetLastError());
    return LFD_OK;
}

// ---- the distance filter (lfd_voxel.hip) -----------------------------------------------------------------------------------------------
int lfd_voxel_downsample(lfd_context* ctx, const float* xyz, const float* rgb, int64_t n, double voxel_size, float* xyz_out, float* rgb_out,
                         int64_t* n_out_host) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (!n_out_host || n < 0 || (n > 0 && (!xyz || !rgb || !xyz_out || !rgb_out))) return fail(ctx, LFD_ERR_INVALID, "lfd_voxel_downsample: bad arguments");
    if (!(voxel_size > 0.0) || !std::isfinite(voxel_size)) return fail(ctx, LFD_ERR_INVALID, "lfd_voxel_downsample: voxel_size must be finite and > 0");
    if (n > 0x7fffffffLL) return fail(ctx, LFD_ERR_INVALID, "lfd_voxel_downsample: at most 2^31 - 1 points");
    *n_out_host = 0;
    if (n == 0) return LFD_OK;
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const CloudPlan p = cloud_plan(n);
    CloudSort w;                                                       // counters: voxel count, big-voxel count
    unsigned* big = nullptr;                                           // big-voxel list
    if (int rc = carve_cloud_ws(ctx, [&](Bump& b) {
            w = carve_sort(b, p.n, 2, true);
            big = b.take<unsigned>((size_t)n / (LFD_VOX_BIG + 1) + 1);
        }))
        return rc;
    unsigned *nv_dev = w.counters, *n_big = w.counters + 1;

    // the refusals are decided before anything is sorted
    LfdVoxStats s;
    if (int rc = cloud_stats(ctx, p, w, xyz, rgb, s)) return rc;
    if (s.flags & LFD_VOX_NONFINITE) return fail(ctx, LFD_ERR_INVALID, "lfd_voxel_downsample: " LFD_FUSE_NONFINITE);
    LfdFuseGrid g;
    if (!lfd_fuse_grid(s.lo, s.hi, voxel_size, g)) return fail(ctx, LFD_ERR_INVALID, "lfd_voxel_downsample: " LFD_FUSE_KEY_RANGE);
    const double cscale = lfd_fuse_cscale(s.cmax, (s.flags & LFD_VOX_NAN_RGB) != 0u);

    hipLaunchKernelGGL(lfd_voxel_keys_kernel, dim3(p.grid), dim3(256), 0, st, xyz, p.n, g.origin[0], g.origin[1], g.origin[2], voxel_size, g.e[1],
                       g.e[2], w.keys[0], w.idx[0]);
    const int cur = cloud_sort(st, p, w, g.bits);
    cloud_heads_count(st, p, w, cur);
    cloud_heads_scatter(st, p, w, cur);
    LFD_HIP(ctx, hipMemsetAsync(n_big, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(lfd_voxel_sums_kernel, dim3(p.grid), dim3(256), 0, st, xyz, rgb, p.n, w.idx[cur], w.vstart, nv_dev, cscale, xyz_out, rgb_out,
                       big, n_big);
    const unsigned big_grid = (unsigned)std::min<long long>(n / (LFD_VOX_BIG + 1) + 1, 8192);
    hipLaunchKernelGGL(lfd_voxel_sums_big_kernel, dim3(big_grid), dim3(64), 0, st, xyz, rgb, p.n, w.idx[cur], w.vstart, nv_dev, cscale, big, n_big,
                       xyz_out, rgb_out);
    LFD_HIP(ctx, hipGetLastError());
    LFD_HIP(ctx, hipMemcpyAsync(ctx->pinned_words, nv_dev, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    LFD_HIP(ctx, hipStreamSynchronize(st));
    *n_out_host = (int64_t)(unsigned)ctx->pinned_words[0];
    return LFD_OK;
}

// ---- cross-reference consensus filter on the final cloud (lfd_consensus.hip) --------------------------------------------------------------------
int lfd_consensus_filter(lfd_context* ctx, const float* xyz, const float* rgb, const float* err, int64_t n, const int64_t* ref_offsets_host,
                         int32_t n_refs, float radius, int32_t min_refs, float* xyz_out, float* rgb_out, float* err_out,
                         int64_t* ref_offsets_out_host, uint8_t* consensus, int64_t* n_out_host) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (const char* why = lfd_consensus_check(xyz, rgb, err, n, ref_offsets_host, n_refs, radius, min_refs, xyz_out, rgb_out, err_out,
                                              ref_offsets_out_host, consensus, n_out_host))
        return fail(ctx, LFD_ERR_INVALID, std::string("lfd_consensus_filter: ") + why);
    for (int32_t r = 0; r <= n_refs; ++r) ref_offsets_out_host[r] = 0;
    *n_out_host = 0;
    if (n == 0) return LFD_OK;
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const CloudPlan p = cloud_plan(n);
    CloudSort w;
    LfdConsensusPt* spt = nullptr;                                     // sorted points
    CloudCompact c;
    if (int rc = carve_cloud_ws(ctx, [&](Bump& b) {
            w = carve_sort(b, p.n, 0, false);
            spt = b.take<LfdConsensusPt>((size_t)n);
            c = carve_compact(b, p, n_refs);
        }))
        return rc;

    // min / max over the finite points; the key-range refusal is decided before anything is sorted
    LFD_HIP(ctx, hipMemcpyAsync(c.offs, ref_offsets_host, ((size_t)n_refs + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    LfdVoxStats s;
    if (int rc = cloud_stats(ctx, p, w, xyz, nullptr, s)) return rc;
    if (!(s.lo[0] <= s.hi[0])) {                                   // no finite point: nothing agrees with anything
        if (consensus) LFD_HIP(ctx, hipMemsetAsync(consensus, 0, (size_t)n, st));
        LFD_HIP(ctx, hipStreamSynchronize(st));
        return LFD_OK;
    }
    LfdConsensusGrid g;
    if (!lfd_consensus_grid(s.lo, s.hi, radius, g))
        return fail(ctx, LFD_ERR_INVALID, "lfd_consensus_filter: key range: more than 2^30 cells along an axis or a linear cell key beyond 63 bits");

    hipLaunchKernelGGL(lfd_consensus_keys_kernel, dim3(p.grid), dim3(256), 0, st, xyz, p.n, g.origin[0], g.origin[1], g.origin[2], g.h, g.e[1],
                       g.e[2], g.sentinel, w.keys[0], w.idx[0]);
    const int cur = cloud_sort(st, p, w, g.bits);
    hipLaunchKernelGGL(lfd_consensus_gather_kernel, dim3(p.grid), dim3(256), 0, st, xyz, w.idx[cur], c.offs, (int)n_refs, p.n, spt);
    hipLaunchKernelGGL(lfd_consensus_count_kernel, dim3((unsigned)p.n_wg), dim3(256), 0, st, w.keys[cur], spt, w.idx[cur], p.n, g.e[1], g.e[2],
                       g.sentinel, lfd_consensus_r2(radius), (int)min_refs, consensus ? LFD_CONSENSUS_CAP : (int)min_refs, c.keep, consensus);
    return cloud_compact(ctx, p, c, xyz, rgb, err, n_refs, xyz_out, rgb_out, err_out, ref_offsets_out_host, n_out_host);
}

// ---- connected-component filter on the final cloud (lfd_component.hip) ---------------------------------------------------------------------------
int lfd_component_filter(lfd_context* ctx, const float* xyz, const float* rgb, const float* err, int64_t n, const int64_t* ref_offsets_host,
                         int32_t n_refs, float radius, int32_t min_points, float* xyz_out, float* rgb_out, float* err_out,
                         int64_t* ref_offsets_out_host, uint32_t* size, uint32_t* label, int64_t* summary_host, int64_t* n_out_host) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (const char* why = lfd_component_check(xyz, rgb, err, n, ref_offsets_host, n_refs, radius, min_points, xyz_out, rgb_out, err_out,
                                              ref_offsets_out_host, size, label, n_out_host))
        return fail(ctx, LFD_ERR_INVALID, std::string("lfd_component_filter: ") + why);
    for (int32_t r = 0; r <= n_refs; ++r) ref_offsets_out_host[r] = 0;
    *n_out_host = 0;
    if (summary_host) std::memset(summary_host, 0, LFD_COMPONENT_SUMMARY * sizeof(int64_t));
    if (n == 0) return LFD_OK;
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const CloudPlan p = cloud_plan(n);
    CloudSort w;
    LfdComponentPt* spt = nullptr;                                     // sorted points
    uint32_t *parent = nullptr, *root = nullptr, *count = nullptr, *first = nullptr;      // per sorted position
    unsigned long long* summary = nullptr;
    CloudCompact c;
    if (int rc = carve_cloud_ws(ctx, [&](Bump& b) {
            w = carve_sort(b, p.n, 0, false);
            spt = b.take<LfdComponentPt>((size_t)n);
            parent = b.take<uint32_t>((size_t)n);
            root = b.take<uint32_t>((size_t)n);
            count = b.take<uint32_t>((size_t)n);
            first = b.take<uint32_t>((size_t)n);
            summary = b.take<unsigned long long>(LFD_COMPONENT_SUMMARY);
            c = carve_compact(b, p, n_refs);
        }))
        return rc;

    // min / max over the finite points; the key-range refusal is decided before anything is sorted
    LFD_HIP(ctx, hipMemcpyAsync(c.offs, ref_offsets_host, ((size_t)n_refs + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    LfdVoxStats s;
    if (int rc = cloud_stats(ctx, p, w, xyz, nullptr, s)) return rc;
    LfdConsensusGrid g;
    if (!lfd_component_grid(s.lo, s.hi, radius, g))
        return fail(ctx, LFD_ERR_INVALID, "lfd_component_filter: key range: more than 2^30 cells along an axis or a linear cell key beyond 63 bits");

    hipLaunchKernelGGL(lfd_consensus_keys_kernel, dim3(p.grid), dim3(256), 0, st, xyz, p.n, g.origin[0], g.origin[1], g.origin[2], g.h, g.e[1],
                       g.e[2], g.sentinel, w.keys[0], w.idx[0]);
    const int cur = cloud_sort(st, p, w, g.bits);
    const dim3 wgs((unsigned)p.n_wg);
    hipLaunchKernelGGL(lfd_component_gather_kernel, dim3(p.grid), dim3(256), 0, st, xyz, w.idx[cur], p.n, spt, parent, count, first, summary);
    hipLaunchKernelGGL(lfd_component_link_kernel, wgs, dim3(256), 0, st, w.keys[cur], spt, p.n, g.e[1], g.e[2], g.sentinel, lfd_consensus_r2(radius),
                       parent);
    hipLaunchKernelGGL(lfd_component_flatten_kernel, wgs, dim3(256), 0, st, parent, p.n, root);
    hipLaunchKernelGGL(lfd_component_size_kernel, wgs, dim3(256), 0, st, root, spt, p.n, ctx->env.component_plain_size ? 0 : 1, count, first);
    hipLaunchKernelGGL(lfd_component_mark_kernel, wgs, dim3(256), 0, st, root, spt, count, first, p.n, (uint32_t)min_points, c.keep, size, label,
                       summary);
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the summary is copied word for word");
    if (summary_host)                                                  // (every word is below 2^63; cloud_compact waits for the stream)
        LFD_HIP(ctx, hipMemcpyAsync(summary_host, summary, LFD_COMPONENT_SUMMARY * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    return cloud_compact(ctx, p, c, xyz, rgb, err, n_refs, xyz_out, rgb_out, err_out, ref_offsets_out_host, n_out_host);
}

// ---- free-space filter on the final cloud (lfd_freespace.hip) ------------------------------------------------------------------------------------
int lfd_freespace_filter(lfd_context* ctx, const float* xyz, const float* rgb, const float* err, int64_t n, const int64_t* ref_offsets_host,
                         int32_t n_refs, const float* cam_P_host, const int32_t* cam_wh_host, int32_t pw, int32_t ph, float tol,
                         int32_t min_violations, float* xyz_out, float* rgb_out, float* err_out, int64_t* ref_offsets_out_host,
                         uint8_t* violations, uint8_t* supports, int64_t* n_out_host) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (const char* why = lfd_freespace_check(xyz, rgb, err, n, ref_offsets_host, n_refs, cam_P_host, cam_wh_host, pw, ph, tol, min_violations,
                                              xyz_out, rgb_out, err_out, ref_offsets_out_host, violations, supports, n_out_host))
        return fail(ctx, LFD_ERR_INVALID, std::string("lfd_freespace_filter: ") + why);
    for (int32_t r = 0; r <= n_refs; ++r) ref_offsets_out_host[r] = 0;
    *n_out_host = 0;
    if (n == 0) return LFD_OK;
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const CloudPlan p = cloud_plan(n);
    const long long n_words = (long long)n_refs * pw * ph;             // <= 2^31 - 1 (lfd_freespace_check)
    std::vector<LfdFreespaceCam> cams((size_t)n_refs);
    for (int32_t r = 0; r < n_refs; ++r) lfd_freespace_cam(cam_P_host + 12 * (size_t)r, cam_wh_host[2 * r], cam_wh_host[2 * r + 1], cams[(size_t)r]);
    uint32_t* zbuf = nullptr;                                          // the references' z-buffers, filled before they are read
    LfdFreespaceCam* d_cams = nullptr;
    CloudCompact c;
    if (int rc = carve_cloud_ws(ctx, [&](Bump& b) {
            zbuf = b.take<uint32_t>((size_t)n_words);
            d_cams = b.take<LfdFreespaceCam>((size_t)n_refs);
            c = carve_compact(b, p, n_refs);
        }))
        return rc;

    LFD_HIP(ctx, hipMemcpyAsync(c.offs, ref_offsets_host, ((size_t)n_refs + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    LFD_HIP(ctx, hipMemcpyAsync(d_cams, cams.data(), (size_t)n_refs * sizeof(LfdFreespaceCam), hipMemcpyHostToDevice, st));
    LFD_HIP(ctx, hipStreamSynchronize(st));                            // `cams` is pageable memory of this call: the copy has read it
    hipLaunchKernelGGL(lfd_freespace_fill_kernel, dim3((unsigned)std::min<long long>((n_words + 255) / 256, 4096)), dim3(256), 0, st, zbuf, n_words);
    hipLaunchKernelGGL(lfd_freespace_splat_kernel, dim3((unsigned)p.n_wg), dim3(256), 0, st, xyz, p.n, c.offs, (int)n_refs, d_cams, (int)pw, (int)ph,
                       zbuf);
    hipLaunchKernelGGL(lfd_freespace_count_kernel, dim3((unsigned)p.n_wg), dim3(256), 0, st, xyz, p.n, c.offs, (int)n_refs, d_cams, zbuf, (int)pw,
                       (int)ph, tol, (int)min_violations, c.keep, violations, supports);
    return cloud_compact(ctx, p, c, xyz, rgb, err, n_refs, xyz_out, rgb_out, err_out, ref_offsets_out_host, n_out_host);
}

// ---- depth and normal maps of the final cloud (lfd_depth.hip) -------------------------------------------------------------------------------------
int lfd_render_depth(lfd_context* ctx, const float* xyz, int64_t n, const float* normals, const float* cam_P_host, const int32_t* cam_wh_host,
                     int32_t n_cams, int32_t pw, int32_t ph, int32_t splat_cells, int32_t window_cells, float tol, int32_t cams_per_batch,
                     float* depth_out, int32_t* index_out, float* normal_out) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (const char* why = lfd_depth_check(xyz, n, normals, cam_P_host, cam_wh_host, n_cams, pw, ph, splat_cells, window_cells, tol, cams_per_batch,
                                          depth_out, index_out, normal_out))
        return fail(ctx, LFD_ERR_INVALID, std::string("lfd_render_depth: ") + why);
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const long long cells = (long long)pw * ph;                        // n_cams * cells <= 2^31 - 1 (lfd_depth_check)
    const int32_t per = lfd_depth_batch(n_cams, pw, ph, cams_per_batch);
    std::vector<LfdFreespaceCam> cams((size_t)n_cams);
    for (int32_t c = 0; c < n_cams; ++c) lfd_freespace_cam(cam_P_host + 12 * (size_t)c, cam_wh_host[2 * c], cam_wh_host[2 * c + 1], cams[(size_t)c]);
    unsigned long long* keys = nullptr;                                // the u64 planes of one batch, filled before they are read
    LfdFreespaceCam* d_cams = nullptr;
    if (int rc = carve_cloud_ws(ctx, [&](Bump& b) {
            keys = b.take<unsigned long long>((size_t)per * (size_t)cells);
            d_cams = b.take<LfdFreespaceCam>((size_t)n_cams);
        }))
        return rc;
    LFD_HIP(ctx, hipMemcpyAsync(d_cams, cams.data(), (size_t)n_cams * sizeof(LfdFreespaceCam), hipMemcpyHostToDevice, st));
    LFD_HIP(ctx, hipStreamSynchronize(st));                            // `cams` is pageable memory of this call: the copy has read it
    const int tiles_x = (pw + 31) / 32, tiles_y = (ph + 15) / 16;      // lfd_depth.hip: LFD_DEPTH_TW x LFD_DEPTH_TH
    const unsigned n_wg = (unsigned)((n + 255) / 256);
    for (int32_t c0 = 0; c0 < n_cams; c0 += per) {
        const int nb = (int)std::min<int32_t>(per, n_cams - c0);
        const long long n_words = (long long)nb * cells, o = (long long)c0 * cells;
        hipLaunchKernelGGL(lfd_depth_fill_kernel, dim3((unsigned)std::min<long long>((n_words + 255) / 256, 4096)), dim3(256), 0, st, keys, n_words);
        if (n > 0) hipLaunchKernelGGL(lfd_depth_splat_kernel, dim3(n_wg), dim3(256), 0, st, xyz, (long long)n, d_cams + c0, nb, (int)pw, (int)ph, keys);
        // tiles_x tiles_y nb <= nb cells <= 2^31 - 1 workgroups
        hipLaunchKernelGGL(lfd_depth_resolve_kernel, dim3((unsigned)((long long)tiles_x * tiles_y * nb)), dim3(256), 0, st, keys, (int)pw, (int)ph, tiles_x,
                           tiles_y, (int)splat_cells, (int)window_cells, tol, normals, depth_out + o, index_out ? index_out + o : nullptr,
                           normal_out ? normal_out + 3 * o : nullptr);
    }
    LFD_HIP(ctx, hipGetLastError());
    LFD_HIP(ctx, hipStreamSynchronize(st));                            // the workspace is free for the next stage on return
    return LFD_OK;
}

// ---- oriented voxel fusion on the final cloud (lfd_fuse.hip; the grid and the sort are lfd_voxel.hip's kernels) ------------------------------------
int lfd_fuse_oriented(lfd_context* ctx, const float* xyz, const float* normals, const float* rgb, int64_t n, double voxel_size, float* xyz_out,
                      float* normals_out, float* rgb_out, uint32_t* count_out, int64_t* n_rows_host, int64_t* n_voxels_host) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (const char* why = lfd_fuse_check(xyz, normals, rgb, n, voxel_size, xyz_out, normals_out, rgb_out, count_out, n_rows_host, n_voxels_host))
        return fail(ctx, LFD_ERR_INVALID, std::string("lfd_fuse_oriented: ") + why);
    *n_rows_host = 0;
    *n_voxels_host = 0;
    if (n == 0) return LFD_OK;
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const CloudPlan p = cloud_plan(n);
    CloudSort w;                                                       // counters: voxel count, big-voxel count, row count
    unsigned *rows = nullptr, *big = nullptr;                          // rows of every voxel, big-voxel list
    uint8_t* flag = nullptr;                                           // flag byte of every sorted point
    if (int rc = carve_cloud_ws(ctx, [&](Bump& b) {
            w = carve_sort(b, p.n, 3, true);
            rows = b.take<unsigned>((size_t)n);
            big = b.take<unsigned>((size_t)n / (LFD_VOX_BIG + 1) + 1);
            flag = b.take<uint8_t>((size_t)n);
        }))
        return rc;
    unsigned *nv_dev = w.counters, *n_big = w.counters + 1, *n_rows_dev = w.counters + 2;

    // the refusals are decided before anything is sorted
    LfdVoxStats s;
    if (int rc = cloud_stats(ctx, p, w, xyz, rgb, s)) return rc;
    if (s.flags & LFD_VOX_NONFINITE) return fail(ctx, LFD_ERR_INVALID, "lfd_fuse_oriented: " LFD_FUSE_NONFINITE);
    LfdFuseGrid g;
    if (!lfd_fuse_grid(s.lo, s.hi, voxel_size, g)) return fail(ctx, LFD_ERR_INVALID, "lfd_fuse_oriented: " LFD_FUSE_KEY_RANGE);
    const double cscale = lfd_fuse_cscale(s.cmax, (s.flags & LFD_VOX_NAN_RGB) != 0u);

    hipLaunchKernelGGL(lfd_voxel_keys_kernel, dim3(p.grid), dim3(256), 0, st, xyz, p.n, g.origin[0], g.origin[1], g.origin[2], voxel_size, g.e[1],
                       g.e[2], w.keys[0], w.idx[0]);
    const int cur = cloud_sort(st, p, w, g.bits);
    cloud_heads_count(st, p, w, cur);
    cloud_heads_scatter(st, p, w, cur);
    // sides and rows, then the first row of every voxel (the voxels, at most n, are cut into the sort's chunks for the row scan), then the sums
    LFD_HIP(ctx, hipMemsetAsync(n_big, 0, sizeof(unsigned), st));
    const unsigned big_grid = (unsigned)std::min<long long>(n / (LFD_VOX_BIG + 1) + 1, 8192);
    hipLaunchKernelGGL(lfd_fuse_side_kernel, dim3(p.grid), dim3(256), 0, st, normals, p.n, w.idx[cur], w.vstart, nv_dev, flag, rows, big, n_big);
    hipLaunchKernelGGL(lfd_fuse_side_big_kernel, dim3(big_grid), dim3(64), 0, st, normals, p.n, w.idx[cur], w.vstart, nv_dev, big, n_big, flag, rows);
    hipLaunchKernelGGL(lfd_fuse_rowsum_kernel, dim3((unsigned)p.G), dim3(256), 0, st, rows, nv_dev, p.chunk, w.counts);
    hipLaunchKernelGGL(lfd_voxel_scan_kernel, dim3(1), dim3(1024), 0, st, w.counts, (int)p.G, n_rows_dev);
    hipLaunchKernelGGL(lfd_fuse_rowstart_kernel, dim3((unsigned)p.G), dim3(256), 0, st, rows, nv_dev, p.chunk, w.counts);
    hipLaunchKernelGGL(lfd_fuse_sums_kernel, dim3(p.grid), dim3(256), 0, st, xyz, normals, rgb, p.n, w.idx[cur], w.vstart, nv_dev, flag, rows, cscale,
                       xyz_out, normals_out, rgb_out, count_out);
    hipLaunchKernelGGL(lfd_fuse_sums_big_kernel, dim3(big_grid), dim3(64), 0, st, xyz, normals, rgb, p.n, w.idx[cur], w.vstart, nv_dev, flag, rows,
                       cscale, big, n_big, xyz_out, normals_out, rgb_out, count_out);
    LFD_HIP(ctx, hipGetLastError());
    LFD_HIP(ctx, hipMemcpyAsync(ctx->pinned_words, nv_dev, 3 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    LFD_HIP(ctx, hipStreamSynchronize(st));
    *n_voxels_host = (int64_t)(unsigned)ctx->pinned_words[0];
    *n_rows_host = (int64_t)(unsigned)ctx->pinned_words[2];
    return LFD_OK;
}

// ---- Gaussian-ready output: exact 3-NN mean squared distance and the 68-byte record (lfd_knn.hip) ---------------------------------------------------
int lfd_knn_dist2(lfd_context* ctx, const float* xyz, int64_t n, double cell_size, float* dist2_out, double* stats_host) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (const char* why = lfd_knn_check(xyz, n, cell_size, dist2_out)) return fail(ctx, LFD_ERR_INVALID, std::string("lfd_knn_dist2: ") + why);
    if (stats_host) stats_host[0] = stats_host[1] = stats_host[2] = stats_host[3] = 0.0;
    if (n == 0) return LFD_OK;
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const CloudPlan p = cloud_plan(n);
    CloudSort w;                                                       // counters: cell count, fullest cell, listed points
    LfdKnnPt* spt = nullptr;                                           // sorted points
    unsigned* list = nullptr;                                          // the points the grid scan did not settle
    if (int rc = carve_cloud_ws(ctx, [&](Bump& b) {
            w = carve_sort(b, p.n, 3, true);
            spt = b.take<LfdKnnPt>((size_t)n);
            list = b.take<unsigned>((size_t)n);
        }))
        return rc;
    unsigned *nv_dev = w.counters, *cell_max = w.counters + 1, *n_list = w.counters + 2;

    // the refusals are decided before anything is sorted
    LfdVoxStats s;
    if (int rc = cloud_stats(ctx, p, w, xyz, nullptr, s)) return rc;
    if (s.flags & LFD_VOX_NONFINITE) return fail(ctx, LFD_ERR_INVALID, "lfd_knn_dist2: " LFD_KNN_NONFINITE);
    double h = cell_size > 0.0 ? cell_size : lfd_knn_auto_h(s.lo, s.hi, (long long)n);
    LfdKnnGrid g;
    if (!lfd_knn_grid(s.lo, s.hi, h, g)) return fail(ctx, LFD_ERR_INVALID, "lfd_knn_dist2: " LFD_KNN_KEY_RANGE);

    int cur = 0;
    for (int rebuilds = 0;;) {
        hipLaunchKernelGGL(lfd_knn_keys_kernel, dim3(p.grid), dim3(256), 0, st, xyz, p.n, g, w.keys[0], w.idx[0]);
        cur = cloud_sort(st, p, w, g.bits);
        cloud_heads_count(st, p, w, cur);
        LFD_HIP(ctx, hipGetLastError());
        if (cell_size > 0.0) break;
        // the automatic rule looks at the occupied cells of this grid (lfd_knn.hpp): the same decisions as the twin's
        LFD_HIP(ctx, hipMemcpyAsync(ctx->pinned_words, nv_dev, sizeof(unsigned), hipMemcpyDeviceToHost, st));
        LFD_HIP(ctx, hipStreamSynchronize(st));
        const long long occupied = (long long)(unsigned)ctx->pinned_words[0];
        LfdKnnGrid finer;
        if (!lfd_knn_refine_more((long long)n, occupied, rebuilds) || !lfd_knn_grid(s.lo, s.hi, h / 4.0, finer)) break;
        h = h / 4.0;
        g = finer;
        ++rebuilds;
    }
    cloud_heads_scatter(st, p, w, cur);
    LFD_HIP(ctx, hipMemsetAsync(cell_max, 0, 2 * sizeof(unsigned), st));           // cell_max and n_list
    hipLaunchKernelGGL(lfd_knn_cellmax_kernel, dim3(p.grid), dim3(256), 0, st, w.vstart, nv_dev, p.n, cell_max);
    hipLaunchKernelGGL(lfd_knn_gather_kernel, dim3(p.grid), dim3(256), 0, st, xyz, w.idx[cur], p.n, spt);
    hipLaunchKernelGGL(lfd_knn_scan_kernel, dim3((unsigned)p.n_wg), dim3(256), 0, st, w.keys[cur], spt, p.n, g, dist2_out, list, n_list);
    hipLaunchKernelGGL(lfd_knn_brute_kernel, dim3((unsigned)std::min<long long>(n, 1024)), dim3(256), 0, st, spt, p.n, list, n_list, dist2_out);
    LFD_HIP(ctx, hipGetLastError());
    LFD_HIP(ctx, hipMemcpyAsync(ctx->pinned_words, nv_dev, 3 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    LFD_HIP(ctx, hipStreamSynchronize(st));
    if (stats_host) {
        stats_host[0] = h;
        for (int k = 0; k < 3; ++k) stats_host[1 + k] = (double)(unsigned)ctx->pinned_words[k];
    }
    return LFD_OK;
}

int lfd_pack_gaussians(lfd_context* ctx, const float* xyz, const float* normals, const float* rgb, const float* dist2, int64_t n, float opacity_logit,
                       double log_flatten, double max_scale, uint8_t* out) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (const char* why = lfd_gauss_check(xyz, normals, rgb, dist2, n, opacity_logit, log_flatten, max_scale, out))
        return fail(ctx, LFD_ERR_INVALID, std::string("lfd_pack_gaussians: ") + why);
    if (n == 0) return LFD_OK;
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(lfd_pack_gaussians_kernel, dim3(grid), dim3(256), 0, ctx->stream, xyz, normals, rgb, dist2, (long long)n, opacity_logit,
                       log_flatten, lfd_gauss_max_m(max_scale), reinterpret_cast<float*>(out));
    LFD_HIP(ctx, hipGetLastError());
    return LFD_OK;
}

// ---- spatial point cap on the final cloud (lfd_cap.hip; the sort, the heads and the compaction prefix are the shared ones) ---------------------------
int lfd_cap_spatial(lfd_context* ctx, const float* xyz, const float* err, int64_t n, int64_t budget, int64_t* keep_out, int64_t* n_keep_host,
                    double* stats_host) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (const char* why = lfd_cap_check(xyz, err, n, budget, keep_out, n_keep_host)) return fail(ctx, LFD_ERR_INVALID, std::string("lfd_cap_spatial: ") + why);
    *n_keep_host = 0;
    if (stats_host) stats_host[0] = stats_host[1] = stats_host[2] = stats_host[3] = 0.0;
    if (n == 0) return LFD_OK;
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const CloudPlan p = cloud_plan(n);
    CloudSort w;                                                       // counters: cell count, then the 22 level bins
    unsigned long long* rep = nullptr;                                 // (rank, index) minimum of every cell
    CloudCompact c;
    if (int rc = carve_cloud_ws(ctx, [&](Bump& b) {
            w = carve_sort(b, p.n, 1 + LFD_CAP_LEVELS + 1, true);
            rep = b.take<unsigned long long>((size_t)n);
            c = carve_compact(b, p, 0);
        }))
        return rc;
    unsigned *nc_dev = w.counters, *hist_dev = w.counters + 1;

    // the refusal is decided before anything is sorted
    LfdVoxStats s;
    if (int rc = cloud_stats(ctx, p, w, xyz, nullptr, s)) return rc;
    if (s.flags & LFD_VOX_NONFINITE) return fail(ctx, LFD_ERR_INVALID, "lfd_cap_spatial: " LFD_CAP_NONFINITE);
    const LfdCapBox box = lfd_cap_box(s.lo, s.hi);

    LFD_HIP(ctx, hipMemsetAsync(hist_dev, 0, (LFD_CAP_LEVELS + 1) * sizeof(unsigned), st));
    hipLaunchKernelGGL(lfd_cap_keys_kernel, dim3(p.grid), dim3(256), 0, st, xyz, p.n, box, w.keys[0], w.idx[0]);
    const int cur = cloud_sort(st, p, w, 3 * LFD_CAP_LEVELS);
    hipLaunchKernelGGL(lfd_cap_levels_kernel, dim3(p.grid), dim3(256), 0, st, w.keys[cur], p.n, hist_dev);
    LFD_HIP(ctx, hipGetLastError());
    LFD_HIP(ctx, hipMemcpyAsync(ctx->pinned_words, hist_dev, (LFD_CAP_LEVELS + 1) * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    LFD_HIP(ctx, hipStreamSynchronize(st));
    unsigned long long hist[LFD_CAP_LEVELS + 1];
    for (int l = 0; l <= LFD_CAP_LEVELS; ++l) hist[l] = (unsigned long long)(unsigned)ctx->pinned_words[l];
    long long cells = 0;
    const int lev = lfd_cap_level(hist, (long long)budget, box.L, &cells, stats_host);

    if (n <= budget) {                                                 // the cap does not act: every point is kept
        LFD_HIP(ctx, hipMemsetAsync(c.keep, 1, (size_t)n, st));
    } else {
        if (lev < LFD_CAP_LEVELS)
            hipLaunchKernelGGL(lfd_cap_coarsen_kernel, dim3(p.grid), dim3(256), 0, st, w.keys[cur], p.n, 3 * (LFD_CAP_LEVELS - lev));
        cloud_heads_count(st, p, w, cur);
        cloud_heads_scatter(st, p, w, cur);
        LFD_HIP(ctx, hipMemsetAsync(rep, 0xff, (size_t)n * sizeof(unsigned long long), st));
        LFD_HIP(ctx, hipMemsetAsync(c.keep, 0, (size_t)n, st));
        hipLaunchKernelGGL(lfd_cap_rep_kernel, dim3((unsigned)p.n_wg), dim3(256), 0, st, w.idx[cur], w.vstart, nc_dev, err, p.n,
                           (unsigned long long)budget, rep);
        hipLaunchKernelGGL(lfd_cap_mark_kernel, dim3(p.grid), dim3(256), 0, st, rep, nc_dev, p.n, (unsigned long long)budget, c.keep);
    }
    cloud_compact_prefix(st, p, c);
    hipLaunchKernelGGL(lfd_cap_index_kernel, dim3((unsigned)p.n_wg), dim3(256), 0, st, c.keep, c.wg_kept, p.n, (long long)std::min<int64_t>(budget, n),
                       reinterpret_cast<long long*>(keep_out));
    LFD_HIP(ctx, hipGetLastError());
    LFD_HIP(ctx, hipMemcpyAsync(ctx->pinned_words, c.wg_kept + p.n_wg, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    LFD_HIP(ctx, hipStreamSynchronize(st));
    *n_keep_host = (int64_t)(unsigned)ctx->pinned_words[0];
    return LFD_OK;
}

// ---- footprint-adaptive thinning of the final cloud (lfd_thin.hip; the representatives are the cap's kernels, the rest is the shared driver) ------------
int lfd_thin_footprint(lfd_context* ctx, const float* xyz, const float* err, int64_t n, const int64_t* ref_offsets_host, int32_t n_refs,
                       const double* ref_rows_host, double thin_cells, int64_t* keep_out, int64_t* n_keep_host, int64_t* ref_offsets_out_host,
                       double* stats_host) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (const char* why = lfd_thin_check(xyz, err, n, ref_offsets_host, n_refs, ref_rows_host, thin_cells, keep_out, n_keep_host, ref_offsets_out_host))
        return fail(ctx, LFD_ERR_INVALID, std::string("lfd_thin_footprint: ") + why);
    for (int32_t r = 0; r <= n_refs; ++r) ref_offsets_out_host[r] = 0;
    *n_keep_host = 0;
    if (stats_host)
        for (int k = 0; k < LFD_THIN_STATS; ++k) stats_host[k] = 0.0;
    if (n == 0) return LFD_OK;
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const CloudPlan p = cloud_plan(n);
    CloudSort w;                                                       // counters: cell count, then points per level and cells per level
    unsigned long long* rep = nullptr;                                 // (rank, index) minimum of every cell
    double* rows = nullptr;                                            // the references' five values
    CloudCompact c;
    if (int rc = carve_cloud_ws(ctx, [&](Bump& b) {
            w = carve_sort(b, p.n, 1 + 2 * LFD_THIN_LEVELS, true);
            rep = b.take<unsigned long long>((size_t)n);
            rows = b.take<double>(LFD_THIN_ROW * (size_t)n_refs);
            c = carve_compact(b, p, n_refs);
        }))
        return rc;
    unsigned *nc_dev = w.counters, *hist_dev = w.counters + 1;

    // the refusal is decided before anything is sorted (the read-back of the statistics also ends the two uploads)
    LFD_HIP(ctx, hipMemcpyAsync(c.offs, ref_offsets_host, ((size_t)n_refs + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    LFD_HIP(ctx, hipMemcpyAsync(rows, ref_rows_host, LFD_THIN_ROW * (size_t)n_refs * sizeof(double), hipMemcpyHostToDevice, st));
    LfdVoxStats s;
    if (int rc = cloud_stats(ctx, p, w, xyz, nullptr, s)) return rc;
    if (s.flags & LFD_VOX_NONFINITE) return fail(ctx, LFD_ERR_INVALID, "lfd_thin_footprint: " LFD_THIN_NONFINITE);
    const LfdCapBox box = lfd_cap_box(s.lo, s.hi);

    LFD_HIP(ctx, hipMemsetAsync(hist_dev, 0, 2 * LFD_THIN_LEVELS * sizeof(unsigned), st));
    hipLaunchKernelGGL(lfd_thin_keys_kernel, dim3(p.grid), dim3(256), 0, st, xyz, p.n, c.offs, (int)n_refs, rows, thin_cells, box, w.keys[0],
                       w.idx[0], hist_dev);
    const int cur = cloud_sort(st, p, w, LFD_THIN_CODE_BITS);
    cloud_heads_count(st, p, w, cur);
    cloud_heads_scatter(st, p, w, cur);
    hipLaunchKernelGGL(lfd_thin_cells_kernel, dim3(p.grid), dim3(256), 0, st, w.keys[cur], w.vstart, nc_dev, p.n, hist_dev + LFD_THIN_LEVELS);
    LFD_HIP(ctx, hipMemsetAsync(rep, 0xff, (size_t)n * sizeof(unsigned long long), st));
    LFD_HIP(ctx, hipMemsetAsync(c.keep, 0, (size_t)n, st));
    const unsigned long long all = (unsigned long long)n;              // a budget of n >= the cell count: lfd_cap_pick takes every cell
    hipLaunchKernelGGL(lfd_cap_rep_kernel, dim3((unsigned)p.n_wg), dim3(256), 0, st, w.idx[cur], w.vstart, nc_dev, err, p.n, all, rep);
    hipLaunchKernelGGL(lfd_cap_mark_kernel, dim3(p.grid), dim3(256), 0, st, rep, nc_dev, p.n, all, c.keep);
    cloud_compact_prefix(st, p, c);
    hipLaunchKernelGGL(lfd_consensus_offsets_kernel, dim3((unsigned)std::min<long long>(((long long)n_refs + 256) / 256, 1024)), dim3(256), 0, st, c.offs,
                       (int)n_refs, c.keep, c.wg_kept, c.offs_out);
    hipLaunchKernelGGL(lfd_cap_index_kernel, dim3((unsigned)p.n_wg), dim3(256), 0, st, c.keep, c.wg_kept, p.n, p.n, reinterpret_cast<long long*>(keep_out));
    LFD_HIP(ctx, hipGetLastError());
    unsigned hist[2 * LFD_THIN_LEVELS];
    LFD_HIP(ctx, hipMemcpyAsync(hist, hist_dev, sizeof(hist), hipMemcpyDeviceToHost, st));
    LFD_HIP(ctx, hipMemcpyAsync(ref_offsets_out_host, c.offs_out, ((size_t)n_refs + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
    LFD_HIP(ctx, hipStreamSynchronize(st));
    *n_keep_host = ref_offsets_out_host[n_refs];
    if (stats_host) {
        for (int k = 0; k < 2 * LFD_THIN_LEVELS; ++k) stats_host[k] = (double)hist[k];
        stats_host[2 * LFD_THIN_LEVELS] = box.L;
    }
    return LFD_OK;
}

// ---- image undistortion in front of everything else (lfd_undistort.hip)-------------------------------------------------------------------------
int lfd_undistort_image(lfd_context* ctx, const uint8_t* src, int32_t w, int32_t h, int32_t channels, int32_t nearest, const double intr[4],
                        const double dist[8], uint8_t* dst, uint8_t* valid255, int64_t* n_invalid_host) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (const char* why = lfd_undistort_check(src, w, h, channels, intr, dist, dst, valid255))
        return fail(ctx, LFD_ERR_INVALID, std::string("lfd_undistort_image: ") + why);
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    const LfdUndistortArgs p = lfd_undistort_args(src, w, h, channels, nearest, intr, dist, dst, valid255);
    unsigned long long* counter = nullptr;
    if (n_invalid_host) {
        if (int rc = ensure(ctx, ctx->undist_cnt, sizeof(unsigned long long))) return rc;
        counter = static_cast<unsigned long long*>(ctx->undist_cnt.ptr);
        LFD_HIP(ctx, hipMemsetAsync(counter, 0, sizeof(unsigned long long), ctx->stream));
    }
    LFD_HIP(ctx, lfd_undistort_launch(p, counter, ctx->stream));
    if (n_invalid_host) {
        LFD_HIP(ctx, hipMemcpyAsync(ctx->pinned_words, counter, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        LFD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        unsigned long long v;
        std::memcpy(&v, ctx->pinned_words, sizeof(v));
        *n_invalid_host = (int64_t)v;
    }
    return LFD_OK;
}

// ---- local correlation of RoMa-v2's refiners (lfd_corr.hip) ----------------------------------------------------------------------------
int lfd_local_corr(lfd_context* ctx, const float* A, const float* Bf, const float* warp, int32_t B, int32_t N, int32_t C, int32_t K, int32_t H1,
                   int32_t W1, const int64_t* a_strides, const int64_t* bf_strides, float* out) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    LfdCorrArgs p;
    if (const char* why = lfd_corr_fill(A, Bf, warp, B, N, C, K, H1, W1, a_strides, bf_strides, out, p))
        return fail(ctx, LFD_ERR_INVALID, std::string("lfd_local_corr: ") + why);
    if ((long long)B * N * K == 0) return LFD_OK;
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    LFD_HIP(ctx, lfd_corr_launch(p, ctx->stream));
    return LFD_OK;
}

// ---- one conv block of RoMa-v2's refiners (lfd_block.hip) --------------------------------------------------------------------------------
int lfd_refiner_block(lfd_context* ctx, const void* x, int32_t x_is_f32, int32_t B, int32_t C, int32_t H, int32_t W, const float* dw_w,
                      const float* scale, const float* shift, const float* pw_wT, const float* pw_b, uint16_t* out) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    LfdBlockArgs p;
    if (const char* why = lfd_block_fill(x, x_is_f32, B, C, H, W, dw_w, scale, shift, pw_wT, pw_b, out, p))
        return fail(ctx, LFD_ERR_INVALID, std::string("lfd_refiner_block: ") + why);
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    LFD_HIP(ctx, lfd_block_launch(p, ctx->stream));
    return LFD_OK;
}

// ---- the output head of RoMa-v2's refiners (lfd_head.hip) ---------------------------------------------------------------------------------
int lfd_refiner_head(lfd_context* ctx, const void* z, int32_t z_is_f32, int32_t B, int32_t C, int32_t H, int32_t W, const float* head_w,
                     const float* head_b, const float* prev_warp, const int64_t* prev_warp_strides, const float* prev_conf,
                     const int64_t* prev_conf_strides, int32_t prev_dim, float refine_init, float* warp, float* conf) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    LfdHeadArgs p;
    if (const char* why = lfd_head_fill(z, z_is_f32, B, C, H, W, head_w, head_b, prev_warp, prev_warp_strides, prev_conf, prev_conf_strides, prev_dim,
                                        refine_init, warp, conf, p))
        return fail(ctx, LFD_ERR_INVALID, std::string("lfd_refiner_head: ") + why);
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    LFD_HIP(ctx, lfd_head_launch(p, ctx->stream));
    return LFD_OK;
}

// ---- forward-backward consistency gate (lfd_cycle.hip) -----------------------------------------------------------------------------------
int lfd_cycle_gate(lfd_context* ctx, int32_t n_pairs, const float* const* cert, const float* const* warp_ab, const float* const* warp_ba, int32_t H,
                   int32_t W, int32_t warp_channels, int32_t Hb, int32_t Wb, const float* axis_x, const float* axis_y, int32_t w_match,
                   int32_t h_match, float certainty_thresh, float cycle_thresh_px, float* const* cert_out, float* const* err_out,
                   int32_t* rejected) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    LfdCycleArgs p;
    if (const char* why = lfd_cycle_fill(n_pairs, cert, warp_ab, warp_ba, H, W, warp_channels, Hb, Wb, axis_x, axis_y, w_match, h_match,
                                         certainty_thresh, cycle_thresh_px, cert_out, err_out, rejected, p))
        return fail(ctx, LFD_ERR_INVALID, std::string("lfd_cycle_gate: ") + why);
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    LFD_HIP(ctx, lfd_cycle_launch(p, ctx->stream));
    return LFD_OK;
}

// ---- the per-point stages behind triangulation: what their entry points share ---------------------------------------------------------------
static int device_guard(lfd_context* ctx) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    return LFD_OK;
}

static LfdSupportGeom launch_geom(const lfd_batch* batch, const LfdLaunch& L, float support_thresh_px, float reproj_thresh) {
    return lfd_support_geom(batch, L.kp.wm1, L.kp.hm1, L.mask_sx, L.mask_sy, support_thresh_px, reproj_thresh);
}

// The header of a stage's arguments: the batch's tables (batch_launch), the input points and the launch geometry.
static int fill_stage(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets, float support_thresh_px,
                      float reproj_thresh, LfdPointStage& st) {
    LfdLaunch L;
    int rc = batch_launch(ctx, batch, L);
    if (rc != LFD_OK) return rc;
    st.refs = L.refs; st.slots = L.slots; st.ref_const = L.ref_const; st.pair_const = L.pair_const;
    st.axis_x = L.axis_x; st.axis_y = L.axis_y;
    st.offs = reinterpret_cast<const long long*>(ref_offsets);
    st.xyz = in->xyz; st.rgb = in->rgb; st.err = in->err; st.cell = in->cell; st.slot = in->slot;
    st.capacity = in->capacity;
    st.n_refs = batch->n_refs; st.k = batch->k; st.n_wg = (int32_t)((in->capacity + 255) / 256);
    st.g = launch_geom(batch, L, support_thresh_px, reproj_thresh);
    return LFD_OK;
}

// The workspace of the three gates (support filter, depth-uncertainty gate, photo-consistency gate), one layout: a keep byte per point of the
// covering workgroups, the workgroups' counts and one word for the total, then - when a plane moves with the points - an f32 per point.  Also
// zeroes the caller's seg_counts, which the gates' kernels add to.
struct GateWs { uint8_t* keep; unsigned* wg_kept; float* extra; };

static int carve_gate_ws(lfd_context* ctx, const LfdPointStage& st, bool extra, int32_t* seg_counts_out, GateWs& w) {
    const size_t n_pad = (size_t)st.n_wg * 256, words = ((size_t)st.n_wg + 1) * sizeof(unsigned);
    int rc = ensure(ctx, ctx->support_ws, n_pad + words + (extra ? n_pad * sizeof(float) : 0));
    if (rc != LFD_OK) return rc;
    unsigned char* ws = static_cast<unsigned char*>(ctx->support_ws.ptr);
    w.keep = ws;
    w.wg_kept = reinterpret_cast<unsigned*>(ws + n_pad);
    w.extra = extra ? reinterpret_cast<float*>(ws + n_pad + words) : nullptr;
    if (seg_counts_out) LFD_HIP(ctx, hipMemsetAsync(seg_counts_out, 0, sizeof(int32_t) * (size_t)st.n_refs * st.k, ctx->stream));
    return LFD_OK;
}

static LfdCompactArgs compact_args(const LfdPointStage& st, const GateWs& w, const lfd_points* out, int64_t* ref_offsets_out, float* extra_out) {
    LfdCompactArgs c = {};
    c.offs_in = st.offs; c.offs_out = reinterpret_cast<long long*>(ref_offsets_out);
    c.xyz = st.xyz; c.rgb = st.rgb; c.err = st.err; c.cell = st.cell; c.slot = st.slot;
    c.o_xyz = out->xyz; c.o_rgb = out->rgb; c.o_err = out->err; c.o_cell = out->cell; c.o_slot = out->slot;
    c.keep = w.keep; c.wg_kept = w.wg_kept; c.extra_in = w.extra; c.extra_out = extra_out;
    c.capacity = st.capacity; c.n_refs = st.n_refs; c.n_wg = st.n_wg;
    return c;
}

// ---- multi-view support filter (lfd_support.hip) -------------------------------------------------------------------------------------------
int lfd_support_filter(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets_in, int32_t min_support,
                       float support_thresh_px, const lfd_points* out, int64_t* ref_offsets_out, int32_t* seg_counts_out, uint8_t* support) {
    if (int rc = device_guard(ctx)) return rc;
    int code = LFD_ERR_INVALID;
    if (const char* why = lfd_support_check(in, ref_offsets_in, min_support, support_thresh_px, out, ref_offsets_out, &code))
        return fail(ctx, code, std::string("lfd_support_filter: ") + why);
    LfdSupportArgs p = {};
    int rc = fill_stage(ctx, batch, in, ref_offsets_in, support_thresh_px, 0.0f, p.st);
    if (rc != LFD_OK) return rc;
    GateWs w;
    rc = carve_gate_ws(ctx, p.st, false, seg_counts_out, w);
    if (rc != LFD_OK) return rc;
    p.seg_counts = seg_counts_out; p.support = support; p.keep = w.keep; p.wg_kept = w.wg_kept; p.min_support = min_support;
    LFD_HIP(ctx, lfd_support_launch(p, compact_args(p.st, w, out, ref_offsets_out, nullptr), ctx->stream));
    return LFD_OK;
}

// ---- multi-view re-triangulation of supported points (lfd_refine.hip) ------------------------------------------------------------------------
// A table of per-(reference, slot) device pointers of a batch (precision planes, neighbour images), where the kernel reads it: like the batch's
// descriptor tables it is compared with what the device already holds and uploaded only when it differs, on the launch stream (an earlier
// launch still reading the old table precedes the copy in it), from a pinned staging buffer that is waited for only while its last upload is
// still on its way.  Entries of slots the batch does not use are null.
static int upload_blob_table(lfd_context* ctx, lfd_context::PointerTable& t, std::vector<unsigned char>& blob, const void** d_tab) {
    const size_t bytes = blob.size();
    if (!t.tab.ptr || t.cache != blob) {
        int rc = ensure(ctx, t.tab, bytes);
        if (rc != LFD_OK) return rc;
        if (!t.free_ev) LFD_HIP(ctx, hipEventCreateWithFlags(&t.free_ev, hipEventDisableTiming));
        if (t.in_flight) { LFD_HIP(ctx, hipEventSynchronize(t.free_ev)); t.in_flight = false; }
        if (t.pinned_bytes < bytes) {
            if (t.pinned) LFD_HIP(ctx, hipHostFree(t.pinned));
            t.pinned = nullptr;
            t.pinned_bytes = std::max<size_t>(bytes * 2, 4096);
            LFD_HIP(ctx, hipHostMalloc(&t.pinned, t.pinned_bytes, hipHostMallocDefault));
        }
        std::memcpy(t.pinned, blob.data(), bytes);
        LFD_HIP(ctx, hipMemcpyAsync(t.tab.ptr, t.pinned, bytes, hipMemcpyHostToDevice, ctx->stream));
        LFD_HIP(ctx, hipEventRecord(t.free_ev, ctx->stream));
        t.in_flight = true;
        t.cache.swap(blob);
    }
    *d_tab = t.tab.ptr;
    return LFD_OK;
}

static int upload_pointer_table(lfd_context* ctx, lfd_context::PointerTable& t, const lfd_batch* b, const void* const* ptrs, const void* const** d_tab) {
    const size_t n = (size_t)b->n_refs * b->k, bytes = n * sizeof(const void*);
    std::vector<unsigned char> blob(bytes, 0);
    const void** tab = reinterpret_cast<const void**>(blob.data());
    for (int r = 0; r < b->n_refs; ++r)
        for (int j = 0; j < b->n_slots[r]; ++j) tab[(size_t)r * b->k + j] = ptrs[(size_t)r * b->k + j];
    const void* d = nullptr;
    int rc = upload_blob_table(ctx, t, blob, &d);
    if (rc != LFD_OK) return rc;
    *d_tab = static_cast<const void* const*>(d);
    return LFD_OK;
}

static int upload_precision_table(lfd_context* ctx, const lfd_batch* b, const float* const* precision, const float* const** d_tab) {
    return upload_pointer_table(ctx, ctx->prec, b, reinterpret_cast<const void* const*>(precision), reinterpret_cast<const void* const**>(d_tab));
}

// (one table for the colour, gain and photo stages: the cache compares content, and the stages of one configuration hand over the same images)
static int upload_image_table(lfd_context* ctx, const lfd_batch* b, const uint8_t* const* nbr_image, const uint8_t* const** d_tab) {
    return upload_pointer_table(ctx, ctx->colour_img, b, reinterpret_cast<const void* const*>(nbr_image), reinterpret_cast<const void* const**>(d_tab));
}

// Both re-triangulation calls.  weighted: lfd_refine_multiview_weighted (precision checked behind the batch, its table uploaded, three
// counters); otherwise lfd_refine_multiview (two).  name: the entry point, for the messages.
static int refine_impl(lfd_context* ctx, const char* name, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets,
                       float support_thresh_px, float reproj_thresh, float* xyz_out, float* err_out, uint8_t* status, int64_t* counters,
                       const float* const* precision, bool weighted) {
    if (int rc = device_guard(ctx)) return rc;
    if (const char* why = lfd_refine_check(in, ref_offsets, support_thresh_px, reproj_thresh, xyz_out, err_out, status))
        return fail(ctx, LFD_ERR_INVALID, std::string(name) + ": " + why);
    LfdRefineArgs p = {};
    int rc = fill_stage(ctx, batch, in, ref_offsets, support_thresh_px, reproj_thresh, p.st);
    if (rc != LFD_OK) return rc;
    if (weighted) {
        if (const char* why = lfd_refine_check_precision(batch, precision)) return fail(ctx, LFD_ERR_INVALID, std::string(name) + ": " + why);
        rc = upload_precision_table(ctx, batch, precision, &p.prec);
        if (rc != LFD_OK) return rc;
    }
    p.o_xyz = xyz_out; p.o_err = err_out; p.status = status;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    LFD_HIP(ctx, lfd_refine_launch(p, ctx->stream));
    return LFD_OK;
}

int lfd_refine_multiview(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets, float support_thresh_px,
                         float reproj_thresh, float* xyz_out, float* err_out, uint8_t* status, int64_t* counters) {
    return refine_impl(ctx, "lfd_refine_multiview", batch, in, ref_offsets, support_thresh_px, reproj_thresh, xyz_out, err_out, status, counters,
                       nullptr, false);
}

int lfd_refine_multiview_weighted(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets,
                                  float support_thresh_px, float reproj_thresh, float* xyz_out, float* err_out, uint8_t* status, int64_t* counters,
                                  const float* const* precision) {
    return refine_impl(ctx, "lfd_refine_multiview_weighted", batch, in, ref_offsets, support_thresh_px, reproj_thresh, xyz_out, err_out, status,
                       counters, precision, true);
}

// ---- per-point surface normals (lfd_normals.hip) ----------------------------------------------------------------------------------------------
int lfd_estimate_normals(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets, int32_t radius_cells,
                         float depth_step_rel, float reproj_thresh, float* normals_out, uint8_t* status, int64_t* counters) {
    if (int rc = device_guard(ctx)) return rc;
    if (const char* why = lfd_normals_check(in, ref_offsets, radius_cells, depth_step_rel, reproj_thresh, normals_out, status))
        return fail(ctx, LFD_ERR_INVALID, std::string("lfd_estimate_normals: ") + why);
    LfdNormalArgs p = {};
    int rc = fill_stage(ctx, batch, in, ref_offsets, 0.0f, reproj_thresh, p.st);
    if (rc != LFD_OK) return rc;
    p.normals = normals_out; p.status = status;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    p.radius = radius_cells; p.depth_step_rel = depth_step_rel;
    LFD_HIP(ctx, lfd_normals_launch(p, ctx->stream));
    return LFD_OK;
}

// ---- multi-view point colour (lfd_colour.hip) --------------------------------------------------------------------------------------------------
int lfd_colour_multiview(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets,
                         const uint8_t* const* nbr_image, float support_thresh_px, int32_t mode, float* rgb_out, uint8_t* status,
                         int64_t* counters) {
    if (int rc = device_guard(ctx)) return rc;
    if (const char* why = lfd_colour_check(in, ref_offsets, nbr_image, support_thresh_px, mode, rgb_out, status))
        return fail(ctx, LFD_ERR_INVALID, std::string("lfd_colour_multiview: ") + why);
    LfdColourArgs p = {};
    int rc = fill_stage(ctx, batch, in, ref_offsets, support_thresh_px, 0.0f, p.st);
    if (rc != LFD_OK) return rc;
    if (const char* why = lfd_colour_check_images(batch, nbr_image)) return fail(ctx, LFD_ERR_INVALID, std::string("lfd_colour_multiview: ") + why);
    rc = upload_image_table(ctx, batch, nbr_image, &p.img);
    if (rc != LFD_OK) return rc;
    p.o_rgb = rgb_out; p.status = status;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    p.mode = mode;
    LFD_HIP(ctx, lfd_colour_launch(p, ctx->stream));
    return LFD_OK;
}

// ---- per-image exposure gains (lfd_gain.hip) ----------------------------------------------------------------------------------------------------
int lfd_gain_accumulate(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets,
                        const uint8_t* const* nbr_image, float support_thresh_px, uint64_t* table) {
    if (int rc = device_guard(ctx)) return rc;
    if (const char* why = lfd_gain_check(in, ref_offsets, nbr_image, support_thresh_px, table, 0))
        return fail(ctx, LFD_ERR_INVALID, std::string("lfd_gain_accumulate: ") + why);
    LfdGainArgs p = {};
    int rc = fill_stage(ctx, batch, in, ref_offsets, support_thresh_px, 0.0f, p.st);
    if (rc != LFD_OK) return rc;
    if (const char* why = lfd_gain_check(in, ref_offsets, nbr_image, support_thresh_px, table, (long long)batch->n_refs * batch->k))
        return fail(ctx, LFD_ERR_INVALID, std::string("lfd_gain_accumulate: ") + why);
    if (const char* why = lfd_colour_check_images(batch, nbr_image)) return fail(ctx, LFD_ERR_INVALID, std::string("lfd_gain_accumulate: ") + why);
    rc = upload_image_table(ctx, batch, nbr_image, &p.img);
    if (rc != LFD_OK) return rc;
    p.table = reinterpret_cast<unsigned long long*>(table);
    LFD_HIP(ctx, lfd_gain_launch(p, ctx->stream));
    return LFD_OK;
}

int lfd_gain_apply(lfd_context* ctx, const float* rgb, int64_t n, const int64_t* ref_offsets, int32_t n_refs, const float* factors, float* rgb_out) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (const char* why = lfd_gain_apply_check(rgb, n, ref_offsets, n_refs, factors, rgb_out))
        return fail(ctx, LFD_ERR_INVALID, std::string("lfd_gain_apply: ") + why);
    LfdGainApplyArgs p;
    std::memset(&p, 0, sizeof(p));
    p.offs = reinterpret_cast<const long long*>(ref_offsets);
    p.factors = factors; p.rgb = rgb; p.o_rgb = rgb_out; p.n = n; p.n_refs = n_refs;
    LFD_HIP(ctx, lfd_gain_apply_launch(p, ctx->stream));
    return LFD_OK;
}

// ---- epipolar audit (lfd_audit.hip) -----------------------------------------------------------------------------------------------------------------
int lfd_epipolar_audit(lfd_context* ctx, const lfd_batch* batch, float audit_certainty, uint64_t* table, uint8_t* best) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (const char* why = lfd_audit_check(audit_certainty, table)) return fail(ctx, LFD_ERR_INVALID, std::string("lfd_epipolar_audit: ") + why);
    LfdLaunch L;
    int rc = batch_launch(ctx, batch, L);
    if (rc != LFD_OK) return rc;
    if (const char* why = lfd_audit_check_batch(batch, table, best)) return fail(ctx, LFD_ERR_INVALID, std::string("lfd_epipolar_audit: ") + why);
    LfdAuditArgs p;
    std::memset(&p, 0, sizeof(p));
    p.refs = L.refs; p.slots = L.slots; p.ref_const = L.ref_const; p.pair_const = L.pair_const;
    p.axis_x = L.axis_x; p.axis_y = L.axis_y;
    p.table = reinterpret_cast<unsigned long long*>(table);
    p.best = best;
    p.n_refs = batch->n_refs; p.k = batch->k;
    p.audit_certainty = audit_certainty;
    p.g = launch_geom(batch, L, 0.0f, 0.0f);
    const char* e = std::getenv("LFD_AUDIT_NO_AGGREGATE");             // profiling: every confident lane issues its own LDS adds (the same table)
    LFD_HIP(ctx, lfd_audit_launch(p, !(e && std::atoi(e) != 0), ctx->stream));
    return LFD_OK;
}

// ---- pose corrections from the matches (lfd_pose.hip) -------------------------------------------------------------------------------------------
// The pairs' constants are derived here, once per launch, from the camera table as it was uploaded (f64 from its f32 values; batch->fundamental
// is not used), and travel to the device like the pointer tables: compared with what the device holds, uploaded on the launch stream when they
// differ.
int lfd_pose_accumulate(lfd_context* ctx, const lfd_batch* batch, float pose_certainty, float pose_inlier_px, int64_t* table) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (const char* why = lfd_pose_check(pose_certainty, pose_inlier_px, table)) return fail(ctx, LFD_ERR_INVALID, std::string("lfd_pose_accumulate: ") + why);
    LfdLaunch L;
    int rc = batch_launch(ctx, batch, L);
    if (rc != LFD_OK) return rc;
    if (const char* why = lfd_pose_check_batch(batch, table)) return fail(ctx, LFD_ERR_INVALID, std::string("lfd_pose_accumulate: ") + why);
    std::vector<unsigned char> blob((size_t)batch->n_refs * batch->k * sizeof(LfdPoseConst), 0);
    LfdPoseConst* pc = reinterpret_cast<LfdPoseConst*>(blob.data());
    for (int r = 0; r < batch->n_refs; ++r)
        for (int j = 0; j < batch->n_slots[r]; ++j) {
            const size_t s = (size_t)r * batch->k + j;
            lfd_pose_make_const(ctx->host_cams[(size_t)batch->ref_cam[r]], ctx->host_cams[(size_t)batch->nbr_cam[s]], pc[s]);
        }
    const void* d_pc = nullptr;
    rc = upload_blob_table(ctx, ctx->pose_const, blob, &d_pc);
    if (rc != LFD_OK) return rc;
    LfdPoseArgs p;
    std::memset(&p, 0, sizeof(p));
    p.refs = L.refs; p.slots = L.slots; p.ref_const = L.ref_const; p.pair_const = L.pair_const;
    p.pose_const = static_cast<const LfdPoseConst*>(d_pc);
    p.axis_x = L.axis_x; p.axis_y = L.axis_y;
    p.table = reinterpret_cast<unsigned long long*>(table);
    p.n_refs = batch->n_refs; p.k = batch->k;
    p.pose_certainty = pose_certainty;
    p.c2 = (double)pose_inlier_px * (double)pose_inlier_px;
    p.g = launch_geom(batch, L, 0.0f, 0.0f);
    LFD_HIP(ctx, lfd_pose_launch(p, ctx->stream));
    return LFD_OK;
}

// ---- far-field shell (lfd_far.hip) -----------------------------------------------------------------------------------------------------------------
int lfd_far_accumulate(lfd_context* ctx, const lfd_batch* batch, float far_thresh_px, float far_certainty, int32_t far_min_views,
                       int32_t shell_cells, uint64_t* table, int64_t* counters) {
    return lfd_far_accumulate_flags(ctx, batch, far_thresh_px, far_certainty, far_min_views, shell_cells, table, counters, nullptr);
}

int lfd_far_accumulate_flags(lfd_context* ctx, const lfd_batch* batch, float far_thresh_px, float far_certainty, int32_t far_min_views,
                             int32_t shell_cells, uint64_t* table, int64_t* counters, uint8_t* flags) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (const char* why = lfd_far_check(far_thresh_px, far_certainty, far_min_views, shell_cells, table))
        return fail(ctx, LFD_ERR_INVALID, std::string("lfd_far_accumulate: ") + why);
    LfdLaunch L;
    int rc = batch_launch(ctx, batch, L);
    if (rc != LFD_OK) return rc;
    if (const char* why = lfd_far_check_batch(batch, shell_cells, table, counters, flags))
        return fail(ctx, LFD_ERR_INVALID, std::string("lfd_far_accumulate: ") + why);
    if (batch->n_refs > 65535) return fail(ctx, LFD_ERR_INVALID, "lfd_far_accumulate: at most 65535 references per batch");
    LfdFarArgs p;
    std::memset(&p, 0, sizeof(p));
    p.cams = L.cams; p.refs = L.refs; p.slots = L.slots; p.ref_const = L.ref_const; p.pair_const = L.pair_const;
    p.axis_x = L.axis_x; p.axis_y = L.axis_y;
    p.table = reinterpret_cast<unsigned long long*>(table);
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    p.flags = flags;
    if (flags) LFD_HIP(ctx, hipMemsetAsync(flags, 0, (size_t)batch->n_refs * batch->H * batch->W, ctx->stream));
    p.n_refs = batch->n_refs; p.k = batch->k; p.S = shell_cells; p.min_views = far_min_views;
    p.far_certainty = far_certainty;
    p.g = launch_geom(batch, L, far_thresh_px, 0.0f);
    const char* e = std::getenv("LFD_FAR_NO_REDUCE");                  // profiling: every far lane issues its own adds (the same table)
    LFD_HIP(ctx, lfd_far_launch(p, !(e && std::atoi(e) != 0), ctx->stream));
    return LFD_OK;
}

int lfd_far_emit(lfd_context* ctx, const uint64_t* table, int32_t shell_cells, int64_t min_samples, const double* centre, double radius,
                 float* xyz, float* rgb, float* normal, int32_t* samples, int64_t capacity, int64_t* n_out) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (const char* why = lfd_far_emit_check(table, shell_cells, min_samples, centre, radius, xyz, rgb, normal, samples, capacity, n_out))
        return fail(ctx, LFD_ERR_INVALID, std::string("lfd_far_emit: ") + why);
    *n_out = 0;
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const long long n_cells = 6LL * shell_cells * shell_cells;
    const CloudPlan p = cloud_plan(n_cells);
    CloudCompact c;
    if (int rc = carve_cloud_ws(ctx, [&](Bump& b) { c = carve_compact(b, p, 0); })) return rc;
    LFD_HIP(ctx, lfd_far_mark_launch(reinterpret_cast<const unsigned long long*>(table), n_cells, (long long)min_samples, c.keep, st));
    cloud_compact_prefix(st, p, c);
    LfdFarEmitArgs a;
    std::memset(&a, 0, sizeof(a));
    a.table = reinterpret_cast<const unsigned long long*>(table); a.keep = c.keep; a.wg_kept = c.wg_kept;
    for (int i = 0; i < 3; ++i) a.centre[i] = centre[i];
    a.radius = radius;
    a.xyz = xyz; a.rgb = rgb; a.normal = normal; a.samples = samples;
    a.n_cells = n_cells; a.capacity = capacity; a.min_samples = min_samples;
    LFD_HIP(ctx, lfd_far_emit_launch(a, st));
    LFD_HIP(ctx, hipMemcpyAsync(ctx->pinned_words, c.wg_kept + p.n_wg, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    LFD_HIP(ctx, hipStreamSynchronize(st));                            // the workspace is free for the next stage on return
    *n_out = (int64_t)(unsigned)ctx->pinned_words[0];
    if (*n_out > capacity) return fail(ctx, LFD_ERR_CAPACITY, "lfd_far_emit: the shell has more points than capacity (n_out holds the number)");
    return LFD_OK;
}

// ---- photo-consistency gate (lfd_photo.hip) -----------------------------------------------------------------------------------------------------
int lfd_photo_gate(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets_in,
                   const uint8_t* const* nbr_image, int32_t window_cells, float min_ncc, float min_texture, const lfd_points* out,
                   int64_t* ref_offsets_out, int32_t* seg_counts_out, uint8_t* status, float* ncc, int64_t* counters) {
    if (int rc = device_guard(ctx)) return rc;
    int code = LFD_ERR_INVALID;
    if (const char* why = lfd_photo_check(in, ref_offsets_in, nbr_image, window_cells, min_ncc, min_texture, out, ref_offsets_out, status, ncc,
                                          counters, &code))
        return fail(ctx, code, std::string("lfd_photo_gate: ") + why);
    LfdPhotoArgs p = {};
    int rc = fill_stage(ctx, batch, in, ref_offsets_in, 0.0f, 0.0f, p.st);
    if (rc != LFD_OK) return rc;
    if (const char* why = lfd_colour_check_images(batch, nbr_image)) return fail(ctx, LFD_ERR_INVALID, std::string("lfd_photo_gate: ") + why);
    rc = upload_image_table(ctx, batch, nbr_image, &p.img);
    if (rc != LFD_OK) return rc;
    GateWs w;
    rc = carve_gate_ws(ctx, p.st, false, seg_counts_out, w);
    if (rc != LFD_OK) return rc;
    p.seg_counts = seg_counts_out; p.status = status; p.ncc = ncc;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    p.keep = w.keep; p.wg_kept = w.wg_kept;
    p.radius = window_cells;
    p.th = lfd_photo_thresholds(min_ncc, min_texture);
    LFD_HIP(ctx, lfd_photo_launch(p, compact_args(p.st, w, out, ref_offsets_out, nullptr), ctx->stream));
    return LFD_OK;
}

// ---- depth-uncertainty gate (lfd_sigma.hip) ---------------------------------------------------------------------------------------------------
int lfd_depth_sigma_filter(lfd_context* ctx, const lfd_batch* batch, const lfd_points* in, const int64_t* ref_offsets_in,
                           const float* const* precision, float iso_sigma_px, const uint8_t* refine_status, float support_thresh_px,
                           float max_rel_sigma, const lfd_points* out, int64_t* ref_offsets_out, int32_t* seg_counts_out, float* sigma_rel,
                           float* sigma_rel_out) {
    if (int rc = device_guard(ctx)) return rc;
    int code = LFD_ERR_INVALID;
    if (const char* why = lfd_sigma_check(in, ref_offsets_in, precision, iso_sigma_px, refine_status, support_thresh_px, max_rel_sigma, out,
                                          ref_offsets_out, sigma_rel, sigma_rel_out, &code))
        return fail(ctx, code, std::string("lfd_depth_sigma_filter: ") + why);
    LfdSigmaArgs p = {};
    int rc = fill_stage(ctx, batch, in, ref_offsets_in, refine_status ? support_thresh_px : 0.0f, 0.0f, p.st);
    if (rc != LFD_OK) return rc;
    if (precision) {
        if (const char* why = lfd_refine_check_precision(batch, precision)) return fail(ctx, LFD_ERR_INVALID, std::string("lfd_depth_sigma_filter: ") + why);
        rc = upload_precision_table(ctx, batch, precision, &p.prec);
        if (rc != LFD_OK) return rc;
    } else {
        p.iso = lfd_recip_refined((double)iso_sigma_px * (double)iso_sigma_px);     // (host build: the IEEE quotient, as in the twin)
    }
    GateWs w;
    rc = carve_gate_ws(ctx, p.st, sigma_rel_out != nullptr, seg_counts_out, w);
    if (rc != LFD_OK) return rc;
    p.seg_counts = seg_counts_out; p.sigma = sigma_rel; p.status = refine_status;
    p.ws_sigma = w.extra; p.keep = w.keep; p.wg_kept = w.wg_kept;
    p.max_rel_sigma = max_rel_sigma;
    LFD_HIP(ctx, lfd_sigma_launch(p, compact_args(p.st, w, out, ref_offsets_out, sigma_rel_out), ctx->stream));
    return LFD_OK;
}

int lfd_copy_segments(void* hip_stream, int32_t device_index, const void* src, void* dst, const lfd_copy_segment* segs, int32_t n) {
    if (n < 0 || (n > 0 && (!src || !dst || !segs))) return LFD_ERR_INVALID;
    if (n == 0) return LFD_OK;
    if (hipSetDevice(device_index) != hipSuccess) return LFD_ERR_HIP;
    for (int32_t first = 0; first < n;) {
        LfdCopyArgs A;
        int m = 0;
        long long chunks = 0;
        A.chunk0[0] = 0;
        for (; first < n && m < LFD_COPY_MAX_SEGS; ++first) {
            const lfd_copy_segment& sg = segs[first];
            if (sg.nbytes < 0 || sg.src_offset < 0 || sg.dst_offset < 0) return LFD_ERR_INVALID;
            if (sg.nbytes == 0) continue;
            const long long c = (sg.nbytes + LFD_COPY_CHUNK - 1) / LFD_COPY_CHUNK;
            if (chunks + c > 0x7fffffffLL) { if (m == 0) return LFD_ERR_INVALID; break; }       // (one launch's grid is full: the rest goes into the next)
            A.src[m] = sg.src_offset; A.dst[m] = sg.dst_offset; A.n[m] = sg.nbytes;
            chunks += c;
            A.chunk0[++m] = (int)chunks;
        }
        if (m == 0) continue;
        A.n_segs = m;
        hipLaunchKernelGGL(lfd_copy_segments_kernel, dim3((unsigned)chunks), dim3(256), 0, static_cast<hipStream_t>(hip_stream), A,
                           static_cast<const unsigned char*>(src), static_cast<unsigned char*>(dst));
        if (hipGetLastError() != hipSuccess) return LFD_ERR_HIP;
    }
    return LFD_OK;
}

int lfd_quantise_rgb(lfd_context* ctx, const float* rgb, int64_t n, uint8_t* out) {
    if (!ctx) return fail(nullptr, LFD_ERR_INVALID, "null context");
    if (ctx->is_host) return fail(ctx, LFD_ERR_STATE, "device entry point called on a host context");
    if (n < 0 || (n > 0 && (!rgb || !out))) return fail(ctx, LFD_ERR_INVALID, "bad arguments");
    if (n == 0) return LFD_OK;
    LFD_HIP(ctx, hipSetDevice(ctx->device));
    const long long n3 = 3 * (long long)n;
    const unsigned grid = (unsigned)std::min<long long>((n3 + 255) / 256, 4096);
    hipLaunchKernelGGL(lfd_quantise_rgb_kernel, dim3(grid), dim3(256), 0, ctx->stream, rgb, n3, out);
    LFD_HIP(ctx, hipGetLastError());
    return LFD_OK;
}

// ---- host-side helpers -----------------------------------------------------------------------
int lfd_identity_axis(int32_t n, float* out) {
    if (n <= 0 || !out) return LFD_ERR_INVALID;
    const LfdAxis a = lfd_make_axis(n);
    for (int j = 0; j < n; ++j) out[j] = lfd_axis_value(a, j);
    return LFD_OK;
}

float lfd_parallax_dot_threshold(float min_deg) {
    // ang(d) = (float)acosf(clip(d)) * (180/pi as f32) is non-increasing in d; find the largest f32 d
    // in [-1, 1] with ang(d) >= min_deg by bisection over the ordered f32 bit patterns.
    const float k = 57.295776f;   // 180.0f / NPY_PIf, the constant np.degrees uses for f32
    auto ok = [&](float d) { return acosf(d) * k >= min_deg; };
    if (!ok(-1.0f)) return -2.0f;             // nothing passes (min_deg > 180)
    if (ok(1.0f)) return 1.0f;                // everything in range passes (min_deg <= 0)
    auto key = [](float f) { int32_t i; std::memcpy(&i, &f, 4); return i >= 0 ? (int64_t)i : -(int64_t)(i & 0x7fffffff); };
    auto unkey = [](int64_t kx) { int32_t i = kx >= 0 ? (int32_t)kx : (int32_t)(0x80000000u | (uint32_t)(-kx)); float f; std::memcpy(&f, &i, 4); return f; };
    int64_t lo = key(-1.0f), hi = key(1.0f);   // ok(lo) true, ok(hi) false
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (ok(unkey(mid))) lo = mid; else hi = mid;
    }
    return unkey(lo);
}

int lfd_host_fundamental(const float* K1, const float* R1, const float* t1, const float* K2, const float* R2,
                         const float* t2, float* F_out) {
    if (!K1 || !R1 || !t1 || !K2 || !R2 || !t2 || !F_out) return LFD_ERR_INVALID;
    lfd_fundamental(K1, R1, t1, K2, R2, t2, F_out);
    return LFD_OK;
}

static void unpack_cam(const float* v, LfdCam& c) {
    std::memcpy(c.K, v, 9 * 4); std::memcpy(c.R, v + 9, 9 * 4); std::memcpy(c.t, v + 18, 3 * 4);
    std::memcpy(c.P, v + 21, 12 * 4); std::memcpy(c.C, v + 33, 3 * 4);
    c.w = (int32_t)v[36]; c.h = (int32_t)v[37]; c.pad[0] = c.pad[1] = 0;
}

int lfd_host_null_vector(const float* A16, double* out4) {
    if (!A16 || !out4) return -LFD_ERR_INVALID;
    return lfd_null_vector(A16, out4);
}

int lfd_host_null_vector_sym(const double* M10, double* out4) {
    if (!M10 || !out4) return -LFD_ERR_INVALID;
    return lfd_null_vector_sym(M10, out4);
}

int lfd_host_eval_correspondence(const float* cam1, const float* cam2, float xa_norm, float ya_norm, float xb_norm,
                                 float yb_norm, int32_t w_match, int32_t h_match, const lfd_params* params, float* out8) {
    if (!cam1 || !cam2 || !params || !out8 || w_match <= 1 || h_match <= 1) return LFD_ERR_INVALID;
    LfdCam a, b;
    unpack_cam(cam1, a); unpack_cam(cam2, b);
    LfdRefConst rc; LfdPairConst pc;
    lfd_make_ref_const(a, w_match, h_match, rc);
    lfd_make_pair_const(a, b, 1, w_match, h_match, pc);
    lfd_batch bb; std::memset(&bb, 0, sizeof(bb));
    bb.w_match = w_match; bb.h_match = h_match;
    LfdKernelParams kp;
    lfd_fill_kernel_params(&bb, params, kp);
    LfdCellResult res;
    lfd_eval_correspondence(rc, pc, xa_norm, ya_norm, xb_norm, yb_norm, kp, res);
    out8[0] = res.x; out8[1] = res.y; out8[2] = res.z; out8[3] = 0.0f; out8[4] = 0.0f; out8[5] = 0.0f;
    out8[6] = res.err; out8[7] = (float)res.keep;
    return LFD_OK;
}

}  // extern "C"
