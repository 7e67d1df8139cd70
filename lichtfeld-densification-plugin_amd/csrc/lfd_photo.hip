// Photo-consistency gate on the device (lfd_photo_gate): every triangulated point's match is tested by the ZNCC of the two
// patches it joins, over a (2R + 1)^2 window of grid cells around the point's own cell (lfd_photo.hpp), and the points that are not refuted
// are compacted in order.
//
// Three launches, nothing waits for another workgroup.  The first is this file's:
//
//   lfd_photo_count_kernel<R>   a lane per input point: the six integer sums of its window in registers, the verdict, a keep byte, the
//                               optional status and ncc, and the kept points of the workgroup; per (reference, winning slot) counters and
//                               the five status counts through LDS, then one integer atomic per workgroup and counter
//
// The scan and the scatter are the shared tail of the gates (lfd_compact_launch, lfd_support.hip).
//
// The frame is the per-point kernels' common one (lfd_device.hpp: lfd_point_span ... lfd_count_flush): coalesced loads of the point's own fields, its reference from ref_offsets (device
// data), the reference's image, mask and its neighbours' plane pointers and image bases staged in LDS (a workgroup whose points straddle
// references takes them one after the other), so that inside a reference every base is uniform across the workgroup but for the winning
// slot, a run-time index into LDS.  A whole window row's certainty and warp loads are issued before its arithmetic; in dense mode neighbouring
// lanes hold neighbouring cells, so a row's loads coalesce across the lanes and the windows of a wave overlap in the caches.  The row is
// walked by a loop that is NOT unrolled: the two bilinear samplers exist once per kernel and only the six sums and the row's values live
// across it.  One instantiation per radius, so that the row's values are registers.  Gather-bound (per participating cell four unaligned 8-byte
// loads, a row's two taps each - lfd_bilinear_fetch, the dense kernel's form of the blend): occupancy hides the latency, nothing goes to scratch
// memory.  No address is formed from a cell outside the grid.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_device.hpp"
#include "lfd_photo.hpp"

hipError_t lfd_compact_launch(const LfdCompactArgs& p, hipStream_t stream);   // lfd_support.hip

// a[e] for a run-time e through compile-time indices: the array stays in registers (lfd_normals.hip has the reason for the empty statement)
template <int N>
__device__ __forceinline__ float lfd_photo_pick(const float (&a)[N], int e) {
    float v = a[0];
#pragma unroll
    for (int j = 1; j < N; ++j) {
        v = (e == j) ? a[j] : v;
        asm volatile("" : "+v"(v));
    }
    return v;
}

template <int R>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) lfd_photo_count_kernel(const LfdPhotoArgs p) {
    constexpr int NW = 2 * R + 1;
    __shared__ LfdPhotoSlot sh[LFD_MAX_SLOTS];
    __shared__ const uint8_t* sh_img_a;
    __shared__ const uint8_t* sh_mask_a;
    __shared__ unsigned sh_seg[LFD_MAX_SLOTS];
    __shared__ unsigned sh_cnt[LFD_PHOTO_STATUSES];
    __shared__ int sh_ref[2];
    __shared__ unsigned sh_kept;
    const int tid = (int)threadIdx.x;
    const LfdPointStage& st = p.st;
    const LfdPointSpan sp = lfd_point_span(st);
    if (!sp.any) {                                                      // the whole workgroup lies past the last point
        if (tid == 0) p.wg_kept[blockIdx.x] = 0u;
        return;
    }
    const long long i = sp.i, ii = sp.ii;
    const bool mine = sp.mine;
    const int cell = st.cell[ii];
    const int s = (int)st.slot[ii];
    if (tid < LFD_PHOTO_STATUSES) sh_cnt[tid] = 0u;
    int r_first, r_last;
    const int r = lfd_ref_range<1>(sh_ref, &sh_kept, st, sp, r_first, r_last);
    const LfdSupportGeom g = st.g;
    const long long HW = (long long)g.H * g.W;
    const LfdRefDesc* refs = static_cast<const LfdRefDesc*>(st.refs);
    unsigned status = LFD_PHOTO_GUARDED;
    float ncc = __builtin_nanf("");
    for (int rr = r_first; rr <= r_last; ++rr) {
        if (lfd_ref_empty(st, rr)) continue;
        const int ns = lfd_ref_slots<LFD_MAX_SLOTS>(st, rr);
        if (tid < LFD_MAX_SLOTS) sh_seg[tid] = 0u;
        if (tid < ns) {
            const LfdSlotDesc& d = static_cast<const LfdSlotDesc*>(st.slots)[(size_t)rr * st.k + tid];
            sh[tid].cert = d.cert; sh[tid].warp = d.warp; sh[tid].mask_b = d.mask_b;
            sh[tid].img = p.img[(size_t)rr * st.k + tid];
        }
        if (tid == 64) { sh_img_a = refs[rr].image; sh_mask_a = refs[rr].mask_a; }
        __syncthreads();
        const bool here = mine && r == rr;
        if (here && !lfd_photo_guarded(cell, HW, s, ns)) {
            const float* cert = sh[s].cert;
            const float* warp = sh[s].warp;
            const uint8_t* mask_b = sh[s].mask_b;
            const uint8_t* img_b = sh[s].img;
            const uint8_t* img_a = sh_img_a;
            const uint8_t* mask_a = sh_mask_a;
            const int y = cell / g.W, x = cell - y * g.W;
            LfdPhotoAcc acc;
            lfd_photo_clear(acc);
#pragma unroll 1
            for (int dy = -R; dy <= R; ++dy) {
                const int qy = y + dy;
                if (qy < 0 || qy >= g.H) continue;
                // the row's loads first (cells outside the grid: nothing is loaded, a certainty of 0), then its arithmetic
                float c[NW], wbx[NW], wby[NW];
#pragma unroll
                for (int e = 0; e < NW; ++e) {
                    const int qx = x + e - R;
                    c[e] = 0.0f; wbx[e] = 0.0f; wby[e] = 0.0f;
                    if (qx >= 0 && qx < g.W) {
                        const size_t q = (size_t)qy * g.W + qx;
                        c[e] = cert[q];
                        const float2 wb = *reinterpret_cast<const float2*>(warp + q * g.C + (g.C - 2));
                        wbx[e] = wb.x; wby[e] = wb.y;
                    }
                }
#pragma unroll 1
                for (int e = 0; e < NW; ++e) {
                    const int qx = x + e - R;
                    if (qx < 0 || qx >= g.W) continue;
                    const float xbn = lfd_photo_pick<NW>(wbx, e), ybn = lfd_photo_pick<NW>(wby, e);
                    if (!lfd_photo_participates(mask_a, mask_b, g, qx, qy, lfd_photo_pick<NW>(c, e), xbn, ybn)) continue;
                    // the cell's reference position, read only where the cell takes part: the other half of the warp's record or two axis values
                    float xan, yan;
                    if (g.C == 4) {
                        const float2 wa = *reinterpret_cast<const float2*>(warp + ((size_t)qy * g.W + qx) * 4);
                        xan = wa.x; yan = wa.y;
                    } else {
                        xan = st.axis_x[qx]; yan = st.axis_y[qy];
                    }
                    lfd_photo_sample(acc, img_a, img_b, g, xan, yan, xbn, ybn);
                }
            }
            status = lfd_photo_verdict(acc, R, p.th, &ncc);
        }
        if (p.seg_counts) lfd_seg_tally<LFD_MAX_SLOTS>(sh_seg, here && status != LFD_PHOTO_REFUTED && s < ns, s);   // (uniform)
        __syncthreads();                                               // the next reference's constants replace these
        if (p.seg_counts) lfd_seg_flush(sh_seg, p.seg_counts, rr, st.k, ns);
    }
    const bool keep = mine && status != LFD_PHOTO_REFUTED;
    if (mine) {
        p.keep[i] = keep ? (uint8_t)1 : (uint8_t)0;
        if (p.status) p.status[i] = (uint8_t)status;
        if (p.ncc) p.ncc[i] = ncc;
    }
    lfd_count_tally<1>(&sh_kept, {keep});
    if (p.counters) {                                                  // (uniform)
        bool hit[LFD_PHOTO_STATUSES];
#pragma unroll
        for (int j = 0; j < LFD_PHOTO_STATUSES; ++j) hit[j] = mine && status == (unsigned)j;
        lfd_count_tally<LFD_PHOTO_STATUSES>(sh_cnt, hit);
    }
    __syncthreads();
    if (tid == 0) p.wg_kept[blockIdx.x] = sh_kept;
    if (p.counters) lfd_count_flush<LFD_PHOTO_STATUSES>(sh_cnt, p.counters);
}

// lfd_api.hip's lfd_photo_gate: the arguments were validated there (capacity <= 2^31 - 1: at most 2^23 workgroups, radius in 1..3)
hipError_t lfd_photo_launch(const LfdPhotoArgs& p, const LfdCompactArgs& tail, hipStream_t stream) {
    if (p.st.n_wg > 0) {
        const dim3 grid((unsigned)p.st.n_wg);
        switch (p.radius) {
            case 1: hipLaunchKernelGGL((lfd_photo_count_kernel<1>), grid, dim3(256), 0, stream, p); break;
            case 2: hipLaunchKernelGGL((lfd_photo_count_kernel<2>), grid, dim3(256), 0, stream, p); break;
            case 3: hipLaunchKernelGGL((lfd_photo_count_kernel<3>), grid, dim3(256), 0, stream, p); break;
            default: return hipErrorInvalidValue;
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return lfd_compact_launch(tail, stream);
}
