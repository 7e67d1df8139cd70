// Multi-view support filter on the device (lfd_support_filter): every triangulated point is checked against the OTHER neighbours of
// its reference and the points that at least min_support of them confirm are compacted in order.
//
// Gather-bound: per input point 17 B of its own fields and 12 B (certainty 4, warp pair 8) per other neighbour, 28-33 B per survivor moved.
// Three launches, nothing waits for another workgroup:
//
//   lfd_support_count_kernel<KMAX>   a lane per input point: support count, a keep byte and the kept points of the workgroup;
//                                    per (reference, winning slot) counters through LDS, then one integer atomic per workgroup and slot
//   lfd_compact_scan_kernel          one workgroup: exclusive prefix of the workgroups' counts, then ref_offsets_out from it
//   lfd_compact_scatter_kernel       a lane per input point: rank inside the wave by ballot / mbcnt, inside the workgroup by wave sums, copy
//
// The scan and the scatter (lfd_compact_launch) are the tail of every gate behind triangulation: this filter's, the depth-uncertainty gate's
// (lfd_sigma.hip) and the photo-consistency gate's (lfd_photo.hip).  All they know of a verdict is the keep byte.
//
// A point's reference comes from ref_offsets_in (device data: the host does not know the totals); the grid covers in->capacity and the
// workgroups past the total retire at once.  The constants of the reference a workgroup works on (other neighbours' plane pointers, projection
// rows, pixel scales) are staged in LDS; a workgroup whose points straddle references takes them one after the other.  That front end is
// lfd_device.hpp's (lfd_point_span ... lfd_count_flush), shared by all the per-point kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_device.hpp"
#include "lfd_support.hpp"

template <int KMAX>
__global__ void __launch_bounds__(256) lfd_support_count_kernel(const LfdSupportArgs p) {
    __shared__ LfdSlot sh[KMAX];
    __shared__ unsigned sh_seg[KMAX];
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
    const float X0 = st.xyz[3 * ii], X1 = st.xyz[3 * ii + 1], X2 = st.xyz[3 * ii + 2];
    int r_first, r_last;
    const int r = lfd_ref_range<1>(sh_ref, &sh_kept, st, sp, r_first, r_last);
    const LfdSupportGeom g = st.g;
    const long long HW = (long long)g.H * g.W;
    const bool cell_ok = cell >= 0 && (long long)cell < HW;            // no address is formed from a cell outside the grid
    int support = 0;
    for (int rr = r_first; rr <= r_last; ++rr) {
        if (lfd_ref_empty(st, rr)) continue;
        const int ns = lfd_ref_slots<KMAX>(st, rr);
        if (tid < KMAX) sh_seg[tid] = 0u;
        lfd_stage_slots(sh, st.slots, st.pair_const, rr, st.k, ns);
        __syncthreads();
        const bool here = mine && r == rr;
        if (here && cell_ok) {
            // all gathers of the point first, then the arithmetic
            float c[KMAX];
            float2 w[KMAX];
#pragma unroll
            for (int j = 0; j < KMAX; ++j) {
                c[j] = 0.0f; w[j] = make_float2(0.0f, 0.0f);
                if (j < ns && j != s) {
                    c[j] = sh[j].cert[cell];
                    w[j] = *reinterpret_cast<const float2*>(sh[j].warp + (size_t)cell * g.C + (g.C - 2));
                }
            }
#pragma unroll
            for (int j = 0; j < KMAX; ++j) {
                if (j < ns && j != s) support += lfd_support_candidate(sh[j], g, c[j], w[j].x, w[j].y, X0, X1, X2) ? 1 : 0;
            }
        }
        if (p.seg_counts) lfd_seg_tally<KMAX>(sh_seg, here && support >= p.min_support, s);
        __syncthreads();
        if (p.seg_counts) lfd_seg_flush(sh_seg, p.seg_counts, rr, st.k, ns);
    }
    const bool keep = mine && support >= p.min_support;
    if (mine) {
        p.keep[i] = keep ? (uint8_t)1 : (uint8_t)0;
        if (p.support) p.support[i] = (uint8_t)support;
    }
    lfd_count_tally<1>(&sh_kept, {keep});
    __syncthreads();
    if (tid == 0) p.wg_kept[blockIdx.x] = sh_kept;
}

// exclusive prefix of wg_kept[0 .. n_wg) in place (the total goes to wg_kept[n_wg]), then ref_offsets_out[r] = kept points before
// ref_offsets_in[r]: the prefix of that point's workgroup plus the kept points in front of it inside the workgroup.  One workgroup.
__global__ void __launch_bounds__(1024) lfd_compact_scan_kernel(const LfdCompactArgs p) {
    __shared__ unsigned wave_sum[16];
    unsigned* v = p.wg_kept;
    const int m = p.n_wg;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (m + 1023) / 1024;
    const int a = (long long)tid * per < m ? tid * per : m;
    const int b = a + per < m ? a + per : m;
    unsigned sum = 0u;
    for (int i = a; i < b; ++i) sum += v[i];
    unsigned incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    unsigned run = incl - sum;
    for (int w = 0; w < wave; ++w) run += wave_sum[w];
    if (tid == 1023) v[m] = run + sum;
    for (int i = a; i < b; ++i) {
        const unsigned c = v[i];
        v[i] = run;
        run += c;
    }
    __threadfence_block();
    __syncthreads();
    const long long total = lfd_support_clamp(p.offs_in[p.n_refs], p.capacity);
    for (int r = tid; r <= p.n_refs; r += 1024) {
        long long at = lfd_support_clamp(p.offs_in[r], p.capacity);
        at = at > total ? total : at;
        const long long wg = at >> 8;                                  // <= n_wg; == n_wg only with nothing to walk
        long long acc = v[wg];
        for (long long q = wg << 8; q < at; ++q) acc += p.keep[q] ? 1 : 0;
        p.offs_out[r] = acc;
    }
}

__global__ void __launch_bounds__(256) lfd_compact_scatter_kernel(const LfdCompactArgs p) {
    __shared__ unsigned wc[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long total = lfd_support_clamp(p.offs_in[p.n_refs], p.capacity);
    const long long base = (long long)blockIdx.x * 256;
    if (base >= total) return;
    const long long i = base + tid;
    const bool keep = i < total && p.keep[i] != 0;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wc[wave] = (unsigned)__popcll(m);
    __syncthreads();
    if (!keep) return;
    unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    for (int w = 0; w < wave; ++w) rank += wc[w];
    const long long o = (long long)p.wg_kept[blockIdx.x] + rank;       // < total <= in->capacity <= out->capacity
    p.o_xyz[3 * o] = p.xyz[3 * i]; p.o_xyz[3 * o + 1] = p.xyz[3 * i + 1]; p.o_xyz[3 * o + 2] = p.xyz[3 * i + 2];
    p.o_rgb[3 * o] = p.rgb[3 * i]; p.o_rgb[3 * o + 1] = p.rgb[3 * i + 1]; p.o_rgb[3 * o + 2] = p.rgb[3 * i + 2];
    p.o_err[o] = p.err[i];
    if (p.o_cell) p.o_cell[o] = p.cell[i];
    if (p.o_slot) p.o_slot[o] = p.slot[i];
    if (p.extra_out) p.extra_out[o] = p.extra_in[i];                   // (uniform)
}

// The compaction behind a per-point verdict: scan, then scatter, of the points whose keep byte is set.  The scan runs even without a workgroup
// to scan: ref_offsets_out is its to write.
hipError_t lfd_compact_launch(const LfdCompactArgs& p, hipStream_t stream) {
    hipLaunchKernelGGL(lfd_compact_scan_kernel, dim3(1), dim3(1024), 0, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (p.n_wg > 0) {
        hipLaunchKernelGGL(lfd_compact_scatter_kernel, dim3((unsigned)p.n_wg), dim3(256), 0, stream, p);
        e = hipGetLastError();
    }
    return e;
}

// lfd_api.hip's lfd_support_filter: the arguments were validated there (capacity <= 2^31 - 1: at most 2^23 workgroups)
hipError_t lfd_support_launch(const LfdSupportArgs& p, const LfdCompactArgs& tail, hipStream_t stream) {
    if (p.st.n_wg > 0) {
        const dim3 grid((unsigned)p.st.n_wg);
        if (p.st.k <= 4) hipLaunchKernelGGL(lfd_support_count_kernel<4>, grid, dim3(256), 0, stream, p);
        else if (p.st.k <= 8) hipLaunchKernelGGL(lfd_support_count_kernel<8>, grid, dim3(256), 0, stream, p);
        else hipLaunchKernelGGL(lfd_support_count_kernel<LFD_MAX_SLOTS>, grid, dim3(256), 0, stream, p);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return lfd_compact_launch(tail, stream);
}
