// Multi-view point colour on the device (lfd_colour_multiview): every point's colour from all the views that see it - its
// reference, the neighbour that won it and the other neighbours lfd_support_candidate accepts - as their mean or median (lfd_colour.hpp).
//
// One launch, a lane per input point, nothing waits for another workgroup and nothing is scanned: the points stay where they are and only
// their colour is written.  The front end is the per-point kernels' common one (lfd_device.hpp): coalesced loads of the point's own fields, its
// reference from ref_offsets (device data), the reference's neighbours - and here their image bases - staged in LDS (a workgroup whose points
// straddle references takes them one after the other), so that inside a reference every image base is uniform.  Certainty (4 B) and warp pair
// (8 B) of every neighbour are issued before any arithmetic; the taps follow per view that takes part, 4 byte triplets each.  Gather-bound:
// occupancy hides the latency, nothing is staged in LDS and nothing goes to scratch memory - the views' colours are registers (compile-time
// indices only; the winning slot, a run-time index, is read from LDS and sampled on its own).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_device.hpp"
#include "lfd_colour.hpp"

// (amdgpu_waves_per_eu(4): at most 128 VGPRs.  Left alone the allocator gives the <8, median> instantiation 177 - two waves per SIMD, too few
// to hide a gather; with the hint it takes 92 and, like all six, no scratch memory - DESIGN 4.21 has the table.)
template <int KMAX, int MODE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) lfd_colour_kernel(const LfdColourArgs p) {
    __shared__ LfdSlot sh[KMAX];
    __shared__ const uint8_t* sh_img[KMAX];
    __shared__ int sh_ref[2];
    __shared__ unsigned sh_cnt[2];
    const int tid = (int)threadIdx.x;
    const LfdPointStage& st = p.st;
    const LfdPointSpan sp = lfd_point_span(st);
    if (!sp.any) return;                                                // the whole workgroup lies past the last point
    const long long i = sp.i, ii = sp.ii;
    const bool mine = sp.mine;
    const int cell = st.cell[ii];
    const int s = (int)st.slot[ii];
    const float X0 = st.xyz[3 * ii], X1 = st.xyz[3 * ii + 1], X2 = st.xyz[3 * ii + 2];
    float rgb[3] = {st.rgb[3 * ii], st.rgb[3 * ii + 1], st.rgb[3 * ii + 2]};
    int r_first, r_last;
    const int r = lfd_ref_range<2>(sh_ref, sh_cnt, st, sp, r_first, r_last);
    const LfdSupportGeom g = st.g;
    const long long HW = (long long)g.H * g.W;
    unsigned n_views = 0u;
    for (int rr = r_first; rr <= r_last; ++rr) {
        if (lfd_ref_empty(st, rr)) continue;
        const int ns = lfd_ref_slots<KMAX>(st, rr);
        lfd_stage_slots(sh, st.slots, st.pair_const, rr, st.k, ns);
        if (tid < ns) sh_img[tid] = p.img[(size_t)rr * st.k + tid];
        __syncthreads();
        if (mine && r == rr && !lfd_colour_guarded(X0, X1, X2, rgb[0], rgb[1], rgb[2], cell, HW, s, ns)) {
            // all gathers of the point first, then the arithmetic
            float c[KMAX], wx[KMAX], wy[KMAX];
            const float2 ws = *reinterpret_cast<const float2*>(sh[s].warp + (size_t)cell * g.C + (g.C - 2));
#pragma unroll
            for (int j = 0; j < KMAX; ++j) {
                c[j] = 0.0f; wx[j] = 0.0f; wy[j] = 0.0f;
                if (j < ns && j != s) {
                    c[j] = sh[j].cert[cell];
                    const float2 w = *reinterpret_cast<const float2*>(sh[j].warp + (size_t)cell * g.C + (g.C - 2));
                    wx[j] = w.x; wy[j] = w.y;
                }
            }
            n_views = lfd_colour_point<KMAX, MODE>(sh, sh_img, ns, s, g, c, wx, wy, ws.x, ws.y, X0, X1, X2, rgb);
        }
        __syncthreads();                                               // the next reference's constants replace these
    }
    if (mine) {
        p.o_rgb[3 * i] = rgb[0]; p.o_rgb[3 * i + 1] = rgb[1]; p.o_rgb[3 * i + 2] = rgb[2];
        if (p.status) p.status[i] = (uint8_t)n_views;
    }
    if (p.counters) {                                                  // (uniform)
        lfd_count_tally<1>(sh_cnt, {mine && n_views != 0u});
        unsigned sum = mine ? n_views : 0u;                            // the second counter is a sum, not a count
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
        if ((tid & 63) == 0 && sum) atomicAdd(&sh_cnt[1], sum);
        __syncthreads();
        lfd_count_flush<2>(sh_cnt, p.counters);
    }
}

template <int MODE>
static void lfd_colour_launch_k(const LfdColourArgs& p, hipStream_t stream) {
    const dim3 grid((unsigned)p.st.n_wg);
    if (p.st.k <= 4) hipLaunchKernelGGL((lfd_colour_kernel<4, MODE>), grid, dim3(256), 0, stream, p);
    else if (p.st.k <= 8) hipLaunchKernelGGL((lfd_colour_kernel<8, MODE>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((lfd_colour_kernel<LFD_MAX_SLOTS, MODE>), grid, dim3(256), 0, stream, p);
}

// lfd_api.hip's lfd_colour_multiview: the arguments were validated there (capacity <= 2^31 - 1: at most 2^23 workgroups, mode 1 or 2)
hipError_t lfd_colour_launch(const LfdColourArgs& p, hipStream_t stream) {
    if (p.st.n_wg <= 0) return hipSuccess;
    if (p.mode == LFD_COLOUR_MEAN) lfd_colour_launch_k<LFD_COLOUR_MEAN>(p, stream);
    else lfd_colour_launch_k<LFD_COLOUR_MEDIAN>(p, stream);
    return hipGetLastError();
}
