// Multi-view point colour on the device (lfd_colour_multiview): every point's colour from all the views that see it - its
// reference, the neighbour that won it and the other neighbours lfd_support_candidate accepts - as their mean or median (lfd_colour.hpp).
//
// One launch, a lane per input point, nothing waits for another workgroup and nothing is scanned: the points stay where they are and only
// their colour is written.  The front end is lfd_support_count_kernel's (lfd_support.hip): coalesced loads of the point's own fields, its
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
    const LfdPointSpan sp = lfd_point_span(p.offs, p.n_refs, p.capacity);
    if (!sp.any) return;                                                // the whole workgroup lies past the last point
    const long long i = sp.i, ii = sp.ii;
    const bool mine = sp.mine;
    const int cell = p.cell[ii];
    const int s = (int)p.slot[ii];
    const float X0 = p.xyz[3 * ii], X1 = p.xyz[3 * ii + 1], X2 = p.xyz[3 * ii + 2];
    float rgb[3] = {p.rgb[3 * ii], p.rgb[3 * ii + 1], p.rgb[3 * ii + 2]};
    const int r = lfd_support_ref_of(p.offs, p.n_refs, p.capacity, ii);
    if (tid == 0) { sh_ref[0] = r; sh_cnt[0] = 0u; sh_cnt[1] = 0u; }
    if (i == sp.last) sh_ref[1] = r;
    __syncthreads();
    const int r_first = sh_ref[0], r_last = sh_ref[1];
    const LfdSupportGeom g = p.g;
    const long long HW = (long long)g.H * g.W;
    const LfdRefDesc* refs = static_cast<const LfdRefDesc*>(p.refs);
    unsigned n_views = 0u;
    for (int rr = r_first; rr <= r_last; ++rr) {
        if (lfd_support_clamp(p.offs[rr + 1], p.capacity) <= lfd_support_clamp(p.offs[rr], p.capacity)) continue;   // uniform: no points
        int ns = refs[rr].n_slots;
        ns = ns < KMAX ? ns : KMAX;
        lfd_stage_slots(sh, p.slots, p.pair_const, rr, p.k, ns);
        if (tid < ns) sh_img[tid] = p.img[(size_t)rr * p.k + tid];
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
        const unsigned long long mb = __ballot(mine && n_views != 0u);
        unsigned sum = mine ? n_views : 0u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
        if ((tid & 63) == 0) {
            if (mb) atomicAdd(&sh_cnt[0], (unsigned)__popcll(mb));
            if (sum) atomicAdd(&sh_cnt[1], sum);
        }
        __syncthreads();
        if (tid < 2 && sh_cnt[tid]) atomicAdd(p.counters + tid, (unsigned long long)sh_cnt[tid]);    // integer adds: order-free
    }
}

template <int MODE>
static void lfd_colour_launch_k(const LfdColourArgs& p, hipStream_t stream) {
    const dim3 grid((unsigned)p.n_wg);
    if (p.k <= 4) hipLaunchKernelGGL((lfd_colour_kernel<4, MODE>), grid, dim3(256), 0, stream, p);
    else if (p.k <= 8) hipLaunchKernelGGL((lfd_colour_kernel<8, MODE>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((lfd_colour_kernel<LFD_MAX_SLOTS, MODE>), grid, dim3(256), 0, stream, p);
}

// lfd_api.hip's lfd_colour_multiview: the arguments were validated there (capacity <= 2^31 - 1: at most 2^23 workgroups, mode 1 or 2)
hipError_t lfd_colour_launch(const LfdColourArgs& p, hipStream_t stream) {
    if (p.n_wg <= 0) return hipSuccess;
    if (p.mode == LFD_COLOUR_MEAN) lfd_colour_launch_k<LFD_COLOUR_MEAN>(p, stream);
    else lfd_colour_launch_k<LFD_COLOUR_MEDIAN>(p, stream);
    return hipGetLastError();
}
