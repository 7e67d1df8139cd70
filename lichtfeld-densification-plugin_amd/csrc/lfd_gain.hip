// Per-image exposure gains on the device (lfd_gain_accumulate / lfd_gain_apply).
//
// lfd_gain_kernel: one launch, a lane per input point, with the per-point kernels' common front end (lfd_device.hpp): coalesced loads of the
// point's own fields, its reference from ref_offsets (device data), the reference's neighbours and their image bases staged in LDS (a
// workgroup whose points straddle references takes them one after the other).  What a lane has per slot is a flag and six integers below
// 2^24; what the table wants is their sum.  The reduction, per (reference, slot):
//   wave        a ballot gives N; each of the six values is summed over the 64 lanes in 32 bits (64 values below 2^24 stay below 2^30),
//               six xor steps each; a wave in which no lane has a sample for the slot skips them (a wave-uniform branch)
//   workgroup   lane 0 of each wave adds the wave's seven sums to u32 accumulators in LDS (four waves: below 2^32), one LDS atomic each
//   global      behind a barrier, lane t < ns * 7 adds accumulator t to the table with ONE 64-bit atomic add - if it is not zero
// so a workgroup issues at most one global atomic per (reference, slot, quantity), a row with nothing to add issues none, and nothing a
// point contributes reaches global memory on its own.  Integer additions only: the table does not depend on the launch geometry.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_device.hpp"
#include "lfd_gain.hpp"

// (amdgpu_waves_per_eu(4): at most 128 VGPRs, as lfd_colour_kernel; DESIGN 4.23 has the table.)
template <int KMAX, int C>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) lfd_gain_kernel(const LfdGainArgs p) {
    __shared__ LfdSlot sh[KMAX];
    __shared__ const uint8_t* sh_img[KMAX];
    __shared__ int sh_ref[2];
    __shared__ unsigned sh_acc[KMAX * LFD_GAIN_QUANTITIES];
    const int tid = (int)threadIdx.x;
    const LfdPointStage& st = p.st;
    const LfdPointSpan sp = lfd_point_span(st);
    if (!sp.any) return;                                                // the whole workgroup lies past the last point
    const long long ii = sp.ii;
    const bool mine = sp.mine;
    const int cell = st.cell[ii];
    const int s = (int)st.slot[ii];
    const float X0 = st.xyz[3 * ii], X1 = st.xyz[3 * ii + 1], X2 = st.xyz[3 * ii + 2];
    const float rgb[3] = {st.rgb[3 * ii], st.rgb[3 * ii + 1], st.rgb[3 * ii + 2]};
    int r_first, r_last;
    const int r = lfd_ref_range<0>(sh_ref, nullptr, st, sp, r_first, r_last);
    const LfdSupportGeom g = st.g;
    const long long HW = (long long)g.H * g.W;
    const bool ref_ok = lfd_gain_in_range(rgb[0]) && lfd_gain_in_range(rgb[1]) && lfd_gain_in_range(rgb[2]);
    // (a value out of range - NaN included - never reaches the conversion)
    const unsigned qr0 = ref_ok ? lfd_gain_quantise(rgb[0]) : 0u, qr1 = ref_ok ? lfd_gain_quantise(rgb[1]) : 0u,
                   qr2 = ref_ok ? lfd_gain_quantise(rgb[2]) : 0u;
    for (int rr = r_first; rr <= r_last; ++rr) {
        if (lfd_ref_empty(st, rr)) continue;
        const int ns = lfd_ref_slots<KMAX>(st, rr);
        lfd_stage_slots(sh, st.slots, st.pair_const, rr, st.k, ns);
        if (tid < ns) sh_img[tid] = p.img[(size_t)rr * st.k + tid];
        if (tid < KMAX * LFD_GAIN_QUANTITIES) sh_acc[tid] = 0u;
        __syncthreads();
        const bool active = mine && r == rr && !lfd_colour_guarded(X0, X1, X2, rgb[0], rgb[1], rgb[2], cell, HW, s, ns);
        // all gathers of the point first, then the arithmetic
        float c[KMAX], wx[KMAX], wy[KMAX];
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            c[j] = 0.0f; wx[j] = 0.0f; wy[j] = 0.0f;
            if (active && j < ns) {
                c[j] = sh[j].cert[cell];
                const float2 w = *reinterpret_cast<const float2*>(sh[j].warp + (size_t)cell * C + (C - 2));
                wx[j] = w.x; wy[j] = w.y;
            }
        }
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            if (j < ns) {                                              // (uniform)
                unsigned q[3] = {0u, 0u, 0u};
                bool counts = false;
                if (active) counts = lfd_gain_sample(sh[j], sh_img[j], g, j == s, ref_ok, c[j], wx[j], wy[j], X0, X1, X2, q);
                const unsigned long long mb = __ballot(counts);
                if (mb) {                                              // (uniform within the wave)
                    unsigned v[6] = {counts ? qr0 : 0u, counts ? qr1 : 0u, counts ? qr2 : 0u, counts ? q[0] : 0u, counts ? q[1] : 0u,
                                     counts ? q[2] : 0u};
#pragma unroll
                    for (int e = 0; e < 6; ++e) {
#pragma unroll
                        for (int off = 32; off > 0; off >>= 1) v[e] += __shfl_xor(v[e], off, 64);
                    }
                    if ((tid & 63) == 0) {
                        unsigned* acc = sh_acc + j * LFD_GAIN_QUANTITIES;
                        atomicAdd(acc, (unsigned)__popcll(mb));
#pragma unroll
                        for (int e = 0; e < 6; ++e) atomicAdd(acc + 1 + e, v[e]);
                    }
                }
            }
        }
        __syncthreads();
        if (tid < ns * LFD_GAIN_QUANTITIES) {
            const unsigned a = sh_acc[tid];                            // row rr * k + tid / 7, quantity tid % 7: consecutive in the table
            if (a) atomicAdd(p.table + (size_t)rr * st.k * LFD_GAIN_QUANTITIES + tid, (unsigned long long)a);
        }
        __syncthreads();                                               // the next reference's constants replace these
    }
}

// A workgroup per 256 points, a lane per colour VALUE (three passes of 256 coalesced 4-byte accesses, 32-bit index arithmetic).  The reference
// of the workgroup's first point is found with uniform (scalar) loads; a workgroup that lies inside one reference - all but n_refs - 1 of
// them - searches nothing else, the others search per value.
__global__ void __launch_bounds__(256) lfd_gain_apply_kernel(const LfdGainApplyArgs p) {
    const long long total = lfd_support_clamp(p.offs[p.n_refs], p.n);
    const long long base = (long long)blockIdx.x * 256;
    if (base >= total) return;                                          // (uniform)
    const long long last = (base + 256 < total ? base + 256 : total) - 1;
    const int r0 = lfd_support_ref_of(p.offs, p.n_refs, p.n, base);
    const bool one = last < lfd_support_clamp(p.offs[r0 + 1], p.n);
    const int n_val = (int)(last - base + 1) * 3;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int v = (int)threadIdx.x + 256 * t;
        if (v < n_val) {
            const int pt = v / 3, ch = v - 3 * pt;
            const int r = one ? r0 : lfd_support_ref_of(p.offs, p.n_refs, p.n, base + pt);
            const long long e = 3 * base + v;
            p.o_rgb[e] = lfd_gain_value(p.rgb[e], p.factors[3 * r + ch]);       // (in place: a value is read and written by one lane)
        }
    }
}

// (C: the warp's channels, 2 or 4 - a compile-time stride for the observation's address)
template <int C>
static void lfd_gain_launch_c(const LfdGainArgs& p, dim3 grid, hipStream_t stream) {
    if (p.st.k <= 4) hipLaunchKernelGGL((lfd_gain_kernel<4, C>), grid, dim3(256), 0, stream, p);
    else if (p.st.k <= 8) hipLaunchKernelGGL((lfd_gain_kernel<8, C>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((lfd_gain_kernel<LFD_MAX_SLOTS, C>), grid, dim3(256), 0, stream, p);
}

// lfd_api.hip's lfd_gain_accumulate: the arguments were validated there (capacity <= 2^31 - 1: at most 2^23 workgroups; warp_channels 2 or 4)
hipError_t lfd_gain_launch(const LfdGainArgs& p, hipStream_t stream) {
    if (p.st.n_wg <= 0) return hipSuccess;
    const dim3 grid((unsigned)p.st.n_wg);
    if (p.st.g.C == 2) lfd_gain_launch_c<2>(p, grid, stream);
    else lfd_gain_launch_c<4>(p, grid, stream);
    return hipGetLastError();
}

// ... lfd_gain_apply (n <= 2^31 - 1: at most 2^23 workgroups)
hipError_t lfd_gain_apply_launch(const LfdGainApplyArgs& p, hipStream_t stream) {
    if (p.n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((p.n + 255) / 256));
    hipLaunchKernelGGL(lfd_gain_apply_kernel, grid, dim3(256), 0, stream, p);
    return hipGetLastError();
}
