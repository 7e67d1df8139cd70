// Forward-backward consistency gate on the device (lfd_cycle_gate): every cell of up to LFD_MAX_SLOTS (reference, neighbour)
// pairs is followed to the neighbour with warp_AB and back with warp_BA; its floored certainty is kept iff it lands within the threshold.
//
// Memory-bound: 24 bytes per cell and pair (certainty 4, warp_AB 8, the warp_BA plane 8 once, store 4), no LDS, nothing crosses a
// workgroup except the optional counter (integer adds: the total does not depend on their order).  Equal inputs give equal bits.
//
//   lfd_cycle_vec_kernel<C>   W % 4 == 0 and aligned planes: a lane owns four consecutive cells of one row - 16-byte loads of certainty and
//                             warp_AB, 8-byte gathers of the sixteen warp_BA texels, a 16-byte store.
//   lfd_cycle_any_kernel      any width and alignment: a lane per cell through lfd_cycle_cell, the twin's own routine.
//
// The pairs lie on blockIdx.y: the k planes of a reference are one launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_cycle.hpp"

// Workgroups are handed to the 8 XCDs (each with an L2 of its own) round-robin over the linear workgroup id, blockIdx.x fastest.  gridDim.x is
// a multiple of 8 (lfd_cycle_launch pads it), so blockIdx.x % 8 names the XCD for every pair alike, and each XCD is given one contiguous run
// of the cells - a band of rows, whose image under a smooth warp_AB is a band of warp_BA that stays in that XCD's L2 - instead of every
// eighth workgroup of the whole grid.  Bijective; a choice of speed alone.
__device__ __forceinline__ unsigned lfd_cycle_block() {
    const unsigned per = gridDim.x / 8u;
    return (blockIdx.x % 8u) * per + blockIdx.x / 8u;
}

// one vector atomic per wave that rejected anything
__device__ __forceinline__ void lfd_cycle_count(int32_t* counter, unsigned n_rejected_in_wave) {
    if (counter && n_rejected_in_wave && (threadIdx.x & (warpSize - 1)) == 0) atomicAdd(counter, (int)n_rejected_in_wave);
}

template <int C>
__global__ void __launch_bounds__(256) lfd_cycle_vec_kernel(const LfdCycleArgs p) {
    const int pair = (int)blockIdx.y;
    const long long quads = ((long long)p.H * p.W) >> 2;
    const long long q = (long long)lfd_cycle_block() * 256 + threadIdx.x;
    const bool active = q < quads;
    const long long qq = active ? q : 0;                               // idle lanes compute on quad 0 and store nothing
    const int cell0 = (int)(qq << 2);
    const int y = cell0 / p.W, x0 = cell0 - y * p.W;                   // W % 4 == 0: the four cells share the row

    const float4 c4 = reinterpret_cast<const float4*>(p.cert[pair])[qq];
    const float4* wab = reinterpret_cast<const float4*>(p.warp_ab[pair]) + qq * C;
    float xa[4], ya[4], xb[4], yb[4];
    if (C == 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float4 w = wab[e]; xa[e] = w.x; ya[e] = w.y; xb[e] = w.z; yb[e] = w.w; }
    } else {
        const float4 w0 = wab[0], w1 = wab[1];
        xb[0] = w0.x; yb[0] = w0.y; xb[1] = w0.z; yb[1] = w0.w; xb[2] = w1.x; yb[2] = w1.y; xb[3] = w1.z; yb[3] = w1.w;
        const float yv = p.axis_y ? p.axis_y[y] : lfd_axis_value(p.ay, y);
#pragma unroll
        for (int e = 0; e < 4; ++e) { xa[e] = p.axis_x ? p.axis_x[x0 + e] : lfd_axis_value(p.ax, x0 + e); ya[e] = yv; }
    }

    // the sixteen gathers first, then the arithmetic: all of them are in flight together
    const float2* wba = reinterpret_cast<const float2*>(p.warp_ba[pair]);
    LfdCycleTaps t[4];
    bool inside[4];
    float2 v[4][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        inside[e] = lfd_cycle_taps(xb[e], yb[e], p.Wb, p.Hb, t[e]);
        v[e][0] = wba[t[e].i00]; v[e][1] = wba[t[e].i01]; v[e][2] = wba[t[e].i10]; v[e][3] = wba[t[e].i11];
    }
    const float cin[4] = {c4.x, c4.y, c4.z, c4.w};
    float co[4], eo[4];
    unsigned rejected = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float d2;
        const bool keep = lfd_cycle_decide(t[e], inside[e], v[e][0].x, v[e][0].y, v[e][1].x, v[e][1].y, v[e][2].x, v[e][2].y, v[e][3].x, v[e][3].y,
                                           xa[e], ya[e], p.wm1, p.hm1, p.tau2, d2);
        co[e] = keep ? lfd_cert_floor(cin[e], p.certainty_thresh) : 0.0f;
        eo[e] = sqrtf(d2);
        rejected += (unsigned)__popcll(__ballot(active && !keep));
    }
    if (active) {
        reinterpret_cast<float4*>(p.cert_out[pair])[qq] = make_float4(co[0], co[1], co[2], co[3]);
        if (p.err_out[pair]) reinterpret_cast<float4*>(p.err_out[pair])[qq] = make_float4(eo[0], eo[1], eo[2], eo[3]);
    }
    lfd_cycle_count(p.rejected ? p.rejected + pair : nullptr, rejected);
}

__global__ void __launch_bounds__(256) lfd_cycle_any_kernel(const LfdCycleArgs p) {
    const int pair = (int)blockIdx.y;
    const long long cells = (long long)p.H * p.W;
    const long long i = (long long)lfd_cycle_block() * 256 + threadIdx.x;
    const bool active = i < cells;
    const int cell = active ? (int)i : 0;
    const int y = cell / p.W, x = cell - y * p.W;
    const float* wp = p.warp_ab[pair] + (size_t)cell * p.C;
    float xa, ya, xb, yb;
    if (p.C == 4) { xa = wp[0]; ya = wp[1]; xb = wp[2]; yb = wp[3]; }
    else {
        xb = wp[0]; yb = wp[1];
        xa = p.axis_x ? p.axis_x[x] : lfd_axis_value(p.ax, x);
        ya = p.axis_y ? p.axis_y[y] : lfd_axis_value(p.ay, y);
    }
    float d2;
    const bool keep = lfd_cycle_cell(p.warp_ba[pair], p.Wb, p.Hb, xa, ya, xb, yb, p.wm1, p.hm1, p.tau2, d2);
    const float c = keep ? lfd_cert_floor(p.cert[pair][cell], p.certainty_thresh) : 0.0f;
    const unsigned rejected = (unsigned)__popcll(__ballot(active && !keep));
    if (active) {
        p.cert_out[pair][cell] = c;
        if (p.err_out[pair]) p.err_out[pair][cell] = sqrtf(d2);
    }
    lfd_cycle_count(p.rejected ? p.rejected + pair : nullptr, rejected);
}

// the vector kernel's layout: rows of whole quads, 16-byte aligned certainty / warp_AB / output planes, 8-byte aligned warp_BA
static bool lfd_cycle_vector_layout(const LfdCycleArgs& p) {
    if (p.W & 3) return false;
    uintptr_t m16 = 0, m8 = 0;
    for (int i = 0; i < p.n_pairs; ++i) {
        m16 |= reinterpret_cast<uintptr_t>(p.cert[i]) | reinterpret_cast<uintptr_t>(p.warp_ab[i]) | reinterpret_cast<uintptr_t>(p.cert_out[i]) |
               reinterpret_cast<uintptr_t>(p.err_out[i]);
        m8 |= reinterpret_cast<uintptr_t>(p.warp_ba[i]);
    }
    return (m16 & 15u) == 0 && (m8 & 7u) == 0;
}

// lfd_api.hip's lfd_cycle_gate: the arguments were validated there (H, W <= 32768: at most 2^30 cells, 2^22 workgroups)
hipError_t lfd_cycle_launch(const LfdCycleArgs& p, hipStream_t stream) {
    const long long cells = (long long)p.H * p.W;
    const bool vec = lfd_cycle_vector_layout(p);
    const long long items = vec ? cells >> 2 : cells;
    const unsigned wgs = (unsigned)((items + 255) / 256);
    const dim3 grid((wgs + 7u) & ~7u, (unsigned)p.n_pairs);
    if (!vec) hipLaunchKernelGGL(lfd_cycle_any_kernel, grid, dim3(256), 0, stream, p);
    else if (p.C == 4) hipLaunchKernelGGL(lfd_cycle_vec_kernel<4>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(lfd_cycle_vec_kernel<2>, grid, dim3(256), 0, stream, p);
    return hipGetLastError();
}
