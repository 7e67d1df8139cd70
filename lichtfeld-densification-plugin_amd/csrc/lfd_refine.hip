// Multi-view re-triangulation of supported points on the device (lfd_refine_multiview): every two-view point that OTHER neighbours
// of its reference confirm is triangulated again from all the views that see it and replaced when the result stands every test.
//
// One launch, a lane per input point, nothing waits for another workgroup and nothing is scanned: the points stay where they are.  The front end
// is lfd_support_count_kernel's (lfd_support.hip): coalesced loads of the point's own fields, its reference from ref_offsets (device data), the
// reference's constants staged in LDS (a workgroup whose points straddle references takes them one after the other), all gathers of a point -
// the winner's warp, the reference's observation, certainty (4 B) and warp pair (8 B) of every other neighbour - issued before any arithmetic.
// The f64 accumulation and the solve (lfd_refine.hpp) run only in lanes that have a candidate.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_device.hpp"
#include "lfd_refine.hpp"

template <int KMAX>
__global__ void __launch_bounds__(256) lfd_refine_kernel(const LfdRefineArgs p) {
    __shared__ LfdRefineSlot sh[KMAX];
    __shared__ LfdRefineRef sh_rc;
    __shared__ int sh_ref[2];
    __shared__ unsigned sh_cnt[2];
    const int tid = (int)threadIdx.x;
    const long long total = lfd_support_clamp(p.offs[p.n_refs], p.capacity);
    const long long base = (long long)blockIdx.x * 256;
    if (base >= total) return;                                         // the whole workgroup lies past the last point
    const long long i = base + tid;
    const bool mine = i < total;
    const long long last = (base + 256 < total ? base + 256 : total) - 1;
    const long long ii = mine ? i : last;                              // idle lanes read the last point and store nothing
    const int cell = p.cell[ii];
    const int s = (int)p.slot[ii];
    float X0 = p.xyz[3 * ii], X1 = p.xyz[3 * ii + 1], X2 = p.xyz[3 * ii + 2];
    float err = p.err[ii];
    const int r = lfd_support_ref_of(p.offs, p.n_refs, p.capacity, ii);
    if (tid == 0) { sh_ref[0] = r; sh_cnt[0] = 0u; sh_cnt[1] = 0u; }
    if (i == last) sh_ref[1] = r;
    __syncthreads();
    const int r_first = sh_ref[0], r_last = sh_ref[1];
    const LfdRefineGeom g = p.g;
    const long long HW = (long long)g.H * g.W;
    const bool cell_ok = cell >= 0 && (long long)cell < HW;            // no address is formed from a cell outside the grid
    const LfdRefDesc* refs = static_cast<const LfdRefDesc*>(p.refs);
    const LfdSlotDesc* slots = static_cast<const LfdSlotDesc*>(p.slots);
    unsigned status = 0u;
    for (int rr = r_first; rr <= r_last; ++rr) {
        if (lfd_support_clamp(p.offs[rr + 1], p.capacity) <= lfd_support_clamp(p.offs[rr], p.capacity)) continue;   // uniform: no points
        int ns = refs[rr].n_slots;
        ns = ns < KMAX ? ns : KMAX;
        if (tid < ns) {
            const LfdSlotDesc& d = slots[(size_t)rr * p.k + tid];
            const LfdPairConst& c = p.pair_const[(size_t)rr * p.k + tid];
            LfdRefineSlot& o = sh[tid];
            o.cert = d.cert; o.warp = d.warp; o.mask_b = d.mask_b;
#pragma unroll
            for (int e = 0; e < 12; ++e) o.P[e] = c.P[e];
            o.sx = c.sx; o.sy = c.sy;
        }
        if (tid == 64) {
            const LfdRefConst& c = p.ref_const[rr];
#pragma unroll
            for (int e = 0; e < 12; ++e) sh_rc.P[e] = c.P[e];
            sh_rc.sx = c.sx; sh_rc.sy = c.sy;
        }
        __syncthreads();
        if (mine && r == rr && cell_ok && s < ns) {
            // all gathers of the point first, then the arithmetic
            float c[KMAX], wx[KMAX], wy[KMAX];
            const float* wp = sh[s].warp + (size_t)cell * g.C;
            const float2 wb = *reinterpret_cast<const float2*>(wp + (g.C - 2));
            float2 wa;
            if (g.C == 4) wa = *reinterpret_cast<const float2*>(wp);
            else {
                const int y = cell / g.W, x = cell - y * g.W;
                wa = make_float2(p.axis_x[x], p.axis_y[y]);
            }
#pragma unroll
            for (int j = 0; j < KMAX; ++j) {
                c[j] = 0.0f; wx[j] = 0.0f; wy[j] = 0.0f;
                if (j < ns && j != s) {
                    c[j] = sh[j].cert[cell];
                    const float2 w = *reinterpret_cast<const float2*>(sh[j].warp + (size_t)cell * g.C + (g.C - 2));
                    wx[j] = w.x; wy[j] = w.y;
                }
            }
            status = lfd_refine_point<KMAX>(sh_rc, sh, ns, s, g, wa.x, wa.y, wb.x, wb.y, c, wx, wy, X0, X1, X2, err);
        }
        __syncthreads();                                               // the next reference's constants replace these
    }
    if (mine) {
        p.o_xyz[3 * i] = X0; p.o_xyz[3 * i + 1] = X1; p.o_xyz[3 * i + 2] = X2;
        p.o_err[i] = err;
        if (p.status) p.status[i] = (uint8_t)status;
    }
    if (p.counters) {                                                  // (uniform)
        const bool accepted = (status & LFD_REFINE_ACCEPTED) != 0u;
        const unsigned long long ma = __ballot(mine && accepted), mf = __ballot(mine && !accepted && status != 0u);
        if ((tid & 63) == 0) {
            if (ma) atomicAdd(&sh_cnt[0], (unsigned)__popcll(ma));
            if (mf) atomicAdd(&sh_cnt[1], (unsigned)__popcll(mf));
        }
        __syncthreads();
        if (tid < 2 && sh_cnt[tid]) atomicAdd(p.counters + tid, (unsigned long long)sh_cnt[tid]);     // integer adds: order-free
    }
}

// Precision-weighted variant (lfd_refine_multiview_weighted): lfd_refine_kernel's front end, plus the plane pointer and the
// pixel-scale reciprocals of every slot in LDS and one 12-byte precision gather per view beside its certainty and warp loads - issued for every
// other slot before it is known which are candidates (the price of having all loads in flight together).
template <int KMAX>
__global__ void __launch_bounds__(256) lfd_refine_weighted_kernel(const LfdRefineWArgs pw) {
    __shared__ LfdRefineSlot sh[KMAX];
    __shared__ LfdRefineWSlot shw[KMAX];
    __shared__ LfdRefineRef sh_rc;
    __shared__ int sh_ref[2];
    __shared__ unsigned sh_cnt[3];
    const LfdRefineArgs& p = pw.a;
    const int tid = (int)threadIdx.x;
    const long long total = lfd_support_clamp(p.offs[p.n_refs], p.capacity);
    const long long base = (long long)blockIdx.x * 256;
    if (base >= total) return;                                         // the whole workgroup lies past the last point
    const long long i = base + tid;
    const bool mine = i < total;
    const long long last = (base + 256 < total ? base + 256 : total) - 1;
    const long long ii = mine ? i : last;                              // idle lanes read the last point and store nothing
    const int cell = p.cell[ii];
    const int s = (int)p.slot[ii];
    float X0 = p.xyz[3 * ii], X1 = p.xyz[3 * ii + 1], X2 = p.xyz[3 * ii + 2];
    float err = p.err[ii];
    const int r = lfd_support_ref_of(p.offs, p.n_refs, p.capacity, ii);
    if (tid == 0) { sh_ref[0] = r; sh_cnt[0] = 0u; sh_cnt[1] = 0u; sh_cnt[2] = 0u; }
    if (i == last) sh_ref[1] = r;
    __syncthreads();
    const int r_first = sh_ref[0], r_last = sh_ref[1];
    const LfdRefineGeom g = p.g;
    const long long HW = (long long)g.H * g.W;
    const bool cell_ok = cell >= 0 && (long long)cell < HW;            // no address is formed from a cell outside the grid
    const LfdRefDesc* refs = static_cast<const LfdRefDesc*>(p.refs);
    const LfdSlotDesc* slots = static_cast<const LfdSlotDesc*>(p.slots);
    unsigned status = 0u;
    for (int rr = r_first; rr <= r_last; ++rr) {
        if (lfd_support_clamp(p.offs[rr + 1], p.capacity) <= lfd_support_clamp(p.offs[rr], p.capacity)) continue;   // uniform: no points
        int ns = refs[rr].n_slots;
        ns = ns < KMAX ? ns : KMAX;
        if (tid < ns) {
            const LfdSlotDesc& d = slots[(size_t)rr * p.k + tid];
            const LfdPairConst& c = p.pair_const[(size_t)rr * p.k + tid];
            LfdRefineSlot& o = sh[tid];
            o.cert = d.cert; o.warp = d.warp; o.mask_b = d.mask_b;
#pragma unroll
            for (int e = 0; e < 12; ++e) o.P[e] = c.P[e];
            o.sx = c.sx; o.sy = c.sy;
            shw[tid].prec = pw.prec[(size_t)rr * p.k + tid];
            lfd_refine_wslot_scale(c.sx, c.sy, shw[tid]);
        }
        if (tid == 64) {
            const LfdRefConst& c = p.ref_const[rr];
#pragma unroll
            for (int e = 0; e < 12; ++e) sh_rc.P[e] = c.P[e];
            sh_rc.sx = c.sx; sh_rc.sy = c.sy;
        }
        __syncthreads();
        if (mine && r == rr && cell_ok && s < ns) {
            // all gathers of the point first, then the arithmetic
            float c[KMAX], wx[KMAX], wy[KMAX], q00[KMAX], q01[KMAX], q11[KMAX], qs[3];
            const float* wp = sh[s].warp + (size_t)cell * g.C;
            const float2 wb = *reinterpret_cast<const float2*>(wp + (g.C - 2));
            float2 wa;
            if (g.C == 4) wa = *reinterpret_cast<const float2*>(wp);
            else {
                const int y = cell / g.W, x = cell - y * g.W;
                wa = make_float2(p.axis_x[x], p.axis_y[y]);
            }
            {
                const float* qp = shw[s].prec + (size_t)cell * 3;
                qs[0] = qp[0]; qs[1] = qp[1]; qs[2] = qp[2];
            }
#pragma unroll
            for (int j = 0; j < KMAX; ++j) {
                c[j] = 0.0f; wx[j] = 0.0f; wy[j] = 0.0f; q00[j] = 0.0f; q01[j] = 0.0f; q11[j] = 0.0f;
                if (j < ns && j != s) {
                    c[j] = sh[j].cert[cell];
                    const float2 w = *reinterpret_cast<const float2*>(sh[j].warp + (size_t)cell * g.C + (g.C - 2));
                    wx[j] = w.x; wy[j] = w.y;
                    const float* qp = shw[j].prec + (size_t)cell * 3;
                    q00[j] = qp[0]; q01[j] = qp[1]; q11[j] = qp[2];
                }
            }
            status = lfd_refine_point_weighted<KMAX>(sh_rc, sh, shw, ns, s, g, wa.x, wa.y, wb.x, wb.y, c, wx, wy, q00, q01, q11, qs, X0, X1, X2,
                                                     err);
        }
        __syncthreads();                                               // the next reference's constants replace these
    }
    if (mine) {
        p.o_xyz[3 * i] = X0; p.o_xyz[3 * i + 1] = X1; p.o_xyz[3 * i + 2] = X2;
        p.o_err[i] = err;
        if (p.status) p.status[i] = (uint8_t)status;
    }
    if (p.counters) {                                                  // (uniform)
        const bool accepted = (status & LFD_REFINE_ACCEPTED) != 0u;
        const unsigned long long ma = __ballot(mine && accepted), mf = __ballot(mine && !accepted && status != 0u),
                                 mw = __ballot(mine && (status & LFD_REFINE_WEIGHTED) != 0u);
        if ((tid & 63) == 0) {
            if (ma) atomicAdd(&sh_cnt[0], (unsigned)__popcll(ma));
            if (mf) atomicAdd(&sh_cnt[1], (unsigned)__popcll(mf));
            if (mw) atomicAdd(&sh_cnt[2], (unsigned)__popcll(mw));
        }
        __syncthreads();
        if (tid < 3 && sh_cnt[tid]) atomicAdd(p.counters + tid, (unsigned long long)sh_cnt[tid]);     // integer adds: order-free
    }
}

// lfd_api.hip's lfd_refine_multiview: the arguments were validated there (capacity <= 2^31 - 1: at most 2^23 workgroups)
hipError_t lfd_refine_launch(const LfdRefineArgs& p, hipStream_t stream) {
    if (p.n_wg <= 0) return hipSuccess;
    const dim3 grid((unsigned)p.n_wg);
    if (p.k <= 4) hipLaunchKernelGGL(lfd_refine_kernel<4>, grid, dim3(256), 0, stream, p);
    else if (p.k <= 8) hipLaunchKernelGGL(lfd_refine_kernel<8>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(lfd_refine_kernel<LFD_MAX_SLOTS>, grid, dim3(256), 0, stream, p);
    return hipGetLastError();
}

// lfd_api.hip's lfd_refine_multiview_weighted (validated there)
hipError_t lfd_refine_weighted_launch(const LfdRefineWArgs& p, hipStream_t stream) {
    if (p.a.n_wg <= 0) return hipSuccess;
    const dim3 grid((unsigned)p.a.n_wg);
    if (p.a.k <= 4) hipLaunchKernelGGL(lfd_refine_weighted_kernel<4>, grid, dim3(256), 0, stream, p);
    else if (p.a.k <= 8) hipLaunchKernelGGL(lfd_refine_weighted_kernel<8>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(lfd_refine_weighted_kernel<LFD_MAX_SLOTS>, grid, dim3(256), 0, stream, p);
    return hipGetLastError();
}
