// Multi-view re-triangulation of supported points on the device (lfd_refine_multiview): every two-view point that OTHER neighbours
// of its reference confirm is triangulated again from all the views that see it and replaced when the result stands every test.
//
// One launch, a lane per input point, nothing waits for another workgroup and nothing is scanned: the points stay where they are.  The front end
// is lfd_support_count_kernel's (lfd_support.hip): coalesced loads of the point's own fields, its reference from ref_offsets (device data), the
// reference's constants staged in LDS (a workgroup whose points straddle references takes them one after the other), all gathers of a point -
// the winner's warp, the reference's observation, certainty (4 B) and warp pair (8 B) of every other neighbour - issued before any arithmetic.
// The f64 accumulation and the solve (lfd_refine.hpp) run only in lanes that have a candidate.
//
// lfd_refine_kernel<KMAX, WEIGHTED> is both calls' kernel.  WEIGHTED (lfd_refine_multiview_weighted, DESIGN 4.10, LfdRefineArgs::prec set) adds
// the plane pointer and the pixel-scale reciprocals of every slot in LDS, one 12-byte precision gather per view beside its certainty and warp
// loads - issued for every other slot before it is known which are candidates (the price of having all loads in flight together) - and the
// third counter; without it none of that is compiled.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_device.hpp"
#include "lfd_refine.hpp"

template <int KMAX, bool WEIGHTED>
__global__ void __launch_bounds__(256) lfd_refine_kernel(const LfdRefineArgs p) {
    constexpr int NC = WEIGHTED ? 3 : 2;                               // counters: the caller of the unweighted call hands two elements
    __shared__ LfdSlot sh[KMAX];
    __shared__ LfdSlotPrec shw[WEIGHTED ? KMAX : 1];                   // (referenced, hence allocated, only when WEIGHTED)
    __shared__ LfdRefineRef sh_rc;
    __shared__ int sh_ref[2];
    __shared__ unsigned sh_cnt[NC];
    const int tid = (int)threadIdx.x;
    const LfdPointSpan sp = lfd_point_span(p.offs, p.n_refs, p.capacity);
    if (!sp.any) return;                                                // the whole workgroup lies past the last point
    const long long i = sp.i, ii = sp.ii;
    const bool mine = sp.mine;
    const int cell = p.cell[ii];
    const int s = (int)p.slot[ii];
    float X0 = p.xyz[3 * ii], X1 = p.xyz[3 * ii + 1], X2 = p.xyz[3 * ii + 2];
    float err = p.err[ii];
    const int r = lfd_support_ref_of(p.offs, p.n_refs, p.capacity, ii);
    if (tid == 0) {
        sh_ref[0] = r;
#pragma unroll
        for (int e = 0; e < NC; ++e) sh_cnt[e] = 0u;
    }
    if (i == sp.last) sh_ref[1] = r;
    __syncthreads();
    const int r_first = sh_ref[0], r_last = sh_ref[1];
    const LfdSupportGeom g = p.g;
    const long long HW = (long long)g.H * g.W;
    const bool cell_ok = cell >= 0 && (long long)cell < HW;            // no address is formed from a cell outside the grid
    const LfdRefDesc* refs = static_cast<const LfdRefDesc*>(p.refs);
    unsigned status = 0u;
    for (int rr = r_first; rr <= r_last; ++rr) {
        if (lfd_support_clamp(p.offs[rr + 1], p.capacity) <= lfd_support_clamp(p.offs[rr], p.capacity)) continue;   // uniform: no points
        int ns = refs[rr].n_slots;
        ns = ns < KMAX ? ns : KMAX;
        lfd_stage_slots(sh, p.slots, p.pair_const, rr, p.k, ns);
        if constexpr (WEIGHTED) {
            if (tid < ns) {
                shw[tid].prec = p.prec[(size_t)rr * p.k + tid];
                lfd_slot_prec_scale(sh[tid].sx, sh[tid].sy, shw[tid]);
            }
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
            float q00[WEIGHTED ? KMAX : 1], q01[WEIGHTED ? KMAX : 1], q11[WEIGHTED ? KMAX : 1], qs[3];
            const float* wp = sh[s].warp + (size_t)cell * g.C;
            const float2 wb = *reinterpret_cast<const float2*>(wp + (g.C - 2));
            float2 wa;
            if (g.C == 4) wa = *reinterpret_cast<const float2*>(wp);
            else {
                const int y = cell / g.W, x = cell - y * g.W;
                wa = make_float2(p.axis_x[x], p.axis_y[y]);
            }
            if constexpr (WEIGHTED) {
                const float* qp = shw[s].prec + (size_t)cell * 3;
                qs[0] = qp[0]; qs[1] = qp[1]; qs[2] = qp[2];
            }
#pragma unroll
            for (int j = 0; j < KMAX; ++j) {
                c[j] = 0.0f; wx[j] = 0.0f; wy[j] = 0.0f;
                if constexpr (WEIGHTED) { q00[j] = 0.0f; q01[j] = 0.0f; q11[j] = 0.0f; }
                if (j < ns && j != s) {
                    c[j] = sh[j].cert[cell];
                    const float2 w = *reinterpret_cast<const float2*>(sh[j].warp + (size_t)cell * g.C + (g.C - 2));
                    wx[j] = w.x; wy[j] = w.y;
                    if constexpr (WEIGHTED) {
                        const float* qp = shw[j].prec + (size_t)cell * 3;
                        q00[j] = qp[0]; q01[j] = qp[1]; q11[j] = qp[2];
                    }
                }
            }
            const LfdRefineGather o = {c, wx, wy, q00, q01, q11, qs};
            const LfdSlotPrec* ws = nullptr;
            if constexpr (WEIGHTED) ws = shw;
            status = lfd_refine_point<KMAX, WEIGHTED>(sh_rc, sh, ws, ns, s, g, wa.x, wa.y, wb.x, wb.y, o, X0, X1, X2, err);
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
                                 mw = WEIGHTED ? __ballot(mine && (status & LFD_REFINE_WEIGHTED) != 0u) : 0ull;
        if ((tid & 63) == 0) {
            if (ma) atomicAdd(&sh_cnt[0], (unsigned)__popcll(ma));
            if (mf) atomicAdd(&sh_cnt[1], (unsigned)__popcll(mf));
            if constexpr (WEIGHTED) {
                if (mw) atomicAdd(&sh_cnt[2], (unsigned)__popcll(mw));
            }
        }
        __syncthreads();
        if (tid < NC && sh_cnt[tid]) atomicAdd(p.counters + tid, (unsigned long long)sh_cnt[tid]);    // integer adds: order-free
    }
}

template <bool WEIGHTED>
static void lfd_refine_launch_k(const LfdRefineArgs& p, hipStream_t stream) {
    const dim3 grid((unsigned)p.n_wg);
    if (p.k <= 4) hipLaunchKernelGGL((lfd_refine_kernel<4, WEIGHTED>), grid, dim3(256), 0, stream, p);
    else if (p.k <= 8) hipLaunchKernelGGL((lfd_refine_kernel<8, WEIGHTED>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((lfd_refine_kernel<LFD_MAX_SLOTS, WEIGHTED>), grid, dim3(256), 0, stream, p);
}

// lfd_api.hip's refine_impl: the arguments were validated there (capacity <= 2^31 - 1: at most 2^23 workgroups); p.prec picks the variant
hipError_t lfd_refine_launch(const LfdRefineArgs& p, hipStream_t stream) {
    if (p.n_wg <= 0) return hipSuccess;
    if (p.prec) lfd_refine_launch_k<true>(p, stream);
    else lfd_refine_launch_k<false>(p, stream);
    return hipGetLastError();
}
