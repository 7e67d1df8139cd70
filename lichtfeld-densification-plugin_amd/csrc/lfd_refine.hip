// Multi-view re-triangulation of supported points on the device (lfd_refine_multiview): every two-view point that OTHER neighbours
// of its reference confirm is triangulated again from all the views that see it and replaced when the result stands every test.
//
// One launch, a lane per input point, nothing waits for another workgroup and nothing is scanned: the points stay where they are.  The front end
// is the per-point kernels' common one (lfd_device.hpp): coalesced loads of the point's own fields, its reference from ref_offsets (device data), the
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
    const LfdPointStage& st = p.st;
    const LfdPointSpan sp = lfd_point_span(st);
    if (!sp.any) return;                                                // the whole workgroup lies past the last point
    const long long i = sp.i, ii = sp.ii;
    const bool mine = sp.mine;
    const int cell = st.cell[ii];
    const int s = (int)st.slot[ii];
    float X0 = st.xyz[3 * ii], X1 = st.xyz[3 * ii + 1], X2 = st.xyz[3 * ii + 2];
    float err = st.err[ii];
    int r_first, r_last;
    const int r = lfd_ref_range<NC>(sh_ref, sh_cnt, st, sp, r_first, r_last);
    const LfdSupportGeom g = st.g;
    const long long HW = (long long)g.H * g.W;
    const bool cell_ok = cell >= 0 && (long long)cell < HW;            // no address is formed from a cell outside the grid
    unsigned status = 0u;
    for (int rr = r_first; rr <= r_last; ++rr) {
        if (lfd_ref_empty(st, rr)) continue;
        const int ns = lfd_ref_slots<KMAX>(st, rr);
        lfd_stage_slots(sh, st.slots, st.pair_const, rr, st.k, ns);
        if constexpr (WEIGHTED) {
            if (tid < ns) {
                shw[tid].prec = p.prec[(size_t)rr * st.k + tid];
                lfd_slot_prec_scale(sh[tid].sx, sh[tid].sy, shw[tid]);
            }
        }
        if (tid == 64) {
            const LfdRefConst& c = st.ref_const[rr];
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
                wa = make_float2(st.axis_x[x], st.axis_y[y]);
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
        bool hit[NC] = {mine && accepted, mine && !accepted && status != 0u};
        if constexpr (WEIGHTED) hit[2] = mine && (status & LFD_REFINE_WEIGHTED) != 0u;
        lfd_count_tally<NC>(sh_cnt, hit);
        __syncthreads();
        lfd_count_flush<NC>(sh_cnt, p.counters);
    }
}

template <bool WEIGHTED>
static void lfd_refine_launch_k(const LfdRefineArgs& p, hipStream_t stream) {
    const dim3 grid((unsigned)p.st.n_wg);
    if (p.st.k <= 4) hipLaunchKernelGGL((lfd_refine_kernel<4, WEIGHTED>), grid, dim3(256), 0, stream, p);
    else if (p.st.k <= 8) hipLaunchKernelGGL((lfd_refine_kernel<8, WEIGHTED>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((lfd_refine_kernel<LFD_MAX_SLOTS, WEIGHTED>), grid, dim3(256), 0, stream, p);
}

// lfd_api.hip's refine_impl: the arguments were validated there (capacity <= 2^31 - 1: at most 2^23 workgroups); p.prec picks the variant
hipError_t lfd_refine_launch(const LfdRefineArgs& p, hipStream_t stream) {
    if (p.st.n_wg <= 0) return hipSuccess;
    if (p.prec) lfd_refine_launch_k<true>(p, stream);
    else lfd_refine_launch_k<false>(p, stream);
    return hipGetLastError();
}
