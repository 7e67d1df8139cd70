// Depth-uncertainty gate on the device (lfd_depth_sigma_filter): every triangulated point gets sigma_rel, the 1-sigma bound on its
// relative depth error along the reference's ray (lfd_sigma.hpp), and the points at or below max_rel_sigma are compacted in order.
//
// Three launches in the scheme of the support filter (lfd_support.hip), nothing waits for another workgroup.  The first is this file's:
//
//   lfd_sigma_count_kernel<KMAX, CAND>   a lane per input point: sigma_rel (f32), a keep byte and the kept points of the workgroup; per
//                                        (reference, winning slot) counters through LDS, then one integer atomic per workgroup and slot
//
// The scan and the scatter are the shared tail (lfd_compact_launch, lfd_support.hip); sigma_rel is the extra plane that moves with the points.
//
// The front end is the per-point kernels' common one (lfd_device.hpp: lfd_point_span ... lfd_seg_flush): coalesced loads of the point's own
// fields, its reference from ref_offsets (device data), the reference's constants - its neighbours' descriptors and projection rows, its own
// centre, with planes the plane pointers and pixel-scale reciprocals - staged in LDS; a workgroup whose points straddle references takes them
// one after the other.  CAND false (no refine status): the winner alone takes part - one 12-byte precision gather per point, none in the
// isotropic form, and no other slot's certainty, warp or precision is touched.  CAND true: all k - 1 certainty loads, 8-byte warp loads and
// precision gathers of a point are issued before any arithmetic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_device.hpp"
#include "lfd_sigma.hpp"

hipError_t lfd_compact_launch(const LfdCompactArgs& p, hipStream_t stream);   // lfd_support.hip

template <int KMAX, bool CAND>
__global__ void __launch_bounds__(256) lfd_sigma_count_kernel(const LfdSigmaArgs p) {
    __shared__ LfdSlot sh[KMAX];
    __shared__ LfdSlotPrec shw[KMAX];
    __shared__ LfdSigmaRef sh_rc;
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
    bool accepted = false;
    if constexpr (CAND) accepted = (p.status[ii] & LFD_REFINE_ACCEPTED) != 0;
    int r_first, r_last;
    const int r = lfd_ref_range<1>(sh_ref, &sh_kept, st, sp, r_first, r_last);
    const LfdSupportGeom g = st.g;
    const long long HW = (long long)g.H * g.W;
    const bool cell_ok = cell >= 0 && (long long)cell < HW;            // no address is formed from a cell outside the grid
    const bool planes = p.prec != nullptr;                             // (uniform)
    float sigma = LFD_SIGMA_INF;
    bool keep = false;
    for (int rr = r_first; rr <= r_last; ++rr) {
        if (lfd_ref_empty(st, rr)) continue;
        const int ns = lfd_ref_slots<KMAX>(st, rr);
        if (tid < KMAX) sh_seg[tid] = 0u;
        lfd_stage_slots(sh, st.slots, st.pair_const, rr, st.k, ns);
        if (planes && tid < ns) {
            shw[tid].prec = p.prec[(size_t)rr * st.k + tid];
            lfd_slot_prec_scale(sh[tid].sx, sh[tid].sy, shw[tid]);
        }
        if (tid == 64) {
            const LfdRefConst& c = st.ref_const[rr];
            sh_rc.C[0] = c.C[0]; sh_rc.C[1] = c.C[1]; sh_rc.C[2] = c.C[2];
        }
        __syncthreads();
        const bool here = mine && r == rr;
        if (here) {
            if (cell_ok && s < ns) {
                float qs[3] = {0.0f, 0.0f, 0.0f};
                if (planes) {
                    const float* qp = shw[s].prec + (size_t)cell * 3;
                    qs[0] = qp[0]; qs[1] = qp[1]; qs[2] = qp[2];
                }
                if constexpr (CAND) {
                    // all gathers of the point first, then the arithmetic
                    float c[KMAX], wx[KMAX], wy[KMAX], q00[KMAX], q01[KMAX], q11[KMAX];
#pragma unroll
                    for (int j = 0; j < KMAX; ++j) {
                        c[j] = 0.0f; wx[j] = 0.0f; wy[j] = 0.0f; q00[j] = 0.0f; q01[j] = 0.0f; q11[j] = 0.0f;
                        if (accepted && j < ns && j != s) {
                            c[j] = sh[j].cert[cell];
                            const float2 w = *reinterpret_cast<const float2*>(sh[j].warp + (size_t)cell * g.C + (g.C - 2));
                            wx[j] = w.x; wy[j] = w.y;
                            if (planes) {
                                const float* qp = shw[j].prec + (size_t)cell * 3;
                                q00[j] = qp[0]; q01[j] = qp[1]; q11[j] = qp[2];
                            }
                        }
                    }
                    const LfdRefineGather o = {c, wx, wy, q00, q01, q11, qs};
                    sigma = lfd_sigma_point<KMAX, true>(sh_rc, sh, shw, ns, s, g, planes, p.iso, accepted, o, X0, X1, X2);
                } else {
                    const LfdRefineGather o = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, qs};
                    sigma = lfd_sigma_point<KMAX, false>(sh_rc, sh, shw, ns, s, g, planes, p.iso, false, o, X0, X1, X2);
                }
            }
            keep = lfd_sigma_keep(sigma, p.max_rel_sigma);
        }
        if (p.seg_counts) lfd_seg_tally<KMAX>(sh_seg, here && keep && s < ns, s);
        __syncthreads();
        if (p.seg_counts) lfd_seg_flush(sh_seg, p.seg_counts, rr, st.k, ns);
    }
    if (mine) {
        if (p.ws_sigma) p.ws_sigma[i] = sigma;                         // (uniform: only when sigma_rel moves with the points)
        p.keep[i] = keep ? (uint8_t)1 : (uint8_t)0;
        if (p.sigma) p.sigma[i] = sigma;
    }
    lfd_count_tally<1>(&sh_kept, {mine && keep});
    __syncthreads();
    if (tid == 0) p.wg_kept[blockIdx.x] = sh_kept;
}

template <bool CAND>
static void lfd_sigma_launch_k(const LfdSigmaArgs& p, hipStream_t stream) {
    const dim3 grid((unsigned)p.st.n_wg);
    if (p.st.k <= 4) hipLaunchKernelGGL((lfd_sigma_count_kernel<4, CAND>), grid, dim3(256), 0, stream, p);
    else if (p.st.k <= 8) hipLaunchKernelGGL((lfd_sigma_count_kernel<8, CAND>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((lfd_sigma_count_kernel<LFD_MAX_SLOTS, CAND>), grid, dim3(256), 0, stream, p);
}

// lfd_api.hip's lfd_depth_sigma_filter: the arguments were validated there (capacity <= 2^31 - 1: at most 2^23 workgroups); p.status picks
// the variant
hipError_t lfd_sigma_launch(const LfdSigmaArgs& p, const LfdCompactArgs& tail, hipStream_t stream) {
    if (p.st.n_wg > 0) {
        if (p.status) lfd_sigma_launch_k<true>(p, stream);
        else lfd_sigma_launch_k<false>(p, stream);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return lfd_compact_launch(tail, stream);
}
