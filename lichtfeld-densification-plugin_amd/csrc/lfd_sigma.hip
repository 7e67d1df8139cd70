// Depth-uncertainty gate on the device (lfd_depth_sigma_filter): every triangulated point gets sigma_rel, the 1-sigma bound on its
// relative depth error along the reference's ray (lfd_sigma.hpp), and the points at or below max_rel_sigma are compacted in order.
//
// Three launches in the scheme of the support filter (lfd_support.hip), nothing waits for another workgroup:
//
//   lfd_sigma_count_kernel<KMAX, CAND>   a lane per input point: sigma_rel (f32), a keep byte and the kept points of the workgroup; per
//                                        (reference, winning slot) counters through LDS, then one integer atomic per workgroup and slot
//   lfd_sigma_scan_kernel                one workgroup: exclusive prefix of the workgroups' counts, then ref_offsets_out from it
//   lfd_sigma_scatter_kernel             a lane per input point: rank inside the wave by ballot / mbcnt, inside the workgroup by wave sums, copy
//
// The front end is lfd_support_count_kernel's and lfd_refine_kernel's, from the same helpers (lfd_device.hpp): coalesced loads of the point's own
// fields, its reference from ref_offsets (device data), the reference's constants - its neighbours' descriptors and projection rows, its own
// centre, with planes the plane pointers and pixel-scale reciprocals - staged in LDS; a workgroup whose points straddle references takes them
// one after the other.  CAND false (no refine status): the winner alone takes part - one 12-byte precision gather per point, none in the
// isotropic form, and no other slot's certainty, warp or precision is touched.  CAND true: all k - 1 certainty loads, 8-byte warp loads and
// precision gathers of a point are issued before any arithmetic.  The scan and the scatter are copies of the support filter's, which stays as
// it is: they read a keep byte instead of a support count, and the scatter also moves sigma_rel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_device.hpp"
#include "lfd_sigma.hpp"

template <int KMAX, bool CAND>
__global__ void __launch_bounds__(256) lfd_sigma_count_kernel(const LfdSigmaArgs p) {
    __shared__ LfdSlot sh[KMAX];
    __shared__ LfdSlotPrec shw[KMAX];
    __shared__ LfdSigmaRef sh_rc;
    __shared__ unsigned sh_seg[KMAX];
    __shared__ int sh_ref[2];
    __shared__ unsigned sh_kept;
    const int tid = (int)threadIdx.x;
    const LfdPointSpan sp = lfd_point_span(p.offs_in, p.n_refs, p.capacity);
    if (!sp.any) {                                                      // the whole workgroup lies past the last point
        if (tid == 0) p.wg_kept[blockIdx.x] = 0u;
        return;
    }
    const long long i = sp.i, ii = sp.ii;
    const bool mine = sp.mine;
    const int cell = p.cell[ii];
    const int s = (int)p.slot[ii];
    const float X0 = p.xyz[3 * ii], X1 = p.xyz[3 * ii + 1], X2 = p.xyz[3 * ii + 2];
    bool accepted = false;
    if constexpr (CAND) accepted = (p.status[ii] & LFD_REFINE_ACCEPTED) != 0;
    const int r = lfd_support_ref_of(p.offs_in, p.n_refs, p.capacity, ii);
    if (tid == 0) { sh_ref[0] = r; sh_kept = 0u; }
    if (i == sp.last) sh_ref[1] = r;
    __syncthreads();
    const int r_first = sh_ref[0], r_last = sh_ref[1];
    const LfdSupportGeom g = p.g;
    const long long HW = (long long)g.H * g.W;
    const bool cell_ok = cell >= 0 && (long long)cell < HW;            // no address is formed from a cell outside the grid
    const bool planes = p.prec != nullptr;                             // (uniform)
    const LfdRefDesc* refs = static_cast<const LfdRefDesc*>(p.refs);
    float sigma = LFD_SIGMA_INF;
    bool keep = false;
    for (int rr = r_first; rr <= r_last; ++rr) {
        if (lfd_support_clamp(p.offs_in[rr + 1], p.capacity) <= lfd_support_clamp(p.offs_in[rr], p.capacity)) continue;   // uniform: no points
        int ns = refs[rr].n_slots;
        ns = ns < KMAX ? ns : KMAX;
        if (tid < KMAX) sh_seg[tid] = 0u;
        lfd_stage_slots(sh, p.slots, p.pair_const, rr, p.k, ns);
        if (planes && tid < ns) {
            shw[tid].prec = p.prec[(size_t)rr * p.k + tid];
            lfd_slot_prec_scale(sh[tid].sx, sh[tid].sy, shw[tid]);
        }
        if (tid == 64) {
            const LfdRefConst& c = p.ref_const[rr];
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
        if (p.seg_counts) {
            const bool kept_here = here && keep && s < ns;
#pragma unroll
            for (int j = 0; j < KMAX; ++j) {
                const unsigned long long m = __ballot(kept_here && s == j);
                if (m && (tid & 63) == 0) atomicAdd(&sh_seg[j], (unsigned)__popcll(m));
            }
        }
        __syncthreads();
        if (p.seg_counts && tid < ns && sh_seg[tid]) atomicAdd(p.seg_counts + (size_t)rr * p.k + tid, (int)sh_seg[tid]);
    }
    if (mine) {
        p.ws_sigma[i] = sigma;
        p.keep[i] = keep ? (uint8_t)1 : (uint8_t)0;
        if (p.sigma) p.sigma[i] = sigma;
    }
    const unsigned long long km = __ballot(mine && keep);
    if ((tid & 63) == 0 && km) atomicAdd(&sh_kept, (unsigned)__popcll(km));
    __syncthreads();
    if (tid == 0) p.wg_kept[blockIdx.x] = sh_kept;
}

// exclusive prefix of wg_kept[0 .. n_wg) in place (the total goes to wg_kept[n_wg]), then ref_offsets_out[r] = kept points before
// ref_offsets_in[r]: the prefix of that point's workgroup plus the kept points in front of it inside the workgroup.  One workgroup.
__global__ void __launch_bounds__(1024) lfd_sigma_scan_kernel(const LfdSigmaArgs p) {
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

__global__ void __launch_bounds__(256) lfd_sigma_scatter_kernel(const LfdSigmaArgs p) {
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
    if (p.o_sigma) p.o_sigma[o] = p.ws_sigma[i];
}

template <bool CAND>
static void lfd_sigma_launch_k(const LfdSigmaArgs& p, hipStream_t stream) {
    const dim3 grid((unsigned)p.n_wg);
    if (p.k <= 4) hipLaunchKernelGGL((lfd_sigma_count_kernel<4, CAND>), grid, dim3(256), 0, stream, p);
    else if (p.k <= 8) hipLaunchKernelGGL((lfd_sigma_count_kernel<8, CAND>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((lfd_sigma_count_kernel<LFD_MAX_SLOTS, CAND>), grid, dim3(256), 0, stream, p);
}

// lfd_api.hip's lfd_depth_sigma_filter: the arguments were validated there (capacity <= 2^31 - 1: at most 2^23 workgroups); p.status picks
// the variant
hipError_t lfd_sigma_launch(const LfdSigmaArgs& p, hipStream_t stream) {
    if (p.n_wg > 0) {
        if (p.status) lfd_sigma_launch_k<true>(p, stream);
        else lfd_sigma_launch_k<false>(p, stream);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(lfd_sigma_scan_kernel, dim3(1), dim3(1024), 0, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (p.n_wg > 0) {
        hipLaunchKernelGGL(lfd_sigma_scatter_kernel, dim3((unsigned)p.n_wg), dim3(256), 0, stream, p);
        e = hipGetLastError();
    }
    return e;
}
