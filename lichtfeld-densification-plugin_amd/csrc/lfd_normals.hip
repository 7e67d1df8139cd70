// Per-point surface normals on the device (lfd_estimate_normals): the normal of every point from the winning neighbour's warp in
// a (2R + 1)^2 window of grid cells around the point's own cell (lfd_normals.hpp).
//
// One launch, a lane per input point, nothing waits for another workgroup and nothing is scanned.  The frame is the per-point kernels' common one
// (lfd_device.hpp): coalesced loads of the point's own fields, its reference from ref_offsets (device data), the reference's constants and its
// neighbours' staged in LDS (a workgroup whose points straddle references takes them one after the other).  Inside a lane the window is
// walked in raster order - the accumulation order is fixed without any cross-lane reduction.  A whole window row's certainty and warp loads
// are issued before its arithmetic; in dense mode neighbouring lanes hold neighbouring cells, so a row's loads coalesce across the lanes.  The
// row is walked by a loop that is NOT unrolled: the two-view solver exists once per kernel, and only the sums of LfdNormalAcc and the row's
// values live across it.  One instantiation per radius, so that the row's values are registers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_device.hpp"
#include "lfd_normals.hpp"

// a[e] for a run-time e through compile-time indices: the array stays in registers.  (The empty statement keeps the optimiser from folding the
// selects back into one indexed load, which would move the array to scratch memory or LDS.)
template <int N>
__device__ __forceinline__ float lfd_pick(const float (&a)[N], int e) {
    float v = a[0];
#pragma unroll
    for (int j = 1; j < N; ++j) {
        v = (e == j) ? a[j] : v;
        asm volatile("" : "+v"(v));
    }
    return v;
}

template <int R>
__global__ void __launch_bounds__(256) lfd_normals_kernel(const LfdNormalArgs p) {
    constexpr int NW = 2 * R + 1;
    __shared__ LfdNormalSlot sh[LFD_MAX_SLOTS];
    __shared__ LfdPairConst sh_pc[LFD_MAX_SLOTS];
    __shared__ LfdRefConst sh_rc;
    __shared__ const uint8_t* sh_mask_a;
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
    int r_first, r_last;
    const int r = lfd_ref_range<2>(sh_ref, sh_cnt, st, sp, r_first, r_last);
    const LfdSupportGeom g = st.g;
    const long long HW = (long long)g.H * g.W;
    const bool cell_ok = cell >= 0 && (long long)cell < HW;            // no address is formed from a cell outside the grid
    const LfdRefDesc* refs = static_cast<const LfdRefDesc*>(st.refs);
    const LfdKernelParams kp = lfd_normal_params(g);
    unsigned status = 0u;
    float nrm[3] = {0.0f, 0.0f, 0.0f};
    for (int rr = r_first; rr <= r_last; ++rr) {
        if (lfd_ref_empty(st, rr)) continue;
        const int ns = lfd_ref_slots<LFD_MAX_SLOTS>(st, rr);
        if (tid < ns) {
            const LfdSlotDesc& d = static_cast<const LfdSlotDesc*>(st.slots)[(size_t)rr * st.k + tid];
            sh[tid].cert = d.cert; sh[tid].warp = d.warp; sh[tid].mask_b = d.mask_b;
            sh_pc[tid] = st.pair_const[(size_t)rr * st.k + tid];
        }
        if (tid == 64) { sh_rc = st.ref_const[rr]; sh_mask_a = refs[rr].mask_a; }
        __syncthreads();
        if (mine && r == rr) {
            LfdNormalPoint pt;
            const bool ok = lfd_normal_begin(sh_rc, X0, X1, X2, p.depth_step_rel, pt, nrm);
            if (ok && cell_ok && s < ns) {
                const float* cert = sh[s].cert;
                const float* warp = sh[s].warp;
                const uint8_t* mask_b = sh[s].mask_b;
                const uint8_t* mask_a = sh_mask_a;
                const int y = cell / g.W, x = cell - y * g.W;
                LfdNormalAcc acc;
                lfd_normal_clear(acc);
#pragma unroll 1
                for (int dy = -R; dy <= R; ++dy) {
                    const int qy = y + dy;
                    if (qy < 0 || qy >= g.H) continue;
                    // the row's loads first (cells outside the grid: nothing is loaded, a certainty of 0), then its arithmetic
                    float c[NW], wax[NW], way[NW], wbx[NW], wby[NW];
                    const float ya = (g.C == 4) ? 0.0f : st.axis_y[qy];
#pragma unroll
                    for (int e = 0; e < NW; ++e) {
                        const int qx = x + e - R;
                        c[e] = 0.0f; wax[e] = 0.0f; way[e] = ya; wbx[e] = 0.0f; wby[e] = 0.0f;
                        if (qx >= 0 && qx < g.W) {
                            const size_t q = (size_t)qy * g.W + qx;
                            c[e] = cert[q];
                            const float* wp = warp + q * g.C;
                            const float2 wb = *reinterpret_cast<const float2*>(wp + (g.C - 2));
                            wbx[e] = wb.x; wby[e] = wb.y;
                            if (g.C == 4) {
                                const float2 wa = *reinterpret_cast<const float2*>(wp);
                                wax[e] = wa.x; way[e] = wa.y;
                            } else {
                                wax[e] = st.axis_x[qx];
                            }
                        }
                    }
#pragma unroll 1
                    for (int e = 0; e < NW; ++e) {
                        const int qx = x + e - R;
                        if (qx < 0 || qx >= g.W) continue;
                        lfd_normal_cell(acc, pt, sh_rc, sh_pc[s], mask_a, mask_b, g, kp, qx, qy, e - R, dy, lfd_pick<NW>(c, e), lfd_pick<NW>(wax, e),
                                        lfd_pick<NW>(way, e), lfd_pick<NW>(wbx, e), lfd_pick<NW>(wby, e));
                    }
                }
                status = lfd_normal_finish(acc, pt, nrm);
            }
        }
        __syncthreads();                                               // the next reference's constants replace these
    }
    if (mine) {
        p.normals[3 * i] = nrm[0]; p.normals[3 * i + 1] = nrm[1]; p.normals[3 * i + 2] = nrm[2];
        if (p.status) p.status[i] = (uint8_t)status;
    }
    if (p.counters) {                                                  // (uniform)
        const bool fitted = (status & LFD_NORMAL_FITTED) != 0u;
        lfd_count_tally<2>(sh_cnt, {mine && fitted, mine && !fitted});
        __syncthreads();
        lfd_count_flush<2>(sh_cnt, p.counters);
    }
}

// lfd_api.hip's lfd_estimate_normals: the arguments were validated there (capacity <= 2^31 - 1: at most 2^23 workgroups, radius in 1..4)
hipError_t lfd_normals_launch(const LfdNormalArgs& p, hipStream_t stream) {
    if (p.st.n_wg <= 0) return hipSuccess;
    const dim3 grid((unsigned)p.st.n_wg);
    switch (p.radius) {
        case 1: hipLaunchKernelGGL((lfd_normals_kernel<1>), grid, dim3(256), 0, stream, p); break;
        case 2: hipLaunchKernelGGL((lfd_normals_kernel<2>), grid, dim3(256), 0, stream, p); break;
        case 3: hipLaunchKernelGGL((lfd_normals_kernel<3>), grid, dim3(256), 0, stream, p); break;
        case 4: hipLaunchKernelGGL((lfd_normals_kernel<4>), grid, dim3(256), 0, stream, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---- 27-byte PLY records with normals (lfd_pack_ply_normals): x y z nx ny nz (f32 LE) r g b (u8), assembled in LDS like lfd_pack_ply_kernel's
extern "C" __global__ void __launch_bounds__(256) lfd_pack_ply_normals_kernel(const float* __restrict__ xyz, const float* __restrict__ normals,
                                                                              const float* __restrict__ rgb, long long n,
                                                                              unsigned char* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) unsigned char rec[256 * 27];
    const int tid = (int)threadIdx.x;
    for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
        const long long i = base + tid;
        if (i < n) {
            unsigned char* r = rec + tid * 27;
            const float v[6] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const unsigned u = __float_as_uint(v[c]);
                r[4 * c + 0] = (unsigned char)(u); r[4 * c + 1] = (unsigned char)(u >> 8);
                r[4 * c + 2] = (unsigned char)(u >> 16); r[4 * c + 3] = (unsigned char)(u >> 24);
            }
            r[24] = lfd_quantise_u8(rgb[3 * i]); r[25] = lfd_quantise_u8(rgb[3 * i + 1]); r[26] = lfd_quantise_u8(rgb[3 * i + 2]);
        }
        __syncthreads();
        // [base * 27, + count * 27) bytes: the block start is 4-byte aligned because the block size is a multiple of 4 points
        const long long left = n - base;
        const int nbytes = (left < 256 ? (int)left : 256) * 27, nwords = nbytes >> 2;
        unsigned* out32 = reinterpret_cast<unsigned*>(out + base * 27);
        const unsigned* lds32 = reinterpret_cast<const unsigned*>(rec);
        for (int w = tid; w < nwords; w += 256) out32[w] = lds32[w];
        for (int b = (nwords << 2) + tid; b < nbytes; b += 256) out[base * 27 + b] = rec[b];
        __syncthreads();
    }
}
