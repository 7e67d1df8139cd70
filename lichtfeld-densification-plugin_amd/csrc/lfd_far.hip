// Far-field shell on the device (lfd_far_accumulate / lfd_far_emit).
//
// lfd_far_kernel: one launch per batch, grid (ceil(H W / 256), n_refs), a lane per grid cell of one reference.  The reference's neighbours
// (plane pointers, projection rows, pixel scales) are staged in LDS by the first lanes, its back-projection matrix by lane 0; the loop over
// slots is uniform, each slot's certainty (4 B) and observation (8 B) are read by consecutive lanes for consecutive cells, all gathers first.
// Only a far cell touches the image (two 6-byte rows) and does f64 work (two divisions, a root, three quotients).
//
// Neighbouring cells usually fall into the same direction cell (a reference's pixel is about a third of a direction cell at the defaults), so
// the seven integers are first summed over every run of consecutive lanes with one key - a segmented suffix sum, six shuffle steps - and the
// first lane of a run issues the seven no-return 64-bit atomic adds: a wave full of sky issues 7 x (runs) instead of 7 x 64 of them.  Integer
// additions only, so the table does not depend on the launch geometry.  A wave without a far cell skips all of it (a uniform branch).
//
// lfd_far_emit: a keep byte per direction cell, the cloud stages' compaction prefix (lfd_consensus_wgcount_kernel + lfd_voxel_scan_kernel),
// then a lane per direction cell writes its record at its rank - key order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_device.hpp"
#include "lfd_far.hpp"

template <int KMAX, int C, bool REDUCE>
__global__ void __launch_bounds__(256) lfd_far_kernel(const LfdFarArgs p) {
    __shared__ LfdSlot sh[KMAX];
    __shared__ float sh_M[9];
    __shared__ unsigned sh_far;
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int r = (int)blockIdx.y;
    const LfdSupportGeom g = p.g;
    const int HW = g.H * g.W;                                          // <= 2^31 - 1 (the batch was validated)
    const long long cell_ll = (long long)blockIdx.x * 256 + tid;
    const bool mine = cell_ll < (long long)HW;
    const int cell = mine ? (int)cell_ll : HW - 1;                     // idle lanes read the last cell and add nothing
    const LfdRefDesc ref = static_cast<const LfdRefDesc*>(p.refs)[r];
    int ns = ref.n_slots;
    ns = ns < KMAX ? ns : KMAX;
    lfd_stage_slots(sh, p.slots, p.pair_const, r, p.k, ns);
    if (tid == 0) {
        float M[9];
        lfd_far_dir_matrix(p.cams[ref.cam], M);
#pragma unroll
        for (int e = 0; e < 9; ++e) sh_M[e] = M[e];
        sh_far = 0u;
    }
    __syncthreads();
    const int y = cell / g.W, x = cell - y * g.W;
    // all gathers of the cell first, then the arithmetic
    float c[KMAX];
    float2 w[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
        c[j] = 0.0f; w[j] = make_float2(0.0f, 0.0f);
        if (j < ns) {                                                  // (uniform)
            c[j] = sh[j].cert[cell];
            w[j] = *reinterpret_cast<const float2*>(sh[j].warp + (size_t)cell * C + (C - 2));
        }
    }
    float xan, yan;
    if (C == 4) {
        const float2 a = *reinterpret_cast<const float2*>(sh[0].warp + (size_t)cell * C);
        xan = a.x; yan = a.y;
    } else {
        xan = p.axis_x[x]; yan = p.axis_y[y];
    }
    bool ok = mine;
    if (ok && ref.mask_a)
        ok = ref.mask_a[(size_t)lfd_nearest_src(y, g.mask_sy, g.h_match) * g.w_match + lfd_nearest_src(x, g.mask_sx, g.w_match)] != 0;
    float M[9], d[3];
#pragma unroll
    for (int e = 0; e < 9; ++e) M[e] = sh_M[e];
    const LfdRefConst& rc = p.ref_const[r];
    lfd_far_direction(M, rc.sx, rc.sy, xan, yan, g.wm1, g.hm1, d);
    int n_conf = 0, n_agree = 0;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
        if (j < ns) {
            const int v = lfd_far_slot(sh[j], g, p.far_certainty, c[j], w[j].x, w[j].y, d[0], d[1], d[2]);
            n_conf += v & 1; n_agree += v >> 1;
        }
    }
    bool far = ok && lfd_far_verdict(n_conf, n_agree, p.min_views, ns);
    const unsigned long long any = __ballot(far);
    if (any) {                                                         // (uniform within the wave)
        long long key = -1, q[3] = {0, 0, 0};
        unsigned col[3] = {0u, 0u, 0u}, cnt = 0u;
        if (far) far = lfd_far_key(d[0], d[1], d[2], p.S, &key, q);
        if (far) {
            float rgb[3];
            lfd_bilinear_rgb_f32(ref.image, g.w_match, g.h_match, lfd_match_px(xan, g.wm1), lfd_match_px(yan, g.hm1), rgb);
#pragma unroll
            for (int e = 0; e < 3; ++e) col[e] = (unsigned)lfd_quantise_u8(rgb[e]);
            cnt = 1u;
        } else {
            key = -1; q[0] = q[1] = q[2] = 0;
        }
        const unsigned long long fm = __ballot(far);
        if (p.flags && far) p.flags[(size_t)r * HW + cell] = (uint8_t)1;      // (the caller cleared them: a far lane is `mine`, cell < H W)
        bool issue = far;
        if (REDUCE && fm) {
            const long long prev = __shfl_up(key, 1, 64);
            const bool head = far && (lane == 0 || prev != key);       // (a lane that is not far carries key -1)
            const unsigned long long brk = __ballot(head) | ~fm;       // lanes at which a run cannot continue
            const unsigned long long above = lane == 63 ? 0ull : brk & ~((2ull << lane) - 1ull);
            const int end = above ? (int)__builtin_ctzll(above) - 1 : 63;   // last lane of this lane's run
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const bool take = lane + off <= end;
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const long long tq = __shfl_down(q[e], off, 64);
                    const unsigned tc = __shfl_down(col[e], off, 64);
                    if (take) { q[e] += tq; col[e] += tc; }
                }
                const unsigned tn = __shfl_down(cnt, off, 64);
                if (take) cnt += tn;
            }
            issue = head;
        }
        if (issue) {                                                   // key in [0, 6 S S): the table holds that many rows
            unsigned long long* row = p.table + (size_t)key * LFD_FAR_QUANTITIES;
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                atomicAdd(row + e, (unsigned long long)q[e]);
                atomicAdd(row + 3 + e, (unsigned long long)col[e]);
            }
            atomicAdd(row + 6, (unsigned long long)cnt);
        }
        if (p.counters && fm && lane == 0) atomicAdd(&sh_far, (unsigned)__popcll(fm));
    }
    if (p.counters) {
        __syncthreads();
        if (tid == 0 && sh_far) atomicAdd(p.counters + r, (unsigned long long)sh_far);
    }
}

// keep byte of every direction cell
__global__ void __launch_bounds__(256) lfd_far_mark_kernel(const unsigned long long* __restrict__ table, long long n_cells, long long min_samples,
                                                           uint8_t* __restrict__ keep) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_cells) return;
    uint64_t row[LFD_FAR_QUANTITIES];
#pragma unroll
    for (int e = 0; e < LFD_FAR_QUANTITIES; ++e) row[e] = table[i * LFD_FAR_QUANTITIES + e];
    keep[i] = lfd_far_kept(row, min_samples) ? (uint8_t)1 : (uint8_t)0;
}

// lfd_consensus_scatter_kernel's placement, a record where that copies a point
__global__ void __launch_bounds__(256) lfd_far_emit_kernel(const LfdFarEmitArgs p) {
    __shared__ unsigned wc[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long i = (long long)blockIdx.x * 256 + tid;
    const bool kept = i < p.n_cells && p.keep[i < p.n_cells ? i : 0] != 0;
    const unsigned long long m = __ballot(kept);
    if (lane == 0) wc[wave] = (unsigned)__popcll(m);
    __syncthreads();
    if (!kept) return;
    unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    for (int w = 0; w < wave; ++w) rank += wc[w];
    const long long o = (long long)p.wg_kept[blockIdx.x] + rank;
    if (o >= p.capacity) return;                                       // counted, not written
    uint64_t row[LFD_FAR_QUANTITIES];
#pragma unroll
    for (int e = 0; e < LFD_FAR_QUANTITIES; ++e) row[e] = p.table[i * LFD_FAR_QUANTITIES + e];
    float xyz[3], rgb[3], nrm[3];
    int32_t samples;
    lfd_far_record(row, p.centre, p.radius, xyz, rgb, nrm, &samples);
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        p.xyz[3 * o + e] = xyz[e];
        p.rgb[3 * o + e] = rgb[e];
        if (p.normal) p.normal[3 * o + e] = nrm[e];
    }
    if (p.samples) p.samples[o] = samples;
}

template <int C, bool REDUCE>
static void lfd_far_launch_c(const LfdFarArgs& p, dim3 grid, hipStream_t stream) {
    if (p.k <= 4) hipLaunchKernelGGL((lfd_far_kernel<4, C, REDUCE>), grid, dim3(256), 0, stream, p);
    else if (p.k <= 8) hipLaunchKernelGGL((lfd_far_kernel<8, C, REDUCE>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((lfd_far_kernel<LFD_MAX_SLOTS, C, REDUCE>), grid, dim3(256), 0, stream, p);
}

// lfd_api.hip's lfd_far_accumulate: the arguments were validated there (H W <= 2^31 - 1, n_refs <= 65535 workgroup rows, warp_channels 2 or 4).
// reduce = false: every far lane issues its own seven adds - the same table, kept for profiles/far_timing.py's comparison.
hipError_t lfd_far_launch(const LfdFarArgs& p, bool reduce, hipStream_t stream) {
    const long long HW = (long long)p.g.H * p.g.W;
    const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)p.n_refs);
    if (p.g.C == 2) { if (reduce) lfd_far_launch_c<2, true>(p, grid, stream); else lfd_far_launch_c<2, false>(p, grid, stream); }
    else { if (reduce) lfd_far_launch_c<4, true>(p, grid, stream); else lfd_far_launch_c<4, false>(p, grid, stream); }
    return hipGetLastError();
}

hipError_t lfd_far_mark_launch(const unsigned long long* table, long long n_cells, long long min_samples, uint8_t* keep, hipStream_t stream) {
    hipLaunchKernelGGL(lfd_far_mark_kernel, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, stream, table, n_cells, min_samples, keep);
    return hipGetLastError();
}

hipError_t lfd_far_emit_launch(const LfdFarEmitArgs& p, hipStream_t stream) {
    hipLaunchKernelGGL(lfd_far_emit_kernel, dim3((unsigned)((p.n_cells + 255) / 256)), dim3(256), 0, stream, p);
    return hipGetLastError();
}
