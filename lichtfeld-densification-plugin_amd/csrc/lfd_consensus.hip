// Cross-reference consensus filter on the device (lfd_consensus_filter): a point of the final cloud is kept iff at least min_refs
// OTHER references own a point within `radius` of it (lfd_consensus.hpp has the test and the per-point count, shared with the twin).
//
// Phases, one launch each, nothing waits for another workgroup (lfd_api.hip's lfd_consensus_filter issues them):
//
//   lfd_consensus_minmax_kernel    min / max over the points whose three coordinates are finite (then lfd_voxel_final_kernel)
//   lfd_consensus_keys_kernel      linear cell key of every point (a sentinel that sorts last for a non-finite one) and the identity payload
//   the stable LSD radix sort      lfd_voxel.hip's histogram / scan / scatter kernels, launched as they are: nothing of them is copied or moved
//   lfd_consensus_gather_kernel    the points in cell order as 16-byte records {x, y, z, reference}; the reference by binary search of the offsets
//   lfd_consensus_count_kernel     the hot path: a lane per sorted point walks the 9 key ranges around its cell; count and keep byte at the
//                                  point's ORIGINAL index
//   lfd_consensus_wgcount_kernel   kept points per 256 input points; lfd_voxel_scan_kernel makes their exclusive prefix
//   lfd_consensus_offsets_kernel   ref_offsets_out from the prefix
//   lfd_consensus_scatter_kernel   stable compaction in input order (the scheme of the support filter's scatter)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_device.hpp"
#include "lfd_consensus.hpp"

extern "C" __global__ void __launch_bounds__(256) lfd_consensus_minmax_kernel(const float* __restrict__ xyz, long long n, LfdVoxStats* __restrict__ part) {
    __shared__ float sh[6][256];
    __shared__ unsigned sh_flags;
    const int tid = (int)threadIdx.x;
    float v[6] = {__builtin_inff(), __builtin_inff(), __builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    unsigned flags = 0u;
    if (tid == 0) sh_flags = 0u;
    for (long long i = (long long)blockIdx.x * 256 + tid; i < n; i += (long long)gridDim.x * 256) {
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        if (lfd_consensus_finite(x, y, z)) {
            v[0] = fminf(v[0], x); v[1] = fminf(v[1], y); v[2] = fminf(v[2], z);
            v[3] = fmaxf(v[3], x); v[4] = fmaxf(v[4], y); v[5] = fmaxf(v[5], z);
        } else {
            flags = LFD_VOX_NONFINITE;
        }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) sh[c][tid] = v[c];
    __syncthreads();
    if (flags) atomicOr(&sh_flags, flags);
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                sh[c][tid] = fminf(sh[c][tid], sh[c][tid + w]);
                sh[3 + c][tid] = fmaxf(sh[3 + c][tid], sh[3 + c][tid + w]);
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        LfdVoxStats s;
#pragma unroll
        for (int c = 0; c < 3; ++c) { s.lo[c] = sh[c][0]; s.hi[c] = sh[3 + c][0]; }
        s.cmax = -__builtin_inff();
        s.flags = sh_flags;
        part[blockIdx.x] = s;
    }
}

extern "C" __global__ void __launch_bounds__(256) lfd_consensus_keys_kernel(const float* __restrict__ xyz, long long n, double o0, double o1, double o2,
                                                                           double h, unsigned long long e1, unsigned long long e2,
                                                                           unsigned long long sentinel, unsigned long long* __restrict__ keys,
                                                                           unsigned* __restrict__ idx) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        keys[i] = lfd_consensus_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], o0, o1, o2, h, e1, e2, sentinel);
        idx[i] = (unsigned)i;
    }
}

// reference of input point i: the last r in [0, n_refs) with offs[r] <= i (offs[0] = 0; an empty reference owns nothing)
__device__ __forceinline__ int consensus_ref_of(const long long* __restrict__ offs, int n_refs, long long i) {
    int lo = 0, hi = n_refs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offs[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

extern "C" __global__ void __launch_bounds__(256) lfd_consensus_gather_kernel(const float* __restrict__ xyz, const unsigned* __restrict__ sorted_idx,
                                                                             const long long* __restrict__ offs, int n_refs, long long n,
                                                                             LfdConsensusPt* __restrict__ spt) {
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long long)gridDim.x * 256) {
        const long long i = sorted_idx[j];
        LfdConsensusPt p;
        p.x = xyz[3 * i]; p.y = xyz[3 * i + 1]; p.z = xyz[3 * i + 2];
        p.ref = consensus_ref_of(offs, n_refs, i);
        spt[j] = p;
    }
}

// One lane per sorted point: the lanes of a wave are neighbours in space, their searches take the same turns and their walks read the same lines.
// bound: min_refs when nobody asked for the counts (the walk stops as soon as the point is kept), else LFD_CONSENSUS_CAP.
extern "C" __global__ void __launch_bounds__(256) lfd_consensus_count_kernel(const unsigned long long* __restrict__ skey,
                                                                            const LfdConsensusPt* __restrict__ spt,
                                                                            const unsigned* __restrict__ sorted_idx, long long n,
                                                                            unsigned long long e1, unsigned long long e2,
                                                                            unsigned long long sentinel, float r2, int min_refs, int bound,
                                                                            uint8_t* __restrict__ keep, uint8_t* __restrict__ consensus) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    int c = 0;
    if (skey[j] != sentinel) c = lfd_consensus_count_point<LFD_CONSENSUS_CAP>(skey, spt, n, j, e1, e2, r2, bound);
    const long long i = sorted_idx[j];                                 // < n: the sort's payload is a permutation of 0 .. n - 1
    keep[i] = c >= min_refs ? (uint8_t)1 : (uint8_t)0;
    if (consensus) consensus[i] = (uint8_t)c;
}

extern "C" __global__ void __launch_bounds__(256) lfd_consensus_wgcount_kernel(const uint8_t* __restrict__ keep, long long n, unsigned* __restrict__ wg_kept) {
    __shared__ unsigned wc[4];
    const int tid = (int)threadIdx.x;
    const long long i = (long long)blockIdx.x * 256 + tid;
    const unsigned long long m = __ballot(i < n && keep[i < n ? i : 0] != 0);
    if ((tid & 63) == 0) wc[tid >> 6] = (unsigned)__popcll(m);
    __syncthreads();
    if (tid == 0) wg_kept[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// offs_out[r] = kept points in front of input point offs[r]: the prefix of that point's workgroup (wg_kept[n_wg] holds the total) plus the kept
// points before it inside the workgroup
extern "C" __global__ void __launch_bounds__(256) lfd_consensus_offsets_kernel(const long long* __restrict__ offs, int n_refs, const uint8_t* __restrict__ keep,
                                                                              const unsigned* __restrict__ wg_kept, long long* __restrict__ offs_out) {
    for (int r = (int)(blockIdx.x * 256 + threadIdx.x); r <= n_refs; r += (int)(gridDim.x * 256)) {
        const long long at = offs[r];                                  // validated on the host: 0 <= at <= n
        const long long wg = at >> 8;
        long long acc = wg_kept[wg];
        for (long long q = wg << 8; q < at; ++q) acc += keep[q] ? 1 : 0;
        offs_out[r] = acc;
    }
}

extern "C" __global__ void __launch_bounds__(256) lfd_consensus_scatter_kernel(const float* __restrict__ xyz, const float* __restrict__ rgb,
                                                                              const float* __restrict__ err, long long n,
                                                                              const uint8_t* __restrict__ keep, const unsigned* __restrict__ wg_kept,
                                                                              float* __restrict__ o_xyz, float* __restrict__ o_rgb,
                                                                              float* __restrict__ o_err) {
    __shared__ unsigned wc[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long i = (long long)blockIdx.x * 256 + tid;
    const bool kept = i < n && keep[i < n ? i : 0] != 0;
    const unsigned long long m = __ballot(kept);
    if (lane == 0) wc[wave] = (unsigned)__popcll(m);
    __syncthreads();
    if (!kept) return;
    unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    for (int w = 0; w < wave; ++w) rank += wc[w];
    const long long o = (long long)wg_kept[blockIdx.x] + rank;         // <= i < n: the outputs hold n points
    o_xyz[3 * o] = xyz[3 * i]; o_xyz[3 * o + 1] = xyz[3 * i + 1]; o_xyz[3 * o + 2] = xyz[3 * i + 2];
    if (rgb) { o_rgb[3 * o] = rgb[3 * i]; o_rgb[3 * o + 1] = rgb[3 * i + 1]; o_rgb[3 * o + 2] = rgb[3 * i + 2]; }
    if (err) o_err[o] = err[i];
}
