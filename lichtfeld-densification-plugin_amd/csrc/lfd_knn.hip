// Gaussian-ready output on the device (lfd_knn_dist2, lfd_pack_gaussians): the exact mean squared distance of every point to its
// three nearest neighbours, and the 68-byte 3DGS record.  lfd_knn.hpp has the distance, the best-three update, the ring scan of one point and the
// record, shared with the twin.
//
// Min / max is lfd_consensus.hip's kernel, the stable LSD radix sort and the cell heads are lfd_voxel.hip's, launched with this call's buffers
// (lfd_api.hip's lfd_knn_dist2 issues everything).  Behind them, one launch each, nothing waits for another workgroup:
//
//   lfd_knn_keys_kernel       linear cell key of every point and the identity payload
//   lfd_knn_cellmax_kernel    points in the fullest cell, from the cell heads (a statistic of the call)
//   lfd_knn_gather_kernel     the points in cell order as 16-byte records {x, y, z, input index}
//   lfd_knn_scan_kernel       the hot path: a lane per sorted point walks the rings around its cell (neighbouring lanes read neighbouring cells);
//                             the result goes to the point's INPUT index; a point no ring settles is appended to a list (one vector atomic on a
//                             counter; the order of the list does not matter)
//   lfd_knn_brute_kernel      a workgroup per listed point: the lanes stride over the whole cloud, their triples are merged across the wave by
//                             shuffles and across the waves through LDS
//   lfd_pack_gaussians_kernel 17 f32 per point, assembled in LDS and written in runs
//
// The best three live in three registers updated by compare-select chains: nothing is indexed at run time.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_device.hpp"
#include "lfd_knn.hpp"

extern "C" __global__ void __launch_bounds__(256) lfd_knn_keys_kernel(const float* __restrict__ xyz, long long n, LfdKnnGrid g,
                                                                     unsigned long long* __restrict__ keys, unsigned* __restrict__ idx) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        keys[i] = lfd_knn_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], g);
        idx[i] = (unsigned)i;
    }
}

// vstart[v]: first sorted position of cell v (lfd_voxel_head_scatter_kernel); *max_out was zeroed by the caller
extern "C" __global__ void __launch_bounds__(256) lfd_knn_cellmax_kernel(const unsigned* __restrict__ vstart, const unsigned* __restrict__ nv_p,
                                                                        long long n, unsigned* __restrict__ max_out) {
    const long long nv = (long long)*nv_p;
    unsigned mine = 0u;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (long long)gridDim.x * 256) {
        const long long a = vstart[v], b = v + 1 < nv ? (long long)vstart[v + 1] : n;
        mine = max(mine, (unsigned)(b - a));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine = max(mine, (unsigned)__shfl_xor((int)mine, off, 64));
    if ((threadIdx.x & 63) == 0 && mine) atomicMax(max_out, mine);
}

extern "C" __global__ void __launch_bounds__(256) lfd_knn_gather_kernel(const float* __restrict__ xyz, const unsigned* __restrict__ sorted_idx,
                                                                       long long n, LfdKnnPt* __restrict__ spt) {
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long long)gridDim.x * 256) {
        const unsigned i = sorted_idx[j];                              // < n: the sort's payload is a permutation of 0 .. n - 1
        LfdKnnPt p;
        p.x = xyz[3 * (long long)i]; p.y = xyz[3 * (long long)i + 1]; p.z = xyz[3 * (long long)i + 2];
        p.idx = i;
        spt[j] = p;
    }
}

// list holds n entries: every point may end up in it
extern "C" __global__ void __launch_bounds__(256) lfd_knn_scan_kernel(const unsigned long long* __restrict__ skey, const LfdKnnPt* __restrict__ spt,
                                                                     long long n, LfdKnnGrid g, float* __restrict__ dist2,
                                                                     unsigned* __restrict__ list, unsigned* __restrict__ n_list) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    float mean;
    if (lfd_knn_scan_point(skey, spt, n, j, g, &mean)) dist2[spt[j].idx] = mean;
    else list[atomicAdd(n_list, 1u)] = (unsigned)j;
}

extern "C" __global__ void __launch_bounds__(256) lfd_knn_brute_kernel(const LfdKnnPt* __restrict__ spt, long long n, const unsigned* __restrict__ list,
                                                                      const unsigned* __restrict__ n_list, float* __restrict__ dist2) {
    __shared__ float sh[4][3];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned nl = *n_list;                                       // <= n
    for (unsigned e = blockIdx.x; e < nl; e += gridDim.x) {
        const long long j = list[e];                                   // < n
        const LfdKnnPt me = spt[j];
        float a = __builtin_inff(), b = __builtin_inff(), c = __builtin_inff();
        for (long long q = tid; q < n; q += 256) {
            if (q == j) continue;
            const LfdKnnPt p = spt[q];
            lfd_knn_insert(lfd_knn_d2(me.x, me.y, me.z, p.x, p.y, p.z), a, b, c);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float oa = __shfl_xor(a, off, 64), ob = __shfl_xor(b, off, 64), oc = __shfl_xor(c, off, 64);
            lfd_knn_insert(oa, a, b, c);
            lfd_knn_insert(ob, a, b, c);
            lfd_knn_insert(oc, a, b, c);
        }
        if (lane == 0) { sh[wave][0] = a; sh[wave][1] = b; sh[wave][2] = c; }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                lfd_knn_insert(sh[w][0], a, b, c);
                lfd_knn_insert(sh[w][1], a, b, c);
                lfd_knn_insert(sh[w][2], a, b, c);
            }
            dist2[me.idx] = lfd_knn_mean(a, b, c);
        }
        __syncthreads();
    }
}

extern "C" __global__ void __launch_bounds__(256) lfd_pack_gaussians_kernel(const float* __restrict__ xyz, const float* __restrict__ normals,
                                                                           const float* __restrict__ rgb, const float* __restrict__ dist2,
                                                                           long long n, float opacity, double log_flatten, float max_m,
                                                                           float* __restrict__ out) {
    __shared__ float rec[256 * LFD_GAUSS_FLOATS];
    const int tid = (int)threadIdx.x;
    for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
        const long long i = base + tid;
        if (i < n) {
            float o[LFD_GAUSS_FLOATS];
            lfd_gauss_record(xyz + 3 * i, normals + 3 * i, rgb + 3 * i, dist2[i], opacity, log_flatten, max_m, o);
#pragma unroll
            for (int c = 0; c < LFD_GAUSS_FLOATS; ++c) rec[tid * LFD_GAUSS_FLOATS + c] = o[c];
        }
        __syncthreads();
        const long long left = n - base;
        const int words = (int)(left < 256 ? left : 256) * LFD_GAUSS_FLOATS;
        for (int k = tid; k < words; k += 256) out[base * LFD_GAUSS_FLOATS + k] = rec[k];
        __syncthreads();
    }
}
