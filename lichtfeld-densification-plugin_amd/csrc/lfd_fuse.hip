// Oriented voxel fusion on the device (lfd_fuse_oriented): one oriented point per visible face of every occupied voxel.
// lfd_fuse.hpp has the usable-normal test, the side of a point and what a row is made of, shared with the twin.
//
// Min / max, keys, the stable LSD radix sort and the voxel heads are lfd_voxel.hip's kernels, launched with this call's buffers (lfd_api.hip's
// lfd_fuse_oriented issues everything).  Behind them, one launch each, nothing waits for another workgroup:
//
//   lfd_fuse_side_kernel        a thread per voxel of at most LFD_VOX_BIG points walks it in sorted (= input) order: the first usable normal
//                               is the pivot; a flag byte per sorted point (side, usable) and the voxel's 1 or 2 rows.  Larger voxels are listed
//   lfd_fuse_side_big_kernel    a wave per listed voxel: the pivot by a ballot over 64 points at a time (it may lie anywhere), then the flags
//   lfd_fuse_rowsum_kernel      rows per workgroup chunk of voxels  -> lfd_voxel_scan_kernel over the chunks (and the total number of rows)
//   lfd_fuse_rowstart_kernel    the row counts become each voxel's first output row, in place
//   lfd_fuse_sums_kernel        a thread per small voxel: both sides' f64 sums in point order, then its rows
//   lfd_fuse_sums_big_kernel    a wave per listed voxel: 256 points at a time staged in LDS while the next 256 load; lane 9 s + c adds
//                               component c (xyz, colour, normal) of side s in point order - 18 accumulators
//
// No atomics on floating-point values; the sums run in ascending input index because the sort is stable.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_device.hpp"
#include "lfd_fuse.hpp"

namespace {

__device__ __forceinline__ void voxel_span(const unsigned* __restrict__ vstart, long long nv, long long n, long long v, long long& a, long long& b) {
    a = vstart[v];
    b = v + 1 < nv ? (long long)vstart[v + 1] : n;
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256) lfd_fuse_side_kernel(const float* __restrict__ normals, long long n,
                                                                      const unsigned* __restrict__ sorted_idx, const unsigned* __restrict__ vstart,
                                                                      const unsigned* __restrict__ nv_p, uint8_t* __restrict__ flag,
                                                                      unsigned* __restrict__ rows, unsigned* __restrict__ big,
                                                                      unsigned* __restrict__ n_big) {
    const long long nv = (long long)*nv_p;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (long long)gridDim.x * 256) {
        long long a, b;
        voxel_span(vstart, nv, n, v, a, b);
        if (b - a > LFD_VOX_BIG) {
            big[atomicAdd(n_big, 1u)] = (unsigned)v;           // (at most n / (LFD_VOX_BIG + 1) voxels are this large: the list holds them)
            continue;
        }
        float piv[3] = {0.0f, 0.0f, 0.0f};
        bool has = false;
        unsigned two = 0u;
        for (long long j = a; j < b; ++j) {
            const long long i = sorted_idx[j];
            const float nn[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
            const unsigned f = lfd_fuse_flag(nn, has, piv);
            if (!has && (f & LFD_FUSE_USABLE)) { has = true; piv[0] = nn[0]; piv[1] = nn[1]; piv[2] = nn[2]; }
            two |= f & LFD_FUSE_SIDE;
            flag[j] = (uint8_t)f;
        }
        rows[v] = 1u + two;
    }
}

extern "C" __global__ void __launch_bounds__(64) lfd_fuse_side_big_kernel(const float* __restrict__ normals, long long n,
                                                                         const unsigned* __restrict__ sorted_idx, const unsigned* __restrict__ vstart,
                                                                         const unsigned* __restrict__ nv_p, const unsigned* __restrict__ big,
                                                                         const unsigned* __restrict__ n_big, uint8_t* __restrict__ flag,
                                                                         unsigned* __restrict__ rows) {
    const int lane = (int)threadIdx.x;
    const long long nv = (long long)*nv_p;
    const unsigned nb = *n_big;
    for (unsigned e = blockIdx.x; e < nb; e += gridDim.x) {
        const long long v = big[e];
        long long a, b;
        voxel_span(vstart, nv, n, v, a, b);
        // the pivot: the first sorted position with a usable normal (the loop is uniform over the wave)
        long long pj = -1;
        for (long long at = a; at < b && pj < 0; at += 64) {
            const long long j = at + lane;
            bool u = false;
            if (j < b) {
                const long long i = sorted_idx[j];
                u = lfd_fuse_usable(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]);
            }
            const unsigned long long m = __ballot(u);
            if (m) pj = at + (long long)__builtin_ctzll(m);
        }
        float piv[3] = {0.0f, 0.0f, 0.0f};
        const bool has = pj >= 0;
        if (has) {
            const long long i = sorted_idx[pj];
            piv[0] = normals[3 * i]; piv[1] = normals[3 * i + 1]; piv[2] = normals[3 * i + 2];
        }
        unsigned two = 0u;
        for (long long j = a + lane; j < b; j += 64) {
            const long long i = sorted_idx[j];
            const float nn[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
            // (the pivot itself and every point in front of it: has_pivot = false gives them side 0, as the definition does)
            const unsigned f = lfd_fuse_flag(nn, has && j > pj, piv);
            two |= f & LFD_FUSE_SIDE;
            flag[j] = (uint8_t)f;
        }
        const unsigned long long any = __ballot(two != 0u);
        if (lane == 0) rows[v] = any ? 2u : 1u;
    }
}

// Workgroup g owns the voxels [g * chunk, min(nv, (g + 1) * chunk)); chunk is a multiple of 256
extern "C" __global__ void __launch_bounds__(256) lfd_fuse_rowsum_kernel(const unsigned* __restrict__ rows, const unsigned* __restrict__ nv_p,
                                                                        long long chunk, unsigned* __restrict__ counts) {
    __shared__ unsigned c;
    if (threadIdx.x == 0) c = 0u;
    __syncthreads();
    const long long nv = (long long)*nv_p;
    const long long lo = (long long)blockIdx.x * chunk;
    const long long hi = lo + chunk < nv ? lo + chunk : nv;
    unsigned mine = 0u;
    for (long long v = lo + threadIdx.x; v < hi; v += 256) mine += rows[v];
    atomicAdd(&c, mine);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// rows[v] (1 or 2) -> the first output row of voxel v; counts: the exclusive prefix of lfd_fuse_rowsum_kernel's sums
extern "C" __global__ void __launch_bounds__(256) lfd_fuse_rowstart_kernel(unsigned* __restrict__ rows, const unsigned* __restrict__ nv_p,
                                                                          long long chunk, const unsigned* __restrict__ counts) {
    __shared__ unsigned wsum[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long nv = (long long)*nv_p;
    const long long lo = (long long)blockIdx.x * chunk;
    const long long hi = lo + chunk < nv ? lo + chunk : nv;
    unsigned base = counts[blockIdx.x];
    for (long long r = lo; r < hi; r += 256) {
        const long long v = r + tid;
        const unsigned mine = v < hi ? rows[v] : 0u;
        unsigned incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned pos = base + incl - mine;
        for (int w = 0; w < wave; ++w) pos += wsum[w];
        if (v < hi) rows[v] = pos;
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
}

extern "C" __global__ void __launch_bounds__(256) lfd_fuse_sums_kernel(const float* __restrict__ xyz, const float* __restrict__ normals,
                                                                      const float* __restrict__ rgb, long long n,
                                                                      const unsigned* __restrict__ sorted_idx, const unsigned* __restrict__ vstart,
                                                                      const unsigned* __restrict__ nv_p, const uint8_t* __restrict__ flag,
                                                                      const unsigned* __restrict__ rowstart, double cscale,
                                                                      float* __restrict__ xyz_out, float* __restrict__ normals_out,
                                                                      float* __restrict__ rgb_out, unsigned* __restrict__ count_out) {
    const long long nv = (long long)*nv_p;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (long long)gridDim.x * 256) {
        long long a, b;
        voxel_span(vstart, nv, n, v, a, b);
        if (b - a > LFD_VOX_BIG) continue;
        LfdFuseAcc s0, s1;
        lfd_fuse_clear(s0);
        lfd_fuse_clear(s1);
        for (long long j = a; j < b; ++j) {
            const long long i = sorted_idx[j];
            const unsigned f = flag[j];
            if (f & LFD_FUSE_SIDE) lfd_fuse_add(s1, xyz + 3 * i, normals + 3 * i, rgb + 3 * i, true, cscale);      // (side 1 implies usable)
            else lfd_fuse_add(s0, xyz + 3 * i, normals + 3 * i, rgb + 3 * i, (f & LFD_FUSE_USABLE) != 0u, cscale);
        }
        const long long r = rowstart[v];                       // r + 1 < n: a voxel of two rows holds at least two points
        lfd_fuse_emit(s0, xyz_out + 3 * r, normals_out + 3 * r, rgb_out + 3 * r);
        if (count_out) count_out[r] = s0.cnt;
        if (s1.cnt) {
            lfd_fuse_emit(s1, xyz_out + 3 * (r + 1), normals_out + 3 * (r + 1), rgb_out + 3 * (r + 1));
            if (count_out) count_out[r + 1] = s1.cnt;
        }
    }
}

extern "C" __global__ void __launch_bounds__(64) lfd_fuse_sums_big_kernel(const float* __restrict__ xyz, const float* __restrict__ normals,
                                                                         const float* __restrict__ rgb, long long n,
                                                                         const unsigned* __restrict__ sorted_idx, const unsigned* __restrict__ vstart,
                                                                         const unsigned* __restrict__ nv_p, const uint8_t* __restrict__ flag,
                                                                         const unsigned* __restrict__ rowstart, double cscale,
                                                                         const unsigned* __restrict__ big, const unsigned* __restrict__ n_big,
                                                                         float* __restrict__ xyz_out, float* __restrict__ normals_out,
                                                                         float* __restrict__ rgb_out, unsigned* __restrict__ count_out) {
    __shared__ double vals[9][257];          // (257: the nine components of one point fall into different LDS banks)
    __shared__ unsigned fl[256];
    const int lane = (int)threadIdx.x;
    const unsigned side = lane >= 9 ? 1u : 0u;
    const int comp = lane < 18 ? lane - 9 * (int)side : 0;
    const long long nv = (long long)*nv_p;
    const unsigned nb = *n_big;
    for (unsigned e = blockIdx.x; e < nb; e += gridDim.x) {
        const long long v = big[e];
        long long a, b;
        voxel_span(vstart, nv, n, v, a, b);
        double nxt[4][9] = {};
        unsigned nf[4] = {};
        auto load = [&](long long at) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long long j = at + 64 * u + lane;
                if (j < b) {
                    const long long i = sorted_idx[j];
                    nf[u] = flag[j];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        nxt[u][c] = (double)xyz[3 * i + c];
                        nxt[u][3 + c] = (double)rgb[3 * i + c] / cscale;
                        nxt[u][6 + c] = (double)normals[3 * i + c];
                    }
                }
            }
        };
        load(a);
        double acc = 0.0;
        unsigned cnt = 0u;
        for (long long at = a; at < b; at += 256) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int c = 0; c < 9; ++c) vals[c][64 * u + lane] = nxt[u][c];
                fl[64 * u + lane] = nf[u];
            }
            __syncthreads();
            if (at + 256 < b) load(at + 256);
            if (lane < 18) {
                const int m = b - at < 256 ? (int)(b - at) : 256;
                // a normal component takes the usable points of its side only (side 1 implies usable)
                const unsigned want = side | (comp >= 6 ? LFD_FUSE_USABLE : 0u), mask = LFD_FUSE_SIDE | (comp >= 6 ? LFD_FUSE_USABLE : 0u);
                for (int t = 0; t < m; ++t) {
                    const unsigned f = fl[t];
                    if ((f & LFD_FUSE_SIDE) == side) ++cnt;
                    if ((f & mask) == want) acc = acc + vals[comp][t];
                }
            }
            __syncthreads();
        }
        // lanes 9 s + 6 .. 9 s + 8 hold N of side s
        const int nb0 = 9 * (int)side + 6;
        const double N0 = __shfl(acc, nb0, 64), N1 = __shfl(acc, nb0 + 1, 64), N2 = __shfl(acc, nb0 + 2, 64);
        if (lane < 18 && cnt) {
            const long long r = (long long)rowstart[v] + side;
            if (comp < 6) {
                const float mean = (float)(acc / (double)cnt);
                if (comp < 3) xyz_out[3 * r + comp] = mean;
                else rgb_out[3 * r + comp - 3] = mean;
                if (comp == 0 && count_out) count_out[r] = cnt;
            } else {
                float u[3];
                lfd_fuse_unit(N0, N1, N2, u);
                normals_out[3 * r + comp - 6] = comp == 6 ? u[0] : (comp == 7 ? u[1] : u[2]);
            }
        }
    }
}
