// The GUI's distance filter on the device (lfd_voxel_downsample): one averaged point per occupied voxel, bit for bit and in the same order
// as the NumPy branch of densify._voxel_downsample.
//
//   origin_c = (f64) min_c - 0.5 * voxel_size                     (the host computes it from lfd_voxel_final_kernel's statistics)
//   key_c    = floor(((f64) x_c - origin_c) / voxel_size)         IEEE f64 subtract and divide (no reciprocal: -fno-fast-math)
//   order    = np.unique(axis=0) = lexicographic (k0, k1, k2)    = ascending k0 E1 E2 + k1 E2 + k2, E_c = max key_c + 1
//   sums     = np.add.at: per voxel, f64 from 0.0 over its points in ascending original index
//
// Phases (one launch each, no inter-workgroup waits): min / max -> keys -> per significant 8-bit digit a stable LSD pass (histogram, scan,
// scatter) of (linear key, original index) -> voxel heads (count, scan, scatter) -> sums.  A stable sort keeps equal keys in ascending
// original index, so the sums below run in np.add.at's order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_device.hpp"

namespace {

__device__ __forceinline__ void stats_merge(LfdVoxStats& a, const LfdVoxStats& b) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { a.lo[c] = fminf(a.lo[c], b.lo[c]); a.hi[c] = fmaxf(a.hi[c], b.hi[c]); }
    a.cmax = fmaxf(a.cmax, b.cmax);
    a.flags |= b.flags;
}

__device__ __forceinline__ LfdVoxStats stats_empty() {
    LfdVoxStats s;
#pragma unroll
    for (int c = 0; c < 3; ++c) { s.lo[c] = __builtin_inff(); s.hi[c] = -__builtin_inff(); }
    s.cmax = -__builtin_inff();
    s.flags = 0u;
    return s;
}

// LDS tree reduction of one LfdVoxStats per thread (256 threads)
__device__ __forceinline__ void stats_block_reduce(LfdVoxStats s, LfdVoxStats* sh, LfdVoxStats* out) {
    const int tid = (int)threadIdx.x;
    sh[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) stats_merge(sh[tid], sh[tid + w]);
        __syncthreads();
    }
    if (tid == 0) *out = sh[0];
}

}  // namespace

// min / max of the coordinates, non-finite flag, colour max + NaN flag: one LfdVoxStats per workgroup
extern "C" __global__ void __launch_bounds__(256) lfd_voxel_minmax_kernel(const float* __restrict__ xyz, const float* __restrict__ rgb, long long n,
                                                                         LfdVoxStats* __restrict__ part) {
    __shared__ LfdVoxStats sh[256];
    LfdVoxStats s = stats_empty();
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float x = xyz[3 * i + c], col = rgb[3 * i + c];
            if (__builtin_isfinite(x)) { s.lo[c] = fminf(s.lo[c], x); s.hi[c] = fmaxf(s.hi[c], x); }
            else s.flags |= LFD_VOX_NONFINITE;
            if (__builtin_isnan(col)) s.flags |= LFD_VOX_NAN_RGB;
            else s.cmax = fmaxf(s.cmax, col);
        }
    }
    stats_block_reduce(s, sh, part + blockIdx.x);
}

extern "C" __global__ void __launch_bounds__(256) lfd_voxel_final_kernel(const LfdVoxStats* __restrict__ part, int n_part, LfdVoxStats* __restrict__ out) {
    __shared__ LfdVoxStats sh[256];
    LfdVoxStats s = stats_empty();
    for (int i = (int)threadIdx.x; i < n_part; i += 256) stats_merge(s, part[i]);
    stats_block_reduce(s, sh, out);
}

// linear key of every point (the caller checked that the largest one fits 63 bits) and the identity payload
extern "C" __global__ void __launch_bounds__(256) lfd_voxel_keys_kernel(const float* __restrict__ xyz, long long n, double o0, double o1, double o2,
                                                                       double vs, unsigned long long e1, unsigned long long e2,
                                                                       unsigned long long* __restrict__ keys, unsigned* __restrict__ idx) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double k0 = floor(((double)xyz[3 * i] - o0) / vs);
        const double k1 = floor(((double)xyz[3 * i + 1] - o1) / vs);
        const double k2 = floor(((double)xyz[3 * i + 2] - o2) / vs);
        keys[i] = ((unsigned long long)k0 * e1 + (unsigned long long)k1) * e2 + (unsigned long long)k2;
        idx[i] = (unsigned)i;
    }
}

// ---- stable LSD radix pass: histogram -> scan -> scatter ------------------------------------------------------------------------------------
// Workgroup b owns the contiguous items [b * chunk, min(n, (b + 1) * chunk)).  counts[d * G + b] = items of digit d in workgroup b, so the
// exclusive scan of the whole table (digit-major) is where workgroup b's items of digit d start in the output.
extern "C" __global__ void __launch_bounds__(256) lfd_voxel_hist_kernel(const unsigned long long* __restrict__ keys, long long n, long long chunk,
                                                                       int shift, unsigned* __restrict__ counts) {
    __shared__ unsigned h[256];
    const int tid = (int)threadIdx.x;
    h[tid] = 0u;
    __syncthreads();
    const long long lo = (long long)blockIdx.x * chunk;
    const long long hi = lo + chunk < n ? lo + chunk : n;
    for (long long i = lo + tid; i < hi; i += 256) atomicAdd(&h[(unsigned)(keys[i] >> shift) & 255u], 1u);
    __syncthreads();
    counts[(long long)tid * gridDim.x + blockIdx.x] = h[tid];
}

// exclusive prefix of v[0 .. m) in place, one workgroup; the total goes to *total (may be null)
extern "C" __global__ void __launch_bounds__(1024) lfd_voxel_scan_kernel(unsigned* __restrict__ v, int m, unsigned* __restrict__ total) {
    __shared__ unsigned wave_sum[16];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (m + 1023) / 1024;
    const int a = tid * per < m ? tid * per : m;
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
    if (tid == 1023 && total) *total = run + sum;
    for (int i = a; i < b; ++i) {
        const unsigned c = v[i];
        v[i] = run;
        run += c;
    }
}

// rank of this lane among the active lanes of its wave that hold the same 8-bit digit, and how many they are
__device__ __forceinline__ void wave_match8(unsigned d, bool valid, int lane, unsigned* rank, unsigned* cnt) {
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
        const unsigned long long m = __ballot(((d >> bit) & 1u) != 0u);
        peers &= ((d >> bit) & 1u) ? m : ~m;
    }
    *rank = (unsigned)__popcll(peers & ((1ull << lane) - 1ull));
    *cnt = (unsigned)__popcll(peers);
}

// stable scatter: the workgroup walks its items in rounds of 512 in order; within a round an item's place is its digit's running base,
// plus the items of that digit in the waves before its own, plus its rank within its wave
extern "C" __global__ void __launch_bounds__(512) lfd_voxel_scatter_kernel(const unsigned long long* __restrict__ kin, const unsigned* __restrict__ iin,
                                                                          long long n, long long chunk, int shift, const unsigned* __restrict__ counts,
                                                                          unsigned long long* __restrict__ kout, unsigned* __restrict__ iout) {
    __shared__ unsigned base[256];
    __shared__ unsigned wh[8][256];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 256) {
        base[tid] = counts[(long long)tid * gridDim.x + blockIdx.x];
#pragma unroll
        for (int w = 0; w < 8; ++w) wh[w][tid] = 0u;
    }
    __syncthreads();
    const long long lo = (long long)blockIdx.x * chunk;
    const long long hi = lo + chunk < n ? lo + chunk : n;
    for (long long r = lo; r < hi; r += 512) {
        const long long i = r + tid;
        const bool valid = i < hi;
        const unsigned long long k = valid ? kin[i] : 0ull;
        const unsigned p = valid ? iin[i] : 0u;
        const unsigned d = (unsigned)(k >> shift) & 255u;
        unsigned rank, cnt;
        wave_match8(d, valid, lane, &rank, &cnt);
        if (valid && rank == 0u) wh[wave][d] = cnt;
        __syncthreads();
        if (valid) {
            unsigned pos = base[d] + rank;
            for (int w = 0; w < wave; ++w) pos += wh[w][d];
            kout[pos] = k;
            iout[pos] = p;
        }
        __syncthreads();
        if (tid < 256) {
            unsigned add = 0u;
#pragma unroll
            for (int w = 0; w < 8; ++w) { add += wh[w][tid]; wh[w][tid] = 0u; }
            base[tid] += add;
        }
        __syncthreads();
    }
}

// ---- voxel heads: sorted position j starts a voxel when j == 0 or its key differs from j - 1's ------------------------------------------------
extern "C" __global__ void __launch_bounds__(256) lfd_voxel_head_count_kernel(const unsigned long long* __restrict__ keys, long long n, long long chunk,
                                                                             unsigned* __restrict__ counts) {
    __shared__ unsigned c;
    if (threadIdx.x == 0) c = 0u;
    __syncthreads();
    const long long lo = (long long)blockIdx.x * chunk;
    const long long hi = lo + chunk < n ? lo + chunk : n;
    unsigned mine = 0u;
    for (long long j = lo + threadIdx.x; j < hi; j += 256) mine += (j == 0 || keys[j] != keys[j - 1]) ? 1u : 0u;
    atomicAdd(&c, mine);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// vstart[v] = first sorted position of voxel v (voxels in key order)
extern "C" __global__ void __launch_bounds__(512) lfd_voxel_head_scatter_kernel(const unsigned long long* __restrict__ keys, long long n, long long chunk,
                                                                               const unsigned* __restrict__ counts, unsigned* __restrict__ vstart) {
    __shared__ unsigned wc[8];
    __shared__ unsigned base;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) base = counts[blockIdx.x];
    __syncthreads();
    const long long lo = (long long)blockIdx.x * chunk;
    const long long hi = lo + chunk < n ? lo + chunk : n;
    for (long long r = lo; r < hi; r += 512) {
        const long long j = r + tid;
        const bool head = j < hi && (j == 0 || keys[j] != keys[j - 1]);
        const unsigned long long m = __ballot(head);
        if (lane == 0) wc[wave] = (unsigned)__popcll(m);
        __syncthreads();
        if (head) {
            unsigned pos = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
            for (int w = 0; w < wave; ++w) pos += wc[w];
            vstart[pos] = (unsigned)j;
        }
        __syncthreads();
        if (tid == 0) {
            unsigned add = 0u;
#pragma unroll
            for (int w = 0; w < 8; ++w) add += wc[w];
            base += add;
        }
        __syncthreads();
    }
}

// ---- sums: np.add.at's sequential f64 order, then mean = sum / count rounded to f32 ----------------------------------------------------------
// A thread per voxel of at most LFD_VOX_BIG points; larger voxels are listed for lfd_voxel_sums_big_kernel.
extern "C" __global__ void __launch_bounds__(256) lfd_voxel_sums_kernel(const float* __restrict__ xyz, const float* __restrict__ rgb, long long n,
                                                                       const unsigned* __restrict__ sorted_idx, const unsigned* __restrict__ vstart,
                                                                       const unsigned* __restrict__ nv_p, double cscale, float* __restrict__ xyz_out,
                                                                       float* __restrict__ rgb_out, unsigned* __restrict__ big, unsigned* __restrict__ n_big) {
    const long long nv = (long long)*nv_p;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (long long)gridDim.x * 256) {
        const long long a = vstart[v];
        const long long b = v + 1 < nv ? (long long)vstart[v + 1] : n;
        if (b - a > LFD_VOX_BIG) {
            big[atomicAdd(n_big, 1u)] = (unsigned)v;
            continue;
        }
        double p0 = 0.0, p1 = 0.0, p2 = 0.0, c0 = 0.0, c1 = 0.0, c2 = 0.0;
        for (long long j = a; j < b; ++j) {
            const long long i = sorted_idx[j];
            p0 += (double)xyz[3 * i]; p1 += (double)xyz[3 * i + 1]; p2 += (double)xyz[3 * i + 2];
            c0 += (double)rgb[3 * i] / cscale; c1 += (double)rgb[3 * i + 1] / cscale; c2 += (double)rgb[3 * i + 2] / cscale;
        }
        const double cnt = (double)(b - a);
        xyz_out[3 * v] = (float)(p0 / cnt); xyz_out[3 * v + 1] = (float)(p1 / cnt); xyz_out[3 * v + 2] = (float)(p2 / cnt);
        rgb_out[3 * v] = (float)(c0 / cnt); rgb_out[3 * v + 1] = (float)(c1 / cnt); rgb_out[3 * v + 2] = (float)(c2 / cnt);
    }
}

// a wave (= workgroup) per listed voxel: 256 points at a time are loaded by all lanes (the next 256 while the current ones are summed) and
// staged in LDS; lanes 0..5 then add one component each, in point order
extern "C" __global__ void __launch_bounds__(64) lfd_voxel_sums_big_kernel(const float* __restrict__ xyz, const float* __restrict__ rgb, long long n,
                                                                          const unsigned* __restrict__ sorted_idx, const unsigned* __restrict__ vstart,
                                                                          const unsigned* __restrict__ nv_p, double cscale, const unsigned* __restrict__ big,
                                                                          const unsigned* __restrict__ n_big, float* __restrict__ xyz_out,
                                                                          float* __restrict__ rgb_out) {
    __shared__ double vals[6][256];
    const int lane = (int)threadIdx.x;
    const long long nv = (long long)*nv_p;
    const unsigned nb = *n_big;
    for (unsigned e = blockIdx.x; e < nb; e += gridDim.x) {
        const long long v = big[e];
        const long long a = vstart[v];
        const long long b = v + 1 < nv ? (long long)vstart[v + 1] : n;
        double nxt[4][6] = {};
        auto load = [&](long long at) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long long j = at + 64 * u + lane;
                if (j < b) {
                    const long long i = sorted_idx[j];
#pragma unroll
                    for (int c = 0; c < 3; ++c) { nxt[u][c] = (double)xyz[3 * i + c]; nxt[u][3 + c] = (double)rgb[3 * i + c] / cscale; }
                }
            }
        };
        load(a);
        double acc = 0.0;
        for (long long at = a; at < b; at += 256) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int c = 0; c < 6; ++c) vals[c][64 * u + lane] = nxt[u][c];
            __syncthreads();
            if (at + 256 < b) load(at + 256);
            if (lane < 6) {
                const int m = b - at < 256 ? (int)(b - at) : 256;
                for (int t = 0; t < m; ++t) acc += vals[lane][t];
            }
            __syncthreads();
        }
        const double mean = acc / (double)(b - a);
        if (lane < 3) xyz_out[3 * v + lane] = (float)mean;
        else if (lane < 6) rgb_out[3 * v + lane - 3] = (float)mean;
    }
}
