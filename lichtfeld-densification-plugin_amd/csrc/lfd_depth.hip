// Depth and normal maps on the device (lfd_render_depth): every camera's view of the final cloud, with the cells dropped through which
// a farther surface shows (lfd_depth.hpp has the key, the keep test and both identities, shared with the twin).
//
// Steps of a batch of cameras, one launch each, nothing waits for another workgroup (lfd_api.hip's lfd_render_depth issues them):
//
//   lfd_depth_fill_kernel          every u64 word of the batch's planes becomes LFD_DEPTH_EMPTY, on every call
//   lfd_depth_splat_kernel         a lane per point in INPUT order walks the batch's cameras (a wave-uniform loop, the camera read through a uniform
//                                  index): per camera it is inside of, a plain read of the point's own cell (r = 0) and, unless the key there is already
//                                  smaller, one no-return 64-bit atomic minimum
//   lfd_depth_resolve_kernel       a workgroup per 32 x 16 tile of a camera's plane: the raw keys with a halo of R + r cells in LDS, a separable u64
//                                  minimum at radius r (the splat), a separable u32 minimum of the depth bits at radius R + r (the window), the keep
//                                  test, then depth, index and the winner's normal
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_device.hpp"
#include "lfd_depth.hpp"

#define LFD_DEPTH_TW 32                            // tile of the resolve kernel: a lane per column, 256 lanes = 8 rows at a time
#define LFD_DEPTH_TH 16
#define LFD_DEPTH_MAX_HALO (LFD_DEPTH_MAX_SPLAT + LFD_DEPTH_MAX_WINDOW)

extern "C" __global__ void __launch_bounds__(256) lfd_depth_fill_kernel(unsigned long long* __restrict__ keys, long long n_words) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (long long)gridDim.x * 256) keys[i] = LFD_DEPTH_EMPTY;
}

// cams: the batch's n_batch cameras; keys: its n_batch planes.  The word is read first and the atomic skipped when the stored key is already <= ours:
// a minimum only falls, so a stale read can cost an atomic that was not needed and never skips one that was - the bits are those of issuing every
// atomic.  The atomics execute at the memory side, a read that hits is served from the caches: the call is 2.9 .. 5.0 x as fast on the 14.6 M-point
// cloud (profiles/r24/depth.txt).
extern "C" __global__ void __launch_bounds__(256) lfd_depth_splat_kernel(const float* __restrict__ xyz, long long n,
                                                                        const LfdFreespaceCam* __restrict__ cams, int n_batch, int pw, int ph,
                                                                        unsigned long long* keys) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    const double dpw = (double)pw, dph = (double)ph;
    const long long plane = (long long)pw * ph;
    for (int c = 0; c < n_batch; ++c) {
        int cx, cy;
        float d;
        if (!lfd_freespace_project(cams[c], dpw, dph, x, y, z, cx, cy, d)) continue;
        // 0 <= cx < pw, 0 <= cy < ph (lfd_freespace_project clamps both): the word lies inside camera c's plane
        unsigned long long* word = keys + ((long long)c * plane + (long long)cy * pw + cx);
        const unsigned long long key = lfd_depth_key(d, (uint32_t)i);
        if (*word <= key) continue;
        atomicMin(word, key);
    }
}

// Workgroup b of tiles_x * tiles_y * n_batch: tile (b % tiles_x, (b / tiles_x) % tiles_y) of camera b / (tiles_x tiles_y) of the batch.  The three
// outputs start at the batch's first camera.  LDS: 38 x 54 keys, 22 x 32 row minima of keys, 38 x 32 row minima of depth bits = 26.3 KiB.
extern "C" __global__ void __launch_bounds__(256) lfd_depth_resolve_kernel(const unsigned long long* __restrict__ keys, int pw, int ph, int tiles_x,
                                                                          int tiles_y, int r, int R, float tol, const float* __restrict__ normals,
                                                                          float* __restrict__ depth_out, int* __restrict__ index_out,
                                                                          float* __restrict__ normal_out) {
    __shared__ unsigned long long raw[(LFD_DEPTH_TH + 2 * LFD_DEPTH_MAX_HALO) * (LFD_DEPTH_TW + 2 * LFD_DEPTH_MAX_HALO)];
    __shared__ unsigned long long row_key[(LFD_DEPTH_TH + 2 * LFD_DEPTH_MAX_SPLAT) * LFD_DEPTH_TW];
    __shared__ unsigned row_bits[(LFD_DEPTH_TH + 2 * LFD_DEPTH_MAX_HALO) * LFD_DEPTH_TW];
    const int tid = (int)threadIdx.x;
    const int H = R + r;                                               // <= 11 (lfd_depth_check)
    const int RW = LFD_DEPTH_TW + 2 * H, RH = LFD_DEPTH_TH + 2 * H;    // the tile with its halo
    long long b = (long long)blockIdx.x;
    const int tx = (int)(b % tiles_x);
    b /= tiles_x;
    const int ty = (int)(b % tiles_y);
    const long long cam = b / tiles_y;
    const int x0 = tx * LFD_DEPTH_TW, y0 = ty * LFD_DEPTH_TH;
    const long long cells = (long long)pw * ph;
    const unsigned long long* plane = keys + cam * cells;

    for (int e = tid; e < RW * RH; e += 256) {                         // halo cells outside the plane are empty
        const int ly = e / RW, lx = e - ly * RW;
        const int gx = x0 - H + lx, gy = y0 - H + ly;
        raw[e] = (gx >= 0 && gx < pw && gy >= 0 && gy < ph) ? plane[(long long)gy * pw + gx] : LFD_DEPTH_EMPTY;
    }
    __syncthreads();
    for (int e = tid; e < RH * LFD_DEPTH_TW; e += 256) {               // along the rows: tile column lx is raw column lx + H
        const int ly = e / LFD_DEPTH_TW, lx = e % LFD_DEPTH_TW;
        const unsigned long long* row = raw + ly * RW + lx;
        unsigned m = LFD_FREESPACE_EMPTY;
        for (int k = 0; k <= 2 * H; ++k) {
            const unsigned bits = lfd_depth_key_bits(row[k]);
            m = bits < m ? bits : m;
        }
        row_bits[e] = m;
        if (ly >= R && ly < RH - R) {                                  // the TH + 2 r rows the splat reads
            unsigned long long a = LFD_DEPTH_EMPTY;
            for (int k = 0; k <= 2 * r; ++k) {
                const unsigned long long v = row[R + k];
                a = v < a ? v : a;
            }
            row_key[(ly - R) * LFD_DEPTH_TW + lx] = a;
        }
    }
    __syncthreads();
    for (int e = tid; e < LFD_DEPTH_TH * LFD_DEPTH_TW; e += 256) {     // down the columns: tile row ly is row ly + r of row_key, ly + H of row_bits
        const int ly = e / LFD_DEPTH_TW, lx = e % LFD_DEPTH_TW;
        const int gx = x0 + lx, gy = y0 + ly;
        if (gx >= pw || gy >= ph) continue;
        unsigned long long K = LFD_DEPTH_EMPTY;
        for (int k = 0; k <= 2 * r; ++k) {
            const unsigned long long v = row_key[(ly + k) * LFD_DEPTH_TW + lx];
            K = v < K ? v : K;
        }
        unsigned m = LFD_FREESPACE_EMPTY;
        for (int k = 0; k <= 2 * H; ++k) {
            const unsigned v = row_bits[(ly + k) * LFD_DEPTH_TW + lx];
            m = v < m ? v : m;
        }
        const unsigned dbits = lfd_depth_key_bits(K);
        const bool keep = !lfd_depth_key_empty(K) && lfd_depth_keep(dbits, m, tol);
        const long long o = cam * cells + (long long)gy * pw + gx;
        depth_out[o] = keep ? __uint_as_float(dbits) : 0.0f;
        const int idx = keep ? (int)lfd_depth_key_index(K) : -1;
        if (index_out) index_out[o] = idx;
        if (normal_out) {
            float nx = 0.0f, ny = 0.0f, nz = 0.0f;
            if (keep) {
                nx = normals[3 * (long long)idx];
                ny = normals[3 * (long long)idx + 1];
                nz = normals[3 * (long long)idx + 2];
            }
            normal_out[3 * o] = nx;
            normal_out[3 * o + 1] = ny;
            normal_out[3 * o + 2] = nz;
        }
    }
}
