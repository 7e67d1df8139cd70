// Local correlation of RoMa-v2's conv refiners on the device (lfd_local_corr):
//
//   out[b, n, k] = sum_c A[b, n, c] * bilinear(Bf[b, :, :, c]; warp[b, n, k])
//
// One launch, no atomics, nothing crosses a workgroup; the summation order depends on the shape alone, so equal inputs give equal bits.
//
//   lfd_corr_vec_kernel<G, CPL>  the fast layout (channels adjacent, C % 4 == 0).  G adjacent lanes own one query pixel (b, n): its A row stays
//                                in registers (CPL float4 per lane), the K coordinates are read G at a time (one per lane, coalesced) and
//                                handed round with a shuffle, and for every sample each lane reads its 16-byte pieces of the four texels -
//                                G lanes x 16 B = one contiguous run per texel - into four running sums; each is added over the G lanes by
//                                a xor butterfly (DPP inside a row of 16) and the four totals are blended.  Lane j keeps the result of
//                                sample k0 + j: the store is coalesced as well.  Where the K samples of a pixel form a lattice of texels
//                                (the model's window) every shared texel is multiplied once instead (see the kernel).
//   lfd_corr_any_kernel          any strides, any C: a lane per output element through lfd_corr_sample, the twin's own routine.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lfd_corr.hpp"

#define LFD_CORR_MAX_SIDE 7          // the lattice form serves windows of up to 7 x 7 samples: (7 + 1)^2 = 64 texel sums per query pixel

// Workgroups are handed to the 8 XCDs (each with an L2 of its own) round-robin.  This gives every XCD one contiguous run of the query
// pixels - a band of image rows, whose neighbourhood in Bf is an eighth of the map and fits its L2 - instead of every eighth workgroup of
// the whole image.  Bijective for any grid size; a choice of speed alone.
__device__ __forceinline__ unsigned lfd_corr_block() {
    const unsigned nwg = gridDim.x, orig = blockIdx.x, xcd = orig % 8u, q = nwg / 8u, r = nwg % 8u;
    return (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + orig / 8u;
}

template <int G>
__device__ __forceinline__ float lfd_corr_group_sum(float s) {
#pragma unroll
    for (int off = G >> 1; off > 0; off >>= 1) s += __shfl_xor(s, off, G);
    return s;
}

// running sums of one 16-byte piece of A against the same piece of four texels
__device__ __forceinline__ void lfd_corr_piece(const float4 av, const float* t0, const float* t1, const float* t2, const float* t3, int ch, float& s0,
                                               float& s1, float& s2, float& s3) {
    const float4 v0 = reinterpret_cast<const float4*>(t0)[ch], v1 = reinterpret_cast<const float4*>(t1)[ch];
    const float4 v2 = reinterpret_cast<const float4*>(t2)[ch], v3 = reinterpret_cast<const float4*>(t3)[ch];
    s0 = __builtin_fmaf(av.w, v0.w, __builtin_fmaf(av.z, v0.z, __builtin_fmaf(av.y, v0.y, __builtin_fmaf(av.x, v0.x, s0))));
    s1 = __builtin_fmaf(av.w, v1.w, __builtin_fmaf(av.z, v1.z, __builtin_fmaf(av.y, v1.y, __builtin_fmaf(av.x, v1.x, s1))));
    s2 = __builtin_fmaf(av.w, v2.w, __builtin_fmaf(av.z, v2.z, __builtin_fmaf(av.y, v2.y, __builtin_fmaf(av.x, v2.x, s2))));
    s3 = __builtin_fmaf(av.w, v3.w, __builtin_fmaf(av.z, v3.z, __builtin_fmaf(av.y, v3.y, __builtin_fmaf(av.x, v3.x, s3))));
}

// `side` > 0: K = side^2 and the caller allows the lattice form.  It is taken per query pixel, when the DATA say so: every one of its K
// samples touches the map and the floor of sample (ky, kx)'s position is that of sample (0, 0) plus (ky, kx) - what the model's window at
// one-texel spacing gives away from the border.  The (side + 1)^2 texels the samples share are then multiplied with the A row ONCE each
// (instead of 4 K times), the sums parked in LDS, and every sample blends its four with its OWN weights.  Any other pixel takes the
// general loop, which performs the same operations on every texel sum: the form never shows in the bits.
template <int G, int CPL>
__global__ void __launch_bounds__(256) lfd_corr_vec_kernel(const LfdCorrArgs p, const int side) {
    __shared__ float sums[256 / G][(LFD_CORR_MAX_SIDE + 1) * (LFD_CORR_MAX_SIDE + 1)];
    const int lane_g = (int)threadIdx.x % G, group = (int)threadIdx.x / G;
    const long long pixel = ((long long)lfd_corr_block() * 256 + threadIdx.x) / G;     // (b, n), the same for the G lanes of a group
    const bool active = pixel < (long long)p.B * p.N;
    const long long px = active ? pixel : 0;                                          // idle groups compute on pixel 0 and store nothing
    const int b = (int)(px / p.N), n = (int)(px - (long long)b * p.N);
    const int C4 = p.C >> 2;
    const float4* a4 = reinterpret_cast<const float4*>(p.a + b * p.sa_b + n * p.sa_n);
    const float* bf = p.bf + b * p.sb_b;
    const float2* warp = reinterpret_cast<const float2*>(p.warp) + px * p.K;
    float* out = p.out + px * p.K;

    float4 a[CPL > 0 ? CPL : 1];
    if (CPL > 0) {
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int ch = lane_g + i * G;
            a[i] = ch < C4 ? a4[ch] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
    auto dots = [&](const float* t0, const float* t1, const float* t2, const float* t3, float& s0, float& s1, float& s2, float& s3) {
        s0 = s1 = s2 = s3 = 0.0f;
        if (CPL > 0) {
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                const int ch = lane_g + i * G;
                if (ch < C4) lfd_corr_piece(a[i], t0, t1, t2, t3, ch, s0, s1, s2, s3);
            }
        } else {
            for (int ch = lane_g; ch < C4; ch += G) lfd_corr_piece(a4[ch], t0, t1, t2, t3, ch, s0, s1, s2, s3);
        }
    };

    // ---- is this pixel's window a lattice of texels? ----------------------------------------------------------------------------------
    int bx = 0, by = 0;
    bool lattice = false;
    if (side > 0) {                                                                    // (uniform over the launch)
        int ok = 1;
        for (int k0 = 0; k0 < p.K; k0 += G) {
            const int kk = k0 + lane_g < p.K ? k0 + lane_g : p.K - 1;
            const float2 xy = warp[kk];
            LfdCorrTaps t;
            const bool inside = lfd_corr_taps(xy.x, xy.y, p.W1, p.H1, t);
            if (k0 == 0) { bx = __shfl(t.x0, 0, G); by = __shfl(t.y0, 0, G); }
            const int ky = kk / side, kx = kk - ky * side;
            ok &= (inside && t.x0 == bx + kx && t.y0 == by + ky) ? 1 : 0;
        }
#pragma unroll
        for (int off = G >> 1; off > 0; off >>= 1) ok &= __shfl_xor(ok, off, G);
        lattice = ok != 0;
    }

    if (lattice) {
        // the (side + 1)^2 shared texels, four of a row at a time; texel (ty, tx) is (by + ty, bx + tx), possibly one step outside the map
        const int tw = side + 1;
        for (int ty = 0; ty < tw; ++ty) {
            const int y = by + ty;
            const bool ly = y >= 0 && y < p.H1;
            const float* row = bf + (ly ? y : 0) * p.sb_y;
            for (int tx = 0; tx < tw; tx += 4) {
                const float* tp[4];
                bool live[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int x = bx + tx + q;
                    live[q] = ly && tx + q < tw && x >= 0 && x < p.W1;
                    tp[q] = row + (live[q] ? x : 0) * p.sb_x;
                }
                float s[4];
                dots(tp[0], tp[1], tp[2], tp[3], s[0], s[1], s[2], s[3]);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float d = lfd_corr_group_sum<G>(s[q]);
                    if (lane_g == (q % G) && tx + q < tw) sums[group][ty * tw + tx + q] = live[q] ? d : 0.0f;
                }
            }
        }
    }
    __syncthreads();
    if (lattice) {
        if (active) {
            const int tw = side + 1;
            for (int kk = lane_g; kk < p.K; kk += G) {
                const float2 xy = warp[kk];
                LfdCorrTaps t;
                lfd_corr_taps(xy.x, xy.y, p.W1, p.H1, t);
                const int at = (t.y0 - by) * tw + (t.x0 - bx);                        // in [0, tw * tw - tw - 2] by the test above
                const float* d = &sums[group][at < 0 ? 0 : (at > tw * tw - tw - 2 ? tw * tw - tw - 2 : at)];
                const float s = (t.live[0] ? t.w[0] * d[0] : 0.0f) + (t.live[1] ? t.w[1] * d[1] : 0.0f);
                out[kk] = s + ((t.live[2] ? t.w[2] * d[tw] : 0.0f) + (t.live[3] ? t.w[3] * d[tw + 1] : 0.0f));
            }
        }
        return;
    }

    // ---- the general loop: the K coordinates G at a time, one per lane, handed round with a shuffle -------------------------------------
    for (int k0 = 0; k0 < p.K; k0 += G) {
        const int kk = k0 + lane_g;
        const float2 xy = kk < p.K ? warp[kk] : make_float2(0.0f, 0.0f);
        const int jn = p.K - k0 < G ? p.K - k0 : G;
        float mine = 0.0f;
        for (int j = 0; j < jn; ++j) {
            const float x = __shfl(xy.x, j, G), y = __shfl(xy.y, j, G);
            LfdCorrTaps t;
            lfd_corr_taps(x, y, p.W1, p.H1, t);                       // outside / non-finite: four dead taps on texel 0
            float s0, s1, s2, s3;
            dots(bf + t.y[0] * p.sb_y + t.x[0] * p.sb_x, bf + t.y[0] * p.sb_y + t.x[1] * p.sb_x, bf + t.y[1] * p.sb_y + t.x[0] * p.sb_x,
                 bf + t.y[1] * p.sb_y + t.x[1] * p.sb_x, s0, s1, s2, s3);
            // each texel's sum over the group first, then the blend: the very operations of the lattice form, so which form a pixel takes
            // never shows in its bits.  A dead texel's sum is dropped, not multiplied by 0: whatever the clamped address held stays out
            const float d0 = lfd_corr_group_sum<G>(s0), d1 = lfd_corr_group_sum<G>(s1), d2 = lfd_corr_group_sum<G>(s2), d3 = lfd_corr_group_sum<G>(s3);
            float s = (t.live[0] ? t.w[0] * d0 : 0.0f) + (t.live[1] ? t.w[1] * d1 : 0.0f);
            s = s + ((t.live[2] ? t.w[2] * d2 : 0.0f) + (t.live[3] ? t.w[3] * d3 : 0.0f));
            if (lane_g == j) mine = s;
        }
        if (active && kk < p.K) out[kk] = mine;
    }
}

__global__ void __launch_bounds__(256) lfd_corr_any_kernel(const LfdCorrArgs p) {
    const long long total = (long long)p.B * p.N * p.K;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long pixel = e / p.K;
        const int b = (int)(pixel / p.N), n = (int)(pixel - (long long)b * p.N);
        const float x = p.warp[2 * e], y = p.warp[2 * e + 1];
        p.out[e] = lfd_corr_sample(p.a + b * p.sa_b + n * p.sa_n, p.sa_c, p.bf + b * p.sb_b, p.sb_y, p.sb_x, p.sb_c, p.C, p.W1, p.H1, x, y);
    }
}

// lfd_api.hip's lfd_local_corr: the arguments were validated there
hipError_t lfd_corr_launch(const LfdCorrArgs& p, hipStream_t stream) {
    const long long pixels = (long long)p.B * p.N;
    if (lfd_corr_vector_layout(p)) {
        const int C4 = p.C >> 2;
        const int G = C4 >= 16 ? 16 : 4;
        const int cpl = (C4 + G - 1) / G;
        const unsigned grid = (unsigned)((pixels * G + 255) / 256);
        int side = 0;                                          // K a square of at most 7 x 7: the kernel may take the lattice form
        for (int s = 1; s <= LFD_CORR_MAX_SIDE; ++s) if (s * s == p.K) side = s;
        if (G == 16) {
            if (cpl <= 3) hipLaunchKernelGGL((lfd_corr_vec_kernel<16, 3>), dim3(grid), dim3(256), 0, stream, p, side);
            else hipLaunchKernelGGL((lfd_corr_vec_kernel<16, 0>), dim3(grid), dim3(256), 0, stream, p, side);
        } else {
            if (cpl <= 3) hipLaunchKernelGGL((lfd_corr_vec_kernel<4, 3>), dim3(grid), dim3(256), 0, stream, p, side);
            else hipLaunchKernelGGL((lfd_corr_vec_kernel<4, 0>), dim3(grid), dim3(256), 0, stream, p, side);
        }
    } else {
        const long long total = pixels * p.K;
        const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, 65536);
        hipLaunchKernelGGL(lfd_corr_any_kernel, dim3(grid), dim3(256), 0, stream, p);
    }
    return hipGetLastError();
}
