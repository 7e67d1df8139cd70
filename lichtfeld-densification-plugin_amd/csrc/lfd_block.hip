// One conv block of RoMa-v2's refiners on the device (lfd_refiner_block): depthwise 5x5 -> folded BatchNorm -> ReLU (-> 1x1 for the
// width-32 refiner) in ONE launch, one read and one write of the activation.  The arithmetic is lfd_block.hpp's, in its order: same bits as the twin.
//
// Both kernels work on tiles of 64 x 16 output pixels: lane l of wave v owns column l and the rows R v .. R v + R - 1 (R = 4 and 256 threads in
// the general kernel, R = 2 and 512 threads in the width-32 one, whose lanes keep 32 accumulators per output).  The
// tile and its two-pixel halo (20 x 68 values, already widened to f32) are staged in LDS; a lane walks the R + 4 staged rows its outputs
// touch once, top to bottom, and feeds every row to the outputs it belongs to - each output still sees its taps in the order ky, kx.  The
// channel is the same for the whole workgroup, so the 25 weights, s, t and the row of Wt are read with scalar loads.
//
//   lfd_block_dw_kernel   any C, no pointwise part: a workgroup owns one tile of one (b, c) plane.
//   lfd_block_pw_kernel   C == 32 with the pointwise part: a workgroup owns one tile of ALL 32 planes of an image and walks them in order;
//                         plane c + 1 travels global -> registers -> the other LDS buffer while plane c is computed, and the hidden value of
//                         plane c goes into the lane's 2 x 32 accumulators at once (z[o] = fmaf(Wt[c][o], h[c], z[o]), c ascending).
//
// A tile whose halo lies inside the plane takes the loop without the inside tests; a tap outside the plane is skipped, never multiplied by 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lfd_block.hpp"

#define LFD_BLOCK_TX 64
#define LFD_BLOCK_TY 16
#define LFD_BLOCK_LY (LFD_BLOCK_TY + 2 * LFD_BLOCK_R)        // 20 staged rows
#define LFD_BLOCK_LX (LFD_BLOCK_TX + 2 * LFD_BLOCK_R)        // 68 staged columns
#define LFD_BLOCK_DW_ROWS 4                                  // outputs per lane of the general kernel: 256 threads
#define LFD_BLOCK_PW_ROWS 2                                  // ... of the width-32 kernel, which keeps 32 accumulators per output: 512 threads
#define LFD_BLOCK_GRID_Y 65535u                              // planes (or images) per z slice of the grid

#define LFD_BLOCK_TILE 1536                                  // LDS words of a staged tile: 20 x 68 = 1360 rounded up to 6 x 256 = 3 x 512, one write per
                                                             // thread and step without a test

// PIN (code inside a loop): the value as it is, but opaque to the optimiser from here on (no instruction is emitted): a per-lane test of it is
// then evaluated where it stands instead of being hoisted out of the loop as a 64-bit lane mask that occupies two scalar registers throughout.
template <bool PIN>
__device__ __forceinline__ int lfd_block_opaque(int v) {
    if (PIN) asm volatile("" : "+v"(v));
    return v;
}

typedef float LfdBlockTile[LFD_BLOCK_TILE];                  // value (r, q) of the staged tile at r * 68 + q

// Staging, in three steps so that the loads of the next plane can be in flight while this one is computed and nothing about them has to be kept
// in scalar registers meanwhile.  lfd_block_offsets: for the words i = tid, tid + NT, ... of the staged tile, whose corner (row 0, column 0) is
// pixel (y0 - 2, x0 - 2), the element offset inside a plane, or -1 for a word outside the plane or beyond the 20 x 68 values.
// lfd_block_fetch: the raw input words of the plane at element `plane`; a word without an offset reads the plane's first element, so every
// load is inside the input.  lfd_block_park: the words widened (an f32 input rounded to bf16 first) and written to LDS, 0 where there is no
// offset - such a word is never used as a tap.
template <int NT>
__device__ __forceinline__ void lfd_block_offsets(int y0, int x0, int H, int W, int off[LFD_BLOCK_TILE / NT]) {
#pragma unroll
    for (int k = 0; k < LFD_BLOCK_TILE / NT; ++k) {
        const int i = (int)threadIdx.x + NT * k;
        const int r = i / LFD_BLOCK_LX, q = i - r * LFD_BLOCK_LX;
        const int gy = y0 - LFD_BLOCK_R + r, gx = x0 - LFD_BLOCK_R + q;
        off[k] = (r < LFD_BLOCK_LY && gy >= 0 && gy < H && gx >= 0 && gx < W) ? (int)((unsigned)gy * (unsigned)W + (unsigned)gx) : -1;           // < H W <= 2^31 - 1
    }
}

template <int NT, bool F32, bool PIN>
__device__ __forceinline__ void lfd_block_fetch(const void* x, int64_t plane, const int off[LFD_BLOCK_TILE / NT], uint32_t v[LFD_BLOCK_TILE / NT]) {
#pragma unroll
    for (int k = 0; k < LFD_BLOCK_TILE / NT; ++k) {
        const int o = lfd_block_opaque<PIN>(off[k]);
        const int64_t at = plane + (o < 0 ? 0 : o);
        v[k] = F32 ? static_cast<const uint32_t*>(x)[at] : (uint32_t)static_cast<const uint16_t*>(x)[at];
    }
}

template <int NT, bool F32, bool PIN>
__device__ __forceinline__ void lfd_block_park(LfdBlockTile& tile, const int off[LFD_BLOCK_TILE / NT], const uint32_t v[LFD_BLOCK_TILE / NT]) {
#pragma unroll
    for (int k = 0; k < LFD_BLOCK_TILE / NT; ++k) {
        const float f = F32 ? lfd_block_round(lfd_block_float(v[k])) : lfd_block_widen((uint16_t)v[k]);
        tile[(int)threadIdx.x + NT * k] = lfd_block_opaque<PIN>(off[k]) < 0 ? 0.0f : f;
    }
}

// the tap sums of the lane's ROWS outputs (column lx, rows r0 .. r0 + ROWS - 1 of the tile; pixel (gy0 + j, gx) of the plane).  BORDER: which
// staged rows and columns lie inside the plane is kept as two bit sets per lane
template <int ROWS, bool BORDER, bool PIN>
__device__ __forceinline__ void lfd_block_window(const LfdBlockTile& tile, const float* __restrict__ w, int lx, int r0, int gy0, int gx, int H, int W,
                                                 float a[ROWS]) {
    unsigned cols = 0u, rows = 0u;
    if (BORDER) {
#pragma unroll
        for (int kx = 0; kx < LFD_BLOCK_K; ++kx) cols |= (gx + kx - LFD_BLOCK_R >= 0 && gx + kx - LFD_BLOCK_R < W) ? 1u << kx : 0u;
#pragma unroll
        for (int r = 0; r < ROWS + LFD_BLOCK_K - 1; ++r) rows |= (gy0 + r - LFD_BLOCK_R >= 0 && gy0 + r - LFD_BLOCK_R < H) ? 1u << r : 0u;
    }
#pragma unroll
    for (int j = 0; j < ROWS; ++j) a[j] = 0.0f;
#pragma unroll
    for (int r = 0; r < ROWS + LFD_BLOCK_K - 1; ++r) {                       // staged row r0 + r = plane row gy0 + r - 2
        float v[LFD_BLOCK_K];
#pragma unroll
        for (int kx = 0; kx < LFD_BLOCK_K; ++kx) v[kx] = tile[(r0 + r) * LFD_BLOCK_LX + lx + kx];
        const unsigned live = (unsigned)lfd_block_opaque<PIN>((int)((rows >> r) & 1u ? cols : 0u));     // the taps of this row that lie inside the plane
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            const int ky = r - j;
            if (ky < 0 || ky >= LFD_BLOCK_K) continue;
#pragma unroll
            for (int kx = 0; kx < LFD_BLOCK_K; ++kx) {
                const float next = lfd_block_tap(w[LFD_BLOCK_K * ky + kx], v[kx], a[j]);
                a[j] = (!BORDER || ((live >> kx) & 1u)) ? next : a[j];
            }
        }
    }
}

__device__ __forceinline__ bool lfd_block_interior(int y0, int x0, int H, int W) {
    return y0 >= LFD_BLOCK_R && x0 >= LFD_BLOCK_R && y0 + LFD_BLOCK_TY + LFD_BLOCK_R <= H && x0 + LFD_BLOCK_TX + LFD_BLOCK_R <= W;
}

// The grid: x counts the tiles of a plane (columns fastest), y and z together the planes (the general kernel) or images (the width-32 one) -
// their number may exceed what one grid dimension holds.  False: a workgroup of the last z slice beyond the end.
__device__ __forceinline__ bool lfd_block_place(unsigned tiles_x, unsigned count, unsigned& index, int& y0, int& x0) {
    const unsigned ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    index = blockIdx.z * gridDim.y + blockIdx.y;
    y0 = (int)ty * LFD_BLOCK_TY; x0 = (int)tx * LFD_BLOCK_TX;
    return index < count;
}

template <bool F32>
__global__ void __launch_bounds__(256) lfd_block_dw_kernel(const LfdBlockArgs p, const unsigned tiles_x) {
    __shared__ LfdBlockTile tile;
    const int lx = (int)threadIdx.x & 63, r0 = ((int)threadIdx.x >> 6) * LFD_BLOCK_DW_ROWS;
    unsigned pl;                                                                  // b * C + c
    int y0, x0;
    if (!lfd_block_place(tiles_x, (unsigned)p.B * (unsigned)p.C, pl, y0, x0)) return;
    const int c = (int)(pl % (unsigned)p.C);
    const int64_t plane = (int64_t)pl * p.H * p.W;
    int off[LFD_BLOCK_TILE / 256];
    uint32_t v[LFD_BLOCK_TILE / 256];
    lfd_block_offsets<256>(y0, x0, p.H, p.W, off);
    lfd_block_fetch<256, F32, false>(p.x, plane, off, v);
    lfd_block_park<256, F32, false>(tile, off, v);
    __syncthreads();
    const float* w = p.w + (int64_t)c * (LFD_BLOCK_K * LFD_BLOCK_K);
    float a[LFD_BLOCK_DW_ROWS];
    if (lfd_block_interior(y0, x0, p.H, p.W)) lfd_block_window<LFD_BLOCK_DW_ROWS, false, false>(tile, w, lx, r0, y0 + r0, x0 + lx, p.H, p.W, a);
    else lfd_block_window<LFD_BLOCK_DW_ROWS, true, false>(tile, w, lx, r0, y0 + r0, x0 + lx, p.H, p.W, a);
    const float s = p.s[c], sh = p.t[c];
#pragma unroll
    for (int j = 0; j < LFD_BLOCK_DW_ROWS; ++j) {
        const int y = y0 + r0 + j, x = x0 + lx;
        if (y < p.H && x < p.W) p.out[plane + (int64_t)y * p.W + x] = lfd_block_bf16(lfd_block_hidden(s, a[j], sh));
    }
}

// the 32 planes of one tile, in order, into the lane's accumulators
template <bool F32, bool BORDER>
__device__ __forceinline__ void lfd_block_pw_planes(const LfdBlockArgs& p, LfdBlockTile (&tile)[2], int64_t image, int64_t hw, int y0, int x0, int lx, int r0,
                                                    const float* bias, float z[LFD_BLOCK_PW_ROWS][LFD_BLOCK_PW_C]) {
    int off[LFD_BLOCK_TILE / 512];
    uint32_t v[LFD_BLOCK_TILE / 512];
    lfd_block_offsets<512>(y0, x0, p.H, p.W, off);
    lfd_block_fetch<512, F32, true>(p.x, image, off, v);
    lfd_block_park<512, F32, true>(tile[0], off, v);
    __syncthreads();
    // z = pb, read back from LDS (one address for all lanes: a broadcast): scalar loads would park the 32 values in SGPRs until the loop starts
#pragma unroll
    for (int o = 0; o < LFD_BLOCK_PW_C; ++o) {
        const float b0 = bias[o];
#pragma unroll
        for (int j = 0; j < LFD_BLOCK_PW_ROWS; ++j) z[j][o] = b0;
    }
#pragma unroll 1
    for (int c = 0; c < LFD_BLOCK_PW_C; ++c) {
        if (c + 1 < LFD_BLOCK_PW_C) lfd_block_fetch<512, F32, true>(p.x, image + (int64_t)(c + 1) * hw, off, v);      // in flight while plane c is computed
        float a[LFD_BLOCK_PW_ROWS], h[LFD_BLOCK_PW_ROWS];
        lfd_block_window<LFD_BLOCK_PW_ROWS, BORDER, true>(tile[c & 1], p.w + c * (LFD_BLOCK_K * LFD_BLOCK_K), lx, r0, y0 + r0, x0 + lx, p.H, p.W, a);
        const float s = p.s[c], sh = p.t[c];
#pragma unroll
        for (int j = 0; j < LFD_BLOCK_PW_ROWS; ++j) h[j] = lfd_block_hidden(s, a[j], sh);
        // the row of Wt in two halves, each behind a scheduling fence: the 25 depthwise weights are dead before the first half is loaded and
        // no more than 16 of the 32 are held at a time
        const float* wt = p.wt + c * LFD_BLOCK_PW_C;
#pragma unroll
        for (int o0 = 0; o0 < LFD_BLOCK_PW_C; o0 += 16) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int o = o0; o < o0 + 16; ++o) {
                const float m = wt[o];
#pragma unroll
                for (int j = 0; j < LFD_BLOCK_PW_ROWS; ++j) z[j][o] = lfd_block_mix(m, h[j], z[j][o]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (c + 1 < LFD_BLOCK_PW_C) lfd_block_park<512, F32, true>(tile[(c + 1) & 1], off, v);     // nobody reads that buffer since the barrier of plane c - 1
        __syncthreads();
    }
}

template <bool F32>
__global__ void __launch_bounds__(512) lfd_block_pw_kernel(const LfdBlockArgs p, const unsigned tiles_x) {
    __shared__ LfdBlockTile tile[2];
    __shared__ float bias[LFD_BLOCK_PW_C];
    const int lx = (int)threadIdx.x & 63, r0 = ((int)threadIdx.x >> 6) * LFD_BLOCK_PW_ROWS;
    unsigned b;
    int y0, x0;
    if (!lfd_block_place(tiles_x, (unsigned)p.B, b, y0, x0)) return;
    const int64_t hw = (int64_t)p.H * p.W, image = (int64_t)b * LFD_BLOCK_PW_C * hw;
    float z[LFD_BLOCK_PW_ROWS][LFD_BLOCK_PW_C];
    if (threadIdx.x < LFD_BLOCK_PW_C) bias[threadIdx.x] = p.pb[threadIdx.x];      // visible behind the first barrier of lfd_block_pw_planes
    if (lfd_block_interior(y0, x0, p.H, p.W)) lfd_block_pw_planes<F32, false>(p, tile, image, hw, y0, x0, lx, r0, bias, z);
    else lfd_block_pw_planes<F32, true>(p, tile, image, hw, y0, x0, lx, r0, bias, z);
#pragma unroll
    for (int j = 0; j < LFD_BLOCK_PW_ROWS; ++j) {
        const int y = y0 + r0 + j, x = x0 + lx;
        if (y < p.H && x < p.W) {
            uint16_t* o_ptr = p.out + image + (int64_t)y * p.W + x;
#pragma unroll
            for (int o = 0; o < LFD_BLOCK_PW_C; ++o) o_ptr[(int64_t)o * hw] = lfd_block_bf16(z[j][o]);
        }
    }
}

// lfd_api.hip's lfd_refiner_block: the arguments were validated there (lfd_block_fill)
hipError_t lfd_block_launch(const LfdBlockArgs& p, hipStream_t stream) {
    const unsigned tiles_x = (unsigned)((p.W + LFD_BLOCK_TX - 1) / LFD_BLOCK_TX), tiles_y = (unsigned)((p.H + LFD_BLOCK_TY - 1) / LFD_BLOCK_TY);
    const unsigned count = (unsigned)p.B * (unsigned)(p.wt ? 1 : p.C);             // planes or images: < 2^31
    const unsigned gy = std::min(count, LFD_BLOCK_GRID_Y), gz = (count + gy - 1) / gy;               // gz <= 2^31 / 65535 < 65535
    const dim3 grid(tiles_x * tiles_y, gy, gz);                                    // x <= 512 * 2048 = 2^20
    if (p.wt && p.x_is_f32) hipLaunchKernelGGL(lfd_block_pw_kernel<true>, grid, dim3(512), 0, stream, p, tiles_x);
    else if (p.wt) hipLaunchKernelGGL(lfd_block_pw_kernel<false>, grid, dim3(512), 0, stream, p, tiles_x);
    else if (p.x_is_f32) hipLaunchKernelGGL(lfd_block_dw_kernel<true>, grid, dim3(256), 0, stream, p, tiles_x);
    else hipLaunchKernelGGL(lfd_block_dw_kernel<false>, grid, dim3(256), 0, stream, p, tiles_x);
    return hipGetLastError();
}
