// The output head of RoMa-v2's refiners on the device (lfd_refiner_head): both 1x1 convolutions, the warp update, the
// Cholesky-to-precision conversion and the addition of the previous state in ONE launch that reads z exactly once.  The arithmetic is
// lfd_head.hpp's, in its order: per output one fmaf chain over the channels, ascending - whatever the loads look like.
//
// A plane of z is H W adjacent elements and both outputs are pixel-major, so the kernel counts pixels n = y W + x of an image and needs (y, x)
// only to address the strided previous state (loaded first, before the planes stream).  Lane l of a workgroup of T threads owns the PX adjacent pixels from (T blockIdx.x + l) PX on and walks the C
// planes in order, LFD_HEAD_UNROLL of them per step: all loads of a step are issued before the fmafs that consume them.  For a fixed plane
// consecutive lanes read consecutive addresses.  The 6 C weights are the same for every lane: scalar loads.
//
//   VEC    H W is a multiple of PX and z, warp and conf are aligned: a lane's PX values of a plane are ONE load (bf16: 4 or 8 bytes, f32: 8 or 16),
//          warp is stored as 16 bytes per two pixels and conf as 16 bytes per pixel.
//   !VEC   element loads (the index clamped to the plane, so every load is inside z) and stores, pixels beyond the plane skipped.
//   PX     4 where the call has at least LFD_HEAD_WIDE_FROM pixels (enough waves to fill the machine with 8-byte loads), else 2.
//   T      256, or 64 where 256 would make fewer than LFD_HEAD_MIN_GROUPS workgroups: the patch-4 refiner's 128 x 128 image is 128 waves, which
//          32 workgroups would put on 32 of the 256 compute units.
//
// No LDS, no atomics, nothing crosses a lane; no address is formed from data.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lfd_head.hpp"

#define LFD_HEAD_THREADS 256
#define LFD_HEAD_FEW_THREADS 64
#define LFD_HEAD_MIN_GROUPS 1024u                            // four workgroups per compute unit
#define LFD_HEAD_UNROLL 8                                    // planes in flight per lane
#define LFD_HEAD_WIDE_FROM (1 << 18)                         // pixels of a call from which a lane owns 4 instead of 2: 1024 waves of 4-pixel lanes
#define LFD_HEAD_GRID_Y 65535u                               // images per z slice of the grid

template <int N>
struct alignas(4 * N) LfdHeadVec { uint32_t v[N]; };

// words a lane holds of one plane
template <bool F32, bool VEC, int PX>
struct LfdHeadRaw { uint32_t v[F32 ? PX : (VEC ? PX / 2 : PX)]; };

// the lane's PX values of the plane that starts at element `plane`, pixels n0 .. n0 + PX - 1
template <bool F32, bool VEC, int PX>
__device__ __forceinline__ void lfd_head_fetch(const void* z, int64_t plane, uint32_t n0, uint32_t hw, LfdHeadRaw<F32, VEC, PX>& r) {
    if (VEC) {
        constexpr int N = F32 ? PX : PX / 2;
        const char* at = static_cast<const char*>(z) + (plane + n0) * (F32 ? 4 : 2);
        const LfdHeadVec<N> w = *reinterpret_cast<const LfdHeadVec<N>*>(at);
#pragma unroll
        for (int k = 0; k < N; ++k) r.v[k] = w.v[k];
    } else {
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const int64_t at = plane + std::min(n0 + (uint32_t)j, hw - 1u);
            r.v[j] = F32 ? static_cast<const uint32_t*>(z)[at] : (uint32_t)static_cast<const uint16_t*>(z)[at];
        }
    }
}

template <bool F32, bool VEC, int PX>
__device__ __forceinline__ float lfd_head_value(const LfdHeadRaw<F32, VEC, PX>& r, int j) {
    uint32_t u;
    if (F32) u = r.v[j];
    else if (VEC) u = (j & 1) ? (r.v[j >> 1] & 0xffff0000u) : (r.v[j >> 1] << 16);
    else u = r.v[j] << 16;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

template <bool F32, bool VEC, int PX>
__global__ void __launch_bounds__(LFD_HEAD_THREADS) lfd_head_kernel(const LfdHeadArgs p) {
    const uint32_t hw = (uint32_t)p.H * (uint32_t)p.W;                            // <= 2^31 - 1
    const uint64_t first = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * PX;
    if (first >= hw) return;
    const uint32_t n0 = (uint32_t)first;
    const uint32_t b = blockIdx.z * gridDim.y + blockIdx.y;                       // the image: grid y and z together, B may exceed one dimension
    if (b >= (uint32_t)p.B) return;
    const int C = p.C;
    // Every load of the weights and the bias stands before the kernel's first store (there is no loop over images around them), which is what
    // lets the compiler prove them unclobbered and fetch them with s_load: inside a batch loop they became 16-byte vector loads of 48 VGPRs a step.
    const float* __restrict__ const wts = p.w;
    const float* __restrict__ const bias = p.bias;
    {
        const int64_t image = (int64_t)b * C * hw;
        // The previous state first: it does not depend on z, its loads are under way while the planes stream, and its eight strides and two
        // pointers are dead before the channel loop instead of occupying scalar registers through it.
        float pw[PX][2], pc[PX][4];
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const uint32_t n = std::min(n0 + (uint32_t)j, hw - 1u);               // a pixel beyond the plane repeats the last one and is not stored
            const uint32_t y = n / (uint32_t)p.W, x = n - y * (uint32_t)p.W;
            const float* q = p.pw + b * p.sw[0] + y * p.sw[1] + x * p.sw[2];
            pw[j][0] = q[0]; pw[j][1] = q[p.sw[3]];
            pc[j][0] = pc[j][1] = pc[j][2] = pc[j][3] = 0.0f;
            if (p.prev_dim) {
                const float* s = p.pc + b * p.sc[0] + y * p.sc[1] + x * p.sc[2];
                pc[j][0] = s[0];
                if (p.prev_dim == 4) { pc[j][1] = s[p.sc[3]]; pc[j][2] = s[2 * p.sc[3]]; pc[j][3] = s[3 * p.sc[3]]; }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        float a[LFD_HEAD_OUT][PX];
#pragma unroll
        for (int o = 0; o < LFD_HEAD_OUT; ++o) {
            const float b0 = bias[o];
#pragma unroll
            for (int j = 0; j < PX; ++j) a[o][j] = b0;
        }
        int c = 0;
        for (; c + LFD_HEAD_UNROLL <= C; c += LFD_HEAD_UNROLL) {
            LfdHeadRaw<F32, VEC, PX> r[LFD_HEAD_UNROLL];
#pragma unroll
            for (int k = 0; k < LFD_HEAD_UNROLL; ++k) lfd_head_fetch<F32, VEC, PX>(p.z, image + (int64_t)(c + k) * hw, n0, hw, r[k]);
#pragma unroll
            for (int k = 0; k < LFD_HEAD_UNROLL; ++k) {
                // the weights of two planes at a time behind a scheduling fence: all 48 of a step at once do not fit the scalar registers
                if (k % 2 == 0) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int o = 0; o < LFD_HEAD_OUT; ++o) {
                    const float w = wts[(int64_t)o * C + c + k];
#pragma unroll
                    for (int j = 0; j < PX; ++j) a[o][j] = lfd_head_mix(w, lfd_head_value<F32, VEC, PX>(r[k], j), a[o][j]);
                }
            }
        }
        for (; c < C; ++c) {
            LfdHeadRaw<F32, VEC, PX> r;
            lfd_head_fetch<F32, VEC, PX>(p.z, image + (int64_t)c * hw, n0, hw, r);
#pragma unroll
            for (int o = 0; o < LFD_HEAD_OUT; ++o) {
                const float w = wts[(int64_t)o * C + c];
#pragma unroll
                for (int j = 0; j < PX; ++j) a[o][j] = lfd_head_mix(w, lfd_head_value<F32, VEC, PX>(r, j), a[o][j]);
            }
        }
        float wv[PX][2], cv[PX][4];
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const float aj[LFD_HEAD_OUT] = {a[0][j], a[1][j], a[2][j], a[3][j], a[4][j], a[5][j]};
            lfd_head_finish(aj, p.qx, p.qy, pw[j], pc[j], p.prev_dim, wv[j], cv[j]);
        }
        const int64_t px = (int64_t)b * hw + n0;                                  // < 2^31
        if (VEC) {
#pragma unroll
            for (int j = 0; j < PX; j += 2) {
                LfdHeadVec<4> t;
                t.v[0] = __float_as_uint(wv[j][0]); t.v[1] = __float_as_uint(wv[j][1]); t.v[2] = __float_as_uint(wv[j + 1][0]); t.v[3] = __float_as_uint(wv[j + 1][1]);
                *reinterpret_cast<LfdHeadVec<4>*>(p.warp + 2 * (px + j)) = t;
            }
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                LfdHeadVec<4> t;
#pragma unroll
                for (int k = 0; k < 4; ++k) t.v[k] = __float_as_uint(cv[j][k]);
                *reinterpret_cast<LfdHeadVec<4>*>(p.conf + 4 * (px + j)) = t;
            }
        } else {
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                if (n0 + (uint32_t)j >= hw) continue;
                p.warp[2 * (px + j)] = wv[j][0]; p.warp[2 * (px + j) + 1] = wv[j][1];
#pragma unroll
                for (int k = 0; k < 4; ++k) p.conf[4 * (px + j) + k] = cv[j][k];
            }
        }
    }
}

template <bool F32, bool VEC, int PX>
static void lfd_head_start(const LfdHeadArgs& p, hipStream_t stream) {
    const uint32_t hw = (uint32_t)p.H * (uint32_t)p.W, gy = std::min((uint32_t)p.B, LFD_HEAD_GRID_Y), gz = ((uint32_t)p.B + gy - 1) / gy;
    uint32_t threads = LFD_HEAD_THREADS, per = threads * PX;
    if ((uint64_t)((hw + per - 1) / per) * p.B < LFD_HEAD_MIN_GROUPS) { threads = LFD_HEAD_FEW_THREADS; per = threads * PX; }      // then x < 4 * 1024
    const dim3 grid((hw + per - 1) / per, gy, gz);                                  // x <= 2^31 / 512
    hipLaunchKernelGGL((lfd_head_kernel<F32, VEC, PX>), grid, dim3(threads), 0, stream, p);
}

// lfd_api.hip's lfd_refiner_head: the arguments were validated there (lfd_head_fill)
hipError_t lfd_head_launch(const LfdHeadArgs& p, hipStream_t stream) {
    const long long hw = (long long)p.H * p.W;
    const uintptr_t zp = reinterpret_cast<uintptr_t>(p.z), outs = reinterpret_cast<uintptr_t>(p.warp) | reinterpret_cast<uintptr_t>(p.conf);
    const unsigned elt = p.z_is_f32 ? 4u : 2u;
    const bool vec2 = hw % 2 == 0 && zp % (2 * elt) == 0 && outs % 16 == 0;
    const bool vec4 = hw % 4 == 0 && zp % (4 * elt) == 0 && outs % 16 == 0 && hw * p.B >= LFD_HEAD_WIDE_FROM;
    if (p.z_is_f32) {
        if (vec4) lfd_head_start<true, true, 4>(p, stream);
        else if (vec2) lfd_head_start<true, true, 2>(p, stream);
        else lfd_head_start<true, false, 2>(p, stream);
    } else {
        if (vec4) lfd_head_start<false, true, 4>(p, stream);
        else if (vec2) lfd_head_start<false, true, 2>(p, stream);
        else lfd_head_start<false, false, 2>(p, stream);
    }
    return hipGetLastError();
}
