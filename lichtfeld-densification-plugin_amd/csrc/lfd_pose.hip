// Pose corrections from the matches on the device (lfd_pose_accumulate).
//
// lfd_pose_kernel: one launch per batch, grid (ceil(H W / 256), n_refs), a lane per grid cell of one reference - the audit kernel's front end
// (lfd_audit.hip): the reference's neighbours and the pairs' constants (32 doubles each) staged in LDS, a uniform loop over slots, each slot's
// certainty (4 B) and observation (8 B) read by consecutive lanes for consecutive cells, the gathers of up to eight slots before their
// arithmetic.  (r, j) is uniform: every lane reads the same words of the pair's constants.  A wave without a confident cell in a slot skips
// that slot's f64 work (a uniform branch).
//
// The reduction has lfd_gain.hip's shape.  What a lane has per slot is a class and seven small integers (Jq [6], rq); what the table wants is
// three counts and 28 sums of products.  Per (reference, slot):
//   wave        three ballots give the counts.  The 28 products are formed in 64 bits and summed over the 64 lanes by a FOLDING butterfly: at
//               the step with lane offset 32 a lane keeps one half of the (padded) 32 sums and hands the other half to its partner, at 16 a
//               half of what it kept, and so on - 16 + 8 + 4 + 2 + 1 exchanges and a last plain one, 32 in all instead of 28 x 6 - after
//               which lane 2 e holds the wave's sum e.  (Summing every product over all lanes took 168 64-bit xor-shuffles per wave and slot
//               and 3.13 ms at 64 x 3 x 512^2 against 2.52 ms; profiles/r30/pose.txt has both.)  A wave
//               without an inlier skips all of it (a uniform branch)
//   workgroup   the even lanes add their non-zero sums to i64 accumulators in LDS: one LDS atomic instruction, 28 different words
//   global      behind a barrier, every NON-ZERO accumulator goes to the table with one no-return 64-bit atomic add
// Integer additions only (two's complement), so the table does not depend on the launch geometry.  No float atomics anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_device.hpp"
#include "lfd_pose.hpp"

#include <utility>

// Sum e (column 3 + e) is the product of q[a] and q[b], q = (Jq [6], rq, 0): a * 8 + b.  e >= 28 pads the 28 sums to 32 with 0 * 0.
__host__ __device__ constexpr int lfd_pose_pair(int e) {
    if (e == 0) return 6 * 8 + 6;
    if (e < 7) return (e - 1) * 8 + 6;
    if (e >= LFD_POSE_SUMS) return 7 * 8 + 7;
    int i = 0, f = e - 7;                                              // row-major upper triangle of 6 x 6
    while (f >= 6 - i) { f -= 6 - i; ++i; }
    return i * 8 + i + f;
}

template <int E>
__device__ __forceinline__ long long lfd_pose_product(const int32_t* q) {
    constexpr int ab = lfd_pose_pair(E);
    return (long long)q[ab >> 3] * q[ab & 7];
}

// the butterfly's first step: sums I and I + 16 are formed, one is kept and the other goes to the lane 32 away (upper: the lane's bit 5)
template <int I>
__device__ __forceinline__ long long lfd_pose_first(const int32_t* q, bool upper) {
    const long long a = lfd_pose_product<I>(q), b = lfd_pose_product<I + 16>(q);
    const long long keep = upper ? b : a, send = upper ? a : b;
    return keep + __shfl_xor(send, 32, 64);
}

template <int... I>
__device__ __forceinline__ void lfd_pose_first_all(const int32_t* q, bool upper, long long* v, std::integer_sequence<int, I...>) {
    ((v[I] = lfd_pose_first<I>(q, upper)), ...);
}

// All 28 sums of a wave: q[0 .. 7] the lane's integers (zero for a lane without an inlier; q[7] = 0).  Returns, in lane 2 e (and 2 e + 1),
// the wave's sum e; e = lane >> 1, of which 28 .. 31 are padding.
__device__ __forceinline__ long long lfd_pose_wave_sums(const int32_t* q, int lane) {
    long long v[16];
    lfd_pose_first_all(q, (lane & 32) != 0, v, std::make_integer_sequence<int, 16>{});
#pragma unroll
    for (int half = 8; half >= 1; half >>= 1) {                        // lane offsets 16, 8, 4, 2: the offset is twice the number of sums kept
        const bool upper = (lane & (2 * half)) != 0;
#pragma unroll
        for (int i = 0; i < half; ++i) {
            const long long keep = upper ? v[i + half] : v[i], send = upper ? v[i] : v[i + half];
            v[i] = keep + __shfl_xor(send, 2 * half, 64);
        }
    }
    return v[0] + __shfl_xor(v[0], 1, 64);
}

template <int KMAX, int C>
__global__ void __launch_bounds__(256) lfd_pose_kernel(const LfdPoseArgs p) {
    __shared__ LfdSlot sh[KMAX];
    __shared__ LfdPoseConst sh_pc[KMAX];
    __shared__ unsigned long long sh_acc[KMAX * LFD_POSE_QUANTITIES];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int r = (int)blockIdx.y;
    const LfdSupportGeom g = p.g;
    const int HW = g.H * g.W;                                          // <= 2^24 (lfd_pose_check_batch)
    const long long cell_ll = (long long)blockIdx.x * 256 + tid;
    const bool mine = cell_ll < (long long)HW;
    const int cell = mine ? (int)cell_ll : HW - 1;                     // idle lanes read the last cell and add nothing
    const LfdRefDesc ref = static_cast<const LfdRefDesc*>(p.refs)[r];
    int ns = ref.n_slots;
    ns = ns < KMAX ? ns : KMAX;
    lfd_stage_slots(sh, p.slots, p.pair_const, r, p.k, ns);
    {
        const double* src = reinterpret_cast<const double*>(p.pose_const + (size_t)r * p.k);
        double* dst = reinterpret_cast<double*>(sh_pc);
        for (int i = tid; i < ns * 32; i += 256) dst[i] = src[i];      // (sizeof(LfdPoseConst) == 32 doubles)
    }
    for (int i = tid; i < KMAX * LFD_POSE_QUANTITIES; i += 256) sh_acc[i] = 0ull;
    __syncthreads();
    const int y = cell / g.W, x = cell - y * g.W;
    float xan, yan;
    if (C == 4 && ns > 0) {
        const float2 a = *reinterpret_cast<const float2*>(sh[0].warp + (size_t)cell * C);
        xan = a.x; yan = a.y;
    } else if (C == 4) {
        xan = 0.0f; yan = 0.0f;                                        // (no slot: nothing is counted)
    } else {
        xan = p.axis_x[x]; yan = p.axis_y[y];
    }
    bool ok = mine;
    if (ok && ref.mask_a)
        ok = ref.mask_a[(size_t)lfd_nearest_src(y, g.mask_sy, g.h_match) * g.w_match + lfd_nearest_src(x, g.mask_sx, g.w_match)] != 0;
    const LfdRefConst& rc = p.ref_const[r];
    const float rsx = rc.sx, rsy = rc.sy;
    // up to eight slots at a time (one turn for k <= 8): all their gathers first, then the arithmetic
    constexpr int GROUP = KMAX < 8 ? KMAX : 8;
    for (int j0 = 0; j0 < ns; j0 += GROUP) {                           // (uniform)
        float c[GROUP];
        float2 w[GROUP];
#pragma unroll
        for (int i = 0; i < GROUP; ++i) {
            c[i] = 0.0f; w[i] = make_float2(0.0f, 0.0f);
            if (j0 + i < ns) {                                         // (uniform)
                c[i] = sh[j0 + i].cert[cell];
                w[i] = *reinterpret_cast<const float2*>(sh[j0 + i].warp + (size_t)cell * C + (C - 2));
            }
        }
        // the arithmetic is long (f64, 28 wave sums), so its code exists once: a rolled loop that picks slot i's gathers with selects (i is uniform)
#pragma unroll 1
        for (int i = 0; i < GROUP && j0 + i < ns; ++i) {
            const int j = j0 + i;
            float ci = c[0], wx = w[0].x, wy = w[0].y;
#pragma unroll
            for (int e = 1; e < GROUP; ++e)
                if (i == e) { ci = c[e]; wx = w[e].x; wy = w[e].y; }
            const bool conf = ok && lfd_far_confident(sh[j], g, p.pose_certainty, ci, wx, wy);
            if (__ballot(conf)) {                                      // (uniform within the wave)
                int32_t q[8];
                const int kind = lfd_pose_sample(sh_pc[j], rsx, rsy, sh[j].sx, sh[j].sy, xan, yan, wx, wy, g.wm1, g.hm1, p.c2, q);
                const bool in = conf && kind == LFD_POSE_INLIER;
                if (!in) {
#pragma unroll
                    for (int e = 0; e < 7; ++e) q[e] = 0;              // (an inlier of a lane that is not confident adds nothing)
                }
                q[7] = 0;
                const unsigned long long mi = __ballot(in), mo = __ballot(conf && kind == LFD_POSE_OUTLIER),
                                         md = __ballot(conf && kind == LFD_POSE_DEGENERATE);
                unsigned long long* acc = sh_acc + j * LFD_POSE_QUANTITIES;
                if (lane == 0) {
                    if (mi) atomicAdd(acc, (unsigned long long)__popcll(mi));
                    if (mo) atomicAdd(acc + 1, (unsigned long long)__popcll(mo));
                    if (md) atomicAdd(acc + 2, (unsigned long long)__popcll(md));
                }
                if (mi) {                                              // (uniform within the wave)
                    const long long s = lfd_pose_wave_sums(q, lane);
                    const int e = lane >> 1;
                    if ((lane & 1) == 0 && e < LFD_POSE_SUMS && s) atomicAdd(acc + 3 + e, (unsigned long long)s);
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < ns * LFD_POSE_QUANTITIES; i += 256) {        // rows r k + j, j < ns <= k: inside the table; column 31 is never non-zero
        const unsigned long long v = sh_acc[i];
        if (v) atomicAdd(p.table + (size_t)r * p.k * LFD_POSE_QUANTITIES + i, v);
    }
}

template <int C>
static void lfd_pose_launch_c(const LfdPoseArgs& p, dim3 grid, hipStream_t stream) {
    if (p.k <= 4) hipLaunchKernelGGL((lfd_pose_kernel<4, C>), grid, dim3(256), 0, stream, p);
    else if (p.k <= 8) hipLaunchKernelGGL((lfd_pose_kernel<8, C>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((lfd_pose_kernel<LFD_MAX_SLOTS, C>), grid, dim3(256), 0, stream, p);
}

// lfd_api.hip's lfd_pose_accumulate: the arguments were validated there (H W <= 2^24, n_refs <= 65535 workgroup rows, warp_channels 2 or 4).
hipError_t lfd_pose_launch(const LfdPoseArgs& p, hipStream_t stream) {
    const long long HW = (long long)p.g.H * p.g.W;
    const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)p.n_refs);
    if (p.g.C == 2) lfd_pose_launch_c<2>(p, grid, stream);
    else lfd_pose_launch_c<4>(p, grid, stream);
    return hipGetLastError();
}
