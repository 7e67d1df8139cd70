// Spatial point cap on the device (lfd_cap_spatial): of n points keep a budget of m, one per cell of the coarsest Morton level that
// has m cells, picked evenly along the curve and represented by their point of smallest error (lfd_cap.hpp has the rule, shared with the twin).
//
// Phases, one launch each, nothing waits for another workgroup (lfd_api.hip's lfd_cap_spatial issues them):
//
//   lfd_consensus_minmax_kernel    min / max and the non-finite flag (then lfd_voxel_final_kernel); the host makes the box
//   lfd_cap_keys_kernel            63-bit Morton key of every point and the identity payload
//   the stable LSD radix sort      lfd_voxel.hip's histogram / scan / scatter kernels over all 63 bits
//   lfd_cap_levels_kernel          the level at which every adjacent pair of sorted keys parts, as a 22-bin histogram; the host reads it, takes
//                                  the prefix sums cells(l) and chooses the level
//   lfd_cap_coarsen_kernel         the sorted keys shifted down to the cell keys of that level (in place; the order stays)
//   the cell heads                 lfd_voxel.hip's head count / scan / scatter: the number of cells and the first sorted position of each
//   lfd_cap_rep_kernel             per picked cell the smallest (error rank, input index), a 64-bit atomicMin behind a segmented wave reduction
//   lfd_cap_mark_kernel            a keep byte at the input index of every picked cell's representative
//   the compaction prefix          lfd_consensus_wgcount_kernel + lfd_voxel_scan_kernel
//   lfd_cap_index_kernel           the input indices of the kept points, ascending
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_device.hpp"
#include "lfd_cap.hpp"

extern "C" __global__ void __launch_bounds__(256) lfd_cap_keys_kernel(const float* __restrict__ xyz, long long n, LfdCapBox box,
                                                                     unsigned long long* __restrict__ keys, unsigned* __restrict__ idx) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        keys[i] = lfd_cap_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], box);
        idx[i] = (unsigned)i;
    }
}

// hist[l] += sorted positions j >= 1 whose key parts from its predecessor's at level l (1 .. 21).  The counts of a wave are wave-uniform (a
// ballot per level); lane 0 adds them to the workgroup's LDS bins, and the workgroup adds its bins to the 22 global ones.
extern "C" __global__ void __launch_bounds__(256) lfd_cap_levels_kernel(const unsigned long long* __restrict__ keys, long long n,
                                                                       unsigned* __restrict__ hist) {
    __shared__ unsigned h[LFD_CAP_LEVELS + 1];
    const int tid = (int)threadIdx.x;
    if (tid <= LFD_CAP_LEVELS) h[tid] = 0u;
    __syncthreads();
    unsigned cnt[LFD_CAP_LEVELS + 1] = {};
    for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {      // (the same trips for every lane)
        const long long j = base + tid;
        const int l = (j >= 1 && j < n) ? lfd_cap_pair_level(keys[j], keys[j - 1]) : 0;
#pragma unroll
        for (int q = 1; q <= LFD_CAP_LEVELS; ++q) cnt[q] += (unsigned)__popcll(__ballot(l == q));
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 1; q <= LFD_CAP_LEVELS; ++q)
            if (cnt[q]) atomicAdd(&h[q], cnt[q]);
    }
    __syncthreads();
    if (tid >= 1 && tid <= LFD_CAP_LEVELS && h[tid]) atomicAdd(&hist[tid], h[tid]);
}

extern "C" __global__ void __launch_bounds__(256) lfd_cap_coarsen_kernel(unsigned long long* __restrict__ keys, long long n, int shift) {
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long long)gridDim.x * 256) keys[j] = keys[j] >> shift;
}

// One lane per sorted position.  Its cell is the last k with vstart[k] <= j; where the cell is picked, the lane's (rank, index) enters the cell's
// minimum.  The lanes of a cell are neighbours, so a segmented down-scan over the wave leaves the minimum of every run of equal cells in the
// run's first lane, which alone goes to memory: a cell costs one atomic per wave that touches it (the fullest cell: points / 64 + 1).
extern "C" __global__ void __launch_bounds__(256) lfd_cap_rep_kernel(const unsigned* __restrict__ sorted_idx, const unsigned* __restrict__ vstart,
                                                                    const unsigned* __restrict__ nc_p, const float* __restrict__ err, long long n,
                                                                    unsigned long long budget, unsigned long long* __restrict__ rep) {
    const int lane = (int)threadIdx.x & 63;
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned nc = *nc_p;
    unsigned k = 0xffffffffu;                                          // no cell: a lane behind the end, or one of a cell that is not picked
    unsigned long long val = ~0ull;
    if (j < n && nc > 0u) {
        unsigned lo = 0u, hi = nc;                                     // vstart[0] = 0 <= j
        while (hi - lo > 1u) {
            const unsigned mid = lo + ((hi - lo) >> 1);
            if ((long long)vstart[mid] <= j) lo = mid; else hi = mid;
        }
        if (lfd_cap_pick(lo, budget, nc)) {
            const unsigned i = sorted_idx[j];                          // < n: the sort's payload is a permutation of 0 .. n - 1
            k = lo;
            val = lfd_cap_pack(err ? lfd_cap_rank(__float_as_uint(err[i])) : 0u, i);
        }
    }
    const unsigned before = __shfl_up(k, 1, 64);
    const bool first = lane == 0 || before != k;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned ok = __shfl_down(k, off, 64);
        const unsigned long long ov = __shfl_down(val, off, 64);
        if (lane + off < 64 && ok == k && ov < val) val = ov;
    }
    if (first && k != 0xffffffffu) atomicMin(&rep[k], val);            // k < nc <= n: rep holds n words
}

extern "C" __global__ void __launch_bounds__(256) lfd_cap_mark_kernel(const unsigned long long* __restrict__ rep, const unsigned* __restrict__ nc_p,
                                                                     long long n, unsigned long long budget, uint8_t* __restrict__ keep) {
    const unsigned nc = *nc_p;
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < (long long)nc; k += (long long)gridDim.x * 256) {
        if (!lfd_cap_pick((unsigned long long)k, budget, nc)) continue;
        const long long i = (long long)(rep[k] & 0xffffffffull);       // every cell holds a point, so a picked cell's word was written
        if (i < n) keep[i] = (uint8_t)1;
    }
}

// the kept input indices in ascending order: lfd_consensus_scatter_kernel's placement, an index where that writes a point
extern "C" __global__ void __launch_bounds__(256) lfd_cap_index_kernel(const uint8_t* __restrict__ keep, const unsigned* __restrict__ wg_kept, long long n,
                                                                      long long capacity, long long* __restrict__ keep_out) {
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
    const long long o = (long long)wg_kept[blockIdx.x] + rank;
    if (o < capacity) keep_out[o] = i;                                 // (exactly min(budget, cells) <= capacity bytes are set)
}
