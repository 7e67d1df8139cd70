// Footprint-adaptive thinning on the device (lfd_thin_footprint): keep one point per cell of a linear octree over the final cloud,
// every point at the level its own reference camera's footprint selects (lfd_thin.hpp has the rule, shared with the twin).
//
// Phases, one launch each, nothing waits for another workgroup (lfd_api.hip's lfd_thin_footprint issues them):
//
//   lfd_consensus_minmax_kernel    min / max and the non-finite flag (then lfd_voxel_final_kernel); the host makes the box
//   lfd_thin_keys_kernel           level and location code of every point, the identity payload, the points-per-level histogram
//   the stable LSD radix sort      lfd_voxel.hip's histogram / scan / scatter kernels over the 61 bits of a code
//   the cell heads                 lfd_voxel.hip's head count / scan / scatter: the number of cells and the first sorted position of each
//   lfd_thin_cells_kernel          cells per level from the head codes' bit length
//   lfd_cap_rep_kernel             per cell the smallest (error rank, input index); lfd_cap_mark_kernel the keep byte of that point - the cap's
//                                  kernels with a budget no smaller than the cell count, under which every cell is picked
//   the compaction prefix          lfd_consensus_wgcount_kernel + lfd_voxel_scan_kernel, lfd_consensus_offsets_kernel for the kept offsets
//   lfd_cap_index_kernel           the input indices of the kept points, ascending
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_device.hpp"
#include "lfd_support.hpp"
#include "lfd_thin.hpp"

// bins[l] += lanes of the wave whose level is l (l < 0: none): one ballot per level present in the wave, lane 0 adds to the workgroup's LDS bins.
// Every lane of the wave calls it.
static __device__ __forceinline__ void lfd_thin_wave_bins(int lev, unsigned* bins) {
    unsigned long long todo = __ballot(lev >= 0);
    while (todo) {                                                     // (wave-uniform)
        const int q = __shfl(lev, __ffsll((long long)todo) - 1, 64);
        const unsigned long long m = __ballot(lev == q);
        if ((threadIdx.x & 63) == 0) atomicAdd(&bins[q], (unsigned)__popcll(m));
        todo &= ~m;
    }
}

// A lane per point of every 256-point block the workgroup strides over.  The reference of a block's first point is found with uniform loads; a
// block that lies inside one reference - all but n_refs - 1 of them - searches nothing else, the others search per point.  The level counts
// stay in the workgroup's LDS bins over all its blocks: at most 21 global adds per workgroup, as lfd_cap_levels_kernel (a workgroup per block
// would put tens of thousands of atomics on the same 21 words).  offs: validated on the host (0 = offs[0] <= .. <= offs[n_refs] = n).
extern "C" __global__ void __launch_bounds__(256) lfd_thin_keys_kernel(const float* __restrict__ xyz, long long n, const long long* __restrict__ offs,
                                                                      int n_refs, const double* __restrict__ rows, double thin_cells, LfdCapBox box,
                                                                      unsigned long long* __restrict__ keys, unsigned* __restrict__ idx,
                                                                      unsigned* __restrict__ hist) {
    __shared__ unsigned h[LFD_THIN_LEVELS];
    const int tid = (int)threadIdx.x;
    if (tid < LFD_THIN_LEVELS) h[tid] = 0u;
    __syncthreads();
    for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {      // (the same trips for every lane)
        const long long last = (base + 256 < n ? base + 256 : n) - 1;
        const int r0 = lfd_support_ref_of(offs, n_refs, n, base);
        const bool one = last < offs[r0 + 1];
        const long long i = base + tid;
        int lev = -1;
        if (i < n) {
            const int r = one ? r0 : lfd_support_ref_of(offs, n_refs, n, i);
            const double* row = rows + LFD_THIN_ROW * (long long)r;
            const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
            lev = lfd_thin_level(lfd_thin_depth(row, x, y, z), row[4], thin_cells, box.L);
            keys[i] = lfd_thin_code(lfd_cap_key(x, y, z, box), lev);
            idx[i] = (unsigned)i;
        }
        lfd_thin_wave_bins(lev, h);
    }
    __syncthreads();
    if (tid < LFD_THIN_LEVELS && h[tid]) atomicAdd(&hist[tid], h[tid]);
}

// hist[l] += cells of level l: the level of a cell is the bit length of its code, read at the cell's first sorted position
extern "C" __global__ void __launch_bounds__(256) lfd_thin_cells_kernel(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ vstart,
                                                                       const unsigned* __restrict__ nc_p, long long n, unsigned* __restrict__ hist) {
    __shared__ unsigned h[LFD_THIN_LEVELS];
    const int tid = (int)threadIdx.x;
    if (tid < LFD_THIN_LEVELS) h[tid] = 0u;
    __syncthreads();
    const long long nc = (long long)*nc_p;                             // <= n
    for (long long base = (long long)blockIdx.x * 256; base < nc; base += (long long)gridDim.x * 256) {     // (the same trips for every lane)
        const long long k = base + tid;
        int lev = -1;
        if (k < nc) {
            const long long j = (long long)vstart[k];
            if (j < n) lev = lfd_thin_code_level(keys[j]);             // (a head is a sorted position: always so)
            lev = lev < LFD_THIN_LEVELS ? lev : LFD_THIN_MAX_LEVEL;    // (a code is below 2^61: always so; no bin lies outside h)
        }
        lfd_thin_wave_bins(lev, h);
    }
    __syncthreads();
    if (tid < LFD_THIN_LEVELS && h[tid]) atomicAdd(&hist[tid], h[tid]);
}
