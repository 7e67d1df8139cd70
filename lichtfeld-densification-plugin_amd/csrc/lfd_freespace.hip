// Free-space filter on the device (lfd_freespace_filter): a point of the final cloud is dropped when more references looked
// THROUGH it than confirm it (lfd_freespace.hpp has the projection, the judgement and the keep decision, shared with the twin).
//
// Steps, one launch each, nothing waits for another workgroup (lfd_api.hip's lfd_freespace_filter issues them):
//
//   lfd_freespace_fill_kernel      every word of the n_refs z-buffers becomes the bits of +inf, on every call
//   lfd_freespace_splat_kernel     a lane per point: its own reference by binary search of the offsets, its cell and depth in its own camera, one
//                                  vector atomic minimum on the u32 pattern (positive finite f32 order like their bits: collisions are deterministic)
//   lfd_freespace_count_kernel     the hot path: a lane per point in INPUT order walks every other reference; keep byte and u8 counts at its index
//   the stable compaction          lfd_consensus.hip's wgcount / offsets / scatter kernels and lfd_voxel.hip's scan, launched as they are
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_device.hpp"
#include "lfd_support.hpp"
#include "lfd_freespace.hpp"

extern "C" __global__ void __launch_bounds__(256) lfd_freespace_fill_kernel(uint32_t* __restrict__ zbuf, long long n_words) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (long long)gridDim.x * 256) zbuf[i] = LFD_FREESPACE_EMPTY;
}

extern "C" __global__ void __launch_bounds__(256) lfd_freespace_splat_kernel(const float* __restrict__ xyz, long long n,
                                                                            const long long* __restrict__ offs, int n_refs,
                                                                            const LfdFreespaceCam* __restrict__ cams, int pw, int ph,
                                                                            uint32_t* __restrict__ zbuf) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int r = lfd_support_ref_of(offs, n_refs, n, i);              // in [0, n_refs)
    const LfdFreespaceCam cam = cams[r];
    int cx, cy;
    float d;
    if (!lfd_freespace_project(cam, (double)pw, (double)ph, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], cx, cy, d)) return;
    // 0 <= cx < pw, 0 <= cy < ph (lfd_freespace_project clamps both): the word lies inside reference r's plane
    atomicMin(&zbuf[((long long)r * ph + cy) * pw + cx], __float_as_uint(d));
}

// The loop over the references is wave-uniform: a camera's 14 values are read through a uniform index (the scalar path), the own reference is
// skipped by a compare, both counters stay in registers.  A reference's points come in cell order, so neighbouring lanes read neighbouring
// z-buffer words.
extern "C" __global__ void __launch_bounds__(256) lfd_freespace_count_kernel(const float* __restrict__ xyz, long long n,
                                                                            const long long* __restrict__ offs, int n_refs,
                                                                            const LfdFreespaceCam* __restrict__ cams,
                                                                            const uint32_t* __restrict__ zbuf, int pw, int ph, float tol,
                                                                            int min_violations, uint8_t* __restrict__ keep,
                                                                            uint8_t* __restrict__ violations, uint8_t* __restrict__ supports) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int own = lfd_support_ref_of(offs, n_refs, n, i);
    int v, s;
    lfd_freespace_count_point(cams, zbuf, n_refs, own, pw, ph, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], tol, v, s);
    keep[i] = lfd_freespace_keep(v, s, min_violations) ? (uint8_t)1 : (uint8_t)0;
    if (violations) violations[i] = lfd_freespace_u8(v);
    if (supports) supports[i] = lfd_freespace_u8(s);
}
