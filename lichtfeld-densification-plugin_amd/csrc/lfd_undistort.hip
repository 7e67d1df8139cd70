// Image undistortion on the device (lfd_undistort_image): every pixel of the pinhole image is sent through the camera's distortion
// model and sampled from the photograph - lfd_undistort_pixel of lfd_undistort.hpp, the twin's own routine.
//
// One lane per output pixel, a 64 x 4 tile per 256-lane workgroup: a wave's lanes are consecutive columns of one row, so its stores are
// contiguous and its taps fall on neighbouring lines of the source.  The tiles lie on a 1-D grid, which has no 65535 limit.  A launch holds
// fewer than 2^32 lanes, so at most 2^24 - 1 tiles: every image of w h < 2^31 except degenerate strips (w = 1 with h > 2^26 and the like), which
// lfd_undistort_launch refuses as an invalid configuration itself.  No LDS beyond four words, nothing crosses a workgroup except the optional counter of invalid pixels: counted per wave, summed
// per workgroup, one vector atomic add per workgroup that found any (integer adds: the total does not depend on their order).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_undistort.hpp"

extern "C" __global__ void __launch_bounds__(256) lfd_undistort_kernel(const LfdUndistortArgs p, unsigned tiles_x, unsigned long long* n_invalid) {
    const unsigned ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const long long j = (long long)tx * 64 + (threadIdx.x & 63);
    const long long i = (long long)ty * 4 + (threadIdx.x >> 6);
    const bool active = j < p.w && i < p.h;
    bool valid = true;
    if (active) valid = lfd_undistort_pixel(p, (int)i, (int)j);
    if (!n_invalid) return;                                            // (uniform: a kernel argument)
    __shared__ unsigned wave_invalid[4];
    const unsigned bad = (unsigned)__popcll(__ballot(active && !valid));
    if ((threadIdx.x & 63) == 0) wave_invalid[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned total = (wave_invalid[0] + wave_invalid[1]) + (wave_invalid[2] + wave_invalid[3]);
        if (total) atomicAdd(n_invalid, (unsigned long long)total);
    }
}

// lfd_api.hip's lfd_undistort_image: the arguments were validated there (lfd_undistort_check)
static const unsigned long long LFD_UNDISTORT_MAX_TILES = (1ull << 24) - 1;      // 256 lanes each: gridDim.x * blockDim.x stays below 2^32

hipError_t lfd_undistort_launch(const LfdUndistortArgs& p, unsigned long long* n_invalid, hipStream_t stream) {
    const unsigned tiles_x = (unsigned)(((long long)p.w + 63) / 64);
    const unsigned tiles_y = (unsigned)(((long long)p.h + 3) / 4);
    if ((unsigned long long)tiles_x * tiles_y > LFD_UNDISTORT_MAX_TILES) return hipErrorInvalidConfiguration;       // (w = 1, h > 2^26 and the like)
    hipLaunchKernelGGL(lfd_undistort_kernel, dim3(tiles_x * tiles_y), dim3(256), 0, stream, p, tiles_x, n_invalid);
    return hipGetLastError();
}
