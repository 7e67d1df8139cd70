// Epipolar audit on the device (lfd_epipolar_audit).
//
// lfd_audit_kernel: one launch per batch, grid (ceil(H W / 256), n_refs), a lane per grid cell of one reference - the far kernel's front end: the
// reference's neighbours staged in LDS by the first lanes, a uniform loop over slots, each slot's certainty (4 B) and observation (8 B) read by
// consecutive lanes for consecutive cells, the gathers of up to eight slots before their arithmetic (sixteen slots' gathers held at once
// cost 240 VGPRs and scratch).  (r, j) is uniform: the pair's F sits in LDS and every lane reads the same word.
//
// Almost every lane of a wave lands in two or three bins, so the histogram is aggregated inside the wave before it touches memory: the first
// remaining lane's bin is broadcast, the lanes that share it are balloted, one lane adds their number to the workgroup's LDS table, they are
// cleared, and so on for LFD_AUDIT_TURNS turns; the lanes left after that - the tail of outliers, each in a bin of its own, for which a turn
// per bin costs more than it saves (profiles/r29/audit.txt) - add for themselves.  The two counters are population counts of two ballots.
// After a barrier the workgroup adds every NON-ZERO entry of its LDS table to the global one with a no-return 64-bit atomic.  Integer
// additions only, so the table does not depend on the launch geometry.  A wave without a confident cell in a slot skips that slot's f64
// work (a uniform branch).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_audit.hpp"
#include "lfd_device.hpp"

#define LFD_AUDIT_TURNS 3           // bins a wave aggregates before its remaining lanes add for themselves

template <int KMAX, int C, bool AGGREGATE>
__global__ void __launch_bounds__(256) lfd_audit_kernel(const LfdAuditArgs p) {
    __shared__ LfdSlot sh[KMAX];
    __shared__ double sh_F[KMAX * 9];
    __shared__ unsigned sh_tab[KMAX * LFD_AUDIT_QUANTITIES];           // (a workgroup adds at most 256 per entry)
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int r = (int)blockIdx.y;
    const LfdSupportGeom g = p.g;
    const int HW = g.H * g.W;                                          // <= 2^31 - 1 (the batch was validated)
    const long long cell_ll = (long long)blockIdx.x * 256 + tid;
    const bool mine = cell_ll < (long long)HW;
    const int cell = mine ? (int)cell_ll : HW - 1;                     // idle lanes read the last cell and add nothing
    const LfdRefDesc ref = static_cast<const LfdRefDesc*>(p.refs)[r];
    int ns = ref.n_slots;
    ns = ns < KMAX ? ns : KMAX;
    lfd_stage_slots(sh, p.slots, p.pair_const, r, p.k, ns);
    if (tid < ns * 9) sh_F[tid] = p.pair_const[(size_t)r * p.k + tid / 9].F[tid % 9];      // (ns * 9 <= 144 lanes)
    for (int i = tid; i < KMAX * LFD_AUDIT_QUANTITIES; i += 256) sh_tab[i] = 0u;
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
    int best = LFD_AUDIT_NONE;
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
#pragma unroll
        for (int i = 0; i < GROUP; ++i) {
            const int j = j0 + i;
            const bool conf = j < ns && ok && lfd_far_confident(sh[j < ns ? j : 0], g, p.audit_certainty, c[i], w[i].x, w[i].y);
            if (__ballot(conf)) {                                      // (uniform within the wave)
                const int bin = lfd_audit_bin(sh_F + j * 9, rsx, rsy, sh[j].sx, sh[j].sy, xan, yan, w[i].x, w[i].y, g.wm1, g.hm1);
                const bool usable = conf && bin >= 0, degenerate = conf && bin < 0;
                if (usable) best = bin < best ? bin : best;
                unsigned* tab = sh_tab + j * LFD_AUDIT_QUANTITIES;
                if (AGGREGATE) {
                    const unsigned long long um = __ballot(usable), dm = __ballot(degenerate);
                    if (lane == 0) {
                        if (um) atomicAdd(tab, (unsigned)__popcll(um));
                        if (dm) atomicAdd(tab + 1, (unsigned)__popcll(dm));
                    }
                    unsigned long long rem = um;
#pragma unroll
                    for (int turn = 0; turn < LFD_AUDIT_TURNS; ++turn) {   // (uniform: one turn per distinct bin of the wave, the first few)
                        if (!rem) break;
                        const int first = (int)__builtin_ctzll(rem);
                        const int b0 = __builtin_amdgcn_readlane(bin, first);      // in [0, 63]: lane `first` is usable
                        const unsigned long long same = __ballot(usable && bin == b0);
                        if (lane == first) atomicAdd(tab + 2 + b0, (unsigned)__popcll(same));
                        rem &= ~same;                                  // (same holds bit `first`)
                    }
                    if ((rem >> lane) & 1ull) atomicAdd(tab + 2 + bin, 1u);        // the tail - outliers, each in a bin of its own - adds for itself
                } else {
                    if (usable) { atomicAdd(tab, 1u); atomicAdd(tab + 2 + bin, 1u); }
                    if (degenerate) atomicAdd(tab + 1, 1u);
                }
            }
        }
    }
    if (p.best && mine) p.best[(size_t)r * HW + cell] = (uint8_t)best;
    __syncthreads();
    for (int i = tid; i < ns * LFD_AUDIT_QUANTITIES; i += 256) {       // rows r k + j, j < ns <= k: inside the table
        const unsigned v = sh_tab[i];
        if (v) atomicAdd(p.table + (size_t)r * p.k * LFD_AUDIT_QUANTITIES + i, (unsigned long long)v);
    }
}

template <int C, bool AGGREGATE>
static void lfd_audit_launch_c(const LfdAuditArgs& p, dim3 grid, hipStream_t stream) {
    if (p.k <= 4) hipLaunchKernelGGL((lfd_audit_kernel<4, C, AGGREGATE>), grid, dim3(256), 0, stream, p);
    else if (p.k <= 8) hipLaunchKernelGGL((lfd_audit_kernel<8, C, AGGREGATE>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((lfd_audit_kernel<LFD_MAX_SLOTS, C, AGGREGATE>), grid, dim3(256), 0, stream, p);
}

// lfd_api.hip's lfd_epipolar_audit: the arguments were validated there (H W <= 2^31 - 1, n_refs <= 65535 workgroup rows, warp_channels 2 or 4).
// aggregate = false: every confident lane issues its own LDS adds - the same table, kept for profiles/audit_timing.py's comparison.
hipError_t lfd_audit_launch(const LfdAuditArgs& p, bool aggregate, hipStream_t stream) {
    const long long HW = (long long)p.g.H * p.g.W;
    const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)p.n_refs);
    if (p.g.C == 2) { if (aggregate) lfd_audit_launch_c<2, true>(p, grid, stream); else lfd_audit_launch_c<2, false>(p, grid, stream); }
    else { if (aggregate) lfd_audit_launch_c<4, true>(p, grid, stream); else lfd_audit_launch_c<4, false>(p, grid, stream); }
    return hipGetLastError();
}
