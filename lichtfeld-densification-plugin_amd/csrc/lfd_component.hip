// Connected-component filter on the device (lfd_component_filter): a point of the final cloud is kept iff the connected component
// of the radius graph it belongs to has at least min_points points (lfd_component.hpp has the rule, the walk over a point's candidates and the
// find / union steps, shared with the twin).
//
// Phases, one launch each on the context's stream (lfd_api.hip's lfd_component_filter issues them); the front end - min / max, cell keys, radix
// sort - and the compaction tail are the shared ones, launched as they are:
//
//   lfd_component_gather_kernel    the points in cell order as 16-byte records {x, y, z, input index}; parent[] the identity, the per-root
//                                  counters and the summary cleared
//   lfd_component_link_kernel      the hot path: a lane per sorted point j unites itself with every agreeing q < j
//   lfd_component_flatten_kernel   root[j] = find(j), plain loads in a launch of its own
//   lfd_component_size_kernel      points and smallest input index per root
//   lfd_component_mark_kernel      keep byte, size and label at the point's ORIGINAL index; the 66 summary words from the roots
//
// The link kernel cannot hang: lfd_component.hpp's TERMINATION paragraph is the argument, ComponentAgent below is the memory it runs on.  Per-XCD
// L2s are not coherent with each other and a CU's L1 is never refreshed by another CU's stores, so inside ONE launch a load of parent[] may be
// stale for as long as the launch runs; that is why nothing in it waits for a value to appear.  The hook is a compare-and-swap at agent scope,
// which acts on the one true word; a failed one continues from the value it returned.  The loads are relaxed agent-scope atomics so that stale
// steps are rare, not because anything depends on them.  Across the launch boundary memory is coherent: flatten, size and mark read plainly.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfd_device.hpp"
#include "lfd_component.hpp"

struct ComponentAgent {          // parent[] while other workgroups change it
    static __device__ __forceinline__ uint32_t load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) {
        __hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expect;                                                 // the value the word held: `expect` itself iff the swap happened
    }
    static __device__ __forceinline__ void lower(uint32_t* p, uint32_t v) {
        if (load(p) > v) __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

struct ComponentPlain {          // parent[] of a finished launch
    static __device__ __forceinline__ uint32_t load(const uint32_t* p) { return *p; }
};

extern "C" __global__ void __launch_bounds__(256) lfd_component_gather_kernel(const float* __restrict__ xyz, const unsigned* __restrict__ sorted_idx,
                                                                             long long n, LfdComponentPt* __restrict__ spt,
                                                                             uint32_t* __restrict__ parent, uint32_t* __restrict__ count,
                                                                             uint32_t* __restrict__ first, unsigned long long* __restrict__ summary) {
    if (blockIdx.x == 0 && threadIdx.x < LFD_COMPONENT_SUMMARY) summary[threadIdx.x] = 0ull;
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long long)gridDim.x * 256) {
        const long long i = sorted_idx[j];                             // < n: the sort's payload is a permutation of 0 .. n - 1
        LfdComponentPt p;
        p.x = xyz[3 * i]; p.y = xyz[3 * i + 1]; p.z = xyz[3 * i + 2];
        p.idx = (uint32_t)i;
        spt[j] = p;
        parent[j] = (uint32_t)j;
        count[j] = 0u;
        first[j] = 0xffffffffu;
    }
}

// One lane per sorted point: the lanes of a wave are neighbours in space, their searches take the same turns and their walks read the same lines.
// `mine` follows the root of the lane's own set through the walk, so a candidate that is already in it costs one find and one compare.  Every
// index into parent[] is a sorted position below n: j itself, a q < j of the walk, or a value read from parent[] (all of which are positions).
extern "C" __global__ void __launch_bounds__(256) lfd_component_link_kernel(const unsigned long long* __restrict__ skey,
                                                                           const LfdComponentPt* __restrict__ spt, long long n,
                                                                           unsigned long long e1, unsigned long long e2,
                                                                           unsigned long long sentinel, float r2, uint32_t* parent) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n || skey[j] == sentinel) return;
    uint32_t mine = (uint32_t)j;
    lfd_component_links(skey, spt, j, e1, e2, r2, [&](uint32_t q) { mine = lfd_component_unite<ComponentAgent, true>(parent, mine, q); });
}

extern "C" __global__ void __launch_bounds__(256) lfd_component_flatten_kernel(const uint32_t* __restrict__ parent, long long n,
                                                                              uint32_t* __restrict__ root) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j < n) root[j] = lfd_component_find<ComponentPlain>(parent, (uint32_t)j);
}

#define COMPONENT_WG 256         // lanes of a workgroup of the size kernel: each brings at most one head
#define COMPONENT_SLOTS 512      // of the workgroup's table of roots: twice the roots the lanes can bring, so a probe always meets a free slot
static_assert(COMPONENT_SLOTS >= 2 * COMPONENT_WG && (COMPONENT_SLOTS & (COMPONENT_SLOTS - 1)) == 0 && COMPONENT_SLOTS == 1 << 9,
              "the probe loop of lfd_component_size_kernel ends at a free slot only while the table outnumbers the heads; the hash keeps 9 bits");

// count[r] += the points whose root is r, first[r] = the smallest input index among them.  A cloud that is one sheet sends every point to ONE
// address, so what shares a root is summed on the way: the lanes of a wave over every run of consecutive lanes with one root (a segmented suffix
// reduction, six shuffle steps - the scheme of lfd_far.hip), the heads of the runs into the workgroup's table in LDS, and from there one add and
// one minimum per workgroup and distinct root.  Integer atomics only: nothing depends on the order of arrival.  aggregate = 0 is the plain form,
// one add and one minimum per point, kept for the measurement of DESIGN 4.29.
extern "C" __global__ void __launch_bounds__(COMPONENT_WG) lfd_component_size_kernel(const uint32_t* __restrict__ root, const LfdComponentPt* __restrict__ spt,
                                                                           long long n, int aggregate, uint32_t* __restrict__ count,
                                                                           uint32_t* __restrict__ first) {
    __shared__ uint32_t t_root[COMPONENT_SLOTS], t_cnt[COMPONENT_SLOTS], t_first[COMPONENT_SLOTS];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const long long j = (long long)blockIdx.x * COMPONENT_WG + tid;
    const bool live = j < n;
    uint32_t r = 0xffffffffu, cnt = 0u, low = 0xffffffffu;             // (0xffffffff is no root: a root is a position below n <= 2^31 - 1)
    if (live) { r = root[j]; cnt = 1u; low = spt[j].idx; }
    if (!aggregate) {
        if (live) { atomicAdd(count + r, 1u); atomicMin(first + r, low); }
        return;
    }
    for (int s = tid; s < COMPONENT_SLOTS; s += COMPONENT_WG) { t_root[s] = 0xffffffffu; t_cnt[s] = 0u; t_first[s] = 0xffffffffu; }
    __syncthreads();
    const uint32_t prev = __shfl_up(r, 1, 64);
    const bool head = live && (lane == 0 || prev != r);
    const unsigned long long brk = __ballot(head) | ~__ballot(live);   // lanes at which a run cannot continue
    const unsigned long long above = lane == 63 ? 0ull : brk & ~((2ull << lane) - 1ull);
    const int end = above ? (int)__builtin_ctzll(above) - 1 : 63;      // last lane of this lane's run
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t tc = __shfl_down(cnt, off, 64), tl = __shfl_down(low, off, 64);
        if (lane + off <= end) { cnt += tc; low = tl < low ? tl : low; }
    }
    if (head) {
        // at most COMPONENT_WG heads meet COMPONENT_SLOTS slots (the static_assert above): a free slot is reached within COMPONENT_SLOTS probes, and the loop is bounded by that count
        uint32_t s = (r * 2654435761u) >> 23;                          // 9 bits
        for (int probe = 0; probe < COMPONENT_SLOTS; ++probe, s = (s + 1u) & (COMPONENT_SLOTS - 1)) {
            const uint32_t was = atomicCAS(&t_root[s], 0xffffffffu, r);
            if (was == 0xffffffffu || was == r) {
                atomicAdd(&t_cnt[s], cnt);
                atomicMin(&t_first[s], low);
                break;
            }
        }
    }
    __syncthreads();
    for (int s = tid; s < COMPONENT_SLOTS; s += COMPONENT_WG) {
        const uint32_t tr = t_root[s];                                 // a root: a sorted position below n
        if (tr != 0xffffffffu) { atomicAdd(count + tr, t_cnt[s]); atomicMin(first + tr, t_first[s]); }
    }
}

// keep / size / label of every point at its original index; the lanes that ARE roots bin their component into the workgroup's 66 words in LDS,
// which go out as at most 66 integer atomics per workgroup.  min_points >= 2, size <= n <= 2^31 - 1.
extern "C" __global__ void __launch_bounds__(256) lfd_component_mark_kernel(const uint32_t* __restrict__ root, const LfdComponentPt* __restrict__ spt,
                                                                           const uint32_t* __restrict__ count, const uint32_t* __restrict__ first,
                                                                           long long n, uint32_t min_points, uint8_t* __restrict__ keep,
                                                                           uint32_t* __restrict__ size, uint32_t* __restrict__ label,
                                                                           unsigned long long* __restrict__ summary) {
    __shared__ unsigned long long sh[LFD_COMPONENT_SUMMARY];
    const int tid = (int)threadIdx.x;
    const long long j = (long long)blockIdx.x * 256 + tid;
    if (tid < LFD_COMPONENT_SUMMARY) sh[tid] = 0ull;
    __syncthreads();
    if (j < n) {
        const uint32_t r = root[j], s = count[r];
        const long long i = spt[j].idx;                                // < n
        keep[i] = s >= min_points ? (uint8_t)1 : (uint8_t)0;
        if (size) size[i] = s;
        if (label) label[i] = first[r];
        if (r == (uint32_t)j) {
            const int b = lfd_component_bin(s);
            atomicAdd(&sh[0], 1ull);
            atomicMax(&sh[1], (unsigned long long)s);
            atomicAdd(&sh[2 + b], 1ull);
            atomicAdd(&sh[2 + LFD_COMPONENT_BINS + b], (unsigned long long)s);
        }
    }
    __syncthreads();
    if (tid < LFD_COMPONENT_SUMMARY && sh[tid] != 0ull) {
        if (tid == 1) atomicMax(summary + 1, sh[1]);
        else atomicAdd(summary + tid, sh[tid]);
    }
}
