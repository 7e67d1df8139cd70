// Connected-component filter (lfd_component_filter): what the kernels (lfd_component.hip) and the twin (lfd_host.hip) share - the
// record of a sorted point, the enumeration of a point's candidate links, the find and union steps, the summary's bins, the grid of a call and
// the checks of its arguments.
//
// Two points are LINKED when lfd_consensus_agree holds for them at lfd_consensus_r2(radius) - the consensus filter's own test, called, not
// copied: symmetric bit for bit, a NaN never agrees.  A component is a class of the transitive closure of the links; a point with a
// non-finite coordinate links to nothing.  size(i): points in i's component; label(i): the smallest input index in it; kept iff
// size(i) >= min_points.  The partition of a graph into components does not depend on the order in which its edges are found, so the device,
// the twin and an all-pairs reference agree element for element.
//
// Candidates come from the consensus filter's grid (lfd_consensus_grid, cells of side 1.000001 radius, sorted linear keys): the 27 cells around
// a point's cell are nine key ranges.  A point unites itself only with agreeing points at sorted positions BELOW its own, so every pair is
// tested once; four of the nine ranges hold only larger keys and are never searched.
//
// The forest: parent[] over sorted positions, the identity at the start.  A union hooks the root with the larger position under the smaller
// one, so parent[x] <= x always holds, every walk goes along strictly decreasing positions, and the final root of a component is its smallest
// sorted position.  TERMINATION (the device runs lfd_component_unite from thousands of waves at once, and a load of parent[] may return a value
// that another wave has since replaced): parent[x] only ever changes to a SMALLER MEMBER OF x's OWN TREE (a hook puts a root under another
// root and so merges two trees; a shortening re-parents a position under a smaller member of the tree it is in), and trees only ever merge.
// So whatever a load returns - current or stale - is x itself or a smaller position in the tree x is in now; it need not still lie on x's path
// to the root (another wave may have shortened past it), and nothing needs that.  A stale value costs a step, never the result.
//   find    steps from x to load(parent[x]) only while that is < x: strictly decreasing, at most x steps whatever the loads return
//   unite   compare-and-swaps parent[hi] from hi to lo (lo < hi).  On failure the value that comes back is the true parent[hi], which is < hi;
//           the pair continues as (find(that), lo): its larger member strictly decreases, so at most hi rounds
//   shorten lowers parent[x] to a smaller member of its tree by a minimum: it never raises a value, and never leaves the tree
// No loop's exit waits for another thread's store to become visible; there is no spin, no flag and no barrier across workgroups.
#pragma once

#include "lfd_consensus.hpp"

struct LfdComponentPt {          // one point of the cloud in cell order: a candidate costs the walk one 16-byte load
    float x, y, z;
    uint32_t idx;                // its index in the input
};

#define LFD_COMPONENT_SUMMARY 66     // n_components, largest size, 32 bins of components, 32 bins of their points
#define LFD_COMPONENT_BINS 32

// bin of a component of `size` >= 1 points: b with 2^b <= size < 2^(b + 1)
LFD_HD int lfd_component_bin(uint32_t size) { return 31 - __builtin_clz(size); }

// Every q < j whose point is linked to the point at sorted position j (not a sentinel one), each once: link(q).  skey: the n keys in ascending
// order, spt: the points in that order.  As lfd_consensus_count_point, per (k0 + a, k1 + b) row the cells k2 - 1 .. k2 + 1 are ONE key range -
// one binary search, over the positions below j, then a walk that ends at j.  The rows (a, b) > (0, 0) start above the point's own key (E2 >= 3)
// and hold no position below j.
template <class Link>
LFD_HD void lfd_component_links(const unsigned long long* skey, const LfdComponentPt* spt, long long j, unsigned long long e1,
                                unsigned long long e2, float r2, Link&& link) {
    const LfdComponentPt me = spt[j];
    const unsigned long long key = skey[j];
    for (int a = -1; a <= 0; ++a)
        for (int b = -1; b <= (a < 0 ? 1 : 0); ++b) {
            const long long off = ((long long)a * (long long)e1 + (long long)b) * (long long)e2;
            const unsigned long long lo = key + (unsigned long long)off - 1ull, hi = lo + 2ull;      // k0, k1, k2 >= 1: never below 0
            long long l = 0, h = j;
            while (l < h) {
                const long long mid = (l + h) >> 1;
                if (skey[mid] < lo) l = mid + 1; else h = mid;
            }
            for (long long q = l; q < j; ++q) {
                if (skey[q] > hi) break;
                const LfdComponentPt p = spt[q];
                if (lfd_consensus_agree(me.x, me.y, me.z, p.x, p.y, p.z, r2)) link((uint32_t)q);
            }
        }
}

// Memory operations of the sequential twin (and of any single-threaded caller); the kernels have their own, atomic at agent scope.
struct LfdComponentSeq {
    static LFD_HD uint32_t load(const uint32_t* p) { return *p; }
    static LFD_HD uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) { const uint32_t old = *p; if (old == expect) *p = v; return old; }
    static LFD_HD void lower(uint32_t* p, uint32_t v) { if (v < *p) *p = v; }
};

// the root above x as the loads show it: x itself or a smaller member of x's tree; at most x steps
template <class Mem>
LFD_HD uint32_t lfd_component_find(const uint32_t* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = Mem::load(parent + x);
        if (p >= x) return x;                  // p == x: a root (p > x never happens; taking it for one keeps the walk decreasing regardless)
        x = p;
    }
}

// Joins the sets of a and b and returns the root they now share as this caller saw it (a member of their tree, not above either).  Each round either hooks, finds the
// two already joined, or continues with a strictly smaller larger member.  With SHORTEN the two start positions are pointed at what was found.
template <class Mem, bool SHORTEN>
LFD_HD uint32_t lfd_component_unite(uint32_t* parent, uint32_t a, uint32_t b) {
    const uint32_t a0 = a, b0 = b;
    a = lfd_component_find<Mem>(parent, a);
    b = lfd_component_find<Mem>(parent, b);
    while (a != b) {
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = Mem::cas(parent + hi, hi, lo);
        if (old == hi) { a = b = lo; break; }  // hooked
        a = lfd_component_find<Mem>(parent, old < hi ? old : lo);      // (old < hi always: parent[hi] <= hi and it was not hi)
        b = lo;
    }
    if (SHORTEN) {
        if (a0 != a) Mem::lower(parent + a0, a);
        if (b0 != a) Mem::lower(parent + b0, a);
    }
    return a;
}

// The grid of a call: the consensus filter's, or - no finite point at all - the empty grid whose only key is the sentinel every non-finite
// point gets.  False: lfd_consensus_grid's refusals.
inline bool lfd_component_grid(const float* lo, const float* hi, float radius, LfdConsensusGrid& g) {
    if (lo[0] <= hi[0]) return lfd_consensus_grid(lo, hi, radius, g);
    g.h = 1.000001 * (double)radius;
    for (int c = 0; c < 3; ++c) { g.origin[c] = 0.0; g.e[c] = 1ull; }
    g.sentinel = 1ull;
    g.bits = 1;
    return true;
}

// summary[66] from the components' sizes, one call per component
inline void lfd_component_summary_add(int64_t* summary, uint32_t size) {
    const int b = lfd_component_bin(size);
    summary[0] += 1;
    if ((int64_t)size > summary[1]) summary[1] = (int64_t)size;
    summary[2 + b] += 1;
    summary[2 + LFD_COMPONENT_BINS + b] += (int64_t)size;
}

// What is wrong with the arguments of lfd_component_filter / lfd_component_filter_host (the context apart), or null.  The cloud, the offsets and
// the radius are the consensus filter's and checked by its routine.
inline const char* lfd_component_check(const float* xyz, const float* rgb, const float* err, int64_t n, const int64_t* offs, int32_t n_refs,
                                       float radius, int32_t min_points, const float* xyz_out, const float* rgb_out, const float* err_out,
                                       const int64_t* offs_out, const uint32_t* size, const uint32_t* label, const int64_t* n_out) {
    if (const char* why = lfd_consensus_check(xyz, rgb, err, n, offs, n_refs, radius, 1, xyz_out, rgb_out, err_out, offs_out, nullptr, n_out)) return why;
    if (min_points < 2) return "min_points must be in [2, 2^31 - 1]";
    const struct { const void* p; long long elem; } a[3] = {{xyz, 12}, {rgb, 12}, {err, 4}}, b[2] = {{size, 4}, {label, 4}};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 2; ++j) {
            if (!a[i].p || !b[j].p) continue;
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(a[i].p), a1 = a0 + (uintptr_t)(a[i].elem * n);
            const uintptr_t b0 = reinterpret_cast<uintptr_t>(b[j].p), b1 = b0 + (uintptr_t)(b[j].elem * n);
            if (a0 < b1 && b0 < a1) return "in and out arrays overlap";
        }
    return nullptr;
}
