// CPU twin of the hot path (include/lfd_densify.h, "CPU twin" section): the same per-cell routine as the kernels -
// the HOST build of lfd_geometry.hpp - driven over host arrays by a pool of threads.  It exists for three things:
// upstream's CPU-only configuration (BASELINE config 1: plumbing without a GPU), the `cpu_baseline` leg of bench.py
// (this build's own C++ restatement timed on the host cores) and CPU-side parity tests.  It is never
// reached from a device context and no device entry point falls back to it: a caller opts in with lfd_create_host().
//
// Differences from the device build of the same source, all inside lfd_geometry.hpp's #if blocks: IEEE division and
// square root where the kernels use v_rcp_f32 / v_sqrt_f32 (1 ulp) and a plain 1.0/d where they Newton-refine v_rcp_f64.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "lfd_context.hpp"
#include "lfd_corr.hpp"
#include "lfd_block.hpp"
#include "lfd_head.hpp"
#include "lfd_cycle.hpp"
#include "lfd_support.hpp"
#include "lfd_refine.hpp"
#include "lfd_sigma.hpp"
#include "lfd_normals.hpp"
#include "lfd_colour.hpp"
#include "lfd_photo.hpp"
#include "lfd_gain.hpp"
#include "lfd_far.hpp"
#include "lfd_audit.hpp"
#include "lfd_pose.hpp"
#include "lfd_consensus.hpp"
#include "lfd_component.hpp"
#include "lfd_undistort.hpp"
#include "lfd_freespace.hpp"
#include "lfd_depth.hpp"
#include "lfd_fuse.hpp"
#include "lfd_knn.hpp"
#include "lfd_cap.hpp"
#include "lfd_thin.hpp"

void lfd_fill_kernel_params(const lfd_batch* b, const lfd_params* p, LfdKernelParams& kp);   // lfd_api.hip

namespace {

struct HostRef {             // what block_prologue stages per reference on the device
    LfdRefConst rc;
    LfdPairConst pc[LFD_MAX_SLOTS];
};

struct HostLaunch {
    const lfd_batch* b;
    LfdKernelParams kp;
    std::vector<float> axis_x, axis_y;      // the matcher's linspace when the caller passes none
    const float* ax;
    const float* ay;
    float mask_sx, mask_sy;
    int HW;
    bool exact_colour;
};

}  // namespace

// The host context's worker threads: started once by lfd_create_host, parked on a condition variable between calls, joined by
// lfd_destroy.  A call hands them a chunk count and a function; chunks are claimed with one atomic counter (the calling thread
// works too), so the cost per call is one wake-up instead of n_threads thread creations.
struct LfdHostPool {
    explicit LfdHostPool(int n_threads) {
        const int extra = std::max(0, n_threads - 1);         // the caller is a worker as well
        workers.reserve((size_t)extra);
        for (int t = 0; t < extra; ++t) workers.emplace_back([this]() { loop(); });
    }
    ~LfdHostPool() {
        { std::lock_guard<std::mutex> g(m); stop = true; ++generation; }
        wake.notify_all();
        for (auto& th : workers) th.join();
    }
    void run(int n_chunks, int max_threads, const std::function<void(int)>& fn) {
        if (n_chunks <= 0) return;
        const int helpers = std::min({(int)workers.size(), std::max(0, max_threads - 1), n_chunks - 1});
        if (helpers == 0) { for (int c = 0; c < n_chunks; ++c) fn(c); return; }
        {
            std::lock_guard<std::mutex> g(m);
            job = &fn; total = n_chunks; next.store(0); wanted = helpers; joined = 0; finished = 0; ++generation;
        }
        wake.notify_all();
        for (int c = next.fetch_add(1); c < n_chunks; c = next.fetch_add(1)) fn(c);
        std::unique_lock<std::mutex> g(m);
        wanted = joined;                                      // no late joiner may start on this job any more
        done.wait(g, [this]() { return finished == joined; });
        job = nullptr;
    }

private:
    void loop() {
        unsigned long long seen = 0;
        for (;;) {
            const std::function<void(int)>* fn = nullptr;
            int n = 0;
            {
                std::unique_lock<std::mutex> g(m);
                wake.wait(g, [&]() { return generation != seen; });
                seen = generation;
                if (stop) return;
                if (job == nullptr || joined >= wanted) continue;
                ++joined; fn = job; n = total;
            }
            for (int c = next.fetch_add(1); c < n; c = next.fetch_add(1)) (*fn)(c);
            { std::lock_guard<std::mutex> g(m); ++finished; }
            done.notify_one();
        }
    }
    std::vector<std::thread> workers;
    std::mutex m;
    std::condition_variable wake, done;
    const std::function<void(int)>* job = nullptr;
    std::atomic<int> next{0};
    int total = 0, wanted = 0, joined = 0, finished = 0;
    unsigned long long generation = 0;
    bool stop = false;
};

void lfd_host_pool_destroy(LfdHostPool* p) { delete p; }      // lfd_destroy (lfd_api.hip)

namespace {

template <class Fn>
void parallel_chunks(lfd_context* ctx, int n_chunks, Fn fn) {
    const std::function<void(int)> f(fn);
    if (ctx->host_pool) ctx->host_pool->run(n_chunks, ctx->host_threads, f);
    else for (int c = 0; c < n_chunks; ++c) f(c);
}

int validate_host(lfd_context* ctx, const lfd_batch* b, const lfd_params* p) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    if (!b || !p) return lfd_fail(ctx, LFD_ERR_INVALID, "null batch/params");
    if (ctx->host_cams.empty()) return lfd_fail(ctx, LFD_ERR_STATE, "lfd_upload_cameras must be called first");
    const int n_cams = (int)ctx->host_cams.size();
    if (b->n_refs <= 0) return lfd_fail(ctx, LFD_ERR_INVALID, "n_refs must be > 0");
    if (b->k <= 0 || b->k > LFD_MAX_SLOTS) return lfd_fail(ctx, LFD_ERR_INVALID, "k must be in [1, LFD_MAX_SLOTS]");
    if (b->H <= 0 || b->W <= 0 || b->w_match <= 1 || b->h_match <= 1) return lfd_fail(ctx, LFD_ERR_INVALID, "bad grid / match size");
    if ((long long)b->H * b->W > 0x7fffffffLL) return lfd_fail(ctx, LFD_ERR_INVALID, "grid too large");
    if (b->warp_channels != 2 && b->warp_channels != 4) return lfd_fail(ctx, LFD_ERR_INVALID, "warp_channels must be 2 or 4");
    if (!b->ref_cam || !b->n_slots || !b->nbr_cam || !b->cert || !b->warp || !b->image) return lfd_fail(ctx, LFD_ERR_INVALID, "null table in batch");
    if ((b->axis_x == nullptr) != (b->axis_y == nullptr)) return lfd_fail(ctx, LFD_ERR_INVALID, "axis_x and axis_y must both be given or both be null");
    for (int r = 0; r < b->n_refs; ++r) {
        if (b->ref_cam[r] < 0 || b->ref_cam[r] >= n_cams) return lfd_fail(ctx, LFD_ERR_INVALID, "ref_cam out of range");
        if (b->n_slots[r] < 1 || b->n_slots[r] > b->k) return lfd_fail(ctx, LFD_ERR_INVALID, "n_slots must be in [1, k]");
        if (!b->image[r]) return lfd_fail(ctx, LFD_ERR_INVALID, "null image pointer");
        for (int j = 0; j < b->n_slots[r]; ++j) {
            const size_t s = (size_t)r * b->k + j;
            if (b->nbr_cam[s] < 0 || b->nbr_cam[s] >= n_cams) return lfd_fail(ctx, LFD_ERR_INVALID, "nbr_cam out of range");
            if (!b->cert[s] || !b->warp[s]) return lfd_fail(ctx, LFD_ERR_INVALID, "null cert/warp pointer in a valid slot");
        }
    }
    return LFD_OK;
}

void prepare_host(const lfd_batch* b, const lfd_params* p, HostLaunch& L) {
    L.b = b;
    lfd_fill_kernel_params(b, p, L.kp);
    L.HW = b->H * b->W;
    L.mask_sx = (float)b->w_match / (float)b->W;
    L.mask_sy = (float)b->h_match / (float)b->H;
    L.exact_colour = (p->flags & LFD_FLAG_EXACT_COLOUR) != 0;
    if (b->axis_x) { L.ax = b->axis_x; L.ay = b->axis_y; }
    else {
        L.axis_x.resize((size_t)b->W); L.axis_y.resize((size_t)b->H);
        const LfdAxis ax = lfd_make_axis(b->W), ay = lfd_make_axis(b->H);
        for (int j = 0; j < b->W; ++j) L.axis_x[(size_t)j] = lfd_axis_value(ax, j);
        for (int j = 0; j < b->H; ++j) L.axis_y[(size_t)j] = lfd_axis_value(ay, j);
        L.ax = L.axis_x.data(); L.ay = L.axis_y.data();
    }
}

void make_ref(const lfd_context* ctx, const HostLaunch& L, int r, HostRef& R) {
    const lfd_batch* b = L.b;
    const LfdCam& ca = ctx->host_cams[(size_t)b->ref_cam[r]];
    lfd_make_ref_const(ca, b->w_match, b->h_match, R.rc);
    for (int j = 0; j < b->n_slots[r]; ++j) {
        const size_t s = (size_t)r * b->k + j;
        lfd_make_pair_const(ca, ctx->host_cams[(size_t)b->nbr_cam[s]], b->nbr_cam[s], b->w_match, b->h_match, R.pc[j],
                            b->fundamental ? b->fundamental + s * 9 : nullptr);
    }
}

// certainty of slot j at one cell after the prologue of core/pipeline.py:407-430 (cell_cert of lfd_kernels.hip)
float host_cell_cert(const HostLaunch& L, int r, int j, int cell, int x, int y) {
    const lfd_batch* b = L.b;
    const size_t s = (size_t)r * b->k + j;
    float c = lfd_cert_floor(b->cert[s][cell], L.kp.certainty_thresh);
    const uint8_t* ma = b->mask_a ? b->mask_a[r] : nullptr;
    if (ma) c = c * (float)ma[(size_t)lfd_nearest_src(y, L.mask_sy, b->h_match) * b->w_match + lfd_nearest_src(x, L.mask_sx, b->w_match)];
    const uint8_t* mb = b->mask_b ? b->mask_b[s] : nullptr;
    if (mb) {
        const float* wv = b->warp[s] + (size_t)cell * b->warp_channels + (b->warp_channels - 2);
        const int ix = lfd_grid_nearest(wv[0], b->W), iy = lfd_grid_nearest(wv[1], b->H);
        float m = 0.0f;
        if (ix >= 0 && iy >= 0)
            m = (float)mb[(size_t)lfd_nearest_src(iy, L.mask_sy, b->h_match) * b->w_match + lfd_nearest_src(ix, L.mask_sx, b->w_match)];
        c = c * m;
    }
    return c;
}

// torch.max(dim=0): first maximum wins, a NaN beats any number (first NaN)
void host_cell_best(const HostLaunch& L, int r, int cell, float& best, int& bj) {
    const int y = cell / L.b->W, x = cell - y * L.b->W;
    best = host_cell_cert(L, r, 0, cell, x, y);
    bj = 0;
    for (int j = 1; j < L.b->n_slots[r]; ++j) {
        const float c = host_cell_cert(L, r, j, cell, x, y);
        if ((c > best) || ((c != c) && !(best != best))) { best = c; bj = j; }
    }
}

struct HostPoint { float x, y, z, r, g, b, err; int cell; int slot; };

// one cell through arg-max -> geometry -> colour; returns false when the cell does not survive
bool host_eval_cell(const HostLaunch& L, const HostRef& R, int r, int cell, HostPoint& o, int& bj_out, bool need_weight = false) {
    const lfd_batch* b = L.b;
    float best; int bj;
    host_cell_best(L, r, cell, best, bj);
    bj_out = bj;
    // dense mode: only cells upstream's sampler could ever draw - a weight that is not <= 0 after floor and masks (core/sampling.py:24-27, 41-43 upstream:
    // p = weights / sum, the coverage pass stops at weights <= 0); a masked-out cell is not a candidate.  Indexed mode: the caller selected.
    if (need_weight && best <= 0.0f) return false;
    const float* wp = b->warp[(size_t)r * b->k + bj] + (size_t)cell * b->warp_channels;
    float xan, yan, xbn, ybn;
    if (b->warp_channels == 4) { xan = wp[0]; yan = wp[1]; xbn = wp[2]; ybn = wp[3]; }
    else { const int y = cell / b->W, x = cell - y * b->W; xan = L.ax[x]; yan = L.ay[y]; xbn = wp[0]; ybn = wp[1]; }
    LfdCellResult res;
    lfd_eval_correspondence(R.rc, R.pc[bj], xan, yan, xbn, ybn, L.kp, res);
    if (!res.keep) return false;
    float rgb[3];
    if (L.exact_colour) lfd_bilinear_rgb(b->image[r], b->w_match, b->h_match, res.xa_px, res.ya_px, 1.0f, 1.0f, rgb);
    else lfd_bilinear_rgb_f32(b->image[r], b->w_match, b->h_match, res.xa_px, res.ya_px, rgb);
    o.x = res.x; o.y = res.y; o.z = res.z; o.r = rgb[0]; o.g = rgb[1]; o.b = rgb[2]; o.err = res.err; o.cell = cell; o.slot = bj;
    return true;
}

void store_point(const lfd_points* out, long long pos, const HostPoint& p) {
    if (pos >= out->capacity) return;           // beyond capacity: counted, not written (as on the device)
    out->xyz[pos * 3 + 0] = p.x; out->xyz[pos * 3 + 1] = p.y; out->xyz[pos * 3 + 2] = p.z;
    out->rgb[pos * 3 + 0] = p.r; out->rgb[pos * 3 + 1] = p.g; out->rgb[pos * 3 + 2] = p.b;
    out->err[pos] = p.err;
    if (out->cell) out->cell[pos] = p.cell;
    if (out->slot) out->slot[pos] = (uint8_t)p.slot;
}

int check_host_points(lfd_context* ctx, const lfd_points* out, const int64_t* ref_offsets) {
    if (!out || !out->xyz || !out->rgb || !out->err) return lfd_fail(ctx, LFD_ERR_INVALID, "null output buffers");
    if (out->capacity < 0) return lfd_fail(ctx, LFD_ERR_INVALID, "negative capacity");
    if (!ref_offsets) return lfd_fail(ctx, LFD_ERR_INVALID, "ref_offsets is required");
    return LFD_OK;
}

constexpr int kChunk = 4096;     // cells per work item

// The stable compaction behind a per-point verdict (the three gates' twins): the points i < total with kept(i), in the input order inside and
// across references; ref_offsets_out and the optional per-(reference, winning slot) counts with them.  extra_out (or null): extra_in[i] moves
// with point i.
template <class Kept>
void compact_points(const lfd_batch* b, const lfd_points* in, const long long* offs, long long cap, long long total, Kept kept,
                    const lfd_points* out, int64_t* ref_offsets_out, int32_t* seg_counts_out, const float* extra_in = nullptr,
                    float* extra_out = nullptr) {
    if (seg_counts_out) std::memset(seg_counts_out, 0, sizeof(int32_t) * (size_t)b->n_refs * b->k);
    long long o = 0;
    int r_next = 0;
    for (long long i = 0; i <= total; ++i) {
        while (r_next <= b->n_refs && std::min(lfd_support_clamp(offs[r_next], cap), total) <= i) ref_offsets_out[r_next++] = o;
        if (i == total || !kept(i)) continue;
        for (int e = 0; e < 3; ++e) { out->xyz[3 * o + e] = in->xyz[3 * i + e]; out->rgb[3 * o + e] = in->rgb[3 * i + e]; }
        out->err[o] = in->err[i];
        if (out->cell) out->cell[o] = in->cell[i];
        if (out->slot) out->slot[o] = in->slot[i];
        if (extra_out) extra_out[o] = extra_in[i];
        if (seg_counts_out) {
            const int r = lfd_support_ref_of(offs, b->n_refs, cap, i), s = (int)in->slot[i];
            if (s < b->n_slots[r]) seg_counts_out[(size_t)r * b->k + s] += 1;
        }
        ++o;
    }
    while (r_next <= b->n_refs) ref_offsets_out[r_next++] = o;       // (offsets that do not ascend: whatever is left counts from the end)
}

}  // namespace

extern "C" {

int lfd_create_host(int32_t n_threads, lfd_context** out) {
    if (!out) return lfd_fail(nullptr, LFD_ERR_INVALID, "out is null");
    lfd_context* ctx = new lfd_context();
    ctx->is_host = true;
    const unsigned hw = std::thread::hardware_concurrency();
    ctx->host_threads = n_threads > 0 ? n_threads : (hw ? (int)hw : 1);
    if (ctx->host_threads > 1) ctx->host_pool = new LfdHostPool(ctx->host_threads);
    *out = ctx;
    return LFD_OK;
}

int lfd_host_threads(const lfd_context* ctx) { return (ctx && ctx->is_host) ? ctx->host_threads : 0; }

int lfd_local_corr_host(lfd_context* ctx, const float* A, const float* Bf, const float* warp, int32_t B, int32_t N, int32_t C, int32_t K, int32_t H1,
                        int32_t W1, const int64_t* a_strides, const int64_t* bf_strides, float* out) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    LfdCorrArgs p;
    if (const char* why = lfd_corr_fill(A, Bf, warp, B, N, C, K, H1, W1, a_strides, bf_strides, out, p))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_local_corr_host: ") + why);
    const long long pixels = (long long)B * N;
    if (pixels * K == 0) return LFD_OK;
    const int per = 64;                                           // query pixels per chunk
    parallel_chunks(ctx, (int)((pixels + per - 1) / per), [&](int c) {
        const long long hi = std::min<long long>(pixels, (long long)(c + 1) * per);
        for (long long px = (long long)c * per; px < hi; ++px) {
            const int b = (int)(px / N), n = (int)(px - (long long)b * N);
            for (int k = 0; k < K; ++k) {
                const long long e = px * K + k;
                out[e] = lfd_corr_sample(p.a + b * p.sa_b + n * p.sa_n, p.sa_c, p.bf + b * p.sb_b, p.sb_y, p.sb_x, p.sb_c, C, W1, H1, warp[2 * e], warp[2 * e + 1]);
            }
        }
    });
    return LFD_OK;
}

int lfd_refiner_block_host(lfd_context* ctx, const void* x, int32_t x_is_f32, int32_t B, int32_t C, int32_t H, int32_t W, const float* dw_w,
                           const float* scale, const float* shift, const float* pw_wT, const float* pw_b, uint16_t* out) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    LfdBlockArgs p;
    if (const char* why = lfd_block_fill(x, x_is_f32, B, C, H, W, dw_w, scale, shift, pw_wT, pw_b, out, p))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_refiner_block_host: ") + why);
    // a chunk is one row of one plane (of one image with the pointwise part): every output element is computed by exactly one chunk, from the
    // inputs alone, so the thread count never shows
    const int planes = pw_wT ? B : B * C;                          // planes * H <= B C H W < 2^31
    parallel_chunks(ctx, planes * H, [&](int chunk) {
        const int pl = chunk / H, y = chunk - pl * H;
        const int b = pw_wT ? pl : pl / C, c = pw_wT ? 0 : pl - b * C;
        for (int xx = 0; xx < W; ++xx) lfd_block_pixel(p, b, c, y, xx);
    });
    return LFD_OK;
}

int lfd_refiner_head_host(lfd_context* ctx, const void* z, int32_t z_is_f32, int32_t B, int32_t C, int32_t H, int32_t W, const float* head_w,
                          const float* head_b, const float* prev_warp, const int64_t* prev_warp_strides, const float* prev_conf,
                          const int64_t* prev_conf_strides, int32_t prev_dim, float refine_init, float* warp, float* conf) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    LfdHeadArgs p;
    if (const char* why = lfd_head_fill(z, z_is_f32, B, C, H, W, head_w, head_b, prev_warp, prev_warp_strides, prev_conf, prev_conf_strides, prev_dim,
                                        refine_init, warp, conf, p))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_refiner_head_host: ") + why);
    // a chunk is one row of one image: every output element is computed by exactly one chunk, from the inputs alone, so the thread count never shows
    parallel_chunks(ctx, B * H, [&](int chunk) {                   // B H <= B C H W < 2^31
        const int b = chunk / H, y = chunk - b * H;
        for (int xx = 0; xx < W; ++xx) lfd_head_pixel(p, b, y, xx);
    });
    return LFD_OK;
}

int lfd_cycle_gate_host(lfd_context* ctx, int32_t n_pairs, const float* const* cert, const float* const* warp_ab, const float* const* warp_ba, int32_t H,
                        int32_t W, int32_t warp_channels, int32_t Hb, int32_t Wb, const float* axis_x, const float* axis_y, int32_t w_match,
                        int32_t h_match, float certainty_thresh, float cycle_thresh_px, float* const* cert_out, float* const* err_out,
                        int32_t* rejected) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    LfdCycleArgs p;
    if (const char* why = lfd_cycle_fill(n_pairs, cert, warp_ab, warp_ba, H, W, warp_channels, Hb, Wb, axis_x, axis_y, w_match, h_match,
                                         certainty_thresh, cycle_thresh_px, cert_out, err_out, rejected, p))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_cycle_gate_host: ") + why);
    const int HW = H * W, chunks_per_pair = (HW + kChunk - 1) / kChunk;
    std::vector<int32_t> counts((size_t)n_pairs * chunks_per_pair, 0);
    parallel_chunks(ctx, n_pairs * chunks_per_pair, [&](int c) {
        const int pair = c / chunks_per_pair, c0 = (c - pair * chunks_per_pair) * kChunk, c1 = std::min(c0 + kChunk, HW);
        int32_t n_rejected = 0;
        for (int cell = c0; cell < c1; ++cell) {
            const int y = cell / W, x = cell - y * W;
            const float* wp = p.warp_ab[pair] + (size_t)cell * p.C;
            float xa, ya, xb, yb;
            if (p.C == 4) { xa = wp[0]; ya = wp[1]; xb = wp[2]; yb = wp[3]; }
            else {
                xb = wp[0]; yb = wp[1];
                xa = p.axis_x ? p.axis_x[x] : lfd_axis_value(p.ax, x);
                ya = p.axis_y ? p.axis_y[y] : lfd_axis_value(p.ay, y);
            }
            float d2;
            const bool keep = lfd_cycle_cell(p.warp_ba[pair], Wb, Hb, xa, ya, xb, yb, p.wm1, p.hm1, p.tau2, d2);
            p.cert_out[pair][cell] = keep ? lfd_cert_floor(p.cert[pair][cell], p.certainty_thresh) : 0.0f;
            if (p.err_out[pair]) p.err_out[pair][cell] = sqrtf(d2);
            n_rejected += keep ? 0 : 1;
        }
        counts[(size_t)c] = n_rejected;
    });
    if (rejected)
        for (int c = 0; c < n_pairs * chunks_per_pair; ++c) rejected[c / chunks_per_pair] += counts[(size_t)c];
    return LFD_OK;
}

namespace {

// The slot table of the twins behind triangulation: what lfd_stage_slots stages per reference on the device, for every reference at once.
// slot[r * LFD_MAX_SLOTS + j], j < n_slots[r]; rref[r] (when asked for): the reference's own constants.
void make_slot_table(const lfd_context* ctx, const HostLaunch& L, std::vector<LfdSlot>& slot, std::vector<LfdRefineRef>* rref) {
    const lfd_batch* b = L.b;
    slot.resize((size_t)b->n_refs * LFD_MAX_SLOTS);
    if (rref) rref->resize((size_t)b->n_refs);
    for (int r = 0; r < b->n_refs; ++r) {
        HostRef R;
        make_ref(ctx, L, r, R);
        if (rref) {
            LfdRefineRef& o = (*rref)[(size_t)r];
            for (int e = 0; e < 12; ++e) o.P[e] = R.rc.P[e];
            o.sx = R.rc.sx; o.sy = R.rc.sy;
        }
        for (int j = 0; j < b->n_slots[r]; ++j) {
            const size_t sj = (size_t)r * b->k + j;
            lfd_slot_fill(slot[(size_t)r * LFD_MAX_SLOTS + j], b->cert[sj], b->warp[sj], b->mask_b ? b->mask_b[sj] : nullptr, R.pc[j]);
        }
    }
}

LfdSupportGeom make_geom(const HostLaunch& L, float support_thresh_px, float reproj_thresh) {
    return lfd_support_geom(L.b, L.kp.wm1, L.kp.hm1, L.mask_sx, L.mask_sy, support_thresh_px, reproj_thresh);
}

}  // namespace

int lfd_support_filter_host(lfd_context* ctx, const lfd_batch* b, const lfd_points* in, const int64_t* ref_offsets_in, int32_t min_support,
                            float support_thresh_px, const lfd_points* out, int64_t* ref_offsets_out, int32_t* seg_counts_out, uint8_t* support) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    int code = LFD_ERR_INVALID;
    if (const char* why = lfd_support_check(in, ref_offsets_in, min_support, support_thresh_px, out, ref_offsets_out, &code))
        return lfd_fail(ctx, code, std::string("lfd_support_filter_host: ") + why);
    lfd_params none;
    std::memset(&none, 0, sizeof(none));
    int rc = validate_host(ctx, b, &none);
    if (rc != LFD_OK) return rc;
    HostLaunch L;
    prepare_host(b, &none, L);
    std::vector<LfdSlot> slot;
    make_slot_table(ctx, L, slot, nullptr);
    const LfdSupportGeom g = make_geom(L, support_thresh_px, 0.0f);
    const long long cap = in->capacity;
    const long long* offs = reinterpret_cast<const long long*>(ref_offsets_in);
    const long long total = lfd_support_clamp(offs[b->n_refs], cap);
    std::vector<uint8_t> counts((size_t)total);
    parallel_chunks(ctx, (int)((total + kChunk - 1) / kChunk), [&](int c) {
        const long long i1 = std::min<long long>(total, (long long)(c + 1) * kChunk);
        for (long long i = (long long)c * kChunk; i < i1; ++i) {
            const int r = lfd_support_ref_of(offs, b->n_refs, cap, i);
            const int cell = in->cell[i], s = (int)in->slot[i];
            int n = 0;
            if (cell >= 0 && cell < L.HW) {                             // no address is formed from a cell outside the grid
                const float X0 = in->xyz[3 * i], X1 = in->xyz[3 * i + 1], X2 = in->xyz[3 * i + 2];
                const LfdSlot* sl = &slot[(size_t)r * LFD_MAX_SLOTS];
                for (int j = 0; j < b->n_slots[r]; ++j) {
                    if (j == s) continue;
                    const float* wv = sl[j].warp + (size_t)cell * g.C + (g.C - 2);
                    n += lfd_support_candidate(sl[j], g, sl[j].cert[cell], wv[0], wv[1], X0, X1, X2) ? 1 : 0;
                }
            }
            counts[(size_t)i] = (uint8_t)n;
            if (support) support[i] = (uint8_t)n;
        }
    });
    compact_points(b, in, offs, cap, total, [&](long long i) { return (int)counts[(size_t)i] >= min_support; }, out, ref_offsets_out,
                   seg_counts_out);
    return LFD_OK;
}

// Both re-triangulation twins.  weighted: lfd_refine_multiview_weighted_host (precision checked behind the batch - a null one is refused, not
// taken for the other call -, three counters); otherwise lfd_refine_multiview_host (two).  name: the entry point, for the messages.
static int refine_host_impl(lfd_context* ctx, const char* name, const lfd_batch* b, const lfd_points* in, const int64_t* ref_offsets,
                            float support_thresh_px, float reproj_thresh, float* xyz_out, float* err_out, uint8_t* status, int64_t* counters,
                            const float* const* precision, bool weighted) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    if (const char* why = lfd_refine_check(in, ref_offsets, support_thresh_px, reproj_thresh, xyz_out, err_out, status))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string(name) + ": " + why);
    lfd_params none;
    std::memset(&none, 0, sizeof(none));
    int rc = validate_host(ctx, b, &none);
    if (rc != LFD_OK) return rc;
    if (weighted)
        if (const char* why = lfd_refine_check_precision(b, precision)) return lfd_fail(ctx, LFD_ERR_INVALID, std::string(name) + ": " + why);
    HostLaunch L;
    prepare_host(b, &none, L);
    std::vector<LfdRefineRef> rref;
    std::vector<LfdSlot> rslot;
    make_slot_table(ctx, L, rslot, &rref);
    std::vector<LfdSlotPrec> wslot(weighted ? rslot.size() : 0);
    if (weighted)
        for (int r = 0; r < b->n_refs; ++r)
            for (int j = 0; j < b->n_slots[r]; ++j) {
                LfdSlotPrec& w = wslot[(size_t)r * LFD_MAX_SLOTS + j];
                w.prec = precision[(size_t)r * b->k + j];
                lfd_slot_prec_scale(rslot[(size_t)r * LFD_MAX_SLOTS + j].sx, rslot[(size_t)r * LFD_MAX_SLOTS + j].sy, w);
            }
    const LfdSupportGeom g = make_geom(L, support_thresh_px, reproj_thresh);
    const long long cap = in->capacity;
    const long long* offs = reinterpret_cast<const long long*>(ref_offsets);
    const long long total = lfd_support_clamp(offs[b->n_refs], cap);
    const int n_chunks = (int)((total + kChunk - 1) / kChunk);
    std::vector<long long> count((size_t)n_chunks * 3, 0);             // per chunk: refined, fallen back, solved with weighted rows
    parallel_chunks(ctx, n_chunks, [&](int c) {
        const long long i1 = std::min<long long>(total, (long long)(c + 1) * kChunk);
        for (long long i = (long long)c * kChunk; i < i1; ++i) {
            const int r = lfd_support_ref_of(offs, b->n_refs, cap, i);
            const int cell = in->cell[i], s = (int)in->slot[i], ns = b->n_slots[r];
            float X0 = in->xyz[3 * i], X1 = in->xyz[3 * i + 1], X2 = in->xyz[3 * i + 2], err = in->err[i];
            unsigned st = 0u;
            if (cell >= 0 && cell < L.HW && s < ns) {                   // no address is formed from a cell outside the grid
                const LfdSlot* sl = &rslot[(size_t)r * LFD_MAX_SLOTS];
                const LfdSlotPrec* ws = weighted ? &wslot[(size_t)r * LFD_MAX_SLOTS] : nullptr;
                float cj[LFD_MAX_SLOTS], wx[LFD_MAX_SLOTS], wy[LFD_MAX_SLOTS], q00[LFD_MAX_SLOTS], q01[LFD_MAX_SLOTS], q11[LFD_MAX_SLOTS], qs[3];
                const float* wp = sl[s].warp + (size_t)cell * g.C;
                const float xbn = wp[g.C - 2], ybn = wp[g.C - 1];
                float xan, yan;
                if (g.C == 4) { xan = wp[0]; yan = wp[1]; }
                else { const int y = cell / g.W, x = cell - y * g.W; xan = L.ax[x]; yan = L.ay[y]; }
                if (weighted)
                    for (int e = 0; e < 3; ++e) qs[e] = ws[s].prec[(size_t)cell * 3 + e];
                for (int j = 0; j < LFD_MAX_SLOTS; ++j) {
                    cj[j] = 0.0f; wx[j] = 0.0f; wy[j] = 0.0f; q00[j] = 0.0f; q01[j] = 0.0f; q11[j] = 0.0f;
                    if (j < ns && j != s) {
                        cj[j] = sl[j].cert[cell];
                        const float* wv = sl[j].warp + (size_t)cell * g.C + (g.C - 2);
                        wx[j] = wv[0]; wy[j] = wv[1];
                        if (weighted) {
                            const float* qp = ws[j].prec + (size_t)cell * 3;
                            q00[j] = qp[0]; q01[j] = qp[1]; q11[j] = qp[2];
                        }
                    }
                }
                const LfdRefineGather o = {cj, wx, wy, q00, q01, q11, qs};
                st = weighted ? lfd_refine_point<LFD_MAX_SLOTS, true>(rref[(size_t)r], sl, ws, ns, s, g, xan, yan, xbn, ybn, o, X0, X1, X2, err)
                              : lfd_refine_point<LFD_MAX_SLOTS, false>(rref[(size_t)r], sl, ws, ns, s, g, xan, yan, xbn, ybn, o, X0, X1, X2, err);
            }
            xyz_out[3 * i] = X0; xyz_out[3 * i + 1] = X1; xyz_out[3 * i + 2] = X2;
            err_out[i] = err;
            if (status) status[i] = (uint8_t)st;
            if (st & LFD_REFINE_ACCEPTED) ++count[(size_t)c * 3];
            else if (st) ++count[(size_t)c * 3 + 1];
            if (st & LFD_REFINE_WEIGHTED) ++count[(size_t)c * 3 + 2];
        }
    });
    if (counters)
        for (int c = 0; c < n_chunks; ++c)
            for (int e = 0; e < (weighted ? 3 : 2); ++e) counters[e] += count[(size_t)c * 3 + e];
    return LFD_OK;
}

int lfd_refine_multiview_host(lfd_context* ctx, const lfd_batch* b, const lfd_points* in, const int64_t* ref_offsets, float support_thresh_px,
                              float reproj_thresh, float* xyz_out, float* err_out, uint8_t* status, int64_t* counters) {
    return refine_host_impl(ctx, "lfd_refine_multiview_host", b, in, ref_offsets, support_thresh_px, reproj_thresh, xyz_out, err_out, status,
                            counters, nullptr, false);
}

int lfd_refine_multiview_weighted_host(lfd_context* ctx, const lfd_batch* b, const lfd_points* in, const int64_t* ref_offsets,
                                       float support_thresh_px, float reproj_thresh, float* xyz_out, float* err_out, uint8_t* status,
                                       int64_t* counters, const float* const* precision) {
    return refine_host_impl(ctx, "lfd_refine_multiview_weighted_host", b, in, ref_offsets, support_thresh_px, reproj_thresh, xyz_out, err_out,
                            status, counters, precision, true);
}

// The twin of lfd_estimate_normals: the routine of lfd_normals.hpp per point over host pointers, on the context's threads.
int lfd_estimate_normals_host(lfd_context* ctx, const lfd_batch* b, const lfd_points* in, const int64_t* ref_offsets, int32_t radius_cells,
                              float depth_step_rel, float reproj_thresh, float* normals_out, uint8_t* status, int64_t* counters) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    if (const char* why = lfd_normals_check(in, ref_offsets, radius_cells, depth_step_rel, reproj_thresh, normals_out, status))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_estimate_normals_host: ") + why);
    lfd_params none;
    std::memset(&none, 0, sizeof(none));
    int rc = validate_host(ctx, b, &none);
    if (rc != LFD_OK) return rc;
    HostLaunch L;
    prepare_host(b, &none, L);
    std::vector<HostRef> href((size_t)b->n_refs);
    std::vector<LfdNormalSlot> slot((size_t)b->n_refs * LFD_MAX_SLOTS);
    for (int r = 0; r < b->n_refs; ++r) {
        make_ref(ctx, L, r, href[(size_t)r]);
        for (int j = 0; j < b->n_slots[r]; ++j) {
            const size_t sj = (size_t)r * b->k + j;
            slot[(size_t)r * LFD_MAX_SLOTS + j] = {b->cert[sj], b->warp[sj], b->mask_b ? b->mask_b[sj] : nullptr};
        }
    }
    const LfdSupportGeom g = make_geom(L, 0.0f, reproj_thresh);
    const LfdKernelParams kp = lfd_normal_params(g);
    const long long cap = in->capacity;
    const long long* offs = reinterpret_cast<const long long*>(ref_offsets);
    const long long total = lfd_support_clamp(offs[b->n_refs], cap);
    const int n_chunks = (int)((total + kChunk - 1) / kChunk);
    std::vector<long long> count((size_t)n_chunks * 2, 0);             // per chunk: fitted, fell back
    parallel_chunks(ctx, n_chunks, [&](int c) {
        const long long i1 = std::min<long long>(total, (long long)(c + 1) * kChunk);
        for (long long i = (long long)c * kChunk; i < i1; ++i) {
            const int r = lfd_support_ref_of(offs, b->n_refs, cap, i);
            float nrm[3];
            const unsigned st = lfd_normal_point(href[(size_t)r].rc, href[(size_t)r].pc, &slot[(size_t)r * LFD_MAX_SLOTS], b->n_slots[r],
                                                 b->mask_a ? b->mask_a[r] : nullptr, L.ax, L.ay, g, kp, radius_cells, depth_step_rel, in->cell[i],
                                                 (int)in->slot[i], in->xyz[3 * i], in->xyz[3 * i + 1], in->xyz[3 * i + 2], nrm);
            normals_out[3 * i] = nrm[0]; normals_out[3 * i + 1] = nrm[1]; normals_out[3 * i + 2] = nrm[2];
            if (status) status[i] = (uint8_t)st;
            ++count[(size_t)c * 2 + ((st & LFD_NORMAL_FITTED) ? 0 : 1)];
        }
    });
    if (counters)
        for (int c = 0; c < n_chunks; ++c)
            for (int e = 0; e < 2; ++e) counters[e] += count[(size_t)c * 2 + e];
    return LFD_OK;
}

// The twin of lfd_colour_multiview: the routine of lfd_colour.hpp per point over host pointers, on the context's threads.
int lfd_colour_multiview_host(lfd_context* ctx, const lfd_batch* b, const lfd_points* in, const int64_t* ref_offsets,
                              const uint8_t* const* nbr_image, float support_thresh_px, int32_t mode, float* rgb_out, uint8_t* status,
                              int64_t* counters) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    if (const char* why = lfd_colour_check(in, ref_offsets, nbr_image, support_thresh_px, mode, rgb_out, status))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_colour_multiview_host: ") + why);
    lfd_params none;
    std::memset(&none, 0, sizeof(none));
    int rc = validate_host(ctx, b, &none);
    if (rc != LFD_OK) return rc;
    if (const char* why = lfd_colour_check_images(b, nbr_image)) return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_colour_multiview_host: ") + why);
    HostLaunch L;
    prepare_host(b, &none, L);
    std::vector<LfdSlot> slot;
    make_slot_table(ctx, L, slot, nullptr);
    const LfdSupportGeom g = make_geom(L, support_thresh_px, 0.0f);
    const long long cap = in->capacity;
    const long long* offs = reinterpret_cast<const long long*>(ref_offsets);
    const long long total = lfd_support_clamp(offs[b->n_refs], cap);
    const int n_chunks = (int)((total + kChunk - 1) / kChunk);
    std::vector<long long> count((size_t)n_chunks * 2, 0);             // per chunk: points blended, the sum of their n
    parallel_chunks(ctx, n_chunks, [&](int c) {
        const long long i1 = std::min<long long>(total, (long long)(c + 1) * kChunk);
        for (long long i = (long long)c * kChunk; i < i1; ++i) {
            const int r = lfd_support_ref_of(offs, b->n_refs, cap, i);
            const int cell = in->cell[i], s = (int)in->slot[i], ns = b->n_slots[r];
            const float X0 = in->xyz[3 * i], X1 = in->xyz[3 * i + 1], X2 = in->xyz[3 * i + 2];
            float rgb[3] = {in->rgb[3 * i], in->rgb[3 * i + 1], in->rgb[3 * i + 2]};
            unsigned n = 0u;
            if (lfd_colour_guarded(X0, X1, X2, rgb[0], rgb[1], rgb[2], cell, L.HW, s, ns)) {
                if (rgb_out != in->rgb) std::memcpy(rgb_out + 3 * i, in->rgb + 3 * i, 3 * sizeof(float));      // bit for bit
            } else {
                const LfdSlot* sl = &slot[(size_t)r * LFD_MAX_SLOTS];
                float cj[LFD_MAX_SLOTS], wx[LFD_MAX_SLOTS], wy[LFD_MAX_SLOTS];
                for (int j = 0; j < LFD_MAX_SLOTS; ++j) {
                    cj[j] = 0.0f; wx[j] = 0.0f; wy[j] = 0.0f;
                    if (j < ns && j != s) {
                        const float* wv = sl[j].warp + (size_t)cell * g.C + (g.C - 2);
                        cj[j] = sl[j].cert[cell]; wx[j] = wv[0]; wy[j] = wv[1];
                    }
                }
                const float* ws = sl[s].warp + (size_t)cell * g.C + (g.C - 2);
                const uint8_t* const* img = nbr_image + (size_t)r * b->k;
                n = mode == LFD_COLOUR_MEAN
                        ? lfd_colour_point<LFD_MAX_SLOTS, LFD_COLOUR_MEAN>(sl, img, ns, s, g, cj, wx, wy, ws[0], ws[1], X0, X1, X2, rgb)
                        : lfd_colour_point<LFD_MAX_SLOTS, LFD_COLOUR_MEDIAN>(sl, img, ns, s, g, cj, wx, wy, ws[0], ws[1], X0, X1, X2, rgb);
                rgb_out[3 * i] = rgb[0]; rgb_out[3 * i + 1] = rgb[1]; rgb_out[3 * i + 2] = rgb[2];
                count[(size_t)c * 2] += 1;
                count[(size_t)c * 2 + 1] += n;
            }
            if (status) status[i] = (uint8_t)n;
        }
    });
    if (counters)
        for (int c = 0; c < n_chunks; ++c)
            for (int e = 0; e < 2; ++e) counters[e] += count[(size_t)c * 2 + e];
    return LFD_OK;
}

// The twin of lfd_gain_accumulate: the routine of lfd_gain.hpp per (point, slot) over host pointers, on the context's threads.
// A chunk keeps the sums of the reference it is in and adds them to the table when the reference changes: integer additions, order-free.
int lfd_gain_accumulate_host(lfd_context* ctx, const lfd_batch* b, const lfd_points* in, const int64_t* ref_offsets,
                             const uint8_t* const* nbr_image, float support_thresh_px, uint64_t* table) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    if (const char* why = lfd_gain_check(in, ref_offsets, nbr_image, support_thresh_px, table, 0))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_gain_accumulate_host: ") + why);
    lfd_params none;
    std::memset(&none, 0, sizeof(none));
    int rc = validate_host(ctx, b, &none);
    if (rc != LFD_OK) return rc;
    if (const char* why = lfd_gain_check(in, ref_offsets, nbr_image, support_thresh_px, table, (long long)b->n_refs * b->k))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_gain_accumulate_host: ") + why);
    if (const char* why = lfd_colour_check_images(b, nbr_image)) return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_gain_accumulate_host: ") + why);
    HostLaunch L;
    prepare_host(b, &none, L);
    std::vector<LfdSlot> slot;
    make_slot_table(ctx, L, slot, nullptr);
    const LfdSupportGeom g = make_geom(L, support_thresh_px, 0.0f);
    const long long cap = in->capacity;
    const long long* offs = reinterpret_cast<const long long*>(ref_offsets);
    const long long total = lfd_support_clamp(offs[b->n_refs], cap);
    const int n_chunks = (int)((total + kChunk - 1) / kChunk);
    parallel_chunks(ctx, n_chunks, [&](int c) {
        uint64_t acc[LFD_MAX_SLOTS * LFD_GAIN_QUANTITIES];
        int cur = -1;
        auto flush = [&]() {
            if (cur < 0) return;
            for (int t = 0; t < b->k * LFD_GAIN_QUANTITIES; ++t)
                if (acc[t]) __atomic_fetch_add(&table[(size_t)cur * b->k * LFD_GAIN_QUANTITIES + t], acc[t], __ATOMIC_RELAXED);
        };
        const long long i1 = std::min<long long>(total, (long long)(c + 1) * kChunk);
        for (long long i = (long long)c * kChunk; i < i1; ++i) {
            const int r = lfd_support_ref_of(offs, b->n_refs, cap, i);
            if (r != cur) {
                flush();
                cur = r;
                std::memset(acc, 0, sizeof(acc));
            }
            const int cell = in->cell[i], s = (int)in->slot[i], ns = b->n_slots[r];
            const float X0 = in->xyz[3 * i], X1 = in->xyz[3 * i + 1], X2 = in->xyz[3 * i + 2];
            const float rgb[3] = {in->rgb[3 * i], in->rgb[3 * i + 1], in->rgb[3 * i + 2]};
            if (lfd_colour_guarded(X0, X1, X2, rgb[0], rgb[1], rgb[2], cell, L.HW, s, ns)) continue;
            const bool ref_ok = lfd_gain_in_range(rgb[0]) && lfd_gain_in_range(rgb[1]) && lfd_gain_in_range(rgb[2]);
            if (!ref_ok) continue;
            const uint32_t qr[3] = {lfd_gain_quantise(rgb[0]), lfd_gain_quantise(rgb[1]), lfd_gain_quantise(rgb[2])};
            const LfdSlot* sl = &slot[(size_t)r * LFD_MAX_SLOTS];
            const uint8_t* const* img = nbr_image + (size_t)r * b->k;
            for (int j = 0; j < ns; ++j) {
                const float* wv = sl[j].warp + (size_t)cell * g.C + (g.C - 2);
                uint32_t q[3];
                if (!lfd_gain_sample(sl[j], img[j], g, j == s, ref_ok, sl[j].cert[cell], wv[0], wv[1], X0, X1, X2, q)) continue;
                uint64_t* a = acc + j * LFD_GAIN_QUANTITIES;
                a[0] += 1;
                for (int e = 0; e < 3; ++e) { a[1 + e] += qr[e]; a[4 + e] += q[e]; }
            }
        }
        flush();
    });
    return LFD_OK;
}

// The twin of lfd_gain_apply: lfd_gain_value per colour value, the same bits.
int lfd_gain_apply_host(lfd_context* ctx, const float* rgb, int64_t n, const int64_t* ref_offsets, int32_t n_refs, const float* factors,
                        float* rgb_out) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    if (const char* why = lfd_gain_apply_check(rgb, n, ref_offsets, n_refs, factors, rgb_out))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_gain_apply_host: ") + why);
    const long long* offs = reinterpret_cast<const long long*>(ref_offsets);
    const long long total = lfd_support_clamp(offs[n_refs], n);
    const int n_chunks = (int)((total + kChunk - 1) / kChunk);
    parallel_chunks(ctx, n_chunks, [&](int c) {
        const long long i1 = std::min<long long>(total, (long long)(c + 1) * kChunk);
        for (long long i = (long long)c * kChunk; i < i1; ++i) {
            const int r = lfd_support_ref_of(offs, n_refs, n, i);
            for (int ch = 0; ch < 3; ++ch) {
                const float v = lfd_gain_value(rgb[3 * i + ch], factors[3 * r + ch]);
                std::memcpy(rgb_out + 3 * i + ch, &v, sizeof(float));                       // (bit for bit, a NaN's payload included)
            }
        }
    });
    return LFD_OK;
}

// The twin of lfd_epipolar_audit: lfd_audit_bin per confident (cell, slot) over host pointers, on the context's threads.  A chunk
// counts into a table of its own and adds the non-zero entries with relaxed atomic adds: integer additions, order-free.
int lfd_epipolar_audit_host(lfd_context* ctx, const lfd_batch* b, float audit_certainty, uint64_t* table, uint8_t* best) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    if (const char* why = lfd_audit_check(audit_certainty, table)) return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_epipolar_audit_host: ") + why);
    lfd_params none;
    std::memset(&none, 0, sizeof(none));
    int rc = validate_host(ctx, b, &none);
    if (rc != LFD_OK) return rc;
    if (const char* why = lfd_audit_check_batch(b, table, best)) return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_epipolar_audit_host: ") + why);
    HostLaunch L;
    prepare_host(b, &none, L);
    std::vector<LfdSlot> slot;
    make_slot_table(ctx, L, slot, nullptr);
    std::vector<double> Fs((size_t)b->n_refs * LFD_MAX_SLOTS * 9, 0.0);
    for (int r = 0; r < b->n_refs; ++r) {
        HostRef R;
        make_ref(ctx, L, r, R);
        for (int j = 0; j < b->n_slots[r]; ++j)
            for (int e = 0; e < 9; ++e) Fs[((size_t)r * LFD_MAX_SLOTS + j) * 9 + e] = R.pc[j].F[e];
    }
    const LfdSupportGeom g = make_geom(L, 0.0f, 0.0f);
    const int chunks_per_ref = (L.HW + kChunk - 1) / kChunk;
    parallel_chunks(ctx, b->n_refs * chunks_per_ref, [&](int c) {
        const int r = c / chunks_per_ref, c0 = (c - r * chunks_per_ref) * kChunk, c1 = std::min(L.HW, c0 + kChunk);
        const LfdCam& cam = ctx->host_cams[(size_t)b->ref_cam[r]];
        LfdRefConst rcst;
        lfd_make_ref_const(cam, b->w_match, b->h_match, rcst);
        const int ns = b->n_slots[r];
        const LfdSlot* sl = &slot[(size_t)r * LFD_MAX_SLOTS];
        const uint8_t* ma = b->mask_a ? b->mask_a[r] : nullptr;
        uint64_t local[LFD_MAX_SLOTS * LFD_AUDIT_QUANTITIES];
        std::memset(local, 0, sizeof(local));
        for (int cell = c0; cell < c1; ++cell) {
            const int y = cell / b->W, x = cell - y * b->W;
            int bst = LFD_AUDIT_NONE;
            const bool ok = !ma || ma[(size_t)lfd_nearest_src(y, g.mask_sy, g.h_match) * g.w_match + lfd_nearest_src(x, g.mask_sx, g.w_match)] != 0;
            if (ok && ns > 0) {
                float xan, yan;
                if (g.C == 4) { const float* a = sl[0].warp + (size_t)cell * 4; xan = a[0]; yan = a[1]; }
                else { xan = L.ax[x]; yan = L.ay[y]; }
                for (int j = 0; j < ns; ++j) {
                    const float* wv = sl[j].warp + (size_t)cell * g.C + (g.C - 2);
                    if (!lfd_far_confident(sl[j], g, audit_certainty, sl[j].cert[cell], wv[0], wv[1])) continue;
                    const int bin = lfd_audit_bin(&Fs[((size_t)r * LFD_MAX_SLOTS + j) * 9], rcst.sx, rcst.sy, sl[j].sx, sl[j].sy, xan, yan, wv[0], wv[1],
                                                  g.wm1, g.hm1);
                    uint64_t* row = local + (size_t)j * LFD_AUDIT_QUANTITIES;
                    if (bin < 0) { ++row[1]; continue; }
                    ++row[0]; ++row[2 + bin];
                    bst = bin < bst ? bin : bst;
                }
            }
            if (best) best[(size_t)r * L.HW + cell] = (uint8_t)bst;
        }
        for (int i = 0; i < ns * LFD_AUDIT_QUANTITIES; ++i)
            if (local[i]) __atomic_fetch_add(table + (size_t)r * b->k * LFD_AUDIT_QUANTITIES + i, local[i], __ATOMIC_RELAXED);
    });
    return LFD_OK;
}

// The twin of lfd_pose_accumulate: lfd_pose_sample per confident (cell, slot) over host pointers, on the context's threads.  A
// chunk sums into a table of its own and adds the non-zero entries with relaxed atomic adds: integer additions, order-free.
int lfd_pose_accumulate_host(lfd_context* ctx, const lfd_batch* b, float pose_certainty, float pose_inlier_px, int64_t* table) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    if (const char* why = lfd_pose_check(pose_certainty, pose_inlier_px, table))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_pose_accumulate_host: ") + why);
    lfd_params none;
    std::memset(&none, 0, sizeof(none));
    int rc = validate_host(ctx, b, &none);
    if (rc != LFD_OK) return rc;
    if (const char* why = lfd_pose_check_batch(b, table)) return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_pose_accumulate_host: ") + why);
    HostLaunch L;
    prepare_host(b, &none, L);
    std::vector<LfdSlot> slot;
    make_slot_table(ctx, L, slot, nullptr);
    std::vector<LfdPoseConst> pcs((size_t)b->n_refs * LFD_MAX_SLOTS);
    for (int r = 0; r < b->n_refs; ++r)
        for (int j = 0; j < b->n_slots[r]; ++j)
            lfd_pose_make_const(ctx->host_cams[(size_t)b->ref_cam[r]], ctx->host_cams[(size_t)b->nbr_cam[(size_t)r * b->k + j]],
                                pcs[(size_t)r * LFD_MAX_SLOTS + j]);
    const LfdSupportGeom g = make_geom(L, 0.0f, 0.0f);
    const double c2 = (double)pose_inlier_px * (double)pose_inlier_px;
    const int chunks_per_ref = (L.HW + kChunk - 1) / kChunk;
    uint64_t* utable = reinterpret_cast<uint64_t*>(table);
    parallel_chunks(ctx, b->n_refs * chunks_per_ref, [&](int c) {
        const int r = c / chunks_per_ref, c0 = (c - r * chunks_per_ref) * kChunk, c1 = std::min(L.HW, c0 + kChunk);
        const LfdCam& cam = ctx->host_cams[(size_t)b->ref_cam[r]];
        LfdRefConst rcst;
        lfd_make_ref_const(cam, b->w_match, b->h_match, rcst);
        const int ns = b->n_slots[r];
        const LfdSlot* sl = &slot[(size_t)r * LFD_MAX_SLOTS];
        const uint8_t* ma = b->mask_a ? b->mask_a[r] : nullptr;
        uint64_t local[LFD_MAX_SLOTS * LFD_POSE_QUANTITIES];
        std::memset(local, 0, sizeof(local));
        for (int cell = c0; cell < c1; ++cell) {
            const int y = cell / b->W, x = cell - y * b->W;
            const bool ok = !ma || ma[(size_t)lfd_nearest_src(y, g.mask_sy, g.h_match) * g.w_match + lfd_nearest_src(x, g.mask_sx, g.w_match)] != 0;
            if (!ok || ns <= 0) continue;
            float xan, yan;
            if (g.C == 4) { const float* a = sl[0].warp + (size_t)cell * 4; xan = a[0]; yan = a[1]; }
            else { xan = L.ax[x]; yan = L.ay[y]; }
            for (int j = 0; j < ns; ++j) {
                const float* wv = sl[j].warp + (size_t)cell * g.C + (g.C - 2);
                if (!lfd_far_confident(sl[j], g, pose_certainty, sl[j].cert[cell], wv[0], wv[1])) continue;
                int32_t q[7];
                const int kind = lfd_pose_sample(pcs[(size_t)r * LFD_MAX_SLOTS + j], rcst.sx, rcst.sy, sl[j].sx, sl[j].sy, xan, yan, wv[0], wv[1], g.wm1,
                                                 g.hm1, c2, q);
                uint64_t* row = local + (size_t)j * LFD_POSE_QUANTITIES;
                ++row[kind];                                           // columns 0 / 1 / 2: inliers, outliers, degenerate
                if (kind != LFD_POSE_INLIER) continue;
                for (int e = 0; e < LFD_POSE_SUMS; ++e) row[3 + e] += (uint64_t)lfd_pose_term(q, e);      // (two's complement)
            }
        }
        for (int i = 0; i < ns * LFD_POSE_QUANTITIES; ++i)
            if (local[i]) __atomic_fetch_add(utable + (size_t)r * b->k * LFD_POSE_QUANTITIES + i, local[i], __ATOMIC_RELAXED);
    });
    return LFD_OK;
}

// The twin of lfd_far_accumulate: the routines of lfd_far.hpp per cell over host pointers, on the context's threads.  A chunk adds
// each far cell's seven integers to the table with relaxed atomic adds: integer additions, order-free.
int lfd_far_accumulate_host(lfd_context* ctx, const lfd_batch* b, float far_thresh_px, float far_certainty, int32_t far_min_views,
                            int32_t shell_cells, uint64_t* table, int64_t* counters) {
    return lfd_far_accumulate_flags_host(ctx, b, far_thresh_px, far_certainty, far_min_views, shell_cells, table, counters, nullptr);
}

int lfd_far_accumulate_flags_host(lfd_context* ctx, const lfd_batch* b, float far_thresh_px, float far_certainty, int32_t far_min_views,
                                  int32_t shell_cells, uint64_t* table, int64_t* counters, uint8_t* flags) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    if (const char* why = lfd_far_check(far_thresh_px, far_certainty, far_min_views, shell_cells, table))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_far_accumulate_host: ") + why);
    lfd_params none;
    std::memset(&none, 0, sizeof(none));
    int rc = validate_host(ctx, b, &none);
    if (rc != LFD_OK) return rc;
    if (const char* why = lfd_far_check_batch(b, shell_cells, table, counters, flags))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_far_accumulate_host: ") + why);
    if (b->n_refs > 65535) return lfd_fail(ctx, LFD_ERR_INVALID, "lfd_far_accumulate_host: at most 65535 references per batch");
    HostLaunch L;
    prepare_host(b, &none, L);
    std::vector<LfdSlot> slot;
    make_slot_table(ctx, L, slot, nullptr);
    const LfdSupportGeom g = make_geom(L, far_thresh_px, 0.0f);
    const int chunks_per_ref = (L.HW + kChunk - 1) / kChunk;
    if (flags) std::memset(flags, 0, (size_t)b->n_refs * L.HW);
    parallel_chunks(ctx, b->n_refs * chunks_per_ref, [&](int c) {
        const int r = c / chunks_per_ref, c0 = (c - r * chunks_per_ref) * kChunk, c1 = std::min(L.HW, c0 + kChunk);
        const LfdCam& cam = ctx->host_cams[(size_t)b->ref_cam[r]];
        LfdRefConst rcst;
        lfd_make_ref_const(cam, b->w_match, b->h_match, rcst);
        float M[9];
        lfd_far_dir_matrix(cam, M);
        const int ns = b->n_slots[r];
        const LfdSlot* sl = &slot[(size_t)r * LFD_MAX_SLOTS];
        const uint8_t* ma = b->mask_a ? b->mask_a[r] : nullptr;
        long long n_far = 0;
        for (int cell = c0; cell < c1; ++cell) {
            const int y = cell / b->W, x = cell - y * b->W;
            if (ma && ma[(size_t)lfd_nearest_src(y, g.mask_sy, g.h_match) * g.w_match + lfd_nearest_src(x, g.mask_sx, g.w_match)] == 0) continue;
            float xan, yan, d[3];
            if (g.C == 4) { const float* a = sl[0].warp + (size_t)cell * 4; xan = a[0]; yan = a[1]; }
            else { xan = L.ax[x]; yan = L.ay[y]; }
            lfd_far_direction(M, rcst.sx, rcst.sy, xan, yan, g.wm1, g.hm1, d);
            int n_conf = 0, n_agree = 0;
            for (int j = 0; j < ns; ++j) {
                const float* wv = sl[j].warp + (size_t)cell * g.C + (g.C - 2);
                const int v = lfd_far_slot(sl[j], g, far_certainty, sl[j].cert[cell], wv[0], wv[1], d[0], d[1], d[2]);
                n_conf += v & 1; n_agree += v >> 1;
            }
            if (!lfd_far_verdict(n_conf, n_agree, far_min_views, ns)) continue;
            long long key, q[3];
            if (!lfd_far_key(d[0], d[1], d[2], shell_cells, &key, q)) continue;
            float rgb[3];
            lfd_bilinear_rgb_f32(b->image[r], b->w_match, b->h_match, lfd_match_px(xan, g.wm1), lfd_match_px(yan, g.hm1), rgb);
            uint64_t* row = table + (size_t)key * LFD_FAR_QUANTITIES;
            for (int e = 0; e < 3; ++e) {
                __atomic_fetch_add(row + e, (uint64_t)q[e], __ATOMIC_RELAXED);
                __atomic_fetch_add(row + 3 + e, (uint64_t)lfd_quantise_u8(rgb[e]), __ATOMIC_RELAXED);
            }
            __atomic_fetch_add(row + 6, (uint64_t)1, __ATOMIC_RELAXED);
            if (flags) flags[(size_t)r * L.HW + cell] = 1;
            ++n_far;
        }
        if (counters && n_far) __atomic_fetch_add(counters + r, (int64_t)n_far, __ATOMIC_RELAXED);
    });
    return LFD_OK;
}

// The twin of lfd_far_emit: lfd_far_kept / lfd_far_record per direction cell in key order, the same bits.
int lfd_far_emit_host(lfd_context* ctx, const uint64_t* table, int32_t shell_cells, int64_t min_samples, const double* centre, double radius,
                      float* xyz, float* rgb, float* normal, int32_t* samples, int64_t capacity, int64_t* n_out) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    if (const char* why = lfd_far_emit_check(table, shell_cells, min_samples, centre, radius, xyz, rgb, normal, samples, capacity, n_out))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_far_emit_host: ") + why);
    const long long n_cells = 6LL * shell_cells * shell_cells;
    long long o = 0;
    for (long long i = 0; i < n_cells; ++i) {
        const uint64_t* row = table + i * LFD_FAR_QUANTITIES;
        if (!lfd_far_kept(row, (long long)min_samples)) continue;
        if (o < capacity) lfd_far_record(row, centre, radius, xyz + 3 * o, rgb + 3 * o, normal ? normal + 3 * o : nullptr, samples ? samples + o : nullptr);
        ++o;
    }
    *n_out = o;
    if (o > capacity) return lfd_fail(ctx, LFD_ERR_CAPACITY, "lfd_far_emit_host: the shell has more points than capacity (n_out holds the number)");
    return LFD_OK;
}

// The twin of lfd_photo_gate: lfd_photo_point per point over host pointers on the context's threads, then the support filter's
// stable compaction.
int lfd_photo_gate_host(lfd_context* ctx, const lfd_batch* b, const lfd_points* in, const int64_t* ref_offsets_in,
                        const uint8_t* const* nbr_image, int32_t window_cells, float min_ncc, float min_texture, const lfd_points* out,
                        int64_t* ref_offsets_out, int32_t* seg_counts_out, uint8_t* status, float* ncc, int64_t* counters) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    int code = LFD_ERR_INVALID;
    if (const char* why = lfd_photo_check(in, ref_offsets_in, nbr_image, window_cells, min_ncc, min_texture, out, ref_offsets_out, status, ncc,
                                          counters, &code))
        return lfd_fail(ctx, code, std::string("lfd_photo_gate_host: ") + why);
    lfd_params none;
    std::memset(&none, 0, sizeof(none));
    int rc = validate_host(ctx, b, &none);
    if (rc != LFD_OK) return rc;
    if (const char* why = lfd_colour_check_images(b, nbr_image)) return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_photo_gate_host: ") + why);
    HostLaunch L;
    prepare_host(b, &none, L);
    std::vector<LfdPhotoSlot> slot((size_t)b->n_refs * LFD_MAX_SLOTS);
    for (int r = 0; r < b->n_refs; ++r)
        for (int j = 0; j < b->n_slots[r]; ++j) {
            const size_t sj = (size_t)r * b->k + j;
            slot[(size_t)r * LFD_MAX_SLOTS + j] = {b->cert[sj], b->warp[sj], b->mask_b ? b->mask_b[sj] : nullptr, nbr_image[sj]};
        }
    const LfdSupportGeom g = make_geom(L, 0.0f, 0.0f);
    const LfdPhotoThresh th = lfd_photo_thresholds(min_ncc, min_texture);
    const long long cap = in->capacity;
    const long long* offs = reinterpret_cast<const long long*>(ref_offsets_in);
    const long long total = lfd_support_clamp(offs[b->n_refs], cap);
    const int n_chunks = (int)((total + kChunk - 1) / kChunk);
    std::vector<uint8_t> st((size_t)total);
    std::vector<long long> count((size_t)n_chunks * LFD_PHOTO_STATUSES, 0);
    parallel_chunks(ctx, n_chunks, [&](int c) {
        const long long i1 = std::min<long long>(total, (long long)(c + 1) * kChunk);
        for (long long i = (long long)c * kChunk; i < i1; ++i) {
            const int r = lfd_support_ref_of(offs, b->n_refs, cap, i);
            float v;
            const unsigned s = lfd_photo_point(&slot[(size_t)r * LFD_MAX_SLOTS], b->n_slots[r], b->image[r], b->mask_a ? b->mask_a[r] : nullptr,
                                               L.ax, L.ay, g, window_cells, th, in->cell[i], (int)in->slot[i], &v);
            st[(size_t)i] = (uint8_t)s;
            if (status) status[i] = (uint8_t)s;
            if (ncc) ncc[i] = v;
            ++count[(size_t)c * LFD_PHOTO_STATUSES + s];
        }
    });
    if (counters)
        for (int c = 0; c < n_chunks; ++c)
            for (int e = 0; e < LFD_PHOTO_STATUSES; ++e) counters[e] += count[(size_t)c * LFD_PHOTO_STATUSES + e];
    compact_points(b, in, offs, cap, total, [&](long long i) { return st[(size_t)i] != LFD_PHOTO_REFUTED; }, out, ref_offsets_out, seg_counts_out);
    return LFD_OK;
}

// The twin of lfd_depth_sigma_filter: lfd_sigma_point per point on the context's threads, then the stable compaction.
int lfd_depth_sigma_filter_host(lfd_context* ctx, const lfd_batch* b, const lfd_points* in, const int64_t* ref_offsets_in,
                                const float* const* precision, float iso_sigma_px, const uint8_t* refine_status, float support_thresh_px,
                                float max_rel_sigma, const lfd_points* out, int64_t* ref_offsets_out, int32_t* seg_counts_out, float* sigma_rel,
                                float* sigma_rel_out) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    int code = LFD_ERR_INVALID;
    if (const char* why = lfd_sigma_check(in, ref_offsets_in, precision, iso_sigma_px, refine_status, support_thresh_px, max_rel_sigma, out,
                                          ref_offsets_out, sigma_rel, sigma_rel_out, &code))
        return lfd_fail(ctx, code, std::string("lfd_depth_sigma_filter_host: ") + why);
    lfd_params none;
    std::memset(&none, 0, sizeof(none));
    int rc = validate_host(ctx, b, &none);
    if (rc != LFD_OK) return rc;
    const bool planes = precision != nullptr;
    if (planes)
        if (const char* why = lfd_refine_check_precision(b, precision))
            return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_depth_sigma_filter_host: ") + why);
    HostLaunch L;
    prepare_host(b, &none, L);
    std::vector<LfdSlot> rslot;
    make_slot_table(ctx, L, rslot, nullptr);
    std::vector<LfdSigmaRef> rref((size_t)b->n_refs);
    for (int r = 0; r < b->n_refs; ++r) {
        const LfdCam& ca = ctx->host_cams[(size_t)b->ref_cam[r]];
        for (int e = 0; e < 3; ++e) rref[(size_t)r].C[e] = ca.C[e];    // LfdRefConst::C (lfd_make_ref_const)
    }
    std::vector<LfdSlotPrec> wslot(rslot.size());
    if (planes)
        for (int r = 0; r < b->n_refs; ++r)
            for (int j = 0; j < b->n_slots[r]; ++j) {
                LfdSlotPrec& w = wslot[(size_t)r * LFD_MAX_SLOTS + j];
                w.prec = precision[(size_t)r * b->k + j];
                lfd_slot_prec_scale(rslot[(size_t)r * LFD_MAX_SLOTS + j].sx, rslot[(size_t)r * LFD_MAX_SLOTS + j].sy, w);
            }
    const double iso = planes ? 0.0 : lfd_recip_refined((double)iso_sigma_px * (double)iso_sigma_px);
    const LfdSupportGeom g = make_geom(L, refine_status ? support_thresh_px : 0.0f, 0.0f);
    const long long cap = in->capacity;
    const long long* offs = reinterpret_cast<const long long*>(ref_offsets_in);
    const long long total = lfd_support_clamp(offs[b->n_refs], cap);
    std::vector<float> sig((size_t)total);
    parallel_chunks(ctx, (int)((total + kChunk - 1) / kChunk), [&](int c) {
        const long long i1 = std::min<long long>(total, (long long)(c + 1) * kChunk);
        for (long long i = (long long)c * kChunk; i < i1; ++i) {
            const int r = lfd_support_ref_of(offs, b->n_refs, cap, i);
            const int cell = in->cell[i], s = (int)in->slot[i], ns = b->n_slots[r];
            float sigma = LFD_SIGMA_INF;
            if (cell >= 0 && cell < L.HW && s < ns) {                   // no address is formed from a cell outside the grid
                const float X0 = in->xyz[3 * i], X1 = in->xyz[3 * i + 1], X2 = in->xyz[3 * i + 2];
                const LfdSlot* sl = &rslot[(size_t)r * LFD_MAX_SLOTS];
                const LfdSlotPrec* ws = &wslot[(size_t)r * LFD_MAX_SLOTS];
                const bool accepted = refine_status && (refine_status[i] & LFD_REFINE_ACCEPTED) != 0;
                float cj[LFD_MAX_SLOTS], wx[LFD_MAX_SLOTS], wy[LFD_MAX_SLOTS], q00[LFD_MAX_SLOTS], q01[LFD_MAX_SLOTS], q11[LFD_MAX_SLOTS];
                float qs[3] = {0.0f, 0.0f, 0.0f};
                if (planes)
                    for (int e = 0; e < 3; ++e) qs[e] = ws[s].prec[(size_t)cell * 3 + e];
                for (int j = 0; j < LFD_MAX_SLOTS; ++j) {
                    cj[j] = 0.0f; wx[j] = 0.0f; wy[j] = 0.0f; q00[j] = 0.0f; q01[j] = 0.0f; q11[j] = 0.0f;
                    if (accepted && j < ns && j != s) {                 // (no other slot is touched for a point the winner alone placed)
                        cj[j] = sl[j].cert[cell];
                        const float* wv = sl[j].warp + (size_t)cell * g.C + (g.C - 2);
                        wx[j] = wv[0]; wy[j] = wv[1];
                        if (planes) {
                            const float* qp = ws[j].prec + (size_t)cell * 3;
                            q00[j] = qp[0]; q01[j] = qp[1]; q11[j] = qp[2];
                        }
                    }
                }
                const LfdRefineGather o = {cj, wx, wy, q00, q01, q11, qs};
                sigma = accepted ? lfd_sigma_point<LFD_MAX_SLOTS, true>(rref[(size_t)r], sl, ws, ns, s, g, planes, iso, true, o, X0, X1, X2)
                                 : lfd_sigma_point<LFD_MAX_SLOTS, false>(rref[(size_t)r], sl, ws, ns, s, g, planes, iso, false, o, X0, X1, X2);
            }
            sig[(size_t)i] = sigma;
            if (sigma_rel) sigma_rel[i] = sigma;
        }
    });
    compact_points(b, in, offs, cap, total, [&](long long i) { return lfd_sigma_keep(sig[(size_t)i], max_rel_sigma); }, out, ref_offsets_out,
                   seg_counts_out, sig.data(), sigma_rel_out);
    return LFD_OK;
}

// The twin of lfd_consensus_filter: the same keys, a stable sort, lfd_consensus_count_point per sorted point on the context's
// threads, then the stable compaction.
int lfd_consensus_filter_host(lfd_context* ctx, const float* xyz, const float* rgb, const float* err, int64_t n, const int64_t* ref_offsets_host,
                              int32_t n_refs, float radius, int32_t min_refs, float* xyz_out, float* rgb_out, float* err_out,
                              int64_t* ref_offsets_out_host, uint8_t* consensus, int64_t* n_out_host) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    if (const char* why = lfd_consensus_check(xyz, rgb, err, n, ref_offsets_host, n_refs, radius, min_refs, xyz_out, rgb_out, err_out,
                                              ref_offsets_out_host, consensus, n_out_host))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_consensus_filter_host: ") + why);
    for (int32_t r = 0; r <= n_refs; ++r) ref_offsets_out_host[r] = 0;
    *n_out_host = 0;
    if (n == 0) return LFD_OK;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long i = 0; i < n; ++i) {
        if (!lfd_consensus_finite(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2])) continue;
        for (int c = 0; c < 3; ++c) { lo[c] = std::min(lo[c], xyz[3 * i + c]); hi[c] = std::max(hi[c], xyz[3 * i + c]); }
    }
    if (!(lo[0] <= hi[0])) {                                           // no finite point: nothing agrees with anything
        if (consensus) std::memset(consensus, 0, (size_t)n);
        return LFD_OK;
    }
    LfdConsensusGrid g;
    if (!lfd_consensus_grid(lo, hi, radius, g))
        return lfd_fail(ctx, LFD_ERR_INVALID, "lfd_consensus_filter_host: key range: more than 2^30 cells along an axis or a linear cell key beyond 63 bits");
    const long long* offs = reinterpret_cast<const long long*>(ref_offsets_host);
    const int n_chunks = (int)((n + kChunk - 1) / kChunk);
    std::vector<std::pair<unsigned long long, unsigned>> order((size_t)n);
    parallel_chunks(ctx, n_chunks, [&](int c) {
        const long long i1 = std::min<long long>(n, (long long)(c + 1) * kChunk);
        for (long long i = (long long)c * kChunk; i < i1; ++i)
            order[(size_t)i] = {lfd_consensus_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], g.origin[0], g.origin[1], g.origin[2], g.h, g.e[1], g.e[2],
                                                  g.sentinel), (unsigned)i};
    });
    std::sort(order.begin(), order.end());                             // (key, original index): the order of a stable sort by key
    std::vector<unsigned long long> skey((size_t)n);
    std::vector<LfdConsensusPt> spt((size_t)n);
    parallel_chunks(ctx, n_chunks, [&](int c) {
        const long long j1 = std::min<long long>(n, (long long)(c + 1) * kChunk);
        for (long long j = (long long)c * kChunk; j < j1; ++j) {
            const long long i = order[(size_t)j].second;
            skey[(size_t)j] = order[(size_t)j].first;
            spt[(size_t)j] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], lfd_support_ref_of(offs, n_refs, n, i)};
        }
    });
    const float r2 = lfd_consensus_r2(radius);
    const int bound = consensus ? LFD_CONSENSUS_CAP : (int)min_refs;
    std::vector<uint8_t> cnt((size_t)n);
    parallel_chunks(ctx, n_chunks, [&](int c) {
        const long long j1 = std::min<long long>(n, (long long)(c + 1) * kChunk);
        for (long long j = (long long)c * kChunk; j < j1; ++j) {
            int v = 0;
            if (skey[(size_t)j] != g.sentinel)
                v = lfd_consensus_count_point<LFD_CONSENSUS_CAP>(skey.data(), spt.data(), (long long)n, j, g.e[1], g.e[2], r2, bound);
            cnt[(size_t)order[(size_t)j].second] = (uint8_t)v;
        }
    });
    // stable compaction: the input order inside and across references, every value copied as bytes
    long long o = 0;
    int r_next = 0;
    for (long long i = 0; i <= n; ++i) {
        while (r_next <= n_refs && offs[r_next] <= i) ref_offsets_out_host[r_next++] = o;
        if (i == n) break;
        if (consensus) consensus[i] = cnt[(size_t)i];
        if ((int)cnt[(size_t)i] < (int)min_refs) continue;
        std::memcpy(xyz_out + 3 * o, xyz + 3 * i, 12);
        if (rgb) std::memcpy(rgb_out + 3 * o, rgb + 3 * i, 12);
        if (err) std::memcpy(err_out + o, err + i, 4);
        ++o;
    }
    *n_out_host = o;
    return LFD_OK;
}

// The twin of lfd_component_filter: the same keys, a stable sort, lfd_component_links per sorted point into a SEQUENTIAL union-find
// (the partition does not depend on the order of the unions, so one thread gives what the device's thousands give), then sizes, labels, the
// summary and the stable compaction.
int lfd_component_filter_host(lfd_context* ctx, const float* xyz, const float* rgb, const float* err, int64_t n, const int64_t* ref_offsets_host,
                              int32_t n_refs, float radius, int32_t min_points, float* xyz_out, float* rgb_out, float* err_out,
                              int64_t* ref_offsets_out_host, uint32_t* size, uint32_t* label, int64_t* summary_host, int64_t* n_out_host) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    if (const char* why = lfd_component_check(xyz, rgb, err, n, ref_offsets_host, n_refs, radius, min_points, xyz_out, rgb_out, err_out,
                                              ref_offsets_out_host, size, label, n_out_host))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_component_filter_host: ") + why);
    for (int32_t r = 0; r <= n_refs; ++r) ref_offsets_out_host[r] = 0;
    *n_out_host = 0;
    if (summary_host) std::memset(summary_host, 0, LFD_COMPONENT_SUMMARY * sizeof(int64_t));
    if (n == 0) return LFD_OK;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long i = 0; i < n; ++i) {
        if (!lfd_consensus_finite(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2])) continue;
        for (int c = 0; c < 3; ++c) { lo[c] = std::min(lo[c], xyz[3 * i + c]); hi[c] = std::max(hi[c], xyz[3 * i + c]); }
    }
    LfdConsensusGrid g;
    if (!lfd_component_grid(lo, hi, radius, g))
        return lfd_fail(ctx, LFD_ERR_INVALID, "lfd_component_filter_host: key range: more than 2^30 cells along an axis or a linear cell key beyond 63 bits");
    const long long* offs = reinterpret_cast<const long long*>(ref_offsets_host);
    const int n_chunks = (int)((n + kChunk - 1) / kChunk);
    std::vector<std::pair<unsigned long long, unsigned>> order((size_t)n);
    parallel_chunks(ctx, n_chunks, [&](int c) {
        const long long i1 = std::min<long long>(n, (long long)(c + 1) * kChunk);
        for (long long i = (long long)c * kChunk; i < i1; ++i)
            order[(size_t)i] = {lfd_consensus_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], g.origin[0], g.origin[1], g.origin[2], g.h, g.e[1], g.e[2],
                                                  g.sentinel), (unsigned)i};
    });
    std::sort(order.begin(), order.end());                             // (key, original index): the order of a stable sort by key
    std::vector<unsigned long long> skey((size_t)n);
    std::vector<LfdComponentPt> spt((size_t)n);
    std::vector<uint32_t> parent((size_t)n), count((size_t)n, 0u), first((size_t)n, 0xffffffffu);
    for (long long j = 0; j < n; ++j) {
        const long long i = order[(size_t)j].second;
        skey[(size_t)j] = order[(size_t)j].first;
        spt[(size_t)j] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], (uint32_t)i};
        parent[(size_t)j] = (uint32_t)j;
    }
    const float r2 = lfd_consensus_r2(radius);
    for (long long j = 0; j < n && skey[(size_t)j] != g.sentinel; ++j) {       // the sentinel keys sort last
        uint32_t mine = (uint32_t)j;
        lfd_component_links(skey.data(), spt.data(), j, g.e[1], g.e[2], r2,
                            [&](uint32_t q) { mine = lfd_component_unite<LfdComponentSeq, true>(parent.data(), mine, q); });
    }
    std::vector<uint32_t> root((size_t)n);
    for (long long j = 0; j < n; ++j) {
        const uint32_t r = lfd_component_find<LfdComponentSeq>(parent.data(), (uint32_t)j);
        root[(size_t)j] = r;
        count[r] += 1u;
        first[r] = std::min(first[r], spt[(size_t)j].idx);
    }
    std::vector<uint8_t> keep((size_t)n);
    for (long long j = 0; j < n; ++j) {
        const uint32_t r = root[(size_t)j], s = count[r];
        const long long i = spt[(size_t)j].idx;
        keep[(size_t)i] = s >= (uint32_t)min_points ? 1 : 0;
        if (size) size[i] = s;
        if (label) label[i] = first[r];
        if (summary_host && r == (uint32_t)j) lfd_component_summary_add(summary_host, s);
    }
    // stable compaction: the input order inside and across references, every value copied as bytes
    long long o = 0;
    int r_next = 0;
    for (long long i = 0; i <= n; ++i) {
        while (r_next <= n_refs && offs[r_next] <= i) ref_offsets_out_host[r_next++] = o;
        if (i == n) break;
        if (!keep[(size_t)i]) continue;
        std::memcpy(xyz_out + 3 * o, xyz + 3 * i, 12);
        if (rgb) std::memcpy(rgb_out + 3 * o, rgb + 3 * i, 12);
        if (err) std::memcpy(err_out + o, err + i, 4);
        ++o;
    }
    *n_out_host = o;
    return LFD_OK;
}

// The twin of lfd_undistort_image: lfd_undistort_pixel over host pointers, on the caller's thread.  No context and no global state: the
// pack threads call it side by side, each on its own image.
int lfd_host_undistort_image(const uint8_t* src, int32_t w, int32_t h, int32_t channels, int32_t nearest, const double intr[4], const double dist[8],
                             uint8_t* dst, uint8_t* valid255, int64_t* n_invalid_host) {
    if (lfd_undistort_check(src, w, h, channels, intr, dist, dst, valid255)) return LFD_ERR_INVALID;
    const LfdUndistortArgs p = lfd_undistort_args(src, w, h, channels, nearest, intr, dist, dst, valid255);
    int64_t bad = 0;
    for (int i = 0; i < h; ++i)
        for (int j = 0; j < w; ++j) bad += lfd_undistort_pixel(p, i, j) ? 0 : 1;
    if (n_invalid_host) *n_invalid_host = bad;
    return LFD_OK;
}

// The twin of lfd_freespace_filter: the z-buffers by a plain minimum, lfd_freespace_count_point per point on the context's threads,
// then the stable compaction.
int lfd_freespace_filter_host(lfd_context* ctx, const float* xyz, const float* rgb, const float* err, int64_t n, const int64_t* ref_offsets_host,
                              int32_t n_refs, const float* cam_P_host, const int32_t* cam_wh_host, int32_t pw, int32_t ph, float tol,
                              int32_t min_violations, float* xyz_out, float* rgb_out, float* err_out, int64_t* ref_offsets_out_host,
                              uint8_t* violations, uint8_t* supports, int64_t* n_out_host) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    if (const char* why = lfd_freespace_check(xyz, rgb, err, n, ref_offsets_host, n_refs, cam_P_host, cam_wh_host, pw, ph, tol, min_violations,
                                              xyz_out, rgb_out, err_out, ref_offsets_out_host, violations, supports, n_out_host))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_freespace_filter_host: ") + why);
    for (int32_t r = 0; r <= n_refs; ++r) ref_offsets_out_host[r] = 0;
    *n_out_host = 0;
    if (n == 0) return LFD_OK;
    const long long* offs = reinterpret_cast<const long long*>(ref_offsets_host);
    const long long plane = (long long)pw * ph;
    std::vector<LfdFreespaceCam> cams((size_t)n_refs);
    for (int32_t r = 0; r < n_refs; ++r) lfd_freespace_cam(cam_P_host + 12 * (size_t)r, cam_wh_host[2 * r], cam_wh_host[2 * r + 1], cams[(size_t)r]);
    std::vector<uint32_t> zbuf((size_t)n_refs * (size_t)plane, LFD_FREESPACE_EMPTY);
    parallel_chunks(ctx, (int)n_refs, [&](int r) {                     // a reference writes its own plane only
        uint32_t* z = zbuf.data() + (size_t)r * (size_t)plane;
        for (long long i = offs[r]; i < offs[r + 1]; ++i) {
            int cx, cy;
            float d;
            if (!lfd_freespace_project(cams[(size_t)r], (double)pw, (double)ph, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], cx, cy, d)) continue;
            uint32_t bits;
            std::memcpy(&bits, &d, 4);
            uint32_t& cell = z[(size_t)cy * (size_t)pw + (size_t)cx];
            cell = std::min(cell, bits);
        }
    });
    const int n_chunks = (int)((n + kChunk - 1) / kChunk);
    std::vector<uint8_t> keep((size_t)n);
    parallel_chunks(ctx, n_chunks, [&](int c) {
        const long long i1 = std::min<long long>(n, (long long)(c + 1) * kChunk);
        for (long long i = (long long)c * kChunk; i < i1; ++i) {
            const int own = lfd_support_ref_of(offs, n_refs, n, i);
            int v, s;
            lfd_freespace_count_point(cams.data(), zbuf.data(), n_refs, own, pw, ph, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], tol, v, s);
            keep[(size_t)i] = lfd_freespace_keep(v, s, min_violations) ? 1 : 0;
            if (violations) violations[i] = lfd_freespace_u8(v);
            if (supports) supports[i] = lfd_freespace_u8(s);
        }
    });
    // stable compaction: the input order inside and across references, every value copied as bytes
    long long o = 0;
    int r_next = 0;
    for (long long i = 0; i <= n; ++i) {
        while (r_next <= n_refs && offs[r_next] <= i) ref_offsets_out_host[r_next++] = o;
        if (i == n) break;
        if (!keep[(size_t)i]) continue;
        std::memcpy(xyz_out + 3 * o, xyz + 3 * i, 12);
        if (rgb) std::memcpy(rgb_out + 3 * o, rgb + 3 * i, 12);
        if (err) std::memcpy(err_out + o, err + i, 4);
        ++o;
    }
    *n_out_host = o;
    return LFD_OK;
}

// The twin of lfd_render_depth, by the definition and with neither identity: a camera at a time on the context's threads, every point
// written into every cell of its footprint, then every cell's window walked.
int lfd_render_depth_host(lfd_context* ctx, const float* xyz, int64_t n, const float* normals, const float* cam_P_host, const int32_t* cam_wh_host,
                          int32_t n_cams, int32_t pw, int32_t ph, int32_t splat_cells, int32_t window_cells, float tol, int32_t cams_per_batch,
                          float* depth_out, int32_t* index_out, float* normal_out) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    if (const char* why = lfd_depth_check(xyz, n, normals, cam_P_host, cam_wh_host, n_cams, pw, ph, splat_cells, window_cells, tol, cams_per_batch,
                                          depth_out, index_out, normal_out))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_render_depth_host: ") + why);
    const size_t cells = (size_t)pw * (size_t)ph;
    const int r = splat_cells, R = window_cells;
    parallel_chunks(ctx, (int)n_cams, [&](int c) {                     // a camera writes its own planes only
        LfdFreespaceCam cam;
        lfd_freespace_cam(cam_P_host + 12 * (size_t)c, cam_wh_host[2 * c], cam_wh_host[2 * c + 1], cam);
        std::vector<uint64_t> K(cells, LFD_DEPTH_EMPTY);
        for (long long i = 0; i < n; ++i) {
            int cx, cy;
            float d;
            if (!lfd_freespace_project(cam, (double)pw, (double)ph, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], cx, cy, d)) continue;
            const uint64_t key = lfd_depth_key(d, (uint32_t)i);
            for (int yy = std::max(0, cy - r); yy <= std::min(ph - 1, cy + r); ++yy)
                for (int xx = std::max(0, cx - r); xx <= std::min(pw - 1, cx + r); ++xx) {
                    uint64_t& cell = K[(size_t)yy * (size_t)pw + (size_t)xx];
                    cell = std::min(cell, key);
                }
        }
        for (int y = 0; y < ph; ++y)
            for (int x = 0; x < pw; ++x) {
                const uint64_t key = K[(size_t)y * (size_t)pw + (size_t)x];
                bool keep = !lfd_depth_key_empty(key);
                if (keep) {
                    uint32_t m = LFD_FREESPACE_EMPTY;                  // the cell itself is in its window: m <= its depth bits
                    for (int yy = std::max(0, y - R); yy <= std::min(ph - 1, y + R); ++yy)
                        for (int xx = std::max(0, x - R); xx <= std::min(pw - 1, x + R); ++xx)
                            m = std::min(m, lfd_depth_key_bits(K[(size_t)yy * (size_t)pw + (size_t)xx]));
                    keep = lfd_depth_keep(lfd_depth_key_bits(key), m, tol);
                }
                const size_t o = (size_t)c * cells + (size_t)y * (size_t)pw + (size_t)x;
                const uint32_t dbits = keep ? lfd_depth_key_bits(key) : 0u;
                std::memcpy(depth_out + o, &dbits, 4);
                const int32_t idx = keep ? (int32_t)lfd_depth_key_index(key) : -1;
                if (index_out) index_out[o] = idx;
                if (normal_out) {
                    if (keep) std::memcpy(normal_out + 3 * o, normals + 3 * (size_t)idx, 12);
                    else normal_out[3 * o] = normal_out[3 * o + 1] = normal_out[3 * o + 2] = 0.0f;
                }
            }
    });
    return LFD_OK;
}

// The twin of lfd_fuse_oriented: lfd_voxel_downsample's grid and keys, a sort of (key, index) pairs - the order of a stable sort by
// key -, then a serial walk over the voxels with lfd_fuse.hpp's routines: the flag of every point, the two sides' sums in input order, the rows.
int lfd_fuse_oriented_host(lfd_context* ctx, const float* xyz, const float* normals, const float* rgb, int64_t n, double voxel_size, float* xyz_out,
                           float* normals_out, float* rgb_out, uint32_t* count_out, int64_t* n_rows_host, int64_t* n_voxels_host) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    if (const char* why = lfd_fuse_check(xyz, normals, rgb, n, voxel_size, xyz_out, normals_out, rgb_out, count_out, n_rows_host, n_voxels_host))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_fuse_oriented_host: ") + why);
    *n_rows_host = 0;
    *n_voxels_host = 0;
    if (n == 0) return LFD_OK;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, cmax = -INFINITY;
    bool nonfinite = false, nan_rgb = false;
    for (long long i = 0; i < 3 * (long long)n; ++i) {
        const int c = (int)(i % 3);
        if (std::isfinite(xyz[i])) { lo[c] = std::min(lo[c], xyz[i]); hi[c] = std::max(hi[c], xyz[i]); }
        else nonfinite = true;
        if (std::isnan(rgb[i])) nan_rgb = true;
        else cmax = std::max(cmax, rgb[i]);
    }
    if (nonfinite) return lfd_fail(ctx, LFD_ERR_INVALID, "lfd_fuse_oriented_host: " LFD_FUSE_NONFINITE);
    LfdFuseGrid g;
    if (!lfd_fuse_grid(lo, hi, voxel_size, g)) return lfd_fail(ctx, LFD_ERR_INVALID, "lfd_fuse_oriented_host: " LFD_FUSE_KEY_RANGE);
    const double cscale = lfd_fuse_cscale(cmax, nan_rgb);
    std::vector<std::pair<unsigned long long, unsigned>> order((size_t)n);
    for (long long i = 0; i < n; ++i)
        order[(size_t)i] = {lfd_fuse_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], g.origin[0], g.origin[1], g.origin[2], voxel_size, g.e[1], g.e[2]),
                            (unsigned)i};
    std::sort(order.begin(), order.end());
    long long r = 0, nv = 0;
    for (long long a = 0; a < n;) {
        long long b = a + 1;
        while (b < n && order[(size_t)b].first == order[(size_t)a].first) ++b;
        LfdFuseAcc side[2];
        lfd_fuse_clear(side[0]);
        lfd_fuse_clear(side[1]);
        float piv[3] = {0.0f, 0.0f, 0.0f};
        bool has = false;
        for (long long j = a; j < b; ++j) {
            const long long i = order[(size_t)j].second;
            const float* nn = normals + 3 * i;
            const unsigned f = lfd_fuse_flag(nn, has, piv);
            if (!has && (f & LFD_FUSE_USABLE)) { has = true; piv[0] = nn[0]; piv[1] = nn[1]; piv[2] = nn[2]; }
            lfd_fuse_add(side[f & LFD_FUSE_SIDE], xyz + 3 * i, nn, rgb + 3 * i, (f & LFD_FUSE_USABLE) != 0u, cscale);
        }
        for (int s = 0; s < 2; ++s) {
            if (!side[s].cnt) continue;
            lfd_fuse_emit(side[s], xyz_out + 3 * r, normals_out + 3 * r, rgb_out + 3 * r);
            if (count_out) count_out[r] = side[s].cnt;
            ++r;
        }
        ++nv;
        a = b;
    }
    *n_rows_host = r;
    *n_voxels_host = nv;
    return LFD_OK;
}

// The twin of lfd_knn_dist2: the same grid, keys, automatic cell size and ring scan (lfd_knn.hpp) over a sort of (key, index) pairs,
// on the context's threads; the points no ring settles are finished by a loop over the whole cloud.
int lfd_knn_dist2_host(lfd_context* ctx, const float* xyz, int64_t n, double cell_size, float* dist2_out, double* stats_host) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    if (const char* why = lfd_knn_check(xyz, n, cell_size, dist2_out)) return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_knn_dist2_host: ") + why);
    if (stats_host) stats_host[0] = stats_host[1] = stats_host[2] = stats_host[3] = 0.0;
    if (n == 0) return LFD_OK;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool nonfinite = false;
    for (long long i = 0; i < 3 * (long long)n; ++i) {
        const int c = (int)(i % 3);
        if (std::isfinite(xyz[i])) { lo[c] = std::min(lo[c], xyz[i]); hi[c] = std::max(hi[c], xyz[i]); }
        else nonfinite = true;
    }
    if (nonfinite) return lfd_fail(ctx, LFD_ERR_INVALID, "lfd_knn_dist2_host: " LFD_KNN_NONFINITE);
    double h = cell_size > 0.0 ? cell_size : lfd_knn_auto_h(lo, hi, (long long)n);
    LfdKnnGrid g;
    if (!lfd_knn_grid(lo, hi, h, g)) return lfd_fail(ctx, LFD_ERR_INVALID, "lfd_knn_dist2_host: " LFD_KNN_KEY_RANGE);
    const int n_chunks = (int)((n + kChunk - 1) / kChunk);
    std::vector<std::pair<unsigned long long, unsigned>> order((size_t)n);
    long long occupied = 0, fullest = 0;
    for (int rebuilds = 0;;) {
        parallel_chunks(ctx, n_chunks, [&](int c) {
            const long long i1 = std::min<long long>(n, (long long)(c + 1) * kChunk);
            for (long long i = (long long)c * kChunk; i < i1; ++i)
                order[(size_t)i] = {lfd_knn_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], g), (unsigned)i};
        });
        std::sort(order.begin(), order.end());
        occupied = 0;
        fullest = 0;
        for (long long a = 0; a < n;) {
            long long b = a + 1;
            while (b < n && order[(size_t)b].first == order[(size_t)a].first) ++b;
            ++occupied;
            fullest = std::max(fullest, b - a);
            a = b;
        }
        LfdKnnGrid finer;
        if (cell_size > 0.0 || !lfd_knn_refine_more((long long)n, occupied, rebuilds) || !lfd_knn_grid(lo, hi, h / 4.0, finer)) break;
        h = h / 4.0;
        g = finer;
        ++rebuilds;
    }
    std::vector<unsigned long long> skey((size_t)n);
    std::vector<LfdKnnPt> spt((size_t)n);
    std::vector<uint8_t> open_pt((size_t)n);
    parallel_chunks(ctx, n_chunks, [&](int c) {
        const long long j1 = std::min<long long>(n, (long long)(c + 1) * kChunk);
        for (long long j = (long long)c * kChunk; j < j1; ++j) {
            const unsigned i = order[(size_t)j].second;
            skey[(size_t)j] = order[(size_t)j].first;
            spt[(size_t)j] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], i};
        }
    });
    parallel_chunks(ctx, n_chunks, [&](int c) {
        const long long j1 = std::min<long long>(n, (long long)(c + 1) * kChunk);
        for (long long j = (long long)c * kChunk; j < j1; ++j) {
            float mean;
            const bool done = lfd_knn_scan_point(skey.data(), spt.data(), (long long)n, j, g, &mean);
            if (done) dist2_out[spt[(size_t)j].idx] = mean;
            open_pt[(size_t)j] = done ? 0 : 1;
        }
    });
    std::vector<long long> list;
    for (long long j = 0; j < n; ++j)
        if (open_pt[(size_t)j]) list.push_back(j);
    parallel_chunks(ctx, (int)std::min<size_t>(list.size(), 1u << 20), [&](int c) {
        for (size_t e = (size_t)c; e < list.size(); e += (size_t)1 << 20) {
            const long long j = list[e];
            const LfdKnnPt me = spt[(size_t)j];
            float a = INFINITY, b = INFINITY, cc = INFINITY;
            for (long long q = 0; q < n; ++q) {
                if (q == j) continue;
                const LfdKnnPt& p = spt[(size_t)q];
                lfd_knn_insert(lfd_knn_d2(me.x, me.y, me.z, p.x, p.y, p.z), a, b, cc);
            }
            dist2_out[me.idx] = lfd_knn_mean(a, b, cc);
        }
    });
    if (stats_host) {
        stats_host[0] = h;
        stats_host[1] = (double)occupied;
        stats_host[2] = (double)fullest;
        stats_host[3] = (double)list.size();
    }
    return LFD_OK;
}

// The twin of lfd_pack_gaussians: lfd_gauss_record per point on the context's threads (IEEE sqrt and divide, the C library's log).
int lfd_pack_gaussians_host(lfd_context* ctx, const float* xyz, const float* normals, const float* rgb, const float* dist2, int64_t n,
                            float opacity_logit, double log_flatten, double max_scale, uint8_t* out) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    if (const char* why = lfd_gauss_check(xyz, normals, rgb, dist2, n, opacity_logit, log_flatten, max_scale, out))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_pack_gaussians_host: ") + why);
    const float max_m = lfd_gauss_max_m(max_scale);
    float* o = reinterpret_cast<float*>(out);
    const int n_chunks = (int)((n + kChunk - 1) / kChunk);
    parallel_chunks(ctx, n_chunks, [&](int c) {
        const long long i1 = std::min<long long>(n, (long long)(c + 1) * kChunk);
        for (long long i = (long long)c * kChunk; i < i1; ++i)
            lfd_gauss_record(xyz + 3 * i, normals + 3 * i, rgb + 3 * i, dist2[i], opacity_logit, log_flatten, max_m, o + LFD_GAUSS_FLOATS * i);
    });
    return LFD_OK;
}

// The twin of lfd_cap_spatial: the same box, keys, level, picks and error ranks (lfd_cap.hpp) over a stable sort of (key, index) pairs.
// The keys are made on the context's threads; everything behind them is one ordered walk, so the result does not depend on the thread count.
int lfd_cap_spatial_host(lfd_context* ctx, const float* xyz, const float* err, int64_t n, int64_t budget, int64_t* keep_out, int64_t* n_keep_host,
                         double* stats_host) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    if (const char* why = lfd_cap_check(xyz, err, n, budget, keep_out, n_keep_host))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_cap_spatial_host: ") + why);
    *n_keep_host = 0;
    if (stats_host) stats_host[0] = stats_host[1] = stats_host[2] = stats_host[3] = 0.0;
    if (n == 0) return LFD_OK;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool nonfinite = false;
    for (long long i = 0; i < 3 * (long long)n; ++i) {
        const int c = (int)(i % 3);
        if (std::isfinite(xyz[i])) { lo[c] = std::min(lo[c], xyz[i]); hi[c] = std::max(hi[c], xyz[i]); }
        else nonfinite = true;
    }
    if (nonfinite) return lfd_fail(ctx, LFD_ERR_INVALID, "lfd_cap_spatial_host: " LFD_CAP_NONFINITE);
    const LfdCapBox box = lfd_cap_box(lo, hi);
    const int n_chunks = (int)((n + kChunk - 1) / kChunk);
    std::vector<std::pair<unsigned long long, unsigned>> order((size_t)n);
    parallel_chunks(ctx, n_chunks, [&](int c) {
        const long long i1 = std::min<long long>(n, (long long)(c + 1) * kChunk);
        for (long long i = (long long)c * kChunk; i < i1; ++i)
            order[(size_t)i] = {lfd_cap_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], box), (unsigned)i};
    });
    std::stable_sort(order.begin(), order.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    unsigned long long hist[LFD_CAP_LEVELS + 1] = {};
    for (long long j = 1; j < n; ++j) ++hist[lfd_cap_pair_level(order[(size_t)j].first, order[(size_t)j - 1].first)];
    long long cells = 0;
    const int lev = lfd_cap_level(hist, (long long)budget, box.L, &cells, stats_host);
    if (n <= budget) {                                                 // the cap does not act: every point is kept
        for (long long i = 0; i < n; ++i) keep_out[i] = i;
        *n_keep_host = n;
        return LFD_OK;
    }
    std::vector<uint8_t> keep((size_t)n, 0);
    long long k = 0;
    for (long long a = 0; a < n; ++k) {
        const unsigned long long cell = lfd_cap_cell_key(order[(size_t)a].first, lev);
        long long b = a;
        unsigned long long best = ~0ull;
        for (; b < n && lfd_cap_cell_key(order[(size_t)b].first, lev) == cell; ++b) {
            const unsigned i = order[(size_t)b].second;
            uint32_t bits = 0u;
            if (err) std::memcpy(&bits, err + i, sizeof(bits));
            best = std::min(best, lfd_cap_pack(err ? lfd_cap_rank(bits) : 0u, i));
        }
        if (lfd_cap_pick((unsigned long long)k, (unsigned long long)budget, (unsigned long long)cells)) keep[(size_t)(best & 0xffffffffull)] = 1;
        a = b;
    }
    long long kept = 0;
    const long long capacity = std::min<long long>(budget, n);
    for (long long i = 0; i < n; ++i)
        if (keep[(size_t)i] && kept < capacity) keep_out[kept++] = i;
    *n_keep_host = kept;
    return LFD_OK;
}

// The twin of lfd_thin_footprint: lfd_thin.hpp's walk - the same box, levels, codes and error ranks over a stable sort of
// (code, index) pairs, one ordered pass, so the result does not depend on the thread count.
int lfd_thin_footprint_host(lfd_context* ctx, const float* xyz, const float* err, int64_t n, const int64_t* ref_offsets_host, int32_t n_refs,
                            const double* ref_rows_host, double thin_cells, int64_t* keep_out, int64_t* n_keep_host, int64_t* ref_offsets_out_host,
                            double* stats_host) {
    if (!ctx) return lfd_fail(nullptr, LFD_ERR_INVALID, "null context");
    if (!ctx->is_host) return lfd_fail(ctx, LFD_ERR_STATE, "the *_host entry points need a context made by lfd_create_host");
    if (const char* why = lfd_thin_check(xyz, err, n, ref_offsets_host, n_refs, ref_rows_host, thin_cells, keep_out, n_keep_host, ref_offsets_out_host))
        return lfd_fail(ctx, LFD_ERR_INVALID, std::string("lfd_thin_footprint_host: ") + why);
    for (int32_t r = 0; r <= n_refs; ++r) ref_offsets_out_host[r] = 0;
    *n_keep_host = 0;
    if (stats_host)
        for (int k = 0; k < LFD_THIN_STATS; ++k) stats_host[k] = 0.0;
    if (n == 0) return LFD_OK;
    const long long kept = lfd_thin_walk(xyz, err, (long long)n, ref_offsets_host, n_refs, ref_rows_host, thin_cells, keep_out, ref_offsets_out_host, stats_host);
    if (kept < 0) return lfd_fail(ctx, LFD_ERR_INVALID, "lfd_thin_footprint_host: " LFD_THIN_NONFINITE);
    *n_keep_host = kept;
    return LFD_OK;
}

int lfd_aggregate_host(lfd_context* ctx, const lfd_batch* b, const lfd_params* p, float* best_cert, uint8_t* best_slot) {
    int rc = validate_host(ctx, b, p);
    if (rc != LFD_OK) return rc;
    if (!best_cert) return lfd_fail(ctx, LFD_ERR_INVALID, "best_cert is null");
    HostLaunch L;
    prepare_host(b, p, L);
    const int chunks_per_ref = (L.HW + kChunk - 1) / kChunk;
    parallel_chunks(ctx, b->n_refs * chunks_per_ref, [&](int c) {
        const int r = c / chunks_per_ref, c0 = (c - r * chunks_per_ref) * kChunk, c1 = std::min(c0 + kChunk, L.HW);
        for (int cell = c0; cell < c1; ++cell) {
            float best; int bj;
            host_cell_best(L, r, cell, best, bj);
            best_cert[(size_t)r * L.HW + cell] = best;
            if (best_slot) best_slot[(size_t)r * L.HW + cell] = (uint8_t)bj;
        }
    });
    return LFD_OK;
}

int lfd_triangulate_dense_host(lfd_context* ctx, const lfd_batch* b, const lfd_params* p, const lfd_points* out,
                               int64_t* ref_offsets, int32_t* seg_counts) {
    int rc = validate_host(ctx, b, p);
    if (rc != LFD_OK) return rc;
    rc = check_host_points(ctx, out, ref_offsets);
    if (rc != LFD_OK) return rc;
    HostLaunch L;
    prepare_host(b, p, L);
    const int chunks_per_ref = (L.HW + kChunk - 1) / kChunk;
    std::vector<HostRef> refs((size_t)b->n_refs);
    for (int r = 0; r < b->n_refs; ++r) make_ref(ctx, L, r, refs[(size_t)r]);
    // Every chunk parks its survivors at its own fixed place of a staging area that belongs to the context (chunk c at
    // c * kChunk: no allocation, no growth, nothing shared between threads); a prefix over the chunk counts then gives every
    // chunk its place in the output - references in batch order, cells in raster order, the device's look-back scan - and a
    // second parallel sweep moves the records there.  References are taken in groups so that the staging area stays bounded.
    const int refs_per_group = std::max(1, (int)(((size_t)256 << 20) / (sizeof(HostPoint) * (size_t)chunks_per_ref * kChunk)));
    const int group_chunks = std::min(b->n_refs, refs_per_group) * chunks_per_ref;
    if (ctx->host_stage.size() < (size_t)group_chunks * kChunk * sizeof(HostPoint)) ctx->host_stage.resize((size_t)group_chunks * kChunk * sizeof(HostPoint));
    HostPoint* stage = reinterpret_cast<HostPoint*>(ctx->host_stage.data());
    std::vector<int> kept((size_t)group_chunks);
    std::vector<int> per_slot(seg_counts ? (size_t)group_chunks * LFD_MAX_SLOTS : 0);
    std::vector<long long> start((size_t)group_chunks + 1);
    if (seg_counts) std::memset(seg_counts, 0, sizeof(int32_t) * (size_t)b->n_refs * b->k);
    long long total = 0;
    for (int r0 = 0; r0 < b->n_refs; r0 += refs_per_group) {
        const int nr = std::min(refs_per_group, b->n_refs - r0), nc = nr * chunks_per_ref;
        parallel_chunks(ctx, nc, [&](int c) {
            const int r = r0 + c / chunks_per_ref, c0 = (c % chunks_per_ref) * kChunk, c1 = std::min(c0 + kChunk, L.HW);
            HostPoint* v = stage + (size_t)c * kChunk;
            int n = 0, bj;
            for (int cell = c0; cell < c1; ++cell)
                if (host_eval_cell(L, refs[(size_t)r], r, cell, v[n], bj, true)) ++n;
            kept[(size_t)c] = n;
            if (seg_counts) {
                int* cnt = per_slot.data() + (size_t)c * LFD_MAX_SLOTS;
                for (int j = 0; j < LFD_MAX_SLOTS; ++j) cnt[j] = 0;
                for (int i = 0; i < n; ++i) cnt[v[i].slot] += 1;
            }
        });
        start[0] = total;
        for (int c = 0; c < nc; ++c) start[(size_t)c + 1] = start[(size_t)c] + kept[(size_t)c];
        for (int r = 0; r < nr; ++r) ref_offsets[r0 + r] = start[(size_t)r * chunks_per_ref];
        total = start[(size_t)nc];
        parallel_chunks(ctx, nc, [&](int c) {
            long long pos = start[(size_t)c];
            const HostPoint* v = stage + (size_t)c * kChunk;
            for (int i = 0; i < kept[(size_t)c]; ++i) store_point(out, pos++, v[i]);
        });
        if (seg_counts)
            for (int c = 0; c < nc; ++c)
                for (int j = 0; j < b->k; ++j) seg_counts[(size_t)(r0 + c / chunks_per_ref) * b->k + j] += per_slot[(size_t)c * LFD_MAX_SLOTS + j];
    }
    ref_offsets[b->n_refs] = total;
    if (total > out->capacity) return lfd_fail(ctx, LFD_ERR_CAPACITY, "output capacity too small (counts are valid)");
    return LFD_OK;
}

int lfd_triangulate_indexed_host(lfd_context* ctx, const lfd_batch* b, const lfd_params* p, const int64_t* sel_idx,
                                 const int64_t* sel_offsets, const lfd_points* out, int64_t* ref_offsets, int32_t* seg_counts,
                                 int32_t* seg_order) {
    int rc = validate_host(ctx, b, p);
    if (rc != LFD_OK) return rc;
    if (!sel_idx || !sel_offsets) return lfd_fail(ctx, LFD_ERR_INVALID, "sel_idx / sel_offsets are required");
    if (sel_offsets[0] != 0) return lfd_fail(ctx, LFD_ERR_INVALID, "sel_offsets[0] must be 0");
    for (int r = 0; r < b->n_refs; ++r)
        if (sel_offsets[r + 1] < sel_offsets[r]) return lfd_fail(ctx, LFD_ERR_INVALID, "sel_offsets must be non-decreasing");
    rc = check_host_points(ctx, out, ref_offsets);
    if (rc != LFD_OK) return rc;
    HostLaunch L;
    prepare_host(b, p, L);
    L.exact_colour = true;       // the upstream-equivalent mode always blends in f64, like lfd_triangulate_indexed
    long long total = 0;
    for (int r = 0; r < b->n_refs; ++r) {
        HostRef R;
        make_ref(ctx, L, r, R);
        const long long s0 = sel_offsets[r], n_sel = sel_offsets[r + 1] - s0;
        std::vector<HostPoint> pts((size_t)n_sel);
        std::vector<int8_t> code((size_t)n_sel, (int8_t)-1);          // -1 dropped index, else slot | 0x40 when kept
        const int n_chunks = (int)((n_sel + kChunk - 1) / kChunk);
        parallel_chunks(ctx, n_chunks, [&](int c) {
            const long long i0 = (long long)c * kChunk, i1 = std::min<long long>(i0 + kChunk, n_sel);
            for (long long i = i0; i < i1; ++i) {
                const long long cl = sel_idx[s0 + i];
                if (cl < 0 || cl >= L.HW) continue;                   // invalid selection index: dropped
                int bj = 0;
                const bool keep = host_eval_cell(L, R, r, (int)cl, pts[(size_t)i], bj);
                code[(size_t)i] = (int8_t)(bj | (keep ? 0x40 : 0));
            }
        });
        // groups in order of first appearance while scanning sel_idx (core/pipeline.py:685-688), members in sel_idx order
        int order[LFD_MAX_SLOTS], n_groups = 0;
        long long count[LFD_MAX_SLOTS] = {0};
        bool seen[LFD_MAX_SLOTS] = {false};
        for (long long i = 0; i < n_sel; ++i) {
            if (code[(size_t)i] < 0) continue;
            const int j = code[(size_t)i] & 0x3f;
            if (!seen[j]) { seen[j] = true; order[n_groups++] = j; }
            if (code[(size_t)i] & 0x40) count[j] += 1;
        }
        long long begin[LFD_MAX_SLOTS] = {0}, acc = total;
        int g_out = 0;
        for (int g = 0; g < n_groups; ++g) {
            const int j = order[g];
            begin[j] = acc; acc += count[j];
            if (count[j] && seg_order) seg_order[(size_t)r * b->k + g_out] = j;
            if (count[j]) ++g_out;
        }
        if (seg_order) for (; g_out < b->k; ++g_out) seg_order[(size_t)r * b->k + g_out] = -1;
        if (seg_counts) for (int j = 0; j < b->k; ++j) seg_counts[(size_t)r * b->k + j] = (j < b->n_slots[r]) ? (int32_t)count[j] : 0;
        for (long long i = 0; i < n_sel; ++i) {
            if (code[(size_t)i] < 0 || !(code[(size_t)i] & 0x40)) continue;
            HostPoint& pt = pts[(size_t)i];
            store_point(out, begin[pt.slot]++, pt);
        }
        ref_offsets[r] = total;
        total = acc;
    }
    ref_offsets[b->n_refs] = total;
    if (total > out->capacity) return lfd_fail(ctx, LFD_ERR_CAPACITY, "output capacity too small (counts are valid)");
    return LFD_OK;
}

}  // extern "C"
