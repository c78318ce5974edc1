// rr_api.hip — the C-ABI entry points of the render path (include/rain_raster.h): forward,
// backward and the Gaussian-sharded step; stage ordering, the single device->host sync and the
// hand-off between a frame's forward and its backward; then runtime tuning, frame statistics, debug
// views and the per-stage profile.  The scratch layout is rr_layout.hpp.
//
// Replaces CudaRasterizer::Rasterizer::{forward,backward,markVisible}
// (rasterizer_impl.cu:130-142,187-430) and the pybind wrappers (rasterize_points.cu:24-212).
#include <algorithm>
#include <chrono>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rain_raster.h"
#include "rr_common.hpp"
#include "rr_contrib.hpp"
#include "rr_kernels.hpp"
#include "rr_layout.hpp"

using namespace rr;

namespace rr {
// The tuning record of the current device (rr_kernels.hpp Tuning): a device index outside the
// table, or no device at all (a CPU-only process setting knobs), uses entry 0.
Tuning& tuning() {
    static Tuning per_device[kMaxDevices];
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= kMaxDevices) {
        (void)hipGetLastError();
        d = 0;
    }
    return per_device[d];
}
}  // namespace rr

namespace {

thread_local std::string g_err;  // rr_last_error

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// ---- event timing (bench.py reads per-stage kernel time through rr_profile_collect) ----
struct EvRec {
    int stage;
    hipEvent_t a, b;
};
bool g_prof = false;
unsigned g_prof_mask = 0xffffffffu;  // stages recorded while profiling (rr_profile_select)
std::vector<EvRec> g_recs;
std::vector<hipEvent_t> g_pool;

hipEvent_t ev_get() {
    if (!g_pool.empty()) {
        hipEvent_t e = g_pool.back();
        g_pool.pop_back();
        return e;
    }
    // timing only: no system-scope fence (cache write-back + invalidate) at each record, which
    // otherwise opens a ~5 us gap before the next kernel of the stream
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipEventCreate(&e);
    }
    return e;
}

struct StageTimer {
    int stage;
    hipStream_t st;
    hipEvent_t a = nullptr;
    StageTimer(int s, hipStream_t stream) : stage(s), st(stream) {
        if (g_prof && ((g_prof_mask >> s) & 1u)) {
            a = ev_get();
            (void)hipEventRecord(a, st);
        }
    }
    ~StageTimer() {
        if (a) {
            hipEvent_t b = ev_get();
            (void)hipEventRecord(b, st);
            g_recs.push_back({stage, a, b});
        }
    }
};

// Launch check: always catch launch errors; with `debug`, synchronise and check the kernel
// (CHECK_CUDA, auxiliary.h:155-162).
int check(const rr_frame* f, hipStream_t st, const char* what) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && f && f->debug) {
        e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(RR_ERR_HIP, std::string("[HIP ERROR] in ") + what + ": " + hipGetErrorString(e));
    return RR_OK;
}
#define RR_CHECK(call, what)                                                              \
    do {                                                                                  \
        hipError_t _e = (call);                                                           \
        if (_e != hipSuccess)                                                             \
            return fail(RR_ERR_HIP, std::string("[HIP ERROR] ") + what + ": " + hipGetErrorString(_e)); \
    } while (0)
#define RR_STAGE_CHECK(what)                   \
    do {                                       \
        int _rc = check(f, st, what);          \
        if (_rc != RR_OK) return _rc;          \
    } while (0)
// One stage whose launches cannot fail on the host: `launch` between the stage's events, then its check.
template <typename F>
int stage(const rr_frame* f, hipStream_t st, int id, const char* what, F&& launch) {
    {
        StageTimer tm(id, st);
        launch();
    }
    return check(f, st, what);
}

// ---------------------------------------------------------------------------------------
// Readback of the forward's pair counts.  A hipMemcpyAsync into pageable host memory + stream
// synchronise after the scan costs a blit kernel and the runtime's blocking wait (measured 30-140
// us of idle GPU per frame before the binning launches).  Instead the split scan's first launch
// (rr_bin.hip k_split_scan_totals: workgroup 0, once the frame's totals and depth cut are known;
// the scan runs on while the host reads) stores the counts and a sequence number into a coherent
// pinned host mailbox (system-scope stores, the sequence number last) and the host thread spins on
// the sequence number.  Once the wait has outlasted any frame the stream is queried: a launch /
// kernel error is reported, and a stream that went idle without the sequence number becoming
// visible falls back to the plain copy.
struct Mailbox {
    uint32_t* host = nullptr;  // [L, rect, seq, wide], coherent pinned
    uint32_t* dev = nullptr;   // device alias of host
    uint32_t seq = 0;
    bool failed = false;       // allocation failed: always use the copy
};
thread_local Mailbox g_mailbox;

struct PairCountRead {
    const FrameTotals* copy = nullptr;  // device totals for the copy path
    uint32_t seq = 0;  // 0: no mailbox (copy + synchronise at wait time)
};
struct PairCounts {
    uint32_t L = 0, rect = 0;  // saturated to 32 bits
    bool wide = false;
};

// The mailbox (allocated on first use) and this read's sequence number; box == null: no mailbox.
uint32_t* pair_counts_box(const FrameTotals* copy, PairCountRead& r) {
    Mailbox& mb = g_mailbox;
    r.copy = copy;
    r.seq = 0;
    if (!mb.host && !mb.failed) {
        void* h = nullptr;
        if (hipHostMalloc(&h, 64, hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess &&
            hipHostGetDevicePointer(reinterpret_cast<void**>(&mb.dev), h, 0) == hipSuccess) {
            mb.host = static_cast<uint32_t*>(h);
            std::memset(h, 0, 64);
        } else {
            if (h) (void)hipHostFree(h);
            (void)hipGetLastError();
            mb.failed = true;
        }
    }
    if (mb.failed) return nullptr;
    r.seq = ++mb.seq == 0 ? ++mb.seq : mb.seq;  // 0 is the mailbox's initial value
    return mb.dev;
}

hipError_t pair_counts_copy(const FrameTotals* src, PairCounts* out, hipStream_t st) {
    FrameTotals v{};
    hipError_t e = hipMemcpyAsync(&v, src, sizeof(v), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    out->L = v.L > 0xffffffffull ? 0xffffffffu : (uint32_t)v.L;
    out->rect = v.rect > 0xffffffffull ? 0xffffffffu : (uint32_t)v.rect;
    out->wide = v.wide != 0;
    return e;
}

thread_local int64_t g_wait_ns = 0, g_waits = 0;  // rr_host_wait_stats
#ifndef RR_WAIT_QUERY_MS
#define RR_WAIT_QUERY_MS 20
#endif
struct WaitClock {  // adds the scope's duration to the host-wait statistics
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~WaitClock() {
        g_wait_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        g_waits++;
    }
};

hipError_t pair_counts_wait(const PairCountRead& r, PairCounts* out, hipStream_t st) {
    WaitClock clock;
    Mailbox& mb = g_mailbox;
    if (r.seq == 0) return pair_counts_copy(r.copy, out, st);
    for (uint32_t spin = 1;; spin++) {
        if (__atomic_load_n(mb.host + 2, __ATOMIC_ACQUIRE) == r.seq) {
            out->L = __atomic_load_n(mb.host + 0, __ATOMIC_RELAXED);
            out->rect = __atomic_load_n(mb.host + 1, __ATOMIC_RELAXED);
            out->wide = __atomic_load_n(mb.host + 3, __ATOMIC_RELAXED) != 0;
            return hipSuccess;
        }
        // the stream is queried only once the wait has outlasted any frame (RR_WAIT_QUERY_MS): a query
        // while the device is still busy with this frame is not free on the device side
        if ((spin & 4095u) == 0 &&
            std::chrono::steady_clock::now() - clock.t0 > std::chrono::milliseconds(RR_WAIT_QUERY_MS)) {
            const hipError_t q = hipStreamQuery(st);
            if (q == hipSuccess) {
                if (__atomic_load_n(mb.host + 2, __ATOMIC_ACQUIRE) == r.seq) continue;
                mb.failed = true;  // idle stream, value not visible: never use the mailbox again
                return pair_counts_copy(r.copy, out, st);
            }
            if (q != hipErrorNotReady) return q;
        }
        __builtin_ia32_pause();
    }
}

// ---- argument checks and the argument blocks several entry points fill ----
int validate(const rr_frame* f, const rr_camera* cam, const rr_gaussians* g, bool forward) {
    if (!f || !cam || !g) return fail(RR_ERR_ARG, "null frame/camera/gaussians");
    if (f->P < 0 || f->width <= 0 || f->height <= 0) return fail(RR_ERR_ARG, "bad P/width/height");
    if (f->P > (int)BIN_ID_MASK) return fail(RR_ERR_ARG, "P >= 2^28 (pair values carry a 4-bit tile mask)");
    if (f->P == 0) return RR_OK;
    if (!g->means3D || (forward && !g->opacities)) return fail(RR_ERR_ARG, "means3D and opacities are required");
    if (!cam->background || !cam->viewmatrix || !cam->projmatrix || !cam->campos)
        return fail(RR_ERR_ARG, "camera arrays are required");
    if ((g->shs == nullptr) == (g->colors_precomp == nullptr))
        return fail(RR_ERR_ARG, "Please provide excatly one of either SHs or precomputed colors!");
    const bool sr = g->scales && g->rotations;
    if (sr == (g->cov3D_precomp != nullptr))
        return fail(RR_ERR_ARG,
                    "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
    if (g->shs && (f->D < 0 || f->D > 3 || f->M < (f->D + 1) * (f->D + 1)))
        return fail(RR_ERR_ARG, "sh_degree must be 0..3 and sh.size(1) >= (degree+1)^2");
    if (f->M > 16) return fail(RR_ERR_ARG, "sh.size(1) > 16 is not supported (SH degree <= 3, forward.cu:9-60)");
    if ((f->flags & RR_FLAG_AUX_NORMAL) && !sr)
        return fail(RR_ERR_ARG, "the aux normal output needs scales/rotations (not cov3D_precomp)");
    if (f->flags & RR_FLAG_RAW_PARAMS) {
        if (!g->shs || !sr || !g->opacities)
            return fail(RR_ERR_ARG, "raw-parameter mode needs SH, scales/rotations and opacities");
        if (f->M > 1 && !g->shs_rest) return fail(RR_ERR_ARG, "raw-parameter mode needs shs_rest when M > 1");
    }
    return RR_OK;
}

int check_views(const rr_view* views, int num_views) {
    for (int v = 0; v < num_views; v++) {
        const rr_view& w = views[v];
        if (!w.viewmatrix || !w.projmatrix || !w.campos || w.width <= 0 || w.height <= 0)
            return fail(RR_ERR_ARG, "bad view");
    }
    return RR_OK;
}

// focal length in pixels of an image `extent` pixels wide (high) with half-angle tangent tan_half
inline float focal(int extent, float tan_half) { return extent / (2.0f * tan_half); }

// The fused optimizer step's groups: moments present and param the matching input array, for every
// group (all_stepped: a group without param is an error) or for the groups that have a param.
// f_rest does not exist when M <= 1.
int check_adam(const rr_frame* f, const rr_gaussians* g, const rr_adam* ad, bool all_stepped) {
    const rr_adam_group* gs[6] = {&ad->xyz, &ad->f_dc, &ad->f_rest, &ad->opacity, &ad->scaling, &ad->rotation};
    const void* in[6] = {g->means3D, g->shs, g->shs_rest, g->opacities, g->scales, g->rotations};
    for (int i = 0; i < 6; i++) {
        if ((i == 2 && f->M <= 1) || (!all_stepped && !gs[i]->param)) continue;
        if (!gs[i]->param || !gs[i]->exp_avg || !gs[i]->exp_avg_sq)
            return fail(RR_ERR_ARG, all_stepped ? "null Adam group array" : "null Adam moment array");
        if (gs[i]->param != in[i]) return fail(RR_ERR_ARG, "Adam group param must be the matching input array");
    }
    return RR_OK;
}

// Preprocess arguments of a frame (the output arrays are set by the caller).
PreArgs pre_args(const rr_frame* f, const rr_camera* cam, const rr_gaussians* g) {
    PreArgs a{};
    a.P = f->P; a.D = f->D; a.M = f->M; a.W = f->width; a.H = f->height;
    a.gx = grid_x(f->width); a.gy = grid_y(f->height);
    a.prefiltered = f->prefiltered;
    a.tanfovx = f->tan_fovx; a.tanfovy = f->tan_fovy;
    a.focal_y = focal(f->height, f->tan_fovy);
    a.focal_x = focal(f->width, f->tan_fovx);
    a.scale_modifier = f->scale_modifier; a.low_pass = f->low_pass;
    a.means3D = g->means3D; a.shs = g->shs; a.colors_precomp = g->colors_precomp; a.opacities = g->opacities;
    a.scales = g->scales; a.rotations = g->rotations; a.cov3D_precomp = g->cov3D_precomp;
    a.view = cam->viewmatrix; a.proj = cam->projmatrix; a.campos = cam->campos;
    a.cull = (f->flags & RR_FLAG_NO_TILE_CULLING) ? 0 : 1;
    a.raw = (f->flags & RR_FLAG_RAW_PARAMS) ? 1 : 0;
    a.antialias = (f->flags & RR_FLAG_ANTIALIAS) ? 1 : 0;
    a.shs_rest = g->shs_rest;
    return a;
}

// The per-Gaussian backward's arguments that do not depend on the camera(s) or on gradient arrays.
GaussBwdArgs gauss_bwd_args(const rr_frame* f, const rr_gaussians* g, const rr_grads* out) {
    GaussBwdArgs a{};
    a.P = f->P; a.D = f->D; a.M = f->M;
    a.scale_modifier = f->scale_modifier;
    a.means3D = g->means3D; a.shs = g->shs; a.scales = g->scales; a.rotations = g->rotations;
    a.raw = (f->flags & RR_FLAG_RAW_PARAMS) ? 1 : 0; a.opacities = g->opacities; a.shs_rest = g->shs_rest;
    a.antialias = (f->flags & RR_FLAG_ANTIALIAS) ? 1 : 0;
    a.grad_accum = out->grad_accum; a.denom = out->denom; a.max_radii2D = out->max_radii2D;
    a.use_adam = out->adam ? 1 : 0;
    if (out->adam) a.adam = *out->adam;  // by value: the kernel must not dereference host memory
    return a;
}

// ---- the hand-off between a pair count, its render and the frame's backward ----
// One render per pair count, into the image buffer the count cleared, on the same thread; the
// workspace registered for the next render is consumed by that render (which zero-fills it inside
// its first blend launch); what the render leaves for its frame's backward is taken by the first
// backward of that image buffer.
struct WsRange {
    void* ptr = nullptr;
    size_t bytes = 0;
};
// What a render leaves for its frame's backward, which may run on another host thread (autograd's
// device thread): the workspace it zero-filled, and the backward's tile order when its phase-B
// duplicate launch computed it (the order array).  A backward whose workspace is the clean one
// skips its clear, and with the order ready it needs no prologue at all.
struct FrameFacts {
    const void* img = nullptr;
    WsRange clean;
    const uint32_t* order = nullptr;
};
struct Handoff {
    // This thread's.  counted_img: the image buffer whose per-frame block the last pair count
    // cleared, not yet rendered into (a second render after one pair count, whose gather counters
    // would start where the first one's ended, past their regions, fails instead).
    const void* counted_img = nullptr;
    WsRange fwd_ws;    // rr_set_forward_workspace: the backward's accumulators, for the next render
    FrameFacts facts;  // of the render in progress
    // Process-wide, keyed by the image buffer: the last few renders' facts.  The first backward of
    // a frame consumes its entry (a second one, of a retained graph, clears and orders by itself).
    static inline std::mutex mu;
    static inline std::deque<FrameFacts> published;
    static constexpr size_t kMaxFacts = 16;

    // false: no pair count of this image buffer to render.  ws: the workspace this render's first
    // blend launch zero-fills
    bool begin_render(const void* img, WsRange ws) {
        if (counted_img != img) return false;
        counted_img = nullptr;
        facts = FrameFacts{img, WsRange{}, nullptr};
        publish();  // drops an earlier render's facts of this buffer
        facts.clean = ws;
        return true;
    }
    int end_render(int rc) {
        if (rc == RR_OK) publish();
        return rc;
    }
    static FrameFacts remove(const void* img) {  // with mu held
        for (auto it = published.begin(); it != published.end(); ++it)
            if (it->img == img) {
                const FrameFacts f = *it;
                published.erase(it);
                return f;
            }
        return FrameFacts{};
    }
    void publish() const {
        std::lock_guard<std::mutex> lk(mu);
        remove(facts.img);
        if (facts.clean.ptr || facts.order) published.push_back(facts);
        if (published.size() > kMaxFacts) published.pop_front();
    }
    static FrameFacts take_facts(const void* img) {
        std::lock_guard<std::mutex> lk(mu);
        return remove(img);
    }
};
thread_local Handoff g_hand;

// Depth cut + the split pair-count scan -> the one device->host read of the forward, over a
// geometry buffer whose per-Gaussian arrays (splats, tiles, depth keys, block sums) are filled.  No
// depth sort: the bins' runs are put in depth order by k_sortexpand (rr_bin.hip).  The scan's first
// launch computes the cut and clears the image buffer's per-frame block (im: the buffer the frame
// is then rendered into).
int count_pairs(const rr_frame* f, const Geom& gm, const Img& im, int P, hipStream_t st, int* num_rendered,
                int* num_pairs) {
    PairCountRead rd;
    uint32_t* box = pair_counts_box(gm.ft, rd);
    const bool full = (f->flags & RR_FLAG_FULL_BINNING) != 0;
    const Tuning& tu = tuning();
    {
        StageTimer tm(RR_STAGE_SCAN, st);
        uint32_t* zero = reinterpret_cast<uint32_t*>(im.ranges);
        const int nzero = (int)(im.zero_bytes / sizeof(uint32_t));
        const CutArgs ca{gm.block_sums, gm.block_wide, full ? 1u : tu.early_den, tu.early_min, box, rd.seq};
        launch_split_scan(gm.tiles, gm.depth_keys, P, gm.lists, gm.ft, gm.temp, tu.pair_scan_direct_blocks, zero,
                          nzero, ca, st);
        RR_CHECK(hipGetLastError(), "pair-count scan");
    }
    g_hand.counted_img = im.final_T;
    RR_STAGE_CHECK("scan");
    // the one device->host sync of the forward (rasterizer_impl.cu:273): pairs to bin, and the
    // reference's num_rendered (sum of bounding-rect areas) which the API returns unchanged; the
    // split into the early-stop phases stays on the device
    PairCounts c;
    RR_CHECK(pair_counts_wait(rd, &c, st), "read L");
    if (c.L > 0x1fffffffu || c.rect > 0x7fffffffu) return fail(RR_ERR_CAPACITY, "more than 2^29 bin/Gaussian pairs");
    *num_rendered = (int)c.rect;
    *num_pairs = (int)c.L;
    return RR_OK;
}

struct PhaseLabels {
    const char *dup, *sort_why, *sort, *expand;
};
constexpr PhaseLabels kLabelsA{"duplicate", "bin sort (", "bin sort", "sort-expand"};
constexpr PhaseLabels kLabelsB{"duplicate (phase B)", "bin sort, phase B (", "bin sort (phase B)",
                               "sort-expand (phase B)"};
// One phase of the windowed binning path: what differs between phase A (or the only phase) and
// phase B.
struct WindowedPhase {
    uint32_t region;                     // where the phase's region of the pair arrays starts: 0 or L
    const uint32_t *n_list, *idx, *off;  // its list (PhaseLists) and, on the device, the list's entries (GA / GB)
    uint32_t* first;                     // its window starts, and whether they are computed already
    bool starts_done;
    const uint32_t* L_dev;               // device: the phase's pairs (FrameTotals LA / LB)
    RadixPlan plan;                      // of its bin sort, chosen for `hint` pairs
    size_t hint;
    uint32_t* unit_len;                  // phase B: pairs kept per window (sparse sort units), else null
    const uint32_t* n_dev;               // device: pairs the bin sort's later passes hold
    uint2* bounds;                       // the bins' runs
    uint32_t out_base;                   // where the phase's region of point_list starts
    uint2* ranges;                       // its tile lists
    const uint32_t* open_bits;           // phase B: tiles to expand for, else null
    PhaseLabels what;                    // the stages' names in error messages
};

// duplicate -> bin sort -> sort-expand of one phase.  d: the duplicate's arguments that the phases
// share, and the ones only one of them sets (phase A's second window set, phase B's filter and
// tile order).  Returns in *starts whether the duplicate computed the window starts.
template <typename K>
int windowed_phase(const rr_frame* f, const Geom& gm, const Bin& bn, DupArgs<K>& d, const WindowedPhase& w,
                   hipStream_t st, bool* starts) {
    K* keys = static_cast<K*>(bn.keys) + w.region;
    K* keys_sorted = static_cast<K*>(bn.keys_sorted) + w.region;
    uint32_t* vals = bn.vals + w.region;
    uint32_t* vals_sorted = bn.vals_sorted + w.region;
    {
        StageTimer tm(RR_STAGE_DUPLICATE, st);
        d.n_list = w.n_list; d.idx = w.idx; d.off = w.off; d.first = w.first;
        d.pair0 = 0; d.win = (uint32_t)w.plan.unit_items; d.nwin = w.plan.units; d.L_dev = w.L_dev;
        d.keys = keys; d.vals = vals; d.dbits = w.plan.dbits0; d.counts = w.plan.counts;
        d.unit_len = w.unit_len;
        d.starts_done = w.starts_done;
        *starts = launch_duplicate<K>(d, st);
        d.first_b = nullptr; d.nwin_b = 0; d.starts_done = false;
    }
    RR_STAGE_CHECK(w.what.dup);
    {
        StageTimer tm(RR_STAGE_TILE_SORT, st);
        RR_CHECK(radix_sort_pairs<K>(bn.temp, bn.temp_bytes, keys, keys_sorted, vals, vals_sorted, bn.L, 0, bn.bits, st,
                                     true, w.unit_len, w.n_dev, w.hint, w.bounds),
                 std::string(w.what.sort_why) + radix_sort_last_error() + ")");
    }
    RR_STAGE_CHECK(w.what.sort);
    return stage(f, st, RR_STAGE_RANGES, w.what.expand, [&] {
        launch_sortexpand<K>(keys_sorted, vals_sorted, gm.depth_keys, gm.ft, d.gx, d.gy, w.out_base, bn.point_list,
                             w.ranges, w.open_bits, w.bounds, st);
    });
}

// Tile lists for one frame: duplicate -> pairs into their bins -> per-bin depth order + tile lists
// -> blend, once (single phase) or as the two phases of early-stop binning (rr_kernels.hpp
// BlendPhase).  The host knows the frame's total L only: phase A's pairs go to region [0, L) of the
// pair arrays and phase B's to region [L, 2L); every launch is sized for L and reads its phase's
// count on the device (FrameTotals LA / LB, or the gather path's counters).
template <typename K>
int render_tiles(const rr_frame* f, const Geom& gm, const Img& im, const Bin& bn, const int* radii, int P, int W,
                 int H, int cull, bool early, BlendFwdArgs b, const DistFwdArgs& dm, hipStream_t st) {
    const int gx = grid_x(W), gy = grid_y(H);
    const uint32_t L = bn.L;
    DupArgs<K> d{};
    d.P = P; d.splats = gm.splats; d.radii = radii;
    d.gx = gx; d.gy = gy; d.cull = cull;
    d.tiles = gm.tiles;
    const PhaseHints h = phase_hints(L, early);
    const bool gather = early && b_gather(W, H);
    const RadixPlan pa = tile_plan<K>(bn.temp, L, bn.bits, h.a);  // phase A (or the only phase)
    const RadixPlan pb = tile_plan<K>(bn.temp, L, bn.bits, h.b);  // phase B (windowed path)
    // window starts marked by the split scan (units of kSplitWin pairs), else a window-starts launch
    const bool marks_a = pa.unit_items == kSplitWin && (uint32_t)pa.units <= gm.lists.nwin;
    const bool marks_b = pb.unit_items == kSplitWin && (uint32_t)pb.units <= gm.lists.nwin;
    // phase A (or the only phase): its pairs for every tile
    if (early && !gather && !marks_a && !marks_b) {  // phase B's window starts computed with phase A's
        d.first_b = bn.first + pa.units; d.pair0_b = 0; d.win_b = (uint32_t)pb.unit_items; d.nwin_b = pb.units;
        d.n_list_b = &gm.ft->GB; d.off_b = gm.lists.off_b;
    }
    bool starts_b = false, starts = false;
    const WindowedPhase wa{0u, &gm.ft->GA, gm.lists.idx_a, gm.lists.off_a, marks_a ? gm.lists.first_a : bn.first,
                           marks_a, &gm.ft->LA, pa, h.a, nullptr, &gm.ft->LA, im.bounds_a, 0u, im.ranges, nullptr,
                           kLabelsA};
    if (int rc = windowed_phase<K>(f, gm, bn, d, wa, st, &starts_b)) return rc;
    b.phase = early ? kBlendPhaseA : kBlendSingle;
    // (clears the registered backward workspace, render_frame, in its drain)
    if (int rc = stage(f, st, RR_STAGE_BLEND_FWD, "blend forward", [&] { launch_blend_fwd(b, st, &dm); })) return rc;
    b.clear = nullptr;
    b.clear_n4 = 0;
    if (!early) return RR_OK;
    // phase B: its pairs, only for tiles phase A left open; region [L, 2L) of the pair arrays.  The
    // backward's tile order is computed on phase A's tile_max by an extra workgroup of the phase-B
    // duplicate launch (counters[1] = T marks it done)
    d.open_bits = im.open_bits; d.n_total = im.counters;
    d.order_cost = im.tile_max; d.order_out = im.order; d.order_flag = im.counters + 1; d.order_T = gx * gy;
    if (P > 0) g_hand.facts.order = im.order;
    if (gather) {
        K* keys = static_cast<K*>(bn.keys);
        d.keys = keys + L; d.vals = bn.vals + L;
        d.n_list = &gm.ft->GB; d.idx = gm.lists.idx_b;
        d.gather_mark = im.counters + 2;
        if (int rc = stage(f, st, RR_STAGE_DUPLICATE, "duplicate (phase B gather)", [&] { launch_dup_gather<K>(d, st); }))
            return rc;
        // phase B's tile lists right after phase A's
        if (int rc = stage(f, st, RR_STAGE_RANGES, "sort-expand (phase B gather)", [&] {
                launch_sortexpand_small<K>(P, keys + L, bn.vals + L, im.counters, im.bin_cnt, bn.vals_sorted + L,
                                           gm.depth_keys, gm.ft, gx, gy, 4u * L, bn.point_list, im.ranges_b,
                                           im.open_bits, im.bounds_b, im.counters + 3, st);
            }))
            return rc;
    } else {
        const WindowedPhase wb{L, &gm.ft->GB, gm.lists.idx_b, gm.lists.off_b,
                               marks_b ? gm.lists.first_b : bn.first + pa.units, starts_b || marks_b, &gm.ft->LB, pb,
                               h.b, bn.unit_len, im.counters, im.bounds_b, 4u * L, im.ranges_b, im.open_bits,
                               kLabelsB};
        if (int rc = windowed_phase<K>(f, gm, bn, d, wb, st, &starts)) return rc;
    }
    b.phase = kBlendPhaseB;
    return stage(f, st, RR_STAGE_BLEND_FWD, "blend forward (phase B)", [&] { launch_blend_fwd(b, st, &dm); });
}

// Binning + blend of a frame whose pairs were just counted (count_pairs) into this image buffer.
int render_frame(const rr_frame* f, const rr_camera* cam, const int* radii, void* geom_buffer, void* image_buffer,
                 void* binning_buffer, size_t binning_bytes, int num_pairs, float* out_color, float* out_depth,
                 float* out_normal, void* stream, const DistFwdArgs& dm) {  // dm.out_moments null: no moment maps
    const int P = f->P, W = f->width, H = f->height, L = num_pairs;
    const int cull = (f->flags & RR_FLAG_NO_TILE_CULLING) ? 0 : 1;
    const WsRange reg = std::exchange(g_hand.fwd_ws, WsRange{});  // used by this render, or dropped by it
    if (P == 0) return RR_OK;
    if (!out_color || !out_depth || !geom_buffer || !image_buffer || (L > 0 && !binning_buffer))
        return fail(RR_ERR_ARG, "null buffer");
    const Geom gm = carve_geom(geom_buffer, P);
    const Img im = carve_img(image_buffer, W, H);
    if (!g_hand.begin_render(im.final_T, reg))
        return fail(RR_ERR_ARG, "render without a pair count of this image buffer (one render per rr_forward_geometry / "
                                "rr_forward_from_geometry on this thread)");
    const Bin bn = carve_bin(binning_buffer, L, W, H);
    if (L > 0 && binning_bytes < bn.total) return fail(RR_ERR_CAPACITY, "binning buffer too small");
    hipStream_t st = (hipStream_t)stream;
    const int gx = grid_x(W), gy = grid_y(H);
    // (the per-frame block of the image buffer was cleared by count_pairs' split scan)
    BlendFwdArgs b{};
    b.W = W; b.H = H; b.gx = gx; b.gy = gy;
    b.ranges = im.ranges; b.ranges_b = im.ranges_b; b.open = im.open; b.open_bits = im.open_bits;
    b.point_list = bn.point_list; b.splats = gm.splats; b.bg = cam->background;
    b.final_T = im.final_T; b.n_contrib = im.n_contrib; b.tile_max = im.tile_max;
    b.clear = static_cast<float4*>(reg.ptr);
    b.clear_n4 = reg.bytes / sizeof(float4);
    b.out_color = out_color; b.out_depth = out_depth;
    b.normals = out_normal ? gm.normals : nullptr; b.out_normal = out_normal;
    if (L == 0) {  // no pairs: every tile keeps the background (one blend over empty lists)
        b.phase = kBlendSingle;
        return g_hand.end_render(
            stage(f, st, RR_STAGE_BLEND_FWD, "blend forward", [&] { launch_blend_fwd(b, st, &dm); }));
    }
    // the split the depth cut makes (its one-phase conditions but "no sampled pair", which leaves
    // phase B empty on the device)
    const Tuning& tu = tuning();
    const bool early = !(f->flags & RR_FLAG_FULL_BINNING) && tu.early_den > 1 && (uint32_t)L >= tu.early_min;
    return g_hand.end_render(bn.wide ? render_tiles<uint32_t>(f, gm, im, bn, radii, P, W, H, cull, early, b, dm, st)
                                     : render_tiles<uint16_t>(f, gm, im, bn, radii, P, W, H, cull, early, b, dm, st));
}

// The tail of rr_forward and rr_forward_from_geometry after the pair count: the binning buffer's
// size query, RR_INCOMPLETE when the given one is smaller, else the render.
int finish_forward(const rr_frame* f, const rr_camera* cam, const int* radii, void* geom_buffer, void* image_buffer,
                   void* binning_buffer, size_t binning_bytes, int num_pairs, size_t* binning_needed, float* out_color,
                   float* out_depth, void* stream) {
    const size_t need = num_pairs > 0 ? carve_bin(nullptr, num_pairs, f->width, f->height).total : 0;
    *binning_needed = need;
    if (binning_bytes < need) return RR_INCOMPLETE;
    // (rr_forward only: rr_forward_from_geometry refuses the flag before it counts)
    if (f->flags & RR_FLAG_AUX_NORMAL) return fail(RR_ERR_ARG, "RR_FLAG_AUX_NORMAL: use rr_forward_render_aux");
    return render_frame(f, cam, radii, geom_buffer, image_buffer, binning_buffer, binning_bytes, num_pairs, out_color,
                        out_depth, nullptr, stream, DistFwdArgs{});
}

// Accumulator clear (+ the backward's tile order) and the blend backward: gacc [P][GACC_STRIDE]
// receives every Gaussian's dmean2D / dconic / dopacity / dcolor sums of the frame.  `mode` is
// plan_backward(pg, ...).blend (rr_bwd_plan.hpp): the depth modes also leave dL/d(view depth) in slot 9
// (the moments' share included), the normal modes dL/d(normal) in slots 10..12.
int blend_backward(const rr_frame* f, const rr_camera* cam, const void* geom_buffer, const void* image_buffer,
                   const void* binning_buffer, int L, const PixelGrads& pg, BlendBwdMode mode, float* gacc,
                   hipStream_t st) {
    const int P = f->P, W = f->width, H = f->height;
    const Geom gm = carve_geom(const_cast<void*>(geom_buffer), P);
    const Img im = carve_img(const_cast<void*>(image_buffer), W, H);
    // point_list sits at the start of the binning buffer, so its position does not depend on the
    // pair count (tests/host/layout_check.hip); tiles whose forward blended nothing (tile_max 0)
    // never read it
    const Bin bn = carve_bin(const_cast<void*>(binning_buffer), 0, W, H);
    const int gx = grid_x(W), gy = grid_y(H);
    const bool blend = L > 0 && binning_buffer;
    uint32_t* order = blend ? im.order : nullptr;  // heaviest tiles first
    // the accumulators already zero-filled by the forward (rr_set_forward_workspace): no clear
    const size_t nacc = (size_t)P * GACC_STRIDE;
    const FrameFacts facts = Handoff::take_facts(im.final_T);  // this backward's accumulation dirties the workspace
    const bool clean = (f->flags & RR_FLAG_WORKSPACE_REGISTERED) && facts.clean.ptr == gacc &&
                       facts.clean.bytes >= nacc * sizeof(float);
    const bool order_ready = order && facts.order == order;
    if (!clean || (order && !order_ready)) {
        StageTimer tm(RR_STAGE_MEMSET, st);
        launch_bwd_prologue(gacc, clean ? 0 : nacc, gx * gy, im.tile_max, order_ready ? nullptr : order,
                            im.counters + 1, st);
        RR_CHECK(hipGetLastError(), "clear accumulators");
    }
    if (blend) {
        StageTimer tm(RR_STAGE_BLEND_BWD, st);
        BlendBwdArgs b{};
        b.W = W; b.H = H; b.gx = gx; b.gy = gy;
        b.ranges = im.ranges; b.ranges_b = im.ranges_b; b.point_list = bn.point_list; b.splats = gm.splats;
        b.tile_max = im.tile_max;
        b.final_T = im.final_T; b.n_contrib = im.n_contrib; b.bg = cam->background; b.dL_dpix = pg.dL_dpix;
        b.gacc = gacc;
        b.order = order;
        launch_blend_bwd(b, pg, mode, gm.normals, st);
    }
    RR_STAGE_CHECK("blend backward");
    return RR_OK;
}

// The five rr_backward* entry points: pg holds the output gradients the entry point takes (with an aux
// map dL_dpix may be null), cg the camera-gradient block of rr_backward_camera or null.
int backward_impl(const rr_frame* f, const rr_camera* cam, const rr_gaussians* g, const int* radii,
                  const void* geom_buffer, const void* image_buffer, const void* binning_buffer, int num_rendered,
                  const PixelGrads& pg, void* workspace, size_t workspace_bytes, const rr_grads* out,
                  const rr_camera_grads* cg, void* stream);

}  // namespace

extern "C" {

size_t rr_geometry_bytes(int P) { return carve_geom(nullptr, P).total; }
size_t rr_image_bytes(int width, int height) { return carve_img(nullptr, width, height).total; }
size_t rr_binning_bytes(int num_rendered, int width, int height) {
    return carve_bin(nullptr, num_rendered, width, height).total;
}
size_t rr_backward_workspace_bytes(int P) { return align_up((size_t)std::max(P, 1) * GACC_STRIDE * sizeof(float)); }
size_t rr_camera_grad_scratch_bytes(int P) {
    return align_up((size_t)cam_grad_rows(std::max(P, 0)) * kCamGradRow * sizeof(float));
}

int rr_forward_geometry(const rr_frame* f, const rr_camera* cam, const rr_gaussians* g, int* radii, void* geom_buffer,
                        size_t geom_bytes, void* image_buffer, size_t image_bytes, int* num_rendered,
                        int* num_pairs, void* stream) {
    int rc = validate(f, cam, g, true);
    if (rc) return rc;
    if (!num_rendered || !num_pairs) return fail(RR_ERR_ARG, "num_rendered / num_pairs is null");
    *num_rendered = 0;
    *num_pairs = 0;
    const int P = f->P, W = f->width, H = f->height;
    if (P == 0) return RR_OK;
    if (!radii || !geom_buffer || !image_buffer) return fail(RR_ERR_ARG, "null output buffer");
    const Geom gm = carve_geom(geom_buffer, P);
    const Img im = carve_img(image_buffer, W, H);
    if (geom_bytes < gm.total || image_bytes < im.total) return fail(RR_ERR_CAPACITY, "scratch buffer too small");
    hipStream_t st = (hipStream_t)stream;
    PreArgs a = pre_args(f, cam, g);
    a.radii = radii; a.splats = gm.splats; a.tiles = gm.tiles; a.depth_keys = gm.depth_keys;
    a.normals = (f->flags & RR_FLAG_AUX_NORMAL) ? gm.normals : nullptr;
    a.block_sums = gm.block_sums;
    a.block_wide = gm.block_wide;
    if (int rc2 = stage(f, st, RR_STAGE_PREPROCESS, "preprocess", [&] { launch_preprocess(a, st); })) return rc2;
    return count_pairs(f, gm, im, P, st, num_rendered, num_pairs);
}

int rr_forward_render_aux(const rr_frame* f, const rr_camera* cam, const rr_gaussians* g, const int* radii,
                          void* geom_buffer, void* image_buffer, void* binning_buffer, size_t binning_bytes,
                          int num_pairs, float* out_color, float* out_depth, float* out_normal, void* stream) {
    int rc = validate(f, cam, g, true);
    if (rc) return rc;
    if (((f->flags & RR_FLAG_AUX_NORMAL) != 0) != (out_normal != nullptr))
        return fail(RR_ERR_ARG, "out_normal must be given exactly when RR_FLAG_AUX_NORMAL is set");
    return render_frame(f, cam, radii, geom_buffer, image_buffer, binning_buffer, binning_bytes, num_pairs, out_color,
                        out_depth, out_normal, stream, DistFwdArgs{});
}

int rr_forward_render_dist(const rr_frame* f, const rr_camera* cam, const rr_gaussians* g, const int* radii,
                           void* geom_buffer, void* image_buffer, void* binning_buffer, size_t binning_bytes,
                           int num_pairs, float* out_color, float* out_depth, float* out_normal, float* out_moments,
                           float dist_near, float dist_far, void* stream) {
    int rc = validate(f, cam, g, true);
    if (rc) return rc;
    if (((f->flags & RR_FLAG_AUX_NORMAL) != 0) != (out_normal != nullptr))
        return fail(RR_ERR_ARG, "out_normal must be given exactly when RR_FLAG_AUX_NORMAL is set");
    if (!out_moments) return fail(RR_ERR_ARG, "out_moments is null (rr_forward_render_aux renders without moments)");
    if (!dist_range_ok(dist_near, dist_far))
        return fail(RR_ERR_ARG, "dist_near / dist_far must be 0 < near < far, or both 0 (metric depth)");
    const DistFwdArgs dm{out_moments, dist_near, dist_scale_of(dist_near, dist_far)};
    return render_frame(f, cam, radii, geom_buffer, image_buffer, binning_buffer, binning_bytes, num_pairs, out_color,
                        out_depth, out_normal, stream, dm);
}

int rr_forward_render(const rr_frame* f, const rr_camera* cam, const rr_gaussians* g, const int* radii,
                      void* geom_buffer, void* image_buffer, void* binning_buffer, size_t binning_bytes,
                      int num_pairs, float* out_color, float* out_depth, void* stream) {
    if (f && (f->flags & RR_FLAG_AUX_NORMAL)) return fail(RR_ERR_ARG, "RR_FLAG_AUX_NORMAL: use rr_forward_render_aux");
    return rr_forward_render_aux(f, cam, g, radii, geom_buffer, image_buffer, binning_buffer, binning_bytes, num_pairs,
                                 out_color, out_depth, nullptr, stream);
}

int rr_forward(const rr_frame* f, const rr_camera* cam, const rr_gaussians* g, int* radii, void* geom_buffer,
               size_t geom_bytes, void* image_buffer, size_t image_bytes, void* binning_buffer, size_t binning_bytes,
               int* num_rendered, int* num_pairs, size_t* binning_needed, float* out_color, float* out_depth,
               void* stream) {
    if (!binning_needed) return fail(RR_ERR_ARG, "binning_needed is null");
    *binning_needed = 0;
    int rc = rr_forward_geometry(f, cam, g, radii, geom_buffer, geom_bytes, image_buffer, image_bytes, num_rendered,
                                 num_pairs, stream);
    if (rc != RR_OK || f->P == 0) return rc;
    return finish_forward(f, cam, radii, geom_buffer, image_buffer, binning_buffer, binning_bytes, *num_pairs,
                          binning_needed, out_color, out_depth, stream);
}

int rr_backward(const rr_frame* f, const rr_camera* cam, const rr_gaussians* g, const int* radii,
                const void* geom_buffer, const void* image_buffer, const void* binning_buffer, int num_rendered,
                const float* dL_dpix, void* workspace, size_t workspace_bytes, const rr_grads* out, void* stream) {
    return backward_impl(f, cam, g, radii, geom_buffer, image_buffer, binning_buffer, num_rendered,
                         PixelGrads{dL_dpix}, workspace, workspace_bytes, out, nullptr, stream);
}

int rr_backward_aux(const rr_frame* f, const rr_camera* cam, const rr_gaussians* g, const int* radii,
                    const void* geom_buffer, const void* image_buffer, const void* binning_buffer, int num_rendered,
                    const float* dL_dpix, const float* dL_ddepth, const float* dL_dalpha, void* workspace,
                    size_t workspace_bytes, const rr_grads* out, void* stream) {
    return backward_impl(f, cam, g, radii, geom_buffer, image_buffer, binning_buffer, num_rendered,
                         PixelGrads{dL_dpix, dL_ddepth, dL_dalpha}, workspace, workspace_bytes, out, nullptr, stream);
}

int rr_backward_camera(const rr_frame* f, const rr_camera* cam, const rr_gaussians* g, const int* radii,
                       const void* geom_buffer, const void* image_buffer, const void* binning_buffer, int num_rendered,
                       const float* dL_dpix, const float* dL_ddepth, const float* dL_dalpha, void* workspace,
                       size_t workspace_bytes, const rr_grads* out, const rr_camera_grads* cg, void* stream) {
    return backward_impl(f, cam, g, radii, geom_buffer, image_buffer, binning_buffer, num_rendered,
                         PixelGrads{dL_dpix, dL_ddepth, dL_dalpha}, workspace, workspace_bytes, out, cg, stream);
}

int rr_backward_aux_normal(const rr_frame* f, const rr_camera* cam, const rr_gaussians* g, const int* radii,
                           const void* geom_buffer, const void* image_buffer, const void* binning_buffer,
                           int num_rendered, const float* dL_dpix, const float* dL_ddepth, const float* dL_dalpha,
                           const float* dL_dnormal, void* workspace, size_t workspace_bytes, const rr_grads* out,
                           void* stream) {
    return backward_impl(f, cam, g, radii, geom_buffer, image_buffer, binning_buffer, num_rendered,
                         PixelGrads{dL_dpix, dL_ddepth, dL_dalpha, dL_dnormal}, workspace, workspace_bytes, out,
                         nullptr, stream);
}

int rr_backward_aux_dist(const rr_frame* f, const rr_camera* cam, const rr_gaussians* g, const int* radii,
                         const void* geom_buffer, const void* image_buffer, const void* binning_buffer,
                         int num_rendered, const float* dL_dpix, const float* dL_ddepth, const float* dL_dalpha,
                         const float* dL_dnormal, const float* dL_dmoments, float dist_near, float dist_far,
                         void* workspace, size_t workspace_bytes, const rr_grads* out, void* stream) {
    return backward_impl(f, cam, g, radii, geom_buffer, image_buffer, binning_buffer, num_rendered,
                         PixelGrads{dL_dpix, dL_ddepth, dL_dalpha, dL_dnormal, dL_dmoments, dist_near, dist_far},
                         workspace, workspace_bytes, out, nullptr, stream);
}

int rr_render_alpha(const rr_frame* f, const void* image_buffer, float* out_alpha, void* stream) {
    if (!f) return fail(RR_ERR_ARG, "null frame");
    const int P = f->P, W = f->width, H = f->height;
    if (P < 0 || W <= 0 || H <= 0) return fail(RR_ERR_ARG, "bad P / width / height");
    if (!out_alpha) return fail(RR_ERR_ARG, "null output buffer");
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)W * H;
    if (P == 0) {  // nothing was rendered: every pixel keeps T = 1
        RR_CHECK(hipMemsetAsync(out_alpha, 0, n * sizeof(float), st), "render alpha");
        return RR_OK;
    }
    if (!image_buffer) return fail(RR_ERR_ARG, "null image buffer");
    const Img im = carve_img(const_cast<void*>(image_buffer), W, H);
    launch_render_alpha(im.final_T, n, out_alpha, st);
    return check(f, st, "render alpha");
}

int rr_contributions(const rr_frame* f, const int* radii, const void* geom_buffer, const void* image_buffer,
                     const void* binning_buffer, int num_rendered, const float* pixel_weight, int accumulate,
                     rr_contrib* out, void* stream) {
    if (!f) return fail(RR_ERR_ARG, "null frame");
    const int P = f->P, W = f->width, H = f->height;
    if (P < 0 || W <= 0 || H <= 0) return fail(RR_ERR_ARG, "bad P / width / height");
    if (num_rendered < 0) return fail(RR_ERR_ARG, "bad num_rendered");
    if (!out) return fail(RR_ERR_ARG, "null output buffer");
    if (((uintptr_t)out & 15u) != 0) return fail(RR_ERR_ARG, "out is not 16-byte aligned");
    if (P == 0) return RR_OK;  // no records
    if (!radii || !geom_buffer || !image_buffer) return fail(RR_ERR_ARG, "null buffer");
    hipStream_t st = (hipStream_t)stream;
    uint32_t* rec = reinterpret_cast<uint32_t*>(out);
    if (!accumulate) launch_contrib_clear(rec, P, st);
    // nothing visible, or a frame without pairs (it has no binning buffer): no list to walk
    if (num_rendered > 0 && binning_buffer) {
        const Geom gm = carve_geom(const_cast<void*>(geom_buffer), P);
        const Img im = carve_img(const_cast<void*>(image_buffer), W, H);
        const Bin bn = carve_bin(const_cast<void*>(binning_buffer), 0, W, H);  // point_list comes first
        ContribArgs a{};
        a.P = P; a.W = W; a.H = H; a.gx = grid_x(W); a.gy = grid_y(H);
        a.ranges = im.ranges; a.ranges_b = im.ranges_b; a.point_list = bn.point_list; a.splats = gm.splats;
        a.tile_max = im.tile_max; a.n_contrib = im.n_contrib; a.pixel_weight = pixel_weight;
        a.out = rec;
        launch_contrib(a, st);
    }
    return check(f, st, "contributions");
}

}  // extern "C"

namespace {

int backward_impl(const rr_frame* f, const rr_camera* cam, const rr_gaussians* g, const int* radii,
                  const void* geom_buffer, const void* image_buffer, const void* binning_buffer, int num_rendered,
                  const PixelGrads& pg, void* workspace, size_t workspace_bytes, const rr_grads* out,
                  const rr_camera_grads* cg, void* stream) {
    int rc = validate(f, cam, g, false);
    if (rc) return rc;
    if (pg.dL_dmoments && !dist_range_ok(pg.dist_near, pg.dist_far))
        return fail(RR_ERR_ARG, "dist_near / dist_far must be 0 < near < far, or both 0 (metric depth)");
    const int P = f->P, W = f->width, H = f->height, L = num_rendered;
    if (cg && (f->flags & RR_FLAG_ANTIALIAS))
        return fail(RR_ERR_ARG, "RR_FLAG_ANTIALIAS: camera gradients of an anti-aliased frame are not supported yet");
    const bool absgrad = (f->flags & RR_FLAG_ABSGRAD) != 0;
    if (absgrad && cg)
        return fail(RR_ERR_ARG, "RR_FLAG_ABSGRAD: rr_backward_camera is not supported yet");
    if (absgrad && pg.aux())
        return fail(RR_ERR_ARG, "RR_FLAG_ABSGRAD: absolute gradients together with a depth / alpha / normal / moments "
                                "gradient are not supported yet");
    if (!absgrad && out && out->dL_dmeans2D_abs)
        return fail(RR_ERR_ARG, "rr_grads.dL_dmeans2D_abs needs RR_FLAG_ABSGRAD");
    if (cg) {  // camera gradients (rr_backward_camera): every refusal before any device work
        if (!cg->dL_dviewmatrix || !cg->dL_dprojmatrix || !cg->dL_dcampos)
            return fail(RR_ERR_ARG, "rr_camera_grads: null gradient output");
        if (!cg->scratch || ((uintptr_t)cg->scratch & 15u) != 0)
            return fail(RR_ERR_ARG, "rr_camera_grads: scratch is null or not 16-byte aligned");
        if (pg.dL_dnormal || pg.dL_dmoments)
            return fail(RR_ERR_ARG, "camera gradients do not combine with dL_dnormal / dL_dmoments yet");
        if (out && (out->adam || out->next))
            return fail(RR_ERR_ARG, "camera gradients do not combine with rr_grads.adam / rr_grads.next");
        if (cg->scratch_bytes < rr_camera_grad_scratch_bytes(P))
            return fail(RR_ERR_CAPACITY, "rr_camera_grads: scratch too small");
    }
    if (P == 0) {
        if (cg) {  // nothing rendered: the three arrays are zeros
            hipStream_t st0 = (hipStream_t)stream;
            RR_CHECK(hipMemsetAsync(cg->dL_dviewmatrix, 0, 16 * sizeof(float), st0), "camera gradients");
            RR_CHECK(hipMemsetAsync(cg->dL_dprojmatrix, 0, 16 * sizeof(float), st0), "camera gradients");
            RR_CHECK(hipMemsetAsync(cg->dL_dcampos, 0, 3 * sizeof(float), st0), "camera gradients");
        }
        return RR_OK;
    }
    if (!out || !pg.any() || !radii || !geom_buffer || !image_buffer || !workspace)
        return fail(RR_ERR_ARG, "null buffer");
    if (pg.dL_dnormal) {
        if (!(f->flags & RR_FLAG_AUX_NORMAL))
            return fail(RR_ERR_ARG, "dL_dnormal needs a frame rendered with RR_FLAG_AUX_NORMAL");
        if (!g->scales || !g->rotations)
            return fail(RR_ERR_ARG, "dL_dnormal needs scales/rotations (not cov3D_precomp)");
    }
    const bool raw = (f->flags & RR_FLAG_RAW_PARAMS) != 0;
    const rr_adam* ad = out->adam;
    if (ad && !raw) return fail(RR_ERR_ARG, "the fused optimizer step needs raw-parameter mode");
    if (ad) {  // every group is stepped (which rr_grads.next relies on)
        if (int rc2 = check_adam(f, g, ad, true)) return rc2;
    } else if (!out->dL_dopacity || !out->dL_dmeans3D || !out->dL_dscales || !out->dL_drotations ||
               (f->M > 0 && !out->dL_dsh) ||
               (!raw && (!out->dL_dmeans2D || !out->dL_dcolors || !out->dL_dcov3D)) ||
               (raw && f->M > 1 && !out->dL_dsh_rest)) {
        return fail(RR_ERR_ARG, "null gradient output");
    }
    if (!raw && !out->dL_dopacity) return fail(RR_ERR_ARG, "null gradient output");
    if (out->grad_accum && (!raw || !out->denom || !out->max_radii2D))
        return fail(RR_ERR_ARG, "densification statistics need raw mode and grad_accum, denom, max_radii2D");
    if (workspace_bytes < rr_backward_workspace_bytes(P)) return fail(RR_ERR_CAPACITY, "workspace too small");
    const rr_next_frame* nx = out->next;
    if (nx) {  // cross-step fusion: the next frame's preprocess on the stepped parameters
        if (!ad) return fail(RR_ERR_ARG, "rr_grads.next needs the fused optimizer step (rr_grads.adam)");
        if (!nx->frame || !nx->cam || !nx->radii || !nx->geom_buffer)
            return fail(RR_ERR_ARG, "rr_next_frame: null frame / camera / radii / geometry buffer");
        const rr_frame* nf = nx->frame;
        if (nf->P != P || nf->M != f->M || nf->D != f->D || !(nf->flags & RR_FLAG_RAW_PARAMS) ||
            (nf->flags & RR_FLAG_AUX_NORMAL) || nf->prefiltered)
            return fail(RR_ERR_ARG, "rr_next_frame: the next frame must have the same P, M and SH degree, raw "
                                    "parameters, no aux normals, no prefiltering");
        if (nf->width <= 0 || nf->height <= 0) return fail(RR_ERR_ARG, "rr_next_frame: bad width / height");
        if (!nx->cam->viewmatrix || !nx->cam->projmatrix || !nx->cam->campos)
            return fail(RR_ERR_ARG, "rr_next_frame: camera arrays are required");
        if (nx->geom_bytes < carve_geom(nullptr, P).total) return fail(RR_ERR_CAPACITY, "next geometry buffer too small");
        if (nx->geom_buffer == geom_buffer) return fail(RR_ERR_ARG, "rr_next_frame: the next frame needs its own geometry buffer");
    }
    hipStream_t st = (hipStream_t)stream;
    float* gacc = static_cast<float*>(workspace);
    const BwdPlan plan = plan_backward(pg, cg != nullptr, absgrad);
    if (int rc2 = blend_backward(f, cam, geom_buffer, image_buffer, binning_buffer, L, pg, plan.blend, gacc, st))
        return rc2;
    {
        StageTimer tm(RR_STAGE_GAUSS_BWD, st);
        GaussBwdArgs a = gauss_bwd_args(f, g, out);
        a.tanfovx = f->tan_fovx; a.tanfovy = f->tan_fovy;
        a.focal_y = focal(H, f->tan_fovy);
        a.focal_x = focal(W, f->tan_fovx);
        a.low_pass = f->low_pass;
        a.cov3D_precomp = g->cov3D_precomp; a.view = cam->viewmatrix; a.proj = cam->projmatrix;
        a.campos = cam->campos; a.radii = radii; a.gacc = gacc;
        a.dL_dmeans2D = out->dL_dmeans2D; a.dL_dcolors = out->dL_dcolors; a.dL_dopacity = out->dL_dopacity;
        a.dL_dmeans3D = out->dL_dmeans3D; a.dL_dcov3D = out->dL_dcov3D; a.dL_dsh = f->M > 0 ? out->dL_dsh : nullptr;
        a.dL_dscales = out->dL_dscales; a.dL_drot = out->dL_drotations;
        a.dL_dsh_rest = out->dL_dsh_rest;
        if (a.antialias) a.splats = carve_geom(const_cast<void*>(geom_buffer), P).splats;
        if (absgrad) {  // the absolute sums and the statistics on them in a pass of their own (rr_kernels.hpp)
            launch_abs_stats(P, gacc, radii, out->dL_dmeans2D_abs, a.grad_accum, a.denom, a.max_radii2D, st);
            a.grad_accum = nullptr; a.denom = nullptr; a.max_radii2D = nullptr;
        }
        if (nx) {
            const Geom ng = carve_geom(nx->geom_buffer, P);
            PreArgs n = pre_args(nx->frame, nx->cam, g);
            n.radii = nx->radii; n.splats = ng.splats; n.tiles = ng.tiles; n.depth_keys = ng.depth_keys;
            n.block_sums = ng.block_sums; n.block_wide = ng.block_wide; n.n_out = P;
            a.next = n;
            a.has_next = 1;
        }
        if (plan.gauss == kGaussBwdCam)
            launch_gauss_bwd_cam(a, static_cast<float*>(cg->scratch), cg->dL_dviewmatrix, cg->dL_dprojmatrix,
                                 cg->dL_dcampos, st);
        else launch_gauss_bwd(a, plan.gauss, st);
    }
    RR_STAGE_CHECK("gaussian backward");
    return RR_OK;
}

}  // namespace

extern "C" {

int rr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present,
                    void* stream) {
    (void)projmatrix;
    if (P < 0) return fail(RR_ERR_ARG, "bad P");
    if (P == 0) return RR_OK;
    if (!means3D || !viewmatrix || !present) return fail(RR_ERR_ARG, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    launch_mark_visible(P, means3D, viewmatrix, present, st);
    return check(nullptr, st, "mark_visible");
}

int rr_set_forward_workspace(void* workspace, size_t bytes) {
    if (workspace && (((uintptr_t)workspace & 15u) != 0 || bytes % 16 != 0))
        return fail(RR_ERR_ARG, "workspace must be 16-byte aligned and a multiple of 16 bytes");
    g_hand.fwd_ws = workspace && bytes ? WsRange{workspace, bytes} : WsRange{};
    return RR_OK;
}

int rr_host_wait_stats(int reset, int64_t* wait_ns, int64_t* waits) {
    if (wait_ns) *wait_ns = g_wait_ns;
    if (waits) *waits = g_waits;
    if (reset) g_wait_ns = g_waits = 0;
    return RR_OK;
}

// ---- Gaussian-sharded multi-GPU step (include/rain_raster.h, "row blocks") ----

int rr_geometry_layout(int P, size_t* offsets) {
    if (P < 0 || !offsets) return fail(RR_ERR_ARG, "bad P / null offsets");
    // carve over a stand-in base address (a null base carves null pointers) and subtract it
    constexpr uintptr_t kBase = 1u << 20;
    const Geom gm = carve_geom(reinterpret_cast<void*>(kBase), P);
    auto off = [](const void* p) { return (size_t)(reinterpret_cast<uintptr_t>(p) - kBase); };
    offsets[0] = off(gm.splats);
    offsets[1] = off(gm.tiles);
    offsets[2] = off(gm.depth_keys);
    offsets[3] = off(gm.block_sums);
    offsets[4] = off(gm.block_wide);
    return RR_OK;
}

int rr_preprocess_rows(const rr_frame* f, const rr_camera* cam, const rr_gaussians* g, int n_rows, int* radii,
                       void* splats, void* tiles, void* depth_keys, void* block_sums, void* block_wide, void* stream) {
    int rc = validate(f, cam, g, true);
    if (rc) return rc;
    if (f->flags & RR_FLAG_ANTIALIAS)
        return fail(RR_ERR_ARG, "RR_FLAG_ANTIALIAS: row blocks (the sharded step) are not supported yet");
    if (n_rows < f->P || (n_rows % 256) != 0) return fail(RR_ERR_ARG, "n_rows must be >= P and a multiple of 256");
    if (n_rows == 0) return RR_OK;
    if (!radii || !splats || !tiles || !depth_keys || !block_sums || !block_wide)
        return fail(RR_ERR_ARG, "null output array");
    if (f->flags & RR_FLAG_AUX_NORMAL) return fail(RR_ERR_ARG, "row blocks carry no aux normals");
    hipStream_t st = (hipStream_t)stream;
    PreArgs a = pre_args(f, cam, g);
    a.radii = radii;
    a.splats = static_cast<Splat*>(splats);
    a.tiles = static_cast<uint2*>(tiles);
    a.depth_keys = static_cast<uint32_t*>(depth_keys);
    a.block_sums = static_cast<uint2*>(block_sums);
    a.block_wide = static_cast<uint32_t*>(block_wide);
    a.n_out = n_rows;
    return stage(f, st, RR_STAGE_PREPROCESS, "preprocess (rows)", [&] { launch_preprocess(a, st); });
}

int rr_preprocess_rows_views(const rr_frame* f, const rr_view* views, int num_views, const rr_gaussians* g,
                             int n_rows, void* out, size_t view_stride, const size_t field_offsets[6], int wire,
                             void* stream) {
    if (!f || !views || !g || !field_offsets) return fail(RR_ERR_ARG, "null argument");
    if (f->flags & RR_FLAG_ANTIALIAS)
        return fail(RR_ERR_ARG, "RR_FLAG_ANTIALIAS: row blocks (the sharded step) are not supported yet");
    if (num_views < 1 || num_views > RR_MAX_VIEWS) return fail(RR_ERR_ARG, "1 <= num_views <= RR_MAX_VIEWS");
    if (n_rows < f->P || (n_rows % 256) != 0) return fail(RR_ERR_ARG, "n_rows must be >= P and a multiple of 256");
    if (f->flags & RR_FLAG_AUX_NORMAL) return fail(RR_ERR_ARG, "row blocks carry no aux normals");
    int rc = check_views(views, num_views);
    if (rc) return rc;
    // the frame's own validation, with view 0 standing in for the camera (the preprocess reads no
    // background)
    const rr_camera cam0{views[0].viewmatrix, views[0].viewmatrix, views[0].projmatrix, views[0].campos};
    rc = validate(f, &cam0, g, true);
    if (rc) return rc;
    if (n_rows == 0) return RR_OK;
    if (!out) return fail(RR_ERR_ARG, "null output buffer");
    PreArgs a = pre_args(f, &cam0, g);
    char* base = static_cast<char*>(out);
    a.radii = reinterpret_cast<int*>(base + field_offsets[0]);
    if (wire) {  // 10-float wire records, no depth keys (rr_unpack_rows rebuilds both)
        if ((field_offsets[1] | view_stride) & 7u) return fail(RR_ERR_ARG, "wire records need 8-B alignment");
        a.wire = reinterpret_cast<float*>(base + field_offsets[1]);
    } else {
        a.splats = reinterpret_cast<Splat*>(base + field_offsets[1]);
        a.depth_keys = reinterpret_cast<uint32_t*>(base + field_offsets[3]);
    }
    a.tiles = reinterpret_cast<uint2*>(base + field_offsets[2]);
    a.block_sums = reinterpret_cast<uint2*>(base + field_offsets[4]);
    a.block_wide = reinterpret_cast<uint32_t*>(base + field_offsets[5]);
    a.n_out = n_rows;
    PreViews vs{};
    vs.V = num_views;
    vs.stride = view_stride;
    for (int v = 0; v < num_views; v++) {
        const rr_view& w = views[v];
        vs.v[v] = PreView{w.viewmatrix, w.projmatrix, w.campos, w.tan_fovx, w.tan_fovy,
                          focal(w.width, w.tan_fovx), focal(w.height, w.tan_fovy), w.low_pass,
                          w.width, w.height, grid_x(w.width), grid_y(w.height)};
    }
    hipStream_t st = (hipStream_t)stream;
    return stage(f, st, RR_STAGE_PREPROCESS, "preprocess (rows, views)", [&] { launch_preprocess_views(a, vs, st); });
}

int rr_unpack_rows(int world, int rows_per_rank, const void* recv, size_t chunk_bytes, const size_t field_offsets[5],
                   void* geom_buffer, size_t geom_bytes, int* radii, void* stream) {
    if (world < 1 || rows_per_rank < 0 || (rows_per_rank % 256) != 0)
        return fail(RR_ERR_ARG, "world >= 1 and rows_per_rank a multiple of 256");
    if (!field_offsets) return fail(RR_ERR_ARG, "null field offsets");
    const int P = world * rows_per_rank;
    if (P == 0) return RR_OK;
    if (!recv || !geom_buffer || !radii) return fail(RR_ERR_ARG, "null buffer");
    if ((chunk_bytes | field_offsets[0] | field_offsets[1]) & 7u)
        return fail(RR_ERR_ARG, "chunks and wire / tile fields need 8-B alignment");
    const Geom gm = carve_geom(geom_buffer, P);
    if (geom_bytes < gm.total) return fail(RR_ERR_CAPACITY, "geometry buffer too small");
    hipStream_t st = (hipStream_t)stream;
    launch_unpack_rows(world, rows_per_rank, static_cast<const char*>(recv), chunk_bytes, field_offsets, gm.splats,
                       gm.tiles, gm.depth_keys, radii, gm.block_sums, gm.block_wide, st);
    return check(nullptr, st, "unpack rows");
}

int rr_forward_from_geometry(const rr_frame* f, const rr_camera* cam, const int* radii, void* geom_buffer,
                             size_t geom_bytes, void* image_buffer, size_t image_bytes, void* binning_buffer,
                             size_t binning_bytes, int* num_rendered, int* num_pairs, size_t* binning_needed,
                             float* out_color, float* out_depth, void* stream) {
    if (!f || !cam || !num_rendered || !num_pairs || !binning_needed) return fail(RR_ERR_ARG, "null argument");
    *num_rendered = 0;
    *num_pairs = 0;
    *binning_needed = 0;
    const int P = f->P, W = f->width, H = f->height;
    if (P < 0 || W <= 0 || H <= 0) return fail(RR_ERR_ARG, "bad P / width / height");
    if (f->flags & RR_FLAG_AUX_NORMAL) return fail(RR_ERR_ARG, "row blocks carry no aux normals");
    if (P == 0) return RR_OK;
    if (!radii || !geom_buffer || !image_buffer || !out_color || !out_depth || !cam->background)
        return fail(RR_ERR_ARG, "null buffer");
    const Geom gm = carve_geom(geom_buffer, P);
    const Img im = carve_img(image_buffer, W, H);
    if (geom_bytes < gm.total || image_bytes < im.total) return fail(RR_ERR_CAPACITY, "scratch buffer too small");
    if (int rc = count_pairs(f, gm, im, P, (hipStream_t)stream, num_rendered, num_pairs)) return rc;
    return finish_forward(f, cam, radii, geom_buffer, image_buffer, binning_buffer, binning_bytes, *num_pairs,
                          binning_needed, out_color, out_depth, stream);
}

int rr_forward_render_geometry(const rr_frame* f, const rr_camera* cam, const int* radii, void* geom_buffer,
                               void* image_buffer, void* binning_buffer, size_t binning_bytes, int num_pairs,
                               float* out_color, float* out_depth, void* stream) {
    if (!f || !cam || (f->flags & RR_FLAG_AUX_NORMAL)) return fail(RR_ERR_ARG, "bad frame / camera");
    if (f->P == 0) return RR_OK;
    if (!radii || !cam->background) return fail(RR_ERR_ARG, "null buffer");
    return render_frame(f, cam, radii, geom_buffer, image_buffer, binning_buffer, binning_bytes, num_pairs, out_color,
                        out_depth, nullptr, stream, DistFwdArgs{});
}

int rr_backward_records(const rr_frame* f, const rr_camera* cam, const int* radii, const void* geom_buffer,
                        const void* image_buffer, const void* binning_buffer, int num_rendered, const float* dL_dpix,
                        void* workspace, size_t workspace_bytes, int rows_per_rank, int chunk_rows, float* records,
                        void* stream) {
    if (!f || !cam) return fail(RR_ERR_ARG, "null frame / camera");
    if (f->flags & RR_FLAG_ABSGRAD)
        return fail(RR_ERR_ARG, "RR_FLAG_ABSGRAD: rr_backward_records (the sharded step) is not supported yet");
    const int P = f->P;
    if (P < 0) return fail(RR_ERR_ARG, "bad P");
    if (rows_per_rank < 0 || (rows_per_rank > 0 && (P % rows_per_rank != 0 || chunk_rows < 1)))
        return fail(RR_ERR_ARG, "rows_per_rank must divide P (and chunk_rows >= 1), or be 0");
    if (P == 0) return RR_OK;
    if (!radii || !geom_buffer || !image_buffer || !dL_dpix || !workspace || !records || !cam->background)
        return fail(RR_ERR_ARG, "null buffer");
    if (workspace_bytes < rr_backward_workspace_bytes(P)) return fail(RR_ERR_CAPACITY, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float* gacc = static_cast<float*>(workspace);
    if (int rc = blend_backward(f, cam, geom_buffer, image_buffer, binning_buffer, num_rendered, PixelGrads{dL_dpix},
                                kBlendBwdPlain, gacc, st))
        return rc;
    launch_pack_records(gacc, radii, P, rows_per_rank, rows_per_rank > 0 ? std::min(chunk_rows, rows_per_rank) : 1,
                        records, st);
    return check(f, st, "pack records");
}

int rr_gauss_backward_views(const rr_frame* f, const rr_view* views, int num_views, const rr_gaussians* g,
                            const float* records, int record_rows, float grad_scale, const rr_grads* out,
                            void* stream) {
    if (!f || !views || !g || !out) return fail(RR_ERR_ARG, "null argument");
    if (f->flags & RR_FLAG_ANTIALIAS)
        return fail(RR_ERR_ARG, "RR_FLAG_ANTIALIAS: the sharded backward is not supported yet");
    if (f->flags & RR_FLAG_ABSGRAD)
        return fail(RR_ERR_ARG, "RR_FLAG_ABSGRAD: rr_gauss_backward_views (the sharded step) is not supported yet");
    if (out->dL_dmeans2D_abs) return fail(RR_ERR_ARG, "rr_grads.dL_dmeans2D_abs needs RR_FLAG_ABSGRAD");
    if (num_views < 1 || num_views > RR_MAX_VIEWS) return fail(RR_ERR_ARG, "1 <= num_views <= RR_MAX_VIEWS");
    const int P = f->P;
    if (P < 0 || record_rows < P) return fail(RR_ERR_ARG, "bad P / record_rows");
    if (!(f->flags & RR_FLAG_RAW_PARAMS)) return fail(RR_ERR_ARG, "the sharded backward runs in raw-parameter mode");
    if (f->M < 1 || f->M > 16 || f->D < 0 || f->D > 3 || f->M < (f->D + 1) * (f->D + 1))
        return fail(RR_ERR_ARG, "sh_degree must be 0..3 and M >= (degree+1)^2, M <= 16");
    if (P == 0) return RR_OK;
    if (!records || !g->means3D || !g->shs || !g->opacities || !g->scales || !g->rotations || (f->M > 1 && !g->shs_rest))
        return fail(RR_ERR_ARG, "raw parameters and records are required");
    if (out->dL_dmeans2D || out->dL_dcolors || out->dL_dopacity || out->dL_dmeans3D || out->dL_dcov3D || out->dL_dsh ||
        out->dL_dscales || out->dL_drotations || out->dL_dsh_rest)
        return fail(RR_ERR_ARG, "the sharded backward writes no gradient arrays (Adam and statistics only)");
    if (out->grad_accum && (!out->denom || !out->max_radii2D))
        return fail(RR_ERR_ARG, "densification statistics need grad_accum, denom, max_radii2D");
    if (out->adam)  // a group without param is not stepped
        if (int rc = check_adam(f, g, out->adam, false)) return rc;
    if (int rc = check_views(views, num_views)) return rc;
    ViewCam cams[RR_MAX_VIEWS];
    for (int v = 0; v < num_views; v++) {
        const rr_view& w = views[v];
        cams[v] = ViewCam{w.viewmatrix, w.projmatrix, w.campos, w.tan_fovx, w.tan_fovy,
                          focal(w.width, w.tan_fovx), focal(w.height, w.tan_fovy), w.low_pass};
    }
    hipStream_t st = (hipStream_t)stream;
    const GaussBwdArgs a = gauss_bwd_args(f, g, out);
    {
        StageTimer tm(RR_STAGE_GAUSS_BWD, st);
        if (launch_gauss_bwd_views(a, cams, num_views, records, record_rows, grad_scale, st))
            return fail(RR_ERR_ARG, "bad number of views");
    }
    return check(f, st, "gaussian backward (views)");
}

// ---- tuning, statistics, debug views, the per-stage profile ----
const char* rr_last_error(void) { return g_err.c_str(); }
const char* rr_version(void) { return "rain_amd-raster 0.1 gfx950"; }

int rr_set_tuning(const char* key, int value) {
    if (!key) return fail(RR_ERR_ARG, "unknown tuning key: (null)");
    const std::string k(key);
    Tuning& tu = tuning();
    const Tuning dflt{};
    if (k == "early_den") tu.early_den = value > 0 ? (uint32_t)value : dflt.early_den;
    else if (k == "pair_scan_direct_blocks") tu.pair_scan_direct_blocks = value >= 0 ? value : dflt.pair_scan_direct_blocks;
    else if (k == "wide_bin_keys") tu.wide_bin_keys = value != 0;
    else if (k == "phase_b_gather") tu.b_gather = value != 0;
    else if (k == "dup_b_rows") tu.dup_b_rows = value != 0;
    else if (k == "dup_big_bins") tu.dup_big_bins = value >= 0 ? value : dflt.dup_big_bins;
    else if (k == "sx_bucket") tu.sx_bucket = value != 0;
    else if (k == "sx_lds_cap") tu.sx_lds_cap = value > 0 ? value : 0;
    else if (k == "sort_min_units") tu.sort_min_units = value > 0 ? value : dflt.sort_min_units;
    else if (k == "sort_min_units_tile") tu.sort_min_units_tile = value > 0 ? value : dflt.sort_min_units_tile;
    else if (k == "sort_max_rounds")
        tu.sort_max_rounds = (value == 1 || value == 2 || value == 4 || value == 8) ? value : dflt.sort_max_rounds;
    else return fail(RR_ERR_ARG, "unknown tuning key: " + k);
    return RR_OK;
}

int rr_set_binning_config(int split_denominator, int min_pairs) {
    if (split_denominator < 0 || min_pairs < 0) return fail(RR_ERR_ARG, "negative binning config");
    Tuning& tu = tuning();
    const Tuning dflt{};
    tu.early_den = split_denominator == 0 ? dflt.early_den : (uint32_t)split_denominator;
    tu.early_min = min_pairs == 0 ? dflt.early_min : (uint32_t)min_pairs;
    return RR_OK;
}

int rr_read_frame_stats(const rr_frame* f, const void* geom_buffer, const void* image_buffer, rr_frame_stats* out,
                        void* stream) {
    if (!f || !out) return fail(RR_ERR_ARG, "null");
    std::memset(out, 0, sizeof(*out));
    const int P = f->P, W = f->width, H = f->height;
    const int T = grid_x(W) * grid_y(H);
    out->tiles = T;
    if (P == 0) return RR_OK;
    const Geom gm = carve_geom(const_cast<void*>(geom_buffer), P);
    const Img im = carve_img(const_cast<void*>(image_buffer), W, H);
    hipStream_t st = (hipStream_t)stream;
    FrameTotals ft{};
    std::vector<uint32_t> tm(T);
    std::vector<uint2> per((size_t)P);
    RR_CHECK(hipMemcpyAsync(&ft, gm.ft, sizeof(ft), hipMemcpyDeviceToHost, st), "stats");
    RR_CHECK(hipMemcpyAsync(per.data(), gm.tiles, (size_t)P * sizeof(uint2), hipMemcpyDeviceToHost, st), "stats");
    RR_CHECK(hipMemcpyAsync(tm.data(), im.tile_max, (size_t)T * 4, hipMemcpyDeviceToHost, st), "stats");
    uint32_t cnt[4] = {0u, 0u, 0u, 0u};  // rr_layout.hpp Img::counters
    RR_CHECK(hipMemcpyAsync(cnt, im.counters, sizeof(cnt), hipMemcpyDeviceToHost, st), "stats");
    RR_CHECK(hipStreamSynchronize(st), "stats");
    int64_t vis = 0;
    for (const uint2& v : per) vis += v.y > 0;  // a Gaussian is visible iff its rect is non-empty (radii > 0)
    out->num_visible = vis;
    out->num_rendered = (int64_t)ft.rect;
    out->num_pairs = (int64_t)ft.L;
    int64_t s = 0;
    for (uint32_t v : tm) s += v;
    out->l_eff = s;
    // phase A's pairs, and the phase-B pairs kept for the tiles phase A left open (by the path the
    // frame took: its phase-B duplicate marks the gather path in counters[2])
    out->num_binned = (int64_t)ft.LA + (cnt[2] ? cnt[3] : cnt[0]);
    out->phase_b_pairs = (int64_t)ft.LB;
    out->phase_b_slots = (int64_t)cnt[0];
    return RR_OK;
}

int rr_debug_get_views(const rr_frame* f, const void* geom_buffer, const void* image_buffer,
                       const void* binning_buffer, int num_rendered, rr_debug_views* out) {
    if (!f || !out) return fail(RR_ERR_ARG, "null");
    const Geom gm = carve_geom(const_cast<void*>(geom_buffer), f->P);
    const Img im = carve_img(const_cast<void*>(image_buffer), f->width, f->height);
    const Bin bn = carve_bin(const_cast<void*>(binning_buffer), num_rendered, f->width, f->height);
    out->point_list = bn.point_list;
    out->ranges = reinterpret_cast<const uint32_t*>(im.ranges);
    out->tile_max = im.tile_max;
    out->final_T = im.final_T;
    out->n_contrib = im.n_contrib;
    out->splats = reinterpret_cast<const float*>(gm.splats);
    return RR_OK;
}

int rr_debug_set_fwd_trace(void* dev_buf) {
    set_fwd_trace(dev_buf);
    return RR_OK;
}

int rr_profile_enable(int enable) {
    g_prof = enable != 0;
    return RR_OK;
}

int rr_profile_select(unsigned stage_mask) {
    g_prof_mask = stage_mask;
    return RR_OK;
}

int rr_profile_collect(double* ms, int64_t* counts) {
    for (auto& r : g_recs) {
        RR_CHECK(hipEventSynchronize(r.b), "profile sync");
        float e = 0.f;
        RR_CHECK(hipEventElapsedTime(&e, r.a, r.b), "profile elapsed");
        if (ms) ms[r.stage] += e;
        if (counts) counts[r.stage] += 1;
        g_pool.push_back(r.a);
        g_pool.push_back(r.b);
    }
    g_recs.clear();
    return RR_OK;
}

const char* rr_stage_name(int stage) {
    static const char* names[RR_NUM_STAGES] = {"preprocess", "depth_sort", "scan", "duplicate", "tile_sort",
                                               "ranges", "blend_fwd", "blend_bwd", "gauss_bwd", "memset"};
    return (stage >= 0 && stage < RR_NUM_STAGES) ? names[stage] : "?";
}

}  // extern "C"
