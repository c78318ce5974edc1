// rr_layout.hpp — the rasterizer's three scratch buffers (geometry, image, binning): what each
// holds, where, and the host-side choices the layout depends on (bin key width, the phases' sort
// units, which path bins phase B).  Host code only; from outside it needs rr::tuning()
// (rr_kernels.hpp).  tests/host/layout_check.hip sweeps it on the CPU.
#pragma once
#include <algorithm>

#include "rr_common.hpp"
#include "rr_kernels.hpp"
#include "rr_sort_plan.hpp"

namespace rr {

constexpr size_t kAlign = 256;
inline size_t align_up(size_t x, size_t a = kAlign) { return (x + a - 1) & ~(a - 1); }

// Bump allocator over an opaque byte buffer (rasterizer_impl.h:10-16 `obtain`); a null base carves
// null pointers (size queries).
struct Carver {
    char* base;
    size_t align;
    size_t off = 0;
    explicit Carver(void* b, size_t a = kAlign) : base(static_cast<char*>(b)), align(a) {}
    template <typename T>
    T* take(size_t n) {
        off = align_up(off, align);
        T* p = reinterpret_cast<T*>(base ? base + off : nullptr);
        off += n * sizeof(T);
        return p;
    }
    // A carver over what comes next, packing its arrays on `a` bytes: take them from it, then take
    // its extent (off) from this one.
    Carver sub(size_t a) {
        off = align_up(off, align);
        return Carver(base ? base + off : nullptr, a);
    }
};

// n's bit length, at least 1: what the binary search of rasterizer_impl.cu:24-39 returns
inline uint32_t higher_msb(uint32_t n) { return 32u - (uint32_t)__builtin_clz(n | 1u); }

inline int grid_x(int W) { return (W + TILE_X - 1) / TILE_X; }
inline int grid_y(int H) { return (H + TILE_Y - 1) / TILE_Y; }
inline int frame_bins(int W, int H) { return bins_x(grid_x(W)) * bins_y(grid_y(H)); }

struct Geom {
    Splat* splats;
    uint2* tiles;         // per Gaussian {pairs emitted, bounding-rect tiles}
    uint32_t* depth_keys;
    PhaseLists lists;     // the early-stop phases' Gaussians in index order with their pair offsets
    float4* normals;      // RR_FLAG_AUX_NORMAL: view-space normal per visible Gaussian
    uint2* block_sums;    // [ceil(P/256)] per-preprocess-block sums of tiles[] (pairs, rect tiles)
    uint32_t* block_wide; // [ceil(P/256)] per block: a visible depth key needs more than kDepthKeyBits
    FrameTotals* ft;      // the frame's counts and early-stop depth cut (rr_bin.hip)
    void* temp;           // the pair scan's block totals
    size_t temp_bytes;
    size_t total;
};
inline Geom carve_geom(void* buf, int P) {
    Carver c(buf);
    Geom g;
    const size_t n = (size_t)std::max(P, 1);
    g.splats = c.take<Splat>(n);
    g.tiles = c.take<uint2>(n);
    g.depth_keys = c.take<uint32_t>(n);
    g.lists.idx_a = c.take<uint32_t>(n);
    g.lists.off_a = c.take<uint32_t>(n);
    g.lists.idx_b = c.take<uint32_t>(n);
    g.lists.off_b = c.take<uint32_t>(n);
    // window starts for up to 2048 * P / 16 pairs per phase (more: a window-starts launch)
    g.lists.nwin = (uint32_t)std::min<size_t>(std::max<size_t>(n / 16, 64), (1u << 29) / kSplitWin + 1);
    g.lists.first_a = c.take<uint32_t>(g.lists.nwin);
    g.lists.first_b = c.take<uint32_t>(g.lists.nwin);
    g.normals = c.take<float4>(n);
    g.block_sums = c.take<uint2>((n + 255) / 256);
    g.block_wide = c.take<uint32_t>((n + 255) / 256);
    g.ft = c.take<FrameTotals>(1);
    g.temp_bytes = split_scan_temp_bytes(P);
    g.temp = c.take<char>(std::max<size_t>(g.temp_bytes, 1));
    g.total = align_up(c.off);
    return g;
}

struct Img {
    float* final_T;
    uint32_t* n_contrib;
    // one block, [ranges, ranges + zero_bytes), cleared before every render (by the split scan's
    // first launch): its arrays packed on 8 B in this order
    uint2* ranges;        // [T] phase-A (or single-phase) lists
    uint2* ranges_b;      // [T] phase-B lists of early-stop binning (all {0,0} otherwise)
    uint32_t* counters;   // [4]: [0] phase-B pairs (gather path: slots reserved), [1] backward tile order
                          // done, [2] phase B took the gather path, [3] phase-B pairs its bin runs hold
    uint32_t* open_bits;  // [ceil(T/32)] open as a bitmask (the phase-A blend sets it)
    uint2* bounds_a;      // [bins] phase A's (or the single phase's) bin runs (k_bin_bounds)
    uint2* bounds_b;      // [bins] phase B's
    uint32_t* bin_cnt;    // [2 bins] phase B's pair count per bin (the gather path), then its fill
    uint32_t* bin_cnt_a;  // [2 bins] phase A's
    size_t zero_bytes;
    uint32_t* tile_max;
    uint8_t* open;        // [T] tile still open after phase A
    uint32_t* order;      // [T] backward blend dispatch order (heaviest tiles first)
    size_t total;
};
inline Img carve_img(void* buf, int W, int H) {
    Carver c(buf);
    Img m;
    const size_t N = (size_t)std::max(W * H, 1);
    const size_t T = (size_t)std::max(grid_x(W) * grid_y(H), 1);
    const size_t NB = (size_t)std::max(frame_bins(W, H), 1);
    m.final_T = c.take<float>(N);
    m.n_contrib = c.take<uint32_t>(N);
    Carver z = c.sub(sizeof(uint2));
    m.ranges = z.take<uint2>(T);
    m.ranges_b = z.take<uint2>(T);
    m.counters = z.take<uint32_t>(4);
    m.open_bits = z.take<uint32_t>((T + 31) / 32);
    m.bounds_a = z.take<uint2>(NB);
    m.bounds_b = z.take<uint2>(NB);
    m.bin_cnt = z.take<uint32_t>(2 * NB);
    m.bin_cnt_a = z.take<uint32_t>(2 * NB);
    m.zero_bytes = z.off;
    c.take<char>(z.off);
    m.tile_max = c.take<uint32_t>(T);
    m.open = c.take<uint8_t>(T);
    m.order = c.take<uint32_t>(T);
    m.total = align_up(c.off);
    return m;
}

// Early-stop binning split (rr_bin.hip depth_cut): phase A bins the pairs of the Gaussians nearer
// than a per-frame depth cut holding ~1/den of the pairs, for every tile; phase B the rest, only for
// the tiles phase A left open (rr_kernels.hpp BlendPhase).  den = 3: on the bench frames (1M
// Gaussians, 1080p) most tiles saturate inside the first third (tools/saturation_stats.py; with the
// depth-rank split of rounds 1-3, tools/step_ab.py --split 2,3,4: 1.509 / 1.491 / 1.525 ms per
// step).  Frames below Tuning::early_min pairs are binned in one phase.  rr_set_binning_config
// changes both (tests force the split onto small frames).
//
// Binning paths: phase A (or the single phase) by the windowed duplicate over the split scan's
// index-ordered list + the stable bin sort; phase B by the gather path (rr_forward.hip k_dup_gather,
// per-bin count / scatter: few pairs) when the grid's bins fit one workgroup's count (kBinScanMax),
// else by the windowed path (Tuning::b_gather off forces it onto small frames).
inline bool b_gather(int W, int H) { return tuning().b_gather && frame_bins(W, H) <= kBinScanMax; }

// Window (= sort unit) length of each phase's sort, chosen for the pairs it is expected to hold
// (the split scan's depth cut aims phase A at ~1/den of the pairs) while its windows cover the
// capacity L.
struct PhaseHints {
    size_t a, b;
};
inline PhaseHints phase_hints(uint32_t L, bool early) {
    const size_t n = std::max<size_t>(L, 1);
    const size_t a = std::max<size_t>(n / std::max<uint32_t>(tuning().early_den, 1u), 1);
    return early ? PhaseHints{a, std::max<size_t>(n - a, 1)} : PhaseHints{n, n};
}
template <typename K>
RadixPlan tile_plan(void* temp, uint32_t n, int bits, size_t hint) {
    return radix_sort_plan<K>(temp, (size_t)n, 0, bits, hint);
}

struct Bin {
    // FIRST, so the backward finds it without knowing the pair count: the per-tile lists
    // k_sortexpand writes, 4 slots per (bin, Gaussian) pair.  The host knows only the frame's
    // total L (the phases' split LA + LB = L stays on the device).  Every pair array has a phase-A
    // region [0, L) and a phase-B region [L, 2L) (point_list: [0, 4L) and [4L, 8L)), plus the bin
    // sort's arrays — 56 B per pair with 16-bit bin keys (point_list 32, keys 4 + 4 sorted, values
    // 8 + 8 sorted) + ~0.5 B of sort counts.
    // Bins of more than 2048 pairs are depth-sorted inside their own point_list region (rr_bin.hip
    // sortexpand_run): no scratch arrays.
    uint32_t* point_list;
    void* keys;            // bin ids of the (bin, Gaussian) pairs
    void* keys_sorted;
    uint32_t* vals;        // Gaussian | tile mask << BIN_SHIFT, then sorted
    uint32_t* vals_sorted;
    uint32_t* first;       // first Gaussian of every duplicate window (= sort unit), phase A then B
    uint32_t* unit_len;    // phase B: pairs kept per window
    void* temp;            // bin-sort scratch, shared by the two phases
    size_t temp_bytes;
    bool wide;  // 32-bit bin keys (more than 65536 bins)
    int bits;
    uint32_t L;  // (bin, Gaussian) pairs of both phases
    size_t total;
};
// What follows point_list, for bin keys of type K.  The layout depends on the frame's pair count L
// only, sized for the early-stop split (its phase-A hint has the most windows; a single-phase
// frame uses fewer).
template <typename K>
void carve_bin_arrays(Carver& c, Bin& b, size_t np) {
    b.keys = c.take<K>(np);
    b.keys_sorted = c.take<K>(np);
    b.vals = c.take<uint32_t>(np);
    b.vals_sorted = c.take<uint32_t>(np);
    const PhaseHints h = phase_hints(b.L, true);
    const int ua = std::max(tile_plan<K>(nullptr, b.L, b.bits, h.a).units, 1);
    const int ub = std::max(tile_plan<K>(nullptr, b.L, b.bits, h.b).units, 1);
    b.first = c.take<uint32_t>((size_t)ua + ub + 2);
    b.unit_len = c.take<uint32_t>((size_t)ub + 1);
    b.temp_bytes = b.L == 0 ? 0 : std::max(radix_sort_temp_bytes<K>(b.L, b.bits, h.a),
                                           radix_sort_temp_bytes<K>(b.L, b.bits, h.b));
    b.temp = c.take<char>(std::max<size_t>(b.temp_bytes, 1));
}
inline Bin carve_bin(void* buf, int L, int W, int H) {
    Carver c(buf);
    Bin b;
    const int NB = frame_bins(W, H);
    b.wide = NB > 65536 || tuning().wide_bin_keys;
    b.bits = std::max(1, (int)higher_msb((uint32_t)NB));  // >= 1: the duplicate windows are sort units
    b.L = (uint32_t)std::max(L, 0);
    const size_t np = 2 * (size_t)std::max(L, 1);  // entries of each pair array: both phases' regions
    b.point_list = c.take<uint32_t>(4 * np + kPointListPad);
    if (b.wide) carve_bin_arrays<uint32_t>(c, b, np);
    else carve_bin_arrays<uint16_t>(c, b, np);
    b.total = align_up(c.off);
    return b;
}

}  // namespace rr
