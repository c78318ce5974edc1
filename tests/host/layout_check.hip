// layout_check.hip — host checker of the rasterizer's scratch layout (rain_amd/csrc/rr_layout.hpp).
//
// A stand-alone program: carves the geometry, image and binning buffers over a stand-in base
// address for a sweep of sizes and tuning records and checks that every array is aligned, inside
// its buffer and disjoint from the others, that the image buffer's zeroed block is what the split
// scan clears, that point_list sits at offset 0 for every pair count (the backward's assumption),
// and that the bin sort's plans fit the arrays carved for them.  Touches no carved memory and opens
// no GPU.  Built and run by tests/test_layout_host.py.
#include <cstdio>
#include <string>
#include <vector>

#include "rr_layout.hpp"

namespace rr {
static Tuning g_tuning;  // the record under test
Tuning& tuning() { return g_tuning; }
}  // namespace rr

using namespace rr;

namespace {

constexpr uintptr_t kBase = 1u << 20;
int g_failed = 0;
long g_checks = 0;
std::string g_case;

void expect(bool ok, const char* what, const char* name = "") {
    g_checks++;
    if (ok) return;
    if (g_failed++ < 40) std::printf("FAIL [%s] %s %s\n", g_case.c_str(), name, what);
}

struct Arr {
    const char* name;
    uintptr_t at;
    size_t bytes, align;
};
template <typename T>
Arr arr(const char* name, const T* p, size_t n) {
    return Arr{name, reinterpret_cast<uintptr_t>(p), n * sizeof(T), alignof(T)};
}
Arr raw(const char* name, const void* p, size_t bytes, size_t align) {
    return Arr{name, reinterpret_cast<uintptr_t>(p), bytes, align};
}

// every array aligned for its type (and on `place` bytes), inside [lo, lo + extent), and in the
// given order without overlap
void check_arrays(const std::vector<Arr>& as, uintptr_t lo, size_t extent, size_t place) {
    uintptr_t end = lo;
    for (const Arr& a : as) {
        expect(a.at % a.align == 0, "misaligned for its element type", a.name);
        expect((a.at - lo) % place == 0, "not on its placement boundary", a.name);
        expect(a.at >= end, "overlaps the array before it (or is out of order)", a.name);
        expect(a.at + a.bytes <= lo + extent, "ends outside its buffer", a.name);
        end = a.at + a.bytes;
    }
}

void check_geom(int P) {
    g_case = "geom P=" + std::to_string(P);
    const Geom g = carve_geom(reinterpret_cast<void*>(kBase), P);
    const size_t n = P > 1 ? P : 1, nb = (n + 255) / 256;
    expect(g.total % 256 == 0, "total is no multiple of 256");
    expect(g.total == carve_geom(nullptr, P).total, "total depends on the base");
    expect(g.lists.nwin >= 64, "fewer than 64 marked windows");
    check_arrays({arr("splats", g.splats, n), arr("tiles", g.tiles, n), arr("depth_keys", g.depth_keys, n),
                  arr("idx_a", g.lists.idx_a, n), arr("off_a", g.lists.off_a, n), arr("idx_b", g.lists.idx_b, n),
                  arr("off_b", g.lists.off_b, n), arr("first_a", g.lists.first_a, g.lists.nwin),
                  arr("first_b", g.lists.first_b, g.lists.nwin), arr("normals", g.normals, n),
                  arr("block_sums", g.block_sums, nb), arr("block_wide", g.block_wide, nb), arr("ft", g.ft, 1),
                  raw("temp", g.temp, g.temp_bytes, 8)},
                 kBase, g.total, 256);
    expect(g.temp_bytes >= ((n + kPairScanItems - 1) / kPairScanItems) * kSplitScanTotalBytes, "temp too small");
}

size_t bins_of(int W, int H) {
    const size_t gx = ((size_t)W + 15) / 16, gy = ((size_t)H + 15) / 16;
    return ((gx + 1) / 2) * ((gy + 1) / 2);
}

void check_img(int W, int H) {
    g_case = "img " + std::to_string(W) + "x" + std::to_string(H);
    const Img m = carve_img(reinterpret_cast<void*>(kBase), W, H);
    const size_t N = (size_t)W * H, T = (((size_t)W + 15) / 16) * (((size_t)H + 15) / 16), NB = bins_of(W, H);
    expect(m.total % 256 == 0, "total is no multiple of 256");
    expect(m.total == carve_img(nullptr, W, H).total, "total depends on the base");
    check_arrays({arr("final_T", m.final_T, N), arr("n_contrib", m.n_contrib, N),
                  raw("zeroed block", m.ranges, m.zero_bytes, 16), arr("tile_max", m.tile_max, T),
                  arr("open", m.open, T), arr("order", m.order, T)},
                 kBase, m.total, 256);
    // the zeroed block: exactly these arrays, in this order, from ranges to ranges + zero_bytes
    const uintptr_t z = reinterpret_cast<uintptr_t>(m.ranges);
    check_arrays({arr("ranges", m.ranges, T), arr("ranges_b", m.ranges_b, T), arr("counters", m.counters, 4),
                  arr("open_bits", m.open_bits, (T + 31) / 32), arr("bounds_a", m.bounds_a, NB),
                  arr("bounds_b", m.bounds_b, NB), arr("bin_cnt", m.bin_cnt, 2 * NB),
                  arr("bin_cnt_a", m.bin_cnt_a, 2 * NB)},
                 z, m.zero_bytes, 4);
    expect(reinterpret_cast<uintptr_t>(m.bin_cnt_a + 2 * NB) == z + m.zero_bytes, "zero_bytes is not the block's extent");
    expect(m.zero_bytes % 4 == 0, "zero_bytes is no whole number of words");
}

template <typename K>
void check_bin_plans(const Bin& b, size_t first_n, size_t unit_len_n) {
    const uintptr_t temp = reinterpret_cast<uintptr_t>(b.temp);
    for (int early = 1; early >= 0; early--) {
        const PhaseHints h = phase_hints(b.L, early != 0);
        const RadixPlan pa = tile_plan<K>(b.temp, b.L, b.bits, h.a), pb = tile_plan<K>(b.temp, b.L, b.bits, h.b);
        expect((size_t)pa.units + (size_t)pb.units <= first_n, "the phases' windows do not fit first");
        expect((size_t)pb.units <= unit_len_n, "phase B's windows do not fit unit_len");
        if (b.L == 0) continue;
        for (int phase = 0; phase < 2; phase++) {
            const RadixPlan& p = phase ? pb : pa;
            const size_t hint = phase ? h.b : h.a;
            expect(p.units > 0 && (size_t)p.units * p.unit_items >= b.L, "the units do not cover L");
            expect(p.unit_items <= kSortMaxUnit, "unit longer than kSortMaxUnit");
            expect(sort_layout<K>(b.temp, b.L, b.bits, hint).total <= b.temp_bytes, "the sort's layout exceeds temp_bytes");
            const uintptr_t c = reinterpret_cast<uintptr_t>(p.counts);
            expect(c >= temp && c + ((size_t)4 << p.dbits0) * p.units <= temp + b.temp_bytes, "counts outside temp");
        }
    }
}

void check_bin(int L, int W, int H, const char* rec) {
    g_case = std::string("bin ") + rec + " L=" + std::to_string(L) + " " + std::to_string(W) + "x" + std::to_string(H);
    const Bin b = carve_bin(reinterpret_cast<void*>(kBase), L, W, H);
    const size_t n = L > 1 ? L : 1, np = 2 * n, kw = b.wide ? 4 : 2;
    expect(b.total % 256 == 0, "total is no multiple of 256");
    expect(b.total == carve_bin(nullptr, L, W, H).total, "total depends on the base");
    expect(reinterpret_cast<uintptr_t>(b.point_list) == kBase, "point_list is not at offset 0");
    expect(b.wide || bins_of(W, H) <= 65536, "16-bit keys for more than 65536 bins");
    expect(b.wide || !tuning().wide_bin_keys, "wide_bin_keys ignored");
    expect(((size_t)1 << b.bits) >= bins_of(W, H) && b.bits >= 1 && b.bits <= (int)(8 * kw), "bad key bits");
    // the arrays after `first` take what is left up to the next one: their use is checked below
    const size_t first_n = (reinterpret_cast<uintptr_t>(b.unit_len) - reinterpret_cast<uintptr_t>(b.first)) / 4;
    const size_t unit_len_n = (reinterpret_cast<uintptr_t>(b.temp) - reinterpret_cast<uintptr_t>(b.unit_len)) / 4;
    check_arrays({arr("point_list", b.point_list, 8 * n + kPointListPad), raw("keys", b.keys, np * kw, kw),
                  raw("keys_sorted", b.keys_sorted, np * kw, kw), arr("vals", b.vals, np),
                  arr("vals_sorted", b.vals_sorted, np), arr("first", b.first, 1), arr("unit_len", b.unit_len, 1),
                  raw("temp", b.temp, b.temp_bytes, 256)},
                 kBase, b.total, 256);
    const size_t key_span = reinterpret_cast<uintptr_t>(b.keys_sorted) - reinterpret_cast<uintptr_t>(b.keys);
    expect(key_span == align_up(np * kw), "the key arrays are not as wide as `wide` says");
    if (b.wide) check_bin_plans<uint32_t>(b, first_n, unit_len_n);
    else check_bin_plans<uint16_t>(b, first_n, unit_len_n);
}

}  // namespace

int main() {
    const int Ps[] = {0, 1, 255, 256, 257, 2047, 2048, 2049, 100000, 1048576, 5000000};
    const int WH[][2] = {{1, 1}, {16, 16}, {17, 33}, {64, 48}, {1920, 1080}, {3840, 2160}, {8208, 8208}};
    const int Ls[] = {0, 1, 2047, 2048, 2049, 65535, 65536, 3000000, (1 << 29) - 1};
    struct Rec {
        const char* name;
        Tuning t;
    };
    std::vector<Rec> recs(5);
    recs[0].name = "default";
    recs[1].name = "wide_bin_keys";
    recs[1].t.wide_bin_keys = true;
    recs[2].name = "units2048";
    recs[2].t.sort_min_units_tile = 1;
    recs[2].t.sort_max_rounds = 8;
    recs[3].name = "early_den=2";
    recs[3].t.early_den = 2;
    recs[4].name = "early_den=4";
    recs[4].t.early_den = 4;
    for (const Rec& r : recs) {
        g_tuning = r.t;
        for (int P : Ps) check_geom(P);
        for (const auto& wh : WH) {
            check_img(wh[0], wh[1]);
            for (int L : Ls) check_bin(L, wh[0], wh[1], r.name);
            g_case = std::string("b_gather ") + r.name;
            expect(b_gather(wh[0], wh[1]) == (bins_of(wh[0], wh[1]) <= (size_t)kBinScanMax), "b_gather disagrees with kBinScanMax");
        }
    }
    g_tuning = Tuning{};
    g_tuning.b_gather = false;
    expect(!b_gather(64, 48), "b_gather ignores Tuning::b_gather");
    std::printf("%ld checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
