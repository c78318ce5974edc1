// rr_sort_plan.hpp — host planning of the radix sort (rr_sort.hip): the unit geometry of a call,
// its scratch layout and the plan a producer kernel needs to emit the first pass's counts.  Host
// code only; from outside it needs rr::tuning() (rr_kernels.hpp).
#pragma once
#include <algorithm>

#include "rr_kernels.hpp"

namespace rr {

constexpr int kWaves = 4;       // waves per workgroup (unit) of the count kernel
constexpr int kMaxRounds = 16;  // rounds of 64 items per wave
static_assert(64 * kWaves * kMaxRounds == kSortMaxUnit, "rr_kernels.hpp kSortMaxUnit");

// passes of a sort of `bits` bits: 8-bit digits, or 9-bit ones for 25..27 bits (3 passes instead of
// 4; the tile sorts, whose first-pass counts come from the duplicate's 256-digit histogram, keep
// 8-bit digits)
__host__ __device__ constexpr int sort_passes(int bits) {
    return bits <= 0 ? 0 : (bits >= 25 && bits <= 27) ? 3 : (bits + 7) / 8;
}
__host__ __device__ constexpr int sort_max_dbits(int bits) {
    return bits <= 0 ? 0 : (bits + sort_passes(bits) - 1) / sort_passes(bits);
}

// rounds per wave: full 16 for large inputs, fewer for small ones so that there are >= ~min_units
// units (Tuning::sort_min_units, default 128; interleaved A/B on the bench step: with 8-bit digits
// 512 beat 1024 by 1.7%; with the 8-wave scatter (round 3) the 3-pass depth sort of 1M keys
// preferred its largest units: 128 (4096-item units) 0.086 vs 0.088 ms/step with 256 and 0.102
// with 512, profiles/r03_sort_units_ab.jsonl).  Sorts of <= 16-bit keys (the bin sorts) target
// more, smaller units (Tuning::sort_min_units_tile, default 1024): their first pass's units are the
// duplicate's windows, whose workgroups are latency-bound (duplicate 0.098 -> 0.092, bin sort 0.087
// -> 0.077 ms/step with 1024).  Tuning::sort_max_rounds caps the rounds (tests: 2048-item units).
inline int rounds_for(size_t n, int bits) {
    const Tuning& tu = tuning();
    const size_t mu = (size_t)(bits <= 16 ? tu.sort_min_units_tile : tu.sort_min_units);
    int r = std::min(tu.sort_max_rounds, kMaxRounds);
    while (r > 1 && (n + (size_t)64 * kWaves * r - 1) / ((size_t)64 * kWaves * r) < mu) r >>= 1;
    return r;
}

// Unit geometry of a sort and where its first-pass digit counts live, so that a producer kernel
// can emit counts[digit * units + unit] for the lowest dbits0 bits itself (then pass
// first_counts_ready = true to radix_sort_pairs).
struct RadixPlan {
    uint32_t* counts;
    int units, unit_items, rounds, dbits0;
};
// The unit geometry alone (rounds, unit_items, units): units of one workgroup x rounds x 64 items
// covering n.  n_hint (0: n): the size the unit length is chosen for, where n is only a capacity
// and the device holds the count (the binning's phases: sized by the frame's pair total, filled
// ~1/3 and ~2/3)
inline RadixPlan sort_units(size_t n, int bits, size_t n_hint) {
    RadixPlan u{};
    u.rounds = rounds_for(n_hint ? n_hint : n, bits);
    u.unit_items = 64 * kWaves * u.rounds;
    u.units = (int)((n + u.unit_items - 1) / u.unit_items);
    return u;
}

struct SortLayout {
    void* keys_alt;
    uint32_t* vals_alt;
    uint32_t* counts;
    uint32_t* offsets;
    uint32_t* totals;  // [512] per-digit totals of the current pass
    size_t total;
};
template <typename K>
SortLayout sort_layout(void* buf, size_t n, int bits, size_t n_hint) {
    auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
    SortLayout s{};
    const size_t units = (size_t)sort_units(n, bits, n_hint).units;
    const int dmax = sort_max_dbits(bits);
    const size_t nc = std::max<size_t>(((size_t)1 << dmax) * units, 1);
    char* p = static_cast<char*>(buf);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        void* r = p ? p + off : nullptr;
        off = al(off + std::max<size_t>(bytes, 1));
        return r;
    };
    s.keys_alt = take(n * sizeof(K));
    s.vals_alt = static_cast<uint32_t*>(take(n * 4));
    s.counts = static_cast<uint32_t*>(take(nc * 4));
    s.offsets = static_cast<uint32_t*>(take(nc * 4));
    s.totals = static_cast<uint32_t*>(take(512 * 4));
    s.total = off;
    return s;
}

template <typename K>
size_t radix_sort_temp_bytes(size_t n, int bits, size_t n_hint = 0) {
    return sort_layout<K>(nullptr, n, bits, n_hint).total;
}

template <typename K>
RadixPlan radix_sort_plan(void* temp, size_t n, int begin_bit, int end_bit, size_t n_hint = 0) {
    const int bits = end_bit - begin_bit;
    if (n == 0 || bits <= 0) return RadixPlan{};
    RadixPlan p = sort_units(n, bits, n_hint);
    p.dbits0 = sort_max_dbits(bits);
    p.counts = sort_layout<K>(temp, n, bits, n_hint).counts;
    return p;
}

}  // namespace rr
