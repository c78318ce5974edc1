// rr_contrib.hip — per-Gaussian blend-contribution statistics (include/rain_raster.h rr_contributions):
// for every Gaussian the sum, the weighted sum and the maximum over the frame's pixels of its blend
// weight w = alpha T, and the number of pixels it was blended into.
//
// The walk is the forward blend's, the mapping the blend backward's (rr_blend.hip): a 16x16 tile is
// one wave64, lane l owning column l % 16 of rows l / 16 + 4q, q < 4.
//   * Front to back over the tile's list (A-list ++ B-list), its first tile_max pairs; alpha is
//     recomputed with the forward's op sequence (blend_p2_x / blend_e2 / exp2 / min 0.99), a pixel
//     takes a pair when the forward blended it there (index < n_contrib, alpha >= 1/255, power <= 0),
//     and T runs from 1 with the forward's own update, so nothing depends on the phases' split.
//   * Rounds of 64 records (the a and b quarters of the 48-B splat record: the colour is not needed)
//     go global -> LDS directly, a round ahead, as in the blend backward.
//   * Per pair a lane holds three values over its 4 pixels (sum w, sum g w, max w).  Two pairs are
//     reduced across the wave together with permlane swaps and DPP row shifts (19 VALU per two
//     pairs, no LDS): the swaps leave {sum w, sum g w} of the two pairs in the four rows of one
//     register and the two maxima in rows 0 and 2 of another.  The hit count is the popcount of the
//     activity ballots (scalar unit).  A pair that no pixel takes skips the reduction.
//   * After each round one atomic per (pair, value), zeros skipped: float adds for the sums, an
//     unsigned max on the float's bits for max w (w >= 0), an unsigned add for the count.
#include "rr_contrib.hpp"

#include "rr_kernels.hpp"

namespace rr {

// Maxima of weights travel as their bit patterns: for floats >= 0 the unsigned order is the float
// order, and an unsigned max is one instruction (DPP-fused in the row steps) where fmaxf also
// canonicalises both operands.  Lanes without a DPP source read 0.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_umax(uint32_t v) {
    return max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ uint32_t row16_umax(uint32_t v) {  // lane 15 of each row: the row's maximum
    v = dpp_umax<0x111>(v);                                   // row_shr:1
    v = dpp_umax<0x112>(v);                                   // row_shr:2
    v = dpp_umax<0x114>(v);                                   // row_shr:4
    v = dpp_umax<0x118>(v);                                   // row_shr:8
    return v;
}
// swap32_add / swap16_add (rr_common.hpp) with max for +: the same named temporaries
__device__ __forceinline__ uint32_t swap32_umax(uint32_t a, uint32_t b) {
    unsigned ua = a, ub = b;
    const auto r = __builtin_amdgcn_permlane32_swap(ua, ub, false, false);
    ua = r[0];
    ub = r[1];
    return max(ua, ub);
}
__device__ __forceinline__ uint32_t swap16_umax(uint32_t a, uint32_t b) {
    unsigned ua = a, ub = b;
    const auto r = __builtin_amdgcn_permlane16_swap(ua, ub, false, false);
    ua = r[0];
    ub = r[1];
    return max(ua, ub);
}

constexpr int kContribVals = 4;  // sum_w, sum_gw, max_w, count

__global__ __launch_bounds__(64) void k_contrib(ContribArgs a) {
    constexpr int PPL = 4;
    constexpr int B = 64;
    const int ntiles = a.gx * a.gy;
    const int tile = xcd_tile(blockIdx.x, ntiles);
    const uint2 range = a.ranges[tile];
    const uint2 range_b = a.ranges_b[tile];
    const uint32_t na_len = range.y - range.x;  // list = A-list ++ B-list (early-stop binning)
    // pairs past tile_max were blended by no pixel (never more than the list holds)
    const int nmax = (int)min(a.tile_max[tile], na_len + (range_b.y - range_b.x));
    if (nmax == 0) return;
    const int tx = tile % a.gx, ty = tile / a.gx;
    const int t = threadIdx.x;
    const int lane = t;
    const int px = tx * TILE_X + (lane & 15);
    const int py0 = ty * TILE_Y + (lane >> 4);
    const float pfx = (float)px;

    __shared__ float4 s_a2[2][B];
    __shared__ float4 s_b2[2][B];
    __shared__ uint32_t s_id2[2][B];
    __shared__ uint32_t s_g[B * kContribVals];

    float T[PPL], gw[PPL];
    int last[PPL];
#pragma unroll
    for (int q = 0; q < PPL; q++) {
        const int py = py0 + 4 * q;
        const bool inside = px < a.W && py < a.H;
        const int pix = a.W * py + px;
        T[q] = 1.f;
        last[q] = inside ? (int)(a.n_contrib[pix] & ~kDoneBit) : 0;
        gw[q] = inside ? (a.pixel_weight ? a.pixel_weight[pix] : 1.f) : 0.f;
    }
    auto pair_at = [&](int idx) -> uint32_t {
        return (uint32_t)idx < na_len ? range.x + idx : range_b.x + ((uint32_t)idx - na_len);
    };
    // round r's records land in stage r & 1, issued (global -> LDS) one round ahead; record t at [t]
    auto glds_round = [&](int buf, uint32_t id) {
        typedef __attribute__((address_space(1))) const void* gp;
        typedef __attribute__((address_space(3))) void* lp;
        const float4* src = reinterpret_cast<const float4*>(a.splats) + 3 * (size_t)id;
        __builtin_amdgcn_global_load_lds((gp)(src + 0), (lp)&s_a2[buf][0], 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gp)(src + 1), (lp)&s_b2[buf][0], 16, 0, 0);
    };
    // ids: lanes past the list load record 0 (staged, never read); an id is never past the records
    const uint32_t idmax = (uint32_t)a.P - 1u;
    uint32_t cid = t < nmax ? min(a.point_list[pair_at(t)], idmax) : 0u;
    glds_round(0, cid);
    uint32_t nid = B + t < nmax ? min(a.point_list[pair_at(B + t)], idmax) : 0u;
    for (int base = 0, cur = 0; base < nmax; base += B, cur ^= 1) {
        float4* const s_a = s_a2[cur];
        float4* const s_b = s_b2[cur];
        uint32_t* const s_id = s_id2[cur];
        s_id[t] = cid;
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this round's records are in LDS
        __syncthreads();
        if (base + B < nmax) {  // block-uniform: the next round's records and the one after's ids
            glds_round(cur ^ 1, nid);
            cid = nid;
            const int k3 = base + 2 * B + t;
            nid = k3 < nmax ? min(a.point_list[pair_at(k3)], idmax) : 0u;
        }
        const int cnt = min(B, nmax - base);
        // one pair over the lane's pixels: its three values, and the wave's hit count (uniform)
        auto pair_w = [&](int j, float& sw, float& sgw, uint32_t& mw) -> uint32_t {
#pragma clang fp contract(off)
            const int contributor = base + j;
            const float4 A = s_a[j];
            const float4 Bv = s_b[j];
            const float dx = A.x - pfx;
            const P2X px2 = blend_p2_x(A.z, A.w, Bv.y, dx);  // identical to the forward's values
            float av[PPL];
            bool acv[PPL];
#pragma unroll
            for (int q = 0; q < PPL; q++) {
                const float dy = A.y - (float)(py0 + 4 * q);
                const float e2 = blend_e2(px2, Bv.x, dy);
                av[q] = fminf(0.99f, __builtin_amdgcn_exp2f(e2));
                acv[q] = contributor < last[q] && e2 <= Bv.y && av[q] >= 1.0f / 255.0f;
            }
            uint32_t hits = 0;
            sw = sgw = 0.f;
            mw = 0u;
#pragma unroll
            for (int q = 0; q < PPL; q++) {
                hits += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(acv[q]));
                if (acv[q]) {
                    const float w = av[q] * T[q];
                    T[q] = T[q] * (1.f - av[q]);  // the forward's update
                    sw += w;
                    sgw = __builtin_fmaf(gw[q], w, sgw);
                    mw = max(mw, __builtin_bit_cast(uint32_t, w));  // w > 0
                }
            }
            return hits;
        };
        for (int j = 0; j < cnt; j += 2) {
            float swa, sga, swb = 0.f, sgb = 0.f;
            uint32_t mwa, mwb = 0u;
            const uint32_t ha = pair_w(j, swa, sga, mwa);
            const bool has_b = j + 1 < cnt;  // block-uniform
            const uint32_t hb = has_b ? pair_w(j + 1, swb, sgb, mwb) : 0u;
            float t0 = 0.f;
            uint32_t t1 = 0u;
            if (ha + hb != 0u) {
                // rows: {sum w, sum g w} of pair j, then of pair j + 1; maxima in rows 0 and 2
                t0 = row16_sum(swap16_add(swap32_add(swa, swb), swap32_add(sga, sgb)));
                t1 = row16_umax(swap16_umax(swap32_umax(mwa, mwb), 0u));
            }
            if ((lane & 15) == 15) {
                const int row = lane >> 4, sel = row >> 1, odd = row & 1;
                if (sel == 0 || has_b) {
                    uint32_t* d = s_g + (j + sel) * kContribVals;
                    d[odd] = __builtin_bit_cast(uint32_t, t0);
                    if (!odd) {
                        d[2] = t1;
                        d[3] = sel ? hb : ha;
                    }
                }
            }
        }
        __syncthreads();
        // one atomic per (pair, value); consecutive lanes hit the four values of a pair's record
#pragma unroll
        for (int c = 0; c < kContribVals; c++) {
            const int e = c * B + t;
            const int pair = e / kContribVals, comp = e % kContribVals;
            if (pair < cnt) {
                const uint32_t v = s_g[e];
                uint32_t* o = a.out + (size_t)s_id[pair] * kContribVals + comp;
                if (comp < 2) {
                    const float f = __builtin_bit_cast(float, v);
                    if (f != 0.f) atomicAdd(reinterpret_cast<float*>(o), f);
                } else if (v != 0u) {
                    if (comp == 2) atomicMax(o, v);
                    else atomicAdd(o, v);
                }
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_contrib_clear(uint4* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = make_uint4(0u, 0u, 0u, 0u);
}

void launch_contrib_clear(uint32_t* out, int P, hipStream_t st) {
    if (P > 0) k_contrib_clear<<<(unsigned)((P + 255) / 256), 256, 0, st>>>(reinterpret_cast<uint4*>(out), (size_t)P);
}

void launch_contrib(const ContribArgs& a, hipStream_t st) {
    const int T = a.gx * a.gy;
    if (T > 0 && a.P > 0) k_contrib<<<T, 64, 0, st>>>(a);
}

}  // namespace rr
