// bwd_plan_check.hip — host checker of the backward's variant choice (rain_amd/csrc/rr_bwd_plan.hpp).
//
// A stand-alone program: walks all 32 presence patterns of the five output-gradient maps, with and
// without a camera request, and compares plan_backward() with the two truth tables written out below
// (transcribed from the if / else chains the function replaced, not recomputed).  Opens no GPU and
// dereferences no map.  Built and run by tests/test_bwd_plan_host.py.
#include <cstdio>

#include "rr_bwd_plan.hpp"

using namespace rr;

namespace {

// Index: bit 0 dL_dpix, bit 1 dL_ddepth, bit 2 dL_dalpha, bit 3 dL_dnormal, bit 4 dL_dmoments.
constexpr BlendBwdMode P = kBlendBwdPlain, D = kBlendBwdDepth, N = kBlendBwdNormal, M = kBlendBwdDist,
                       NM = kBlendBwdNormalDist;
constexpr BlendBwdMode kBlend[32] = {
    // no normal, no moments: (none) pix | depth, pix+depth | alpha, pix+alpha | depth+alpha, all three
    P, P, D, D, D, D, D, D,
    // normal
    N, N, N, N, N, N, N, N,
    // moments
    M, M, M, M, M, M, M, M,
    // normal + moments
    NM, NM, NM, NM, NM, NM, NM, NM,
};
constexpr GaussBwdMode GP = kGaussBwdPlain, GD = kGaussBwdDepth, GN = kGaussBwdNormal, GC = kGaussBwdCam;
constexpr GaussBwdMode kGauss[32] = {
    GP, GP, GD, GD, GD, GD, GD, GD,  // no normal, no moments
    GN, GN, GN, GN, GN, GN, GN, GN,  // normal
    GD, GD, GD, GD, GD, GD, GD, GD,  // moments (they ride slot 9: the depth kernel)
    GN, GN, GN, GN, GN, GN, GN, GN,  // normal + moments
};

}  // namespace

int main() {
    // the modes are template arguments and table indices: their values are part of the contract
    static_assert(kBlendBwdPlain == 0 && kBlendBwdDepth == 1 && kBlendBwdNormal == 2 && kBlendBwdDist == 3 &&
                      kBlendBwdNormalDist == 4, "BlendBwdMode values");
    static_assert(kGaussBwdPlain == 0 && kGaussBwdDepth == 1 && kGaussBwdNormal == 2 && kGaussBwdCam == 3,
                  "GaussBwdMode values");
    static const float map[1] = {0.f};  // a present map (never read)
    int failed = 0, checks = 0;
    for (int bits = 0; bits < 32; bits++) {
        for (int cam = 0; cam < 2; cam++) {
            if (cam && (bits & 24)) continue;  // refused before the plan is asked (a follow-up defines it)
            PixelGrads g{};
            g.dL_dpix = (bits & 1) ? map : nullptr;
            g.dL_ddepth = (bits & 2) ? map : nullptr;
            g.dL_dalpha = (bits & 4) ? map : nullptr;
            g.dL_dnormal = (bits & 8) ? map : nullptr;
            g.dL_dmoments = (bits & 16) ? map : nullptr;
            g.dist_near = 0.2f;
            g.dist_far = 100.f;
            const BwdPlan p = plan_backward(g, cam != 0);
            const GaussBwdMode want_gauss = cam ? GC : kGauss[bits];
            checks += 2;
            if (p.blend != kBlend[bits]) {
                failed++;
                std::printf("FAIL bits %d cam %d: blend mode %d, expected %d\n", bits, cam, (int)p.blend,
                            (int)kBlend[bits]);
            }
            if (p.gauss != want_gauss) {
                failed++;
                std::printf("FAIL bits %d cam %d: gauss mode %d, expected %d\n", bits, cam, (int)p.gauss,
                            (int)want_gauss);
            }
            // any() / aux() are what backward_impl's "null buffer" refusal reads
            checks += 2;
            if (g.any() != (bits != 0) || g.aux() != ((bits & ~1) != 0)) {
                failed++;
                std::printf("FAIL bits %d: any() / aux()\n", bits);
            }
        }
    }
    std::printf("%d checks, %d failed\n", checks, failed);
    return failed ? 1 : 0;
}
