// absgrad_plan_check.hip — host checker of plan_backward()'s third argument (rain_amd/csrc/rr_bwd_plan.hpp,
// RR_FLAG_ABSGRAD).
//
// A stand-alone program: for the presence patterns the API lets through with the flag (no aux map, no camera
// request) the blend plan must be kBlendBwdPlainAbs and the per-Gaussian plan the plain kernel; with the
// argument omitted or false every one of the 32 patterns, with and without a camera request, must plan what
// the two-argument call plans (tests/host/bwd_plan_check.hip holds those truth tables).  Opens no GPU and
// dereferences no map.  Built and run by tests/test_absgrad_abi_cpu.py.
#include <cstdio>

#include "rr_bwd_plan.hpp"

using namespace rr;

int main() {
    static_assert(kBlendBwdPlainAbs == 5, "BlendBwdMode values");
    static const float map[1] = {0.f};  // a present map (never read)
    int failed = 0, checks = 0;
    for (int bits = 0; bits < 32; bits++) {
        for (int cam = 0; cam < 2; cam++) {
            PixelGrads g{};
            g.dL_dpix = (bits & 1) ? map : nullptr;
            g.dL_ddepth = (bits & 2) ? map : nullptr;
            g.dL_dalpha = (bits & 4) ? map : nullptr;
            g.dL_dnormal = (bits & 8) ? map : nullptr;
            g.dL_dmoments = (bits & 16) ? map : nullptr;
            const BwdPlan two = plan_backward(g, cam != 0);
            const BwdPlan off = plan_backward(g, cam != 0, false);
            checks++;
            if (off.blend != two.blend || off.gauss != two.gauss) {
                failed++;
                std::printf("FAIL bits %d cam %d: absgrad = false changes the plan\n", bits, cam);
            }
            checks++;
            if (two.blend == kBlendBwdPlainAbs) {
                failed++;
                std::printf("FAIL bits %d cam %d: the abs variant planned without the flag\n", bits, cam);
            }
            if (cam || (bits & ~1)) continue;  // the flag with these is refused before the plan is asked
            const BwdPlan on = plan_backward(g, false, true);
            checks++;
            if (on.blend != kBlendBwdPlainAbs || on.gauss != kGaussBwdPlain) {
                failed++;
                std::printf("FAIL bits %d: absgrad plan is blend %d gauss %d\n", bits, (int)on.blend, (int)on.gauss);
            }
        }
    }
    std::printf("%d checks, %d failed\n", checks, failed);
    return failed ? 1 : 0;
}
