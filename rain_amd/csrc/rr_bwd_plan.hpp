// rr_bwd_plan.hpp — which output gradients a backward call carries, and the kernel variants that
// follow from them.  Host-pure (standard headers only): tests/host/bwd_plan_check.hip includes it
// and walks every presence pattern.
#pragma once

namespace rr {

// The per-pixel output gradients of one backward call; a null map is absent (zero).
struct PixelGrads {
    const float* dL_dpix;      // [3,H,W] colour
    const float* dL_ddepth;    // [H*W] depth map D = sum alpha_i T_i z_i
    const float* dL_dalpha;    // [H*W] accumulated alpha A = 1 - T_final
    const float* dL_dnormal;   // [3,H,W] aux normal map
    const float* dL_dmoments;  // [2,H,W] depth-moment maps (dL/dM1, dL/dM2)
    float dist_near, dist_far; // the moments' depth mapping (read with dL_dmoments only)

    bool aux() const { return dL_ddepth || dL_dalpha || dL_dnormal || dL_dmoments; }
    bool any() const { return dL_dpix || aux(); }
};

// k_blend_bwd<MODE> (rr_blend.hip)
enum BlendBwdMode {
    kBlendBwdPlain = 0,
    kBlendBwdDepth = 1,
    kBlendBwdNormal = 2,
    kBlendBwdDist = 3,        // depth + moments
    kBlendBwdNormalDist = 4,  // depth + normal + moments
    kBlendBwdPlainAbs = 5,    // plain + the absolute mean2D sums (RR_FLAG_ABSGRAD; accumulator slots 13, 14)
};

// The per-Gaussian backward's kernel (rr_backward.hip): k_gauss_bwd, _depth (reads accumulator slot
// 9), _normal (slots 9 and 10..12), _cam (the depth kernel plus the camera partials).
enum GaussBwdMode {
    kGaussBwdPlain = 0,
    kGaussBwdDepth = 1,
    kGaussBwdNormal = 2,
    kGaussBwdCam = 3,
};

struct BwdPlan {
    BlendBwdMode blend;
    GaussBwdMode gauss;
};

// The one place that picks the variants.  dL_dpix changes neither; the moments ride slot 9, so they
// need no per-Gaussian variant beyond depth's.  (camera with dL_dnormal / dL_dmoments is refused
// before this is asked.)  absgrad (RR_FLAG_ABSGRAD): the plain blend becomes its abs variant; the flag
// with an aux map or camera gradients is refused before this is asked, so every other plan stands.
inline BwdPlan plan_backward(const PixelGrads& g, bool camera, bool absgrad = false) {
    BwdPlan p;
    if (g.dL_dmoments) p.blend = g.dL_dnormal ? kBlendBwdNormalDist : kBlendBwdDist;
    else if (g.dL_dnormal) p.blend = kBlendBwdNormal;
    else p.blend = g.aux() ? kBlendBwdDepth : kBlendBwdPlain;
    if (camera) p.gauss = kGaussBwdCam;
    else if (g.dL_dnormal) p.gauss = kGaussBwdNormal;
    else p.gauss = g.aux() ? kGaussBwdDepth : kGaussBwdPlain;
    if (absgrad && p.blend == kBlendBwdPlain) p.blend = kBlendBwdPlainAbs;
    return p;
}

}  // namespace rr
