// mcmc.hip — MCMC densification (include/rain_train.h rt_mcmc_*; "3D Gaussian Splatting as Markov
// Chain Monte Carlo", Kheradmand et al., NeurIPS 2024).
//
//   rt_mcmc_relocate  rare (one densification event): dead Gaussians become copies of live ones, in
//                     place, with the paper's closed-form opacity / scale correction in double.
//                       k_reloc_count    per pair: integer atomic count of every source's draws
//                       k_reloc_pairs    one wave per pair: row dst[j] <- row src[j] (old values),
//                                        corrected opacity / scaling, zero moments
//                       k_reloc_sources  per row with a count: its own corrected opacity / scaling,
//                                        zero moments in every group
//                     Race-free because no row is both a source and a destination and the
//                     destinations are distinct: the pair pass only reads source rows and writes
//                     each destination row from one wave; the source pass, a later launch on the
//                     same stream, writes source rows only, each from one thread.
//   rt_mcmc_step      every iteration: L1 opacity / scale regulariser + Adam + covariance-shaped
//                     position noise for xyz, opacity, scaling and rotation in ONE pass.
//
// Layout of the step kernel.  A workgroup owns a tile of kTileRows consecutive Gaussians.  In every
// group the tile is one contiguous, 16-B aligned run of floats, so the Adam part streams it in
// rt_adam_step's flat, lane-consecutive float4 order (Adam and both regulariser terms are
// elementwise) — the order that measured 1.8-4x faster than a row-per-lane order on this chip
// (tools/probe_rowwise_adam.hip).  Only the noise couples a row's parameters: the updated opacity,
// scaling and rotation of the tile are left in LDS on their way out (32 KB), one thread per row
// turns them into the row's displacement Sigma (noise gate scale), written over the row's scaling
// slots, and the xyz group's flat pass adds it after its own Adam update.  Traffic per row: the 77
// floats of an Adam step over these groups plus the 3 normals.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/rain_train.h"
#include "adam_math.hpp"

namespace rt_internal {
void set_error(const std::string& m);  // train.hip: the message rt_last_error() returns
}

namespace {

int fail(const std::string& m, int code = 1) {
    rt_internal::set_error(m);
    return code;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---------------------------------------------------------------------------------------------
// relocation
// ---------------------------------------------------------------------------------------------

struct RelocGroup {
    float* p;
    float* m;
    float* v;
    int width;
    int kind;
};
struct RelocArgs {
    RelocGroup grp[RT_MAX_GROUPS];
    int n_groups;
    int P;
    int n;
    const int64_t* src;
    const int64_t* dst;
    uint32_t* counts;
    const float* opacity;  // the OPACITY group's parameter
    float min_opacity;
};

static_assert(sizeof(rt_mcmc_group) == 32, "rt_mcmc_group layout (rain_amd/_native.py RTMcmcGroup)");
static_assert(sizeof(rt_mcmc_step_group) == 48, "rt_mcmc_step_group layout (rain_amd/_native.py RTMcmcStepGroup)");
static_assert(sizeof(rt_mcmc_step_args) == 272, "rt_mcmc_step_args layout (rain_amd/_native.py RTMcmcStepArgs)");

// The corrected raw opacity and log(coeff) of a source drawn `count` times (rain_train.h), in double.
// D's double sum is summed over a first: sum_{a=k+1..N} C(a-1, k) = C(N, k+1), so
//   D = sum_{k=0..N-1} C(N, k+1) (-1)^k o'^(k+1) / sqrt(k+1)
// with the same terms.  The binomials are exact in double (C(51, 25) * 26 < 2^53).
__device__ void reloc_values(float raw_opacity, uint32_t count, float min_opacity, float& new_raw_opacity,
                             double& log_coeff) {
    const int N = (int)min(count, (uint32_t)(RT_MCMC_N_MAX - 1)) + 1;
    const double x = (double)raw_opacity;
    const double o = 1.0 / (1.0 + exp(-x));
    const double q = 1.0 / (1.0 + exp(x));  // 1 - o, without the cancellation
    double on = o, coeff = 1.0;
    if (N > 1) {
        on = -expm1(log(q) / (double)N);  // 1 - (1 - o)^(1/N)
        double D = 0.0, binom = (double)N, pw = on, sign = 1.0;
        for (int k = 0; k < N; k++) {
            D += sign * binom * pw / sqrt((double)(k + 1));
            binom = binom * (double)(N - k - 1) / (double)(k + 2);
            pw *= on;
            sign = -sign;
        }
        coeff = o / D;
    }
    const double xc = fmin(fmax(on, (double)min_opacity), 1.0 - (double)FLT_EPSILON);
    new_raw_opacity = (float)log(xc / (1.0 - xc));
    log_coeff = log(coeff);
}

__device__ __forceinline__ bool in_rows(int64_t i, int P) { return i >= 0 && i < (int64_t)P; }

__global__ __launch_bounds__(256) void k_reloc_count(RelocArgs a) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.n) return;
    const int64_t s = a.src[j], d = a.dst[j];
    if (!in_rows(s, a.P) || !in_rows(d, a.P)) return;  // the pair is skipped everywhere
    atomicAdd(a.counts + s, 1u);
}

__global__ __launch_bounds__(64) void k_reloc_pairs(RelocArgs a) {
    const int j = blockIdx.x;
    const int64_t s = a.src[j], d = a.dst[j];
    if (!in_rows(s, a.P) || !in_rows(d, a.P)) return;
    float new_op;
    double log_coeff;
    reloc_values(a.opacity[s], a.counts[s], a.min_opacity, new_op, log_coeff);
    for (int gi = 0; gi < a.n_groups; gi++) {
        const RelocGroup& G = a.grp[gi];
        for (int col = threadIdx.x; col < G.width; col += 64) {
            float val = G.p[s * G.width + col];
            if (G.kind == RT_GROUP_OPACITY) val = new_op;
            if (G.kind == RT_GROUP_SCALING) val = (float)((double)val + log_coeff);
            const int64_t e = d * G.width + col;
            G.p[e] = val;
            if (G.m) {
                G.m[e] = 0.f;
                G.v[e] = 0.f;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_reloc_sources(RelocArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.P) return;
    const uint32_t c = a.counts[i];
    if (c == 0) return;
    float new_op;
    double log_coeff;
    reloc_values(a.opacity[i], c, a.min_opacity, new_op, log_coeff);
    for (int gi = 0; gi < a.n_groups; gi++) {
        const RelocGroup& G = a.grp[gi];
        for (int col = 0; col < G.width; col++) {
            const int64_t e = (int64_t)i * G.width + col;
            if (G.kind == RT_GROUP_OPACITY) G.p[e] = new_op;
            if (G.kind == RT_GROUP_SCALING) G.p[e] = (float)((double)G.p[e] + log_coeff);
            if (G.m) {
                G.m[e] = 0.f;
                G.v[e] = 0.f;
            }
        }
    }
}

constexpr size_t kWsAlign = 256;
size_t reloc_workspace_bytes(int P) {
    const size_t n = (size_t)(P > 0 ? P : 1) * sizeof(uint32_t);
    return (n + kWsAlign - 1) & ~(kWsAlign - 1);
}

// ---------------------------------------------------------------------------------------------
// step
// ---------------------------------------------------------------------------------------------

// Non-temporal loads and stores, like rt_adam_step's: every element is read once and written once
// per step.  A/B (tools/build_variant.py --lib librain_train.so -DRT_MCMC_NT_STORES=0 [-DRT_MCMC_NT_LOADS=0],
// tools/mcmc_cost.py --variant, 1M rows, profiles/mcmc_step_bench.json): with the caches swept between
// calls, as a frame sweeps them between two training steps, 64.2 us against 69.9 with plain stores
// and 82.8 with plain loads too; only called back to back, where a third of the arrays stays in the
// Infinity Cache, the plain accesses win (49.3 against 55.1 us).  128-thread workgroups: no difference.
#ifndef RT_MCMC_NT_LOADS
#define RT_MCMC_NT_LOADS 1
#endif
#ifndef RT_MCMC_NT_STORES
#define RT_MCMC_NT_STORES 1
#endif

constexpr int kThreads = 256;
constexpr int kRowsPerThread = 4;
constexpr int kTileRows = kThreads * kRowsPerThread;

enum { kXyz = 0, kOpacity = 1, kScaling = 2, kRotation = 3 };

struct StepGroup {
    float* p;
    const float* g;
    float* m;
    float* v;
    double lr;
    float bc1, bc2s;
    int vec;  // every array of the group that the launch touches is 16-B aligned
};
struct StepArgs {
    int P;
    StepGroup grp[4];  // indexed by kXyz ..
    double beta1, beta2, eps;
    float reg_opacity;  // (float)(lambda_o / P), 0: off
    float reg_scaling;  // (float)(lambda_s / (3 P)), 0: off
    const float* noise;
    float noise_scale;
    float gate_k, gate_x0;
};

typedef float v4f __attribute__((ext_vector_type(4)));

// one float4 slot of a tile: vector access when the group is aligned and the slot is whole, else
// the elements below n one by one (the ragged end of the last tile, unaligned arrays)
__device__ __forceinline__ float4 ld_slot(const float* base, int e, int n, bool vec) {
    if (vec && e + 4 <= n) {
#if RT_MCMC_NT_LOADS
        const v4f t = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(base + e));
#else
        const v4f t = *reinterpret_cast<const v4f*>(base + e);
#endif
        return make_float4(t.x, t.y, t.z, t.w);
    }
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < n) r.x = base[e];
    if (e + 1 < n) r.y = base[e + 1];
    if (e + 2 < n) r.z = base[e + 2];
    if (e + 3 < n) r.w = base[e + 3];
    return r;
}
__device__ __forceinline__ void st_slot(float* base, int e, int n, bool vec, float4 r) {
    if (vec && e + 4 <= n) {
        const v4f t = {r.x, r.y, r.z, r.w};
#if RT_MCMC_NT_STORES
        __builtin_nontemporal_store(t, reinterpret_cast<v4f*>(base + e));
#else
        *reinterpret_cast<v4f*>(base + e) = t;
#endif
        return;
    }
    if (e < n) base[e] = r.x;
    if (e + 1 < n) base[e + 1] = r.y;
    if (e + 2 < n) base[e + 2] = r.z;
    if (e + 3 < n) base[e + 3] = r.w;
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// the regulariser's gradient at parameter value p (before the update), added to g
template <int KIND>
__device__ __forceinline__ float reg_grad(float g, float p, float w) {
    if (KIND == kOpacity) {
        const float s = sigmoidf(p);
        return g + w * (s * (1.0f - s));
    }
    return g + w * expf(p);
}

// One group's part of the tile: W floats per row, i.e. W float4 slots per thread, all loaded before
// the first is stored.  ADAM: the Adam update, with the regulariser's gradient when reg != 0.
// `lds`: the (updated) values go there as well (opacity / scaling / rotation under noise), or, for
// xyz, hold the displacement that is added after the update.
template <int W, int KIND, bool ADAM, bool NOISE>
__device__ __forceinline__ void group_pass(const StepArgs& a, int row0, int rows, float* lds) {
    const StepGroup& G = a.grp[KIND];
    const int64_t base = (int64_t)row0 * W;
    const int n = rows * W;
    const bool vec = G.vec != 0;
    float4 p[W], g[W], m[W], v[W];
#pragma unroll
    for (int k = 0; k < W; k++) {
        const int e = 4 * ((int)threadIdx.x + kThreads * k);
        p[k] = ld_slot(G.p + base, e, n, vec);
        if (ADAM) {
            g[k] = ld_slot(G.g + base, e, n, vec);
            m[k] = ld_slot(G.m + base, e, n, vec);
            v[k] = ld_slot(G.v + base, e, n, vec);
        }
    }
    const float reg = KIND == kOpacity ? a.reg_opacity : KIND == kScaling ? a.reg_scaling : 0.f;
    AdamC c;
    if (ADAM) c = adam_consts(G.lr, G.bc1, G.bc2s, a.beta1, a.beta2, a.eps);
#pragma unroll
    for (int k = 0; k < W; k++) {
        const int e = 4 * ((int)threadIdx.x + kThreads * k);
        if (ADAM) {
            if ((KIND == kOpacity || KIND == kScaling) && reg != 0.f) {
                g[k].x = reg_grad<KIND>(g[k].x, p[k].x, reg);
                g[k].y = reg_grad<KIND>(g[k].y, p[k].y, reg);
                g[k].z = reg_grad<KIND>(g[k].z, p[k].z, reg);
                g[k].w = reg_grad<KIND>(g[k].w, p[k].w, reg);
            }
            adam_elem(p[k].x, g[k].x, m[k].x, v[k].x, c);
            adam_elem(p[k].y, g[k].y, m[k].y, v[k].y, c);
            adam_elem(p[k].z, g[k].z, m[k].z, v[k].z, c);
            adam_elem(p[k].w, g[k].w, m[k].w, v[k].w, c);
        }
        if (NOISE && e < n) {
            float4* slot = reinterpret_cast<float4*>(lds + e);  // (elements past n: the tile's padding)
            if (KIND == kXyz) {
                const float4 d = *slot;
                p[k].x += d.x;
                p[k].y += d.y;
                p[k].z += d.z;
                p[k].w += d.w;
            } else {
                *slot = p[k];
            }
        }
        if (ADAM || KIND == kXyz) st_slot(G.p + base, e, n, vec, p[k]);
        if (ADAM) {
            st_slot(G.m + base, e, n, vec, m[k]);
            st_slot(G.v + base, e, n, vec, v[k]);
        }
    }
}

template <bool ADAM, bool NOISE>
__global__ __launch_bounds__(kThreads) void k_mcmc_step(StepArgs a) {
    __shared__ __attribute__((aligned(16))) float s_op[NOISE ? kTileRows : 4];
    __shared__ __attribute__((aligned(16))) float s_sc[NOISE ? 3 * kTileRows : 4];
    __shared__ __attribute__((aligned(16))) float s_rot[NOISE ? 4 * kTileRows : 4];
    const int row0 = (int)blockIdx.x * kTileRows;
    const int rows = min(kTileRows, a.P - row0);
    group_pass<1, kOpacity, ADAM, NOISE>(a, row0, rows, s_op);
    group_pass<3, kScaling, ADAM, NOISE>(a, row0, rows, s_sc);
    group_pass<4, kRotation, ADAM, NOISE>(a, row0, rows, s_rot);
    if (NOISE) {
        __syncthreads();
        // per row: d = Sigma (z gate noise_scale), Sigma = R diag(s^2) R^T, left in the row's scaling slots
#pragma unroll
        for (int j = 0; j < kRowsPerThread; j++) {
            const int r = (int)threadIdx.x + kThreads * j;
            if (r >= rows) break;
            const float o = sigmoidf(s_op[r]);
            // exp overflows to +inf for o - x0 > ~0.89 at k = 100: the gate is then exactly 0
            const float gate = 1.0f / (1.0f + expf(a.gate_k * (o - a.gate_x0)));
            const float f = gate * a.noise_scale;
            const float* z = a.noise + 3 * ((int64_t)row0 + r);
            const float z0 = z[0] * f, z1 = z[1] * f, z2 = z[2] * f;
            const float4 q4 = *reinterpret_cast<const float4*>(s_rot + 4 * r);
            const float inv = 1.0f / sqrtf(q4.x * q4.x + q4.y * q4.y + q4.z * q4.z + q4.w * q4.w);
            const float w = q4.x * inv, x = q4.y * inv, y = q4.z * inv, zz = q4.w * inv;
            const float r00 = 1.f - 2.f * (y * y + zz * zz), r01 = 2.f * (x * y - w * zz), r02 = 2.f * (x * zz + w * y);
            const float r10 = 2.f * (x * y + w * zz), r11 = 1.f - 2.f * (x * x + zz * zz), r12 = 2.f * (y * zz - w * x);
            const float r20 = 2.f * (x * zz - w * y), r21 = 2.f * (y * zz + w * x), r22 = 1.f - 2.f * (x * x + y * y);
            const float e0 = expf(s_sc[3 * r]), e1 = expf(s_sc[3 * r + 1]), e2 = expf(s_sc[3 * r + 2]);
            const float u0 = (r00 * z0 + r10 * z1 + r20 * z2) * (e0 * e0);  // diag(s^2) R^T z
            const float u1 = (r01 * z0 + r11 * z1 + r21 * z2) * (e1 * e1);
            const float u2 = (r02 * z0 + r12 * z1 + r22 * z2) * (e2 * e2);
            s_sc[3 * r] = r00 * u0 + r01 * u1 + r02 * u2;
            s_sc[3 * r + 1] = r10 * u0 + r11 * u1 + r12 * u2;
            s_sc[3 * r + 2] = r20 * u0 + r21 * u1 + r22 * u2;
        }
        __syncthreads();
    }
    group_pass<3, kXyz, ADAM, NOISE>(a, row0, rows, s_sc);
}

}  // namespace

extern "C" {

size_t rt_mcmc_workspace_bytes(int P) { return reloc_workspace_bytes(P); }

int rt_mcmc_relocate(int P, const int64_t* src, const int64_t* dst, int n, float min_opacity,
                     const rt_mcmc_group* groups, int n_groups, void* workspace, size_t workspace_bytes,
                     void* stream) {
    if (P < 0 || n < 0) return fail("rt_mcmc_relocate: negative P / n");
    if (!(min_opacity > 0.f && min_opacity < 1.f)) return fail("rt_mcmc_relocate: min_opacity must be in (0, 1)");
    if (n_groups < 0 || n_groups > RT_MAX_GROUPS) return fail("rt_mcmc_relocate: n_groups must be 0..RT_MAX_GROUPS");
    if (n > 0 && !groups) return fail("rt_mcmc_relocate: null groups");
    if (n > 0 && !workspace) return fail("rt_mcmc_relocate: null workspace");
    if (n > 0 && (!src || !dst)) return fail("rt_mcmc_relocate: null src / dst");
    RelocArgs a{};
    bool has_scaling = false;
    for (int k = 0; groups && k < n_groups; k++) {
        const rt_mcmc_group& g = groups[k];
        if (!g.param || g.width <= 0) return fail("rt_mcmc_relocate: a group has a null param or width <= 0");
        if ((g.exp_avg != nullptr) != (g.exp_avg_sq != nullptr))
            return fail("rt_mcmc_relocate: a group's moments must be given or absent together");
        if (g.kind == RT_GROUP_OPACITY) {
            if (g.width != 1) return fail("rt_mcmc_relocate: the opacity group must have width 1");
            a.opacity = g.param;
        }
        has_scaling = has_scaling || g.kind == RT_GROUP_SCALING;
        a.grp[k] = RelocGroup{g.param, g.exp_avg, g.exp_avg_sq, g.width, g.kind};
    }
    if (groups && (!a.opacity || !has_scaling)) return fail("rt_mcmc_relocate: no group of kind OPACITY or SCALING");
    if (n == 0 || P == 0) return 0;
    if (workspace_bytes < reloc_workspace_bytes(P)) return fail("rt_mcmc_relocate: workspace too small", 3);
    a.n_groups = n_groups;
    a.P = P;
    a.n = n;
    a.src = src;
    a.dst = dst;
    a.counts = static_cast<uint32_t*>(workspace);
    a.min_opacity = min_opacity;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(a.counts, 0, (size_t)P * sizeof(uint32_t), st);
    if (e != hipSuccess) return fail(std::string("mcmc relocate clear: ") + hipGetErrorString(e), 2);
    k_reloc_count<<<(n + 255) / 256, 256, 0, st>>>(a);
    k_reloc_pairs<<<n, 64, 0, st>>>(a);
    k_reloc_sources<<<(P + 255) / 256, 256, 0, st>>>(a);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(std::string("mcmc relocate launch: ") + hipGetErrorString(e), 2);
    return 0;
}

int rt_mcmc_step(const rt_mcmc_step_args* s, void* stream) {
    if (!s) return fail("rt_mcmc_step: null args");
    if (s->P < 0) return fail("rt_mcmc_step: negative P");
    if (!(s->opacity_reg >= 0.0) || !(s->scale_reg >= 0.0)) return fail("rt_mcmc_step: negative regulariser weight");
    const rt_mcmc_step_group* in[4] = {&s->xyz, &s->opacity, &s->scaling, &s->rotation};  // kXyz ..
    const bool adam = s->do_adam != 0, noise = s->noise != nullptr;
    StepArgs a{};
    for (int k = 0; k < 4; k++) {
        const rt_mcmc_step_group& g = *in[k];
        if (adam && (!g.param || !g.grad || !g.exp_avg || !g.exp_avg_sq))
            return fail("rt_mcmc_step: null param / grad / moment in a group");
        if (!adam && noise && !g.param) return fail("rt_mcmc_step: null param in a group");
        StepGroup& d = a.grp[k];
        d.p = g.param;
        d.g = g.grad;
        d.m = g.exp_avg;
        d.v = g.exp_avg_sq;
        d.lr = g.lr;
        d.bc1 = g.bias_correction1;
        d.bc2s = g.bias_correction2_sqrt;
        d.vec = aligned16(g.param) && (!adam || (aligned16(g.grad) && aligned16(g.exp_avg) && aligned16(g.exp_avg_sq)));
    }
    if (s->P == 0 || (!adam && !noise)) return 0;
    a.P = s->P;
    a.beta1 = s->beta1;
    a.beta2 = s->beta2;
    a.eps = s->eps;
    a.reg_opacity = s->opacity_reg > 0.0 ? (float)(s->opacity_reg / (double)s->P) : 0.f;
    a.reg_scaling = s->scale_reg > 0.0 ? (float)(s->scale_reg / (3.0 * (double)s->P)) : 0.f;
    a.noise = s->noise;
    a.noise_scale = (float)s->noise_scale;
    a.gate_k = s->gate_k;
    a.gate_x0 = s->gate_x0;
    const unsigned blocks = (unsigned)(((int64_t)s->P + kTileRows - 1) / kTileRows);
    hipStream_t st = (hipStream_t)stream;
    if (adam && noise) k_mcmc_step<true, true><<<blocks, kThreads, 0, st>>>(a);
    else if (adam) k_mcmc_step<true, false><<<blocks, kThreads, 0, st>>>(a);
    else k_mcmc_step<false, true><<<blocks, kThreads, 0, st>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(std::string("mcmc step launch: ") + hipGetErrorString(e), 2);
    return 0;
}

}  // extern "C"
