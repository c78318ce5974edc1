// geom_loss.hip — fused depth-normal consistency + depth loss (include/rain_loss.h, rl_geom_*).
//
// Inputs are the rasterizer's unnormalised maps D = sum a T z, A = sum a T, N = sum a T n.  With
// z = D / A where A >= alpha_min, r(p) the pixel-centre ray (r_z = 1) and P = z r, the depth normal
// of an interior pixel whose four axis neighbours are all usable is n_d = c / |c|,
// c = t_v x t_u, t_u = P(x+1,y) - P(x-1,y), t_v = P(x,y+1) - P(x,y-1), and
//   L_n = (1/HW) sum_valid (A - N . n_d),   L_d = (1/HW) sum_{ok, gt>0} |z - gt|.
//
// t_u = r du + dx su e_x and t_v = r dv + dy sv e_y with du = zE - zW, su = zE + zW (dv, sv likewise
// along y) and dx = 2 tanfovx / W, dy = 2 tanfovy / H the ray step per pixel, so the products P
// are never differenced.  The r x r terms of the cross product cancel exactly, which leaves
//   c = (a, b, -(rx a + ry b + e)),  a = dy sv du,  b = dx su dv,  e = dx dy su sv.
// The centre depth does not enter c: the stencil's gradient is four scalars per pixel,
// dL/dzE, dL/dzW, dL/dzS, dL/dzN.  The forward stores them with n_d (seven planes); the backward
// gathers, for pixel q, gE(x-1,y) + gW(x+1,y) + gS(x,y-1) + gN(x,y+1) — no atomics — and applies
// z = D / A's chain rule.  Loss sums: per-block partials in double, reduced in a fixed order.
//
// Each thread owns V consecutive pixels of a row: V = 4 (16-byte loads and stores) when W is a
// multiple of 4 and every pointer is 16-byte aligned, else V = 1.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/rain_loss.h"
#include "loss_err.hpp"

namespace {

using rl_detail::g_err;

constexpr int kThreads = 256;  // per block; also the finalize's width
constexpr int kPlanes = 7;     // gE, gW, gS, gN, n_d.xyz
constexpr int kNbMax = 1 << 22;

struct GeomP {
    const float* D;
    const float* A;
    const float* N;   // null or unused when the normal term is off
    const float* gt;  // null or unused when the depth term is off
    int H, W;
    float tx, ty;      // tan(fov/2)
    float hx, hy;      // tanfov / extent: r_x = (2x+1) hx - tx
    float dx, dy;      // 2 tanfov / extent: the ray step per pixel
    float alpha_min;
    float kn, kd;      // lambda_normal / HW, lambda_depth / HW (0 = term off)
    float lam_n, lam_d;
    double inv_n;      // 1 / HW
};

template <int V>
struct Geo {
    static constexpr int BX = V == 4 ? 16 : 64;  // threads along x: a block covers 64 pixels of a row
    static constexpr int BY = kThreads / BX;
};

template <int V>
__device__ __forceinline__ void load_v(const float* __restrict__ p, size_t i, float (&o)[V]) {
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p + i);
        o[0] = t.x;
        o[1] = t.y;
        o[2] = t.z;
        o[3] = t.w;
    } else {
        o[0] = p[i];
    }
}
template <int V>
__device__ __forceinline__ void store_v(float* __restrict__ p, size_t i, const float (&o)[V]) {
    if constexpr (V == 4) {
        *reinterpret_cast<float4*>(p + i) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
        p[i] = o[0];
    }
}

// z = D / A where A >= alpha_min (a NaN alpha is not usable); returns the mask
__device__ __forceinline__ bool depth_of(float d, float a, float alpha_min, float& z) {
    const bool ok = a >= alpha_min;
    z = ok ? d / a : 0.f;
    return ok;
}

// V pixels' depths of row y starting at column x0 (in the image)
template <int V>
__device__ __forceinline__ void depth_row(const GeomP& g, size_t i, float (&z)[V], bool (&ok)[V]) {
    float d[V], a[V];
    load_v<V>(g.D, i, d);
    load_v<V>(g.A, i, a);
#pragma unroll
    for (int k = 0; k < V; k++) ok[k] = depth_of(d[k], a[k], g.alpha_min, z[k]);
}

// Block sums in a fixed order: lanes by butterfly, then the waves in order.
__device__ __forceinline__ void block_partial(double s0, double s1, double s2, double* __restrict__ out) {
    __shared__ double sm[kThreads / 64][3];
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o);
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
    }
    if ((tid & 63) == 0) {
        sm[tid >> 6][0] = s0;
        sm[tid >> 6][1] = s1;
        sm[tid >> 6][2] = s2;
    }
    __syncthreads();
    if (tid == 0) {
        double t0 = 0.0, t1 = 0.0, t2 = 0.0;
        for (int w = 0; w < kThreads / 64; w++) {
            t0 += sm[w][0];
            t1 += sm[w][1];
            t2 += sm[w][2];
        }
        out[0] = t0;
        out[1] = t1;
        out[2] = t2;
    }
}

// The loss from the block partials, by one block of kThreads (its own launch after the forward, or
// the extra block of the backward launch: the same additions in the same order).
__device__ __forceinline__ void geom_finalize(const double* __restrict__ partial, int nb, const GeomP& g,
                                              float* __restrict__ loss, float* __restrict__ parts) {
    __shared__ double fin[3];
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = tid; i < nb; i += kThreads) {
        s0 += partial[3 * (size_t)i + 0];
        s1 += partial[3 * (size_t)i + 1];
        s2 += partial[3 * (size_t)i + 2];
    }
    block_partial(s0, s1, s2, fin);
    if (tid == 0) {
        const float ln = (float)(fin[0] * g.inv_n);
        const float ld = (float)(fin[1] * g.inv_n);
        const float total = g.lam_n * ln + g.lam_d * ld;
        loss[0] = total;
        if (parts) {
            parts[0] = total;
            parts[1] = ln;
            parts[2] = ld;
            parts[3] = (float)fin[2];
        }
    }
}

template <int V>
__global__ __launch_bounds__(kThreads) void k_geom_fwd(GeomP g, float* __restrict__ ws, double* __restrict__ partial) {
    const int x0 = (blockIdx.x * Geo<V>::BX + threadIdx.x) * V;
    const int y = blockIdx.y * Geo<V>::BY + threadIdx.y;
    const int H = g.H, W = g.W;
    const size_t plane = (size_t)H * W;
    float ln = 0.f, ld = 0.f;
    int cnt = 0;
    if (y < H && x0 < W) {  // V == 4: W is a multiple of 4, so x0 + 3 < W
        const size_t i = (size_t)y * W + x0;
        float zc[V + 2];  // columns x0-1 .. x0+V of row y
        bool okc[V + 2];
        float a[V];
        {
            float d[V];
            load_v<V>(g.D, i, d);
            load_v<V>(g.A, i, a);
#pragma unroll
            for (int k = 0; k < V; k++) okc[k + 1] = depth_of(d[k], a[k], g.alpha_min, zc[k + 1]);
        }
        if (g.kd != 0.f) {
            float t[V];
            load_v<V>(g.gt, i, t);
#pragma unroll
            for (int k = 0; k < V; k++)
                if (okc[k + 1] && t[k] > 0.f) ld += fabsf(zc[k + 1] - t[k]);
        }
        if (g.kn != 0.f) {
            float gE[V], gW[V], gS[V], gN[V], nx[V], ny[V], nz[V];
#pragma unroll
            for (int k = 0; k < V; k++) gE[k] = gW[k] = gS[k] = gN[k] = nx[k] = ny[k] = nz[k] = 0.f;
            if (y >= 1 && y <= H - 2) {  // rows with a depth normal
                okc[0] = okc[V + 1] = false;
                zc[0] = zc[V + 1] = 0.f;
                if (x0 >= 1) okc[0] = depth_of(g.D[i - 1], g.A[i - 1], g.alpha_min, zc[0]);
                if (x0 + V < W) okc[V + 1] = depth_of(g.D[i + V], g.A[i + V], g.alpha_min, zc[V + 1]);
                float zn[V], zs[V], nm[3][V];
                bool okn[V], oks[V];
                depth_row<V>(g, i - W, zn, okn);
                depth_row<V>(g, i + W, zs, oks);
#pragma unroll
                for (int c = 0; c < 3; c++) load_v<V>(g.N + c * plane, i, nm[c]);
                const float ry = fmaf((float)(2 * y + 1), g.hy, -g.ty);
#pragma unroll
                for (int k = 0; k < V; k++) {
                    const int x = x0 + k;
                    if (x >= 1 && x <= W - 2 && okc[k + 1] && okc[k] && okc[k + 2] && okn[k] && oks[k]) {
                        const float rx = fmaf((float)(2 * x + 1), g.hx, -g.tx);
                        const float du = zc[k + 2] - zc[k], su = zc[k + 2] + zc[k];
                        const float dv = zs[k] - zn[k], sv = zs[k] + zn[k];
                        const float ca = g.dy * sv * du, cb = g.dx * su * dv, ce = g.dx * g.dy * su * sv;
                        const float cz = -(rx * ca + ry * cb + ce);
                        const float c2 = ca * ca + cb * cb + cz * cz;
                        if (c2 > 0.f) {
                            const float inv = 1.0f / sqrtf(c2);
                            const float n0 = ca * inv, n1 = cb * inv, n2 = cz * inv;
                            const float dot = nm[0][k] * n0 + nm[1][k] * n1 + nm[2][k] * n2;
                            ln += a[k] - dot;
                            cnt++;
                            // d(-N.n_d)/dc = -(N - (N.n_d) n_d) / |c|, scaled by lambda_normal / HW
                            const float s = -g.kn * inv;
                            const float g0 = s * (nm[0][k] - dot * n0), g1 = s * (nm[1][k] - dot * n1),
                                        g2 = s * (nm[2][k] - dot * n2);
                            const float fa = g0 - rx * g2, fb = g1 - ry * g2, fe = -g2;
                            const float fdu = fa * g.dy * sv, fsv = fa * g.dy * du + fe * g.dx * g.dy * su;
                            const float fdv = fb * g.dx * su, fsu = fb * g.dx * dv + fe * g.dx * g.dy * sv;
                            gE[k] = fsu + fdu;
                            gW[k] = fsu - fdu;
                            gS[k] = fsv + fdv;
                            gN[k] = fsv - fdv;
                            nx[k] = n0;
                            ny[k] = n1;
                            nz[k] = n2;
                        }
                    }
                }
            }
            store_v<V>(ws, i, gE);
            store_v<V>(ws + plane, i, gW);
            store_v<V>(ws + 2 * plane, i, gS);
            store_v<V>(ws + 3 * plane, i, gN);
            store_v<V>(ws + 4 * plane, i, nx);
            store_v<V>(ws + 5 * plane, i, ny);
            store_v<V>(ws + 6 * plane, i, nz);
        }
    }
    block_partial((double)ln, (double)ld, (double)cnt, partial + 3 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x));
}

__global__ __launch_bounds__(kThreads) void k_geom_finalize(GeomP g, const double* __restrict__ partial, int nb,
                                                            float* __restrict__ loss, float* __restrict__ parts) {
    geom_finalize(partial, nb, g, loss, parts);
}

template <int V>
__global__ __launch_bounds__(kThreads) void k_geom_bwd(GeomP g, const float* __restrict__ ws,
                                                       const float* __restrict__ grad_loss, float* __restrict__ dD,
                                                       float* __restrict__ dA, float* __restrict__ dN,
                                                       const double* __restrict__ partial, int nb,
                                                       float* __restrict__ loss, float* __restrict__ parts) {
    if (loss && blockIdx.x == gridDim.x - 1) {  // the extra column (block-uniform): the forward's finalize
        if (blockIdx.y == 0) geom_finalize(partial, nb, g, loss, parts);
        return;
    }
    const int x0 = (blockIdx.x * Geo<V>::BX + threadIdx.x) * V;
    const int y = blockIdx.y * Geo<V>::BY + threadIdx.y;
    const int H = g.H, W = g.W;
    if (y >= H || x0 >= W) return;
    const size_t plane = (size_t)H * W;
    const size_t i = (size_t)y * W + x0;
    const float gl = grad_loss[0];
    float d[V], a[V], dz[V], od[V], oa[V];
    load_v<V>(g.D, i, d);
    load_v<V>(g.A, i, a);
#pragma unroll
    for (int k = 0; k < V; k++) dz[k] = 0.f;
    const bool use_n = g.kn != 0.f;
    float n[3][V];
    if (use_n) {
        // the four stencils that contain pixel (x, y): those of (x-1,y), (x+1,y), (x,y-1), (x,y+1)
        float e[V], w[V], t[V];
        load_v<V>(ws, i, e);          // gE of columns x0 .. x0+V-1; wanted: x-1
        load_v<V>(ws + plane, i, w);  // gW; wanted: x+1
        const float e_left = x0 >= 1 ? ws[i - 1] : 0.f;
        const float w_right = x0 + V < W ? ws[plane + i + V] : 0.f;
#pragma unroll
        for (int k = 0; k < V; k++) dz[k] = (k == 0 ? e_left : e[k - 1]) + (k == V - 1 ? w_right : w[k + 1]);
        if (y >= 1) {
            load_v<V>(ws + 2 * plane, i - W, t);  // gS of (x, y-1)
#pragma unroll
            for (int k = 0; k < V; k++) dz[k] += t[k];
        }
        if (y + 1 < H) {
            load_v<V>(ws + 3 * plane, i + W, t);  // gN of (x, y+1)
#pragma unroll
            for (int k = 0; k < V; k++) dz[k] += t[k];
        }
#pragma unroll
        for (int c = 0; c < 3; c++) load_v<V>(ws + (4 + c) * plane, i, n[c]);
    }
    float gtv[V];
    if (g.kd != 0.f) load_v<V>(g.gt, i, gtv);
#pragma unroll
    for (int k = 0; k < V; k++) {
        float z;
        const bool ok = depth_of(d[k], a[k], g.alpha_min, z);
        float gz = dz[k];  // zero unless ok: a stencil that contains this pixel needed it usable
        if (g.kd != 0.f && ok && gtv[k] > 0.f) {
            const float df = z - gtv[k];
            gz += g.kd * (df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f));
        }
        float ga = 0.f, gd = 0.f;
        if (ok) {
            gd = gz / a[k];
            ga = -gd * z;
            if (use_n && (n[0][k] != 0.f || n[1][k] != 0.f || n[2][k] != 0.f)) ga += g.kn;  // valid: n_d is a unit vector
        }
        od[k] = gl * gd;
        oa[k] = gl * ga;
    }
    store_v<V>(dD, i, od);
    store_v<V>(dA, i, oa);
    if (dN) {
        const float s = -gl * g.kn;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float o[V];
#pragma unroll
            for (int k = 0; k < V; k++) o[k] = use_n ? s * n[c][k] : 0.f;
            store_v<V>(dN + c * plane, i, o);
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline dim3 grid_of(int H, int W, int V) {
    const int by = V == 4 ? Geo<4>::BY : Geo<1>::BY;
    return dim3((W + 63) / 64, (H + by - 1) / by, 1);  // a block covers 64 columns in either form
}
// the larger of the two forms' block counts (V = 1: 4 rows per block)
inline size_t max_blocks(int H, int W) { return (size_t)((W + 63) / 64) * ((H + Geo<1>::BY - 1) / Geo<1>::BY); }
inline size_t maps_bytes(int H, int W) { return (((size_t)kPlanes * H * W * sizeof(float)) + 15) & ~(size_t)15; }

GeomP make_params(const float* D, const float* A, const float* N, const float* gt, int H, int W, float tanfovx,
                  float tanfovy, float alpha_min, float lam_n, float lam_d) {
    GeomP g;
    const double n = (double)H * W;
    g.D = D;
    g.A = A;
    g.N = N;
    g.gt = gt;
    g.H = H;
    g.W = W;
    g.tx = tanfovx;
    g.ty = tanfovy;
    g.hx = (float)((double)tanfovx / W);
    g.hy = (float)((double)tanfovy / H);
    g.dx = (float)(2.0 * (double)tanfovx / W);
    g.dy = (float)(2.0 * (double)tanfovy / H);
    g.alpha_min = alpha_min;
    g.lam_n = N ? lam_n : 0.f;
    g.lam_d = gt ? lam_d : 0.f;
    g.kn = (float)((double)g.lam_n / n);
    g.kd = (float)((double)g.lam_d / n);
    g.inv_n = 1.0 / n;
    return g;
}

// shared argument checks (before any HIP call); `need_ws_bytes`: 0 = the size is not known here
int validate(const char* who, const float* D, const float* A, const float* N, const float* gt, int H, int W,
             float lam_n, float lam_d, const void* ws, bool check_ws_bytes, size_t ws_bytes) {
    if (H <= 0 || W <= 0) {
        g_err = std::string(who) + ": bad argument (H and W must be positive)";
        return 1;
    }
    if (!D || !A || !ws) {
        g_err = std::string(who) + ": bad argument (null depth, alpha or workspace)";
        return 1;
    }
    if (lam_n != 0.f && !N) {
        g_err = std::string(who) + ": lambda_normal is non-zero but no normal map is given";
        return 1;
    }
    if (lam_d != 0.f && !gt) {
        g_err = std::string(who) + ": lambda_depth is non-zero but no gt_depth is given";
        return 1;
    }
    if ((size_t)H * W >= ((size_t)1 << 30) || max_blocks(H, W) > (size_t)kNbMax) {
        g_err = std::string(who) + ": image larger than 2^30 pixels";
        return 1;
    }
    if (check_ws_bytes && ws_bytes < rl_geom_workspace_bytes(H, W)) {
        g_err = std::string(who) + ": workspace too small";
        return 3;
    }
    return 0;
}

int pick_v(const GeomP& g, const void* ws, const float* dD, const float* dA, const float* dN) {
    const bool al = aligned16(g.D) && aligned16(g.A) && aligned16(g.N) && aligned16(g.gt) && aligned16(ws) &&
                    aligned16(dD) && aligned16(dA) && aligned16(dN);
    return (g.W % 4 == 0 && al) ? 4 : 1;
}

void launch_fwd(const GeomP& g, int V, float* ws, double* partial, hipStream_t st) {
    const dim3 grid = grid_of(g.H, g.W, V);
    if (V == 4)
        k_geom_fwd<4><<<grid, dim3(Geo<4>::BX, Geo<4>::BY), 0, st>>>(g, ws, partial);
    else
        k_geom_fwd<1><<<grid, dim3(Geo<1>::BX, Geo<1>::BY), 0, st>>>(g, ws, partial);
}

void launch_bwd(const GeomP& g, int V, const float* ws, const float* grad_loss, float* dD, float* dA, float* dN,
                const double* partial, float* loss, float* parts, hipStream_t st) {
    dim3 grid = grid_of(g.H, g.W, V);
    const int nb = (int)(grid.x * grid.y);
    if (loss) grid.x += 1;
    if (V == 4)
        k_geom_bwd<4><<<grid, dim3(Geo<4>::BX, Geo<4>::BY), 0, st>>>(g, ws, grad_loss, dD, dA, dN, partial, nb, loss,
                                                                    parts);
    else
        k_geom_bwd<1><<<grid, dim3(Geo<1>::BX, Geo<1>::BY), 0, st>>>(g, ws, grad_loss, dD, dA, dN, partial, nb, loss,
                                                                    parts);
}

int launch_status(const char* who) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        g_err = std::string(who) + ": " + hipGetErrorString(e);
        return 2;
    }
    return 0;
}

}  // namespace

extern "C" {

size_t rl_geom_workspace_bytes(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return maps_bytes(H, W) + max_blocks(H, W) * 3 * sizeof(double) + 256;
}

int rl_geom_forward(const float* depth, const float* alpha, const float* normal, const float* gt_depth, int H, int W,
                    float tanfovx, float tanfovy, float alpha_min, float lambda_normal, float lambda_depth,
                    void* workspace, size_t workspace_bytes, float* loss, float* parts, void* stream) {
    const char* who = "rl_geom_forward";
    if (int rc = validate(who, depth, alpha, normal, gt_depth, H, W, lambda_normal, lambda_depth, workspace, true,
                          workspace_bytes))
        return rc;
    if (!loss) {
        g_err = std::string(who) + ": bad argument (null loss)";
        return 1;
    }
    const GeomP g = make_params(depth, alpha, normal, gt_depth, H, W, tanfovx, tanfovy, alpha_min, lambda_normal,
                                lambda_depth);
    float* ws = static_cast<float*>(workspace);
    double* partial = reinterpret_cast<double*>(static_cast<char*>(workspace) + maps_bytes(H, W));
    hipStream_t st = (hipStream_t)stream;
    const int V = pick_v(g, ws, nullptr, nullptr, nullptr);
    launch_fwd(g, V, ws, partial, st);
    const dim3 grid = grid_of(H, W, V);
    k_geom_finalize<<<1, dim3(Geo<1>::BX, Geo<1>::BY), 0, st>>>(g, partial, (int)(grid.x * grid.y), loss, parts);
    return launch_status(who);
}

int rl_geom_backward(const float* depth, const float* alpha, const float* normal, const float* gt_depth, int H, int W,
                     float tanfovx, float tanfovy, float alpha_min, float lambda_normal, float lambda_depth,
                     const void* workspace, const float* grad_loss, float* d_depth, float* d_alpha, float* d_normal,
                     void* stream) {
    const char* who = "rl_geom_backward";
    if (int rc = validate(who, depth, alpha, normal, gt_depth, H, W, lambda_normal, lambda_depth, workspace, false, 0))
        return rc;
    if (!grad_loss || !d_depth || !d_alpha || (normal && !d_normal)) {
        g_err = std::string(who) + ": bad argument (null grad_loss or gradient output)";
        return 1;
    }
    const GeomP g = make_params(depth, alpha, normal, gt_depth, H, W, tanfovx, tanfovy, alpha_min, lambda_normal,
                                lambda_depth);
    const float* ws = static_cast<const float*>(workspace);
    const int V = pick_v(g, ws, d_depth, d_alpha, d_normal);
    launch_bwd(g, V, ws, grad_loss, d_depth, d_alpha, d_normal, nullptr, nullptr, nullptr, (hipStream_t)stream);
    return launch_status(who);
}

int rl_geom_forward_backward(const float* depth, const float* alpha, const float* normal, const float* gt_depth,
                             int H, int W, float tanfovx, float tanfovy, float alpha_min, float lambda_normal,
                             float lambda_depth, void* workspace, size_t workspace_bytes, float* loss, float* parts,
                             const float* grad_loss, float* d_depth, float* d_alpha, float* d_normal, void* stream) {
    const char* who = "rl_geom_forward_backward";
    if (int rc = validate(who, depth, alpha, normal, gt_depth, H, W, lambda_normal, lambda_depth, workspace, true,
                          workspace_bytes))
        return rc;
    if (!loss || !grad_loss || !d_depth || !d_alpha || (normal && !d_normal)) {
        g_err = std::string(who) + ": bad argument (null loss, grad_loss or gradient output)";
        return 1;
    }
    const GeomP g = make_params(depth, alpha, normal, gt_depth, H, W, tanfovx, tanfovy, alpha_min, lambda_normal,
                                lambda_depth);
    float* ws = static_cast<float*>(workspace);
    double* partial = reinterpret_cast<double*>(static_cast<char*>(workspace) + maps_bytes(H, W));
    hipStream_t st = (hipStream_t)stream;
    const int V = pick_v(g, ws, d_depth, d_alpha, d_normal);
    launch_fwd(g, V, ws, partial, st);
    launch_bwd(g, V, ws, grad_loss, d_depth, d_alpha, d_normal, partial, loss, parts, st);
    return launch_status(who);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Depth-distortion loss (include/rain_loss.h, rl_dist_*): with the rasterizer's accumulated alpha A
// and depth-moment maps M1 = sum w m, M2 = sum w m^2 (include/rain_raster.h rr_forward_render_dist),
//   L = lambda (1/HW) sum_p (A M2 - M1^2)       (= sum_{i>j} w_i w_j (m_i - m_j)^2 per pixel; no clamp)
//   dL/dA = lambda/HW M2,  dL/dM1 = -2 lambda/HW M1,  dL/dM2 = lambda/HW A.
// Pointwise: the maps are walked as flat arrays of HW pixels, V = 4 per thread when HW is a multiple
// of 4 and every pointer is 16-byte aligned (the M2 plane then is too), else V = 1.  Loss sum: per-block
// partials in double, reduced in a fixed order by one block (its own launch after the forward, or
// the extra block of the backward launch: the same additions in the same order).  No atomics.
namespace {

constexpr int kDistNbMax = 1 << 20;

struct DistP {
    const float* A;
    const float* M;  // [2,HW]
    size_t n;        // HW
    float lam, k;    // lambda, lambda / HW
    double inv_n;
};

__device__ __forceinline__ double block_sum1(double s) {
    __shared__ double sm1[kThreads / 64];
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((tid & 63) == 0) sm1[tid >> 6] = s;
    __syncthreads();
    double t = 0.0;
    if (tid == 0)
        for (int w = 0; w < kThreads / 64; w++) t += sm1[w];
    return t;  // thread 0's value is the block's sum
}

__device__ __forceinline__ void dist_finalize(const double* __restrict__ partial, int nb, const DistP& g,
                                              float* __restrict__ loss, float* __restrict__ parts) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += kThreads) s += partial[i];
    const double t = block_sum1(s);
    if (threadIdx.x == 0) {
        const float mean = (float)(t * g.inv_n);
        const float total = g.lam * mean;
        loss[0] = total;
        if (parts) {
            parts[0] = total;
            parts[1] = mean;
        }
    }
}

template <int V>
__global__ __launch_bounds__(kThreads) void k_dist_fwd(DistP g, double* __restrict__ partial) {
    const size_t i = ((size_t)blockIdx.x * kThreads + threadIdx.x) * V;
    double s = 0.0;
    if (i < g.n) {  // V == 4: n is a multiple of 4, so i + 3 < n
        float a[V], m1[V], m2[V];
        load_v<V>(g.A, i, a);
        load_v<V>(g.M, i, m1);
        load_v<V>(g.M + g.n, i, m2);
#pragma unroll
        for (int k = 0; k < V; k++) s += (double)(a[k] * m2[k] - m1[k] * m1[k]);
    }
    const double t = block_sum1(s);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__global__ __launch_bounds__(kThreads) void k_dist_finalize(DistP g, const double* __restrict__ partial, int nb,
                                                            float* __restrict__ loss, float* __restrict__ parts) {
    dist_finalize(partial, nb, g, loss, parts);
}

template <int V>
__global__ __launch_bounds__(kThreads) void k_dist_bwd(DistP g, const float* __restrict__ grad_loss,
                                                       float* __restrict__ dA, float* __restrict__ dM, int accumulate,
                                                       const double* __restrict__ partial, int nb,
                                                       float* __restrict__ loss, float* __restrict__ parts) {
#pragma clang fp contract(off)  // the accumulated alpha gradient is old + (c M2), never fma(c, M2, old)
    if (loss && blockIdx.x == gridDim.x - 1) {  // the extra block (block-uniform): the forward's finalize
        dist_finalize(partial, nb, g, loss, parts);
        return;
    }
    const size_t i = ((size_t)blockIdx.x * kThreads + threadIdx.x) * V;
    if (i >= g.n) return;
    const float c = grad_loss[0] * g.k;
    float a[V], m1[V], m2[V], oa[V], o1[V], o2[V];
    load_v<V>(g.A, i, a);
    load_v<V>(g.M, i, m1);
    load_v<V>(g.M + g.n, i, m2);
    if (accumulate) load_v<V>(dA, i, oa);
#pragma unroll
    for (int k = 0; k < V; k++) {
        const float ga = c * m2[k];
        oa[k] = accumulate ? oa[k] + ga : ga;  // a plain add of the rounded gradient
        o1[k] = -2.f * c * m1[k];
        o2[k] = c * a[k];
    }
    store_v<V>(dA, i, oa);
    store_v<V>(dM, i, o1);
    store_v<V>(dM + g.n, i, o2);
}

inline int dist_blocks(size_t n, int V) { return (int)((n + (size_t)kThreads * V - 1) / ((size_t)kThreads * V)); }

int dist_validate(const char* who, const float* A, const float* M, int H, int W) {
    if (H <= 0 || W <= 0) {
        g_err = std::string(who) + ": bad argument (H and W must be positive)";
        return 1;
    }
    if (!A || !M) {
        g_err = std::string(who) + ": bad argument (null alpha or moments)";
        return 1;
    }
    if ((size_t)H * W >= ((size_t)1 << 28)) {
        g_err = std::string(who) + ": image larger than 2^28 pixels";
        return 1;
    }
    return 0;
}

DistP dist_params(const float* A, const float* M, int H, int W, float lam) {
    DistP g;
    g.A = A;
    g.M = M;
    g.n = (size_t)H * W;
    g.lam = lam;
    g.k = (float)((double)lam / (double)g.n);
    g.inv_n = 1.0 / (double)g.n;
    return g;
}

int dist_pick_v(const DistP& g, const float* dA, const float* dM) {
    return (g.n % 4 == 0 && aligned16(g.A) && aligned16(g.M) && aligned16(dA) && aligned16(dM)) ? 4 : 1;
}

void dist_launch_fwd(const DistP& g, int V, double* partial, hipStream_t st) {
    if (V == 4)
        k_dist_fwd<4><<<dist_blocks(g.n, 4), kThreads, 0, st>>>(g, partial);
    else
        k_dist_fwd<1><<<dist_blocks(g.n, 1), kThreads, 0, st>>>(g, partial);
}

void dist_launch_bwd(const DistP& g, int V, const float* grad_loss, float* dA, float* dM, int accumulate,
                     const double* partial, float* loss, float* parts, hipStream_t st) {
    const int nb = dist_blocks(g.n, V);
    const int grid = nb + (loss ? 1 : 0);
    if (V == 4)
        k_dist_bwd<4><<<grid, kThreads, 0, st>>>(g, grad_loss, dA, dM, accumulate, partial, nb, loss, parts);
    else
        k_dist_bwd<1><<<grid, kThreads, 0, st>>>(g, grad_loss, dA, dM, accumulate, partial, nb, loss, parts);
}

}  // namespace

extern "C" {

size_t rl_dist_workspace_bytes(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return (size_t)dist_blocks((size_t)H * W, 1) * sizeof(double) + 256;  // the V = 1 form's block count
}

int rl_dist_forward(const float* alpha, const float* moments, int H, int W, float lambda_dist, void* workspace,
                    size_t workspace_bytes, float* loss, float* parts, void* stream) {
    const char* who = "rl_dist_forward";
    if (int rc = dist_validate(who, alpha, moments, H, W)) return rc;
    if (!workspace || !loss) {
        g_err = std::string(who) + ": bad argument (null workspace or loss)";
        return 1;
    }
    if (workspace_bytes < rl_dist_workspace_bytes(H, W)) {
        g_err = std::string(who) + ": workspace too small";
        return 3;
    }
    const DistP g = dist_params(alpha, moments, H, W, lambda_dist);
    double* partial = static_cast<double*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    const int V = dist_pick_v(g, nullptr, nullptr);
    dist_launch_fwd(g, V, partial, st);
    k_dist_finalize<<<1, kThreads, 0, st>>>(g, partial, dist_blocks(g.n, V), loss, parts);
    return launch_status(who);
}

int rl_dist_backward(const float* alpha, const float* moments, int H, int W, float lambda_dist,
                     const float* grad_loss, float* d_alpha, float* d_moments, int accumulate_alpha, void* stream) {
    const char* who = "rl_dist_backward";
    if (int rc = dist_validate(who, alpha, moments, H, W)) return rc;
    if (!grad_loss || !d_alpha || !d_moments) {
        g_err = std::string(who) + ": bad argument (null grad_loss or gradient output)";
        return 1;
    }
    const DistP g = dist_params(alpha, moments, H, W, lambda_dist);
    const int V = dist_pick_v(g, d_alpha, d_moments);
    dist_launch_bwd(g, V, grad_loss, d_alpha, d_moments, accumulate_alpha, nullptr, nullptr, nullptr,
                    (hipStream_t)stream);
    return launch_status(who);
}

int rl_dist_forward_backward(const float* alpha, const float* moments, int H, int W, float lambda_dist,
                             void* workspace, size_t workspace_bytes, float* loss, float* parts,
                             const float* grad_loss, float* d_alpha, float* d_moments, int accumulate_alpha,
                             void* stream) {
    const char* who = "rl_dist_forward_backward";
    if (int rc = dist_validate(who, alpha, moments, H, W)) return rc;
    if (!workspace || !loss || !grad_loss || !d_alpha || !d_moments) {
        g_err = std::string(who) + ": bad argument (null workspace, loss, grad_loss or gradient output)";
        return 1;
    }
    if (workspace_bytes < rl_dist_workspace_bytes(H, W)) {
        g_err = std::string(who) + ": workspace too small";
        return 3;
    }
    const DistP g = dist_params(alpha, moments, H, W, lambda_dist);
    double* partial = static_cast<double*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    // the forward's vector width: the loss is then bitwise rl_dist_forward's whatever the gradient
    // outputs' alignment
    const int Vf = dist_pick_v(g, nullptr, nullptr);
    dist_launch_fwd(g, Vf, partial, st);
    const int nbf = dist_blocks(g.n, Vf);
    const int V = dist_pick_v(g, d_alpha, d_moments);
    const int nb = dist_blocks(g.n, V);
    if (V == 4)
        k_dist_bwd<4><<<nb + 1, kThreads, 0, st>>>(g, grad_loss, d_alpha, d_moments, accumulate_alpha, partial, nbf, loss,
                                                   parts);
    else
        k_dist_bwd<1><<<nb + 1, kThreads, 0, st>>>(g, grad_loss, d_alpha, d_moments, accumulate_alpha, partial, nbf, loss,
                                                   parts);
    return launch_status(who);
}

}  // extern "C"
