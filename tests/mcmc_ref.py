"""numpy float64 restatement of the MCMC kernels (include/rain_train.h rt_mcmc_relocate / rt_mcmc_step),
independent of rain_amd/mcmc.py: the relocation with its per-source counts, the cap at 51 copies, the
opacity clamp and the zeroed moments, and the step with regulariser, Adam and position noise."""
import math

import numpy as np

N_MAX = 51
FLT_EPSILON = float(np.finfo(np.float32).eps)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


def relocation(o, N):
    """(o', D, coeff) of one Gaussian with activated opacity `o` standing N times in one place:
    o' = 1 - (1 - o)^(1/N); D = sum_{a=1..N} sum_{k=0..a-1} C(a-1,k) (-1)^k o'^(k+1) / sqrt(k+1); coeff = o / D.
    N above N_MAX behaves as N_MAX; N = 1 is exact (o, o, 1)."""
    o = float(o)
    N = min(int(N), N_MAX)
    if N <= 1:
        return o, o, 1.0
    on = 1.0 - (1.0 - o) ** (1.0 / N)
    D = 0.0
    for a in range(1, N + 1):
        for k in range(a):
            D += math.comb(a - 1, k) * (-1.0) ** k * on ** (k + 1) / math.sqrt(k + 1)
    return on, D, o / D


def relocate(groups, src, dst, min_opacity):
    """groups: {name: (param, exp_avg or None, exp_avg_sq or None)} of float arrays [P, ...], with the
    raw "opacity" [P,1] and "scaling" [P,3] among them.  Returns the same structure after the relocation
    (float64 copies), plus the per-row counts.  Pairs with an index outside [0, P) are skipped."""
    P = groups["opacity"][0].shape[0]
    pairs = [(int(s), int(d)) for s, d in zip(src, dst) if 0 <= s < P and 0 <= d < P]
    counts = np.zeros(P, dtype=np.int64)
    for s, _d in pairs:
        counts[s] += 1
    out = {k: tuple(None if a is None else np.array(a, dtype=np.float64) for a in v) for k, v in groups.items()}
    old = {k: np.array(v[0], dtype=np.float64) for k, v in groups.items()}
    new_op, log_coeff = {}, {}
    for i in np.nonzero(counts)[0]:
        on, _D, coeff = relocation(sigmoid(old["opacity"][i, 0]), counts[i] + 1)
        xc = min(max(on, float(np.float32(min_opacity))), 1.0 - FLT_EPSILON)
        new_op[i] = math.log(xc / (1.0 - xc))
        log_coeff[i] = math.log(coeff)
    for s, d in pairs:  # pass 1: the destinations
        for k, (p, m, v) in out.items():
            p[d] = old[k][s]
            if k == "opacity":
                p[d] = new_op[s]
            if k == "scaling":
                p[d] = old[k][s] + log_coeff[s]
            if m is not None:
                m[d] = 0.0
                v[d] = 0.0
    for i in new_op:  # pass 2: the sources
        for k, (p, m, v) in out.items():
            if k == "opacity":
                p[i] = new_op[i]
            if k == "scaling":
                p[i] = old[k][i] + log_coeff[i]
            if m is not None:
                m[i] = 0.0
                v[i] = 0.0
    return out, counts


def reg_gradients(opacity, scaling, opacity_reg, scale_reg):
    """Gradients of opacity_reg * mean(sigmoid(opacity)) over [P,1] and scale_reg * mean(exp(scaling)) over [P,3]."""
    P = opacity.shape[0]
    s = sigmoid(opacity)
    return opacity_reg / P * s * (1.0 - s), scale_reg / (3.0 * P) * np.exp(np.asarray(scaling, dtype=np.float64))


def adam(p, g, m, v, lr, step, beta1=0.9, beta2=0.999, eps=1e-15):
    """One Adam step (torch.optim.Adam, no weight decay) in float64: returns (p, m, v)."""
    p, g, m, v = (np.asarray(t, dtype=np.float64) for t in (p, g, m, v))
    m = m + (1.0 - beta1) * (g - m)
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1 = 1.0 - beta1 ** step
    bc2s = math.sqrt(1.0 - beta2 ** step)
    return p - lr / bc1 * m / (np.sqrt(v) / bc2s + eps), m, v


def rotation_matrices(q):
    q = np.asarray(q, dtype=np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - w * z)
    R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y)
    R[:, 2, 1] = 2 * (y * z + w * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def noise_gate(opacity, gate_k=100.0, gate_x0=0.005):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(gate_k * (sigmoid(opacity) - gate_x0)))


def noise_delta(opacity, scaling, rotation, noise, noise_scale, gate_k=100.0, gate_x0=0.005):
    """Sigma (noise * gate * noise_scale) with Sigma = R diag(exp(scaling)^2) R^T, per row [P,3]."""
    R = rotation_matrices(rotation)
    s2 = np.exp(2.0 * np.asarray(scaling, dtype=np.float64))
    cov = np.einsum("pij,pj,pkj->pik", R, s2, R)
    z = np.asarray(noise, dtype=np.float64) * noise_gate(opacity, gate_k, gate_x0).reshape(-1, 1) * noise_scale
    return np.einsum("pik,pk->pi", cov, z)


def step(params, grads, moments, lrs, steps, do_adam=True, opacity_reg=0.0, scale_reg=0.0, noise=None,
         noise_scale=0.0, beta1=0.9, beta2=0.999, eps=1e-15):
    """The whole rt_mcmc_step on dicts keyed "xyz", "opacity", "scaling", "rotation": params / grads
    arrays, moments (m, v) pairs, lrs floats, steps the step number each group's Adam is at.  Returns
    (params, moments) in float64."""
    p = {k: np.array(a, dtype=np.float64) for k, a in params.items()}
    mom = {k: (np.array(m, dtype=np.float64), np.array(v, dtype=np.float64)) for k, (m, v) in moments.items()}
    if do_adam:
        g = {k: np.array(a, dtype=np.float64) for k, a in grads.items()}
        go, gs = reg_gradients(p["opacity"], p["scaling"], opacity_reg, scale_reg)
        g["opacity"] = g["opacity"] + go
        g["scaling"] = g["scaling"] + gs
        for k in p:
            p[k], m, v = adam(p[k], g[k], mom[k][0], mom[k][1], lrs[k], steps[k], beta1, beta2, eps)
            mom[k] = (m, v)
    if noise is not None:
        p["xyz"] = p["xyz"] + noise_delta(p["opacity"], p["scaling"], p["rotation"], noise, noise_scale)
    return p, mom
