"""Pins the reference the depth-moment gradient tests use (tests/dist_ref.py), on the CPU, for both
depth mappings: a render with colours [m_i, 1, m_i^2] over a zero background carries M1 in channel 0
and M2 in channel 2, the oracle's backward of that run equals float64 autograd of its own forward,
the chain from dL/dm_i to dL/dmeans3D equals float64 autograd of m(z(means3D)), and the per-pixel
distortion sum_{i>j} w_i w_j (m_i - m_j)^2 equals A M2 - M1^2 by brute force over the blend lists.
It pins the reference, not the feature."""
import numpy as np
import pytest
import torch

from oracle import torch_ref
from tests.common import make_scene, oracle_run, rel_l1
from tests.dist_ref import MAPPINGS, dist_part, dist_scene, mapped_depth

CASES = {
    "sh3": dict(P=250, W=48, H=40, sh_degree=3),
    "bg_mod": dict(P=200, W=40, H=32, sh_degree=2, bg=(1.0, 0.5, 0.25), scale_modifier=0.8),
}


def _pixel_weights(internals, lists, W):
    """Per pixel, float64 (ids, w = alpha T) of the oracle's blend list (forward.cu:329-347)."""
    xy = internals["xy"].astype(np.float64)
    co = internals["conic_opacity"].astype(np.float64)
    out = []
    for i, ids in enumerate(lists):
        ids = ids.astype(np.int64)
        dx, dy = xy[ids, 0] - float(i % W), xy[ids, 1] - float(i // W)
        power = -0.5 * (co[ids, 0] * dx * dx + co[ids, 2] * dy * dy) - co[ids, 1] * dx * dy
        alpha = np.minimum(0.99, co[ids, 3] * np.exp(power))
        T = np.concatenate([[1.0], np.cumprod(1.0 - alpha)[:-1]]) if len(ids) else np.zeros(0)
        out.append((ids, alpha * T))
    return out


@pytest.mark.parametrize("mapping", list(MAPPINGS))
@pytest.mark.parametrize("case", list(CASES))
def test_trick_run_is_the_moments_and_its_backward_equals_autograd(oracle, case, mapping):
    near, far = MAPPINGS[mapping]
    inp, st = make_scene(**CASES[case])
    H, W = st["image_height"], st["image_width"]
    col = oracle_run(oracle, inp, st, nthreads=1)
    internals = col["state"].internals()
    z = internals["depths"]
    rng = np.random.default_rng(5)
    dmom = rng.standard_normal((2, H, W)).astype(np.float32)
    part, tr = dist_part(oracle, inp, st, z, dmom, near, far, nthreads=1)
    assert np.array_equal(tr["radii"], col["radii"])

    # channels 0 / 2 are M1 / M2, and the distortion identity, by brute force in float64
    lists = tr["state"].blend_lists()
    vis = tr["radii"] > 0
    m, dmdz = mapped_depth(z, near, far)
    M1, M2, A, brute = (np.zeros(H * W) for _ in range(4))
    for i, (ids, w) in enumerate(_pixel_weights(internals, lists, W)):
        mi = m[ids]
        M1[i], M2[i], A[i] = (w * mi).sum(), (w * mi * mi).sum(), w.sum()
        d = mi[:, None] - mi[None, :]
        brute[i] = 0.5 * (w[:, None] * w[None, :] * d * d).sum()  # every unordered pair once
    e0, e2 = rel_l1(tr["color"][0].ravel(), M1), rel_l1(tr["color"][2].ravel(), M2)
    e1 = rel_l1(tr["color"][1], 1.0 - internals["final_T"])
    print(f"{case} {mapping}: channel 0 vs M1 {e0:.3e}, channel 2 vs M2 {e2:.3e}, channel 1 vs alpha {e1:.3e}")
    assert e0 < 1e-5 and e2 < 1e-5 and e1 < 1e-5
    assert brute.sum() > 0.0
    ident = np.abs(brute - (A * M2 - M1 * M1)).sum() / (A * M2 + M1 * M1).sum()
    print(f"{case} {mapping}: |sum_(i>j) w_i w_j (m_i - m_j)^2 - (A M2 - M1^2)| / (A M2 + M1^2) = {ident:.3e}")
    assert ident < 1e-12

    # the oracle's backward of the trick run against float64 autograd of its forward
    inp2, st2 = dist_scene(inp, st, z, near, far)
    dtrick = np.zeros((3, H, W), np.float32)
    dtrick[0], dtrick[2] = dmom[0], dmom[1]
    stn = {k: (v.numpy() if hasattr(v, "numpy") else v) for k, v in st2.items()}
    ag = torch_ref.render_autograd(stn, {k: v.numpy() for k, v in inp2.items()}, lists, vis, dtrick)
    assert rel_l1(tr["color"], ag["image"]) < 1e-5
    checked = 0
    for k in ag:
        if k == "image":
            continue
        a, b = tr["grads"][k], ag[k]
        if k == "dL_dcov3D":  # written for visible Gaussians only
            a, b = a[vis], b[vis]
        if np.abs(b).sum() == 0:
            assert np.abs(a).max() < 1e-9, k
            continue
        r = rel_l1(a, b)
        print(f"{case} {mapping}: {k} oracle vs autograd {r:.3e}")
        assert r < 1e-4, f"{k}: rel L1 {r:.3e}"
        checked += 1
    assert checked >= 6

    # the chain dL/dm_i, dL/d(m_i^2) -> dL/dmeans3D against float64 autograd of m(z(means3D))
    view = torch.as_tensor(np.asarray(st["viewmatrix"]), dtype=torch.float64).reshape(4, 4)
    mean = inp["means3D"].double().clone().requires_grad_()
    zt = mean @ view[:3, 2] + view[3, 2]
    assert rel_l1(zt.detach().numpy(), z) < 1e-6
    if near == 0.0:
        mt = zt
    else:
        mt = far / (far - near) * (1.0 - near / zt)
    dc = torch.from_numpy(np.asarray(ag["dL_dcolors"], np.float64))
    (g,) = torch.autograd.grad((dc[:, 0] * mt + dc[:, 2] * mt * mt).sum(), mean)
    chain = part["dL_dmeans3D"] - np.asarray(tr["grads"]["dL_dmeans3D"], np.float64)
    r = rel_l1(chain, g.numpy())
    print(f"{case} {mapping}: depth chain into dL_dmeans3D vs autograd {r:.3e}")
    assert np.abs(g.numpy()).sum() > 0.0 and r < 1e-4
    # nothing reaches the colour inputs
    assert np.abs(part["dL_dcolors"]).sum() == 0.0 and np.abs(part["dL_dsh"]).sum() == 0.0
