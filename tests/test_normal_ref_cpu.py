"""Pins the reference the normal gradient tests use (tests/normal_ref.py), on the CPU: a render with
colours n_i (float64 torch normals) over a zero background is the oracle's aux normal map, the
oracle's backward of that run equals float64 autograd of its own forward, and on the GPU tests'
scenes no visible Gaussian sits close enough to a tie of its two smallest scales or to a grazing
view for the float32 device code to pick another axis or sign than the reference.  It pins the
reference, not the feature."""
import numpy as np
import pytest
import torch

from oracle import torch_ref
from tests.common import oracle_run, oracle_settings, rel_l1
from tests.normal_ref import SCENES, normal_scene, normal_terms, perturbed_scene, smallest_axis

CASES = {
    "sh3": dict(P=250, W=48, H=40, sh_degree=3),
    "bg_mod": dict(P=200, W=40, H=32, sh_degree=2, bg=(1.0, 0.5, 0.25), scale_modifier=0.8),
}


def _oracle_normal_map(oracle, inp, st, nthreads=0):
    n = {k: v.numpy() for k, v in inp.items()}
    out = oracle.forward(oracle_settings(oracle, st), n["means3D"], n["opacities"], shs=n.get("shs"),
                         scales=n["scales"], rotations=n["rotations"], nthreads=nthreads, normal=True)
    return out[2], out[5]


@pytest.mark.parametrize("case", list(CASES))
def test_trick_run_is_the_normal_map_and_its_backward_equals_autograd(oracle, case):
    inp, st = perturbed_scene(**CASES[case])
    H, W = st["image_height"], st["image_width"]
    radii, nmap = _oracle_normal_map(oracle, inp, st, nthreads=1)
    inp2, st2 = normal_scene(inp, st)
    rng = np.random.default_rng(5)
    dn = rng.standard_normal((3, H, W)).astype(np.float32)
    tr = oracle_run(oracle, inp2, st2, dL_dpix=dn, nthreads=1)
    assert np.array_equal(tr["radii"], radii)
    e = rel_l1(tr["color"], nmap)
    print(f"{case}: trick render vs oracle normal map rel L1 {e:.3e}")
    assert e <= 1e-5
    k = smallest_axis(inp["scales"]).numpy()
    assert len(set(k[radii > 0])) == 3, "every axis must be some visible Gaussian's smallest"

    lists = tr["state"].blend_lists()
    stn = {k: (v.numpy() if hasattr(v, "numpy") else v) for k, v in st2.items()}
    ag = torch_ref.render_autograd(stn, {k: v.numpy() for k, v in inp2.items()}, lists, tr["radii"] > 0, dn)
    assert rel_l1(tr["color"], ag["image"]) < 1e-5
    vis = tr["radii"] > 0
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
        print(f"{case}: {k} oracle vs autograd {r:.3e}")
        assert r < 1e-4, f"{k}: rel L1 {r:.3e}"
        checked += 1
    assert checked >= 6


@pytest.mark.parametrize("scene", list(SCENES))
def test_gpu_scene_input_conditions(oracle, scene):
    """Measured minima over the three scenes: 2.9e-4 (grazing) and 1.1e-5 (scale gap)."""
    inp, st = perturbed_scene(**SCENES[scene])
    radii, _nmap = _oracle_normal_map(oracle, inp, st)
    vis = torch.from_numpy(radii > 0)
    assert int(vis.sum()) > 0
    nv, p_view, k = normal_terms(inp["scales"], inp["rotations"], st["viewmatrix"], inp["means3D"])
    cosine = ((nv * p_view).sum(-1).abs() / (nv.norm(dim=-1) * p_view.norm(dim=-1)))[vis]
    s = torch.sort(inp["scales"].double(), dim=1).values[vis]
    gap = (s[:, 1] - s[:, 0]) / s[:, 1]
    counts = np.bincount(k.numpy(), minlength=3)
    print(f"{scene}: min |cos| {float(cosine.min()):.3e}, min scale gap {float(gap.min()):.3e}, k spread {counts}")
    assert float(cosine.min()) >= 1e-4
    assert float(gap.min()) >= 1e-6
    assert counts.min() > 0
