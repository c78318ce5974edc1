"""Pins the float64 reference of the camera-pose gradients (tests/camera_ref.py) without a GPU: its
Gaussian gradients against the oracle's backward, the translation invariance that ties the camera
gradients to dL/dmeans3D, central differences through CameraPose with the blend lists held fixed,
the entries that must be exactly zero, and the conditioning of every scene the GPU test uses."""
import numpy as np
import pytest
import torch

from rain_amd import cameras
from tests.camera_ref import COMBOS, SCENES, camera_reference, chain_pose, combine, kappa, scene_reference
from tests.common import make_scene, oracle_run, rel_l1
from tests.test_oracle_autograd import CASES


@pytest.mark.parametrize("scene", list(SCENES))
def test_scenes_are_well_conditioned(oracle, scene):
    """A condition on the scenes, not a measurement: with kappa = sum S / sum |gradient| <= 50 the fp32
    rounding of a sum of P terms, ~ eps * kappa = 3e-6, leaves 30x under the 1e-4 bar."""
    ref = scene_reference(oracle, scene)
    for combo, which in COMBOS.items():
        r = {k: combine(ref["parts"], which, k) for k in ("view", "proj", "campos", "S_view", "S_proj", "S_campos")}
        k = kappa(r)
        print(f"{scene} {combo}: kappa {k}")
        for x, v in k.items():
            assert v <= 50.0, (scene, combo, x, v)
    maps = ref["parts"]["colour"]["maps"]
    for part in ref["parts"].values():
        for k, v in part.items():
            if k not in ("maps", "loss"):
                assert np.isfinite(v).all(), k
    if scene == "clamp":
        assert maps["clamped"].sum() > 0, "the clamp scene must blend a Gaussian with a clamped EWA coordinate"


@pytest.mark.parametrize("case", list(CASES))
def test_gaussian_gradients_equal_oracle_backward(oracle, case):
    inp, st = make_scene(**CASES[case])
    rng = np.random.default_rng(3)
    dpix = rng.standard_normal((3, st["image_height"], st["image_width"])).astype(np.float32)
    ref = oracle_run(oracle, inp, st, dL_dpix=dpix, nthreads=1)
    r = camera_reference(st, inp, ref["state"].blend_lists(), dict(c=(dpix, None, None)))["c"]
    assert rel_l1(ref["color"], r["maps"]["image"]) < 1e-5
    g, vis = ref["grads"], ref["radii"] > 0
    for k in ("dL_dmeans3D", "dL_dopacity", "dL_dmeans2D", "dL_dsh", "dL_dcolors", "dL_dscales", "dL_drotations",
              "dL_dcov3D"):
        if k not in r:
            continue
        a, b = g[k], r[k]
        if k == "dL_dsh":
            K = (st["sh_degree"] + 1) ** 2
            a, b = a[:, :K], b[:, :K]
        if k == "dL_dcov3D":
            a, b = a[vis], b[vis]
        if np.abs(b).sum() == 0:
            assert np.abs(a).max() < 1e-9, k
            continue
        e = rel_l1(a, b)
        assert e < 1e-4, f"{k}: rel L1 {e:.3e}"


def _chain_centre(st, r):
    """dL/d(camera centre) from the camera gradients: the centre c enters the translation row of the
    view matrix, -c . Rw, through it the last row of proj = view . Pm (Pm = view^-1 . proj), and campos."""
    view = np.asarray(st["viewmatrix"], np.float64).reshape(4, 4)
    proj = np.asarray(st["projmatrix"], np.float64).reshape(4, 4)
    Pm = np.linalg.inv(view) @ proj
    Rw = view[:3, :3]
    return -Rw @ r["view"][3, :3] - (Rw @ Pm[:3, :]) @ r["proj"][3, :] + r["campos"]


def test_translation_invariance(oracle):
    """Moving the camera centre by d is moving every mean by -d: the chain above equals
    -sum_i dL/dmeans3D_i.  (Not with clamped EWA coordinates, whose constants break the symmetry.)"""
    ref = scene_reference(oracle, "tiny")
    assert ref["parts"]["colour"]["maps"]["clamped"].sum() == 0
    r = {k: combine(ref["parts"], COMBOS["all"], k) for k in ("view", "proj", "campos", "dL_dmeans3D")}
    got, want = _chain_centre(ref["st"], r), -r["dL_dmeans3D"].sum(0)
    e = rel_l1(got, want)
    print(f"translation invariance: rel L1 {e:.3e}")
    assert np.abs(want).sum() > 0 and e <= 1e-9


def test_central_differences_through_camera_pose(oracle):
    """The six CameraPose gradients by autograd through the camera arrays against central differences
    of the loss in float64, the blend lists held fixed.  A radian moves a splat by ~1e2 pixels, a few
    of its widths, so each derivative in the pose gains a factor ~1e2: at h = 1e-6 the truncation,
    ~ h^2 f''' / f' ~ 1e-12 * 1e4, and the rounding, ~ 1e-16 |L| / (h |f'|), both stay under 1e-7
    relative; 1e-6 is asserted."""
    ref = scene_reference(oracle, "tiny")
    maps = ref["parts"]["colour"]["maps"]
    assert maps["clamped"].sum() == 0 and maps["n_alpha_clamped"] == 0  # a smooth function of the pose
    cam = cameras.fibonacci_cameras(8, 64, 48, radius=SCENES["tiny"]["radius"])[0]  # make_scene's camera
    pose = cameras.CameraPose(cam, dtype=torch.float64)
    assert np.array_equal(pose.world_view_transform.detach().float().numpy(), ref["st"]["viewmatrix"].numpy())
    douts = dict(all=(ref["dpix"], ref["dd"], ref["da"]))

    def run(delta):
        with torch.no_grad():
            pose.rot_delta.copy_(torch.as_tensor(delta[:3]))
            pose.trans_delta.copy_(torch.as_tensor(delta[3:]))
        return camera_reference(ref["st"], ref["inp"], ref["lists"], douts, view=pose.world_view_transform,
                                proj=pose.full_proj_transform, campos=pose.camera_center)["all"]

    x0 = np.array([4e-4, -3e-4, 2e-4, 1e-3, -6e-4, 8e-4])  # (nonzero: the matrix_exp path; no new clamp)
    at = run(x0)
    assert at["maps"]["clamped"].sum() == 0 and at["maps"]["n_alpha_clamped"] == 0  # smooth at x0 too
    got = chain_pose(pose, at)
    h, fd = 1e-6, np.zeros(6)
    for i in range(6):
        e = np.zeros(6)
        e[i] = h
        fd[i] = (run(x0 + e)["loss"] - run(x0 - e)["loss"]) / (2 * h)
    err = rel_l1(got, fd)
    print(f"central differences: analytic {got}, numeric {fd}, rel L1 {err:.3e}")
    assert np.abs(fd).min() > 0 and err <= 1e-6


@pytest.mark.parametrize("scene", ["sh3", "precomp", "clamp"])
def test_entries_no_kernel_reads_are_exactly_zero(oracle, scene):
    ref = scene_reference(oracle, scene)
    for part in ref["parts"].values():
        assert np.all(part["view"][:, 3] == 0) and np.all(part["S_view"][:, 3] == 0)  # memory 3, 7, 11, 15
        assert np.all(part["proj"][:, 2] == 0) and np.all(part["S_proj"][:, 2] == 0)  # the z row: 2, 6, 10, 14
    for p in ("depth", "alpha"):  # the direction feeds the colour only
        assert np.all(ref["parts"][p]["S_campos"] == 0)
    if scene == "precomp":
        assert np.all(ref["parts"]["colour"]["S_campos"] == 0)
    else:
        assert np.abs(ref["parts"]["colour"]["campos"]).sum() > 0
