"""Float64 reference for the camera-pose gradients (include/rain_raster.h rr_backward_camera).

Restates oracle/torch_ref.render_autograd over the oracle forward's blend lists (the same deviations:
no mask for the 0.99 alpha clamp, a clamped EWA coordinate is a constant, dL/dmeans2D in NDC units,
dL/dscales w.r.t. the modified scale), with three additions:

* viewmatrix, projmatrix and campos are three independent inputs, expanded to per-Gaussian leaves
  ([P,4,4], [P,4,4], [P,3]), so every Gaussian's contribution to each camera entry is known: the
  gradient is their sum, and S, the sum of their absolute values, measures the cancellation
  (kappa = sum S / sum |gradient|);
* the depth map sum_i w_i t_z,i and the accumulated alpha sum_i w_i (w = alpha T) are formed beside the
  colour image, t_z from the unclamped (mean, 1) . view;
* the blend runs over chunks of pixels on detached per-Gaussian quantities, whose accumulated
  gradients then go through the per-Gaussian graph once per requested loss: the backward is linear in
  the output gradients, so several (dL_dpix, dL_ddepth, dL_dalpha) triples share one forward.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle.torch_ref import _rot, _sh

DT = torch.float64
GAUSS = ("dL_dmeans3D", "dL_dopacity", "dL_dmeans2D", "dL_dsh", "dL_dcolors", "dL_dscales", "dL_drotations",
         "dL_dcov3D")


def _t(x):
    return torch.as_tensor(np.asarray(x), dtype=DT) if not isinstance(x, torch.Tensor) else x.detach().to(DT)


def camera_reference(st, inputs, blend_lists, douts, view=None, proj=None, campos=None, chunk=2048):
    """st, inputs: the settings and inputs of tests.common.make_scene (numpy or torch); blend_lists: the
    oracle forward's per-pixel lists; douts: {name: (dL_dpix [3,H,W] | None, dL_ddepth [1,H,W] | None,
    dL_dalpha [1,H,W] | None)}; view / proj / campos: override the settings' camera arrays (float64
    tensors, e.g. a CameraPose's).  Returns {name: dict} with the float64 numpy gradients of the
    Gaussians (the oracle backward's names), "view" [4,4], "proj" [4,4], "campos" [3] and "S_view",
    "S_proj", "S_campos", the loss value "loss", and under "maps" the shared (image, depth, alpha,
    visible-and-clamped mask, number of blended alphas at the 0.99 clamp)."""
    H, W = int(st["image_height"]), int(st["image_width"])
    view = _t(st["viewmatrix"] if view is None else view).reshape(4, 4)  # column-major memory: x' = (x, 1) @ view
    proj = _t(st["projmatrix"] if proj is None else proj).reshape(4, 4)
    campos = _t(st["campos"] if campos is None else campos).reshape(3)
    bg = _t(st["bg"])
    tanfovx, tanfovy = float(st["tanfovx"]), float(st["tanfovy"])
    fx, fy = W / (2.0 * tanfovx), H / (2.0 * tanfovy)
    mod, low_pass, D = float(st["scale_modifier"]), float(st["low_pass"]), int(st["sh_degree"])

    leaf = {k: _t(v).clone().requires_grad_(True) for k, v in inputs.items()}
    m = leaf["means3D"]
    P = m.shape[0]
    view_e = view[None].expand(P, 4, 4).clone().requires_grad_(True)
    proj_e = proj[None].expand(P, 4, 4).clone().requires_grad_(True)
    campos_e = campos[None].expand(P, 3).clone().requires_grad_(True)
    mh = torch.cat([m, torch.ones((P, 1), dtype=DT)], 1)
    p_hom = torch.einsum("pr,prc->pc", mh, proj_e)
    p_w = 1.0 / (p_hom[:, 3:4] + 1e-7)
    ndc = p_hom[:, :2] * p_w
    pix = torch.stack([((ndc[:, 0] + 1.0) * W - 1.0) * 0.5, ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5], 1)
    t = torch.einsum("pr,prc->pc", mh, view_e)[:, :3]

    if "cov3D_precomp" in leaf:
        cov6 = leaf["cov3D_precomp"]
    else:
        R = _rot(leaf["rotations"])
        sc = leaf["scales"]
        s = sc + (mod - 1.0) * sc.detach()  # value mod*s, gradient w.r.t. mod*s
        Mm = s[:, :, None] * R.transpose(1, 2)
        Sg = Mm.transpose(1, 2) @ Mm
        cov6 = torch.stack([Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]], 1)
    V = torch.stack([torch.stack([cov6[:, 0], cov6[:, 1], cov6[:, 2]], -1),
                     torch.stack([cov6[:, 1], cov6[:, 3], cov6[:, 4]], -1),
                     torch.stack([cov6[:, 2], cov6[:, 4], cov6[:, 5]], -1)], 1)
    limx, limy = 1.3 * tanfovx, 1.3 * tanfovy
    tz = t[:, 2]
    txtz, tytz = t[:, 0] / tz, t[:, 1] / tz
    cx = (txtz < -limx) | (txtz > limx)
    cy = (tytz < -limy) | (tytz > limy)
    tx = torch.where(cx, (txtz.clamp(-limx, limx) * tz).detach(), t[:, 0])
    ty = torch.where(cy, (tytz.clamp(-limy, limy) * tz).detach(), t[:, 1])
    zero = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx / tz, zero, -(fx * tx) / (tz * tz)], -1),
                     torch.stack([zero, fy / tz, -(fy * ty) / (tz * tz)], -1)], 1)  # [P,2,3]
    Wr = view_e[:, :3, :3].transpose(1, 2)  # R_w2c[i][j] = view_mem[4j+i]
    A = J @ Wr
    cov2 = A @ V @ A.transpose(1, 2)
    a = cov2[:, 0, 0] + low_pass
    b = cov2[:, 0, 1]
    c = cov2[:, 1, 1] + low_pass
    det = a * c - b * b
    conic = torch.stack([c / det, -b / det, a / det], 1)
    opac = leaf["opacities"].reshape(-1)
    if "colors_precomp" in leaf:
        colors = leaf["colors_precomp"]
    else:
        d = m - campos_e
        d = d / d.norm(dim=1, keepdim=True)
        colors = torch.clamp_min(_sh(D, leaf["shs"], d), 0.0)

    # ---- blend over pixel chunks, on detached per-Gaussian quantities ----
    per_g = (pix, conic, opac, colors, tz)
    q = [x.detach().clone().requires_grad_(True) for x in per_g]
    names = list(douts)
    acc = {n: [torch.zeros_like(x) for x in q] for n in names}
    loss = dict.fromkeys(names, 0.0)
    npix = H * W
    dmaps = {}
    for n in names:
        dp, dd, da = douts[n]
        dmaps[n] = (None if dp is None else _t(dp).reshape(3, npix), None if dd is None else _t(dd).reshape(npix),
                    None if da is None else _t(da).reshape(npix))
    img = bg[:, None].repeat(1, npix).clone()
    depth, alpha_map = torch.zeros(npix, dtype=DT), torch.zeros(npix, dtype=DT)
    blended = np.zeros(P, bool)
    n_alpha_clamped = 0
    for p0 in range(0, npix, chunk):
        lists = blend_lists[p0:p0 + chunk]
        n = len(lists)
        Kmax = max((len(l) for l in lists), default=0)
        if Kmax == 0:
            for nm in names:  # background only: a constant
                dp = dmaps[nm][0]
                if dp is not None:
                    loss[nm] += float((img[:, p0:p0 + n] * dp[:, p0:p0 + n]).sum())
            continue
        ids = torch.full((n, Kmax), -1, dtype=torch.long)
        for i, l in enumerate(lists):
            if len(l):
                ids[i, :len(l)] = torch.as_tensor(l.astype(np.int64))
                blended[l] = True
        valid = ids >= 0
        g = ids.clamp(min=0)
        lin = torch.arange(p0, p0 + n)
        pxy = torch.stack([(lin % W).to(DT), (lin // W).to(DT)], -1).reshape(-1, 1, 2)  # (x, y)
        dxy = q[0][g] - pxy
        co = q[1][g]
        power = -0.5 * (co[..., 0] * dxy[..., 0] ** 2 + co[..., 2] * dxy[..., 1] ** 2) \
            - co[..., 1] * dxy[..., 0] * dxy[..., 1]
        oG = q[2][g] * torch.exp(power)
        n_alpha_clamped += int(((oG > 0.99) & valid).sum())
        al = oG - (oG - 0.99).clamp(min=0).detach()  # value min(0.99, oG), gradient of oG
        al = torch.where(valid, al, torch.zeros_like(al))
        one_m = 1.0 - al
        Tpre = torch.cumprod(torch.cat([torch.ones((n, 1), dtype=DT), one_m[:, :-1]], 1), 1)
        wgt = al * Tpre
        Tfin = torch.prod(one_m, 1)
        im = (wgt[..., None] * q[3][g]).sum(1).T + Tfin[None] * bg[:, None]  # [3, n]
        dm = (wgt * q[4][g]).sum(1)
        am = wgt.sum(1)
        img[:, p0:p0 + n], depth[p0:p0 + n], alpha_map[p0:p0 + n] = im.detach(), dm.detach(), am.detach()
        for k, nm in enumerate(names):
            dp, dd, da = dmaps[nm]
            L = torch.zeros((), dtype=DT)
            if dp is not None:
                L = L + (im * dp[:, p0:p0 + n]).sum()
            if dd is not None:
                L = L + (dm * dd[p0:p0 + n]).sum()
            if da is not None:
                L = L + (am * da[p0:p0 + n]).sum()
            loss[nm] += float(L.detach())
            if L.requires_grad:
                gs = torch.autograd.grad(L, q, retain_graph=k + 1 < len(names), allow_unused=True)
                for dst, gq in zip(acc[nm], gs):
                    if gq is not None:
                        dst += gq

    # ---- the per-Gaussian graph, once per loss ----
    wanted = dict(dL_dmeans3D=m, dL_dopacity=leaf["opacities"], ndc=ndc, view=view_e, proj=proj_e, campos=campos_e)
    if "shs" in leaf:
        wanted.update(dL_dsh=leaf["shs"], dL_dcolors=colors)
    else:
        wanted.update(dL_dcolors=leaf["colors_precomp"])
    if "scales" in leaf:
        wanted.update(dL_dscales=leaf["scales"], dL_drotations=leaf["rotations"], dL_dcov3D=cov6)
    else:
        wanted.update(dL_dcov3D=leaf["cov3D_precomp"])
    keys = list(wanted)
    maps = dict(image=img.reshape(3, H, W).numpy(), depth=depth.reshape(1, H, W).numpy(),
                alpha=alpha_map.reshape(1, H, W).numpy(), clamped=(cx | cy).numpy() & blended, blended=blended,
                n_alpha_clamped=n_alpha_clamped)
    out = {}
    for k, nm in enumerate(names):
        gs = torch.autograd.grad(list(per_g), [wanted[x] for x in keys], grad_outputs=acc[nm],
                                 retain_graph=k + 1 < len(names), allow_unused=True)
        r = {x: (np.zeros(tuple(wanted[x].shape)) if gq is None else gq.numpy()) for x, gq in zip(keys, gs)}
        r["dL_dmeans2D"] = np.concatenate([r.pop("ndc"), np.zeros((P, 1))], 1)
        for x in ("view", "proj", "campos"):
            per = r[x]
            r["S_" + x] = np.abs(per).sum(0)
            r[x] = per.sum(0)
        r["loss"] = loss[nm]
        r["maps"] = maps
        out[nm] = r
    return out


# The scenes of the camera-gradient tests: the four of tests/test_depth_grad_gpu.py, one full workgroup
# of the per-Gaussian backward plus one lane, and a scene with clamped EWA coordinates.
SCENES = {
    "sh3": dict(P=3000, W=128, H=96, sh_degree=3),
    "ragged_bg": dict(P=2000, W=100, H=75, sh_degree=1, bg=(1.0, 0.5, 0.25)),
    "low_pass_300": dict(P=800, W=160, H=120, sh_degree=3, low_pass=300.0),
    "precomp": dict(P=1500, W=96, H=80, sh_degree=3, precomp_colors=True, precomp_cov=True),
    "tiny": dict(P=257, W=64, H=48, sh_degree=3, radius=5.0),  # (radius 5: no clamped EWA coordinate)
    "clamp": dict(P=300, W=48, H=40, sh_degree=3, extent=3.0, radius=3.2),
}
PARTS = ("colour", "depth", "alpha")
COMBOS = {"colour_only": ("colour",), "depth_only": ("depth",), "alpha_only": ("alpha",),
          "all": ("colour", "depth", "alpha")}
_REF = {}


def scene_reference(oracle, name):
    """Per scene, computed once and left unchanged: the inputs, random output gradients
    (default_rng(11): dL_dpix, dL_ddepth, dL_dalpha), the oracle forward's radii and blend lists, and
    the reference's colour-only, depth-only and alpha-only results ("parts"; every combination is
    their sum)."""
    if name in _REF:
        return _REF[name]
    from tests.common import make_scene, oracle_run

    inp, st = make_scene(**SCENES[name])
    H, W = st["image_height"], st["image_width"]
    rng = np.random.default_rng(11)
    dpix = rng.standard_normal((3, H, W)).astype(np.float32)
    dd = rng.standard_normal((1, H, W)).astype(np.float32)
    da = rng.standard_normal((1, H, W)).astype(np.float32)
    fw = oracle_run(oracle, inp, st)
    lists = fw["state"].blend_lists()
    parts = camera_reference(st, inp, lists, dict(colour=(dpix, None, None), depth=(None, dd, None),
                                                  alpha=(None, None, da)))
    _REF[name] = dict(inp=inp, st=st, dpix=dpix, dd=dd, da=da, radii=fw["radii"], lists=lists, parts=parts)
    return _REF[name]


def combine(parts, which, key):
    return sum(np.asarray(parts[p][key], np.float64) for p in which)


def kappa(r):
    """sum S / sum |gradient| of the three camera arrays of one camera_reference result."""
    return {x: float(r["S_" + x].sum() / max(np.abs(r[x]).sum(), 1e-300)) for x in ("view", "proj", "campos")}


def chain_pose(pose, r):
    """The six CameraPose gradients (rot_delta, trans_delta) of a camera_reference result `r` taken at
    `pose`'s own matrices, by autograd through the (float64) CameraPose."""
    L = (pose.world_view_transform * torch.as_tensor(r["view"])).sum() \
        + (pose.full_proj_transform * torch.as_tensor(r["proj"])).sum() \
        + (pose.camera_center * torch.as_tensor(r["campos"])).sum()
    g = torch.autograd.grad(L, [pose.rot_delta, pose.trans_delta])
    return np.concatenate([g[0].numpy(), g[1].numpy()])
