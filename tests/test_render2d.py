"""`render(gs_type="2d_gs")` and `spawn_gaussians(gs_type="2d_gs")` end to end on the GPU, against the 3d_gs spawn
and the 2DGS restatement (tests/raster2d_ref.py)."""
import copy
import gc
import math

import pytest
import torch

from conftest import rel_err
from test_render import _scene
from tests import raster2d_ref as R2

KEYS = ("render", "rend_alpha", "rend_normal", "rend_dist", "surf_depth", "surf_normal", "viewspace_points",
        "visibility_filter", "radii", "gaussian_xyz", "gaussian_scale", "alpha_all", "local_view_gaussian_count")


def _render(gs_type="2d_gs", hidden=64, **kw):
    from pings_amd.renderer import render

    dev = "cuda"
    data, decs, cam, geo, cfe = _scene(dev, gs_type, hidden=hidden)
    bg = torch.tensor([0.2, 0.4, 0.6], device=dev)
    with torch.no_grad():
        cam.exposure_mat.copy_(torch.eye(3, device=dev) * 0.9 + 0.05)
        cam.exposure_offset.copy_(torch.tensor([0.01, -0.02, 0.03], device=dev))
    args = dict(view_concat_on=True, learn_color_residual=True, gs_type=gs_type, displacement_range_ratio=2.0,
                max_scale_ratio=2.0, unit_scale_ratio=0.5)
    args.update(kw)
    return render(cam, None, data, decs, None, bg, **args), cam, bg, geo, cfe, decs


@pytest.mark.gpu
@pytest.mark.parametrize("median,d2n", [(False, True), (True, False), (True, True)])
def test_render_2d_gs_keys_shapes_and_values(median, d2n):
    pkg, cam, bg, geo, cfe, decs = _render(use_median_depth=median, d2n_on=d2n)
    for k in KEYS:
        assert k in pkg, k
    assert "contributions" not in pkg
    H, W = 96, 160
    assert pkg["render"].shape == (3, H, W) and pkg["rend_alpha"].shape == (1, H, W)
    assert pkg["rend_normal"].shape == (3, H, W) and pkg["rend_dist"].shape == (1, H, W)
    assert pkg["surf_depth"].shape == (1, H, W)
    assert (pkg["surf_normal"] is not None) == d2n
    assert pkg["gaussian_scale"].shape[1] == 2
    # restatement on the very Gaussians that were spawned (fp64)
    c = lambda t: t.detach().cpu().to(torch.float64)
    cam_d = dict(viewmatrix=c(cam.world_view_transform), projmatrix=c(cam.full_proj_transform))
    sc = dict(means=c(pkg["gaussian_xyz"]), scales=c(pkg["gaussian_scale"]), rot=c(pkg["gaussian_rot"]),
              op=c(pkg["gaussian_alpha"]), col=c(pkg["gaussian_color"]), bg=c(bg), cam=cam_d, W=W, H=H)
    r32 = R2.full(sc, torch.float32, keep_pairs=True)
    o = R2.full(sc, torch.float64, keep_pairs=True)
    keep = ~R2.undecidable(r32, o, W, H).view(H, W)
    assert keep.float().mean().item() >= 0.98
    assert torch.equal(pkg["radii"].cpu().long(), r32["pre32"]["radii"])
    img = o["image"].permute(1, 2, 0).reshape(-1, 3) @ c(cam.exposure_mat).T + c(cam.exposure_offset)
    img = img.view(H, W, 3).permute(2, 0, 1)
    assert rel_err(pkg["render"][:, keep], img[:, keep]) <= 1e-4
    am = o["allmap"]
    alpha = am[1:2]
    assert rel_err(pkg["rend_alpha"][:, keep], alpha[:, keep]) <= 1e-4
    assert rel_err(pkg["rend_normal"][:, keep], am[2:5][:, keep]) <= 1e-4
    # the distortion is the published running sum of O(m^2) <= 1 terms that cancel (a nearly planar map leaves ~1e-6):
    # fp32 holds it to ~1e-7 absolute, so it is compared absolutely, not relative to its tiny maximum
    assert (pkg["rend_dist"].detach().cpu().double()[:, keep] - am[6:7][:, keep]).abs().max().item() <= 1e-6
    exp_d = torch.where(alpha > 1e-3, am[0:1] / alpha.clamp_min(1e-30), am[0:1])
    want = am[5:6] if median else exp_d
    sel = keep[None] & ((alpha - 1e-3).abs() > 1e-5)        # away from the min_alpha mask edge
    assert rel_err(pkg["surf_depth"][sel], want[sel]) <= 1e-4


@pytest.mark.gpu
def test_render_2d_gs_spawn_matches_the_spawn_oracle():
    """First link of the oracle chain: the Gaussians `render(gs_type="2d_gs")` spawned equal oracle/spawn_cpu.py's 2d_gs
    spawn (fp64, CPU; the 3d_gs activation with the first two scale columns, :672-673) on the same visible mask.  The
    second link (those Gaussians -> the 2DGS restatement) is test_render_2d_gs_keys_shapes_and_values."""
    from oracle.spawn_cpu import spawn_gaussians as spawn_ref
    from pings_amd import renderer

    pkg, cam, bg, geo, cfe, decs = _render(d2n_on=False)
    data, _, _, _, _ = _scene("cuda", "2d_gs")
    H, W = 96, 160
    rast = renderer._settings(cam, "2d_gs", H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), bg, 1.0, 0,
                              True, "cuda")
    vis = rast.markVisible(data["position"]).cpu()
    d64 = {k: (v.detach().cpu().double() if torch.is_tensor(v) and v.is_floating_point() else
               (v.cpu() if torch.is_tensor(v) else v)) for k, v in data.items()}
    dec64 = {n: copy.deepcopy(d).cpu().double() for n, d in decs.items()}
    ref = spawn_ref(d64, dec64, vis, cam.camera_center.detach().cpu().double(), False, True, z_far=cam.zfar,
                    learn_color_residual=True, gs_type="2d_gs", displacement_range_ratio=2.0, max_scale_ratio=2.0,
                    unit_scale_ratio=0.5)
    assert ref["gaussian_scale"].shape[1] == 2
    assert pkg["local_view_gaussian_count"] == ref["local_view_gaussian_count"]
    for k in ("gaussian_xyz", "gaussian_scale", "gaussian_rot", "gaussian_alpha", "gaussian_color", "alpha_all"):
        assert pkg[k].shape == ref[k].shape, k
        assert rel_err(pkg[k], ref[k]) <= 1e-4, k


@pytest.mark.gpu
def test_render_2d_gs_mapper_loss_backpropagates_with_distortion():
    from pings_amd import _lib

    from pings_amd import renderer

    assert renderer.ONE_SYNC
    _lib.sync_counts(reset=True)
    pkg, cam, bg, geo, cfe, decs = _render(d2n_on=True, hidden=128)
    counts = _lib.sync_counts(reset=True)
    counts.pop("settings_tensor_readback", None)     # a camera tensor's first read
    assert counts == {"raster_instance_count": 1}, counts
    loss = (pkg["render"] - 0.5).abs().mean() + 0.1 * pkg["rend_dist"].mean() + \
        0.05 * (1 - (pkg["rend_normal"] * pkg["surf_normal"]).sum(0)).mean() + 0.01 * pkg["surf_depth"].mean()
    loss.backward()
    assert geo.grad is not None and cfe.grad is not None
    assert torch.isfinite(geo.grad).all() and torch.isfinite(cfe.grad).all()
    assert geo.grad.abs().sum() > 0
    for d in decs.values():
        for p in d.parameters():
            if p.grad is not None:
                assert torch.isfinite(p.grad).all()


@pytest.mark.gpu
def test_spawn_2d_gs_equals_3d_gs_with_two_scale_columns():
    from pings_amd.renderer import spawn_gaussians

    dev = "cuda"
    outs = {}
    for gs in ("3d_gs", "2d_gs"):
        data, decs, cam, geo, cfe = _scene(dev, gs)
        sp = spawn_gaussians(data, decs, None, cam.camera_center, False, True, gs_type=gs, learn_color_residual=True)
        g = torch.Generator().manual_seed(9)
        loss = 0
        for k in ("gaussian_xyz", "gaussian_rot", "gaussian_alpha", "gaussian_color"):
            loss = loss + (sp[k] * torch.randn(sp[k].shape, generator=g).to(dev)).sum()
        sc = sp["gaussian_scale"][:, :2]
        loss = loss + (sc * torch.randn(sc.shape, generator=g).to(dev)).sum()
        loss.backward()
        outs[gs] = (sp, geo.grad.clone(), cfe.grad.clone(),
                    [p.grad.clone() for d in decs.values() for p in d.parameters() if p.grad is not None])
    a, b = outs["3d_gs"], outs["2d_gs"]
    assert b[0]["gaussian_scale"].shape[1] == 2
    assert torch.equal(b[0]["gaussian_scale"], a[0]["gaussian_scale"][:, :2])
    for k in ("gaussian_xyz", "gaussian_rot", "gaussian_alpha", "gaussian_color", "alpha_all"):
        assert torch.equal(a[0][k], b[0][k]), k
    assert a[0]["local_view_gaussian_count"] == b[0]["local_view_gaussian_count"]
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert len(a[3]) == len(b[3]) and all(torch.equal(x, y) for x, y in zip(a[3], b[3]))


def _stable_after(step):
    gc.collect()
    gc.disable()
    try:
        step()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        grown = torch.cuda.memory_allocated() - base
    finally:
        gc.enable()
    assert grown <= 0, f"{grown} bytes still allocated after two more steps with the cycle collector off"


@pytest.mark.gpu
def test_2dgs_node_and_render_step_free_by_refcount():
    sc = R2.make_scene(3000, 160, 96, seed=5)
    from test_raster2d import _hip, _leaves

    rast = _hip(sc)
    lv = _leaves(sc)

    def node_step():
        for t in lv.values():
            t.grad = None
        m2 = torch.zeros_like(lv["means"], requires_grad=True)
        img, radii, allm = rast(means3D=lv["means"], means2D=m2, opacities=lv["op"], colors_precomp=lv["col"],
                                scales=lv["scales"], rotations=lv["rot"])
        (img.sum() + allm.sum()).backward()

    _stable_after(node_step)

    from pings_amd.renderer import render

    dev = "cuda"
    data, decs, cam, geo, cfe = _scene(dev, "2d_gs")
    bg = torch.tensor([0.2, 0.4, 0.6], device=dev)

    def render_step():
        geo.grad = None
        cfe.grad = None
        pkg = render(cam, None, data, decs, None, bg, view_concat_on=True, gs_type="2d_gs", d2n_on=True)
        (pkg["render"].mean() + pkg["rend_dist"].mean() + pkg["surf_depth"].mean()).backward()

    _stable_after(render_step)


# ------------------------------------------------------------------ one host synchronisation per frame
def _run_render2d(one_sync, with_frozen, dev="cuda"):
    """render(gs_type="2d_gs") + a loss over every output and the returned Gaussians + backward (pkg, grads, syncs)."""
    from pings_amd import _lib, renderer

    data, decs, cam, geo, cfe = _scene(dev, "2d_gs", hidden=128)
    data["valid_mask"][100:140] = False
    data["free_mask"][::7] = True
    bg = torch.tensor([0.2, 0.4, 0.6], device=dev)
    frozen = None
    if with_frozen:                      # a frozen 2d_gs map keeps two scale columns
        g = torch.Generator().manual_seed(11)
        m = 300
        fz = torch.stack([(torch.rand(m, generator=g) - 0.5) * 5, (torch.rand(m, generator=g) - 0.5) * 3,
                          3.0 + torch.rand(m, generator=g)], 1)
        frozen = {"gaussian_xyz": fz.to(dev), "gaussian_alpha": torch.rand(m, 1, generator=g).to(dev),
                  "gaussian_scale": (0.05 + 0.1 * torch.rand(m, 2, generator=g)).to(dev),
                  "gaussian_rot": torch.nn.functional.normalize(torch.randn(m, 4, generator=g), dim=1).to(dev),
                  "gaussian_color": torch.rand(m, 3, generator=g).to(dev)}
    prev = renderer.ONE_SYNC
    renderer.ONE_SYNC = one_sync
    try:
        _lib.sync_counts(reset=True)
        pkg = renderer.render(cam, None, data, decs, frozen, bg, view_concat_on=True, learn_color_residual=True,
                              d2n_on=True, gs_type="2d_gs", use_median_depth=with_frozen,
                              displacement_range_ratio=2.0, max_scale_ratio=2.0, unit_scale_ratio=0.5)
        syncs = _lib.sync_counts(reset=True)
    finally:
        renderer.ONE_SYNC = prev
    loss = pkg["render"].mean() + 0.1 * pkg["surf_depth"].mean() + 0.05 * pkg["rend_alpha"].mean() \
        + 0.3 * pkg["surf_normal"].abs().mean() + 0.2 * pkg["rend_normal"].abs().mean() + pkg["rend_dist"].mean() \
        + 0.01 * pkg["gaussian_scale"].mean() + 0.02 * pkg["gaussian_alpha"].abs().mean() \
        + 0.01 * pkg["alpha_all"].pow(2).mean() + 0.01 * pkg["gaussian_xyz"].pow(2).mean() \
        + 0.01 * (pkg["gaussian_rot"] * pkg["gaussian_color"][:, :1]).sum()
    loss.backward()
    grads = {"geo": geo.grad, "cfe": cfe.grad, "rot_delta": cam.cam_rot_delta.grad,
             "trans_delta": cam.cam_trans_delta.grad, "exposure_mat": cam.exposure_mat.grad,
             "exposure_offset": cam.exposure_offset.grad, "viewspace": pkg["viewspace_points"].grad}
    for nm, d in decs.items():
        for i, p in enumerate(d.parameters()):
            grads[f"{nm}.{i}"] = p.grad
    return pkg, grads, syncs


@pytest.mark.gpu
@pytest.mark.parametrize("with_frozen", [False, True])
def test_one_sync_2d_gs_render_equals_the_legacy_path_bit_for_bit(with_frozen):
    """The fused spawn + 2DGS rasteriser node (render_core.py) against the legacy path: one host synchronisation,
    every returned tensor, shape and gradient identical."""
    p1, g1, s1 = _run_render2d(True, with_frozen)
    p0, g0, s0 = _run_render2d(False, with_frozen)
    s1.pop("settings_tensor_readback", None)
    s0.pop("settings_tensor_readback", None)
    assert s1 == {"raster_instance_count": 1}, s1
    assert sum(s0.values()) >= 4, s0
    assert set(p1.keys()) == set(p0.keys())
    assert p1["gaussian_scale"].shape[1] == 2
    for k in p0:
        a, b = p1[k], p0[k]
        if torch.is_tensor(b):
            assert a.shape == b.shape and a.dtype == b.dtype, k
            assert torch.equal(a, b), k
        else:
            assert a == b, (k, a, b)
    assert g1["rot_delta"] is None and g1["trans_delta"] is None      # no pose tangent in 2d_gs (:351-358)
    for k in g0:
        a, b = g1[k], g0[k]
        assert (a is None) == (b is None), k
        if b is not None:
            assert a.shape == b.shape and torch.equal(a, b), k
