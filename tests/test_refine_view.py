"""`camera_ops.refine_view`: the per-view camera refinement loop of `gs_eval_offline` (utils/mapper.py:1888-1948) on the
device, against the same loop written here from the reference's expressions with `torch.optim.AdamW`, `.backward()` and
the torch `Camera.update_pose`.

Scene: the pattern of tests/test_render.py::_scene (900 neural points, K = 4, 160x96, surfel mode, view concat on).  The
ground truth is a `no_grad` render at the true pose; the camera then starts TAU0 away, more than `iters x lr`, so the
loop cannot converge within the iterations run and every iteration takes a full Adam step."""
import gc

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

ITERS = 8
LR_ROT, LR_TRANS, LR_EXPOSURE, ADAM_EPS = 0.003, 0.001, 0.001, 1e-15    # utils/config.py:195-198, tools.py:361
# [rho, theta]: 0.061 m / 0.044 rad, against 8 x 0.001 m / 8 x 0.003 rad the optimiser can move in ITERS iterations.
# Seed and TAU0 were picked among four seeds x three offsets for the precondition of the trajectory test: the smallest
# component of the first gradient is 6.4e-3 (depth case) and 1.9e-3 (SSIM case) of the largest.
TAU0 = (0.04, 0.03, -0.035, -0.03, 0.025, 0.02)
SEED = 2
DEPTH_KW = dict(depth_min=0.3, depth_max=50.0, depth_min_accu_alpha=0.5)
WVT_TOL, LOSS_TOL = 1e-5, 1e-4


class _Case:
    def __init__(self, seed=SEED, tau0=TAU0):
        from pings_amd.camera import se3_exp
        from pings_amd.renderer import render
        from test_render import _scene

        self.dev = dev = "cuda"
        self.data, self.decs, cam, self.geo, self.cfe = _scene(dev, seed=seed)
        self.bg = torch.tensor([0.2, 0.4, 0.6], device=dev)
        self.render = lambda c: render(c, None, self.data, self.decs, None, self.bg, view_concat_on=True,
                                       learn_color_residual=True)
        with torch.no_grad():
            gt = self.render(cam)
        self.gt_rgb = gt["render"].clamp(0, 1).clone()
        self.gt_depth = gt["surf_depth"].clone()
        T_cw = se3_exp(torch.tensor(tau0, dtype=torch.float64))           # true pose: identity
        self.start = torch.linalg.inv(T_cw)

    def camera(self):
        from pings_amd.camera import Camera

        return Camera(160, 96, 140.0, 150.0, 78.3, 49.1, 0.05, 60.0, self.start.clone(), device=self.dev)

    @staticmethod
    def groups(cam, lr_rot=LR_ROT, lr_trans=LR_TRANS, exposure=True):
        g = [{"params": [cam.exposure_mat], "lr": LR_EXPOSURE}, {"params": [cam.exposure_offset], "lr": LR_EXPOSURE}] \
            if exposure else []
        return g + [{"params": [cam.cam_rot_delta], "lr": lr_rot}, {"params": [cam.cam_trans_delta], "lr": lr_trans}]

    def net_params(self):
        return [self.geo, self.cfe] + [p for d in self.decs.values() for p in d.parameters()]

    def clear_net_grads(self):
        for p in self.net_params():
            p.grad = None


@pytest.fixture(scope="module")
def case():
    return _Case()


def _loop_b(case, lambda_ssim, lambda_depth, iters=ITERS):
    """utils/mapper.py:1888-1948 in the reference's own expressions.  Returns per-iteration poses (before each
    iteration, then the final one), total losses, first-iteration gradients and the iteration count."""
    from pings_amd.ssim import fused_ssim

    cam = case.camera()
    opt = torch.optim.AdamW(case.groups(cam), betas=(0.9, 0.99), eps=ADAM_EPS)
    gt, gtd = case.gt_rgb, case.gt_depth
    v0, v1 = 0, -1
    gt_win = gt[:, v0:v1, :]
    valid = (gtd > DEPTH_KW["depth_min"]) & (gtd < DEPTH_KW["depth_max"])
    poses, losses, first_grads, done = [], [], None, 0
    for _ in range(iters + 1):
        poses.append(cam.world_view_transform.clone())
        pkg = case.render(cam)
        if pkg is None:
            break
        rgb, depth, alpha = pkg["render"], pkg["surf_depth"], pkg["rend_alpha"]
        rgb = torch.clamp(rgb, 0, 1)[:, v0:v1, :]
        l1 = torch.abs(rgb - gt_win).mean()
        if lambda_ssim > 0.0:
            rgb_loss = (1.0 - lambda_ssim) * l1 + lambda_ssim * (1.0 - fused_ssim(rgb.unsqueeze(0), gt_win.unsqueeze(0)))
        else:
            rgb_loss = l1
        depth_loss = 0.0
        if depth is not None and lambda_depth > 0:
            valid = valid & (alpha.detach() > DEPTH_KW["depth_min_accu_alpha"])
            depth_loss = torch.abs(gtd[valid] - depth[valid]).mean() * lambda_depth
        total = rgb_loss + depth_loss
        losses.append(total.detach().clone())
        total.backward(retain_graph=True)
        if first_grads is None:
            first_grads = [p.grad.detach().clone() for g in opt.param_groups for p in g["params"]]
        with torch.no_grad():
            opt.step()
            converged = cam.update_pose()
        opt.zero_grad(set_to_none=True)
        case.clear_net_grads()
        done += 1
        if converged:
            break
    poses.append(cam.world_view_transform.clone())
    return poses, torch.stack(losses), first_grads, done


def _loop_a(case, lambda_ssim, lambda_depth, iters=ITERS, **kw):
    from pings_amd import camera_ops
    from pings_amd.optim import FusedAdamW

    cam = case.camera()
    opt = FusedAdamW(case.groups(cam), betas=(0.9, 0.99), eps=ADAM_EPS)
    poses = []

    def render_fn(c):
        poses.append(c.world_view_transform.clone())
        return case.render(c)

    res = camera_ops.refine_view(cam, render_fn, case.gt_rgb, opt, gt_depth=case.gt_depth if lambda_depth > 0 else None,
                                 iters=iters, lambda_ssim=lambda_ssim, lambda_depth=lambda_depth, **DEPTH_KW, **kw)
    poses.append(cam.world_view_transform.clone())
    return res, poses, cam, opt


@pytest.mark.parametrize("name,lambda_ssim,lambda_depth", [("depth", 0.0, 0.5), ("ssim", 0.2, 0.0)])
def test_trajectory_matches_the_reference_loop(case, name, lambda_ssim, lambda_depth):
    """Loop A (`refine_view`, FusedAdamW, device `update_pose`) against loop B (the reference's expressions,
    `torch.optim.AdamW`, `.backward()`, torch `Camera.update_pose`): per iteration `world_view_transform` to 1e-5 and
    the total loss to 1e-4 relative, the project's gates for these quantities.  Measured on an MI355X, maxima over the
    nine iterations: depth case 1.8e-7 / 4.4e-6, SSIM case 3.0e-7 / 1.5e-6."""
    poses_b, losses_b, grads_b, done_b = _loop_b(case, lambda_ssim, lambda_depth)
    # precondition (asserted, not skipped): Adam at eps = 1e-15 turns the rounding sign of a near-zero gradient component
    # into a full step, so no component of the first gradient may be near zero
    gmax = max(float(g.abs().max()) for g in grads_b)
    gmin = min(float(g.abs().min()) for g in grads_b)
    print(f"[{name}] first gradient: min |g| {gmin:.3e}, max |g| {gmax:.3e}, ratio {gmin / gmax:.3e}")
    assert gmin > 1e-3 * gmax
    print(f"[{name}] reference loop losses: {[round(v, 6) for v in losses_b.tolist()]}")
    assert float(losses_b[-1]) < float(losses_b[0])              # the loop does refine: the case is not vacuous

    case.clear_net_grads()
    res, poses_a, cam, _ = _loop_a(case, lambda_ssim, lambda_depth)
    assert res.iterations == done_b == ITERS + 1 and not res.converged
    assert len(poses_a) == len(poses_b) and res.losses.shape == losses_b.shape
    e_pose = [rel_err(a, b) for a, b in zip(poses_a, poses_b)]
    e_loss = ((res.losses - losses_b).abs() / losses_b.abs()).tolist()
    print(f"[{name}] max rel_err world_view_transform {max(e_pose):.3e}, max relative loss difference {max(e_loss):.3e}")
    assert max(e_pose) <= WVT_TOL, e_pose
    assert max(e_loss) <= LOSS_TOL, e_loss
    assert res.render_pkg is not None and res.render_pkg["render"].shape == (3, 96, 160)
    # the decoders and the features are not in this optimiser: their backward was not run
    assert all(p.grad is None for p in case.net_params())
    assert all(p.grad is None for g in _Case.groups(cam) for p in g["params"])


def test_early_stop_after_one_small_step(case):
    """Both pose learning rates 1e-5, exposure out of the optimiser: the first Adam step moves every component by its
    learning rate, |tau| = sqrt(6) 1e-5 < 1e-4."""
    from pings_amd import _lib, camera_ops
    from pings_amd.optim import FusedAdamW

    cam = case.camera()
    opt = FusedAdamW(case.groups(cam, 1e-5, 1e-5, exposure=False), betas=(0.9, 0.99), eps=ADAM_EPS)
    start = cam.world_view_transform.clone()
    _lib.sync_counts(reset=True)
    res = camera_ops.refine_view(cam, case.render, case.gt_rgb, opt, iters=ITERS)
    counts = _lib.sync_counts(reset=True)
    assert res.iterations == 1 and res.converged and res.losses.shape == (1,)
    assert counts["refine_converged"] == 1
    moved = rel_err(cam.world_view_transform, start)
    assert 0 < moved < 1e-4
    assert cam.cam_rot_delta.abs().max() == 0 and cam.cam_trans_delta.abs().max() == 0


def test_refine_off_renders_once_and_changes_nothing(case):
    from pings_amd import camera_ops
    from pings_amd.optim import FusedAdamW

    cam = case.camera()
    opt = FusedAdamW(case.groups(cam), betas=(0.9, 0.99), eps=ADAM_EPS)
    before = [p.detach().clone() for g in opt.param_groups for p in g["params"]] + [cam.world_view_transform.clone()]
    calls = []

    def render_fn(c):
        calls.append(1)
        return case.render(c)

    res = camera_ops.refine_view(cam, render_fn, case.gt_rgb, opt, iters=ITERS, refine_on=False)
    after = [p.detach().clone() for g in opt.param_groups for p in g["params"]] + [cam.world_view_transform.clone()]
    assert len(calls) == 1 and res.iterations == 0 and not res.converged and res.losses.numel() == 0
    assert res.render_pkg is not None
    assert all(torch.equal(a, b) for a, b in zip(before, after))


def test_render_fn_returning_none_ends_the_loop(case):
    from pings_amd import camera_ops
    from pings_amd.optim import FusedAdamW

    cam = case.camera()
    opt = FusedAdamW(case.groups(cam), betas=(0.9, 0.99), eps=ADAM_EPS)
    calls = []

    def render_fn(c):
        calls.append(1)
        return None

    res = camera_ops.refine_view(cam, render_fn, case.gt_rgb, opt, iters=ITERS)
    assert len(calls) == 1 and res.render_pkg is None and res.iterations == 0 and res.losses.numel() == 0


def test_negative_depth_min_is_refused(case):
    from pings_amd import camera_ops
    from pings_amd.optim import FusedAdamW

    cam = case.camera()
    opt = FusedAdamW(case.groups(cam), betas=(0.9, 0.99), eps=ADAM_EPS)
    with pytest.raises(ValueError):
        camera_ops.refine_view(cam, case.render, case.gt_rgb, opt, gt_depth=case.gt_depth, lambda_depth=0.5,
                               depth_min=-1.0)


def test_refine_view_frees_by_refcount(case):
    """tests/test_leaks.py's check on one `refine_view` call: allocated bytes do not grow with the cycle collector off."""
    from pings_amd import camera_ops
    from pings_amd.optim import FusedAdamW

    cam = case.camera()
    opt = FusedAdamW(case.groups(cam), betas=(0.9, 0.99), eps=ADAM_EPS)

    def step():
        camera_ops.set_pose(cam, case.start)
        res = camera_ops.refine_view(cam, case.render, case.gt_rgb, opt, gt_depth=case.gt_depth, iters=2,
                                     lambda_ssim=0.2, lambda_depth=0.5, **DEPTH_KW)
        assert res.iterations == 3

    case.clear_net_grads()
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
    assert grown <= 0, f"{grown} bytes still allocated after two more calls with the cycle collector off"
