"""Camera poses on the HIP device (csrc/camera.hip).

`update_pose(camera)` and `set_pose(camera, cam_pose)` are the reference's `utils/campose_utils.py:79-98` and
`CamImage.set_pose` (gaussian_splatting/utils/cameras.py:207-219), each as one allocation and one launch with no host
wait; `refine_view` is the per-view camera refinement loop of `gs_eval_offline` (utils/mapper.py:1888-1948) on top of
them with one host read per iteration.  `install` rebinds the reference's names.  `pings_amd.camera.Camera` keeps its
torch methods: they are the CPU path and the baseline of the tests.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _abi, _lib

BLOCK_WORDS = 40        # wvt [0,16), fpt [16,32), centre [32,35), |tau| 36, converged 37 (include/pings_hip.h)
_FLAG_BYTE = 37 * 4     # low byte of the little-endian uint32 flag


def _entry(name: str):
    L = _lib.lib()
    if not hasattr(L, name):    # a library built before this entry existed (same ABI version)
        raise _lib.PingsHipError(f"{_lib.LIB_PATH} has no {name}: rebuild it with `python -m pings_amd.build`")
    return getattr(L, name)


def _f32_dev(name: str, t, numel: int) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise _lib.PingsHipError(f"camera_ops: the camera has no {name} (set a pose first)")
    if not t.is_cuda:
        raise _lib.PingsHipError(f"camera_ops runs on the HIP device only ({name} is a CPU tensor); "
                                 "there is no CPU fallback")
    if t.dtype is not torch.float32 or t.numel() != numel:
        raise _lib.PingsHipError(f"camera_ops: {name} must hold {numel} float32 values, got {t.dtype} "
                                 f"{tuple(t.shape)}")
    return t


def _bind(camera, block: torch.Tensor) -> None:
    wvt = block[:16].view(4, 4)
    camera.world_view_transform = wvt
    camera.full_proj_transform = block[16:32].view(4, 4)
    camera.camera_center = block[32:35]
    camera.R = wvt[:3, :3].T            # T_cw[:3, :3]
    camera.T = wvt[3, :3]               # T_cw[:3, 3]


@torch.no_grad()
def update_pose(camera, converged_threshold=1e-4) -> torch.Tensor:
    """`T_cw <- SE3_exp([cam_trans_delta, cam_rot_delta]) @ T_cw` in one launch; rebinds `world_view_transform`,
    `full_proj_transform`, `camera_center`, `R` and `T` of `camera` to views of one new block (detached) and zeroes the
    deltas.  Returns a 0-dim bool device tensor with the reference's return value (`|tau| < converged_threshold`, True
    for `|tau| == 0`, where the camera's tensors are carried over bit for bit); reading it is the only host wait."""
    R, T = _f32_dev("R", camera.R, 9), _f32_dev("T", camera.T, 3)
    P = _f32_dev("projection_matrix", camera.projection_matrix, 16)
    wvt = _f32_dev("world_view_transform", camera.world_view_transform, 16)
    fpt = _f32_dev("full_proj_transform", camera.full_proj_transform, 16)
    cen = _f32_dev("camera_center", camera.camera_center, 3)
    rho = _f32_dev("cam_trans_delta", camera.cam_trans_delta, 3).detach()
    theta = _f32_dev("cam_rot_delta", camera.cam_rot_delta, 3).detach()
    dev = R.device
    for name, t in (("T", T), ("projection_matrix", P), ("world_view_transform", wvt), ("full_proj_transform", fpt),
                    ("camera_center", cen), ("cam_trans_delta", rho), ("cam_rot_delta", theta)):
        if t.device != dev:
            raise _lib.PingsHipError(f"camera_ops: {name} is on {t.device}, R on {dev}")
    if not (rho.is_contiguous() and theta.is_contiguous()):
        raise _lib.PingsHipError("camera_ops: the pose deltas must be contiguous")
    fn = _entry("pings_camera_update_pose")
    block = torch.empty(BLOCK_WORDS, dtype=torch.float32, device=dev)
    R, P, wvt, fpt = R.reshape(3, 3), P.reshape(4, 4), wvt.reshape(4, 4), fpt.reshape(4, 4)    # views: shapes agree
    T, cen = T.reshape(3), cen.reshape(3)
    a = _abi.CameraPoseArgs(
        R.data_ptr(), T.data_ptr(), P.data_ptr(), wvt.data_ptr(), fpt.data_ptr(), cen.data_ptr(), rho.data_ptr(),
        theta.data_ptr(), block.data_ptr(), R.stride(0), R.stride(1), T.stride(0), P.stride(0), P.stride(1),
        wvt.stride(0), wvt.stride(1), fpt.stride(0), fpt.stride(1), cen.stride(0), float(converged_threshold))
    if dev.index != torch.cuda.current_device():
        with torch.cuda.device(dev):
            st = fn(C.byref(a), _lib.stream_ptr(dev))
    else:
        st = fn(C.byref(a), _lib.stream_ptr(dev))
    _lib.check(st, "pings_camera_update_pose")
    _bind(camera, block)
    return block.view(torch.uint8)[_FLAG_BYTE].view(torch.bool)


@torch.no_grad()
def set_pose(camera, cam_pose) -> None:
    """`CamImage.set_pose`: `cam_pose` is T_wc (camera -> world), fp64 or fp32; None changes nothing.  T_cw is the
    general 4x4 inverse in fp64.  A singular pose gives non-finite matrices instead of torch's exception (raising would
    need the host wait this function removes).  A CPU pose is copied to the camera's device first."""
    if cam_pose is None:
        return
    P = _f32_dev("projection_matrix", camera.projection_matrix, 16)
    dev = P.device
    pose = cam_pose.detach()
    if pose.device != dev:
        pose = pose.to(dev)
    if pose.dtype not in (torch.float64, torch.float32):
        pose = pose.to(torch.float64)
    if pose.shape != (4, 4):
        raise _lib.PingsHipError(f"camera_ops.set_pose: cam_pose must be [4, 4], got {tuple(pose.shape)}")
    P = P.reshape(4, 4)
    fn = _entry("pings_camera_set_pose")
    block = torch.empty(BLOCK_WORDS, dtype=torch.float32, device=dev)
    args = (pose.data_ptr(), int(pose.dtype is torch.float64), pose.stride(0), pose.stride(1), P.data_ptr(),
            P.stride(0), P.stride(1), block.data_ptr(), _lib.stream_ptr(dev))
    if dev.index != torch.cuda.current_device():
        with torch.cuda.device(dev):
            st = fn(*args)
    else:
        st = fn(*args)
    _lib.check(st, "pings_camera_set_pose")
    _bind(camera, block)


# ---------------------------------------------------------------- install
def install(*caller_modules, cam_cls=None) -> None:
    """`import utils.campose_utils as CU, utils.mapper as M, inspect_pings as IP; install(CU, M, IP, cam_cls=CamImage)`:
    the name `update_pose` is rebound in every module given (those that imported it by name included) and, if a class
    is given, its `set_pose`.  The originals are kept for `uninstall`.  Installing twice changes nothing."""
    for mod in caller_modules:
        cur = getattr(mod, "update_pose", None)
        if cur is not update_pose:
            mod._pings_update_pose_original = cur
            mod.update_pose = update_pose
    if cam_cls is not None and cam_cls.__dict__.get("set_pose") is not set_pose:
        cam_cls._pings_set_pose_original = cam_cls.__dict__.get("set_pose")
        cam_cls.set_pose = set_pose


def uninstall(*caller_modules, cam_cls=None) -> None:
    """Puts the reference's own `update_pose` / `set_pose` back wherever `install` replaced them."""
    for mod in caller_modules:
        if getattr(mod, "update_pose", None) is update_pose and hasattr(mod, "_pings_update_pose_original"):
            mod.update_pose = mod._pings_update_pose_original
            del mod._pings_update_pose_original
    if cam_cls is not None and cam_cls.__dict__.get("set_pose") is set_pose:
        orig = cam_cls.__dict__.get("_pings_set_pose_original")
        if orig is not None:
            cam_cls.set_pose = orig
        else:
            del cam_cls.set_pose
        if "_pings_set_pose_original" in cam_cls.__dict__:
            del cam_cls._pings_set_pose_original


# ---------------------------------------------------------------- per-view refinement loop
class RefineResult(NamedTuple):
    render_pkg: Optional[dict]      # the last render package: the one rendered before the final update (None: no render)
    iterations: int                 # optimiser steps taken
    converged: bool                 # the last `update_pose` reported |tau| < converged_threshold
    losses: torch.Tensor            # [iterations] total loss of every iteration, on the device


def refine_view(camera, render_fn, gt_rgb: torch.Tensor, opt, *, gt_depth: Optional[torch.Tensor] = None,
                iters: int = 50, refine_on: bool = True, lambda_ssim: float = 0.0, lambda_depth: float = 0.0,
                depth_min: float = 0.0, depth_max: float = float("inf"), depth_min_accu_alpha: float = 0.0,
                pixel_v_min: int = 0, pixel_v_max: int = -1, converged_threshold: float = 1e-4) -> RefineResult:
    """The camera refinement loop of `gs_eval_offline` (utils/mapper.py:1888-1948): up to `iters + 1` passes of
    `render_fn(camera)` (the caller closes over the map, the decoders and the render options), L1 (+ SSIM) colour loss
    over the row window `pixel_v_min:pixel_v_max`, depth L1 over the valid mask, `opt.step()`, `update_pose`, and ONE
    host read per iteration (the converged flag).  Gradients are taken for the parameters of `opt` only, so the
    backward of the decoders and features, which this optimiser does not hold, is not run.

    As in the reference, the valid-depth mask is AND-ed with the alpha mask cumulatively: a pixel whose accumulated alpha
    was once at or below `depth_min_accu_alpha` stays out of the depth term for the rest of the loop (:1929-1931)."""
    from .image_losses import image_losses
    from .ssim import fused_ssim

    params = [p for g in opt.param_groups for p in g["params"] if p.requires_grad]
    depth_on = gt_depth is not None and lambda_depth > 0
    if depth_on and not depth_min >= 0:
        raise ValueError("refine_view: depth_min must be >= 0 (pixels that left the depth mask are marked by depth 0)")
    gt_win = gt_rgb[:, pixel_v_min:pixel_v_max, :]
    alive = None                    # pixels whose alpha stayed above the threshold in every earlier iteration
    losses = []
    pkg, done, converged = None, 0, False
    for _ in range(iters + 1):
        pkg = render_fn(camera)
        if pkg is None:
            break
        if not refine_on:
            break
        rgb = torch.clamp(pkg["render"], 0, 1)
        depth, alpha = pkg.get("surf_depth"), pkg.get("rend_alpha")
        use_depth = depth_on and depth is not None
        gtd = None
        if use_depth:
            gtd = gt_depth if alive is None else torch.where(alive, gt_depth, torch.zeros_like(gt_depth))
        L = image_losses(rgb, gt_rgb, depth if use_depth else None, gtd, alpha if use_depth else None,
                         pixel_v_min=pixel_v_min, pixel_v_max=pixel_v_max, depth_min=depth_min, depth_max=depth_max,
                         depth_min_accu_alpha=depth_min_accu_alpha)
        if lambda_ssim > 0.0:
            ssim_value = fused_ssim(rgb[:, pixel_v_min:pixel_v_max, :].unsqueeze(0), gt_win.unsqueeze(0))
            total = (1.0 - lambda_ssim) * L.rgb_l1 + lambda_ssim * (1.0 - ssim_value)
        else:
            total = L.rgb_l1
        if use_depth:
            total = total + L.depth_l1 * lambda_depth
            if alpha is not None:
                above = alpha.detach() > depth_min_accu_alpha
                alive = above if alive is None else alive & above
        losses.append(total.detach())
        grads = torch.autograd.grad(total, params, allow_unused=True)
        for p, g in zip(params, grads):
            p.grad = g
        with torch.no_grad():
            opt.step()
            flag = update_pose(camera, converged_threshold)
        _lib.note_sync("refine_converged")
        converged = bool(flag)
        for p in params:
            p.grad = None
        done += 1
        if converged:
            break
    dev = gt_rgb.device
    stacked = torch.stack(losses) if losses else torch.empty(0, dtype=torch.float32, device=dev)
    return RefineResult(pkg, done, converged, stacked)
