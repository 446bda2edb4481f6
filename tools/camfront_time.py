"""Wall time, launches and host waits of the camera frame front-end against a restatement of the reference's lines.

  image_pyramid_<n>cam_<W>x<H>   `camfront_ops.image_pyramids` (RGB from the loader's uint8 image, depth, sky mask, normal)
                                 for 1, 2 and 4 cameras at 1920 x 1080 and at 1392 x 512, against the float / permute /
                                 divide / clamp chain and the twelve `F.interpolate` calls per camera of
                                 `CamImage.__init__` (gaussian_splatting/utils/cameras.py:39, :116-182) in torch on the device
  mono_frame_1392x512            `camfront_ops.mono_frame`, one camera, against dataset/slam_dataset.py:366-399 and
                                 :432-437 as the reference runs them: two images copied to the host, `np.polyfit`, the
                                 numpy gates, the sky mask uploaded again
  process_frame_mono             the mono-depth branch of `pool_ops.process_frame` (`pool_ops._mono_update`) against
                                 utils/mapper.py:297-331 in float32 torch on the device, `voxel_down_sample_torch`
                                 (utils/tools.py:924-967) included

The baselines are the reference's arithmetic, never the code under test.  Open3D is not installed, so its two steps of
the mono-depth block (`create_from_rgbd_image`, `voxel_down_sample`, :438-453) and the float64 round trip behind them
(:472-477) CANNOT be timed: the baseline of `mono_frame` stops at the gated depth image, which favours the baseline, and
the JSON says so.

Wall time: the two versions alternate inside one loop after a warm-up, fresh inputs and a synchronise on both sides of
every call; median and minimum over --iters calls.  Host waits and launches: the helpers of tools/pose_step_time.py,
taken after the timing.  No time is a gate.

    python tools/camfront_time.py [--iters 20] [--out profiles/camfront/camfront_time.json]
"""
import argparse
import json
import sys
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

OPEN3D_NOTE = ("open3d is not installed: create_from_rgbd_image and voxel_down_sample (slam_dataset.py:438-453) and the "
               "float64 round trip (:472-477) are missing from the mono_frame baseline, which stops at the gated depth")


# ---------------------------------------------------------------- restatements of the reference's lines
def torch_cam_lists(u8, depth, sky, normal):
    """cameras.py:39, :116-182, with the loader's `torch.tensor(img).float() / 255` and permute in front."""
    rgb = (u8.float() / 255.0).permute(2, 0, 1).clamp(0.0, 1.0)
    half = lambda x, mode, **kw: F.interpolate(x.unsqueeze(0), scale_factor=0.5, mode=mode, **kw).squeeze(0)  # noqa: E731
    lists = [[rgb], [depth], [sky], [normal]]
    for _ in range(3):
        lists[0].append(half(lists[0][-1], "bilinear", align_corners=False))
        lists[1].append(half(lists[1][-1], "nearest-exact"))
        lists[2].append(half(lists[2][-1].float(), "nearest").bool())
        lists[3].append(half(lists[3][-1], "bilinear", align_corners=False))
    return lists


def numpy_mono_block(pred, lidar, cfg, high_z, dev):
    """slam_dataset.py:366-399, :432-437 for one camera, without the Open3D steps."""
    pred_np = pred.permute(1, 2, 0).squeeze(-1).detach().cpu().numpy()
    lidar_np = lidar.permute(1, 2, 0).squeeze(-1).detach().cpu().numpy()
    valid = (lidar_np > cfg.min_range) & (pred_np > cfg.min_range) & (lidar_np < cfg.max_range * 0.8)
    meas, with_gt = lidar_np[valid], pred_np[valid]
    rmse_before = np.sqrt(np.mean((with_gt - meas) ** 2))
    if meas.shape[0] > 100:
        (k, b), residuals, _, _, _ = np.polyfit(with_gt, meas, 1, full=True)
        rmse_after = np.sqrt(residuals[0] / meas.shape[0])
        pred_np = k * pred_np + b
    sky_np = pred_np > cfg.max_range * 1.2
    pred_np[sky_np] = 0.0
    sky = torch.tensor(sky_np, dtype=torch.bool, device=dev).unsqueeze(0)
    if high_z:
        pred_np[pred_np > 0.8 * cfg.max_range] = 0.0
        pred_np[pred_np < 2.0 * cfg.min_range] = 0.0
    else:
        pred_np[pred_np < 0.2 * cfg.max_range] = 0.0
    return sky, pred_np


def torch_voxel_down_sample(points, voxel_size):
    """utils/tools.py:924-967 in float32 torch on the points' device."""
    q = 1000
    offset = torch.floor(points.min(dim=0)[0] / voxel_size).long()
    grid = torch.floor(points / voxel_size)
    center = (grid + 0.5) * voxel_size
    dist = ((points - center) ** 2).sum(dim=1) ** 0.5
    dist = (dist / dist.max() * (q - 1)).long()
    grid = grid.long() - offset
    v_size = grid.max()
    grid_idx = grid[:, 0] + grid[:, 1] * v_size + grid[:, 2] * v_size * v_size
    unique, inverse = torch.unique(grid_idx, return_inverse=True)
    idx_d = torch.arange(inverse.size(0), dtype=inverse.dtype, device=points.device)
    off = 10 ** len(str(idx_d.max().item()))
    idx_d = idx_d + dist * off
    idx = torch.empty(unique.shape, dtype=inverse.dtype, device=points.device).scatter_reduce_(
        0, inverse, idx_d, reduce="amin", include_self=False)
    return idx % off


def torch_mono_update(mono, update_points, pose, cfg, high_z, sink):
    """utils/mapper.py:297-331 without normals."""
    homo = torch.cat([mono[:, :3], torch.ones(mono.shape[0], 1).to(mono)], dim=1)
    mono[:, :3] = torch.matmul(homo, pose.to(mono).T)[:, :3]
    if high_z:
        used = mono[:, 2] > torch.quantile(update_points[:, 2], 0.98) + cfg.voxel_size_m
    else:
        used = mono[:, 2] < torch.quantile(update_points[:, 2], 0.2) + cfg.voxel_size_m
    mono = mono[used]
    if mono.shape[0] > 0:
        mono = mono[torch_voxel_down_sample(mono[:, :3], cfg.monodepth_gaussian_res)]
    if mono.shape[0] > 0:
        sink(mono[:, :3], mono[:, 3:])


# ---------------------------------------------------------------- workload
def build(dev):
    import camfront_ref as CR
    from pings_amd import camfront_ops, pool_ops

    rng = np.random.default_rng(0)
    state, calls = {}, {}

    def camera(H, W, seed):
        r = np.random.default_rng(seed)
        u8 = torch.from_numpy(r.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
        depth = torch.from_numpy(r.uniform(0.0, 80.0, (1, H, W)).astype(np.float32)).to(dev)
        sky = torch.from_numpy(r.random((1, H, W)) < 0.3).to(dev)
        normal = F.normalize(torch.from_numpy(r.normal(size=(3, H, W)).astype(np.float32)).to(dev), dim=0)
        return u8, depth, sky, normal

    for W, H in ((1920, 1080), (1392, 512)):
        cams = [camera(H, W, s) for s in range(4)]
        for n in (1, 2, 4):
            calls[f"image_pyramid_{n}cam_{W}x{H}"] = (
                (lambda: None, lambda c=cams[:n]: camfront_ops.image_pyramids(c)),
                (lambda: None, lambda c=cams[:n]: [torch_cam_lists(*x) for x in c]))

    # mono_frame: one camera at 1392 x 512, LiDAR depth on a fifth of the pixels
    H, W = 512, 1392
    pred = torch.from_numpy(rng.uniform(1.0, 90.0, (1, H, W)).astype(np.float32)).to(dev)
    lidar = 1.07 * pred - 0.6 + 0.5 * torch.randn(1, H, W, device=dev)
    lidar[torch.rand(1, H, W, device=dev) > 0.2] = 0.0
    u8 = camera(H, W, 9)[0]
    K = np.array([[720.0, 0.0, 0.5 * W], [0.0, 720.0, 0.5 * H], [0.0, 0.0, 1.0]])
    ds = CR.Dataset([("cam0", K, CR.rig_pose(1))], min_range=2.75, max_range=60.0, local_map_radius=50.0, vox_down_m=0.08)
    calls["mono_frame_1392x512"] = (
        (lambda: None, lambda: camfront_ops.mono_frame(ds, {"cam0": u8}, {"cam0": pred}, {"cam0": lidar})),
        (lambda: None, lambda: numpy_mono_block(pred, lidar, ds.config, False, dev)))

    # the mono branch of process_frame: 400,000 mono rows against 40,000 update points
    cfg = NS(voxel_size_m=0.3, monodepth_gaussian_res=0.2)
    base = torch.cat([torch.rand(400_000, 3, device=dev) * torch.tensor([80.0, 80.0, 8.0], device=dev)
                      - torch.tensor([40.0, 40.0, 2.0], device=dev), torch.rand(400_000, 3, device=dev)], dim=1)
    update_points = torch.rand(40_000, 3, device=dev) * 6.0 - 1.0
    pose = torch.as_tensor(CR.rig_pose(2), dtype=torch.float64).to(dev)
    me = NS(config=cfg, dataset=NS(loader=NS(mono_depth_for_high_z=False)),
            neural_points=NS(update=lambda *a, **k: None))

    def prep():
        state["mono"] = base.clone()

    calls["process_frame_mono"] = (
        (prep, lambda: pool_ops._mono_update(me, state["mono"], update_points, pose, 0)),
        (prep, lambda: torch_mono_update(state["mono"], update_points, pose, cfg, False, lambda *a: None)))
    shape = {"image_pyramid": {"sizes": [[1920, 1080], [1392, 512]], "cameras": [1, 2, 4],
                               "maps": ["rgb uint8", "depth", "sky_mask", "normal"]},
             "mono_frame": {"image": [W, H], "cameras": 1, "lidar_share": 0.2, "vox_down_m": 0.08},
             "process_frame_mono": {"mono_rows": 400_000, "update_points": 40_000, "monodepth_gaussian_res": 0.2}}
    return calls, shape


def main():
    from frame_pool_time import time_pair
    from pose_step_time import host_waits, launches

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("camfront_time.py measures on a HIP device; none is available")
    calls, shape = build("cuda")
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "shape": shape, "not_timed": OPEN3D_NOTE,
           "baseline": "float32 torch + numpy restatement of the reference's lines, same process", "calls": {}}
    host_waits(lambda: torch.zeros(1, device="cuda").item(), lambda: None)     # spends torch's once-per-process warning
    for name, (ours, theirs) in calls.items():
        t_ours, t_theirs = time_pair(ours, theirs, a.iters)
        res["calls"][name] = {"camfront_ops": {**t_ours, "host_waits": host_waits(ours[1], ours[0])},
                              "reference_lines": {**t_theirs, "host_waits": host_waits(theirs[1], theirs[0])}}
    for name, (ours, theirs) in calls.items():
        for key, (prep, fn) in (("camfront_ops", ours), ("reference_lines", theirs)):
            res["calls"][name][key].update(launches(fn, prep, calls=1))         # one traced call on fresh inputs
        print(name, json.dumps(res["calls"][name]), flush=True)
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
