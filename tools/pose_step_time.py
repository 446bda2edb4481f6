"""Launches, host waits and wall time of a camera pose update and of one view-refinement iteration.

Per call, for
* `Camera.update_pose`        the torch restatement of utils/campose_utils.py:79-98 (pings_amd/camera.py), the path a
                              caller without `camera_ops.install` runs;
* `camera_ops.update_pose`    one launch of csrc/camera.hip;
* one `refine_view` iteration at 640x480 over neural points on `room_scene` (K Gaussians each, the decoders of
  bench.py's render step): render, L1 + depth L1, gradients of the optimiser's parameters, FusedAdamW, update_pose;
* the same iteration composed from `render` + the reference's loss expressions + `.backward()` +
  `torch.optim.AdamW` + `Camera.update_pose` (utils/mapper.py:1888-1948 as it runs without this module).

The two `update_pose` calls include the two 12-byte copies that set the deltas before each call (2 launches).
Wall time: median over --iters calls with a synchronise on both sides.  Host waits: what
`torch.cuda.set_sync_debug_mode("warn")` reports during one call plus the reads the package itself counts
(`_lib.sync_counts`).  Launches: device events of a torch.profiler pass in a process of its own (`--pass profile`),
because tracing slows the host.

    python tools/pose_step_time.py [--iters 30] [--points 40000] [--out profiles/camera/pose_step_time.json]
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
import warnings
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

W, H, FX, K = 640, 480, 600.0, 8
TAU = (0.004, -0.003, 0.005, 0.006, -0.004, 0.003)
DEPTH_KW = dict(depth_min=0.3, depth_max=50.0, depth_min_accu_alpha=0.4)
LAMBDA_DEPTH = 0.5


def build(points, dev):
    import bench
    from pings_amd import camera_ops
    from pings_amd.camera import Camera, se3_exp
    from pings_amd.optim import FusedAdamW
    from pings_amd.renderer import render
    from scenes import room_scene

    g = torch.Generator().manual_seed(8)
    pos, base_col, _, _, _ = room_scene(points, device=dev, seed=1)
    n = pos.shape[0]
    geo = (0.3 * torch.randn(n + 1, 32, generator=g)).to(dev).requires_grad_(True)
    cfe = (0.3 * torch.randn(n + 1, 16, generator=g)).to(dev).requires_grad_(True)
    D = bench._BenchDecoder
    decs = {"gauss_xyz": D(32, 128, 3, K, g, dev), "gauss_rot": D(32, 128, 4, K, g, dev),
            "gauss_scale": D(32, 128, 3, K, g, dev), "gauss_alpha": D(32, 128, 1, K, g, dev),
            "gauss_color": D(16 + 3, 128, 3, K, g, dev)}
    data = {"position": pos, "orientation": torch.tensor([1.0, 0, 0, 0], device=dev).repeat(n, 1), "color": base_col,
            "geo_feature": geo, "color_feature": cfe, "resolution": 0.2,
            "free_mask": torch.zeros(n, dtype=torch.bool, device=dev),
            "valid_mask": torch.ones(n, dtype=torch.bool, device=dev)}
    bg = torch.ones(3, device=dev)
    net = [geo, cfe] + [p for d in decs.values() for p in d.parameters()]
    rfn = lambda c: render(c, None, data, decs, None, bg, view_concat_on=True, learn_color_residual=True)
    true_pose = torch.eye(4, dtype=torch.float64)
    start = torch.linalg.inv(se3_exp(torch.tensor(TAU, dtype=torch.float64) * 5))
    mk = lambda: Camera(W, H, FX, FX, W / 2 - 0.5, H / 2 - 0.5, 0.05, 60.0, start.clone(), device=dev)
    with torch.no_grad():
        gt = rfn(Camera(W, H, FX, FX, W / 2 - 0.5, H / 2 - 0.5, 0.05, 60.0, true_pose, device=dev))
    gt_rgb, gt_depth = gt["render"].clamp(0, 1).clone(), gt["surf_depth"].clone()
    groups = lambda c: [{"params": [c.exposure_mat], "lr": 1e-3}, {"params": [c.exposure_offset], "lr": 1e-3},
                        {"params": [c.cam_rot_delta], "lr": 3e-3}, {"params": [c.cam_trans_delta], "lr": 1e-3}]
    tau = torch.tensor(TAU, device=dev)

    cam_t, cam_k = mk(), mk()

    def torch_update():
        cam_t.cam_trans_delta.data.copy_(tau[:3])
        cam_t.cam_rot_delta.data.copy_(tau[3:])
        cam_t.update_pose()

    def kernel_update():
        cam_k.cam_trans_delta.data.copy_(tau[:3])
        cam_k.cam_rot_delta.data.copy_(tau[3:])
        camera_ops.update_pose(cam_k)

    cam_a, cam_b = mk(), mk()
    opt_a = FusedAdamW(groups(cam_a), betas=(0.9, 0.99), eps=1e-15)
    opt_b = torch.optim.AdamW(groups(cam_b), betas=(0.9, 0.99), eps=1e-15)

    def refine_new():
        camera_ops.refine_view(cam_a, rfn, gt_rgb, opt_a, gt_depth=gt_depth, iters=0, lambda_depth=LAMBDA_DEPTH,
                               **DEPTH_KW)

    def refine_composed():
        pkg = rfn(cam_b)
        rgb = torch.clamp(pkg["render"], 0, 1)[:, 0:-1, :]
        loss = torch.abs(rgb - gt_rgb[:, 0:-1, :]).mean()
        valid = (gt_depth > DEPTH_KW["depth_min"]) & (gt_depth < DEPTH_KW["depth_max"]) & \
            (pkg["rend_alpha"].detach() > DEPTH_KW["depth_min_accu_alpha"])
        loss = loss + torch.abs(gt_depth[valid] - pkg["surf_depth"][valid]).mean() * LAMBDA_DEPTH
        loss.backward(retain_graph=True)
        with torch.no_grad():
            opt_b.step()
            cam_b.update_pose()
        opt_b.zero_grad(set_to_none=True)
        for p in net:
            p.grad = None

    def reset():
        for c in (cam_a, cam_b):
            c.set_pose(start.clone())

    return {"Camera.update_pose": torch_update, "camera_ops.update_pose": kernel_update,
            "refine_view_iteration": refine_new, "composed_iteration": refine_composed}, reset


def time_calls(fn, reset, iters):
    for _ in range(3):
        reset()
        fn()
    wall = []
    for _ in range(iters):
        reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    return {"wall_ms_median": round(statistics.median(wall), 4), "wall_ms_min": round(min(wall), 4)}


def host_waits(fn, reset):
    from pings_amd import _lib

    reset()
    torch.cuda.synchronize()
    _lib.sync_counts(reset=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    own = _lib.sync_counts(reset=True)
    seen = sum("synchroniz" in str(x.message).lower() for x in w)
    # the converged flag is read through torch (`bool(flag)`), so torch reports it too: count it once.  The rasteriser's
    # instance count is read by polling mapped host memory, which torch does not see.
    return {"torch_reported": seen, "package_counted": own,
            "total": seen + sum(v for k, v in own.items() if k != "refine_converged")}


def launches(fn, reset, calls=5):
    from torch.profiler import ProfilerActivity, profile

    for _ in range(3):
        reset()
        fn()
    reset()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
           and not e.name.startswith("Optimizer.step#")]
    return {"launches_per_call": len(evs) / calls,
            "device_ms_per_call": round(sum(e.device_time for e in evs) / 1e3 / calls, 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--points", type=int, default=40_000)
    ap.add_argument("--pass", dest="mode", choices=("all", "time", "profile"), default="all")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_step_time.py measures on a HIP device; none is available")
    fns, reset = build(a.points, "cuda")
    if a.mode == "profile":
        print("PROFILE_JSON " + json.dumps({k: launches(f, reset) for k, f in fns.items()}))
        return
    res = {"device": torch.cuda.get_device_name(0), "image": [W, H], "neural_points": a.points, "K": K,
           "iters": a.iters, "delta_copy_launches_in_update_calls": 2, "calls": {}}
    for k, f in fns.items():
        res["calls"][k] = {**time_calls(f, reset, a.iters), "host_waits": host_waits(f, reset)}
        print(k, json.dumps(res["calls"][k]), flush=True)
    if a.mode == "all":
        torch.cuda.synchronize()
        r = subprocess.run([sys.executable, __file__, "--pass", "profile", "--points", str(a.points)],
                           capture_output=True, text=True, timeout=300)
        line = [x for x in r.stdout.splitlines() if x.startswith("PROFILE_JSON ")]
        if line:
            for k, v in json.loads(line[0][len("PROFILE_JSON "):]).items():
                res["calls"][k].update(v)
        else:
            res["profile_error"] = (r.stderr or r.stdout)[-2000:]
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
