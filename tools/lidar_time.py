"""Wall time, launches and host waits of the LiDAR frame front-end against its torch restatement.

For `lidar_ops.deskew`, `lidar_ops.project_to_cams` (1, 2 and 4 cameras of 1392 x 512, with compaction) and
`crop_rows` + `select_rows` (the crop branch of `filter_and_correct`), each next to a float32 torch restatement of the
reference's lines run on the device in the same process (dataset/slam_dataset.py:584-621, :803-856;
utils/tools.py:1088-1163, :1242-1351; gaussian_splatting/utils/cameras.py:233-243).  The reference interpolates the
rotation with `roma.rotmat_slerp`; the restatement forms axis and angle with torch operators and builds the same
[N,3,3] tensor.  Shapes: 120,000 points, six columns, time stamps, normals and two label tensors as companions.

Wall time: the two versions alternate inside one loop after a warm-up, fresh inputs and a synchronise on both sides of
every call; median and minimum over --iters calls.  Host waits and launches: the helpers of tools/pose_step_time.py,
taken after the timing because tracing slows the host.  No time is a gate.

    python tools/lidar_time.py [--iters 20] [--points 120000] [--out profiles/lidar/lidar_time.json]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))


# ---------------------------------------------------------------- torch restatement (float32, on the device)
def torch_crop_select(ds):
    cfg, p = ds.config, ds.cur_point_cloud_torch
    dist = torch.norm(p[:, :2], dim=1)
    keep = (dist > cfg.min_range) & (dist < ds.crop_max_range) & (p[:, 2] > cfg.min_z) & (p[:, 2] < cfg.max_z)
    ds.cur_point_cloud_torch = p[keep]
    ds.cur_point_ts_torch = ds.cur_point_ts_torch[keep]
    ds.cur_point_lidar_idx_torch = ds.cur_point_lidar_idx_torch[keep]


def torch_deskew(points, ts, pose, ts_ref_pose=0.5):
    ts = ts.squeeze(-1)
    ts = (ts - torch.min(ts)) / (torch.max(ts) - torch.min(ts))
    ts = ts - ts_ref_pose
    R = pose[:3, :3].to(points)
    w = torch.stack([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sin_t = 0.5 * torch.linalg.norm(w)
    theta = torch.atan2(sin_t, 0.5 * (torch.trace(R) - 1.0))
    axis = w / (2.0 * sin_t).clamp_min(1e-30)
    Kx = torch.zeros(3, 3, device=points.device)
    Kx[0, 1], Kx[0, 2], Kx[1, 0], Kx[1, 2], Kx[2, 0], Kx[2, 1] = -axis[2], axis[1], axis[2], -axis[0], -axis[1], axis[0]
    ang = (ts * theta)[:, None, None]
    rot = torch.eye(3, device=points.device) + torch.sin(ang) * Kx + (1.0 - torch.cos(ang)) * (Kx @ Kx)   # [N,3,3]
    tran = ts[:, None] * pose[:3, 3].to(points)
    points[:, :3] = (rot @ points[:, :3].unsqueeze(-1)).squeeze(-1) + tran
    return points


def torch_project_points_to_cam(points, rgb, img, T_c_l, K, min_depth, max_depth=100.0):
    homo = torch.cat([points[:, :3], torch.ones(points.shape[0], 1).to(points)], dim=1)
    cam = torch.matmul(homo, T_c_l.T)[:, :3]
    proj = torch.matmul(K[:3, :3].reshape(1, 3, 3), cam.T)
    depth = proj[:, 2, :]
    depth[depth == 0] = -1e-6
    u = torch.round(proj[:, 0, :] / torch.abs(depth))[0].to(torch.int64)
    v = torch.round(proj[:, 1, :] / torch.abs(depth))[0].to(torch.int64)
    depth = depth[0]
    _, H, W = img.shape
    depth_map = torch.zeros((1, H, W)).to(img)
    count = torch.zeros((H, W), dtype=torch.int, device=points.device)
    mask = (u >= 0) & (u < W) & (v >= 0) & (v < H) & (depth > min_depth) & (depth < max_depth)
    vv, uu, dd = v[mask], u[mask], depth[mask]
    idx = vv * W + uu
    depth_map.view(-1).scatter_reduce_(0, idx, dd, reduce="amin", include_self=False)
    count.view(-1).scatter_reduce_(0, idx, torch.ones_like(dd, dtype=torch.int), reduce="sum")
    colour = torch.transpose(img[:, vv, uu], 0, 1)
    rgb[mask] = torch.cat((colour, torch.zeros((dd.shape[0], 1)).to(dd)), dim=-1)
    return rgb, depth_map


def torch_set_depth_img(cam, depth):
    cam.depth_on = True
    l1 = F.interpolate(depth.unsqueeze(0), scale_factor=0.5, mode="nearest-exact").squeeze(0)
    l2 = F.interpolate(l1.unsqueeze(0), scale_factor=0.5, mode="nearest-exact").squeeze(0)
    l3 = F.interpolate(l2.unsqueeze(0), scale_factor=0.5, mode="nearest-exact").squeeze(0)
    cam.depth_image_list[0:4] = [depth, l1, l2, l3]


def torch_project_to_cams(ds, only=True):
    cloud = ds.cur_point_cloud_torch
    rgb = -1.0 * torch.ones((cloud.shape[0], 4)).to(cloud)
    for name, cam in ds.cur_cam_img.items():
        if cam is None:
            continue
        T = torch.tensor(ds.T_c_l_mats[name], device=ds.device, dtype=ds.dtype)
        K = torch.tensor(ds.K_mats[name], device=ds.device, dtype=ds.dtype)
        rgb, depth = torch_project_points_to_cam(cloud, rgb, cam.rgb_image_list[0], T, K, ds.config.min_range)
        torch_set_depth_img(cam, depth)
    cloud[:, 3:] = rgb[:, :3]
    if only:
        keep = rgb[:, 3] == 0
        ds.cur_point_cloud_torch = cloud[keep]
        ds.cur_point_ts_torch = ds.cur_point_ts_torch[keep]
        ds.cur_point_normals = ds.cur_point_normals[keep]
        ds.cur_sem_labels_torch = ds.cur_sem_labels_torch[keep]
        ds.cur_sem_labels_full = ds.cur_sem_labels_full[keep]


# ---------------------------------------------------------------- workload
def build(points, dev):
    import lidar_ref as LR
    from pings_amd import lidar_ops

    H, W = 512, 1392
    sc = LR.scene(points, H, W, seed=1, ncam=4)
    state = {}

    def fresh(ncam):
        def prep():
            ds = LR.Dataset(sc, device=dev, cams=sc.names[:ncam], set_depth_img=lidar_ops.set_depth_img)
            if "mats" in state:
                ds._pings_cam_mats = state["mats"].get(ncam)                  # a dataset lives across frames
            ds.cur_point_lidar_idx_torch = torch.zeros(points, dtype=torch.int64, device=dev)
            state["ds"] = ds
        return prep

    pose = torch.as_tensor(LR.look_along_x(0.02, 0.01, (0.9, 0.05, 0.0)) @ np.linalg.inv(LR.look_along_x()),
                           dtype=torch.float32).to(dev)
    ts = torch.rand(points, device=dev)
    base = torch.as_tensor(sc.cloud).to(dev)

    def prep_cloud():
        state["cloud"] = base.clone()

    def ours_crop():
        ds = state["ds"]
        ds.cur_sem_labels_torch = None
        lidar_ops.filter_and_correct(ds)

    calls = {
        "deskew": ((prep_cloud, lambda: lidar_ops.deskew(state["cloud"], ts, pose)),
                   (prep_cloud, lambda: torch_deskew(state["cloud"], ts, pose))),
        "crop_select": ((fresh(1), ours_crop), (fresh(1), lambda: torch_crop_select(state["ds"]))),
    }
    state["mats"] = {}

    def ours_project(ncam):
        def run():
            lidar_ops.project_to_cams(state["ds"], True)
            state["mats"][ncam] = state["ds"]._pings_cam_mats
        return run

    for ncam in (1, 2, 4):
        calls[f"project_to_cams_{ncam}"] = ((fresh(ncam), ours_project(ncam)),
                                            (fresh(ncam), lambda: torch_project_to_cams(state["ds"], True)))
    return calls, {"points": points, "image": [H, W], "cameras": [1, 2, 4]}


def main():
    from frame_pool_time import time_pair
    from pose_step_time import host_waits, launches

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--points", type=int, default=120_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lidar_time.py measures on a HIP device; none is available")
    calls, shape = build(a.points, "cuda")
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "shape": shape, "calls": {}}
    # torch adds a once-per-process warning about the sync debug mode itself to the first report: spend it here
    host_waits(lambda: torch.zeros(1, device="cuda").item(), lambda: None)
    for name, (ours, theirs) in calls.items():
        t_ours, t_theirs = time_pair(ours, theirs, a.iters)
        res["calls"][name] = {"lidar_ops": {**t_ours, "host_waits": host_waits(ours[1], ours[0])},
                              "torch": {**t_theirs, "host_waits": host_waits(theirs[1], theirs[0])}}
        print(name, json.dumps(res["calls"][name]), flush=True)
    for name, (ours, theirs) in calls.items():
        for key, (prep, fn) in (("lidar_ops", ours), ("torch", theirs)):
            res["calls"][name][key].update(launches(fn, prep, calls=1))      # one traced call on fresh inputs
        print(name, json.dumps(res["calls"][name]), flush=True)
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
