"""The LiDAR frame front-end on the HIP device (csrc/lidar.hip).

What turns a raw scan and the frame's camera images into what the mapper trains on, on the reference's own tensors; no
state lives here:

  `crop_rows`, `select_rows`      `crop_frame` as one mask launch; boolean-mask indexing of every companion tensor with
                                  ONE host read (the count) and one gather launch
  `deskew`                        `deskewing` (utils/tools.py:1088-1163), in place, two launches, no read
  `slerp_pose`                    `slerp_pose` (:1165-1177), one 64-lane launch, no read
  `project_points_to_cam`         `project_points_to_cam_torch` (:1242-1327) for one camera
  `project_to_cams`               `SLAMDataset.project_pointcloud_to_cams` (dataset/slam_dataset.py:803-856): one projection
                                  launch for all cameras, one launch for every depth pyramid, one read for the compaction
  `depth_pyramid`                 the arithmetic of `CamImage.set_depth_img` (gaussian_splatting/utils/cameras.py:233-243)

`install` rebinds the module-level names and the methods and keeps the originals, which are called for the inputs the
kernels do not take (CPU tensors, other dtypes, more than 8 cameras or 8 other LiDARs, images smaller than 8 pixels).
There is no torch path of this module's own: with no original kept, such a call raises.
"""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np
import torch

from . import _abi, _lib, neural_map
from .pool_ops import _entry, _guard, _rebind, _restore

MAX_CAMS, MAX_LIDARS = _abi.LIDAR_MAX_CAMS, _abi.LIDAR_MAX_LIDARS

_kept: dict = {}               # module-level names of the reference kept by `install`


def _kept_original(name: str):
    orig = _kept.get(name)
    if orig is None:
        raise _lib.PingsHipError(f"lidar_ops.{name}: these inputs take the reference's own function, and none was kept "
                                 "(`lidar_ops.install` keeps it); the HIP path needs float32 device tensors")
    return orig


def _original(self, name: str):
    orig = getattr(type(self), f"_pings_{name}_original", None)
    if orig is None:
        raise _lib.PingsHipError(f"lidar_ops.{name}: these inputs take the reference's own method, and none was kept "
                                 "(`lidar_ops.install` keeps it); the HIP path needs float32 device tensors")
    return orig


def _cloud_ok(t, cols_at_least: int = 3, dev=None) -> bool:
    """float32 [N,C] on the device, C >= 3, unit stride along a row (a row-strided view is fine)."""
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype is torch.float32 and t.dim() == 2
            and int(t.shape[1]) >= cols_at_least and t.stride(1) == 1 and (int(t.shape[0]) < 2 or t.stride(0) >= 3)
            and (dev is None or t.device == dev))


def _row_stride(t) -> int:
    return int(t.stride(0)) if int(t.shape[0]) > 1 else max(int(t.stride(0)), int(t.shape[1]))


def _mat_dev(t, dev=None) -> bool:
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in (torch.float32, torch.float64)
            and tuple(t.shape) == (4, 4) and (dev is None or t.device == dev))


def _image_ok(t, dev) -> bool:
    return (isinstance(t, torch.Tensor) and t.device == dev and t.dtype is torch.float32 and t.dim() == 3
            and int(t.shape[0]) == 3 and int(t.shape[1]) >= 8 and int(t.shape[2]) >= 8 and t.is_contiguous())


# ---------------------------------------------------------------- crop and compaction
@torch.no_grad()
def crop_rows(points: torch.Tensor, min_z, max_z, min_range, max_range, on_xy_plane: bool) -> torch.Tensor:
    """`crop_frame` (dataset/slam_dataset.py:1626-1645): the bool mask of the rows with min_range < dist < max_range and
    min_z < z < max_z, every comparison strict, dist over x, y (`on_xy_plane`) or x, y, z.  A NaN row is dropped.  One
    launch, no host read."""
    if not _cloud_ok(points):
        raise _lib.PingsHipError("lidar_ops.crop_rows: points must be a float32 [N,C>=3] device tensor with unit stride "
                                 "along a row")
    n, dev = int(points.shape[0]), points.device
    mask = torch.empty(n, dtype=torch.bool, device=dev)
    if n:
        with _guard(dev):
            _lib.check(_entry("pings_lidar_crop")(points.data_ptr(), n, _row_stride(points), float(min_z), float(max_z),
                                                  float(min_range), float(max_range), int(bool(on_xy_plane)),
                                                  mask.view(torch.uint8).data_ptr(), _lib.stream_ptr(dev)),
                       "pings_lidar_crop")
    return mask


@torch.no_grad()
def select_rows(mask_or_rows: torch.Tensor, *tensors):
    """`t[mask]` for every companion `t` (any dtype, any trailing shape; `None` stays `None`), kept rows in order.  A
    bool / uint8 mask is turned into its ascending rows by `pings_mask_rows`, whose count is the call's single host
    read; an int64 row list (every entry inside the companions) is used as it is, with no read.  All companions are
    gathered by one `pings_gather_rows_multi` launch (one per 16 of them)."""
    m = mask_or_rows
    if not (isinstance(m, torch.Tensor) and m.is_cuda and m.dim() == 1):
        raise _lib.PingsHipError("lidar_ops.select_rows: the mask or row list must be a 1-D device tensor")
    L = _lib.lib()
    live = [(j, t) for j, t in enumerate(tensors) if t is not None]
    for _, t in live:
        if not (isinstance(t, torch.Tensor) and t.device == m.device and t.dim() >= 1):
            raise _lib.PingsHipError(f"lidar_ops.select_rows: every companion must be a tensor on {m.device}")
    with _guard(m.device):
        if m.dtype in (torch.bool, torch.uint8):
            for _, t in live:
                if int(t.shape[0]) != int(m.shape[0]):
                    raise _lib.PingsHipError(f"lidar_ops.select_rows: a companion has {int(t.shape[0])} rows, the mask "
                                             f"{int(m.shape[0])}")
            rows, k, _ = neural_map._mask_rows(L, m)
        elif m.dtype is torch.int64:
            rows, k = m.contiguous(), int(m.shape[0])
        else:
            raise _lib.PingsHipError("lidar_ops.select_rows: a bool / uint8 mask or int64 rows")
        outs = [None] * len(tensors)
        wide = [(j, t) for j, t in live if t.numel() > 0 and k > 0]
        for j, t in live:
            if not (t.numel() > 0 and k > 0):
                outs[j] = t.new_empty((k,) + tuple(t.shape[1:]))
        for head in range(0, len(wide), 16):
            part = wide[head:head + 16]
            for (j, _), o in zip(part, neural_map._gather_many(L, [(t, k) for _, t in part], rows)):
                outs[j] = o
    return tuple(outs)


# ---------------------------------------------------------------- deskewing
def _pose_dev(pose, dev):
    """A [4,4] float32 / float64 contiguous tensor on `dev` from what the caller holds."""
    if not isinstance(pose, torch.Tensor):
        pose = torch.as_tensor(np.asarray(pose))
    if pose.dtype not in (torch.float32, torch.float64):
        pose = pose.to(torch.float64)
    return pose.detach().to(dev).contiguous()


@torch.no_grad()
def deskew(points, ts, pose, ts_ref_pose=0.5, points_lidar_idx=None, T_l_lm_list=None, ts_diff_list=None):
    """`deskewing` (utils/tools.py:1088-1163), in place on the first three columns of `points` (float32 [N,C>=3], a
    row-strided view is fine); returns `points` itself.  s_i = (ts_i - min) / (max - min) - ts_ref_pose in float64,
    rounded to float32; a point becomes R(s_i) p_i + s_i t with R(s) the rotation by s times the angle of `pose`'s
    rotation about its axis.  With `T_l_lm_list` and `points_lidar_idx` both given the rows of LiDAR k >= 1 are
    deskewed in that LiDAR's own frame (pose_k = T pose T^-1, time shifted by `ts_diff_list[k-1]`), rows of an index the
    list does not name stay as they are, and an empty list returns `points` unchanged, as the reference does.  Two
    launches, no host read, no `nonzero`, no [N,3,3] tensor; bitwise reproducible.  `ts is None` returns at once; N = 0
    raises before any launch (the reference's `torch.min` raises there)."""
    if ts is None:
        return points
    multi = T_l_lm_list is not None and points_lidar_idx is not None
    if multi and len(T_l_lm_list) == 0:
        return points
    ok = (_cloud_ok(points) and isinstance(ts, torch.Tensor) and ts.device == points.device
          and ts.dtype in (torch.float32, torch.float64)
          and (ts.dim() == 1 or (ts.dim() == 2 and int(ts.shape[1]) == 1)) and int(ts.shape[0]) == int(points.shape[0])
          and isinstance(pose, torch.Tensor) and tuple(pose.shape) == (4, 4))
    T = diff = None
    if ok and multi:
        T = np.ascontiguousarray(np.stack([np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t,
                                                      dtype=np.float64) for t in T_l_lm_list]))
        ok = (T.shape == (len(T_l_lm_list), 4, 4) and len(T_l_lm_list) <= MAX_LIDARS
              and bool(np.all(T[:, 3] == np.array([0.0, 0.0, 0.0, 1.0])))
              and isinstance(points_lidar_idx, torch.Tensor) and points_lidar_idx.device == points.device
              and not points_lidar_idx.is_floating_point() and points_lidar_idx.numel() == int(points.shape[0]))
        if ok and ts_diff_list is not None:
            diff = np.ascontiguousarray(np.asarray([float(d) for d in ts_diff_list], dtype=np.float64))
            ok = diff.shape[0] >= len(T_l_lm_list)
    if not ok:
        return _kept_original("deskewing")(points, ts, pose, ts_ref_pose, points_lidar_idx, T_l_lm_list, ts_diff_list)
    n, dev = int(points.shape[0]), points.device
    if n == 0:
        raise _lib.PingsHipError("lidar_ops.deskew: an empty scan has no first and last time stamp")
    with _guard(dev):
        tsc = ts.detach().reshape(-1).contiguous()
        posec = _pose_dev(pose, dev)
        lidx = None
        if multi:
            lidx = points_lidar_idx.detach().reshape(-1)
            if lidx.dtype not in (torch.int32, torch.int64):
                lidx = lidx.to(torch.int64)
            lidx = lidx.contiguous()
        scratch = torch.empty(_entry("pings_lidar_deskew_scratch_bytes")(), dtype=torch.uint8, device=dev)
        as_f64 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
        _lib.check(_entry("pings_lidar_deskew")(
            points.data_ptr(), n, _row_stride(points), tsc.data_ptr(), int(tsc.dtype is torch.float64),
            posec.data_ptr(), int(posec.dtype is torch.float64), float(ts_ref_pose),
            None if lidx is None else lidx.data_ptr(), int(lidx is not None and lidx.dtype is torch.int64),
            0 if T is None else int(T.shape[0]), as_f64(T), as_f64(diff), scratch.data_ptr(), _lib.stream_ptr(dev)),
            "pings_lidar_deskew")
    return points


def _slerp(pose: torch.Tensor, s: float, out: torch.Tensor, left: torch.Tensor = None, invert: bool = False) -> None:
    dev = pose.device
    _lib.check(_entry("pings_lidar_slerp_pose")(
        pose.data_ptr(), int(pose.dtype is torch.float64), float(s), None if left is None else left.data_ptr(),
        int(left is not None and left.dtype is torch.float64), int(bool(invert)), out.data_ptr(),
        int(out.dtype is torch.float64), _lib.stream_ptr(dev)), "pings_lidar_slerp_pose")


@torch.no_grad()
def slerp_pose(relative_pose: torch.Tensor, ts: float, ts_ref_pose: float) -> torch.Tensor:
    """`slerp_pose` (utils/tools.py:1165-1177): the [4,4] transform with rotation R(ts - ts_ref_pose) and translation
    (ts - ts_ref_pose) t, of `relative_pose`'s dtype on its device.  float64 arithmetic rounded once; one 64-lane
    launch, no host read."""
    if not _mat_dev(relative_pose):
        return _kept_original("slerp_pose")(relative_pose, ts, ts_ref_pose)
    dev = relative_pose.device
    out = torch.empty((4, 4), dtype=relative_pose.dtype, device=dev)
    with _guard(dev):
        _slerp(relative_pose.detach().contiguous(), float(ts) - float(ts_ref_pose), out)
    return out


# ---------------------------------------------------------------- projection to the cameras
def _cam_table(entries):
    """ctypes array of pings_lidar_cam from dicts with the struct's field names (tensors or None)."""
    cams = (_abi.LidarCam * len(entries))()
    for c, e in enumerate(entries):
        p = lambda k: None if e.get(k) is None else e[k].data_ptr()  # noqa: E731
        cams[c] = _abi.LidarCam(p("image"), p("K"), p("T"), p("keys"), p("src"), p("l0"), p("l1"), p("l2"), p("l3"),
                                int(e["H"]), int(e["W"]))
    return cams


def _levels(H: int, W: int, dev, with_l0: bool = True):
    return [torch.empty((1, H >> k, W >> k), dtype=torch.float32, device=dev) if (k or with_l0) else None
            for k in range(4)]


@torch.no_grad()
def project_points_to_cam(points_torch, points_rgb_torch, img_torch, T_c_l, K_mat, min_depth=1.0, max_depth=100.0):
    """`project_points_to_cam_torch` (utils/tools.py:1242-1327): `points_rgb_torch` [N,4] gets (r, g, b, 0) of pixel
    (v, u) in the rows of the visible points, in place, and is returned with the [1,H,W] depth image (the smallest depth
    per pixel, 0 where no point landed).  One clear, one projection launch, one decode launch; no host read."""
    dev = points_torch.device if isinstance(points_torch, torch.Tensor) else None
    ok = (_cloud_ok(points_torch) and _cloud_ok(points_rgb_torch, 4, dev)
          and int(points_rgb_torch.shape[0]) == int(points_torch.shape[0])
          and isinstance(img_torch, torch.Tensor) and img_torch.device == dev and img_torch.dtype is torch.float32
          and img_torch.dim() == 3 and int(img_torch.shape[0]) == 3 and img_torch.is_contiguous()
          and min(img_torch.shape[1:]) >= 1 and _mat_dev(T_c_l, dev) and isinstance(K_mat, torch.Tensor)
          and K_mat.device == dev and K_mat.dim() == 2 and min(K_mat.shape) >= 3 and float(min_depth) >= 0.0)
    if not ok:
        return _kept_original("project_points_to_cam_torch")(points_torch, points_rgb_torch, img_torch, T_c_l, K_mat,
                                                             min_depth, max_depth)
    n, H, W = int(points_torch.shape[0]), int(img_torch.shape[1]), int(img_torch.shape[2])
    with _guard(dev):
        T = T_c_l.detach().to(torch.float32).contiguous()
        K = K_mat.detach()[:3, :3].to(torch.float32).contiguous()
        keys = torch.zeros(H * W, dtype=torch.int32, device=dev)
        depth = torch.empty((1, H, W), dtype=torch.float32, device=dev)
        cams = _cam_table([dict(image=img_torch, K=K, T=T, keys=keys, l0=depth, H=H, W=W)])
        rs = _row_stride(points_rgb_torch)
        _lib.check(_entry("pings_lidar_project")(
            points_torch.data_ptr() if n else None, n, _row_stride(points_torch), cams, 1, float(min_depth),
            float(max_depth), points_rgb_torch.data_ptr() if n else None, rs,
            points_rgb_torch.data_ptr() + 12 if n else None, rs, None, 0, _lib.stream_ptr(dev)), "pings_lidar_project")
        _lib.check(_entry("pings_lidar_depth_pyramid")(cams, 1, _lib.stream_ptr(dev)), "pings_lidar_depth_pyramid")
    return points_rgb_torch, depth


@torch.no_grad()
def depth_pyramid(depth: torch.Tensor):
    """The four depth levels of `CamImage.set_depth_img` from a [1,H,W] float32 device image: level 0 is `depth` itself,
    level k the 'nearest-exact' half-scaling applied k times ([1, H >> k, W >> k], source pixel 2^k i + 2^k - 1).  One
    launch, no host read."""
    if not (isinstance(depth, torch.Tensor) and depth.is_cuda and depth.dtype is torch.float32 and depth.dim() == 3
            and int(depth.shape[0]) == 1 and depth.is_contiguous() and min(depth.shape[1:]) >= 8):
        raise _lib.PingsHipError("lidar_ops.depth_pyramid: a contiguous float32 [1,H,W] device image with H, W >= 8")
    dev, H, W = depth.device, int(depth.shape[1]), int(depth.shape[2])
    lv = _levels(H, W, dev, with_l0=False)
    with _guard(dev):
        cams = _cam_table([dict(src=depth, l1=lv[1], l2=lv[2], l3=lv[3], H=H, W=W)])
        _lib.check(_entry("pings_lidar_depth_pyramid")(cams, 1, _lib.stream_ptr(dev)), "pings_lidar_depth_pyramid")
    return [depth, lv[1], lv[2], lv[3]]


def set_depth_img(self, depth_img_torch):
    """`CamImage.set_depth_img`: `depth_on` and the four entries of `depth_image_list`, through `depth_pyramid`."""
    if depth_img_torch is None:
        return
    d = depth_img_torch.to(self.device) if isinstance(depth_img_torch, torch.Tensor) else depth_img_torch
    if not (isinstance(d, torch.Tensor) and d.is_cuda and d.dtype is torch.float32 and d.dim() == 3
            and int(d.shape[0]) == 1 and d.is_contiguous() and min(d.shape[1:]) >= 8):
        return _original(self, "set_depth_img")(self, depth_img_torch)
    self.depth_on = True
    self.depth_image_list[0:4] = depth_pyramid(d)


@torch.no_grad()
def project_to_cams(dataset, use_only_colorized_points: bool = True, tran_in_frame=None):
    """`SLAMDataset.project_pointcloud_to_cams` (dataset/slam_dataset.py:803-856) with its side effects in its order:
    no images, nothing changes; `None` cameras are skipped; with `tran_in_frame` and `cur_sensor_ts` each camera's
    T_c_l is multiplied by the inverse of `slerp_pose(tran_in_frame, ratio, deskew_ref_ratio)` (one 64-lane launch per
    camera, on the device); every camera gets its depth image and the three levels below it; columns 3: of the cloud get
    the colours (-1 where no camera sees the point; a later camera overwrites an earlier one); with
    `use_only_colorized_points` the cloud, `cur_point_ts_torch`, `cur_point_normals`, `cur_sem_labels_torch` and
    `cur_sem_labels_full` are compacted through `select_rows`: one host read, none without.  The camera matrices are
    uploaded once and again only when `K_mats` / `T_c_l_mats` change (kept as `dataset._pings_cam_mats`); per call one
    clear, one projection launch for all cameras and one launch for every pyramid."""
    if dataset.cur_cam_img is None:
        return
    cloud, cfg = dataset.cur_point_cloud_torch, dataset.config
    named = [(name, cam) for name, cam in dataset.cur_cam_img.items() if cam is not None]
    dev = cloud.device if isinstance(cloud, torch.Tensor) else None
    slerp_on = tran_in_frame is not None and dataset.cur_sensor_ts is not None
    ok = (_cloud_ok(cloud, 6) and int(cloud.shape[1]) == 6 and cloud.is_contiguous() and len(named) <= MAX_CAMS
          and float(cfg.min_range) >= 0.0
          and all(getattr(cam, "rgb_image_list", None) and _image_ok(cam.rgb_image_list[0], dev) for _, cam in named)
          and all(t is None or (isinstance(t, torch.Tensor) and t.device == dev and int(t.shape[0]) == int(cloud.shape[0]))
                  for t in (dataset.cur_point_ts_torch, dataset.cur_point_normals, dataset.cur_sem_labels_torch)))
    if not ok:
        return _original(dataset, "project_pointcloud_to_cams")(dataset, use_only_colorized_points, tran_in_frame)
    n, ncam = int(cloud.shape[0]), len(named)
    with _guard(dev):
        entries, levels = [], []
        if ncam:
            host = np.zeros((ncam, 25), dtype=np.float32)
            for c, (name, _) in enumerate(named):
                host[c, :9] = np.asarray(dataset.K_mats[name], dtype=np.float64)[:3, :3].reshape(9)
                host[c, 9:] = np.asarray(dataset.T_c_l_mats[name], dtype=np.float64).reshape(16)
            held = getattr(dataset, "_pings_cam_mats", None)         # the rig's matrices are uploaded when they change
            if held is None or held[0] != host.tobytes() or held[1].device != dev:
                held = dataset._pings_cam_mats = (host.tobytes(), torch.from_numpy(host).to(dev))
            mats = held[1]
            if slerp_on:
                moved = torch.empty((ncam, 16), dtype=torch.float32, device=dev)
                tran = _pose_dev(tran_in_frame, dev)
            sizes = [tuple(int(s) for s in cam.rgb_image_list[0].shape[1:]) for _, cam in named]
            keys = torch.zeros(sum(h * w for h, w in sizes), dtype=torch.int32, device=dev)
            at = 0
            for c, ((name, cam), (H, W)) in enumerate(zip(named, sizes)):
                T = mats[c, 9:]
                if slerp_on:
                    ratio = dataset.get_cur_cam_ref_ts_ratio(name)
                    _slerp(tran, float(ratio) - float(cfg.deskew_ref_ratio), moved[c], left=T, invert=True)
                    T = moved[c]
                lv = _levels(H, W, dev)
                levels.append(lv)
                entries.append(dict(image=cam.rgb_image_list[0], K=mats[c, :9], T=T, keys=keys[at:at + H * W], l0=lv[0],
                                    l1=lv[1], l2=lv[2], l3=lv[3], H=H, W=W))
                at += H * W
        cams = _cam_table(entries) if ncam else None
        seen = torch.empty(n, dtype=torch.uint8, device=dev) if use_only_colorized_points else None
        _lib.check(_entry("pings_lidar_project")(
            cloud.data_ptr() if n else None, n, 6, cams, ncam, float(cfg.min_range), 100.0,
            cloud.data_ptr() + 12 if n else None, 6, None, 1, None if seen is None else seen.data_ptr(), 1,
            _lib.stream_ptr(dev)), "pings_lidar_project")
        if ncam:
            _lib.check(_entry("pings_lidar_depth_pyramid")(cams, ncam, _lib.stream_ptr(dev)),
                       "pings_lidar_depth_pyramid")
        for (_, cam), lv in zip(named, levels):
            if isinstance(getattr(cam, "depth_image_list", None), list) and len(cam.depth_image_list) >= 4:
                cam.depth_on = True
                cam.depth_image_list[0:4] = lv
            else:
                cam.set_depth_img(lv[0])
    if use_only_colorized_points:
        sem = dataset.cur_sem_labels_torch
        full = dataset.cur_sem_labels_full if sem is not None else None
        out = select_rows(seen, cloud, dataset.cur_point_ts_torch, dataset.cur_point_normals, sem, full)
        dataset.cur_point_cloud_torch = out[0]
        if dataset.cur_point_ts_torch is not None:
            dataset.cur_point_ts_torch = out[1]
        if dataset.cur_point_normals is not None:
            dataset.cur_point_normals = out[2]
        if sem is not None:
            dataset.cur_sem_labels_torch, dataset.cur_sem_labels_full = out[3], out[4]


# ---------------------------------------------------------------- the two other methods
def _module_of(self):
    return sys.modules.get(type(self).__module__)


def filter_and_correct(self):
    """`SLAMDataset.filter_and_correct` (dataset/slam_dataset.py:584-621): the crop branch through `crop_rows` and
    `select_rows` (one host read for the cloud, the time stamps and the LiDAR indices together), then the reference's
    own `intrinsic_correct` when `kitti_correction_on`.  The semantic-KITTI branch is the original's."""
    cloud, cfg = self.cur_point_cloud_torch, self.config
    ts, lidx = self.cur_point_ts_torch, self.cur_point_lidar_idx_torch
    if self.cur_sem_labels_torch is not None or not _cloud_ok(cloud) or any(
            t is not None and not (isinstance(t, torch.Tensor) and t.device == cloud.device
                                   and int(t.shape[0]) == int(cloud.shape[0])) for t in (ts, lidx)):
        return _original(self, "filter_and_correct")(self)
    mask = crop_rows(cloud, cfg.min_z, cfg.max_z, cfg.min_range, self.crop_max_range,
                     cfg.range_filter_2d and (not self.is_rgbd))
    out = select_rows(mask, cloud, ts, lidx)
    self.cur_point_cloud_torch = out[0]
    if ts is not None:
        self.cur_point_ts_torch = out[1]
    if lidx is not None:
        self.cur_point_lidar_idx_torch = out[2]
    if cfg.kitti_correction_on:
        correct = getattr(_module_of(self), "intrinsic_correct", None) or _kept_original("intrinsic_correct")
        self.cur_point_cloud_torch = correct(self.cur_point_cloud_torch, cfg.correction_deg)


def voxel_downsample_points_for_mapping(self):
    """`SLAMDataset.voxel_downsample_points_for_mapping` (:776-784): `neural_map.voxel_down_sample` on the coordinates,
    then the cloud, the time stamps and both label tensors gathered in one launch.  No read beyond the down-sampler's."""
    cloud = self.cur_point_cloud_torch
    ts, sem = self.cur_point_ts_torch, self.cur_sem_labels_torch
    full = self.cur_sem_labels_full if sem is not None else None
    if not _cloud_ok(cloud) or int(cloud.shape[0]) == 0 or any(
            t is not None and not (isinstance(t, torch.Tensor) and t.device == cloud.device
                                   and int(t.shape[0]) == int(cloud.shape[0])) for t in (ts, sem, full)):
        return _original(self, "voxel_downsample_points_for_mapping")(self)
    idx = neural_map.voxel_down_sample(cloud[:, :3], self.train_voxel_m)
    out = select_rows(idx, cloud, ts, sem, full)
    self.cur_point_cloud_torch = out[0]
    if ts is not None:
        self.cur_point_ts_torch = out[1]
    if sem is not None:
        self.cur_sem_labels_torch, self.cur_sem_labels_full = out[2], out[3]


# ---------------------------------------------------------------- install
_NAMES = (("deskewing", deskew), ("slerp_pose", slerp_pose), ("project_points_to_cam_torch", project_points_to_cam))
_METHODS = (("filter_and_correct", filter_and_correct),
            ("voxel_downsample_points_for_mapping", voxel_downsample_points_for_mapping),
            ("project_pointcloud_to_cams", project_to_cams))


def install(slam_dataset_module, cam_cls=None) -> None:
    """`import dataset.slam_dataset as sd; from gaussian_splatting.utils.cameras import CamImage; install(sd, CamImage)`:
    rebinds the module's names `deskewing`, `slerp_pose` and `project_points_to_cam_torch` (so the reference's own
    `preprocess_source_points` and `update_odom_pose` deskew on the device), the methods `filter_and_correct`,
    `voxel_downsample_points_for_mapping` and `project_pointcloud_to_cams` of its `SLAMDataset` and, with `cam_cls`,
    `set_depth_img`.  The originals are kept as `_pings_<name>_original` for the fallbacks and for `uninstall`.
    Installing twice changes nothing."""
    mod = slam_dataset_module
    for name, fn in _NAMES:
        if getattr(mod, name, None) is not fn:
            orig = getattr(mod, name, None)
            setattr(mod, f"_pings_{name}_original", orig)
            if orig is not None:
                _kept[name] = orig
            setattr(mod, name, fn)
    if getattr(mod, "intrinsic_correct", None) is not None:
        _kept["intrinsic_correct"] = mod.intrinsic_correct
    cls = getattr(mod, "SLAMDataset", None)
    if cls is not None:
        for name, fn in _METHODS:
            _rebind(cls, name, fn)
    if cam_cls is not None:
        _rebind(cam_cls, "set_depth_img", set_depth_img)


def uninstall(slam_dataset_module, cam_cls=None) -> None:
    """Puts the reference's own names and methods back wherever `install` replaced them."""
    mod = slam_dataset_module
    for name, fn in _NAMES:
        kept = f"_pings_{name}_original"
        if getattr(mod, name, None) is fn:
            orig = getattr(mod, kept, None)
            if orig is not None:
                setattr(mod, name, orig)
            else:
                delattr(mod, name)
        if hasattr(mod, kept):
            delattr(mod, kept)
        _kept.pop(name, None)
    _kept.pop("intrinsic_correct", None)
    cls = getattr(mod, "SLAMDataset", None)
    if cls is not None:
        for name, fn in _METHODS:
            _restore(cls, name, fn)
    if cam_cls is not None:
        _restore(cam_cls, "set_depth_img", set_depth_img)
