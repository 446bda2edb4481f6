"""float64 restatement of the LiDAR frame front-end (pings_amd/lidar_ops.py, csrc/lidar.hip), written from the behaviour
the operators document, for tests/test_lidar_ref.py (CPU) and tests/test_lidar_ops.py (GPU).

Inputs are float32 values widened to float64; nothing is rounded on the way.  Every decision a float32 implementation may
take the other way is reported next to the result as an "undecided" set:
  projection   a point whose q_x / |d| or q_y / |d| lies within PIX_EPS of a half-integer or whose d lies within
               DEPTH_EPS * max(1, |d|) of a depth bound; a pixel such a point projects to, or a neighbour of it
  crop         a row whose distance or z lies within CROP_EPS (relative) of a threshold
The rotation interpolation is defined from first principles: (a, theta) = axis and angle in [0, pi] of R, R(s) = the
rotation by s theta about a.  tests/test_lidar_ref.py checks it against scipy's `Rotation.from_rotvec(s * rotvec)`.
"""
from types import SimpleNamespace as NS

import numpy as np
import torch

PIX_EPS, DEPTH_EPS, CROP_EPS = 1e-3, 1e-4, 1e-5
MAX_DEPTH = 100.0


def f64(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


# ================================================================ rotation
def axis_angle(R):
    """(axis [3], angle in [0, pi]) of a rotation matrix, through its quaternion with the largest pivot."""
    R = f64(R)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif R[1, 1] > R[2, 2]:
        s = np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.array(q)
    if q[0] < 0:
        q = -q
    nv = np.linalg.norm(q[1:])
    if nv == 0:
        return np.array([1.0, 0.0, 0.0]), 0.0
    return q[1:] / nv, 2.0 * np.arctan2(nv, q[0])


def rotations(R, s):
    """[n,3,3]: the rotation by s_i theta about the axis of R (Rodrigues)."""
    a, theta = axis_angle(R)
    ang = np.atleast_1d(f64(s)) * theta
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    sn, cs = np.sin(ang)[:, None, None], np.cos(ang)[:, None, None]
    return cs * np.eye(3) + sn * Kx + (1 - cs) * np.outer(a, a)


def slerp_pose(pose, ts, ts_ref_pose):
    pose = f64(pose)
    s = float(ts) - float(ts_ref_pose)
    T = np.eye(4)
    T[:3, :3] = rotations(pose[:3, :3], s)[0]
    T[:3, 3] = s * pose[:3, 3]
    return T


def normalised_time(ts, ts_ref_pose):
    ts = f64(ts).reshape(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (ts - ts.min()) / (ts.max() - ts.min()) - ts_ref_pose


def deskew(points, ts, pose, ts_ref_pose=0.5, points_lidar_idx=None, T_l_lm_list=None, ts_diff_list=None):
    """The first three columns after deskewing, float64 [N,3]."""
    p = f64(points)[:, :3].copy()
    if ts is None:
        return p
    multi = T_l_lm_list is not None and points_lidar_idx is not None
    if multi and len(T_l_lm_list) == 0:
        return p
    pose = f64(pose)
    s = normalised_time(ts, ts_ref_pose)

    def apply(q, sv, P):
        return np.einsum("nij,nj->ni", rotations(P[:3, :3], sv), q) + sv[:, None] * P[:3, 3]

    if not multi:
        return apply(p, s, pose)
    idx = np.asarray(points_lidar_idx.detach().cpu() if isinstance(points_lidar_idx, torch.Tensor)
                     else points_lidar_idx).reshape(-1)
    out = p.copy()
    main = idx == 0
    out[main] = apply(p[main], s[main], pose)
    for k, T in enumerate(T_l_lm_list, start=1):
        T = f64(T)
        Ti = np.linalg.inv(T)
        rows = idx == k
        sv = s[rows] + (float(ts_diff_list[k - 1]) if ts_diff_list is not None else 0.0)
        q = p[rows] @ T[:3, :3].T + T[:3, 3]
        q = apply(q, sv, T @ pose @ Ti)
        out[rows] = q @ Ti[:3, :3].T + Ti[:3, 3]
    return out


# ================================================================ crop
def crop(points, min_z, max_z, min_range, max_range, on_xy_plane):
    """(mask, undecided) of `crop_frame`."""
    p = f64(points)
    with np.errstate(invalid="ignore"):
        dist = np.sqrt((p[:, :2] ** 2).sum(1) if on_xy_plane else (p[:, :3] ** 2).sum(1))
        z = p[:, 2]
        mask = (dist > min_range) & (dist < max_range) & (z > min_z) & (z < max_z)
        near = np.zeros(len(p), bool)
        for v, thr in ((dist, min_range), (dist, max_range), (z, min_z), (z, max_z)):
            near |= np.abs(v - thr) <= CROP_EPS * max(abs(thr), 1.0)
    return mask, near


# ================================================================ projection
def project(points, T_c_l, K, H, W, min_depth, max_depth=MAX_DEPTH):
    """Per point: u, v (int64, valid where visible), d, visible, undecided."""
    p, T, K = f64(points)[:, :3], f64(T_c_l), f64(K)[:3, :3]
    with np.errstate(all="ignore"):
        P = p @ T[:3, :3].T + T[:3, 3]
        q = P @ K.T
        d = q[:, 2].copy()
        d[d == 0] = -1e-6
        fu, fv = q[:, 0] / np.abs(d), q[:, 1] / np.abs(d)
        u, v = np.rint(fu), np.rint(fv)
        vis = (u >= 0) & (u < W) & (v >= 0) & (v < H) & (d > min_depth) & (d < max_depth)
        half = lambda x: np.abs(x - np.floor(x) - 0.5) < PIX_EPS  # noqa: E731
        in_reach = (fu > -1.5) & (fu < W + 0.5) & (fv > -1.5) & (fv < H + 0.5) & (d > 0.5 * min_depth) & \
                   (d < 2 * max_depth)
        und = in_reach & (half(fu) | half(fv) | (np.abs(d - min_depth) < DEPTH_EPS * np.maximum(1, np.abs(d)))
                          | (np.abs(d - max_depth) < DEPTH_EPS * np.maximum(1, np.abs(d))))
        und &= np.isfinite(fu) & np.isfinite(fv)
    ui = np.where(vis, u, 0).astype(np.int64)
    vi = np.where(vis, v, 0).astype(np.int64)
    return NS(u=ui, v=vi, d=d, visible=vis, undecided=und, fu=fu, fv=fv)


def depth_image(pr, H, W):
    """([H,W] minimum depth of the visible points, 0 where none landed; [H,W] undecided pixels)."""
    depth = np.full(H * W, np.inf)
    pix = pr.v[pr.visible] * W + pr.u[pr.visible]
    np.minimum.at(depth, pix, pr.d[pr.visible])
    depth[np.isinf(depth)] = 0.0
    und = np.zeros((H + 2, W + 2), bool)
    rows = np.nonzero(pr.undecided)[0]
    cu = np.clip(np.rint(pr.fu[rows]), -1, W).astype(np.int64) + 1
    cv = np.clip(np.rint(pr.fv[rows]), -1, H).astype(np.int64) + 1
    for dv in (-1, 0, 1):
        for du in (-1, 0, 1):
            und[np.clip(cv + dv, 0, H + 1), np.clip(cu + du, 0, W + 1)] = True
    return depth.reshape(H, W), und[1:-1, 1:-1]


def project_points_to_cam(points, points_rgb, img, T_c_l, K, min_depth=1.0, max_depth=MAX_DEPTH):
    """(rgb [N,4], depth [1,H,W], undecided points, undecided pixels) of `project_points_to_cam_torch`."""
    img = f64(img)
    _, H, W = img.shape
    pr = project(points, T_c_l, K, H, W, min_depth, max_depth)
    rgb = f64(points_rgb).copy()
    rows = np.nonzero(pr.visible)[0]
    rgb[rows, :3] = img[:, pr.v[rows], pr.u[rows]].T
    rgb[rows, 3] = 0.0
    depth, und_px = depth_image(pr, H, W)
    return rgb, depth[None], pr.undecided.copy(), und_px, pr


def depth_pyramid(depth):
    """[l0, l1, l2, l3]: 'nearest-exact' at scale 0.5 reads source index 2 i + 1 and gives floor(n / 2) entries."""
    d = f64(depth)
    out = [d]
    for _ in range(3):
        d = d[:, 1:(d.shape[1] // 2) * 2:2, 1:(d.shape[2] // 2) * 2:2]
        out.append(d)
    return out


def project_to_cams(ds, use_only_colorized_points=True, tran_in_frame=None):
    """`SLAMDataset.project_pointcloud_to_cams` on the stand-in `ds` WITHOUT changing it: a namespace with the cloud
    [*,6], the kept rows, each camera's four depth levels and the undecided points / pixels."""
    cloud = f64(ds.cur_point_cloud_torch).copy()
    if ds.cur_cam_img is None:
        return None
    n = cloud.shape[0]
    rgb = -np.ones((n, 4))
    und = np.zeros(n, bool)
    cams = {}
    for name, cam in ds.cur_cam_img.items():
        if cam is None:
            continue
        T = f64(ds.T_c_l_mats[name])
        if tran_in_frame is not None and ds.cur_sensor_ts is not None:
            ratio = ds.get_cur_cam_ref_ts_ratio(name)
            T = T @ np.linalg.inv(slerp_pose(tran_in_frame, ratio, ds.config.deskew_ref_ratio))
        rgb, depth, u_pt, u_px, _ = project_points_to_cam(cloud, rgb, cam.rgb_image_list[0], T, ds.K_mats[name],
                                                          ds.config.min_range)
        und |= u_pt
        cams[name] = NS(levels=depth_pyramid(depth), undecided=u_px)
    cloud[:, 3:] = rgb[:, :3]
    keep = rgb[:, 3] == 0 if use_only_colorized_points else np.ones(n, bool)
    return NS(cloud=cloud, keep=keep, undecided=und, cams=cams)


def voxel_downsample_rows(ds):
    """Kept rows of `voxel_downsample_points_for_mapping`: the reference's float32 down-sampler, op for op."""
    from oracle import map_cpu

    return map_cpu.voxel_down_sample(ds.cur_point_cloud_torch[:, :3].detach().cpu().float(), ds.train_voxel_m).numpy()


# ================================================================ scenes and stand-ins
def look_along_x(yaw=0.0, pitch=0.0, t=(0.0, 0.0, 0.0)):
    """T_c_l of a camera whose optical axis is the LiDAR's x (image x = -y, image y = -z), turned by yaw and pitch."""
    base = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    T = np.eye(4)
    T[:3, :3] = base @ Ry @ Rz
    T[:3, 3] = t
    return T


def intrinsics(H, W, scale=0.7):
    return np.array([[scale * W, 0.0, 0.5 * W - 0.25], [0.0, scale * W, 0.5 * H + 0.125], [0.0, 0.0, 1.0]])


def scene(n, H, W, seed, ncam=1):
    """A random scan in front of `ncam` overlapping cameras: float32 cloud [n,6] (colour columns 0), images [3,H,W],
    float64 T_c_l / K per camera.  About a fifth of the points lie behind the cameras, beyond 100 m or below min_depth."""
    g = np.random.default_rng(seed)
    x = g.uniform(0.3, 60.0, n)
    far = g.random(n) < 0.05
    x[far] = g.uniform(90.0, 130.0, far.sum())
    x[g.random(n) < 0.1] *= -1.0
    y = g.uniform(-0.9, 0.9, n) * np.abs(x)
    z = g.uniform(-0.6, 0.6, n) * np.abs(x)
    cloud = np.zeros((n, 6), np.float32)
    cloud[:, :3] = np.stack([x, y, z], 1)
    names = [f"cam{c}" for c in range(ncam)]
    r32 = lambda m: m.astype(np.float32).astype(np.float64)  # noqa: E731  (float32 values, held as float64)
    T = {nm: r32(look_along_x(0.5 * c, 0.03 * c, (0.05 * c, -0.02, 0.1))) for c, nm in enumerate(names)}
    K = {nm: r32(intrinsics(H, W, 0.7 + 0.05 * c)) for c, nm in enumerate(names)}
    img = {nm: g.random((3, H, W)).astype(np.float32) for nm in names}
    return NS(cloud=cloud, names=names, T=T, K=K, img=img, H=H, W=W, min_range=1.5)


class Cam:
    """Stand-in `CamImage`: the attributes `set_depth_img` and `project_pointcloud_to_cams` touch."""

    def __init__(self, img, device="cpu", set_depth_img=None):
        self.device = device
        self.rgb_image_list = [torch.as_tensor(img).to(device)] + [None] * 3
        self.depth_image_list = [None] * 4
        self.depth_on = False
        self._set = set_depth_img

    def set_depth_img(self, depth):
        return self._set(self, depth)


class Dataset:
    """Stand-in `SLAMDataset` with the attributes the front-end methods read and write."""

    def __init__(self, sc, device="cpu", companions=True, cams=None, set_depth_img=None, seed=0):
        g = torch.Generator().manual_seed(seed)
        n = sc.cloud.shape[0]
        self.device, self.dtype = device, torch.float32
        self.config = NS(min_range=sc.min_range, deskew_ref_ratio=0.5, min_z=-3.0, max_z=40.0, range_filter_2d=True,
                         kitti_correction_on=False, correction_deg=0.0)
        self.crop_max_range, self.is_rgbd, self.train_voxel_m = 50.0, False, 2.5
        self.cur_point_cloud_torch = torch.as_tensor(sc.cloud).clone().to(device)
        self.cur_point_ts_torch = torch.rand(n, generator=g).to(device) if companions else None
        self.cur_point_normals = torch.randn(n, 3, generator=g).to(device) if companions else None
        self.cur_sem_labels_torch = torch.randint(0, 20, (n,), generator=g).to(device) if companions else None
        self.cur_sem_labels_full = torch.randint(0, 300, (n,), generator=g).to(device) if companions else None
        self.cur_point_lidar_idx_torch = None
        self.cur_sensor_ts = None
        self.T_c_l_mats, self.K_mats = dict(sc.T), dict(sc.K)
        names = sc.names if cams is None else cams
        self.cur_cam_img = {nm: (None if nm is None or nm.startswith("none") else Cam(sc.img[nm], device, set_depth_img))
                            for nm in names}
        self.loader = NS(main_lidar_name="lidar")

    def get_cur_cam_ref_ts_ratio(self, cam_name, lidar_t_interval: float = 0.1):
        if self.cur_sensor_ts is None:
            return None
        return (self.cur_sensor_ts[cam_name] - (self.cur_sensor_ts[self.loader.main_lidar_name] - lidar_t_interval)) \
            / lidar_t_interval


def crop_cloud(n, seed):
    """A random scan around the sensor, float32 [n,4], with NaN in two rows."""
    g = np.random.default_rng(seed)
    p = np.concatenate([g.normal(0, 25.0, (n, 2)), g.normal(0, 4.0, (n, 1)), g.random((n, 1))], 1).astype(np.float32)
    if n > 40:
        p[17, 0] = np.nan
        p[33, 2] = np.nan
    return p
