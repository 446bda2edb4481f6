"""numpy restatement of the camera frame front-end (pings_amd/camfront_ops.py), with the reference's line numbers.

`CamImage.__init__` (gaussian_splatting/utils/cameras.py):
  :39        rgb_image.clamp(0.0, 1.0)                                           `clamp01`
  :131-135   F.interpolate(scale_factor=0.5, mode='bilinear', align_corners=False), three times     `bilinear_levels`
  :138-140   F.interpolate(scale_factor=0.5, mode='nearest-exact'), three times                     `nearest_exact_levels`
  :147-149   F.interpolate(mask.float(), scale_factor=0.5, mode='nearest').bool(), three times      `nearest_levels`
  :157-159   the normal image, as the RGB image                                  `bilinear_levels`
  :164-186   the four lists, `cur_best_level`, `free_memory_under_levels`        `cam_lists`

With scale 0.5 the bilinear source index of output pixel i is 2 i + 0.5: pixels 2 i and 2 i + 1 with weight 0.5 each, so
a level is `0.5 (0.5 a + 0.5 b) + 0.5 (0.5 c + 0.5 d)` over the 2 x 2 blocks of the level above.  `bilinear_levels`
evaluates that in float64 from the float32 level above and rounds to float32 once per level (`exact=False`), or in
float32 operation by operation as the device does (`exact=True`); the two differ by at most one unit in the last place.
A trailing odd row or column is dropped at every level.  Inputs are examples the tests choose: `example`.

The mono-depth block of `read_frame_with_loader` (dataset/slam_dataset.py) in float64:
  :369-390   the mask, `np.polyfit`, the two rmse figures                        `fit_mask`, `align`
  :388-436   `k * pred + b`, the sky mask, the range gates                       `fitted_depth`, `thresholds`, `mono_cloud`
  :438-447   Open3D's RGBD cloud: 0 < d < depth_trunc, back-projection, colours  `mono_cloud`
  :453       Open3D's `voxel_down_sample`, over six columns                       `voxel_cells`, `voxel_average`
and the stand-ins the frame tests and tools/make_camfront_golden.py share (`Dataset`, `MonoMapRecorder`, `mono_points`).
"""
import numpy as np

LEVELS = 4


def clamp01(img):
    """torch.clamp(img, 0, 1): a NaN stays a NaN."""
    img = np.asarray(img, np.float32)
    return np.where(img < 0, np.float32(0), np.where(img > 1, np.float32(1), img)).astype(np.float32)


def u8_level0(u8_hwc):
    """float32(u) / float32(255), IEEE division, as CHW."""
    return np.ascontiguousarray((u8_hwc.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1))


def _half(a, b, c, d, dtype):
    h = dtype(0.5)
    return h * (h * a.astype(dtype) + h * b.astype(dtype)) + h * (h * c.astype(dtype) + h * d.astype(dtype))


def bilinear_levels(level0, exact=True):
    out = [np.asarray(level0, np.float32)]
    for _ in range(LEVELS - 1):
        p = out[-1]
        h, w = p.shape[1] // 2, p.shape[2] // 2
        p = p[:, :2 * h, :2 * w]
        with np.errstate(invalid="ignore"):
            nxt = _half(p[:, 0::2, 0::2], p[:, 0::2, 1::2], p[:, 1::2, 0::2], p[:, 1::2, 1::2],
                        np.float32 if exact else np.float64)
        out.append(np.ascontiguousarray(nxt.astype(np.float32)))
    return out


def nearest_exact_levels(level0):
    """Level k takes level-0 pixel (2^k y + 2^k - 1, 2^k x + 2^k - 1)."""
    H, W = level0.shape[1:]
    return [np.ascontiguousarray(level0[:, (1 << k) - 1::1 << k, (1 << k) - 1::1 << k][:, :H >> k, :W >> k])
            for k in range(LEVELS)]


def nearest_levels(level0):
    """Level k takes level-0 pixel (2^k y, 2^k x)."""
    H, W = level0.shape[1:]
    return [np.ascontiguousarray(level0[:, ::1 << k, ::1 << k][:, :H >> k, :W >> k]) for k in range(LEVELS)]


def cam_lists(rgb_chw, depth=None, sky=None, normal=None, img_down_rate=0, exact=True):
    """The four lists and `cur_best_level` after the constructor: levels below `img_down_rate` are `None`."""
    lists = [bilinear_levels(clamp01(rgb_chw), exact),
             [None] * LEVELS if depth is None else nearest_exact_levels(depth),
             [None] * LEVELS if sky is None else nearest_levels(sky),
             [None] * LEVELS if normal is None else bilinear_levels(normal, exact)]
    freed = min(max(img_down_rate, 0), LEVELS)
    lists = [[None if k < freed else lv for k, lv in enumerate(ls)] for ls in lists]
    return lists, (img_down_rate if img_down_rate >= 1 else 0)


class Cam:
    """Stand-in for `CamImage` with what the rebound constructor relies on: the original called with `rgb_image=None`
    keeps the size and leaves four empty lists (:40-44, :86-90; `depth_on` stays unset), and the two methods that free
    levels (:245-258).  A call with an image is recorded, for the fallback tests."""

    def __init__(self, frame_id, rgb_image, K_mat, z_min=0.1, z_max=100.0, cam_id="cam", img_down_rate=0,
                 depth_image=None, normal_img=None, sky_mask=None, device="cuda", cam_pose=None, img_width=None,
                 img_height=None, pyramid_level=4):
        self.frame_id, self.K_mat, self.device = frame_id, K_mat, device
        self.fell_back = rgb_image is not None
        self.image_width, self.image_height = img_width, img_height
        self.pyramid_level = pyramid_level
        self.rgb_image_list = [None] * pyramid_level
        self.depth_image_list = [None] * pyramid_level
        self.sky_mask_list = [None] * pyramid_level
        self.normal_img_list = [None] * pyramid_level

    def free_memory_at_level(self, level=0):
        if 0 <= level < len(self.rgb_image_list):
            for ls in (self.rgb_image_list, self.depth_image_list, self.normal_img_list, self.sky_mask_list):
                ls[level] = None
            self.cur_best_level = level + 1

    def free_memory_under_levels(self, highest=0):
        for level in range(min(highest + 1, len(self.rgb_image_list))):
            self.free_memory_at_level(level)
        self.cur_best_level = highest + 1


def example(H, W, seed=0):
    """uint8 [H,W,3] holding all 256 values (when it has room), depth [1,H,W] with zeros, a bool sky mask, unit normals."""
    rng = np.random.default_rng(seed)
    u8 = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    flat = u8.reshape(-1)
    n = min(256, flat.size)
    flat[rng.permutation(flat.size)[:n]] = np.arange(n, dtype=np.uint8)
    depth = rng.uniform(1.0, 80.0, (1, H, W)).astype(np.float32)
    depth[rng.random((1, H, W)) < 0.3] = 0.0
    sky = rng.random((1, H, W)) < 0.4
    normal = rng.normal(size=(3, H, W))
    normal = (normal / np.linalg.norm(normal, axis=0, keepdims=True)).astype(np.float32)
    return u8, depth, sky, normal


# ================================================================ the mono-depth cloud (dataset/slam_dataset.py:366-477)
MIN_FIT = 100                                              # :382 `valid_depth_count > 100`
NEAR = 1e-5                                                # a depth this close (relative) to a threshold is undecided


def fit_mask(pred, lidar, min_range, max_range):
    """:370; numpy rounds each Python scalar to the arrays' float32 once."""
    lo, hi = np.float32(min_range), np.float32(max_range * 0.8)
    return (lidar > lo) & (pred > lo) & (lidar < hi)


def align(pred, lidar, min_range, max_range):
    """:369-390 in float64: (count, k, b, rmse_before, rmse_after); count <= 100 gives k = 1, b = 0, rmse_after NaN."""
    m = fit_mask(pred, lidar, min_range, max_range)
    x, y = pred[m].astype(np.float64), lidar[m].astype(np.float64)
    n = int(m.sum())
    before = float(np.sqrt(np.mean((x - y) ** 2))) if n else float("nan")
    if n <= MIN_FIT:
        return n, 1.0, 0.0, before, float("nan")
    (k, b), res, _, _, _ = np.polyfit(x, y, 1, full=True)
    return n, float(k), float(b), before, float(np.sqrt(res[0] / n))


def thresholds(min_range, max_range, high_z):
    """(sky, far or None, near) as float32: :396, :433-436."""
    return (np.float32(max_range * 1.2), np.float32(0.8 * max_range) if high_z else None,
            np.float32(2.0 * min_range) if high_z else np.float32(0.2 * max_range))


def fitted_depth(pred, k=1.0, b=0.0):
    """:388 with numpy 2, which promotes `k * pred_depth_np + b` to float64 (numpy 1 would stay in float32); the depth
    image Open3D reads is float32, so the value is rounded once."""
    return (np.float64(k) * pred.astype(np.float64) + np.float64(b)).astype(np.float32)


def mono_cloud(pred, u8, K, T_c_l, min_range, max_range, depth_trunc, high_z, k=1.0, b=0.0):
    """:388-447 for one camera -> (rows float64 [M,6], sky [H,W] bool, gated depth float32 [H,W], undecided [H,W]).
    `undecided` marks the pixels whose fitted depth lies within NEAR (relative) of a threshold or of depth_trunc."""
    sky_t, far_t, near_t = thresholds(min_range, max_range, high_z)
    d = fitted_depth(pred, k, b)
    und = np.zeros(d.shape, bool)
    for t in (sky_t, far_t, near_t, depth_trunc):
        if t is not None:
            und |= np.abs(d.astype(np.float64) - float(t)) <= NEAR * float(t)
    with np.errstate(invalid="ignore"):
        sky = d > sky_t                                                      # :397
        d[sky] = 0.0
        if high_z:
            d[d > far_t] = 0.0                                               # :433
        d[d < near_t] = 0.0                                                  # :434 / :436
        keep = (d.astype(np.float64) > 0.0) & (d.astype(np.float64) < float(depth_trunc))   # Open3D: 0 < d < depth_trunc
    v, u = np.nonzero(keep)                                                  # row-major pixel order
    z = d[keep].astype(np.float64)
    K = np.asarray(K, np.float64)
    x = (u.astype(np.float64) - K[0, 2]) * z / K[0, 0]
    y = (v.astype(np.float64) - K[1, 2]) * z / K[1, 1]
    T = np.linalg.inv(np.asarray(T_c_l, np.float64).reshape(4, 4))
    xyz = np.stack([T[r, 0] * x + T[r, 1] * y + T[r, 2] * z + T[r, 3] for r in range(3)], axis=1)
    rgb = u8[keep].astype(np.float64) / 255.0
    return np.concatenate([xyz, rgb], axis=1), sky, d, und


def voxel_cells(rows, voxel):
    """Open3D's grid: anchored at the minimum minus half a voxel; the linear key has x fastest (21 bits per axis)."""
    p = np.asarray(rows, np.float64)[:, :3]
    t = (p - (p.min(axis=0) - 0.5 * voxel)) / voxel
    c = np.floor(t).astype(np.int64)
    frac = t - c
    return c[:, 0] + (c[:, 1] << 21) + (c[:, 2] << 42), np.minimum(frac, 1.0 - frac).min(axis=1)


def voxel_average(rows, voxel):
    """`voxel_down_sample` over all six columns in float64, in ascending cell key."""
    rows = np.asarray(rows, np.float64)
    key, _ = voxel_cells(rows, voxel)
    order = np.argsort(key, kind="stable")
    _, start = np.unique(key[order], return_index=True)
    counts = np.diff(np.append(start, len(rows)))
    return np.add.reduceat(rows[order], start, axis=0) / counts[:, None]


def voxel_rows(n, voxel, seed, extent=6.0):
    """n float32 rows (position, colour) none of which lies within 1e-3 voxel of a cell face of its own grid."""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([rng.uniform(-extent, extent, (3 * n + 64, 3)),
                           rng.integers(0, 256, (3 * n + 64, 3)) / 255.0], axis=1).astype(np.float32)
    while True:
        _, margin = voxel_cells(pool[:n], voxel)
        near = margin < 1e-3
        if not near.any():
            return np.ascontiguousarray(pool[:n])
        pool = np.concatenate([pool[:n][~near], pool[n:]])
        assert len(pool) >= n


def fit_example(H=33, W=70, seed=0, valid=None):
    """The issue's setup: pred uniform in [1, 80] m, LiDAR = 1.07 pred - 0.6 + N(0, 0.5) on a third of the pixels and 0
    elsewhere; with `valid`, on exactly that many pixels that pass the mask at min_range 2.75, max_range 60."""
    rng = np.random.default_rng(seed)
    pred = rng.uniform(1.0, 80.0, (H, W)).astype(np.float32)
    lidar = (1.07 * pred - 0.6 + rng.normal(0.0, 0.5, (H, W))).astype(np.float32)
    if valid is None:
        lidar[rng.random((H, W)) >= 1.0 / 3.0] = 0.0
    else:
        ok = np.flatnonzero(fit_mask(pred, lidar, 2.75, 60.0).reshape(-1))
        drop = np.ones(H * W, bool)
        drop[rng.permutation(ok)[:valid]] = False
        lidar.reshape(-1)[drop] = 0.0
    return pred, lidar


def cloud_example(H, W, seed, min_range, max_range, depth_trunc, high_z, k=1.0, b=0.0, nudge=False):
    """Predicted depths that land on both sides of every gate, and an image.  With `nudge` every pixel whose fitted
    depth is within NEAR of a threshold is moved by 1e-3 of its value until none is."""
    rng = np.random.default_rng(seed)
    pred = rng.uniform(0.5, 1.5 * max_range, (H, W)).astype(np.float32)
    u8 = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    K = np.array([[0.9 * W, 0.0, 0.5 * W - 0.25], [0.0, 0.8 * W, 0.5 * H + 0.125], [0.0, 0.0, 1.0]])
    while nudge:
        und = mono_cloud(pred, u8, K, np.eye(4), min_range, max_range, depth_trunc, high_z, k, b)[3]
        if not und.any():
            break
        pred[und] *= np.float32(1.001)
    return pred, u8, K


def rig_pose(seed):
    """A rigid T_c_l with a rotation of about a radian."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = q, rng.uniform(-1.0, 1.0, 3)
    return T


class Config:
    def __init__(self, min_range=2.75, max_range=60.0, local_map_radius=50.0, vox_down_m=0.8):
        self.min_range, self.max_range = min_range, max_range
        self.local_map_radius, self.vox_down_m = local_map_radius, vox_down_m


class Loader:
    mono_depth_for_high_z = False


class Dataset:
    """Stand-in for `SLAMDataset` with what `camfront_ops.mono_frame` reads."""

    def __init__(self, cams, is_rgbd=False, **cfg):
        self.config, self.loader = Config(**cfg), Loader()
        self.cam_names = [name for name, _, _ in cams]
        self.K_mats = {name: K for name, K, _ in cams}
        self.T_c_l_mats = {name: T for name, _, T in cams}
        self.is_rgbd, self.silence = is_rgbd, True
        self.cur_point_cloud_mono_depth = None


# ================================================================ the mono-depth branch of Mapper.process_frame
MONO_CFG = dict(monodepth_on=True, voxel_size_m=0.3, monodepth_gaussian_res=12.0)
MONO_CASES = {"high": (True, 40.0), "low": (False, 40.0), "none": (True, 1.0)}       # mono_depth_for_high_z, extent


def mono_points(n, seed, extent=40.0, channels=3):
    """A mono-depth cloud in the sensor frame, float32 [n, 3 + channels], uniform in a cube of half side `extent`; a
    small cube stays under the 0.98 quantile of the frame's update points, so the mask keeps nothing."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-extent, extent, (n, 3)), rng.uniform(0.0, 1.0, (n, channels))],
                          axis=1).astype(np.float32)


class MonoMapRecorder:
    """`neural_points` stand-in that takes `is_reliable` (utils/mapper.py:327-331) and keeps every call's arguments."""

    def __init__(self):
        self.updates, self.resets, self.memory = [], [], 0

    def reset_local_map(self, origin, orientation, frame_id):
        self.resets.append((origin, orientation, frame_id))

    def update(self, points, colors, normals, origin, orientation, frame_id, is_reliable=False):
        self.updates.append((points, colors, normals, origin, orientation, frame_id, is_reliable))

    def record_memory(self, verbose=True, record_footprint=True):
        self.memory += 1


def mono_update(mono, update_z, pose, high_z, voxel_size_m, down_sample):
    """utils/mapper.py:297-331 without normals: (the cloud with xyz moved by `pose` in float64 (:299), the rows the
    second `update` receives).  The mask (:303-310) and `down_sample(xyz) -> row indices` (:316) work on the moved cloud
    rounded to float32, as the reference holds it."""
    import torch

    T = pose.double()
    moved = mono.double().clone()
    moved[:, :3] = mono[:, :3].double() @ T[:3, :3].T + T[:3, 3]
    held = moved.float()
    q = torch.quantile(update_z, 0.98 if high_z else 0.2) + voxel_size_m
    used = held[:, 2] > q if high_z else held[:, 2] < q
    rows = held[used]
    if rows.shape[0] > 0:
        rows = rows[down_sample(rows[:, :3])]
    return moved, rows
