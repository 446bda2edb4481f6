"""The camera frame front-end on the HIP device (csrc/camfront.hip).

The image pyramids the reference builds in `CamImage.__init__` (gaussian_splatting/utils/cameras.py:39, :116-182) and the
mono-depth cloud it builds on the host in `read_frame_with_loader` (dataset/slam_dataset.py:366-477), on the reference's
own tensors; no state lives here:

  `image_pyramids`     the RGB, depth, sky-mask and normal pyramids of up to 8 cameras in ONE launch, no host read
  `image_pyramid`      the same for one camera
  `cam_init`           `CamImage.__init__`: the kept original sets matrices, pose and parameters, the four lists come
                       from `image_pyramid`
  `align_mono_depth`   the least-squares fit of the predicted depth to the LiDAR depth image, as a device record
  `mono_cloud`         fitted depth, sky mask, range gates, back-projection and colours of one camera as [.,6] rows
  `voxel_average`      Open3D's `voxel_down_sample` over six columns, appended at a device offset
  `mono_frame`         all of it for every camera of a frame, with ONE host read

`install` rebinds the constructor and keeps the original, which is called for the inputs the kernel does not take (CPU
tensors, other dtypes, images under 8 x 8, `pyramid_level != 4`).  There is no torch path of this module's own: with no
original kept, such a call raises.  `last_launches` is the number of kernel launches of the latest `image_pyramids`
call, as the library reports it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _abi, _lib
from .pool_ops import _entry, _guard, _rebind, _restore

MAX_CAMS = _abi.LIDAR_MAX_CAMS
TILE_H, TILE_W = _abi.CAMFRONT_TILE_H, _abi.CAMFRONT_TILE_W
LEVELS = 4

last_launches = 0


def _dev_tensor(t, dtype, dev=None) -> bool:
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype is dtype and (dev is None or t.device == dev)


def _rgb_size(rgb):
    """(H, W) of an RGB image the kernel takes, else None: uint8 [H,W,3] contiguous or float32 [3,H,W] (any strides)."""
    if _dev_tensor(rgb, torch.uint8) and rgb.dim() == 3 and int(rgb.shape[2]) == 3 and rgb.is_contiguous():
        H, W = int(rgb.shape[0]), int(rgb.shape[1])
    elif _dev_tensor(rgb, torch.float32) and rgb.dim() == 3 and int(rgb.shape[0]) == 3:
        H, W = int(rgb.shape[1]), int(rgb.shape[2])
    else:
        return None
    return (H, W) if H >= 8 and W >= 8 and 3 * H * W < 2 ** 31 - 16 else None


def _planar_ok(t, dtype, channels: int, H: int, W: int, dev) -> bool:
    return t is None or (_dev_tensor(t, dtype, dev) and tuple(t.shape) == (channels, H, W))


def _frame_ok(rgb, depth, sky_mask, normal) -> bool:
    size = _rgb_size(rgb)
    return (size is not None and _planar_ok(depth, torch.float32, 1, *size, rgb.device)
            and _planar_ok(sky_mask, torch.bool, 1, *size, rgb.device)
            and _planar_ok(normal, torch.float32, 3, *size, rgb.device))


def _map(kind: int, src: torch.Tensor, levels, H: int, W: int, write_l0: bool):
    if kind == _abi.CAMFRONT_RGB_U8:
        sc = sy = sx = 0
    else:
        sc, sy, sx = (int(s) for s in src.stride())
        if int(src.shape[0]) == 1:
            sc = 0
    p = [None if (lv is None or (k == 0 and not write_l0)) else lv.data_ptr() for k, lv in enumerate(levels)]
    return _abi.CamfrontMap(src.data_ptr(), p[0], p[1], p[2], p[3], sc, sy, sx, H, W, kind, 0)


@torch.no_grad()
def image_pyramids(frames, first_level: int = 0):
    """`frames`: up to 8 tuples `(rgb, depth, sky_mask, normal)` (the last three may be `None`), one per camera, all on
    one device.  Returns per camera the four lists `(rgb_levels, depth_levels, sky_levels, normal_levels)` of four
    entries each; a map that was not given is four `None`s.

    `rgb` is uint8 [H,W,3] as the loaders deliver it (level 0 is `float(u) / 255`) or float32 [3,H,W] with any strides
    (the reference passes a permuted HWC view; level 0 is the value clamped to [0,1], a NaN stays).  `depth` float32
    [1,H,W], `sky_mask` bool [1,H,W], `normal` float32 [3,H,W].  Level k has (H >> k, W >> k) pixels: RGB and normal by
    `F.interpolate(scale_factor=0.5, mode='bilinear')` chained, depth by `'nearest-exact'`, the sky mask by `'nearest'`.
    Every level is a contiguous CHW tensor of its own; level 0 of depth, sky mask and normal is the input object.
    Levels below `first_level` are `None`: neither allocated nor written.  One launch for everything, no host read."""
    global last_launches
    frames = [tuple(f) + (None,) * (4 - len(f)) for f in frames]
    first_level = int(first_level)
    if not (0 <= first_level <= LEVELS):
        raise _lib.PingsHipError("camfront_ops.image_pyramids: first_level is 0..4")
    if not (1 <= len(frames) <= MAX_CAMS):
        raise _lib.PingsHipError(f"camfront_ops.image_pyramids: 1..{MAX_CAMS} cameras per call")
    dev = frames[0][0].device if isinstance(frames[0][0], torch.Tensor) else None
    for rgb, depth, sky, normal in frames:
        if not (_frame_ok(rgb, depth, sky, normal) and rgb.device == dev):
            raise _lib.PingsHipError(
                "camfront_ops.image_pyramids: rgb is a uint8 [H,W,3] (contiguous) or float32 [3,H,W] device tensor "
                "with H, W >= 8; depth float32 [1,H,W], sky_mask bool [1,H,W], normal float32 [3,H,W] on its device")
    out, maps = [], []
    for rgb, depth, sky, normal in frames:
        H, W = _rgb_size(rgb)
        u8 = rgb.dtype is torch.uint8

        def levels(src, channels, dtype, own_l0):
            if src is None:
                return [None] * LEVELS
            return [None if k < first_level else (src if (k == 0 and not own_l0) else
                                                  torch.empty((channels, H >> k, W >> k), dtype=dtype, device=dev))
                    for k in range(LEVELS)]

        lists = (levels(rgb, 3, torch.float32, True), levels(depth, 1, torch.float32, False),
                 levels(sky, 1, torch.bool, False), levels(normal, 3, torch.float32, False))
        out.append(lists)
        if first_level < LEVELS:
            maps.append(_map(_abi.CAMFRONT_RGB_U8 if u8 else _abi.CAMFRONT_RGB_F32, rgb, lists[0], H, W, True))
            if any(lv is not None for lv in lists[1][1:]):
                maps.append(_map(_abi.CAMFRONT_DEPTH, depth, lists[1], H, W, False))
            if any(lv is not None for lv in lists[2][1:]):
                maps.append(_map(_abi.CAMFRONT_SKY, sky, lists[2], H, W, False))
            if any(lv is not None for lv in lists[3][1:]):
                maps.append(_map(_abi.CAMFRONT_NORMAL, normal, lists[3], H, W, False))
    last_launches = 0
    if maps:
        made = C.c_int(0)
        table = (_abi.CamfrontMap * len(maps))(*maps)
        with _guard(dev):
            _lib.check(_entry("pings_camfront_pyramid")(table, len(maps), C.byref(made), _lib.stream_ptr(dev)),
                       "pings_camfront_pyramid")
        last_launches = made.value
    return out


def image_pyramid(rgb, depth=None, sky_mask=None, normal=None, first_level: int = 0):
    """`image_pyramids` for one camera: the four lists `(rgb_levels, depth_levels, sky_levels, normal_levels)`."""
    return image_pyramids([(rgb, depth, sky_mask, normal)], first_level)[0]


# ---------------------------------------------------------------- the mono-depth cloud
def _scratch(nbytes: int, dev) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


def _plane(name: str, t, dtype=torch.float32, size=None, dev=None) -> torch.Tensor:
    """[1,H,W] or [H,W] of `dtype` on the device -> contiguous [H,W]."""
    if not (_dev_tensor(t, dtype, dev) and (t.dim() == 2 or (t.dim() == 3 and int(t.shape[0]) == 1)) and t.numel() > 0
            and (size is None or tuple(t.shape[-2:]) == tuple(size))):
        raise _lib.PingsHipError(f"camfront_ops: {name} must be a {dtype} [1,H,W] or [H,W] device tensor"
                                 + (f" of {tuple(size)} pixels" if size else ""))
    return t.detach().reshape(t.shape[-2:]).contiguous()


def _doubles(values, n: int):
    return (C.c_double * n)(*(float(v) for v in values))


@torch.no_grad()
def align_mono_depth(pred, lidar_depth, min_range, max_range) -> torch.Tensor:
    """The fit of dataset/slam_dataset.py:369-390 on the device: over the pixels with `lidar > min_range`,
    `pred > min_range` and `lidar < 0.8 max_range` the least-squares line lidar = k pred + b from float64 sums.  Returns
    the device record float64 [5] = count, k, b, rmse before, rmse after; `count <= 100` gives k = 1, b = 0 (and rmse
    after NaN).  Two launches, no host read; bitwise the same from run to run."""
    p = _plane("pred", pred)
    d = _plane("lidar_depth", lidar_depth, size=p.shape, dev=p.device)
    dev = p.device
    rec = torch.empty(_abi.CAMFRONT_FIT_RECORD, dtype=torch.float64, device=dev)
    with _guard(dev):
        scratch = _scratch(_entry("pings_camfront_align_scratch_bytes")(), dev)
        _lib.check(_entry("pings_camfront_align")(p.data_ptr(), d.data_ptr(), p.numel(), float(min_range),
                                                  float(max_range), scratch.data_ptr(), rec.data_ptr(),
                                                  _lib.stream_ptr(dev)), "pings_camfront_align")
    return rec


def _cloud_into(p, img, record, K, T_c_l, min_range, max_range, depth_trunc, high_z, scratch, sky, gated, rows, count):
    H, W = (int(s) for s in p.shape)
    K = np.asarray(K, dtype=np.float64)
    T = np.linalg.inv(np.asarray(T_c_l, dtype=np.float64).reshape(4, 4))       # Open3D: extrinsic^-1 * camera points
    _lib.check(_entry("pings_camfront_mono_cloud")(
        p.data_ptr(), img.data_ptr(), H, W, None if record is None else record.data_ptr(),
        _doubles((K[0, 0], K[1, 1], K[0, 2], K[1, 2]), 4), _doubles(T[:3].reshape(-1), 12), float(min_range),
        float(max_range), float(depth_trunc), int(bool(high_z)), scratch.data_ptr(), sky.data_ptr(),
        None if gated is None else gated.data_ptr(), rows.data_ptr(), count.data_ptr(), _lib.stream_ptr(p.device)),
        "pings_camfront_mono_cloud")


def _image_u8(image, size=None) -> torch.Tensor:
    if not (_dev_tensor(image, torch.uint8) and image.dim() == 3 and int(image.shape[2]) == 3 and image.numel() > 0
            and (size is None or tuple(image.shape[:2]) == tuple(size))):
        raise _lib.PingsHipError("camfront_ops: the image must be a uint8 [H,W,3] device tensor of the depth's size")
    return image.detach().contiguous()


def _fit_record(record, dev):
    if record is None:
        return None
    if not (_dev_tensor(record, torch.float64, dev) and record.numel() >= 3 and record.is_contiguous()):
        raise _lib.PingsHipError("camfront_ops: the fit record is the float64 device tensor of `align_mono_depth`")
    return record


@torch.no_grad()
def mono_cloud(pred, image_u8, K_mat, T_c_l, min_range, max_range, depth_trunc, high_z: bool, record=None,
               with_depth: bool = False):
    """dataset/slam_dataset.py:388-447 for one camera, each step in the reference's order: `d = k pred + b` (float64
    from the device `record` of `align_mono_depth`, rounded to float32; no record: the prediction itself), the sky mask
    `d > 1.2 max_range` (d = 0 there), the range gates (`high_z`: `d > 0.8 max_range` and `d < 2 min_range` give 0,
    otherwise `d < 0.2 max_range`), and for every pixel with `0 < d < depth_trunc` a row `xyz, rgb`:
    xyz = T_c_l^-1 ((u - cx) d / fx, (v - cy) d / fy, d), rgb = byte / 255.  `K_mat` [3,3] and `T_c_l` [4,4] are host
    values.  Returns `(rows [H W, 6], count, sky [1,H,W] bool, depth)`: `count` is a device int64 [1], only the first
    `count` rows are written, in row-major pixel order; `depth` is the gated depth image [1,H,W] with `with_depth`,
    else `None`.  Three launches, no host read."""
    p = _plane("pred", pred)
    img = _image_u8(image_u8, p.shape)
    dev = p.device
    if img.device != dev:
        raise _lib.PingsHipError("camfront_ops.mono_cloud: the image and the depth are on different devices")
    record = _fit_record(record, dev)
    H, W = (int(s) for s in p.shape)
    with _guard(dev):
        rows = torch.empty((H * W, 6), dtype=torch.float32, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        sky = torch.empty((1, H, W), dtype=torch.bool, device=dev)
        gated = torch.empty((1, H, W), dtype=torch.float32, device=dev) if with_depth else None
        scratch = _scratch(_entry("pings_camfront_cloud_scratch_bytes")(H * W), dev)
        _cloud_into(p, img, record, K_mat, T_c_l, min_range, max_range, depth_trunc, high_z, scratch, sky, gated, rows,
                    count)
    return rows, count, sky, gated


def _average_into(rows, n_dev, voxel, scratch, out, offset, count, status):
    _lib.check(_entry("pings_camfront_voxel_average")(
        rows.data_ptr(), int(rows.shape[0]), None if n_dev is None else n_dev.data_ptr(), float(voxel),
        scratch.data_ptr(), out.data_ptr(), int(out.shape[0]), None if offset is None else offset.data_ptr(),
        count.data_ptr(), status.data_ptr(), _lib.stream_ptr(rows.device)), "pings_camfront_voxel_average")


@torch.no_grad()
def voxel_average(rows, voxel, n_dev=None, out=None, offset=None):
    """Open3D's `voxel_down_sample(voxel)` of a coloured cloud: `rows` float32 [N,6] (position, colour), of which the
    first `n_dev` (device int64 [1]; `None`: all) are live.  Cells come from the positions in float64 on the grid
    anchored at the minimum minus half a voxel; a cell's row is the mean of its rows over all six columns, summed in
    float64 in input order; cells come out in ascending cell key.  They are appended to `out` [cap,6] (`None`: a new
    [N,6] buffer) behind `offset` rows (device int64 [1]; `None`: 0), so cameras chain without the host.  Returns
    `(out, count, status)`: `count` a new device int64 [1] = offset + cells, `status` a device int32 [1] with
    `_abi.EVAL_EXTENT` (the cloud spans more than 2^21 cells on an axis) and `_abi.CAMFRONT_FULL` (`out` had no room for
    every cell).  No host read; bitwise the same from run to run."""
    voxel = float(voxel)
    if not (voxel > 0.0 and np.isfinite(voxel)):
        raise ValueError(f"voxel must be positive and finite, got {voxel}")
    if not (_dev_tensor(rows, torch.float32) and rows.dim() == 2 and int(rows.shape[1]) == 6 and rows.is_contiguous()
            and int(rows.shape[0]) > 0):
        raise _lib.PingsHipError("camfront_ops.voxel_average: rows must be a contiguous float32 [N>0,6] device tensor")
    dev = rows.device
    for name, t in (("n_dev", n_dev), ("offset", offset)):
        if t is not None and not (_dev_tensor(t, torch.int64, dev) and t.numel() == 1):
            raise _lib.PingsHipError(f"camfront_ops.voxel_average: {name} must be a device int64 [1]")
    if out is None:
        out = torch.empty((int(rows.shape[0]), 6), dtype=torch.float32, device=dev)
    elif not (_dev_tensor(out, torch.float32, dev) and out.dim() == 2 and int(out.shape[1]) == 6 and out.is_contiguous()
              and int(out.shape[0]) > 0):
        raise _lib.PingsHipError("camfront_ops.voxel_average: out must be a contiguous float32 [cap>0,6] device tensor")
    with _guard(dev):
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        scratch = _scratch(_entry("pings_camfront_voxel_scratch_bytes")(int(rows.shape[0])), dev)
        _average_into(rows, n_dev, voxel, scratch, out, offset, count, status)
    return out, count, status


@torch.no_grad()
def mono_frame(dataset, images_u8, pred_depth, lidar_depth=None, high_z=None):
    """The mono-depth block of `read_frame_with_loader` (dataset/slam_dataset.py:366-399, :432-477) for every camera of
    `dataset.cam_names` that `images_u8` names, in that order: the fit against the camera's LiDAR depth image
    (`lidar_depth[name]`, where there is one and the dataset is not `is_rgbd`), the cloud, and its voxel average at
    `config.vox_down_m`, appended to the frame's merged cloud at a device offset.  `images_u8`, `pred_depth` and
    `lidar_depth` are dicts by camera name of uint8 [H,W,3], float32 [1,H,W] and float32 [1,H,W] device tensors.
    `high_z` defaults to `dataset.loader.mono_depth_for_high_z`.

    Sets `dataset.cur_point_cloud_mono_depth` to the merged float32 [M,6] device cloud when the dataset is not `is_rgbd`
    and the last camera's fit had more than 100 pixels (a camera without LiDAR depth keeps k = 1, b = 0 and the flag);
    prints the rmse figures unless `dataset.silence`.  Returns `{name: sky mask bool [1,H,W]}` for `CamImage`.  ONE host
    read per frame: every camera's fit record and the merged count together."""
    cfg = dataset.config
    names = [n for n in dataset.cam_names if n in images_u8]
    if not names:
        return {}
    if high_z is None:
        high_z = bool(dataset.loader.mono_depth_for_high_z)
    lidar_depth = lidar_depth or {}
    is_rgbd = bool(dataset.is_rgbd)
    preds = [_plane(f"pred_depth[{n!r}]", pred_depth[n]) for n in names]
    dev = preds[0].device
    imgs = [_image_u8(images_u8[n], p.shape) for n, p in zip(names, preds)]
    lidars = [None if is_rgbd or lidar_depth.get(n) is None else
              _plane(f"lidar_depth[{n!r}]", lidar_depth[n], size=p.shape, dev=dev) for n, p in zip(names, preds)]
    if any(t.device != dev for t in preds + imgs):
        raise _lib.PingsHipError("camfront_ops.mono_frame: every image of a frame is on one device")
    ncam, most = len(names), max(p.numel() for p in preds)
    nrec = _abi.CAMFRONT_FIT_RECORD
    skies = {}
    with _guard(dev):
        words = torch.zeros(nrec * ncam + ncam + 1, dtype=torch.int64, device=dev)      # records | row counts so far
        records = words[:nrec * ncam].view(torch.float64).view(ncam, nrec)
        counts = words[nrec * ncam:]
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        merged = torch.empty((sum(p.numel() for p in preds), 6), dtype=torch.float32, device=dev)
        rows = torch.empty((most, 6), dtype=torch.float32, device=dev)
        kept = torch.zeros(1, dtype=torch.int64, device=dev)
        fit_scratch = _scratch(_entry("pings_camfront_align_scratch_bytes")(), dev)
        scratch = _scratch(max(_entry("pings_camfront_cloud_scratch_bytes")(most),
                               _entry("pings_camfront_voxel_scratch_bytes")(most)), dev)
        for c, (name, p, img, lid) in enumerate(zip(names, preds, imgs, lidars)):
            H, W = (int(s) for s in p.shape)
            if lid is not None:
                _lib.check(_entry("pings_camfront_align")(p.data_ptr(), lid.data_ptr(), p.numel(), float(cfg.min_range),
                                                          float(cfg.max_range), fit_scratch.data_ptr(),
                                                          records[c].data_ptr(), _lib.stream_ptr(dev)),
                           "pings_camfront_align")
            sky = skies[name] = torch.empty((1, H, W), dtype=torch.bool, device=dev)
            _cloud_into(p, img, records[c] if lid is not None else None, dataset.K_mats[name], dataset.T_c_l_mats[name],
                        cfg.min_range, cfg.max_range, cfg.local_map_radius, high_z, scratch, sky, None, rows, kept)
            _average_into(rows[:p.numel()], kept, cfg.vox_down_m, scratch, merged, counts[c:c + 1], counts[c + 1:c + 2],
                          status)
        _lib.note_sync("camfront_mono_frame")
        host = torch.cat([words, status.to(torch.int64)]).cpu()
    rec = host[:nrec * ncam].view(torch.float64).view(ncam, nrec).tolist()
    total, st = int(host[nrec * ncam + ncam]), int(host[-1])
    if st & _abi.EVAL_EXTENT:
        raise _lib.PingsHipError("camfront_ops.mono_frame: a camera's cloud spans more than 2**21 voxels on an axis")
    use = not is_rgbd
    for c, lid in enumerate(lidars):
        if lid is None:
            continue
        fitted = rec[c][0] > _abi.CAMFRONT_MIN_FIT
        if not getattr(dataset, "silence", True):
            print("mono depth rmse (m): ", rec[c][3])
            if fitted:
                print("depth fitting rmse (m): ", rec[c][4])
        if c == ncam - 1:
            use = fitted
    if use:
        dataset.cur_point_cloud_mono_depth = merged[:total].clone()
    return skies


# ---------------------------------------------------------------- the constructor
def _same_device(device, dev: torch.device) -> bool:
    try:
        d = torch.device(device)
    except (TypeError, RuntimeError):
        return False
    return d.type == dev.type and (d.index is None and dev.index == torch.cuda.current_device() or d.index == dev.index)


def cam_init(self, frame_id, rgb_image, K_mat, z_min=0.1, z_max=100.0, cam_id: str = "cam", img_down_rate=0,
             depth_image=None, normal_img=None, sky_mask=None, device="cuda", cam_pose=None, img_width=None,
             img_height=None, pyramid_level: int = 4):
    """`CamImage.__init__` (gaussian_splatting/utils/cameras.py:23-186).  The kept original runs with `rgb_image=None`
    and the image's size, which sets the matrices, the pose and the parameters and leaves the four lists empty; the
    lists, `depth_on`, `sky_mask_on`, `mono_normal_on` and `cur_best_level` are then set from `image_pyramid`, and the
    class's own `free_memory_under_levels(img_down_rate - 1)` runs last.  Levels below `img_down_rate` are never built.
    One departure from the reference: RGB level 0 is contiguous CHW, where the reference keeps its input's strides."""
    orig = getattr(type(self), "_pings___init___original", None)
    if orig is None:
        raise _lib.PingsHipError("camfront_ops.cam_init: no original constructor was kept (`camfront_ops.install` keeps "
                                 "it); it sets the camera's matrices and takes the inputs the HIP path does not")
    if not (pyramid_level == 4 and _frame_ok(rgb_image, depth_image, sky_mask, normal_img)
            and _same_device(device, rgb_image.device)):
        return orig(self, frame_id, rgb_image, K_mat, z_min, z_max, cam_id, img_down_rate, depth_image, normal_img,
                    sky_mask, device, cam_pose, img_width, img_height, pyramid_level)
    H, W = _rgb_size(rgb_image)
    orig(self, frame_id, None, K_mat, z_min, z_max, cam_id, img_down_rate, None, None, None, device, cam_pose, W, H,
         pyramid_level)
    down = int(img_down_rate)
    rgb, depth, sky, normal = image_pyramid(rgb_image, depth_image, sky_mask, normal_img,
                                            first_level=min(max(down, 0), LEVELS))
    self.depth_on = depth_image is not None
    self.sky_mask_on = sky_mask is not None
    self.mono_normal_on = normal_img is not None
    self.rgb_image_list[0:LEVELS] = rgb
    self.depth_image_list[0:LEVELS] = depth
    self.sky_mask_list[0:LEVELS] = sky
    self.normal_img_list[0:LEVELS] = normal
    self.cur_best_level = 0
    self.free_memory_under_levels(down - 1)


# ---------------------------------------------------------------- install
def install(cam_cls=None) -> None:
    """`from gaussian_splatting.utils.cameras import CamImage; install(cam_cls=CamImage)`: rebinds `CamImage.__init__` and
    keeps the original as `_pings___init___original` for the fallbacks and for `uninstall`.  Installing twice changes
    nothing."""
    if cam_cls is not None:
        _rebind(cam_cls, "__init__", cam_init)


def uninstall(cam_cls=None) -> None:
    """Puts the reference's own constructor back wherever `install` replaced it."""
    if cam_cls is not None:
        _restore(cam_cls, "__init__", cam_init)
