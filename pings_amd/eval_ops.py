"""View evaluation on the HIP device (csrc/eval.hip): the figures `Mapper.gs_eval_offline`
(utils/mapper.py:1950-2056) and eval/eval_mesh_utils.py report per evaluated view, without Open3D and without a host
loop of one KD-tree query per point.

  view_metrics       PSNR, SSIM, depth L1 and depth RMSE of one view: one streaming kernel, one host read
  backproject_depth  rendered depth (+ colour) -> world points, Open3D's RGBD rules, row-major pixel order
  voxel_centroids    Open3D `voxel_down_sample`: the mean of each occupied cell, grid anchored at min - voxel/2
  nn_distance        exact nearest neighbour below `max_dist` through a sorted cell grid
  eval_pair          the reference's eleven Chamfer / F-score figures; the whole call reads one record
  eval_mesh          box crop + surface sample of a mesh (mesh_ops.sample_surface), then eval_pair's body
  crop_intersection  the ground-truth points near every predicted mesh's sampled surface; one host read
  install(module)    rebinds `eval_pair` and `nn_correspondance` of eval/eval_mesh_utils.py, and the two above on request

The raw operators take fp32 tensors on the HIP device and raise for anything else: there is no CPU fallback.  Counts
that only a later stage needs stay on the device; every host read goes through `_read`, which notes it in
`_lib.sync_counts()` under an `eval_` name."""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple

import numpy as np
import torch

from . import _abi, _lib

PAIR_KEYS = ("MAE_accuracy(m)", "MAE_completeness(m)", "Chamfer_L1(m)", "Chamfer_L2(m)", "Precision[Accuracy](%)",
             "Recall[Completeness](%)", "F-score(%)", "Spacing(m)", "Inlier_threshold(m)", "Outlier_truncation_acc(m)",
             "Outlier_truncation_com(m)")


class ViewMetrics(NamedTuple):
    psnr: float
    ssim: float         # NaN with ssim=False
    depth_l1: float     # NaN without depth images or on an empty mask
    depth_rmse: float
    n_valid: int        # pixels under the depth mask


def _read(t: torch.Tensor, what: str) -> torch.Tensor:
    """The one place where this module waits for device values."""
    _lib.note_sync("eval_" + what)
    return t.cpu()


def _device_f32_all(*specs) -> list:
    """Every (name, tensor, shapes) checked as an fp32 HIP tensor of one of `shapes` (None = any extent; a None tensor
    passes as None): ValueError for a shape, TypeError for a type, then PingsHipError for a CPU tensor, all before any
    GPU work."""
    for name, t, dims in specs:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
        if not any(t.dim() == len(d) and all(w is None or w == s for w, s in zip(d, t.shape)) for d in dims):
            raise ValueError(f"{name} must have shape {' or '.join(str(list(d)) for d in dims)}, got {list(t.shape)}")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
    for name, t, _ in specs:
        if t is not None and not t.is_cuda:
            raise _lib.PingsHipError(f"{name}: pings_amd.eval_ops runs on the HIP device only (got a CPU tensor); "
                                     "there is no CPU fallback")
    return [None if t is None else t.detach().contiguous() for _, t, _ in specs]


def _device_f32(name: str, t, dims) -> torch.Tensor:
    return _device_f32_all((name, t, dims))[0]


def _positive(name: str, v) -> float:
    v = float(v)
    if not (v > 0.0 and np.isfinite(v)):
        raise ValueError(f"{name} must be positive and finite, got {v}")
    return v


def _scratch(nbytes: int, dev) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


# ------------------------------------------------------------------ view metrics (mapper.py:1950-1982)
def view_metrics_record(rendered_rgb, gt_rgb, rendered_depth=None, gt_depth=None, rendered_alpha=None, *, depth_min,
                        depth_max, min_alpha=None, ssim=True) -> torch.Tensor:
    """The device record behind `view_metrics`, not read: float64 [EVAL_VIEW_RECORD] = psnr, ssim, depth_l1,
    depth_rmse, n_valid, mse of channels 0..3 (NaN past the image's channels)."""
    shape = tuple(getattr(rendered_rgb, "shape", ()))
    if len(shape) != 3 or not 1 <= shape[0] <= 4 or shape[1] * shape[2] == 0:
        raise ValueError(f"rendered_rgb must be [1..4, H, W] and not empty, got {list(shape)}")
    Cn, H, W = (int(s) for s in shape)
    maps = [(1, H, W), (H, W)]
    with_depth = rendered_depth is not None and gt_depth is not None
    with_alpha = with_depth and rendered_alpha is not None and min_alpha is not None
    rgb, gt, depth, gtd, alpha = _device_f32_all(
        ("rendered_rgb", rendered_rgb, [shape]), ("gt_rgb", gt_rgb, [shape]),
        ("rendered_depth", rendered_depth if with_depth else None, maps),
        ("gt_depth", gt_depth if with_depth else None, maps),
        ("rendered_alpha", rendered_alpha if with_alpha else None, maps))
    dev = rgb.device
    L = _lib.lib()
    s = None
    if ssim:
        from .ssim import fused_ssim
        s = fused_ssim(rgb.unsqueeze(0), gt.unsqueeze(0), train=False).reshape(1)
    rec = torch.empty(_abi.EVAL_VIEW_RECORD, dtype=torch.float64, device=dev)
    scratch = _scratch(L.pings_eval_view_metrics_scratch_bytes(H * W), dev)
    _lib.check(L.pings_eval_view_metrics(_lib.ptr(rgb), _lib.ptr(gt), Cn, H * W, _lib.ptr(depth), _lib.ptr(gtd),
                                         _lib.ptr(alpha), float(depth_min), float(depth_max),
                                         float(min_alpha) if alpha is not None else 0.0, int(alpha is not None),
                                         _lib.ptr(s), _lib.ptr(scratch), _lib.ptr(rec), _lib.stream_ptr(dev)),
               "pings_eval_view_metrics")
    return rec


def view_metrics(rendered_rgb, gt_rgb, rendered_depth=None, gt_depth=None, rendered_alpha=None, *, depth_min,
                 depth_max, min_alpha=None, ssim=True) -> ViewMetrics:
    """PSNR (the reference's: per channel 20 log10(1 / sqrt(mse)), then the mean), SSIM (`fused_ssim(train=False)`),
    and depth L1 / RMSE under the reference's mask (four strict comparisons with depth_min / depth_max, and
    alpha > min_alpha when both are given).  Images [C, H, W], depths and alpha [1, H, W] or [H, W], fp32 on the
    device.  One host read."""
    rec = _read(view_metrics_record(rendered_rgb, gt_rgb, rendered_depth, gt_depth, rendered_alpha,
                                    depth_min=depth_min, depth_max=depth_max, min_alpha=min_alpha, ssim=ssim),
                "view_metrics").tolist()
    return ViewMetrics(rec[0], rec[1], rec[2], rec[3], int(rec[4]))


# ------------------------------------------------------------------ back-projection (mapper.py:1987-2013)
def _host_matrix(m) -> np.ndarray:
    if isinstance(m, torch.Tensor):
        m = _read(m.detach(), "extrinsic") if m.is_cuda else m.detach()
        m = m.numpy()
    m = np.asarray(m, dtype=np.float64)
    if m.shape != (4, 4):
        raise ValueError(f"extrinsic must be 4x4, got {m.shape}")
    return m


def backproject_device(depth, K, extrinsic, depth_trunc, *, rgb=None, alpha=None, min_alpha=None):
    """`backproject_depth` without its host read: (points [H*W, 3], colors [H*W, 3] or None, count) where count is a
    device int64 [1] and only the first `count` rows are written.  `eval_pair(..., pred_count=count)` takes them."""
    if not isinstance(depth, torch.Tensor):
        raise TypeError(f"depth must be a torch tensor, got {type(depth).__name__}")
    if depth.dim() not in (2, 3) or (depth.dim() == 3 and depth.shape[0] != 1) or depth.numel() == 0:
        raise ValueError(f"depth must be [1, H, W] or [H, W] and not empty, got {list(depth.shape)}")
    H, W = (int(s) for s in depth.shape[-2:])
    if len(K) != 4:
        raise ValueError("K must be (fx, fy, cx, cy)")
    maps = [(1, H, W), (H, W)]
    d, col, a = _device_f32_all(("depth", depth, maps), ("rgb", rgb, [(3, H, W)]),
                                ("alpha", alpha if min_alpha is not None else None, maps))
    T = np.linalg.inv(_host_matrix(extrinsic))           # Open3D: points = extrinsic^-1 * camera points
    dev = d.device
    L = _lib.lib()
    points = torch.empty(H * W, 3, device=dev)
    colors = torch.empty(H * W, 3, device=dev) if col is not None else None
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = _scratch(L.pings_eval_backproject_scratch_bytes(H * W), dev)
    k4 = (C.c_double * 4)(*(float(v) for v in K))
    t12 = (C.c_double * 12)(*T[:3].reshape(-1).tolist())
    _lib.check(L.pings_eval_backproject(_lib.ptr(d), _lib.ptr(col), _lib.ptr(a), H, W, k4, t12, float(depth_trunc),
                                        float(min_alpha) if a is not None else 0.0, int(a is not None),
                                        _lib.ptr(scratch), _lib.ptr(points), _lib.ptr(colors), _lib.ptr(count),
                                        _lib.stream_ptr(dev)), "pings_eval_backproject")
    return points, colors, count


def backproject_depth(depth, K, extrinsic, depth_trunc, *, rgb=None, alpha=None, min_alpha=None):
    """Open3D's `create_from_color_and_depth(depth_scale=1, depth_trunc, convert_rgb_to_intensity=False)` +
    `create_from_rgbd_image(intrinsic, extrinsic)` on the device: a pixel gives a point iff 0 < d < depth_trunc (and
    alpha > min_alpha when both are given); z = d, x = (u - cx) z / fx, y = (v - cy) z / fy, then extrinsic^-1.
    -> points [M, 3], and with `rgb` [3, H, W] also colors [M, 3] = floor(rgb * 255) / 255; row-major pixel order.
    `extrinsic` is host data (array, list or CPU tensor).  One host read (M)."""
    points, colors, count = backproject_device(depth, K, extrinsic, depth_trunc, rgb=rgb, alpha=alpha,
                                               min_alpha=min_alpha)
    m = int(_read(count, "backproject_count")[0])
    return points[:m] if colors is None else (points[:m], colors[:m])


# ------------------------------------------------------------------ voxel centroids, nearest neighbour
def _status(dev) -> torch.Tensor:
    return torch.zeros(1, dtype=torch.int32, device=dev)


def _raise_on_status(status: int) -> None:
    if status & _abi.EVAL_EXTENT:
        raise _lib.PingsHipError("eval_ops: a cloud spans more than 2**21 cells on an axis and cannot be filed; "
                                 "use a larger voxel / cell or crop the cloud")


def _voxel(points, n_dev, voxel, status):
    """-> (centroids [cap, 3], count device int64 [1]); rows past count are not written."""
    dev = points.device
    n = points.shape[0]
    L = _lib.lib()
    out = torch.empty(n, 3, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = _scratch(L.pings_eval_voxel_scratch_bytes(n), dev)
    _lib.check(L.pings_eval_voxel_centroids(_lib.ptr(points), n, _lib.ptr(n_dev), voxel, _lib.ptr(scratch),
                                            _lib.ptr(out), _lib.ptr(count), _lib.ptr(status), _lib.stream_ptr(dev)),
               "pings_eval_voxel_centroids")
    return out, count


def voxel_centroids(points, voxel) -> torch.Tensor:
    """Open3D `voxel_down_sample(voxel)`: grid anchored at min_bound - voxel/2, cell floor((p - anchor) / voxel), the
    mean of each occupied cell's points in ascending linear cell key (x fastest).  [N, 3] -> [M, 3]; bitwise the same
    from run to run.  One host read (M)."""
    voxel = _positive("voxel", voxel)
    p = _device_f32("points", points, [(None, 3)])
    if p.shape[0] == 0:
        return p.new_zeros(0, 3)
    status = _status(p.device)
    out, count = _voxel(p, None, voxel, status)
    m, st = _read(torch.cat([count, status.to(torch.int64)]), "voxel_count").tolist()
    _raise_on_status(st)
    return out[:m]


def default_cell(max_dist: float, spacing=None) -> float:
    """Cell size of the search grid: max(2 * spacing hint, max_dist / 8), so at most 8 rings are walked."""
    return max(2.0 * float(spacing) if spacing else 0.0, max_dist / 8.0)


def _nn(src, n_dev, dst, m_dev, cell, max_dist, status):
    dev = src.device
    n, m = src.shape[0], dst.shape[0]
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    scratch = _scratch(L.pings_eval_nn_scratch_bytes(m), dev)
    _lib.check(L.pings_eval_nn_build(_lib.ptr(dst), m, _lib.ptr(m_dev), cell, _lib.ptr(scratch), _lib.ptr(status), st),
               "pings_eval_nn_build")
    dist = torch.empty(n, device=dev)
    idx = torch.empty(n, dtype=torch.int64, device=dev)
    _lib.check(L.pings_eval_nn_query(_lib.ptr(src), n, _lib.ptr(n_dev), _lib.ptr(scratch), m, cell, max_dist,
                                     _lib.ptr(dist), _lib.ptr(idx), st), "pings_eval_nn_query")
    return dist, idx


def nn_distance(src, dst, max_dist, *, spacing=None, cell=None):
    """Exact nearest neighbour of every `src` [N, 3] point among `dst` [M, 3]: (dist [N] fp32, idx [N] int64), with
    dist = +inf and idx = -1 where no `dst` point lies at distance < max_dist; ties in fp32 distance go to the
    smallest index.  `spacing` is a hint of the clouds' point spacing for the cell size (`default_cell`), `cell`
    sets it outright.  No host read: a `dst` too wide for the grid (2**21 cells per axis) shows as NaN / -2 rows."""
    max_dist = _positive("max_dist", max_dist)
    cell = _positive("cell", cell) if cell is not None else default_cell(max_dist, spacing)
    s, d = _device_f32_all(("src", src, [(None, 3)]), ("dst", dst, [(None, 3)]))
    if s.device != d.device:
        raise ValueError("src and dst are on different devices")
    n, m = s.shape[0], d.shape[0]
    if n == 0 or m == 0:
        return (torch.full((n,), float("inf"), device=s.device),
                torch.full((n,), -1, dtype=torch.int64, device=s.device))
    return _nn(s, None, d, None, cell, max_dist, _status(s.device))


# ------------------------------------------------------------------ eval_pair (eval_mesh_utils.py:100-182)
def _as_cloud(x, name: str):
    """A checked [N, 3] cloud from a device tensor, a numpy array or any object with a `.points` array: a device fp32
    tensor, or still a host fp32 array (`_on_device` uploads it once the call knows that it has work to do)."""
    if hasattr(x, "points") and not isinstance(x, torch.Tensor):
        x = np.asarray(x.points)
    if isinstance(x, torch.Tensor):
        if x.dim() != 2 or x.shape[1] != 3:
            raise ValueError(f"{name} must have shape [N, 3], got {list(x.shape)}")
        if not x.is_cuda:
            raise _lib.PingsHipError(f"{name}: pings_amd.eval_ops runs on the HIP device only (got a CPU tensor); "
                                     "pass a device tensor or a numpy array")
        return x.detach().to(torch.float32).contiguous()
    a = np.asarray(x)
    if a.size == 0:
        a = a.reshape(0, 3)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"{name} must have shape [N, 3], got {list(a.shape)}")
    return np.ascontiguousarray(a, dtype=np.float32)


def _on_device(x, like=None) -> torch.Tensor:
    dev = like.device if isinstance(like, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
    return x.to(dev) if isinstance(x, torch.Tensor) else torch.from_numpy(x).to(dev)


def pair_metrics(record, down_sample_res, threshold, truncation_acc, truncation_com) -> dict:
    """The reference's eleven figures from the eight sums of `pings_eval_pair_reduce`, formed as numpy forms them
    (an empty side or 0 / 0 gives NaN)."""
    kp, sp, sp2, ip, kr, sr, sr2, ir = (np.float64(v) for v in record[:8])
    with np.errstate(all="ignore"):
        dist_p_mean, dist_r_mean = sp / kp, sr / kr
        chamfer_l1 = 0.5 * (dist_p_mean + dist_r_mean)
        chamfer_l2 = np.sqrt(0.5 * (sp2 / kp + sr2 / kr))
        precision, recall = ip / kp * 100.0, ir / kr * 100.0
        fscore = 2 * precision * recall / (precision + recall)
    vals = (dist_p_mean, dist_r_mean, chamfer_l1, chamfer_l2, precision, recall, fscore, down_sample_res, threshold,
            truncation_acc, truncation_com)
    return {k: float(v) for k, v in zip(PAIR_KEYS, vals)}


def eval_pair(pred_points, trgt_points, down_sample_res=0.02, threshold=0.05, truncation_acc=0.5, truncation_com=0.5,
              *, pred_count=None, trgt_count=None) -> dict:
    """The reference's `eval_pair`: both clouds voxel-down-sampled at `down_sample_res`, nearest-neighbour distances in
    both directions, then accuracy (pred -> trgt, distances >= truncation_acc dropped), completeness (trgt -> pred,
    distances >= truncation_com counted as truncation_com), Chamfer L1 / L2, precision, recall (d < threshold) and
    F-score, under the reference's eleven keys.  Clouds: device tensors, numpy arrays or objects with `.points`;
    `pred_count` / `trgt_count` (device int64 [1]) give the live length of a buffer such as `backproject_device`'s.
    The whole call reads one record."""
    res, thr = _positive("down_sample_res", down_sample_res), _positive("threshold", threshold)
    tacc, tcom = _positive("truncation_acc", truncation_acc), _positive("truncation_com", truncation_com)
    pred, trgt = _as_cloud(pred_points, "pred_points"), _as_cloud(trgt_points, "trgt_points")
    if pred.shape[0] == 0 or trgt.shape[0] == 0:
        # np.mean of an empty list on one side, and nn_correspondance returns nothing at all when either is empty
        return pair_metrics([0.0] * 8, down_sample_res, threshold, truncation_acc, truncation_com)
    pred = _on_device(pred, trgt)
    trgt = _on_device(trgt, pred)
    rec = _read(_pair_record(pred, pred_count, trgt, trgt_count, res, thr, tacc, tcom, _status(pred.device)),
                "pair").tolist()
    _raise_on_status(int(rec[10]))
    return pair_metrics(rec, down_sample_res, threshold, truncation_acc, truncation_com)


def _pair_record(pred, pred_count, trgt, trgt_count, res, thr, tacc, tcom, status) -> torch.Tensor:
    """The device work of `eval_pair` on two non-empty device clouds: the float64 [EVAL_PAIR_RECORD] record, not read.
    `status` (device int32 [1]) travels in it as entry 10, with whatever bits earlier stages OR-ed into it."""
    dev = pred.device
    P, np_dev = _voxel(pred, pred_count, res, status)
    T, nt_dev = _voxel(trgt, trgt_count, res, status)
    # queries arrive in cell order (the centroids' order), so neighbouring lanes walk the same rows
    dist_p, _ = _nn(P, np_dev, T, nt_dev, default_cell(tacc, res), tacc, status)
    dist_r, _ = _nn(T, nt_dev, P, np_dev, default_cell(tcom, res), tcom, status)
    L = _lib.lib()
    rec = torch.empty(_abi.EVAL_PAIR_RECORD, dtype=torch.float64, device=dev)
    _lib.check(L.pings_eval_pair_reduce(_lib.ptr(dist_p), P.shape[0], _lib.ptr(np_dev), _lib.ptr(dist_r), T.shape[0],
                                        _lib.ptr(nt_dev), thr, tcom, _lib.ptr(status), _lib.ptr(rec),
                                        _lib.stream_ptr(dev)), "pings_eval_pair_reduce")
    return rec


def nn_correspondance(verts1, verts2, truncation_dist, ignore_outlier=True):
    """The reference's `nn_correspondance`: for each vertex of `verts2` the nearest of `verts1` -> ([indices],
    [distances]).  A vertex with no neighbour below `truncation_dist` is left out, or with ignore_outlier=False kept
    with the truncation distance; its index is then -1 (the search stops at the truncation distance; the reference
    reports the far neighbour's index, which none of its callers uses).  One host read."""
    v1, v2 = _as_cloud(verts1, "verts1"), _as_cloud(verts2, "verts2")
    if v1.shape[0] == 0 or v2.shape[0] == 0:
        return [], []
    trunc = _positive("truncation_dist", truncation_dist)
    v2 = _on_device(v2, v1)
    v1 = _on_device(v1, v2)
    dist, idx = _nn(v2, None, v1, None, default_cell(trunc), trunc, _status(v2.device))
    both = _read(torch.stack([dist.to(torch.float64), idx.to(torch.float64)]), "nn_correspondance").numpy()
    d, i = both[0], both[1].astype(np.int64)
    if (i == -2).any():
        _raise_on_status(_abi.EVAL_EXTENT)
    far = ~np.isfinite(d)
    if ignore_outlier:
        return i[~far].tolist(), d[~far].tolist()
    return i.tolist(), np.where(far, trunc, d).tolist()


# ------------------------------------------------------------------ eval_mesh, crop_intersection (:8-60, :221-257)
def _as_mesh(x, name: str):
    """(verts fp32 [V, 3], faces int64 [F, 3]) on the device from a PLY path, a `mesh_ops.Mesh` or a (verts, faces) pair
    of device tensors or host arrays; float64 coordinates are rounded once, on upload."""
    from . import mesh_ops

    if isinstance(x, (str, os.PathLike)):
        ply = mesh_ops.read_ply(x)
        x = (ply["verts"], ply["faces"])
    elif isinstance(x, mesh_ops.Mesh):
        x = (x.verts, x.faces)
    if not (isinstance(x, (tuple, list)) and len(x) == 2):
        raise TypeError(f"{name} must be a PLY path, a mesh_ops.Mesh or a (verts, faces) pair, got {type(x).__name__}")
    v = _as_cloud(x[0], name + " vertices")
    f = x[1]
    if isinstance(f, torch.Tensor):
        if not f.is_cuda:
            raise _lib.PingsHipError(f"{name}: pings_amd.eval_ops runs on the HIP device only (got CPU faces); pass a "
                                     "device tensor or a numpy array")
        f = f.detach().to(torch.int64)
    else:
        f = np.ascontiguousarray(np.asarray(f).reshape(-1, 3), dtype=np.int64)
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"{name} faces must have shape [F, 3], got {list(f.shape)}")
    return v, f


def _as_target(x, name: str):
    if isinstance(x, (str, os.PathLike)):
        from . import mesh_ops
        x = mesh_ops.read_ply(x)["verts"]
    return _as_cloud(x, name)


def _raise_on_sample_status(status: int) -> None:
    from . import mesh_ops
    msg = mesh_ops.sample_status_error(status)
    if msg:
        raise _lib.PingsHipError(msg)


def eval_mesh(pred, trgt, down_sample_res=0.02, threshold=0.05, truncation_acc=0.50, truncation_com=0.50,
              gt_bbx_mask_on=True, mesh_sample_point=20000000, possion_sample_on=True, possion_sample_init_factor=5,
              *, seed=0) -> dict:
    """The reference's `eval_mesh` (same signature, spelling included): the predicted mesh cropped to the target's
    bounding box (z widened by `down_sample_res` at both ends, with `gt_bbx_mask_on`), `mesh_sample_point` points
    sampled on its surface in proportion to triangle area, then `eval_pair` of that cloud against the target.
    `pred`: a PLY path, a `mesh_ops.Mesh` or a (verts, faces) pair; `trgt`: a PLY path or any cloud `eval_pair` takes.
    The box is formed on the device and the crop is fused into the sampler (`mesh_ops.sample_surface`), so the whole call
    makes one host read: the pair record, which carries the sampler's status.  A mesh that leaves no sample gives what
    `eval_pair` gives for an empty `pred`.
    Poisson-disk elimination (Open3D's sequential priority-queue pass) is not built.  `possion_sample_on` is accepted
    as long as `down_sample_res > 0`: the area-stratified sample serves it, since the voxel down-sampling at
    `down_sample_res` that follows is what makes the scored cloud uniform; `possion_sample_init_factor` has no effect.
    With `possion_sample_on=True` and `down_sample_res <= 0` the call raises NotImplementedError."""
    from . import mesh_ops

    if possion_sample_on and not float(down_sample_res) > 0.0:
        raise NotImplementedError("eval_mesh: Poisson-disk sample elimination is not built; it is only stood in for by "
                                  "the voxel down-sampling of down_sample_res > 0")
    res, thr = _positive("down_sample_res", down_sample_res), _positive("threshold", threshold)
    tacc, tcom = _positive("truncation_acc", truncation_acc), _positive("truncation_com", truncation_com)
    n = int(mesh_sample_point)
    if not 0 < n <= 2**31 - 1:
        raise ValueError(f"mesh_sample_point must lie in [1, 2**31 - 1], got {n}")
    verts, faces = _as_mesh(pred, "pred")
    target = _as_target(trgt, "trgt")
    empty = pair_metrics([0.0] * 8, down_sample_res, threshold, truncation_acc, truncation_com)
    if verts.shape[0] == 0 or faces.shape[0] == 0 or target.shape[0] == 0:
        return empty
    like = next((t for t in (verts, faces, target) if isinstance(t, torch.Tensor)), None)
    target = _on_device(target, like)
    verts, faces = _on_device(verts, target), _on_device(faces, target)
    box = None
    if gt_bbx_mask_on:
        box = torch.stack([target.amin(0), target.amax(0)]).double()       # exact: fp32 -> fp64
        box[0, 2] -= res
        box[1, 2] += res
    status = _status(target.device)
    sample = mesh_ops.sample_surface(verts, faces, n, seed=seed, box=box, status=status)
    rec = _read(_pair_record(sample.points, sample.count, target, None, res, thr, tacc, tcom, status), "pair").tolist()
    _raise_on_sample_status(int(rec[10]))
    _raise_on_status(int(rec[10]))
    if rec[8] == 0.0:                                                      # no live sample: the empty-pred answer
        return empty
    return pair_metrics(rec, down_sample_res, threshold, truncation_acc, truncation_com)


def crop_intersection(gt, preds, out_file_crop=None, dist_thre=0.1, mesh_sample_point=1000000, *, seed=0):
    """The reference's `crop_intersection`: the ground-truth points that lie closer than `dist_thre` (strictly, the
    search's own rule) to the sampled surface of every predicted mesh in `preds`.  `gt`: a PLY path or a cloud; each
    entry of `preds` as `eval_mesh` takes it.  Survival is chained on the device as one flag per ground-truth point (a
    point already dropped is still queried, which changes no result), the flags are compacted once at the end, and the
    samplers' status words travel with the count: one host read.  -> the kept [K, 3] device tensor in the order of
    `gt`, also written to `out_file_crop` as a PLY cloud when that is given."""
    from . import lidar_ops, mesh_ops

    thre = _positive("dist_thre", dist_thre)
    n = int(mesh_sample_point)
    if not 0 < n <= 2**31 - 1:
        raise ValueError(f"mesh_sample_point must lie in [1, 2**31 - 1], got {n}")
    cloud = _as_target(gt, "gt")
    meshes = [_as_mesh(p, f"preds[{k}]") for k, p in enumerate(preds)]
    cloud = _on_device(cloud, next((v for v, _ in meshes if isinstance(v, torch.Tensor)), None))
    dev = cloud.device
    G = cloud.shape[0]
    alive = torch.ones(G, dtype=torch.bool, device=dev)
    status = _status(dev)
    for verts, faces in meshes:
        if G == 0:
            break
        if verts.shape[0] == 0 or faces.shape[0] == 0:
            alive.zero_()                                   # nothing to be near to
            continue
        sample = mesh_ops.sample_surface(_on_device(verts, cloud), _on_device(faces, cloud), n, seed=seed,
                                         status=status)
        dist, _ = _nn(cloud, None, sample.points, sample.count, default_cell(thre), thre, status)
        alive &= torch.isfinite(dist)
    # kept rows first and in order, by a stable sort of the flags: their number is the call's one read
    rows = torch.argsort(~alive, stable=True)
    k, st = _read(torch.cat([alive.sum().reshape(1), status.to(torch.int64)]), "crop_intersection").tolist()
    _raise_on_sample_status(st)
    _raise_on_status(st)
    kept, = lidar_ops.select_rows(rows[:k].contiguous(), cloud)
    if out_file_crop is not None:
        mesh_ops.write_ply(out_file_crop, kept, np.zeros((0, 3), dtype=np.int64))
    return kept


def install(eval_mesh_utils_module, mesh=False) -> None:
    """`import eval.eval_mesh_utils as E; install(E)`: E.eval_pair and E.nn_correspondance -> the device versions; with
    `mesh=True` also E.eval_mesh and E.crop_intersection."""
    eval_mesh_utils_module.eval_pair = eval_pair
    eval_mesh_utils_module.nn_correspondance = nn_correspondance
    if mesh:
        eval_mesh_utils_module.eval_mesh = eval_mesh
        eval_mesh_utils_module.crop_intersection = crop_intersection
