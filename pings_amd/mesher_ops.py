"""Mesher bulk query on the HIP device: `Mesher.query_points` (utils/mesher.py:40-166).

The reference walks the marching-cubes grid in batches of `bs` points through `query_feature` (hash search, top-k,
feature gather, IDW weights), the SDF decoder and a weighted sum, copying every batch to the host.  Here each batch is
one launch of the fused kNN + SDF kernel (`pings_sdf_forward`, csrc/knn_sdf.hip) writing straight into device-resident
result arrays; the host copy happens once at the end.  The colour and semantic heads (`query_color`, `query_sem`) run
HIP `query_feature`, the head's decoder through the fused MFMA kernels and one activation + IDW-sum (+ arg-max) pass
(`pings_head_reduce`).  Same arguments and the same 4-tuple
(sdf_pred, sem_pred, color_pred, mc_mask) with the reference's container types: numpy float64 arrays, or CPU float32
tensors with `out_torch=True`.  `install(mesher_module)` rebinds the method.

Marching cubes (`Mesher.mc_mesh`, skimage on the host in the reference) runs on the device too: `marching_cubes`
(csrc/mc.hip), the drop-ins `mc_mesh` / `mc_mesh_torch` (`install(M, mc=True)`), and `mesh_bbx`, one
chunk from box to mesh without a host copy of the grid."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _abi, _lib
from . import neural_points as _np


def head_reduce(raw: torch.Tensor, w_knn, mode: int):
    """`pings_head_reduce` (csrc/heads.hip): raw = decoder outputs [B, k, C] (per-neighbour) or [B, C] (`weighted_first`),
    w_knn = IDW weights [B, k, 1] or None.  mode _abi.HEAD_COLOR -> colours [B, C] (any k); _abi.HEAD_SEMANTIC -> int64
    labels [B] (the kernel for k <= 16, the reference's torch composition on the device beyond)."""
    L = _lib.lib()
    raw = raw.detach().to(torch.float32).contiguous()
    if raw.dim() == 2:
        B, k, Cn, w = raw.shape[0], 1, raw.shape[1], None
    else:
        B, k, Cn = raw.shape
        w = None if w_knn is None else w_knn.detach().to(torch.float32).reshape(B, k).contiguous()
    dev = raw.device
    if mode == _abi.HEAD_SEMANTIC and k > 16:
        # the semantic kernel holds one log-sum-exp and one weight per neighbour in registers (k <= 16); a larger
        # query_nn_k takes the reference's composition (Decoder.sem_label_prob, decoder.py:119-122, then the IDW sum)
        if not raw.is_cuda:
            raise _lib.PingsHipError("pings_amd ops run on the HIP device only (got a CPU tensor); "
                                     "there is no CPU fallback")
        prob = torch.log_softmax(raw, dim=-1)
        prob = prob.sum(dim=1) if w is None else (prob * w.unsqueeze(-1)).sum(dim=1)
        return torch.argmax(prob, dim=1)
    val = torch.empty(B, Cn, device=dev) if mode == _abi.HEAD_COLOR else None
    lab = torch.empty(B, dtype=torch.int64, device=dev) if mode == _abi.HEAD_SEMANTIC else None
    _lib.check(L.pings_head_reduce(_lib.ptr(raw), _lib.ptr(w), B, k, Cn, mode, _lib.ptr(val), _lib.ptr(lab),
                                   _lib.stream_ptr(dev)), "pings_head_reduce")
    return val if mode == _abi.HEAD_COLOR else lab


def _query_device(self, coord, bs, query_sdf=True, query_sem=False, query_color=False, query_mask=True,
                  query_locally=False, mask_min_nn_count: int = 4):
    """The batch loop of `query_points` with its results left on the device: (sdf, sem, color, mask) tensors or None."""
    if not coord.is_cuda:
        raise _lib.PingsHipError("Mesher.query_points runs on the HIP device only (got a CPU tensor); "
                                 "there is no CPU fallback")
    from . import decoder as _dec

    n = coord.shape[0]
    dev = coord.device
    npm = self.neural_points
    sdf = torch.zeros(n, device=dev) if query_sdf else None
    sem = torch.zeros(n, device=dev) if query_sem else None
    mask = torch.zeros(n, device=dev) if query_mask else None
    channels = getattr(self.config, "color_channel", 3)
    color = torch.zeros(n, channels, device=dev) if query_color else None
    with torch.no_grad():
        for k in range(math.ceil(n / bs) if n else 0):
            head, tail = k * bs, min((k + 1) * bs, n)
            x = coord[head:tail]
            if query_sdf or query_mask:
                # points without any neighbour get sdf 0 (mesher.py:118-131: zeros outside pred_mask).  With
                # weighted_first the fused kernel returns the decoder's value of an all-zero feature there (what the
                # tracker's un-masked query needs), so the mask is applied here
                s, _, cnt, _ = _np.sdf_fused(npm, self.sdf_mlp, x, need_grad=False, need_certainty=False,
                                             query_locally=query_locally, use_only_valid_points=True)
                if query_sdf:
                    sdf[head:tail] = torch.where(cnt >= 1, s, torch.zeros_like(s))
                if query_mask:
                    mask[head:tail] = (cnt >= mask_min_nn_count).to(mask.dtype)
            if query_color or query_sem:
                # vertex colouring / labelling (mesher.py:132-153, :420): HIP `query_feature`, the head's decoder on the
                # matrix cores (`decoder.mlp`, csrc/mlp.hip) and ONE pass for activation + IDW sum (+ arg-max)
                # (`pings_head_reduce`, csrc/heads.hip) — no torch tail
                gf, cf, w_knn, _, _ = npm.query_feature(x, accumulate_stability=False, query_locally=query_locally,
                                                        query_geo_feature=bool(query_sem), query_color_feature=bool(query_color),
                                                        use_only_valid_points=True)
                wk = None if self.config.weighted_first else w_knn
                if query_color:
                    color[head:tail] = head_reduce(_dec.mlp(self.color_mlp, cf), wk, _abi.HEAD_COLOR)
                if query_sem:
                    sem[head:tail] = head_reduce(_dec.mlp(self.sem_mlp, gf), wk, _abi.HEAD_SEMANTIC).to(sem.dtype)
    return sdf, sem, color, mask


def query_points(self, coord, bs, query_sdf=True, query_sem=False, query_color=False, query_mask=True,
                 query_locally=False, mask_min_nn_count: int = 4, out_torch: bool = False):
    sdf, sem, color, mask = _query_device(self, coord, bs, query_sdf, query_sem, query_color, query_mask, query_locally,
                                          mask_min_nn_count)
    if out_torch:
        host = lambda t: None if t is None else t.cpu()
    else:
        host = lambda t: None if t is None else t.cpu().numpy().astype(np.float64)
    return host(sdf), host(sem), host(color), host(mask)


# ------------------------------------------------------------------ marching cubes (utils/mesher.py:363-389, :570-581)
def marching_cubes(volume: torch.Tensor, level: float = 0.0, mask=None, allow_degenerate: bool = False,
                   gradient_direction: str = "descent"):
    """The surface `volume == level` of a device [nx, ny, nz] grid (csrc/mc.hip, rules in DESIGN §2.7): verts [V, 3]
    fp32 in index units, faces [F, 3] int64, both on the device.  `mask` (any dtype, nonzero = true, the volume's
    shape) gates each cell by its lowest corner.  One host read per call (the two totals)."""
    if gradient_direction not in ("descent", "ascent"):
        raise ValueError(f"gradient_direction must be 'descent' or 'ascent', got {gradient_direction!r}")
    if not volume.is_cuda:
        raise _lib.PingsHipError("marching_cubes runs on the HIP device only (got a CPU tensor); "
                                 "there is no CPU fallback")
    if volume.dim() != 3:
        raise ValueError(f"marching_cubes needs a 3-D volume, got shape {tuple(volume.shape)}")
    dev = volume.device
    vol = volume.detach().to(torch.float32).contiguous()
    nx, ny, nz = (int(d) for d in vol.shape)
    empty = torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int64, device=dev)
    if vol.numel() == 0:
        return empty
    m = None
    if mask is not None:
        if tuple(mask.shape) != (nx, ny, nz):
            raise ValueError(f"mask shape {tuple(mask.shape)} differs from the volume's {(nx, ny, nz)}")
        if not mask.is_cuda:
            raise _lib.PingsHipError("marching_cubes: the mask must be on the HIP device")
        m = (mask.detach() != 0).to(torch.uint8).contiguous()
    flags = (_abi.MC_ALLOW_DEGENERATE if allow_degenerate else 0) | (_abi.MC_ASCENT if gradient_direction == "ascent" else 0)
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    scratch = torch.empty(L.pings_mc_scratch_bytes(nx, ny, nz), dtype=torch.uint8, device=dev)
    tot = (C.c_int64 * 2)(0, 0)
    _lib.note_sync("mc_count")
    _lib.check(L.pings_mc_count(_lib.ptr(vol), _lib.ptr(m), nx, ny, nz, float(level), flags, _lib.ptr(scratch), tot, st),
               "pings_mc_count")
    nv, nf = int(tot[0]), int(tot[1])
    if nv == 0:
        return empty
    keys = torch.empty(nv, dtype=torch.int64, device=dev)
    verts = torch.empty(nv, 3, device=dev)
    faces = torch.empty(nf, 3, dtype=torch.int64, device=dev)
    _lib.check(L.pings_mc_emit(_lib.ptr(vol), _lib.ptr(m), nx, ny, nz, float(level), flags, _lib.ptr(scratch), nv, nf,
                               _lib.ptr(keys), _lib.ptr(verts), _lib.ptr(faces), st), "pings_mc_emit")
    return verts, faces


def _device(self):
    dev = getattr(self, "cur_device", None) or getattr(self, "device", None)
    dev = torch.device(dev) if dev is not None else torch.device("cuda", torch.cuda.current_device())
    return dev if dev.type == "cuda" else torch.device("cuda", torch.cuda.current_device())


def mc_mesh(self, mc_sdf, mc_mask, voxel_size, mc_origin):
    """`Mesher.mc_mesh` (mesher.py:363-389) on the device: numpy grid and mask in, numpy (verts, faces) out, verts in
    world units.  No surface: the reference's `except` return, zeros((0, 3)) for both (verts shifted by the origin)."""
    dev = _device(self)
    vol = torch.from_numpy(np.ascontiguousarray(mc_sdf, dtype=np.float32)).to(dev)
    mask = None if mc_mask is None else torch.from_numpy(np.ascontiguousarray(mc_mask)).to(dev)
    verts, faces = marching_cubes(vol, 0.0, mask, allow_degenerate=False)
    if faces.shape[0] == 0:
        return mc_origin + np.zeros((0, 3)) * voxel_size, np.zeros((0, 3))
    return mc_origin + verts.cpu().numpy() * voxel_size, faces.cpu().numpy()


def mc_mesh_torch(self, mc_sdf, mc_mask, voxel_size, mc_origin):
    """The `Mesher.mc_mesh_torch` that `recon_aabb_mesh(use_torch_mc=True)` calls (mesher.py:570-581): CPU or device
    tensors in, device (verts in world units, fp32 origin + verts * voxel_size; faces int64) out."""
    dev = mc_sdf.device if mc_sdf.is_cuda else _device(self)
    vol = mc_sdf.to(dev, torch.float32)
    mask = None if mc_mask is None else mc_mask.to(dev)
    verts, faces = marching_cubes(vol, 0.0, mask, allow_degenerate=False)
    origin = torch.as_tensor(mc_origin).to(dev, torch.float32)
    return origin + verts * voxel_size, faces


def grid_from_bbx(bbx_min, bbx_max, voxel_size, pad_voxel=0, skip_top_voxel=0, device=None):
    """`Mesher.get_query_from_bbx` (mesher.py:168-212) on the device: (coord [N, 3] fp32, voxel_num_xyz, voxel_origin),
    or (None, None, None) past the reference's 5e8-point cap."""
    min_bound, max_bound = np.asarray(bbx_min, dtype=np.float64), np.asarray(bbx_max, dtype=np.float64)
    num = (np.ceil((max_bound - min_bound) / voxel_size) + pad_voxel * 2).astype(np.int_)
    origin = min_bound - pad_voxel * voxel_size
    origin[2] -= voxel_size          # one extra voxel underground
    num[2] += 1
    num[2] -= skip_top_voxel
    if num[0] * num[1] * num[2] > 5e8:
        return None, None, None
    ax = [torch.arange(int(k), dtype=torch.int16, device=device) for k in num]
    x, y, z = torch.meshgrid(*ax, indexing="ij")
    coord = torch.stack((x.flatten(), y.flatten(), z.flatten())).transpose(0, 1).float()
    coord *= voxel_size
    coord += torch.tensor(origin, dtype=torch.float32, device=device)
    return coord, num, origin


def mesh_bbx(self, bbx_min, bbx_max, voxel_size, query_locally=False, mesh_min_nn=10):
    """One mesher chunk on the device (recon_aabb_mesh, mesher.py:540-581, without Open3D): the grid by
    `get_query_from_bbx`'s rule with config.pad_voxel / skip_top_voxel, the fused SDF + mask query, marching cubes.
    -> (verts [V, 3] fp32 world units, faces [F, 3] int64) on the device, or None past the 5e8-point cap."""
    cfg = self.config
    coord, num, origin = grid_from_bbx(bbx_min, bbx_max, voxel_size, cfg.pad_voxel, cfg.skip_top_voxel, _device(self))
    if coord is None:
        return None
    sdf, _, _, mask = _query_device(self, coord, cfg.infer_bs, True, False, False, getattr(cfg, "mc_mask_on", True),
                                    query_locally, mesh_min_nn)
    shape = tuple(int(k) for k in num)
    verts, faces = marching_cubes(sdf.view(shape), 0.0, None if mask is None else mask.view(shape))
    return torch.tensor(origin, dtype=torch.float32, device=coord.device) + verts * voxel_size, faces


def label_vertices(self, verts, query_locally=False):
    """Semantic labels of mesh vertices (`estimate_vertices_sem`, mesher.py:398-401): the batch loop of `query_points`
    with `query_sem` alone, -> int64 [V] on the device."""
    if getattr(self, "sem_mlp", None) is None:
        raise ValueError("label_vertices: the mesher has no semantic decoder (sem_mlp)")
    _, sem, _, _ = _query_device(self, verts, self.config.infer_bs, False, True, False, False, query_locally)
    return sem.to(torch.int64)


def color_table(color_map, device=None):
    """(table uint8 [T, 3], valid bool [T]) of a {label: (r, g, b)} dict such as the reference's
    `sem_kitti_color_map`, T = the largest label + 1: the `label_colors` argument of `mesh_ops.recon_mesh`."""
    keys = [int(k) for k in color_map]
    if not keys or min(keys) < 0:
        raise ValueError("color_table: the colour map needs at least one entry and no negative label")
    table = np.zeros((max(keys) + 1, 3), dtype=np.uint8)
    valid = np.zeros(max(keys) + 1, dtype=bool)
    for k, rgb in color_map.items():
        rgb = np.asarray(rgb)
        if rgb.shape != (3,) or (rgb < 0).any() or (rgb > 255).any() or (rgb != np.floor(rgb)).any():
            raise ValueError(f"color_table: label {k} needs three integers in 0..255, got {rgb!r}")
        table[int(k)], valid[int(k)] = rgb, True
    return torch.from_numpy(table).to(device), torch.from_numpy(valid).to(device)


def recon_mesh(self, aabbs, voxel_size, **kw):
    """`Mesher.recon_mesh`: `mesh_ops.recon_mesh`, the finished mesh as device tensors.  After
    `install(..., semantic=True)` a call with `estimate_sem` gets the installed colour table unless it passes one."""
    from . import mesh_ops

    if aabbs is None:
        return None
    if kw.get("estimate_sem") and kw.get("label_colors") is None:
        kw["label_colors"] = _installed_table(self)
    return mesh_ops.recon_mesh(self, aabbs, voxel_size, **kw)


def _installed_table(self):
    """The colour table `install(..., semantic=True)` read, on the mesher's device (uploaded once per device)."""
    host = getattr(type(self), "_pings_label_colors", None)
    if host is None:
        raise ValueError("estimate_sem needs a colour table: install(mesher_module, finish=True, semantic=True), or "
                         "pass label_colors")
    dev = _device(self)
    cache = type(self)._pings_label_colors_device
    if dev not in cache:
        cache[dev] = tuple(t.to(dev) for t in host)
    return cache[dev]


def _finished(original, semantic=False):
    def recon_aabb_collections_mesh(self, aabbs, voxel_size, mesh_path=None, query_locally=False, estimate_sem=False,
                                    estimate_color=False, mesh_normal=True, filter_isolated_mesh=False,
                                    filter_free_space_vertices=True, mesh_min_nn=10, use_torch_mc=False):
        from . import mesh_ops

        if estimate_sem and not semantic:     # not asked for: the labelled mesh stays the reference's
            return original(self, aabbs, voxel_size, mesh_path, query_locally, estimate_sem, estimate_color, mesh_normal,
                            filter_isolated_mesh, filter_free_space_vertices, mesh_min_nn, use_torch_mc)
        mesh = recon_mesh(self, aabbs, voxel_size, query_locally=query_locally, estimate_color=estimate_color,
                          mesh_normal=mesh_normal, filter_isolated_mesh=filter_isolated_mesh, mesh_min_nn=mesh_min_nn,
                          mesh_path=mesh_path, estimate_sem=estimate_sem,
                          filter_free_space_vertices=filter_free_space_vertices)
        return None if mesh is None else mesh_ops.to_open3d(mesh)

    recon_aabb_collections_mesh._pings_original = original
    return recon_aabb_collections_mesh


def install(mesher_module, mc: bool = False, finish: bool = False, semantic: bool = False) -> None:
    """`import utils.mesher as M; install(M)`: Mesher.query_points -> one fused kernel launch per batch.  With mc=True
    also Mesher.mc_mesh and Mesher.mc_mesh_torch -> marching cubes on the device (csrc/mc.hip).  With finish=True also
    Mesher.recon_aabb_collections_mesh -> `mesh_ops.recon_mesh` (csrc/mesh.hip) returned through `mesh_ops.to_open3d`
    (the saved original with `estimate_sem`), and a new Mesher.recon_mesh for callers that want the device tensors.
    With finish=True and semantic=True a call with `estimate_sem` takes that route too (csrc/mesh_label.hip): the colour
    table is built here, once, from `mesher_module.sem_kitti_color_map`, the dict the reference's module imports."""
    if semantic and not finish:
        raise ValueError("install: semantic=True routes recon_aabb_collections_mesh(estimate_sem=True) and needs "
                         "finish=True")
    mesher_module.Mesher.query_points = query_points
    if mc:
        mesher_module.Mesher.mc_mesh = mc_mesh
        mesher_module.Mesher.mc_mesh_torch = mc_mesh_torch
    if finish:
        if semantic:
            color_map = getattr(mesher_module, "sem_kitti_color_map", None)
            if not isinstance(color_map, dict):
                raise ValueError("install: semantic=True needs the module's sem_kitti_color_map dict")
            mesher_module.Mesher._pings_label_colors = color_table(color_map)
            mesher_module.Mesher._pings_label_colors_device = {}
        current = getattr(mesher_module.Mesher, "recon_aabb_collections_mesh", None)
        original = getattr(current, "_pings_original", current)
        mesher_module.Mesher.recon_aabb_collections_mesh = _finished(original, semantic)
        mesher_module.Mesher.recon_mesh = recon_mesh
