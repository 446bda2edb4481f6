"""Torch restatement of the reference's sample-pool functions, for tests/test_pool_ops.py and tools/make_pool_golden.py.

`sample` is `DataSampler.sample` (utils/data_sampler.py:18-264), `get_batch` is `Mapper.get_batch`
(utils/mapper.py:704-771), `transform` is `transform_batch_torch(pool, pose_diff[time_pool])` (utils/mapper.py:774-778,
utils/tools.py:903-921) and `window` is utils/mapper.py:429-438.  The random draws and index tensors are arguments, and
the arithmetic runs in `dtype`: float32 is the reference's own arithmetic, float64 the yardstick of the GPU tests (fed
the same float32 inputs and draws).
"""
from types import SimpleNamespace as NS

import torch

U = 2.0 ** -24      # unit round-off of float32

SAMPLE_CFG = dict(surface_sample_range_m=0.25, free_sample_begin_ratio=0.3, free_sample_end_dist_m=1.0,
                  dist_weight_scale=0.8, max_range=60.0)

# name -> (P, (ns, nf, nb), dist_weight_on, behind_dropoff_on, colour channels | None, normals, labels, origin point)
GOLDEN_SAMPLE = {
    "p65_321": (65, (3, 2, 1), True, True, 3, True, True, False),
    "p257_012": (257, (0, 1, 2), False, True, 1, False, False, False),
    "p64_403": (64, (4, 0, 3), True, False, None, True, False, False),
    "p1_000": (1, (0, 0, 0), True, True, 4, False, True, False),
    "p63_320_origin": (63, (3, 2, 0), True, True, 4, True, True, True),
}
# name -> (bs, bs_new_sample, local indices, new_idx rows (None: no new_idx), lose_track, colour, normals, labels)
GOLDEN_BATCH = {
    "local_new": (257, 31, True, 40, False, True, True, True),
    "plain": (256, 0, False, None, False, False, False, False),
    "new_empty": (255, 16, True, 0, False, True, False, True),
    "lose_track": (64, 16, True, 40, True, False, True, False),
}
# name -> (N, pose dtype, ts dtype)
GOLDEN_TRANSFORM = {"f64_i32": (257, "float64", "int32"), "f32_i64": (255, "float32", "int64")}
POOL_ROWS, POSES = 1000, 50


def sample_cfg(ns, nf, nb, dist_weight_on, behind_dropoff_on, **kw):
    return NS(surface_sample_n=ns, free_front_n=nf, free_behind_n=nb, dist_weight_on=dist_weight_on,
              behind_dropoff_on=behind_dropoff_on, **{**SAMPLE_CFG, **kw})


def sample_inputs(P, channels, normals, labels, origin_point, seed):
    """float32 points (1 m .. 55 m from the sensor), unit normals, labels 0..19, colours in [0, 1] (CPU tensors)."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(P, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    pts = (d * (1.0 + 54.0 * torch.rand(P, 1, generator=g))).float()
    if origin_point:
        pts[P // 2] = 0.0
    nrm = torch.randn(P, 3, generator=g)
    nrm = (nrm / nrm.norm(dim=1, keepdim=True)).float() if normals else None
    sem = torch.randint(0, 20, (P,), generator=g, dtype=torch.int32) if labels else None
    col = torch.rand(P, channels, generator=g) if channels else None
    return pts, nrm, sem, col


def sample(cfg, points, normal, sem, color, noise, dtype=torch.float32):
    """-> (coord, sdf_label, normal, sem, color, weight), coord / sdf_label / weight in `dtype`."""
    z_s, u_f, u_b = (t.to(dtype).reshape(-1, 1) for t in noise)
    pts = points.to(dtype)
    ns, nb, nf = cfg.surface_sample_n, cfg.free_behind_n, cfg.free_front_n
    S = ns + nb + nf + 1
    rng, end, begin = cfg.surface_sample_range_m, cfg.free_sample_end_dist_m, cfg.free_sample_begin_ratio
    P = pts.shape[0]
    dist = torch.linalg.norm(pts, dim=1, keepdim=True)
    disp0, ratio0 = torch.zeros_like(dist), torch.ones_like(dist)
    disp_s = z_s * rng
    ratio_s = disp_s / dist.repeat(ns, 1) + 1.0
    sigma_ratio = 2.0
    rd = dist.repeat(nf, 1)
    free_max = 1.0 - sigma_ratio * rng / rd
    ratio_f = u_f * (free_max - begin) + begin
    disp_f = (ratio_f - 1.0) * rd
    rd = dist.repeat(nb, 1)
    free_max = end / rd + 1.0
    behind_min = 1.0 + sigma_ratio * rng / rd
    ratio_b = u_b * (free_max - behind_min) + behind_min
    disp_b = (ratio_b - 1.0) * rd
    disp = torch.cat((disp0, disp_s, disp_f, disp_b), 0)
    ratio = torch.cat((ratio0, ratio_s, ratio_f, ratio_b), 0)
    rd = dist.repeat(S, 1)
    coord = pts.repeat(S, 1) * ratio
    weight = torch.ones_like(rd)
    n_surf = P * (ns + 1)
    if cfg.dist_weight_on:
        weight[:n_surf] = 1 + cfg.dist_weight_scale * 0.5 - (rd[:n_surf] / cfg.max_range) * cfg.dist_weight_scale
    if cfg.behind_dropoff_on:
        dropoff_min, dropoff_max = 0.2 * end, end
        w = torch.clamp((dropoff_max - disp) / (dropoff_max - dropoff_min), min=0.0, max=1.0)
        weight = weight * (w * 0.8 + 0.2)
    weight[n_surf:] *= -1.0
    ray = lambda t, c: t.reshape(S, -1, c).transpose(0, 1).reshape(-1, c)  # noqa: E731
    out_n = None if normal is None else ray(normal.repeat(S, 1), 3)
    out_s = None
    if sem is not None:
        free = torch.zeros(P * (nf + nb), dtype=torch.float32, device=sem.device)
        out_s = ray(torch.cat((sem.repeat(ns + 1).float(), free), 0).int().reshape(-1, 1), 1).reshape(-1)
    out_c = None
    if color is not None:
        C = color.shape[1]
        free = -torch.ones(P * (nf + nb), C, dtype=color.dtype, device=color.device)
        out_c = ray(torch.cat((color.repeat(ns + 1, 1), free), 0), C)
    return ray(coord, 3), ray(disp, 1).reshape(-1) * -1, out_n, out_s, out_c, ray(weight, 1).reshape(-1)


def get_batch(m, r_hist, r_new=None):
    """`m`: namespace with the mapper's pool attributes, `config.bs` / `config.bs_new_sample`, `dataset`.  The index
    chain of the reference with the `randint` results given: (coord, sdf_label, ts, normal, sem, color, weight)."""
    local = m.local_sample_indices
    if (m.config.bs_new_sample > 0 and m.new_idx is not None and not m.dataset.lose_track
            and not m.dataset.stop_status):
        if m.new_idx.shape[0] > 0:
            hist = local[r_hist] if local is not None else r_hist
            index = torch.cat((hist, m.new_idx[r_new]), dim=0)
        else:
            index = r_hist
    else:
        index = local[r_hist] if local is not None else r_hist
    pick = lambda t: None if t is None else t[index]  # noqa: E731
    return (m.global_coord_pool[index, :], m.sdf_label_pool[index], m.time_pool[index], pick(m.normal_label_pool),
            pick(m.sem_label_pool), pick(m.color_pool), m.weight_pool[index])


def draw_sizes(m):
    """((n_hist, high_hist), (n_new, high_new) | None): the shapes and bounds of the reference's `randint` calls."""
    local = m.local_sample_indices
    count = local.shape[0] if local is not None else m.pool_sample_count
    if (m.config.bs_new_sample > 0 and m.new_idx is not None and not m.dataset.lose_track
            and not m.dataset.stop_status):
        k = m.new_idx.shape[0]
        if k > 0:
            bs_new = min(k, m.config.bs_new_sample)
            return (m.config.bs - bs_new, count), (bs_new, k)
        return (m.config.bs, m.pool_sample_count), None
    return (m.config.bs, count), None


def transform(points, ts, pose_diff, dtype=torch.float32):
    """`transform_batch_torch(points, pose_diff[ts])` in `dtype`; the poses are rounded to the points' float32 first."""
    tr = pose_diff[ts.long()]
    rot = tr[:, :3, :3].to(points).to(dtype)
    trans = tr[:, :3, 3:].to(points).to(dtype)
    return (torch.bmm(rot, points.to(dtype).unsqueeze(-1)) + trans).squeeze(-1)


def window_dist(pool, origin, range_filter_2d):
    """Distances of utils/mapper.py:429-434 in float64 from the float32 difference `pool - origin`."""
    rel = (pool - origin.to(pool)).double()
    return torch.norm(rel[:, :2], p=2, dim=1) if range_filter_2d else torch.norm(rel, p=2, dim=1)


def window(pool, origin, radius, range_filter_2d):
    return torch.nonzero(window_dist(pool, origin, range_filter_2d) < radius).reshape(-1)


def pool_state(rows, color, normals, labels, seed, device="cpu"):
    """A pool of `rows` samples as the mapper holds it."""
    g = torch.Generator().manual_seed(seed)
    m = NS(global_coord_pool=torch.randn(rows, 3, generator=g) * 20.0, sdf_label_pool=torch.randn(rows, generator=g),
           time_pool=torch.randint(0, POSES, (rows,), generator=g, dtype=torch.int32),
           weight_pool=torch.randn(rows, generator=g),
           normal_label_pool=torch.randn(rows, 3, generator=g) if normals else None,
           sem_label_pool=torch.randint(0, 20, (rows,), generator=g, dtype=torch.int32) if labels else None,
           color_pool=torch.rand(rows, 3, generator=g) if color else None,
           local_sample_indices=None, new_idx=None, pool_sample_count=rows, device=torch.device(device))
    for k, v in list(vars(m).items()):
        if isinstance(v, torch.Tensor):
            setattr(m, k, v.to(device))
    return m


def batch_state(bs, bs_new_sample, local, new_rows, lose_track, color, normals, labels, seed, rows=POOL_ROWS,
                device="cpu"):
    m = pool_state(rows, color, normals, labels, seed, device)
    g = torch.Generator().manual_seed(seed + 1)
    if local:
        m.local_sample_indices = torch.nonzero(torch.rand(rows, generator=g) < 0.4).reshape(-1).to(device)
    if new_rows is not None:
        m.new_idx = (rows - 1 - torch.randperm(min(rows, 60), generator=g)[:new_rows].sort().values).flip(0).to(device)
    m.config = NS(bs=bs, bs_new_sample=bs_new_sample)
    m.dataset = NS(lose_track=lose_track, stop_status=False)
    return m


def rigid_poses(T, dtype, seed):
    """[T,4,4] rigid corrections: rotations of up to ~0.2 rad, translations of a few metres."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(T, 3, generator=g, dtype=torch.float64) * 0.1
    K = torch.zeros(T, 3, 3, dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 2] = -w[:, 2], w[:, 1], -w[:, 0]
    K = K - K.transpose(1, 2)
    pose = torch.eye(4, dtype=torch.float64).repeat(T, 1, 1)
    pose[:, :3, :3] = torch.linalg.matrix_exp(K)
    pose[:, :3, 3] = torch.randn(T, 3, generator=g, dtype=torch.float64) * 3.0
    return pose.to(getattr(torch, dtype) if isinstance(dtype, str) else dtype)
