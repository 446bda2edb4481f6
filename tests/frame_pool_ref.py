"""Torch restatement of the body of the reference's `Mapper.process_frame` (utils/mapper.py:186-447), for
tests/test_frame_pool.py and tools/make_frame_pool_golden.py.

`process_frame` runs on a stand-in mapper (`mapper_state`) whose `sampler`, `dynamic_filter` and `neural_points` are the
stubs below; the capacity filter's `torch.randint` result is an argument, and the transforms run in `dtype`: float32 is
the reference's own arithmetic, float64 the yardstick of the GPU tests (fed the same float32 inputs).  `append`,
`filter_pool` and `select_update` are the three blocks on their own.
"""
from types import SimpleNamespace as NS

import torch

import pool_ref as PR

U = PR.U
POOLS = ("global_coord_pool", "sdf_label_pool", "weight_pool", "time_pool", "sem_label_pool", "color_pool",
         "normal_label_pool")
SECTIONS = (3, 2, 1)            # surface, front, behind samples per point: S = 7 rows per point
POINTS = 45                     # points per frame: 315 sample rows

# name -> colour channels, labels, normals, filter_dynamic, from_sample_points, from_all_samples, pose dtype, 2-D window
SEQUENCES = {
    "rgb_labels": dict(color=3, labels=True, normals=False, dynamic=False, from_samples=True, all_samples=False,
                       pose="float64", range_2d=False),
    "plain": dict(color=0, labels=False, normals=False, dynamic=False, from_samples=True, all_samples=False,
                  pose="float32", range_2d=True),
    "dynamic_gray_normals": dict(color=1, labels=False, normals=True, dynamic=True, from_samples=True,
                                 all_samples=False, pose="float64", range_2d=False),
    "all_samples_rgb_normals": dict(color=3, labels=True, normals=True, dynamic=True, from_samples=True,
                                    all_samples=True, pose="float32", range_2d=False),
    "frame_points": dict(color=3, labels=False, normals=True, dynamic=False, from_samples=False, all_samples=False,
                         pose="float64", range_2d=True),
}
FRAMES = 5
CFG = dict(pool_filter_freq=2, pool_capacity=500, bs_new_sample=0, window_radius=30.0, map_surface_ratio=0.5,
           prune_map_on=False, prune_freq_frame=100, monodepth_on=False, max_prune_certainty=2.0)


def frame_cfg(seq, device="cpu", **kw):
    """The configuration fields `process_frame` and the sampler read, for sequence description `seq`."""
    ns, nf, nb = SECTIONS
    return NS(device=device, color_channel=seq["color"], from_sample_points=seq["from_samples"],
              from_all_samples=seq["all_samples"], range_filter_2d=seq["range_2d"], surface_sample_n=ns,
              free_front_n=nf, free_behind_n=nb, dist_weight_on=True, behind_dropoff_on=True,
              **{**PR.SAMPLE_CFG, **CFG, **kw})


def frame_inputs(seq, frame, seed):
    """(point cloud [P,3+C], labels | None, normals | None, pose [4,4], static mask [P]) of one frame (CPU)."""
    pts, nrm, sem, col = PR.sample_inputs(POINTS, seq["color"] or None, seq["normals"], seq["labels"], False,
                                          seed=1000 * seed + frame)
    pc = pts if col is None else torch.cat((pts, col), 1).contiguous()
    pose = PR.rigid_poses(1, seq["pose"], seed=7 * seed + frame)[0]
    pose[:3, 3] = pose[:3, 3] * 0.5 + torch.tensor([1.5 * frame, 0.0, 0.0], dtype=pose.dtype)
    g = torch.Generator().manual_seed(31 * seed + frame)
    static = torch.rand(POINTS, generator=g) > 0.2
    return pc, sem, nrm, pose.contiguous(), static


class Sampler:
    """`DataSampler.sample` stand-in: the restatement of tests/pool_ref.py with noise seeded by the call number, so the
    reference, the restatement and the library see the same samples; keeps what it was given and what it returned."""

    def __init__(self, config, seed):
        self.config, self.seed, self.calls = config, seed, []

    def sample(self, points, normal, sem, color, color_valid_mask=None):
        cfg = self.config
        P = points.shape[0]
        g = torch.Generator().manual_seed(self.seed + len(self.calls))
        noise = tuple(t.to(points.device) for t in (torch.randn(P * cfg.surface_sample_n, 1, generator=g),
                                                    torch.rand(P * cfg.free_front_n, 1, generator=g),
                                                    torch.rand(P * cfg.free_behind_n, 1, generator=g)))
        out = tuple(None if t is None else t.contiguous()
                    for t in PR.sample(cfg, points.contiguous(), normal, sem, color, noise))
        self.calls.append(((points, normal, sem, color), out))
        return out


class MapRecorder:
    """`neural_points` stand-in: keeps the arguments of every call."""

    def __init__(self):
        self.updates, self.resets, self.memory = [], [], 0

    def reset_local_map(self, origin, orientation, frame_id):
        self.resets.append((origin, orientation, frame_id))

    def update(self, points, colors, normals, origin, orientation, frame_id):
        self.updates.append((points, colors, normals, origin, orientation, frame_id))

    def record_memory(self, verbose=True, record_footprint=True):
        self.memory += 1


def mapper_state(cfg, seed, device="cpu", dtype=torch.float32):
    """A stand-in `self` with the attributes `Mapper.__init__` gives the pool (utils/mapper.py:110-130)."""
    dev = torch.device(device)
    m = NS(config=cfg, silence=True, device=dev, dataset=NS(static_mask=None, lose_track=False, stop_status=False),
           sampler=Sampler(cfg, seed), neural_points=MapRecorder(), sdf_train_frame_count=0, cur_sample_count=0,
           pool_sample_count=0, local_sample_indices=None, new_idx=None, static_mask=None, next_static=None,
           global_coord_pool=torch.empty((0, 3), device=dev, dtype=dtype),
           sdf_label_pool=torch.empty((0,), device=dev), weight_pool=torch.empty((0,), device=dev),
           time_pool=torch.empty((0,), device=dev, dtype=torch.int),
           sem_label_pool=torch.empty((0,), device=dev, dtype=torch.int),
           color_pool=torch.empty((0, cfg.color_channel), device=dev),
           normal_label_pool=torch.empty((0, 3), device=dev))
    m.dynamic_filter = lambda points, type_2_on=True: m.next_static     # the frame's stored mask
    return m


def transform(points, pose, dtype=torch.float32, rotate_only=False):
    """`transform_torch(points, pose)` (utils/tools.py:888-900) in `dtype`; the pose is rounded to float32 first."""
    T = pose.to(points).to(dtype)
    out = points.to(dtype) @ T[:3, :3].T
    return out if rotate_only else out + T[:3, 3]


def transform_bound(points, pose, rotate_only=False):
    """4u (sum_j |R_ij| |p_j| + |t_i|): three products and three sums."""
    T = pose.to(torch.float32).double().to(points.device)
    b = points.double().abs() @ T[:3, :3].abs().T
    return 4 * U * (b if rotate_only else b + T[:3, 3].abs())


def select_update(coord, sdf_label, color, normal, pose, thr=None, dtype=torch.float32):
    """utils/mapper.py:262-284 for the sampled rows: (points, colours | None, normals | None)."""
    if thr is not None:
        mask = torch.abs(sdf_label) < thr
        coord = coord[mask, :]
        color = None if color is None else color[mask, :]
        normal = None if normal is None else normal[mask, :]
    return (transform(coord, pose, dtype), color,
            None if normal is None else transform(normal, pose, dtype, rotate_only=True))


def append(m, coord, sdf_label, normal_label, sem_label, color_label, weight, pose, frame_id, dtype=torch.float32):
    """utils/mapper.py:340-366."""
    time_repeat = torch.tensor(frame_id, dtype=torch.int, device=coord.device).repeat(coord.shape[0])
    m.weight_pool = torch.cat((m.weight_pool, weight), 0)
    m.sdf_label_pool = torch.cat((m.sdf_label_pool, sdf_label), 0)
    m.time_pool = torch.cat((m.time_pool, time_repeat), 0)
    m.sem_label_pool = None if sem_label is None else torch.cat((m.sem_label_pool, sem_label), 0)
    m.color_pool = None if color_label is None else torch.cat((m.color_pool, color_label), 0)
    m.normal_label_pool = None if normal_label is None else torch.cat((m.normal_label_pool, normal_label), 0)
    m.global_coord_pool = torch.cat((m.global_coord_pool, transform(coord, pose, dtype)), 0)


def filter_mask(rows, capacity, draw):
    """The mask of utils/mapper.py:386-399 with the `randint` result given (None at or under the capacity)."""
    mask = torch.ones(rows, dtype=torch.bool, device=None if draw is None else draw.device)
    if rows > capacity:
        assert draw.shape == (rows - capacity,)
        mask[draw] = False
    return mask


def filter_pool(m, draw):
    """utils/mapper.py:386-423."""
    mask = filter_mask(m.global_coord_pool.shape[0], m.config.pool_capacity, draw).to(m.global_coord_pool.device)
    for name in POOLS:
        t = getattr(m, name)
        if t is not None:
            setattr(m, name, t[mask])
    m.cur_sample_count = int(mask[-m.cur_sample_count:].sum())
    m.pool_sample_count = int(mask.sum())


def process_frame(m, point_cloud, frame_label, frame_normal, pose, frame_id, filter_dynamic=False, draw=None,
                  dtype=torch.float32):
    """utils/mapper.py:186-447 (no mono-depth branch, `bs_new_sample == 0`)."""
    cfg = m.config
    origin, orientation = pose[:3, 3], pose[:3, :3]
    points = point_cloud[:, :3]
    m.static_mask = torch.ones(points.shape[0], dtype=torch.bool, device=point_cloud.device)
    if filter_dynamic:
        m.neural_points.reset_local_map(origin, orientation, frame_id)
        m.static_mask = m.dynamic_filter(transform(points, pose, dtype))
        points = points[m.static_mask]
    color = None
    if cfg.color_channel > 0:
        color = point_cloud[:, 3:]
        if filter_dynamic:
            color = color[m.static_mask]
    if frame_label is not None and filter_dynamic:
        frame_label = frame_label[m.static_mask]
    if frame_normal is not None:
        frame_normal = frame_normal[m.static_mask]
    m.dataset.static_mask = m.static_mask
    coord, sdf_label, normal_label, sem_label, color_label, weight = m.sampler.sample(points, frame_normal,
                                                                                      frame_label, color)
    m.sdf_train_frame_count += 1
    m.cur_sample_count = sdf_label.shape[0]
    m.pool_sample_count = m.sdf_label_pool.shape[0]
    if cfg.from_sample_points:
        thr = None if cfg.from_all_samples else cfg.surface_sample_range_m * cfg.map_surface_ratio
        upd = select_update(coord, sdf_label, None if color is None else color_label,
                            None if frame_normal is None else normal_label, pose, thr, dtype)
    else:
        upd = select_update(points, None, color, frame_normal, pose, None, dtype)
    m.neural_points.update(*upd, origin, orientation, frame_id)
    m.neural_points.record_memory(verbose=not m.silence, record_footprint=True)
    append(m, coord, sdf_label, normal_label, sem_label, color_label, weight, pose, frame_id, dtype)
    if (frame_id + 1) % cfg.pool_filter_freq == 0:
        filter_pool(m, draw)
    else:
        m.cur_sample_count = coord.shape[0]
        m.pool_sample_count = m.global_coord_pool.shape[0]
    m.local_sample_indices = PR.window(m.global_coord_pool.float(), origin.to(m.global_coord_pool.device),
                                       cfg.window_radius, cfg.range_filter_2d)


def discard_count(m, frame_id, incoming_rows):
    """Size of the capacity filter's draw after `incoming_rows` more rows (0: no `randint` call)."""
    if (frame_id + 1) % m.config.pool_filter_freq:
        return 0
    return max(int(m.global_coord_pool.shape[0]) + incoming_rows - m.config.pool_capacity, 0)
