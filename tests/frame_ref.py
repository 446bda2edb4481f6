"""Torch restatement of the mapper's per-frame point tests, for tests/test_frame_ops.py and tools/make_frame_golden.py.

`new_samples` is the block `if self.config.bs_new_sample > 0:` of `Mapper.process_frame` (utils/mapper.py:447-513),
`dynamic_filter` / `dynamic_filter_neural_points` are :528-585 and `check_invalid_neural_points` is :1636-1655, written
on `oracle.sdf_cpu` (`NeuralPointMap`, `MLP`, `get_gradient`).  With a float32 map they are the reference's lines op for
op (what the fixtures pin with `torch.equal`); `decisions` evaluates the compared quantities in float64 from the same
float32 inputs and says which rows lie too close to a threshold to be decided (the threshold bands of the GPU tests).

The maps are the reference's own (tests/golden/sdf_<case>.npz, written by oracle/make_golden.py); `dress` replaces the
certainty tables by the ones of the scenario, and `stand_in` is the mapper the functions run on.
"""
import math
from types import SimpleNamespace as NS

import numpy as np
import torch

from oracle import sdf_cpu

CASES = ("gs_f32", "pin_f8")            # per-neighbour decoding, F = 32 / weighted-first, F = 8
CHUNK = 512                             # rows a wave owns in pings_frame_new_count (csrc/frame.hip: kChunk)
FIXTURE_ROWS = 8 * CHUNK + 7            # rows of the frame in the fixtures
SIZES = (1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 65 * CHUNK + 7)   # the last: more than 64 per-wave counts
BAND = 1e-4                             # parity gate of the SDF query, relative to max |ref|

# Scenario scalars: name -> config of the stand-in mapper.  The decoders of the reference's maps are random, so their
# SDF lives in a narrow range around -0.03 (and is the same number at many points); the thresholds are placed inside
# the distribution of the quantity they cut and away from its clusters, which the CPU tests assert with `check_gates`.
# `dynamic_sdf_ratio_thre` is the one of the two dynamic filters; check_invalid_neural_points compares |sdf| and runs
# with CHECK_RATIO instead.
CONFIG = {
    "gs_f32": dict(voxel_size_m=0.25, new_certainty_thre=1.0, surface_sample_range_m=0.25, dynamic_certainty_thre=1.0,
                   dynamic_sdf_ratio_thre=-0.1224, dynamic_min_grad_norm_thre=0.02, infer_bs=300),
    "pin_f8": dict(voxel_size_m=0.4, new_certainty_thre=1.0, surface_sample_range_m=0.3, dynamic_certainty_thre=1.0,
                   dynamic_sdf_ratio_thre=-0.075, dynamic_min_grad_norm_thre=0.05, infer_bs=4096),
}
CHECK_RATIO = {"gs_f32": 0.124, "pin_f8": 0.057}
CHECK_MIN_NN = (6, 14)                  # the default, and a count inside the distribution of the stable rows
ADAPTIVE = dict(adaptive_iters=True, new_sample_ratio_less=0.02, new_sample_ratio_more=0.15,
                new_sample_ratio_restart=0.3, freeze_after_frame=30, bs_new_sample=2048)
STABILITY_THRESHOLD = 1.0               # the default of check_invalid_neural_points
HISTORY = 1000                          # pool rows in front of the frame's samples


def load_state(golden_dir, case):
    with np.load(golden_dir / f"sdf_{case}.npz") as z:
        return {k: z[k] for k in z.files}


# ---------------------------------------------------------------- scenario
def certainty_tables(st, seed=0):
    """(point_certainties [Np], local_point_certainties [Nl]) of the scenario.  Global: uniform in [0, 2), so the
    new-sample test sees both sides of its threshold.  Local: 4.0 for x > 0.6 and 0.25 elsewhere, so a queried
    certainty (a convex combination of its neighbours') is far from 1.0 except in a strip around x = 0.6, and the
    stable rows of check_invalid_neural_points are the right-hand part of the local map."""
    g = torch.Generator().manual_seed(1000 + seed)
    glob = (torch.rand(st["neural_points"].shape[0], generator=g) * 2.0).float()
    loc_x = torch.as_tensor(st["local_neural_points"])[:, 0]
    loc = torch.where(loc_x > 0.6, torch.tensor(4.0), torch.tensor(0.25)).float()
    return glob, loc


def dress(npm, cert_global, cert_local, config):
    """The scenario's certainty tables on an oracle map, and the `config` the HIP functions read from a map."""
    npm.point_certainties = cert_global.to(device=npm.device, dtype=npm.point_certainties.dtype)
    npm.local_point_certainties = cert_local.to(device=npm.device, dtype=npm.local_point_certainties.dtype)
    npm.config = config
    return npm


def frame_samples(st, n, seed):
    """(coord [n,3], sdf_label [n]) of a frame: samples around the map's points (negative coordinates included: the
    sheet is centred on the origin), one in eight displaced by a few metres into cells without a point, one in eight
    sent to a far cell that shares its table slot, and labels on both sides of 3 * surface_sample_range_m."""
    g = torch.Generator().manual_seed(seed)
    pts = torch.as_tensor(st["neural_points"])
    res = float(st["resolution"])
    coord = pts[torch.randint(0, pts.shape[0], (n,), generator=g)] + (torch.rand(n, 3, generator=g) - 0.5) * res
    far = torch.arange(n) % 8 == 5
    coord[far] += torch.tensor([0.0, 0.0, 7.0])
    # one in eight moved by +-buffer_size cells along x: the hash changes by a multiple of the table size, so the sample
    # finds the slot of the cell it came from, whose point is 50 km away (a hash collision beyond the one-cell distance)
    hit = torch.arange(n) % 8 == 3
    coord[hit, 0] += torch.where(torch.arange(n)[hit] % 16 == 3, 1.0, -1.0) * (float(st["buffer_size"]) * res)
    label = torch.randn(n, generator=g) * 0.6
    return coord.float().contiguous(), label.float().contiguous()


def frame_points(st, n, seed):
    """Query points of `dynamic_filter`: around the local points, one in sixteen 30 m away (no neighbour)."""
    g = torch.Generator().manual_seed(seed)
    pts = torch.as_tensor(st["local_neural_points"])
    res = float(st["resolution"])
    x = pts[torch.randint(0, pts.shape[0], (n,), generator=g)] + torch.randn(n, 3, generator=g) * (0.5 * res)
    x[torch.arange(n) % 16 == 9] += 30.0
    return x.float().contiguous()


def make_config(case, st, **kw):
    return NS(**{**CONFIG[case], **ADAPTIVE, "weighted_first": bool(st["weighted_first"]),
                 "query_nn_k": int(st["nn_k"]), "layer_norm_on": False, "num_nei_cells": 2,
                 "search_alpha": {"gs_f32": 0.8, "pin_f8": 0.5}[case], **kw})


def stand_in(npm, dec, config, device="cpu", **pool):
    """The attributes of `Mapper` the four functions read."""
    return NS(config=config, neural_points=npm, sdf_mlp=dec, device=torch.device(device), dtype=torch.float32,
              silence=True, new_idx=None, new_obs_ratio=0.0, adaptive_iter_offset=0,
              dataset=NS(processed_frame=0), **pool)


def pool_of(coord, label, history, seed=5):
    """Pool tensors whose last rows are the frame's samples, behind `history` older rows."""
    g = torch.Generator().manual_seed(seed)
    old_c = (torch.randn(history, 3, generator=g) * 5.0).to(coord)
    old_l = (torch.randn(history, generator=g) * 0.3).to(label)
    n = coord.shape[0]
    return dict(global_coord_pool=torch.cat((old_c, coord)).contiguous(), sdf_label_pool=torch.cat((old_l, label)).contiguous(),
                cur_sample_count=n, pool_sample_count=history + n)


# ---------------------------------------------------------------- model/neural_gaussians.py on the oracle's map
def set_search_neighborhood(npm, num_nei_cells=1, search_alpha=1.0):                 # :1026-1058
    npm.neighbor_dx = sdf_cpu.neighbor_offsets(num_nei_cells, search_alpha).to(npm.primes.device)
    npm.neighbor_K = npm.neighbor_dx.shape[0]
    npm.max_valid_dist2 = 3 * ((num_nei_cells + 1) * npm.resolution) ** 2


def query_certainty(npm, query_points):                                               # :1117-1133
    _, idx = npm.radius_neighborhood_search(query_points)
    certainty = npm.point_certainties[idx]
    certainty[idx < 0] = 0.0
    return torch.max(certainty, dim=-1)[0]


# ---------------------------------------------------------------- utils/mapper.py
def new_samples(m, frame_id=0):
    """utils/mapper.py:447-513 as written."""
    if m.config.bs_new_sample > 0:
        cur_sample_filtered = m.global_coord_pool[-m.cur_sample_count:]
        cur_sample_filtered_count = cur_sample_filtered.shape[0]
        bs = m.config.infer_bs
        iter_n = math.ceil(cur_sample_filtered_count / bs)
        cur_sample_certainty = torch.zeros(cur_sample_filtered_count, device=m.device)
        cur_label_filtered = m.sdf_label_pool[-m.cur_sample_count:]
        set_search_neighborhood(m.neural_points, num_nei_cells=1, search_alpha=0.0)
        for n in range(iter_n):
            head = n * bs
            tail = min((n + 1) * bs, cur_sample_filtered_count)
            cur_sample_certainty[head:tail] = query_certainty(m.neural_points, cur_sample_filtered[head:tail, :])
        set_search_neighborhood(m.neural_points, num_nei_cells=m.config.num_nei_cells,
                                search_alpha=m.config.search_alpha)
        m.new_idx = torch.where((cur_sample_certainty < m.config.new_certainty_thre)
                                & (torch.abs(cur_label_filtered) < m.config.surface_sample_range_m * 3.0))[0]
        m.new_idx += m.pool_sample_count - m.cur_sample_count
        new_sample_count = m.new_idx.shape[0]
        m.adaptive_iter_offset = 0
        m.new_obs_ratio = new_sample_count / m.cur_sample_count
        if m.config.adaptive_iters:
            if m.new_obs_ratio < m.config.new_sample_ratio_less:
                m.adaptive_iter_offset = -5
            elif m.new_obs_ratio > m.config.new_sample_ratio_more:
                m.adaptive_iter_offset = 5
                if frame_id > m.config.freeze_after_frame and m.new_obs_ratio > m.config.new_sample_ratio_restart:
                    m.adaptive_iter_offset = 10


def _sdf_and_certainty(m, points, need_grad):
    """:533-549 / :570-577: (sdf, gradient norm | None, certainty, nn_count)."""
    npm = m.neural_points
    geo_feature, _, weight_knn, nn_count, certainty = npm.query_feature(points, accumulate_stability=False)
    sdf_pred = m.sdf_mlp.sdf(geo_feature)
    if not m.config.weighted_first:
        sdf_pred = torch.sum(sdf_pred * weight_knn, dim=1).squeeze(1)
    grad_norm = None
    if need_grad:
        sdf_grad = sdf_cpu.get_gradient(points, sdf_pred).detach()
        grad_norm = sdf_grad.norm(dim=-1, keepdim=True).squeeze()
    return sdf_pred.detach(), grad_norm, certainty, nn_count


def dynamic_filter(m, points_torch, type_2_on=True):
    """utils/mapper.py:528-566."""
    if type_2_on:
        points_torch.requires_grad_(True)
    sdf_pred, grad_norm, certainty, _ = _sdf_and_certainty(m, points_torch, type_2_on)
    static_mask = (certainty < m.config.dynamic_certainty_thre) | (
        sdf_pred < m.config.dynamic_sdf_ratio_thre * m.config.voxel_size_m)
    if type_2_on:
        static_mask_2 = (grad_norm > m.config.dynamic_min_grad_norm_thre) | (certainty < m.config.dynamic_certainty_thre)
        static_mask = static_mask & static_mask_2
    return static_mask


def dynamic_filter_neural_points(m):
    """utils/mapper.py:568-585."""
    sdf_pred, _, certainty, _ = _sdf_and_certainty(m, m.neural_points.local_neural_points, False)
    return (certainty < m.config.dynamic_certainty_thre) | (
        sdf_pred < m.config.dynamic_sdf_ratio_thre * m.config.voxel_size_m)


def sdf_batch(m, x, bs, min_nn_count=1):
    """utils/mapper.py:2292-2316 with `Mapper.sdf` (:2273-2289) inlined."""
    count = x.shape[0]
    sdf_pred = torch.zeros(count, dtype=x.dtype, device=m.device)
    valid_mask = torch.ones(count, dtype=bool, device=m.device)
    for n in range(math.ceil(count / bs)):
        head, tail = n * bs, min((n + 1) * bs, count)
        s, _, _, nn_count = _sdf_and_certainty(m, x[head:tail, :], False)
        sdf_pred[head:tail] = s
        valid_mask[head:tail] = nn_count >= min_nn_count
    return sdf_pred, valid_mask


@torch.no_grad()
def check_invalid_neural_points(m, stability_threshold=1.0, render_min_nn_count=6):
    """utils/mapper.py:1636-1655."""
    npm = m.neural_points
    stable_mask = npm.local_point_certainties > stability_threshold
    stable = npm.local_neural_points[stable_mask]
    sdf, valid_nnk_mask = sdf_batch(m, stable, m.config.infer_bs, min_nn_count=render_min_nn_count)
    static_mask = torch.abs(sdf) < m.config.dynamic_sdf_ratio_thre * m.config.voxel_size_m
    npm.local_valid_gs_mask[stable_mask] = static_mask & valid_nnk_mask
    npm.valid_gs_mask[npm.local_mask[:-1]] = npm.local_valid_gs_mask


# ---------------------------------------------------------------- float64 yardstick with threshold bands
def map64(st, cert_global, cert_local, config):
    """The oracle map in float64 (from the same float32 values), dressed with the scenario."""
    npm = sdf_cpu.NeuralPointMap(st)
    npm.local_valid_gs_mask = torch.as_tensor(st["local_valid_gs_mask"]).clone()
    npm.local_mask = torch.as_tensor(st["local_mask"]).clone()
    dress(npm, cert_global, cert_local, config)
    for k, v in list(vars(npm).items()):
        if torch.is_tensor(v) and v.dtype == torch.float32:
            setattr(npm, k, v.double())
    npm.dtype = torch.float64
    return npm


def dec64(st):
    d = sdf_cpu.MLP.from_state(st)
    return sdf_cpu.MLP(d.W1.double(), d.b1.double(), d.W2.double(), d.b2.double(), d.sdf_scale)


def _near(v, thr):
    """Rows whose float64 value lies within BAND * max |v| of the threshold it is compared with."""
    return (v - thr).abs() <= BAND * float(v.abs().max())


def decisions(m64, points, type_2_on, absolute=False, min_nn=None):
    """(mask, undecidable) of one of the three decisions in float64.  `points` are the float32 query points;
    `absolute` selects |sdf| < thr && nn_count >= min_nn (check_invalid_neural_points), else the static mask."""
    cfg = m64.config
    x = points.detach().double().clone().requires_grad_(bool(type_2_on))
    sdf, grad_norm, certainty, nn_count = _sdf_and_certainty(m64, x, bool(type_2_on))
    thr = cfg.dynamic_sdf_ratio_thre * cfg.voxel_size_m
    if absolute:
        return (sdf.abs() < thr) & (nn_count >= min_nn), _near(sdf.abs(), thr)
    uncertain = certainty < cfg.dynamic_certainty_thre
    mask = uncertain | (sdf < thr)
    near = _near(sdf, thr)
    if type_2_on:
        mask = mask & ((grad_norm > cfg.dynamic_min_grad_norm_thre) | uncertain)
        near = near | _near(grad_norm, cfg.dynamic_min_grad_norm_thre)
    return mask, near


def check_gates(mask, near, what):
    """The gates of the scenario itself: at most 1 % of the rows undecidable, and among the decidable ones each outcome
    at least 5 % of the rows (a constant mask fails)."""
    n = mask.numel()
    dec = ~near
    share, ones, zeros = float(near.sum()) / n, float((mask & dec).sum()) / n, float((~mask & dec).sum()) / n
    print(f"{what}: n={n} undecidable {share:.4f}  static {ones:.3f}  dynamic {zeros:.3f}")
    assert share <= 0.01, f"{what}: {share:.4f} of the rows are undecidable"
    assert ones >= 0.05 and zeros >= 0.05, f"{what}: outcomes {ones:.3f} / {zeros:.3f} of the rows"
