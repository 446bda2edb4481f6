"""Torch restatement of the reference's loop-closure context (utils/loop_detector.py) for tests/test_loop_ops.py,
tools/make_loop_golden.py and tools/loop_time.py.

Three parts:

  * the fp32 restatement, op for op: `ptcloud2sc_torch`, `sc2rk`, `distance_sc_torch`, `distance_sc_feature_torch` and
    `NeuralPointMapContextManager` under the reference's own names, so that this module can stand where
    `utils.loop_detector` stands (`loop_ops.install(loop_ref)`).  On the CPU it equals tests/golden/loop_*.npz exactly,
    up to the order in which torch's horizontal reductions add on the CPU at hand (tests/test_loop_ops.py).
  * the fp64 judge: `judge_contexts` (descriptors with the bins fp32 cannot decide marked) and `judge_search`.
  * the scenario builder (`field`, `pose`, `context_case`, `search_case`) and the fixture reader.

Decidability.  With e = 4 * 2^-23 * (|p|_1 + |t|_1) for a point p under a transform with translation t, a (pose, point)
pair is undecidable when, in fp64, its range is within e + 4 * 2^-23 * r of an inner ring edge, its arc distance to a
sector edge r_xy * |theta - k * gap| is below e + 8 pi * 2^-23 * r_xy, or its range is within e + 4 * 2^-23 * max_length
of max_length.  Only edges between two different bins count (ring edges 1..R-1, all S sector edges, the wrap included).
A pair so close to the z axis that half a sector's arc is below the sector bound could fall into any sector: its whole
ring is left out.  Both bins (all four when a pair is near a ring and a sector edge) are left out of the comparison
for that pose.
"""
import math
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -23
TIE = 1e-12                 # fp64 values closer than this (relative to max(1, scale)) come from identical inputs
GOLDEN = Path(__file__).resolve().parent / "golden"


# ================================================================ fp32, op for op (the reference's names)
def ptcloud2sc_torch(ptcloud, pt_feature, sc_shape, max_length):
    r = torch.norm(ptcloud, dim=1)
    kept_mask = r < max_length
    points = ptcloud[kept_mask]
    r = r[kept_mask]
    num_ring, num_sector = sc_shape[0], sc_shape[1]
    gap_ring = max_length / num_ring
    gap_sector = 360.0 / num_sector
    sc = torch.zeros(num_ring * num_sector, dtype=points.dtype, device=points.device)
    sc_feature = None
    if pt_feature is not None:
        pt_feature_kept = (pt_feature.clone())[kept_mask]
        sc_feature = torch.zeros(num_ring * num_sector, pt_feature.shape[1], dtype=points.dtype, device=points.device)
    theta = torch.atan2(points[:, 1], points[:, 0])
    theta_degrees = theta * 180.0 / math.pi + 180.0
    idx_ring = torch.clamp((r // gap_ring).long(), 0, num_ring - 1)
    idx_sector = torch.clamp((theta_degrees // gap_sector).long(), 0, num_sector - 1)
    grid_indices = idx_ring * num_sector + idx_sector
    sc = sc.scatter_reduce_(dim=0, index=grid_indices, src=points[:, 2], reduce="amax", include_self=False)
    sc = sc.view(num_ring, num_sector)
    if pt_feature is not None:
        grid_indices = grid_indices.view(-1, 1).repeat(1, pt_feature.shape[1])
        sc_feature = sc_feature.scatter_reduce_(dim=0, index=grid_indices, src=pt_feature_kept, reduce="mean",
                                                include_self=False)
        sc_feature = sc_feature.view(num_ring, num_sector, pt_feature.shape[1])
    return sc, sc_feature


def sc2rk(sc):
    return torch.mean(sc, dim=1)


def _shift_search(sc1, sc2, flat):
    num_rings, num_sectors = sc1.shape[0], sc1.shape[1]
    sims = torch.zeros(num_sectors)
    for i in range(num_sectors):
        sc1 = torch.roll(sc1, 1, 1)
        if flat:
            cossim = F.cosine_similarity(sc1.view(num_rings, -1), sc2.view(num_rings, -1), dim=0)
        else:
            cossim = F.cosine_similarity(sc1, sc2, dim=0)
        sims[i] = torch.mean(cossim)
    yaw_diff = torch.argmax(sims) + 1
    dist = 1 - torch.max(sims)
    return dist.item(), yaw_diff.item()


def distance_sc_torch(sc1, sc2):
    return _shift_search(sc1, sc2, False)


def distance_sc_feature_torch(sc1, sc2):
    return _shift_search(sc1, sc2, True)


def transform_torch(points, transformation):
    homo = torch.cat([points, torch.ones(points.shape[0], 1).to(points)], dim=1)
    return torch.matmul(homo, transformation.to(points).T)[:, :3]


class NeuralPointMapContextManager:
    """The reference's manager, restated: same attributes, same arithmetic, same quirks."""

    def __init__(self, config):
        self.config = config
        self.device, self.dtype, self.tran_dtype, self.silence = config.device, config.dtype, config.tran_dtype, config.silence
        self.des_shape = config.context_shape
        self.num_candidates = config.context_num_candidates
        self.ringkey_dist_thre = (config.max_z - config.min_z) * 0.25
        self.sc_cosdist_threshold = config.context_cosdist_threshold
        if config.local_map_context:
            self.sc_cosdist_threshold += 0.08
            if config.loop_with_feature:
                self.sc_cosdist_threshold += 0.08
                self.ringkey_dist_thre = 0.25
        self.max_length = config.npmc_max_dist
        self.ENOUGH_LARGE = config.end_frame
        self.contexts = [None] * self.ENOUGH_LARGE
        self.ringkeys = [None] * self.ENOUGH_LARGE
        self.contexts_feature = [None] * self.ENOUGH_LARGE
        self.ringkeys_feature = [None] * self.ENOUGH_LARGE
        self.query_contexts = []
        self.tran_from_frame = []
        self.curr_node_idx = 0
        self.virtual_step_m = config.context_virtual_step_m
        self.virtual_side_count = config.context_virtual_side_count
        self.virtual_sdf_thre = 0.0

    def add_node(self, frame_id, ptcloud, ptfeatures=None):
        sc, sc_feature = ptcloud2sc_torch(ptcloud, ptfeatures, self.des_shape, self.max_length)
        rk = sc2rk(sc)
        self.curr_node_idx = frame_id
        self.contexts[frame_id] = sc
        self.ringkeys[frame_id] = rk
        if sc_feature is not None:
            self.contexts_feature[frame_id] = sc_feature
            self.ringkeys_feature[frame_id] = sc2rk(sc_feature)
        self.query_contexts = []
        self.tran_from_frame = []

    def set_virtual_node(self, ptcloud_global, frame_pose, last_frame_pose, ptfeatures=None):
        if last_frame_pose is not None:
            tran_direction = frame_pose[:3, 3] - last_frame_pose[:3, 3]
            tran_direction_unit = tran_direction / torch.norm(tran_direction)
            lat_rot = torch.tensor([[0, -1, 0], [1, 0, 0], [0, 0, 1]], device=self.device, dtype=self.dtype)
            lat_direction_unit = lat_rot @ tran_direction_unit.float()
        else:
            lat_direction_unit = torch.tensor([0, 1, 0], device=self.device, dtype=self.dtype)
        dx = torch.arange(-self.virtual_side_count, self.virtual_side_count + 1, device=self.device) * self.virtual_step_m
        lat_tran = dx.view(-1, 1) @ lat_direction_unit.view(1, 3)
        for idx in range(lat_tran.shape[0]):
            cur_lat_tran = lat_tran[idx]
            cur_tran_from_frame = torch.eye(4, device=self.device, dtype=torch.float64)
            cur_tran_from_frame[:3, 3] = cur_lat_tran
            cur_virtual_pose = frame_pose @ torch.linalg.inv(cur_tran_from_frame)
            if torch.norm(cur_lat_tran) == 0:
                if ptfeatures is None:
                    cur_sc = self.contexts[self.curr_node_idx]
                else:
                    cur_sc_feature = self.contexts_feature[self.curr_node_idx]
            else:
                ptcloud = transform_torch(ptcloud_global, torch.linalg.inv(cur_virtual_pose))
                cur_sc, cur_sc_feature = ptcloud2sc_torch(ptcloud, ptfeatures, self.des_shape, self.max_length)
            self.query_contexts.append(cur_sc if ptfeatures is None else cur_sc_feature)
            self.tran_from_frame.append(cur_tran_from_frame)

    def detect_loop(self, candidate_idx, use_feature=False):
        if candidate_idx.shape[0] == 0:
            return None, None, None
        keys = self.ringkeys_feature if use_feature else self.ringkeys
        history = torch.stack([keys[i] for i in candidate_idx])
        min_dist_ringkey, min_loop_idx, min_query_idx = 1e5, None, 0
        if len(self.query_contexts) == 0:
            self.tran_from_frame.append(torch.eye(4, device=self.device, dtype=torch.float64))
            self.query_contexts.append((self.contexts_feature if use_feature else self.contexts)[self.curr_node_idx])
        for query_idx in range(len(self.query_contexts)):
            query_key = sc2rk(self.query_contexts[query_idx])
            if use_feature:
                dist_to_history = 1.0 - F.cosine_similarity(query_key.view(1, -1),
                                                            history.view(history.shape[0], -1), dim=1)
            else:
                dist_to_history = torch.norm(query_key - history, p=1, dim=1)
            min_idx = torch.argmin(dist_to_history)
            cur_dist_ringkey = dist_to_history[min_idx].item()
            if cur_dist_ringkey < min_dist_ringkey:
                min_dist_ringkey = cur_dist_ringkey
                min_loop_idx = candidate_idx[min_idx].item()
                min_query_idx = query_idx
        if min_dist_ringkey > self.ringkey_dist_thre:
            return None, None, None
        if use_feature:
            cosdist, yaw_diff = distance_sc_feature_torch(self.contexts_feature[min_loop_idx],
                                                          self.query_contexts[min_query_idx])
        else:
            cosdist, yaw_diff = distance_sc_torch(self.contexts[min_loop_idx], self.query_contexts[min_query_idx])
        if not cosdist < self.sc_cosdist_threshold:
            return None, None, None
        yawdiff_rad = math.radians(yaw_diff * (360.0 / self.des_shape[1]))
        transformation = np.eye(4)
        transformation[0, 0] = transformation[1, 1] = math.cos(yawdiff_rad)
        transformation[0, 1] = math.sin(yawdiff_rad)
        transformation[1, 0] = -math.sin(yawdiff_rad)
        transformation = transformation @ self.tran_from_frame[min_query_idx].detach().cpu().numpy()
        return min_loop_idx, cosdist, transformation


def make_config(device="cpu", **kw):
    """The fields of the reference's `Config` that the manager reads, at the reference's defaults."""
    c = SimpleNamespace(device=device, dtype=torch.float32, tran_dtype=torch.float64, silence=True,
                        context_shape=[20, 60], context_num_candidates=1, max_z=60.0, min_z=-5.0,
                        context_cosdist_threshold=0.2, local_map_context=False, loop_with_feature=False,
                        npmc_max_dist=60.0, end_frame=100000, context_virtual_step_m=2.0,
                        context_virtual_side_count=5)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


# ================================================================ scenario
def field(n, seed, width=160.0, centre=(150.0, -80.0, 3.0), below=False):
    """A rolling-height field `width` m wide under a sensor at `centre`: float32 world points [n,3]."""
    g = torch.Generator().manual_seed(seed)
    xy = (torch.rand(n, 2, generator=g, dtype=torch.float64) - 0.5) * width
    z = 1.5 * torch.sin(xy[:, 0] * 0.11) * torch.cos(xy[:, 1] * 0.07) + 0.8 * torch.sin(xy[:, 1] * 0.31 + 1.0)
    z = z + (xy.norm(dim=1) * 0.02) + (-9.0 if below else 0.0)
    c = torch.tensor(centre, dtype=torch.float64)
    return torch.cat([xy + c[:2], (z + c[2] - 3.0).unsqueeze(1)], dim=1).float()


def features(points, d, seed):
    g = torch.Generator().manual_seed(seed + 7)
    return (torch.randn(points.shape[0], d, generator=g) * 0.5).float()


def pose(centre=(150.0, -80.0, 3.0), yaw=0.7):
    T = torch.eye(4, dtype=torch.float64)
    T[0, 0] = T[1, 1] = math.cos(yaw)
    T[0, 1], T[1, 0] = -math.sin(yaw), math.sin(yaw)
    T[:3, 3] = torch.tensor(centre, dtype=torch.float64)
    return T


def virtual_transforms(frame_pose, last_pose, side, step):
    """fp64 restatement of the virtual poses: (transforms [M,12] float32 = inv(frame_pose @ inv(T_k)) rounded once,
    tran_from_frame [M,4,4] float64, lat_tran [M,3] float32), the lateral offsets in the reference's fp32."""
    if last_pose is not None:
        d = frame_pose[:3, 3] - last_pose[:3, 3]
        u = (d / torch.norm(d)).float()
        lat_dir = torch.tensor([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dtype=torch.float32) @ u
    else:
        lat_dir = torch.tensor([0, 1, 0], dtype=torch.float32)
    dx = torch.arange(-side, side + 1) * step
    lat = dx.view(-1, 1) @ lat_dir.view(1, 3)
    M = lat.shape[0]
    tran = torch.eye(4, dtype=torch.float64).repeat(M, 1, 1)
    tran[:, :3, 3] = lat.double()
    T = torch.linalg.inv(frame_pose.unsqueeze(0) @ torch.linalg.inv(tran))
    return T[:, :3, :].reshape(M, 12).float().contiguous(), tran, lat


IDENTITY = torch.eye(3, 4).reshape(1, 12)


def to_sensor(points, frame_pose):
    """World points in the sensor frame of `frame_pose`: fp64 arithmetic, rounded once."""
    Ti = torch.linalg.inv(frame_pose)
    return (points.double() @ Ti[:3, :3].T + Ti[:3, 3]).float()


# ================================================================ fp64 judge: descriptors
def _pairs(points, t12, R, S, max_length):
    """Per point of one pose, in fp64: kept, bin, z', e, undecidable, and the bins it could fall into."""
    p = points.double()
    T = t12.double().view(3, 4)
    q = p @ T[:, :3].T + T[:, 3]
    e = 4 * U * (p.abs().sum(dim=1) + T[:, 3].abs().sum())
    r = q.norm(dim=1)
    rxy = q[:, :2].norm(dim=1)
    finite = torch.isfinite(q).all(dim=1)
    kept = finite & (r < max_length)
    gap_r, gap_s = max_length / R, 2 * math.pi / S
    theta = torch.atan2(q[:, 1], q[:, 0]) + math.pi
    safe = lambda t: torch.where(finite, t, torch.zeros_like(t))  # noqa: E731
    ring = torch.clamp(torch.floor(safe(r) / gap_r), 0, R - 1).long()
    sector = torch.clamp(torch.floor(safe(theta) / gap_s), 0, S - 1).long()
    kr = torch.round(safe(r) / gap_r)
    edge_r = finite & (kr >= 1) & (kr <= R - 1) & ((r - kr * gap_r).abs() < e + 4 * U * r)
    ring_alt = torch.where(edge_r, torch.where(ring == kr.long(), kr.long() - 1, kr.long()), ring)
    ks = torch.round(safe(theta) / gap_s)
    bound_s = e + 8 * math.pi * U * rxy
    edge_s = finite & (rxy * (theta - ks * gap_s).abs() < bound_s)
    sector_alt = torch.where(edge_s, torch.where(sector == (ks.long() % S), (ks.long() - 1) % S, ks.long() % S), sector)
    axis = finite & (rxy * (gap_s / 2) < bound_s)
    near_max = finite & ((r - max_length).abs() < e + 4 * U * max_length)
    concerned = kept | near_max
    undecidable = concerned & (edge_r | edge_s | near_max | axis)
    return dict(kept=kept, ring=ring, sector=sector, z=q[:, 2], e=e, undecidable=undecidable, ring_alt=ring_alt,
                sector_alt=sector_alt, axis=axis & concerned)


def undecidable_points(points, transforms, R, S, max_length):
    """bool [N]: the point is undecidable for at least one of the poses."""
    out = torch.zeros(points.shape[0], dtype=torch.bool)
    for m in range(transforms.shape[0]):
        out |= _pairs(points, transforms[m], R, S, max_length)["undecidable"]
    return out


def judge_contexts(points, feats, transforms, R, S, max_length):
    """fp64 descriptors of the M poses: sc [M,R,S], e_win (e of the bin's winning point), n (points per bin), and with
    features mean [M,R,S,D] and fmax (largest |feature| among the bin's points); left_out [M,R,S] marks the bins that
    an undecidable pair could fall into."""
    M, RS = transforms.shape[0], R * S
    D = 0 if feats is None else feats.shape[1]
    out = dict(sc=torch.zeros(M, RS, dtype=torch.float64), e_win=torch.zeros(M, RS, dtype=torch.float64),
               n=torch.zeros(M, RS, dtype=torch.int64), left_out=torch.zeros(M, RS, dtype=torch.bool))
    if D:
        out["mean"] = torch.zeros(M, RS, D, dtype=torch.float64)
        out["fmax"] = torch.zeros(M, RS, dtype=torch.float64)
    for m in range(M):
        P = _pairs(points, transforms[m], R, S, max_length)
        u = P["undecidable"]
        for rr in (P["ring"][u], P["ring_alt"][u]):
            for ss in (P["sector"][u], P["sector_alt"][u]):
                out["left_out"][m, rr * S + ss] = True
        ax = P["axis"]
        for rr in (P["ring"][ax], P["ring_alt"][ax]):
            for s in range(S):
                out["left_out"][m, rr * S + s] = True
        k = P["kept"]
        b, z, e = (P["ring"] * S + P["sector"])[k], P["z"][k], P["e"][k]
        if b.numel() == 0:
            continue
        n = torch.bincount(b, minlength=RS)
        zmax = torch.full((RS,), -math.inf, dtype=torch.float64).scatter_reduce_(0, b, z, "amax", include_self=True)
        win = z == zmax[b]
        out["e_win"][m].scatter_reduce_(0, b[win], e[win], "amax", include_self=True)
        out["sc"][m] = torch.where(n > 0, zmax, torch.zeros_like(zmax))
        out["n"][m] = n
        if D:
            f = feats.double()[k]
            out["mean"][m] = torch.zeros(RS, D, dtype=torch.float64).index_add_(0, b, f) / n.clamp(min=1).unsqueeze(1)
            out["fmax"][m].scatter_reduce_(0, b, f.abs().amax(dim=1), "amax", include_self=True)
    for key in out:
        out[key] = out[key].view(M, R, S, *out[key].shape[2:])
    return out


def context_case(n, M, D, shape, filtered, seed, variant="field"):
    """Inputs of one build case: (points [n,3], features [n,D] | None, transforms [M,12], max_length).  M == 1 is the
    sensor-frame case (the cloud moved into the sensor frame in fp64, identity transform); M > 1 are the lateral
    virtual poses of the scenario, 2 m apart, on the world cloud.  `filtered` draws more points, removes the undecidable
    ones and keeps the first n.  Variants: "below" (every z' negative), "beyond" (every point past max_length),
    "nonfinite" (NaN / inf rows mixed in)."""
    R, S = shape
    max_length = 60.0
    fp = pose()
    pts = field(2 * n + 64 if filtered else n, seed, below=(variant == "below"))
    if variant == "beyond":
        pts = pts + torch.tensor([400.0, 0.0, 0.0])
    if M == 1:
        pts, T = to_sensor(pts, fp), IDENTITY.clone()
    else:
        T, _, _ = virtual_transforms(fp, pose(centre=(149.0, -81.0, 3.0)), (M - 1) // 2, 2.0)
    if filtered:
        pts = pts[~undecidable_points(pts, T, R, S, max_length)][:n]
        assert pts.shape[0] == n
    if variant == "nonfinite" and n >= 8:
        pts = pts.clone()
        pts[1, 0], pts[3, 2], pts[5, 1], pts[6] = float("nan"), float("inf"), float("-inf"), float("nan")
    f = features(pts, D, seed) if D else None
    return pts.contiguous(), f, T.contiguous(), max_length


def check_contexts(got, J, sensor_frame, S):
    """Asserts the bounds of the issue for one build result `got` = (sc, rk, scf, rkf) (CPU tensors) against the judge's
    dict `J`.  Returns the number of compared bins."""
    sc, rk, scf, rkf = [None if t is None else t.double() for t in got]
    keep = ~J["left_out"]
    if sensor_frame:                                     # z' = z exactly: bit-equal to fp64 rounded to fp32
        assert torch.equal(got[0][keep], J["sc"].float()[keep])
    else:
        assert bool(((sc - J["sc"]).abs() <= J["e_win"])[keep].all())
    assert torch.equal(got[0][keep & (J["n"] == 0)], torch.zeros_like(got[0][keep & (J["n"] == 0)]))
    # ring keys as a function of the descriptor that was written: S * 2^-23 * max|value| of summation error
    tol = S * U * sc.abs().amax(dim=2)
    assert bool(((rk - sc.mean(dim=2)).abs() <= tol).all())
    clean = keep.all(dim=2)                              # rings with every bin decidable: against fp64 itself
    bin_tol = torch.zeros_like(J["e_win"]) if sensor_frame else J["e_win"]
    tol64 = bin_tol.amax(dim=2) + S * U * J["sc"].abs().amax(dim=2) + (U / 2) * J["sc"].abs().amax(dim=2)
    assert bool(((rk - J["sc"].mean(dim=2)).abs() <= tol64)[clean].all())
    if scf is not None:
        ftol = (J["n"] + 2).double() * U * J["fmax"]
        assert bool(((scf - J["mean"]).abs() <= ftol.unsqueeze(-1))[keep].all())
        assert torch.equal(got[2][keep & (J["n"] == 0)], torch.zeros_like(got[2][keep & (J["n"] == 0)]))
        tolf = S * U * scf.abs().amax(dim=2)
        assert bool(((rkf - scf.mean(dim=2)).abs() <= tolf).all())
        tolf64 = ftol.amax(dim=2).unsqueeze(-1) + S * U * J["mean"].abs().amax(dim=2)
        assert bool(((rkf - J["mean"].mean(dim=2)).abs() <= tolf64)[clean].all())
    return int(keep.sum())


# ================================================================ fp64 judge: search
def judge_search(bank_ctx, bank_key, cand, q_ctx, q_key, use_feature):
    """fp64 search over descriptors given as inputs.  bank_* are indexed by slot; cand are slots.  Returns the winner
    (position in cand, query), its ring-key distance, the margin to the next larger distance (relative to the largest
    distance), the cosine distance, the shift in 1..S and the margin to the next smaller shift mean."""
    cand = torch.as_tensor(np.asarray(cand), dtype=torch.long)
    Q, C = q_key.shape[0], cand.shape[0]
    qk, hk = q_key.double().reshape(Q, -1), bank_key.double()[cand].reshape(C, -1)
    if use_feature:
        dot = (qk.unsqueeze(1) * hk.unsqueeze(0)).sum(dim=2)
        d = 1.0 - dot / (qk.norm(dim=1).clamp(min=1e-8).unsqueeze(1) * hk.norm(dim=1).clamp(min=1e-8).unsqueeze(0))
    else:
        d = (qk.unsqueeze(1) - hk.unsqueeze(0)).abs().sum(dim=2)
    flat = d.reshape(-1)
    tie = TIE * max(1.0, float(flat.abs().max()))     # identical inputs: equal up to the order of an fp64 sum
    best = float(flat.min())
    w = int(torch.nonzero(flat <= best + tie)[0])     # the first minimum in (query, candidate) order
    q, cpos = divmod(w, C)
    larger = flat[flat > best + tie]
    rk_margin = float((larger.min() - best) / flat.max().clamp(min=1e-30)) if larger.numel() else math.inf
    A, B = bank_ctx.double()[cand[cpos]], q_ctx.double()[q]
    R, S = A.shape[0], A.shape[1]
    sims = torch.zeros(S, dtype=torch.float64)
    for i in range(1, S + 1):
        a, b = torch.roll(A, i, 1).reshape(R, -1), B.reshape(R, -1)
        den = a.norm(dim=0).clamp(min=1e-8) * b.norm(dim=0).clamp(min=1e-8)
        sims[i - 1] = ((a * b).sum(dim=0) / den).mean()
    arg = int(torch.nonzero(sims >= sims.max() - TIE)[0])     # the first maximum
    smaller = sims[sims < sims.max() - TIE]
    shift_margin = float(sims[arg] - smaller.max()) if smaller.numel() else math.inf
    return dict(cpos=cpos, q=q, rk=best, rk_margin=rk_margin, cos=float(1.0 - sims[arg]), shift=arg + 1,
                shift_margin=shift_margin, sims=sims)


def search_case(C, Q, use_feature, seed, shape=(20, 60), D=8, slots=None, tie=None):
    """A bank and queries with one clear winner: query `qw` is candidate `cw` rolled by `shift` sectors plus a
    little noise; every other descriptor is independent.  Slots are non-contiguous.  tie: "slot" stores the winning
    node in a second slot later in cand, "query" repeats the winning query later, "period" gives the winner columns
    that repeat with period S/2 (S even)."""
    R, S = shape
    g = torch.Generator().manual_seed(seed)
    Dd = D if use_feature else 1
    cap = slots if slots is not None else 2 * C + 5
    perm = torch.randperm(cap, generator=g)[:C]
    cand = perm.numpy().astype(np.int32)
    ctx = torch.rand(cap, R, S, Dd, generator=g) * 3.0 - (1.5 if use_feature else 0.0)
    ctx = ctx * (torch.rand(cap, R, S, 1, generator=g) > 0.2)                     # empty bins
    if not use_feature:
        ctx[:, :, 3] = 0.0                                                       # a column of zero norm everywhere
    cw, qw, shift = (C * 2) // 3, (Q * 2) // 3, 1 + (seed * 7) % S
    if tie == "period":
        half = ctx[cand[cw], :, : S // 2].clone()
        ctx[cand[cw]] = torch.cat([half, half], dim=1)
        shift = 1 + shift % (S // 2)
    q_ctx = torch.rand(Q, R, S, Dd, generator=g) * 3.0 - (1.5 if use_feature else 0.0)
    q_ctx[qw] = torch.roll(ctx[cand[cw]], shift, 1) + 0.01 * torch.rand(R, S, Dd, generator=g)
    if tie == "slot":
        assert C >= 3
        later = C - 1 if cw != C - 1 else C - 2
        assert later > cw
        ctx[cand[later]] = ctx[cand[cw]]
    if tie == "query":
        assert Q >= 3 and qw < Q - 1
        q_ctx[Q - 1] = q_ctx[qw]
    if not use_feature:
        ctx, q_ctx = ctx[..., 0], q_ctx[..., 0]
    key, q_key = ctx.mean(dim=2), q_ctx.mean(dim=2)
    return dict(ctx=ctx.contiguous(), key=key.contiguous(), cand=cand, q_ctx=q_ctx.contiguous(),
                q_key=q_key.contiguous(), cw=cw, qw=qw, shift=shift, R=R, S=S, D=D if use_feature else 0,
                use_feature=use_feature)


def distance_tol(R, S, D, d64):
    """(R + S * D + 8) * 2^-23 relative to max(1, |d|): a sum of R (ring key) or a mean of S * D cosines of R-term dot
    products carries at most that many half-ulp roundings of a quantity no larger than max(1, |d|)."""
    return (R + S * max(D, 1) + 8) * U * max(1.0, abs(d64))


# ================================================================ fixtures
def load(name):
    z = np.load(GOLDEN / name)
    return {k: z[k] for k in z.files}


def sequence_inputs(fix):
    """The manager sequence of tests/golden/loop_sequence.npz as tensors: the world cloud (float32), its features
    (stored as float16, exact in float32), K node poses (float64)."""
    pts = torch.from_numpy(fix["points"].astype(np.float32))
    feats = torch.from_numpy(fix["features"].astype(np.float32))
    poses_ = torch.from_numpy(fix["poses"].astype(np.float64))
    return pts, feats, poses_


def run_sequence(module, fix, use_feature, device="cpu"):
    """add_node x K, set_virtual_node, detect_loop through `module.NeuralPointMapContextManager` on the fixture's inputs:
    (manager, triple).  Every node's cloud is the world cloud in that node's sensor frame (`to_sensor`)."""
    pts, feats, poses_ = sequence_inputs(fix)
    cfg = make_config(device=device, end_frame=int(fix["end_frame"]), loop_with_feature=bool(use_feature),
                      local_map_context=True, context_cosdist_threshold=float(fix["cosdist_threshold"]))
    mgr = module.NeuralPointMapContextManager(cfg)
    K = poses_.shape[0]
    f_dev = feats.to(device) if use_feature else None
    for k in range(K):
        mgr.add_node(int(fix["frame_ids"][k]), to_sensor(pts, poses_[k]).to(device), f_dev)
    last = K - 1
    mgr.set_virtual_node(pts.to(device), poses_[last].to(device), poses_[last - 1].to(device), f_dev)
    triple = mgr.detect_loop(fix["candidates"], use_feature=bool(use_feature))
    return mgr, triple
