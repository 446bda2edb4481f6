"""Map maintenance kernels (csrc/map.hip) against the CPU oracle at count, window, slot and threshold edges.

tests/test_map.py runs the golden sequences and two large random maps, all with one configuration.  Here every case is
the smallest input that reaches one branch of the kernels: counts at 1 and around the 256-thread block, the
"fewer than 100 points in the window -> take all" rule on both sides of 100, the timestamp window, a map without
colours or without the temporal window, an empty map, tables small enough to force duplicate slots, squared distances
placed exactly ON the thresholds, the byte kernels of the row copies, the 16-job limit.

The reference is oracle/map_cpu.py (pinned by the G8 / G12 golden vectors) on CPU tensors with the same inputs.  Every
comparison is exact — equal dtype, shape and `torch.equal` — except the positions and orientations after `adjust_map`
with a non-identity pose, which keep 2e-6 (test_map.py::_run_closure: a 3-term fp32 dot product and a quaternion
product, association free).

Every case is a *scenario*: a function that drives either the oracle or the HIP path through the same calls and
records snapshots.  `test_oracle_reaches_the_branch` (no GPU) runs the oracle alone; the scenario asserts there that its
inputs reach the branch it is named after.  `test_hip_matches_oracle` runs both and compares every snapshot."""
import math

import numpy as np
import pytest
import torch

from oracle import map_cpu as M

GLOBAL = ("neural_points", "point_colors", "valid_color_mask", "free_gs_mask", "point_ts_create", "point_ts_update",
          "buffer_pt_index", "geo_features", "color_features", "point_orientations", "valid_gs_mask",
          "point_certainties")
UPDATE = GLOBAL + ("_last_update_mask", "_last_sample_idx")
LOCAL = ("local_mask", "sorrounding_mask", "global2local", "local_neural_points", "local_point_orientations",
         "local_point_certainties", "local_point_ts_update", "local_point_colors", "local_valid_color_mask",
         "local_valid_gs_mask", "local_free_gs_mask", "local_geo_features", "local_color_features")
ASSIGNED = ("geo_features", "color_features", "point_certainties", "point_ts_update")
GEO, COL = 8, 4


class _Run:
    """The oracle or the HIP path behind one set of call shapes, and the snapshots a scenario records."""

    def __init__(self, hip: bool):
        self.hip, self.oracle = hip, not hip
        self.dev = "cuda" if hip else "cpu"
        self.snaps = []
        if hip:
            from pings_amd import neural_map as NM
            self.NM = NM

    def T(self, t):
        return None if t is None else t.clone().to(self.dev)

    def new_map(self, *a, **kw):
        return self.NM.new_map(*a, device="cuda", **kw) if self.hip else M.new_map(*a, **kw)

    def vds(self, pts, voxel, value=None):
        if self.hip:
            return self.NM.voxel_down_sample(self.T(pts), voxel, self.T(value))
        return M.voxel_down_sample(pts, voxel) if value is None else M.voxel_down_sample_min_value(pts, voxel, value)

    def update(self, m, pts, cols, ts, is_reliable=True):
        if self.hip:
            self.NM.update(m, self.T(pts), self.T(cols), cur_ts=ts, is_reliable=is_reliable)
        else:
            _, m._last_sample_idx, m._last_update_mask = M.update(m, pts, cols, ts, is_reliable=is_reliable)
        _fill(m)

    def reset(self, m, sensor, ts, use_travel_dist=True, diff_ts_local=50):
        if self.hip:
            self.NM.reset_local_map(m, self.T(sensor), None, ts, use_travel_dist, diff_ts_local)
        else:
            M.reset_local_map(m, sensor, ts, use_travel_dist, diff_ts_local)

    def assign(self, m):
        (self.NM if self.hip else M).assign_local_to_global(m)

    def prune(self, m, thre, min_count):
        return (self.NM if self.hip else M).prune_map(m, thre, min_count)

    def adjust(self, m, pose):
        (self.NM if self.hip else M).adjust_map(m, self.T(pose))

    def recreate(self, m, sensor, kept, with_ts, cur_ts):
        (self.NM if self.hip else M).recreate_hash(m, self.T(sensor), None, kept, with_ts, cur_ts)

    def rec(self, tag, m, names):
        snap = {}
        for k in names:
            v = getattr(m, k, None)
            snap[k] = v.detach().cpu().clone() if isinstance(v, torch.Tensor) else v
        self.snaps.append((tag, snap))

    def rec_value(self, tag, v):
        self.snaps.append((tag, {"value": v.detach().cpu().clone() if isinstance(v, torch.Tensor) else v}))


def _compare(hip: _Run, cpu: _Run, tol=None):
    assert [t for t, _ in hip.snaps] == [t for t, _ in cpu.snaps]
    for (tag, a), (_, b) in zip(hip.snaps, cpu.snaps):
        assert list(a) == list(b), tag
        for k, y in b.items():
            x = a[k]
            if not isinstance(y, torch.Tensor):
                assert type(x) is type(y) and x == y, (tag, k, x, y)
                continue
            assert isinstance(x, torch.Tensor) and x.dtype == y.dtype and x.shape == y.shape, \
                (tag, k, getattr(x, "dtype", None), y.dtype, getattr(x, "shape", None), y.shape)
            if tol is not None and k in ("neural_points", "point_orientations"):
                d = (x.double() - y.double()).abs().max().item() if y.numel() else 0.0
                assert d <= tol * max(1.0, y.abs().max().item()), (tag, k, d)
            else:
                assert torch.equal(x, y), (tag, k, int((x != y).sum()))


def _fill(m):
    """Row-dependent content (exact in fp32) for everything `update` initialises to a constant, so that a misrouted row
    of a gather or scatter shows.  In place: the HIP path's backing buffers stay adopted."""
    n = int(m.neural_points.shape[0])
    dev = m.neural_points.device
    i = torch.arange(n + 1, dtype=torch.float32, device=dev)
    with torch.no_grad():
        m.geo_features.copy_(i[:, None] + torch.arange(m.geo_features.shape[1], device=dev) / 16.0)
        if m.color_features is not None:
            m.color_features.copy_(-i[:, None] - torch.arange(m.color_features.shape[1], device=dev) / 8.0)
        m.point_certainties.copy_(0.5 * i[:n])
        m.point_orientations.copy_(torch.stack((i[:n] + 1.0, -i[:n], 0.25 * i[:n], i[:n] * 0.0 + 3.0), 1))


def _direct(R, pts, ts_create, ts_update, buffer_size=100_003, res=0.25, geo=GEO, color_on=True, cert=None, **kw):
    """A map whose per-point tensors are set directly (no `update`): exact control over counts and timestamps."""
    n = int(pts.shape[0])
    g = torch.Generator().manual_seed(n + 17)
    m = R.new_map(buffer_size, geo, COL, res, color_on=color_on, **kw)
    m.neural_points = R.T(pts.float())
    m.point_orientations = R.T(torch.zeros(n, 4))
    m.point_ts_create, m.point_ts_update = R.T(ts_create.to(torch.int32)), R.T(ts_update.to(torch.int32))
    m.point_certainties = R.T(torch.zeros(n))
    if color_on:
        m.point_colors = R.T(torch.rand(n, 3, generator=g))
        m.color_features = R.T(torch.zeros(n + 1, COL))
    m.valid_color_mask = R.T(torch.arange(n) % 3 != 0)
    m.valid_gs_mask = R.T(torch.arange(n) % 5 != 0)
    m.free_gs_mask = R.T(torch.arange(n) % 7 == 0)
    m.geo_features = R.T(torch.zeros(n + 1, geo))
    _fill(m)
    if cert is not None:
        m.point_certainties = R.T(cert.float())
    return m


def _edit_and_assign(R, m, tag):
    """What the mapper does between reset and write-back: optimise the local features, raise the certainties, stamp."""
    with torch.no_grad():
        m.local_geo_features += 0.25
        if getattr(m, "local_color_features", None) is not None:
            m.local_color_features -= 0.5
    m.local_point_certainties = m.local_point_certainties + 1.0
    m.local_point_ts_update = torch.full_like(m.local_point_ts_update, int(m.cur_ts))
    R.assign(m)
    R.rec(tag + ":assigned", m, ASSIGNED)


def _cycle(R, m, pts, cols, ts, sensor, is_reliable=True, **reset_kw):
    R.update(m, pts, cols, ts, is_reliable=is_reliable)
    R.rec(f"f{ts}:update", m, UPDATE)
    R.reset(m, sensor, ts, **reset_kw)
    R.rec(f"f{ts}:reset", m, LOCAL)
    _edit_and_assign(R, m, f"f{ts}")


def _lookup(m, pts):
    """The oracle's view of a frame BEFORE `update`: representatives, raw hash values, looked-up points, fp32 d2."""
    sidx = M.voxel_down_sample(pts, m.resolution)
    sp = pts[sidx]
    hv = M.hash_slots(sp, m.resolution, m.buffer_size)
    hidx = m.buffer_pt_index[hv]
    d2 = ((m.neural_points[hidx] - sp) ** 2).sum(-1) if m.neural_points.shape[0] else None
    return sidx, sp, hv, hidx, d2


def _grid(pts, voxel):
    """The integer grid of `voxel_down_sample` (utils/tools.py:929-944): shifted coordinates, v_size, linear ids."""
    offset = torch.floor(pts.min(dim=0)[0] / voxel).long()
    grid = torch.floor(pts / voxel).long() - offset
    vs = grid.max()
    return grid, int(vs), grid[:, 0] + grid[:, 1] * vs + grid[:, 2] * vs * vs


def _bits(t):
    return t.contiguous().view(torch.int32)


def _f32(v):
    return np.float32(v)


def _targets(ref_double, parent_value):
    """fp32(reference threshold), its two fp32 neighbours and the value the kernels used before ABI 11 (the square of the
    argument already rounded to fp32)."""
    t = _f32(ref_double)
    out = []
    for v in (np.nextafter(t, _f32(-np.inf)), t, np.nextafter(t, _f32(np.inf)), _f32(parent_value)):
        if not any(v == o for o in out):
            out.append(v)
    return out


def _xy_with_d2(target, x):
    """fp32 (x, y) with fp32(x*x + y*y) == target in torch's own arithmetic: x fixed, y swept over consecutive floats."""
    x = _f32(x)
    y0 = _f32(math.sqrt(float(target) - float(x) ** 2))
    ys = (y0.view(np.int32) + np.arange(-4000, 4000, dtype=np.int32)).view(np.float32)
    ys = torch.from_numpy(ys.copy())
    d2 = (torch.stack((torch.full_like(ys, float(x)), ys), 1) ** 2).sum(-1)
    hit = torch.nonzero(d2 == float(target)).flatten()
    assert hit.numel() > 0, (target, x)
    return float(x), float(ys[hit[0]])


def _cloud(seed, n_vox, res, per_voxel=2, shift=0, zshift=0):
    """`per_voxel` points in each of n_vox distinct voxels on both sides of zero, shuffled; colours with negatives."""
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(n_vox)
    # z spans the widest range: v_size (the largest shifted coordinate) stays above every x and y, so that the
    # reference's aliasing linear voxel id does not merge two of these voxels
    vox = torch.stack(((i % 16) - 8 + shift, (i // 16) - 8, (i % 23) - 11 + zshift), 1).float()
    pts = torch.cat([(vox + 0.15 + 0.7 * torch.rand(n_vox, 3, generator=g)) * res for _ in range(per_voxel)])
    perm = torch.randperm(pts.shape[0], generator=g)
    cols = torch.rand(pts.shape[0], 3, generator=g)
    cols[torch.rand(pts.shape[0], generator=g) < 0.3, 0] = -1.0
    return pts[perm], cols


TRAVEL4 = torch.tensor([0.0, 1.0, 2.0, 3.0])
KW = dict(temporal_local_map_on=True, use_mid_ts=False, range_filter_2d=True, local_map_radius=1.5,
          sorrounding_map_radius=2.5, diff_travel_dist_local=5.0)


# =================================================================== voxel down-sampling
def _sc_vds(R, pts, voxel, value, reach):
    out = R.vds(pts, voxel)
    R.rec_value("plain", out)
    outs = [out]
    for j, v in enumerate(value):
        o = R.vds(pts, voxel, v)
        R.rec_value(f"min_value{j}", o)
        outs.append(o)
    if R.oracle:
        reach(outs)


def sc_vds_count(R, N):
    """N points, ~32 per voxel at the large counts; min-value with ties inside every voxel.  131,072 points fill the 512
    blocks of the bounds kernel, one more starts its grid stride."""
    g = torch.Generator().manual_seed(N)
    pts = (torch.rand(N, 3, generator=g) - 0.5) * 4.0
    value = torch.randint(0, 4, (N,), generator=g).float()

    def reach(outs):
        n_vox = int(torch.unique(_grid(pts, 0.25)[2]).numel())
        assert all(o.numel() == n_vox for o in outs) and (N < 255 or n_vox < N)
        assert N == 1 or not torch.equal(outs[0], outs[1]) or N == 2
    _sc_vds(R, pts, 0.25, [value], reach)


def sc_vds_one_voxel(R):
    g = torch.Generator().manual_seed(1)
    pts = 0.1 + 0.8 * torch.rand(50, 3, generator=g)

    def reach(outs):
        assert _grid(pts, 1.0)[1] == 0 and all(o.numel() == 1 for o in outs)          # v_size == 0
    _sc_vds(R, pts, 1.0, [torch.rand(50, generator=g)], reach)


def sc_vds_coincident(R):
    pts = torch.tensor([[0.31, -0.12, 0.77]]).repeat(5, 1)

    def reach(outs):
        assert all(o.tolist() == [0] for o in outs)                                    # ties go to the lowest index
    _sc_vds(R, pts, 0.25, [torch.full((5,), 2.0)], reach)


def sc_vds_centres(R):
    """Points exactly on voxel centres: every distance is 0, dist / dist.max() is 0 / 0.  The expected result is the
    lowest index per voxel in ascending voxel id."""
    vox = torch.tensor([[2, 0, 0], [0, 0, 0], [1, 1, 0], [0, 0, 0], [2, 0, 0], [1, 1, 0], [0, 0, 0], [-1, -2, 0]])
    pts = (vox.float() + 0.5) * 0.5

    def reach(outs):
        centre = (torch.floor(pts / 0.5) + 0.5) * 0.5
        assert float(((pts - centre) ** 2).sum(1).max()) == 0.0
        ids = _grid(pts, 0.5)[2]
        expect = [int(torch.nonzero(ids == u)[0]) for u in torch.unique(ids)]
        assert outs[0].tolist() == expect and len(expect) == 4
    _sc_vds(R, pts, 0.5, [], reach)


def sc_vds_signs(R):
    """Both sides of zero: -0.0, exact negative boundaries and the floats next to them."""
    one = lambda v, to: float(np.nextafter(_f32(v), _f32(to)))
    xs = [-0.0, 0.0, 0.25, -0.25, one(-0.5, -9), -0.5, one(-0.5, 0), 0.5, one(0.5, 0), -1.0, one(-1.0, -9), one(0.0, -9)]
    pts = torch.tensor([[x, y, 0.1] for x in xs for y in (-0.0, 0.3, one(-0.5, -9))], dtype=torch.float32)

    def reach(outs):
        grid = torch.floor(pts / 0.5)
        assert grid[:, 0].min() == -3 and grid[:, 0].max() == 1 and bool((_bits(pts[:, 0]) == _bits(torch.tensor([-0.0]))).any())
        assert 1 < outs[0].numel() < pts.shape[0]
    _sc_vds(R, pts, 0.5, [torch.arange(pts.shape[0]).float() % 4], reach)


def sc_vds_alias(R):
    """grid.max() is reached on x, so voxel (3, 0, 0) and voxel (0, 1, 0) share the linear id 3 (the reference's id
    aliases; the kernels restate it)."""
    pts = torch.tensor([[.1, .1, .1], [3.1, .1, .1], [.1, 1.1, .1], [.12, .1, .1]])

    def reach(outs):
        grid, vs, ids = _grid(pts, 1.0)
        assert vs == 3 and int(grid[:, 0].max()) == vs and ids.tolist() == [0, 3, 3, 0]
        assert outs[0].numel() == 2                                                   # three voxels, two ids
    _sc_vds(R, pts, 1.0, [torch.tensor([1.0, 2.0, 1.0, 0.0])], reach)


def sc_vds_min_value(R):
    """Min-value variants: all-zero value (0 / 0 in the reference: bins to 0), ties inside a voxel, N = 1."""
    g = torch.Generator().manual_seed(3)
    pts = (torch.rand(300, 3, generator=g) - 0.5) * 2.0
    tied = torch.randint(0, 2, (300,), generator=g).float() * 5.0

    def reach(outs):
        ids = _grid(pts, 0.5)[2]
        lowest = [int(torch.nonzero(ids == u)[0]) for u in torch.unique(ids)]
        assert outs[1].tolist() == lowest                                             # all-zero value: lowest index
        assert outs[2].tolist() != lowest and len(lowest) < 300
    _sc_vds(R, pts, 0.5, [torch.zeros(300), tied], reach)
    one = torch.tensor([[0.3, -0.2, 0.1]])
    for j, v in enumerate((torch.tensor([0.0]), torch.tensor([4.0]))):
        R.rec_value(f"n1_{j}", R.vds(one, 0.5, v))


# =================================================================== update
def sc_update_first_frame_one_point(R):
    m = R.new_map(100_003, GEO, COL, 0.25, **KW)
    m.travel_dist = R.T(TRAVEL4)
    _cycle(R, m, torch.tensor([[0.3, -0.2, 0.1]]), torch.tensor([[0.5, 0.5, 0.5]]), 0, torch.zeros(3))
    if R.oracle:
        assert m.neural_points.shape[0] == 1 and m._last_update_mask.tolist() == [True]
    _cycle(R, m, torch.tensor([[0.31, -0.21, 0.1]]), torch.tensor([[0.1, 0.2, 0.3]]), 1, torch.zeros(3))
    if R.oracle:
        assert m.neural_points.shape[0] == 1 and m._last_update_mask.tolist() == [False]


def sc_update_count(R, Mv):
    """M representatives around one block of the classify / commit kernels; the second frame overlaps the first."""
    m = R.new_map(100_003, GEO, COL, 0.25, **KW)
    m.travel_dist = R.T(TRAVEL4)
    for ts in (0, 1):                                   # frame 1: every other voxel 23 voxels higher, so half are new
        pts, cols = _cloud(10 * Mv + ts, Mv, 0.25, zshift=23 * ts * (torch.arange(Mv) % 2))
        _cycle(R, m, pts, cols, ts, torch.tensor([0.1, -0.2, 0.0]))
        if R.oracle:
            assert m._last_sample_idx.numel() == Mv
    if R.oracle:
        u = m._last_update_mask
        assert bool(u.any()) and not bool(u.all())


def sc_update_small_table(R, S):
    """A table of S slots: many samples share a slot over three frames (the last sample wins the slot), and — frame 0
    has no valid colour — many samples refresh the colour of ONE point (the last sample wins)."""
    m = R.new_map(S, GEO, COL, 0.25, **KW)
    m.travel_dist = R.T(TRAVEL4)
    seen = {"neg": False, "disagree": False, "colour_dups": False}
    for ts, shift in ((0, 0), (1, 0), (2, 3)):
        pts, cols = _cloud(7, 40, 0.25, shift=shift)
        if ts == 0:
            cols[:, 0] = -1.0
        if ts == 1:
            cols[:, 0] = cols[:, 0].abs()
            cols[5:9, 0] = -1.0
        if R.oracle:
            sidx, sp, hv, hidx, d2 = _lookup(m, pts)
            seen["neg"] |= bool((hv < 0).any())
            if ts > 0:
                cm = (hidx > -1) & (~m.valid_color_mask[hidx]) & (cols[sidx][:, 0] >= 0.0)
                seen["colour_dups"] |= int(torch.bincount(hidx[cm]).max()) >= 2 if bool(cm.any()) else False
        _cycle(R, m, pts, cols, ts, torch.tensor([0.1, -0.2, 0.0]))
        if R.oracle and ts > 0:
            slot, upd = torch.where(hv < 0, hv + S, hv), m._last_update_mask
            for s in torch.unique(slot):
                u = upd[slot == s]
                seen["disagree"] |= bool(u.any()) and not bool(u.all())
    if R.oracle:
        assert seen["disagree"] and seen["colour_dups"] and seen["neg"] == (S > 1), seen


def sc_update_threshold(R):
    """res = 0.1, one slot: every sample looks up the one existing point at the origin, and its fp32 d2 is fp32(3 * 0.1
    ** 2), one of its fp32 neighbours, or the threshold the kernels formed before ABI 11 (fp32(3 * fp32(0.1) ** 2), one
    ulp above the reference's).  `d2 > threshold`: only values above fp32(0.03) give a new point."""
    res = 0.1
    targets = _targets(3 * res ** 2, (3.0 * float(_f32(res))) * float(_f32(res)))
    m = R.new_map(1, GEO, COL, res, temporal_local_map_on=False, local_map_radius=1.0, sorrounding_map_radius=2.0)
    _cycle(R, m, torch.tensor([[0.0, 0.0, 0.05]]), torch.tensor([[0.5, 0.5, 0.5]]), 0, torch.zeros(3))
    rows = []
    for j, t in enumerate(targets):
        x, y = _xy_with_d2(t, 0.172)
        for q in (2 * j, 2 * j + 1):                     # two placements per target, all eight in different voxels
            a, b = (x, y) if q < 4 else (y, x)
            rows.append([a if q & 1 else -a, b if q & 2 else -b, 0.05])
    rows.append([0.05, 0.05, 5.05])      # far away in z: v_size 50, so the aliasing voxel id keeps the eight apart
    pts = torch.tensor(rows, dtype=torch.float32)
    if R.oracle:
        sidx, sp, hv, hidx, d2 = _lookup(m, pts)
        assert sidx.numel() == len(rows) and bool((hidx == 0).all())
        want = torch.tensor([float(t) for t in targets])
        assert sorted(set(_bits(d2[d2 < 1.0]).tolist())) == sorted(_bits(want).tolist()), (d2.tolist(), targets)
        assert float(targets[-1]) > float(_f32(3 * res ** 2))        # the two roundings differ: the old one is above
        expect = d2 > 3 * res ** 2
        assert int(expect.sum()) == 3 and int((d2 == float(_f32(3 * res ** 2))).sum()) == 2
        assert int((d2 == float(targets[-1])).sum()) == 2            # new for the reference, existing for the old value
    R.update(m, pts, torch.rand(len(rows), 3, generator=torch.Generator().manual_seed(0)), 1)
    R.rec("threshold:update", m, UPDATE)
    if R.oracle:
        assert torch.equal(m._last_update_mask, expect) and m.neural_points.shape[0] == 1 + 3


def sc_update_travel_edge(R):
    """travel_dist[cur] - travel_dist[ts] exactly diff_travel_dist_local: not new (`>`); one ulp above: new."""
    kw = dict(KW, diff_travel_dist_local=2.0)
    m = R.new_map(100_003, GEO, COL, 0.25, **kw)
    m.travel_dist = R.T(torch.tensor([0.0, 2.0, float(np.nextafter(_f32(2.0), _f32(3.0)))]))
    pts, cols = _cloud(11, 20, 0.25)
    news = []
    for ts in range(3):
        R.update(m, pts, cols, ts)
        R.rec(f"f{ts}:update", m, UPDATE)
        news.append(int(m._last_update_mask.sum()))
    if R.oracle:
        assert news == [20, 0, 20], news


def _sc_update_config(R, temporal=True, color_on=True, colours="mixed", reliable=True):
    kw = dict(KW, temporal_local_map_on=temporal)
    m = R.new_map(100_003, GEO, COL, 0.25, color_on=color_on, **kw)
    if temporal:
        m.travel_dist = R.T(torch.tensor([0.0, 1.0, 7.0]))     # frame 2 lies outside the window of frame-0 points
    for ts, shift in ((0, 0), (1, 4), (2, 0)):
        pts, cols = _cloud(20 + ts, 60, 0.25, shift=shift)
        if colours == "none":
            cols = None
        elif colours == "negative" and ts != 1:
            cols[:, 0] = -cols[:, 0].abs() - 0.01
        elif colours == "negative":
            cols[:, 0] = cols[:, 0].abs()
        _cycle(R, m, pts, cols, ts, torch.tensor([0.1, -0.2, 0.0]), is_reliable=reliable)
    return m


def sc_update_temporal_off(R):
    m = _sc_update_config(R, temporal=False)
    if R.oracle:
        assert m.travel_dist is None and not bool(m._last_update_mask.all())


def sc_update_temporal_window_makes_new_points(R):
    m = _sc_update_config(R, temporal=True)
    if R.oracle:                                           # same clouds as temporal_off, but the window re-creates them
        assert bool(m._last_update_mask.all())


def sc_update_no_colours(R):
    m = _sc_update_config(R, color_on=False, colours="none")
    if R.oracle:
        assert m.point_colors is None and m.color_features is None and bool(m.valid_color_mask.all())
        assert not hasattr(m, "local_point_colors")


def sc_update_negative_colours(R):
    """Frames 0 and 2 carry only negative colours (no valid colour is stored), frame 1 refreshes frame-0 points."""
    kw = dict(KW)
    m = R.new_map(100_003, GEO, COL, 0.25, **kw)
    m.travel_dist = R.T(TRAVEL4)
    pts, cols = _cloud(31, 60, 0.25)
    neg = cols.clone()
    neg[:, 0] = -cols[:, 0].abs() - 0.01
    _cycle(R, m, pts, neg, 0, torch.zeros(3))
    if R.oracle:
        assert not bool(m.valid_color_mask.any())
    pos = cols.clone()
    pos[:, 0] = cols[:, 0].abs()
    _cycle(R, m, pts, pos, 1, torch.zeros(3))
    if R.oracle:
        assert m.neural_points.shape[0] == 60 and int(m.valid_color_mask.sum()) > 0
    pts2, cols2 = _cloud(32, 60, 0.25, shift=6)
    cols2[:, 0] = -1.0
    _cycle(R, m, pts2, cols2, 2, torch.zeros(3))
    if R.oracle:
        assert not bool(m.valid_color_mask[60:].any()) and m.neural_points.shape[0] > 60


def sc_update_unreliable(R):
    m = _sc_update_config(R, temporal=False, reliable=False)
    if R.oracle:
        assert bool(m.free_gs_mask.all())


# =================================================================== reset_local_map
def _sc_reset(R, m, sensor, ts, tag="reset", assign=True, **kw):
    R.reset(m, sensor, ts, **kw)
    R.rec(tag, m, LOCAL)
    if assign:
        _edit_and_assign(R, m, tag)


def sc_reset_count(R, n):
    """n points around one block: the padding element n is handled by thread n of `rst_mask_kernel` / `rst_index_kernel`,
    in a block of its own at n == 256.  n == 0 is the empty map."""
    g = torch.Generator().manual_seed(40 + n)
    pts = (torch.rand(n, 3, generator=g) - 0.5) * torch.tensor([6.0, 6.0, 2.0])
    tsc = (torch.arange(n) % 4 != 0).int() * 3                      # three quarters inside the window
    m = _direct(R, pts, tsc, tsc, **dict(KW, diff_travel_dist_local=1.5))
    m.travel_dist = R.T(TRAVEL4)
    _sc_reset(R, m, torch.tensor([0.2, -0.1, 0.0]), 3)
    if R.oracle:
        lm = m.local_mask
        assert lm.shape[0] == n + 1 and bool(lm[-1]) and int(m.global2local[-1]) == -1
        if n == 0:
            assert m.local_geo_features.shape == (1, GEO) and m.local_neural_points.shape == (0, 3)
        if n >= 255:
            assert 100 <= int((tsc == 3).sum()) < n and 0 < int(lm[:-1].sum()) < int((tsc == 3).sum())
            assert int(m.sorrounding_mask[:-1].sum()) > 0


def sc_reset_large(R):
    """70,000 points, 16 geometry features: the window count wraps its 256 shards (274 blocks) and the gather of the
    local geometry features exceeds 4096 x 256 words, so the multi-gather kernel strides."""
    n = 70_000
    g = torch.Generator().manual_seed(5)
    pts = (torch.rand(n, 3, generator=g) - 0.5) * torch.tensor([20.0, 20.0, 2.0])
    tsc = (torch.arange(n) % 50 != 0).int() * 3
    m = _direct(R, pts, tsc, tsc, geo=16, **dict(KW, diff_travel_dist_local=1.5, local_map_radius=13.6,
                                                 sorrounding_map_radius=14.0))
    m.travel_dist = R.T(TRAVEL4)
    _sc_reset(R, m, torch.zeros(3), 3)
    if R.oracle:
        nl = int(m.local_mask.sum())
        assert nl * 16 > 4096 * 256 and nl < n - n // 50 and int(m.sorrounding_mask[:-1].sum()) > 0
        assert (n + 255) // 256 > 256


def sc_reset_window(R, k, mode):
    """Exactly k points inside the window, by travel distance or by timestamp: 99 -> every point is taken, 100 and 101
    -> only those inside.  The timestamp window uses `diff_ts_local` = 7 with points on both sides of |dt| == 7."""
    n = 150
    g = torch.Generator().manual_seed(k)
    pts = (torch.rand(n, 3, generator=g) - 0.5) * torch.tensor([4.0, 4.0, 1.0])
    inside = torch.randperm(n, generator=g)[:k]
    if mode == "travel":
        tsc = torch.zeros(n, dtype=torch.int32)
        tsc[inside] = 3
        cur, kw = 3, {}
        travel = torch.tensor([0.0, 10.0, 20.0, 30.0])
    else:
        tsc = torch.full((n,), 33, dtype=torch.int32)               # |40 - 33| == 7: not inside (`<`)
        tsc[torch.arange(n) % 2 == 0] = 47
        tsc[inside] = torch.tensor([34, 40, 46, 37], dtype=torch.int32).repeat(k)[:k]
        cur, kw = 40, dict(use_travel_dist=False, diff_ts_local=7)
        travel = torch.zeros(48)
    m = _direct(R, pts, tsc, tsc, **dict(KW, diff_travel_dist_local=5.0))
    m.travel_dist = R.T(travel)
    _sc_reset(R, m, torch.zeros(3), cur, **kw)
    if R.oracle:
        if mode == "travel":
            tm = torch.abs(travel[cur] - travel[tsc.long()]) < 5.0
        else:
            tm = torch.abs(cur - tsc) < 7
        assert int(tm.sum()) == k
        both = m.local_mask[:-1] | m.sorrounding_mask[:-1]
        assert int(both.sum()) > 0
        assert bool(both[~tm].any()) == (k < 100)                   # points outside the window only below 100


def sc_reset_mid_ts(R, use_mid):
    """((create + update) / 2).int() with odd sums (1.5 -> 1, 2.5 -> 2) against the creation stamp alone."""
    n = 300
    g = torch.Generator().manual_seed(6)
    pts = (torch.rand(n, 3, generator=g) - 0.5) * torch.tensor([3.0, 3.0, 1.0])
    combos = torch.tensor([[1, 2], [2, 3], [3, 3], [1, 3], [0, 3]], dtype=torch.int32)[torch.arange(n) % 5]
    m = _direct(R, pts, combos[:, 0], combos[:, 1], **dict(KW, use_mid_ts=use_mid, diff_travel_dist_local=15.0))
    travel = torch.tensor([0.0, 10.0, 20.0, 30.0])
    m.travel_dist = R.T(travel)
    _sc_reset(R, m, torch.zeros(3), 3)
    if R.oracle:
        ts_mid = ((combos[:, 0] + combos[:, 1]) / 2).int()
        assert bool(((combos[:, 0] + combos[:, 1]) % 2 == 1).any()) and not torch.equal(ts_mid, combos[:, 0])
        used = ts_mid if use_mid else combos[:, 0]
        tm = torch.abs(travel[3] - travel[used.long()]) < 15.0
        assert int(tm.sum()) == (180 if use_mid else 120)           # both above 100: the window is applied
        assert torch.equal(m.local_mask[:-1] | m.sorrounding_mask[:-1], tm)


def sc_reset_range_filter(R, flag2d):
    """Pairs of points that differ only in z: the 2D filter gives both the same class, the 3D filter does not."""
    g = torch.Generator().manual_seed(8)
    xy = (torch.rand(60, 2, generator=g) - 0.5) * 4.0
    pts = torch.cat((torch.cat((xy, torch.zeros(60, 1)), 1), torch.cat((xy, torch.full((60, 1), 2.0)), 1)))
    z = torch.zeros(120, dtype=torch.int32)
    m = _direct(R, pts, z, z, **dict(KW, temporal_local_map_on=False, range_filter_2d=flag2d))
    _sc_reset(R, m, torch.zeros(3), 0)
    if R.oracle:
        lo, hi = m.local_mask[:60], m.local_mask[60:120]
        assert torch.equal(lo, hi) == flag2d and bool(lo.any())


def sc_reset_temporal_off(R):
    n = 300
    g = torch.Generator().manual_seed(9)
    pts = (torch.rand(n, 3, generator=g) - 0.5) * torch.tensor([6.0, 6.0, 1.0])
    tsc = (torch.arange(n) % 2).int() * 3
    m = _direct(R, pts, tsc, tsc, **dict(KW, temporal_local_map_on=False))
    _sc_reset(R, m, torch.zeros(3), 3)
    if R.oracle:                                            # old points are local although 150 lie inside a window
        assert m.travel_dist is None and bool(m.local_mask[:-1][tsc == 0].any())


def sc_reset_nothing_local(R):
    n = 300
    g = torch.Generator().manual_seed(10)
    pts = (torch.rand(n, 3, generator=g) - 0.5) * 4.0
    z = torch.zeros(n, dtype=torch.int32)
    m = _direct(R, pts, z, z, **KW)
    m.travel_dist = R.T(TRAVEL4)
    _sc_reset(R, m, torch.tensor([1000.0, 0.0, 0.0]), 0)
    if R.oracle:
        assert int(m.local_mask.sum()) == 1 and int(m.sorrounding_mask.sum()) == 1
        assert m.local_geo_features.shape[0] == 1 and bool((m.global2local[:-1] == 1).all())


def sc_reset_everything_local(R):
    n = 300
    g = torch.Generator().manual_seed(11)
    pts = (torch.rand(n, 3, generator=g) - 0.5) * 4.0
    z = torch.zeros(n, dtype=torch.int32)
    m = _direct(R, pts, z, z, **dict(KW, local_map_radius=50.0, sorrounding_map_radius=60.0))
    m.travel_dist = R.T(TRAVEL4)
    _sc_reset(R, m, torch.zeros(3), 0)
    if R.oracle:
        assert bool(m.local_mask.all()) and int(m.sorrounding_mask.sum()) == 1
        assert torch.equal(m.global2local[:-1], torch.arange(n))


def sc_reset_no_colours(R):
    n = 257
    g = torch.Generator().manual_seed(12)
    pts = (torch.rand(n, 3, generator=g) - 0.5) * 6.0
    z = torch.zeros(n, dtype=torch.int32)
    m = _direct(R, pts, z, z, color_on=False, **KW)
    m.travel_dist = R.T(TRAVEL4)
    _sc_reset(R, m, torch.zeros(3), 0)
    if R.oracle:
        assert m.point_colors is None and not hasattr(m, "local_point_colors") and 1 < int(m.local_mask.sum()) < n


def sc_reset_radius_thresholds(R):
    """Radii 0.7 and 5.1, sensor at the origin, 2D filter: points whose fp32 d2 is fp32(0.7 ** 2) / fp32(5.1 ** 2), an
    fp32 neighbour, or the threshold formed before ABI 11 (the square of the fp32-rounded radius, one ulp below the
    reference's for both).  `d2 < radius ** 2` decides local / surrounding / outside."""
    rows, want, k = [], [], 0
    for radius, x in ((0.7, 0.69), (5.1, 5.0)):
        k = k or len(rows)
        for j, t in enumerate(_targets(radius ** 2, float(_f32(radius)) ** 2)):
            a, b = _xy_with_d2(t, x)
            rows.append([a if j & 1 else -a, -b if j & 2 else b, 0.3 * j])
            want.append(float(t))
    g = torch.Generator().manual_seed(13)
    pts = torch.cat((torch.tensor(rows, dtype=torch.float32), (torch.rand(40, 3, generator=g) - 0.5) * 12.0))
    z = torch.zeros(pts.shape[0], dtype=torch.int32)
    m = _direct(R, pts, z, z, **dict(KW, temporal_local_map_on=False, local_map_radius=0.7, sorrounding_map_radius=5.1))
    _sc_reset(R, m, torch.zeros(3), 0)
    if R.oracle:
        d2 = (pts[:len(rows), :2] ** 2).sum(-1)
        assert _bits(d2).tolist() == _bits(torch.tensor(want)).tolist()
        for radius in (0.7, 5.1):
            ref, parent = _f32(radius ** 2), _f32(float(_f32(radius)) ** 2)
            assert parent != ref and int((d2 == float(ref)).sum()) == 1 and int((d2 == float(parent)).sum()) == 1
        assert 0 < k < len(rows)
        assert m.local_mask[:k].tolist() == (d2[:k] < 0.7 ** 2).tolist() and 0 < int(m.local_mask[:k].sum()) < k
        assert m.sorrounding_mask[k:len(rows)].tolist() == (d2[k:] < 5.1 ** 2).tolist()
        assert 0 < int(m.sorrounding_mask[k:len(rows)].sum()) < len(rows) - k


def sc_assign_fallback(R):
    """`assign_local_to_global` after edits, once with the row list of the reset and once rebuilt from `local_mask`
    (`_local_idx` deleted: the local map was set by other code)."""
    n = 300
    g = torch.Generator().manual_seed(14)
    pts = (torch.rand(n, 3, generator=g) - 0.5) * 6.0
    z = torch.zeros(n, dtype=torch.int32)
    m = _direct(R, pts, z, z, **KW)
    m.travel_dist = R.T(TRAVEL4)
    _sc_reset(R, m, torch.zeros(3), 2, tag="with_row_list")
    R.reset(m, torch.tensor([0.5, 0.5, 0.0]), 3)
    had = m.__dict__.pop("_local_idx", None)
    assert (had is not None) == R.hip
    _edit_and_assign(R, m, "from_mask")
    if R.oracle:
        assert 1 < int(m.local_mask.sum()) < n and int((m.point_ts_update == 3).sum()) == int(m.local_mask.sum()) - 1


# =================================================================== loop closure
def _closure_map(R, n=60, S=100_003, **kw):
    g = torch.Generator().manual_seed(15)
    pts = (torch.rand(n, 3, generator=g) - 0.5) * 6.0 + 0.01
    m = _direct(R, pts, torch.arange(n) % 4, torch.arange(n) % 4, buffer_size=S, **dict(KW, **kw))
    m.travel_dist = R.T(torch.tensor([0.0, 1.0, 2.0, 3.0, 10.0]))
    m.cur_ts = 4
    return m


def sc_prune_count(R, extra):
    """Exactly `min_prune_count` prunable points: kept (`>`); one more: pruned.  Timestamps -1 and -T index the travel
    distances from the end, as python does."""
    n, min_count = 60, 20
    m = _closure_map(R, n)
    tsu = torch.full((n,), 4, dtype=torch.int32)
    tsu[1::2] = -1                                                  # travel[-1] == travel[4]: active
    k = min_count + extra
    tsu[:k] = torch.tensor([0, 1, -5, 2, -4, 3], dtype=torch.int32).repeat(k)[:k]     # -5 == -T -> 0, -4 -> 1
    cert = torch.full((n,), 5.0)
    cert[:k] = 0.1
    cert[30:34] = 0.1                                               # uncertain but active: kept
    tsu[40:43] = 0                                                  # inactive but certain: kept
    m.point_ts_update, m.point_certainties = R.T(tsu), R.T(cert)
    pruned = R.prune(m, 1.0, min_count)
    R.rec_value("pruned", pruned)
    R.rec("after", m, tuple(k_ for k_ in GLOBAL if k_ != "buffer_pt_index"))
    if R.oracle:
        assert bool((tsu == -5).any()) and bool((tsu == -1).any())
        assert pruned == (extra > 0) and m.neural_points.shape[0] == (n - k if extra else n)


def sc_adjust(R, kind):
    """Identity poses (fp32 and fp64) leave the positions bitwise unchanged; a non-identity fp32 pose against the oracle
    at 2e-6.  257 points, mid timestamps with odd sums, timestamp -1 (python indexing)."""
    n = 257
    m = _closure_map(R, n, use_mid_ts=True)
    tsu = (torch.arange(n) % 3 + 1).int()
    m.point_ts_update = R.T(tsu)
    tsc = (torch.arange(n) % 4).int()
    tsc[5], tsu[5] = -1, -1
    m.point_ts_create, m.point_ts_update = R.T(tsc), R.T(tsu)
    before = m.neural_points.detach().cpu().clone()
    dt = torch.float64 if kind == "identity64" else torch.float32
    pose = torch.eye(4, dtype=torch.float64).repeat(5, 1, 1)
    if kind == "pose32":
        for t in range(5):
            a, b = 0.3 * (t + 1), -0.1 * t
            rz = torch.tensor([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]], dtype=torch.float64)
            rx = torch.tensor([[1.0, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]], dtype=torch.float64)
            pose[t, :3, :3] = rz @ rx
            pose[t, :3, 3] = torch.tensor([0.5 * t, -1.0, 0.25 * t], dtype=torch.float64)
    R.adjust(m, pose.to(dt))
    R.rec("adjusted", m, ("neural_points", "point_orientations"))
    after = m.neural_points.detach().cpu()
    if kind != "pose32":
        assert torch.equal(_bits(after), _bits(before))             # holds for the oracle and for the kernels
    if R.oracle:
        assert bool(((tsc + tsu) % 2 == 1).any()) and (kind != "pose32" or not torch.equal(after, before))


def sc_rehash_empty(R):
    """`recreate_hash` on a map without points: the stale table is cleared to -1 and nothing else happens.  The oracle's
    down-sampling does not take an empty cloud; its `recreate_hash` starts by refilling the table with -1, which is the
    whole expected effect here."""
    m = R.new_map(101, GEO, COL, 0.25, **KW)
    m.travel_dist = R.T(TRAVEL4)
    m.buffer_pt_index = R.T(torch.arange(101) - 3)
    if R.hip:
        R.recreate(m, None, True, True, 0)
    else:
        assert m.neural_points.shape[0] == 0
        m.buffer_pt_index = torch.full((m.buffer_size,), -1, dtype=torch.int64)
    R.rec("table", m, ("buffer_pt_index",))
    assert bool((m.buffer_pt_index == -1).all()) and m.buffer_pt_index.shape[0] == 101


def sc_rehash_small_table(R, kept):
    """30 voxels with three points each into 7 slots: duplicate slots, the last representative wins; `kept_points`
    True keeps the map and stores the representatives' indices, False reduces the map to them."""
    g = torch.Generator().manual_seed(16)
    i = torch.arange(30)
    vox = torch.stack(((i % 6) - 3, (i // 6) - 2, (i % 11) - 5), 1).float()     # v_size 10: no aliased ids
    pts = torch.cat([(vox + 0.1 + 0.8 * torch.rand(30, 3, generator=g)) * 0.25 for _ in range(3)])
    pts = pts[torch.randperm(90, generator=g)]
    tsc = torch.randint(0, 4, (90,), generator=g).int()
    cert = torch.randint(0, 5, (90,), generator=g).float()
    m = _direct(R, pts, tsc, tsc, buffer_size=7, cert=cert, **KW)
    m.travel_dist = R.T(torch.tensor([0.0, 1.0, 2.0, 3.0, 4.0]))
    R.recreate(m, torch.zeros(3), kept, kept, 3)
    R.rec("rehash", m, GLOBAL + LOCAL)
    if R.oracle:
        assert m.neural_points.shape[0] == (90 if kept else 30)
        used = m.buffer_pt_index[m.buffer_pt_index >= 0]
        hv = M.hash_slots(pts, 0.25, 7)
        assert used.numel() <= 7 < 30 and bool((hv < 0).any())


SCENARIOS = {}
for _N in (1, 2, 255, 256, 257, 131072, 131073):
    SCENARIOS[f"vds_count_{_N}"] = (lambda R, N=_N: sc_vds_count(R, N))
for _f in (sc_vds_one_voxel, sc_vds_coincident, sc_vds_centres, sc_vds_signs, sc_vds_alias, sc_vds_min_value,
           sc_update_first_frame_one_point):
    SCENARIOS[_f.__name__[3:]] = _f
for _M in (255, 256, 257):
    SCENARIOS[f"update_count_{_M}"] = (lambda R, Mv=_M: sc_update_count(R, Mv))
for _S in (1, 7):
    SCENARIOS[f"update_small_table_{_S}"] = (lambda R, S=_S: sc_update_small_table(R, S))
for _f in (sc_update_threshold, sc_update_travel_edge, sc_update_temporal_off,
           sc_update_temporal_window_makes_new_points, sc_update_no_colours, sc_update_negative_colours,
           sc_update_unreliable):
    SCENARIOS[_f.__name__[3:]] = _f
for _n in (0, 1, 255, 256, 257):
    SCENARIOS[f"reset_count_{_n}"] = (lambda R, n=_n: sc_reset_count(R, n))
SCENARIOS["reset_large"] = sc_reset_large
for _mode in ("travel", "timestamps"):
    for _k in (99, 100, 101):
        SCENARIOS[f"reset_window_{_mode}_{_k}"] = (lambda R, k=_k, mode=_mode: sc_reset_window(R, k, mode))
for _b in (True, False):
    SCENARIOS[f"reset_mid_ts_{_b}"] = (lambda R, b=_b: sc_reset_mid_ts(R, b))
    SCENARIOS[f"reset_range_filter_2d_{_b}"] = (lambda R, b=_b: sc_reset_range_filter(R, b))
for _f in (sc_reset_temporal_off, sc_reset_nothing_local, sc_reset_everything_local, sc_reset_no_colours,
           sc_reset_radius_thresholds, sc_assign_fallback):
    SCENARIOS[_f.__name__[3:]] = _f
for _e in (0, 1):
    SCENARIOS[f"prune_count_min_plus_{_e}"] = (lambda R, e=_e: sc_prune_count(R, e))
for _kind in ("identity32", "identity64", "pose32"):
    SCENARIOS[f"adjust_{_kind}"] = (lambda R, kind=_kind: sc_adjust(R, kind))
SCENARIOS["rehash_empty"] = sc_rehash_empty
for _b in (True, False):
    SCENARIOS[f"rehash_small_table_kept_{_b}"] = (lambda R, b=_b: sc_rehash_small_table(R, b))


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_oracle_reaches_the_branch(name):
    """No GPU: the oracle alone; the scenario asserts that its inputs reach the branch it is named after."""
    R = _Run(hip=False)
    SCENARIOS[name](R)
    assert len(R.snaps) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_hip_matches_oracle(name):
    cpu, hip = _Run(hip=False), _Run(hip=True)
    SCENARIOS[name](cpu)
    SCENARIOS[name](hip)
    _compare(hip, cpu, tol=2e-6 if name == "adjust_pose32" else None)


# ------------------------------------------------------------------- timestamps beyond the trajectory
def _oob_map(R):
    m = _closure_map(R, 60)
    tsu = torch.full((60,), 4, dtype=torch.int32)
    tsu[7] = -6                                                     # -T - 1 with T = 5
    m.point_ts_update = R.T(tsu)
    return m


def test_oracle_timestamp_below_minus_T_is_an_index_error():
    m = _oob_map(_Run(hip=False))
    assert int(m.travel_dist.shape[0]) == 5 and int(m.point_ts_update.min()) == -6
    with pytest.raises(IndexError):
        M.prune_map(m, 1.0, 20)


@pytest.mark.gpu
def test_hip_timestamp_below_minus_T_is_an_index_error():
    R = _Run(hip=True)
    m = _oob_map(R)
    with pytest.raises(IndexError):
        R.prune(m, 1.0, 20)
    assert int(m.neural_points.shape[0]) == 60


# =================================================================== row copies through the C ABI
ROW_BYTES = (1, 3, 4, 12, 20)
OFFSETS = ((0, 0), (1, 0), (0, 1))                      # (source, destination) base offsets in bytes


def _byte_path(row_bytes, src_off, dst_off):
    """map.hip: rows move as 4-byte words only when the row size and both bases are multiples of 4."""
    return row_bytes % 4 != 0 or src_off % 4 != 0 or dst_off % 4 != 0


def test_row_copy_cases_cover_both_kernels():
    taken = {(rb, so, do): _byte_path(rb, so, do) for rb in ROW_BYTES for so, do in OFFSETS}
    assert {rb for (rb, so, do), b in taken.items() if not b} == {4, 12, 20}           # the word kernel
    assert all(taken[(rb, 1, 0)] and taken[(rb, 0, 1)] for rb in (4, 12, 20))         # byte kernel, rows % 4 == 0
    assert all(taken[(rb, 0, 0)] for rb in (1, 3))


def _row_copy_inputs(row_bytes, n_rows, n, unique):
    g = torch.Generator().manual_seed(row_bytes + n)
    table = torch.randint(0, 256, (n_rows, row_bytes), generator=g, dtype=torch.uint8)
    idx = torch.randperm(n_rows, generator=g)[:n] if unique else torch.randint(0, n_rows, (n,), generator=g)
    if n >= 3 and not unique:
        idx[0], idx[1], idx[2] = n_rows - 1, 0, n_rows - 1          # repeated indices, first and last row
    return table, idx


@pytest.mark.gpu
@pytest.mark.parametrize("src_off,dst_off", OFFSETS)
@pytest.mark.parametrize("row_bytes", ROW_BYTES)
@pytest.mark.parametrize("n", [0, 300])
def test_gather_rows_matches_torch_indexing(n, row_bytes, src_off, dst_off):
    from pings_amd import _lib

    L = _lib.lib()
    table, idx = _row_copy_inputs(row_bytes, 77, n, unique=False)
    src = torch.zeros(src_off + table.numel() + 8, dtype=torch.uint8, device="cuda")
    src[src_off:src_off + table.numel()] = table.flatten().cuda()
    dst = torch.full((dst_off + n * row_bytes + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    idx_d = idx.cuda()
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    _lib.check(L.pings_gather_rows(src.data_ptr() + src_off, row_bytes, _lib.ptr(idx_d), n, dst.data_ptr() + dst_off,
                                   _lib.stream_ptr(src.device)), "pings_gather_rows")
    expect = torch.full_like(dst, 0xAB).cpu()
    expect[dst_off:dst_off + n * row_bytes] = table[idx].flatten()
    assert torch.equal(dst.cpu(), expect)                           # the rows, and not a byte before or behind them


@pytest.mark.gpu
@pytest.mark.parametrize("src_off,dst_off", OFFSETS)
@pytest.mark.parametrize("row_bytes", ROW_BYTES)
@pytest.mark.parametrize("n", [0, 60])
def test_scatter_rows_matches_torch_indexing(n, row_bytes, src_off, dst_off):
    from pings_amd import _lib

    L = _lib.lib()
    rows, idx = _row_copy_inputs(row_bytes, 300, n, unique=True)    # rows[:n] go to the distinct rows idx of a table
    rows = rows[:n]
    g = torch.Generator().manual_seed(99)
    table = torch.randint(0, 256, (300, row_bytes), generator=g, dtype=torch.uint8)
    src = torch.zeros(src_off + n * row_bytes + 8, dtype=torch.uint8, device="cuda")
    src[src_off:src_off + n * row_bytes] = rows.flatten().cuda()
    dst = torch.full((dst_off + table.numel() + 8,), 0xCD, dtype=torch.uint8, device="cuda")
    dst[dst_off:dst_off + table.numel()] = table.flatten().cuda()
    idx_d = idx.cuda()
    _lib.check(L.pings_scatter_rows(src.data_ptr() + src_off, row_bytes, _lib.ptr(idx_d), n, dst.data_ptr() + dst_off,
                                    _lib.stream_ptr(src.device)), "pings_scatter_rows")
    table[idx] = rows
    expect = torch.full_like(dst, 0xCD).cpu()
    expect[dst_off:dst_off + table.numel()] = table.flatten()
    assert torch.equal(dst.cpu(), expect)


def _multi_jobs(n_jobs):
    """(row_bytes, rows) per job: byte rows, word rows, one job without rows."""
    widths = [1, 3, 4, 12, 20, 2, 8, 16, 5, 28, 32, 7, 64, 36, 1, 4, 12]
    return [(widths[j], 0 if j == 6 else 40 + 3 * j) for j in range(n_jobs)]


def test_multi_gather_cases_hold_the_limit_and_an_empty_job():
    jobs = _multi_jobs(16)
    assert len(jobs) == 16 and sum(r == 0 for _, r in jobs) == 1 and len(_multi_jobs(17)) == 17
    assert any(w % 4 for w, _ in jobs) and any(w % 4 == 0 for w, _ in jobs)


@pytest.mark.gpu
def test_gather_rows_multi_takes_16_jobs_and_refuses_17():
    from pings_amd import _abi, _lib

    L = _lib.lib()
    g = torch.Generator().manual_seed(21)
    idx = torch.randint(0, 120, (100,), generator=g)
    idx_d = idx.cuda()

    def build(n_jobs):
        jobs, keep = (_abi.GatherJob * n_jobs)(), []
        for j, (w, rows) in enumerate(_multi_jobs(n_jobs)):
            table = torch.randint(0, 256, (120, w), generator=g, dtype=torch.uint8)
            src, dst = table.cuda(), torch.full((rows * w + 8,), 0xEE, dtype=torch.uint8, device="cuda")
            keep.append((table, src, dst, w, rows))
            jobs[j] = _abi.GatherJob(src.data_ptr(), dst.data_ptr() if rows else None, w, rows)
        return jobs, keep

    jobs, keep = build(16)
    _lib.check(L.pings_gather_rows_multi(jobs, 16, _lib.ptr(idx_d), _lib.stream_ptr(idx_d.device)), "gather_rows_multi")
    for table, _, dst, w, rows in keep:
        expect = torch.full((rows * w + 8,), 0xEE, dtype=torch.uint8)
        expect[:rows * w] = table[idx[:rows]].flatten()
        assert torch.equal(dst.cpu(), expect), (w, rows)
    jobs, keep = build(17)
    status = L.pings_gather_rows_multi(jobs, 17, _lib.ptr(idx_d), _lib.stream_ptr(idx_d.device))
    assert status == 1                                              # PINGS_ERR_ARG, before any launch
    with pytest.raises(_lib.PingsHipError, match="status 1"):
        _lib.check(status, "pings_gather_rows_multi")
    torch.cuda.synchronize()
    for _, _, dst, w, rows in keep:
        assert bool((dst == 0xEE).all()), (w, rows)                 # nothing was written


MASKS = {
    "one_set": [1], "one_clear": [0], "all_clear": [0] * 300, "all_set": [1] * 300,
    "last_set": [0, 1, 0] * 100 + [1], "last_clear": [1, 1, 0] * 100 + [0],
}


def test_mask_row_cases_cover_the_count_and_the_last_word():
    assert {(sum(v), v[-1]) for v in MASKS.values()} == {(1, 1), (0, 0), (300, 1), (101, 1), (200, 0)}
    assert [len(v) for v in MASKS.values()][:2] == [1, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MASKS))
def test_mask_rows_count_rows_and_last(name):
    from pings_amd import _lib, neural_map as NM

    mask = torch.tensor(MASKS[name], dtype=torch.bool)
    rows, count, last = NM._mask_rows(_lib.lib(), mask.cuda())
    assert count == int(mask.sum()) and last == int(mask[-1])
    assert torch.equal(rows[:count].cpu(), torch.nonzero(mask).flatten())
