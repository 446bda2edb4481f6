"""LiDAR scans fused into the sparse TSDF volume on the device (TSDFVolume.integrate_points, csrc/tsdf_points.hip,
DESIGN §2.9b) against the fp64 numpy restatement (tests/tsdf_points_ref.py) on the analytic sphere scans and on
single rays.

Outside the voxels the reference calls marginal (their share is asserted from the reference alone in
tests/test_tsdf_points_ref.py) the block set and every weight are exact, tsdf and colour pass the project's 1e-4 gate
(`rel_err`; the largest reference tsdf is 1), and a voxel without an updating sample keeps its bits."""
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import tsdf_points_ref as P
import tsdf_ref as R
from conftest import rel_err

KMAT = np.array([[R.K[0], 0.0, R.K[2]], [0.0, R.K[1], R.K[3]], [0.0, 0.0, 1.0]])
MODES = [("point", False), ("point", True), ("ray", False), ("ray", True)]


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


@functools.lru_cache(maxsize=None)
def scans(carved=False):
    return [(dev(p), dev(c), dev(o)) for p, c, o in P.sphere_scans(carved)]


def new_volume(voxel=R.VOXEL, trunc=R.TRUNC, **kw):
    from pings_amd import tsdf_ops

    return tsdf_ops.TSDFVolume(voxel, trunc, **kw)


def carve_kw(carved):
    return dict(space_carving=carved, max_range=P.CARVE_RANGE if carved else np.inf)


def fuse(vol, sdf_mode="point", carved=False, n=3, **kw):
    for p, c, o in scans(carved)[:n]:
        vol.integrate_points(p, o, c if vol.color else None, sdf_mode=sdf_mode, **carve_kw(carved), **kw)
    return vol


@functools.lru_cache(maxsize=None)
def fused(sdf_mode="point", carved=False):
    """The three scans in a volume of ample capacity; read-only."""
    return fuse(new_volume(), sdf_mode, carved)


def blocks_of(vol):
    return [tuple(r) for r in vol.block_coords().cpu().tolist()]


def agree(vol, ref, box=P.BOX):
    """Block set, weights exactly, tsdf and colour within 1e-4, all outside the reference's marginal set."""
    assert (set(blocks_of(vol)) ^ set(ref.coords)) <= ref.marginal_blocks
    if not ref.marginal_blocks:
        assert blocks_of(vol) == ref.coords
    t, w, c, m = ref.dense(*box)
    dt, dw, dc = vol.dense(*box)
    assert bool(torch.isfinite(dt).all())
    keep = torch.from_numpy(~m)
    upd = w > 0
    print(f"blocks {vol.n_blocks} / {ref.n_blocks}, updated {upd.sum()}, marginal {(m & upd).sum()}, "
          f"weight mismatches outside {(dw.cpu()[keep] != torch.from_numpy(w)[keep]).sum().item()}, "
          f"tsdf rel_err {rel_err(dt.cpu()[keep], torch.from_numpy(t)[keep]):.3e}")
    assert torch.equal(dw.cpu()[keep].double(), torch.from_numpy(w)[keep])
    assert rel_err(dt.cpu()[keep], torch.from_numpy(t)[keep]) <= 1e-4
    if vol.color:
        assert rel_err(dc.cpu()[keep], torch.from_numpy(c)[keep]) <= 1e-4
    else:
        assert dc is None
    return int(upd.sum())


def one_scan(points, origin, voxel=0.5, trunc=1.0, box=((-24, -24, -24), (24, 24, 24)), color=False, **kw):
    """One scan of `points` (numpy [N, 3]) into a fresh device volume and a fresh reference."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    cols = P.point_color(points) if color else None
    ref = P.Volume(voxel, trunc, color=color)
    ref.integrate_points(points, origin, cols, **kw)
    vol = new_volume(voxel, trunc, color=color)
    vol.integrate_points(dev(points), origin, dev(cols) if color else None, **kw)
    return vol, ref, agree(vol, ref, box)


# ---------------------------------------------------------------- 1. the three scans against the reference
@pytest.mark.gpu
@pytest.mark.parametrize("sdf_mode,carved", MODES)
def test_every_scan_matches_the_reference_outside_the_marginal_voxels(sdf_mode, carved):
    _, snaps = P.sphere_reference(sdf_mode, carved)
    vol = new_volume()
    for (p, c, o), (coords, (t, w, col, m), marginal_blocks, counts) in zip(scans(carved), snaps):
        before = [x.clone() for x in vol.dense(*P.BOX)]
        vol.integrate_points(p, o, c, sdf_mode=sdf_mode, **carve_kw(carved))
        assert (set(blocks_of(vol)) ^ set(coords)) <= marginal_blocks
        if not marginal_blocks:
            assert blocks_of(vol) == coords                       # and in the same slot order
        dt, dw, dc = vol.dense(*P.BOX)
        keep = torch.from_numpy(~m)
        tt, tw, tc = torch.from_numpy(t), torch.from_numpy(w), torch.from_numpy(col)
        print(f"blocks {vol.n_blocks}, weight mismatches outside the marginal set "
              f"{(dw.cpu()[keep].double() != tw[keep]).sum().item()} (inside: "
              f"{(dw.cpu()[~keep].double() != tw[~keep]).sum().item()} of {(~keep).sum().item()}), "
              f"tsdf {rel_err(dt.cpu()[keep], tt[keep]):.3e} colour {rel_err(dc.cpu()[keep], tc[keep]):.3e}")
        assert torch.equal(dw.cpu()[keep].double(), tw[keep])
        assert rel_err(dt.cpu()[keep], tt[keep]) <= 1e-4
        assert rel_err(dc.cpu()[keep], tc[keep]) <= 1e-4
        # a voxel without an updating sample in this call keeps every bit, in touched blocks too
        still = (keep & torch.from_numpy(P.counts_dense(counts) == 0)).to(dt.device)
        assert int(still.sum()) > 8 * 512
        for x, y in zip(before, (dt, dw, dc)):
            assert torch.equal(x[still], y[still])


# ---------------------------------------------------------------- 2. determinism and growth
def _store(vol):
    n = vol.n_blocks
    return [vol._keys[:n], vol._tsdf[:n], vol._weight[:n]] + ([vol._color[:n]] if vol.color else [])


@pytest.mark.gpu
@pytest.mark.parametrize("carved", [False, True])
def test_shuffled_rows_and_a_second_run_give_the_same_bits(carved):
    a = fused("point", carved)
    b = fuse(new_volume(), "point", carved)
    s = new_volume()
    for k, (p, c, o) in enumerate(scans(carved)):
        perm = torch.randperm(p.shape[0], generator=torch.Generator().manual_seed(k)).to(p.device)
        s.integrate_points(p[perm].contiguous(), o, c[perm].contiguous(), **carve_kw(carved))
    assert a.n_blocks > 100
    for x, y, z in zip(_store(a), _store(b), _store(s)):
        assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.gpu
def test_a_store_that_outgrows_its_capacity_keeps_values_and_slots():
    small = new_volume(capacity_blocks=8)
    fuse(small, n=1)
    first = small.block_coords().clone()
    assert first.shape[0] > 8 and small.capacity >= first.shape[0]
    for p, c, o in scans()[1:]:
        small.integrate_points(p, o, c)
    big = fused()
    assert torch.equal(small.block_coords()[:first.shape[0]], first)
    for x, y in zip(_store(small), _store(big)):
        assert torch.equal(x, y)


# ---------------------------------------------------------------- 3. single rays and boundaries
CASES = {
    "a single point": ((2.3, 1.1, -0.7), (-1.2, 0.4, 0.6)),
    # the faces between g = -1 and g = 0 lie at -0.25 on every axis: a corner of cubes and of blocks
    "a point on a cube face and on a block corner": ((-0.25, -0.25, -0.25), (1.75, 0.875, 0.375)),
    "a ray parallel to an axis": ((2.125, 0.0625, -0.125), (0.125, 0.0625, -0.125)),
    "a point closer than sdf_trunc": ((0.4, 0.3, 0.2), (0.1, 0.1, 0.1)),
    "the sensor inside a block with negative indices": ((-1.8, -2.8, -4.3), (-3.3, -2.1, -5.2)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("sdf_mode", ["point", "ray"])
@pytest.mark.parametrize("case", list(CASES))
def test_single_rays_and_boundaries(case, sdf_mode):
    from pings_amd import _lib

    p, o = CASES[case]
    _lib.sync_counts(reset=True)
    vol, ref, updated = one_scan([p], o, sdf_mode=sdf_mode)
    assert _lib.sync_counts() == {"tsdf_touch_points": 1}              # the call's one host read
    assert updated > 0 and vol.n_blocks > 0
    vol, ref, carved = one_scan([p], o, sdf_mode=sdf_mode, space_carving=True, max_range=8.0, color=True)
    assert carved >= updated
    if case == "the sensor inside a block with negative indices":
        assert int(vol.block_coords().max()) < 0
    if case == "a ray parallel to an axis":
        # exactly the cubes of the line, all in one row of voxels
        _, w, _ = vol.dense((-24, 0, 0), (24, 1, 1))
        assert int(w.sum()) == int(vol.dense((-24, -24, -24), (24, 24, 24))[1].sum()) == carved


# ---------------------------------------------------------------- 4. filters and empty scans
@pytest.mark.gpu
def test_range_filters_and_non_finite_rows_are_left_out():
    pts, col, o = (x.copy() for x in P.sphere_scans()[0])
    pts[::7] = np.nan
    pts[3::11, 1] = np.inf
    pts[5::13, 2] = -np.inf
    ok = np.isfinite(pts).all(1)
    r = np.linalg.norm(pts[ok].astype(np.float64) - o.astype(np.float64), axis=1)
    lo, hi = 2.2, 2.6
    assert np.abs(r - lo).min() > 1e-5 and np.abs(r - hi).min() > 1e-5   # no range that fp32 could put on the other side
    assert (r <= lo).sum() > 50 and (r >= hi).sum() > 20 and ((r > lo) & (r < hi)).sum() > 50
    for kw in (dict(), dict(min_range=lo), dict(max_range=hi), dict(min_range=lo, max_range=hi, space_carving=True)):
        ref = P.Volume(R.VOXEL, R.TRUNC)
        ref.integrate_points(pts, o, col, **kw)
        vol = new_volume()
        vol.integrate_points(dev(pts), dev(o), dev(col), **kw)
        assert agree(vol, ref) > 1000


@pytest.mark.gpu
def test_an_empty_or_all_invalid_scan_is_a_no_op_with_one_host_read():
    from pings_amd import _lib

    vol = fuse(new_volume(), n=1)
    before = [x.clone() for x in _store(vol)]
    p, c, o = scans()[1]
    _lib.sync_counts(reset=True)
    vol.integrate_points(p[:0], o, c[:0])
    vol.integrate_points(torch.full_like(p, float("nan")), o, c)
    vol.integrate_points(p, o, c, min_range=50.0)
    vol.integrate_points(p, o, c, max_range=0.5, space_carving=True)
    assert _lib.sync_counts() == {"tsdf_touch_points": 4}
    for x, y in zip(before, _store(vol)):
        assert torch.equal(x, y)
    empty = new_volume()
    empty.integrate_points(p[:0], o, c[:0])
    assert empty.n_blocks == 0 and empty.extract_mesh().faces.shape == (0, 3)


# ---------------------------------------------------------------- 5. colour, the weight cap, depth views
@pytest.mark.gpu
def test_colour_off():
    vol = fuse(new_volume(color=False))
    t, w, c = vol.dense(*P.BOX)
    assert c is None and vol._color is None
    bt, bw, _ = fused().dense(*P.BOX)
    assert torch.equal(t, bt) and torch.equal(w, bw)


@pytest.mark.gpu
def test_max_weight_clamps_and_feeds_the_next_call():
    ref = P.Volume(R.VOXEL, R.TRUNC)
    vol = new_volume()
    for (p, c, o), (hp, hc, ho) in zip(scans(), P.sphere_scans()):
        ref.integrate_points(hp, ho, hc, max_weight=2)
        vol.integrate_points(p, o, c, max_weight=2)
    assert agree(vol, ref) > 10000
    w = vol.dense(*P.BOX)[1]
    assert float(w.max()) == 2.0 and float(fused().dense(*P.BOX)[1].max()) > 2.0


@pytest.mark.gpu
def test_a_depth_view_and_a_scan_share_a_volume():
    depth, img, E = R.sphere_frames()[0]
    hp, hc, ho = P.sphere_scans()[1]
    ref = P.Volume(R.VOXEL, R.TRUNC)
    ref.integrate(depth, R.K, E, img)
    ref.integrate_points(hp, ho, hc, sdf_mode="ray")
    vol = new_volume()
    vol.integrate(dev(depth), KMAT, E, dev(img))
    vol.integrate_points(*(scans()[1][i] for i in (0, 2, 1)), sdf_mode="ray")
    assert agree(vol, ref) > 10000
    assert float(vol.dense(*P.BOX)[1].max()) >= 2.0              # some voxel was seen by both


# ---------------------------------------------------------------- 6. arguments and the extent status
@pytest.mark.gpu
def test_arguments_that_raise():
    from pings_amd import _abi, _lib

    p, c, o = scans()[0]
    vol = new_volume()
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        vol.integrate_points(torch.zeros(5, 4, device="cuda"), o, c)
    with pytest.raises(ValueError):
        vol.integrate_points(p, o, c[:-1])
    with pytest.raises(_lib.PingsHipError, match="CPU tensor"):
        vol.integrate_points(p.cpu(), o, c)
    with pytest.raises(ValueError, match="colour"):
        vol.integrate_points(p, o)
    with pytest.raises(ValueError, match="finite max_range"):
        vol.integrate_points(p, o, c, space_carving=True)
    with pytest.raises(ValueError, match="sdf_mode"):
        vol.integrate_points(p, o, c, sdf_mode="projective")
    with pytest.raises(ValueError, match="origin"):
        vol.integrate_points(p, (0.0, 1.0), c)
    with pytest.raises(ValueError, match="max_weight"):
        vol.integrate_points(p, o, c, max_weight=0)
    many = torch.zeros(_abi.TSDF_POINTS_MAX + 1, 3, device="cuda")
    with pytest.raises(ValueError, match="at most"):
        new_volume(color=False).integrate_points(many, o)
    assert vol.n_blocks == 0
    # the origin as a host sequence and as a device tensor
    vol.integrate_points(p, o.cpu().tolist(), c)
    other = new_volume()
    other.integrate_points(p, o, c)
    for x, y in zip(_store(vol), _store(other)):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_the_extent_status_raises_after_the_rest_is_applied():
    from pings_amd import _lib

    p, c, o = scans()[0]
    far = torch.cat([p, torch.tensor([[1.0e6, 0.0, 0.0]], device=p.device)])       # grid index 2e7 > 2^23
    vol = new_volume()
    with pytest.raises(_lib.PingsHipError, match="2\\*\\*20"):
        vol.integrate_points(far, o, torch.cat([c, c[:1]]))
    want = new_volume()
    want.integrate_points(p, o, c)
    for x, y in zip(_store(vol), _store(want)):
        assert torch.equal(x, y)


# ---------------------------------------------------------------- 7. extraction
@pytest.mark.gpu
def test_the_fused_scans_mesh_into_the_sphere():
    ref, _ = P.sphere_reference("ray", False)
    lo, hi = ref.bounds()
    t, w, c, _ = ref.dense(lo, hi)
    rv, rf, _ = R.extract(R.masked(t, w), c, lo, ref.origin, R.VOXEL)
    want = np.abs(np.linalg.norm(rv, axis=1) - 1.0).mean()
    mesh = fused("ray", False).extract_mesh(chunk=40)
    v, f = mesh.verts.double(), mesh.faces
    got = float((v.norm(dim=1) - 1.0).abs().mean())
    print(f"faces {f.shape[0]} (reference {rf.shape[0]}), mean | |v| - 1 | {got:.3e} (reference {want:.3e})")
    assert f.shape[0] > 1000
    tri = v[f]
    normal = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert bool(((normal * tri.mean(1)).sum(1) > 0).all())
    assert got <= 2.0 * want                  # a marginal voxel may move single vertices


# ---------------------------------------------------------------- 8. the SLAMDataset method
@pytest.mark.gpu
def test_install_adds_lidar_tsdf_fusion(tmp_path):
    from pings_amd import lidar_ops, mesh_ops, neural_map, tsdf_ops
    from test_mesh_ops import read_ply

    a = 0.3
    rot = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    poses, clouds = [], []
    for pts, _, o in [P.sphere_scans()[0]] + P.sphere_scans():           # frame 0 is skipped: nothing to deskew it with
        pose = np.eye(4)
        pose[:3, :3], pose[:3, 3] = rot, o.astype(np.float64)
        poses.append(pose)
        local = (pts.astype(np.float64) - pose[:3, 3]) @ rot                       # rows of R^T (p - c)
        clouds.append(np.concatenate([local, np.ones((len(local), 1))], 1).astype(np.float32))

    module = NS(SLAMDataset=type("SLAMDataset", (), {}))
    tsdf_ops.install(module)
    assert not hasattr(module.SLAMDataset, "lidar_tsdf_fusion")             # the default call adds nothing
    tsdf_ops.install(module, lidar=True)
    ds = module.SLAMDataset()
    ds.device, ds.gt_poses, ds.gt_pose_provided, ds.total_pc_count = "cuda", poses, True, len(poses)
    ds.config = NS(kitti_correction_on=False, deskew=True, vox_down_m=0.01, min_z=-10.0, max_z=10.0, min_range=0.5,
                   max_range=4.0, range_filter_2d=False, pgo_on=False, track_on=False)
    calls = []
    ds.init_temp_data = lambda: setattr(ds, "cur_point_cloud_torch", None)
    ds.read_frame_with_loader = lambda i, *_: setattr(ds, "cur_point_cloud_torch", dev(clouds[i]))
    ds.get_tran_in_frame = lambda i, gt: (i, gt)
    ds.deskew_at_frame = calls.append
    path = tmp_path / "lidar.ply"
    got = ds.lidar_tsdf_fusion(R.VOXEL, sdf_mode="ray", use_gt_pose=True, output_path=path)
    assert isinstance(got, mesh_ops.Mesh)                                    # Open3D does not import here
    assert calls == [(1, True), (2, True), (3, True)]

    vol = tsdf_ops.TSDFVolume(R.VOXEL, 4.0 * R.VOXEL, color=False)
    for cloud, pose in list(zip(clouds, poses))[1:]:
        cloud = dev(cloud)
        cloud, = lidar_ops.select_rows(neural_map.voxel_down_sample(cloud[:, :3], 0.01), cloud)
        cloud, = lidar_ops.select_rows(lidar_ops.crop_rows(cloud, -10.0, 10.0, 0.5, 4.0, False), cloud)
        T = torch.as_tensor(pose, device="cuda")
        world = (cloud[:, :3].double() @ T[:3, :3].T + T[:3, 3]).float().contiguous()
        vol.integrate_points(world, T[:3, 3], sdf_mode="ray")
    want = vol.extract_mesh()
    assert want.faces.shape[0] > 1000 and want.colors is None
    for x, y in zip(got, want):
        assert (x is None and y is None) or torch.equal(x, y)
    _, rv, rf = read_ply(path)
    assert np.array_equal(rf.astype(np.int64), want.faces.cpu().numpy())
    assert np.array_equal(np.stack([rv["x"], rv["y"], rv["z"]], -1), want.verts.cpu().numpy().astype(np.float64))
