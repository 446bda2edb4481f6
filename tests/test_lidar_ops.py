"""The LiDAR frame front-end on the device (pings_amd/lidar_ops.py, csrc/lidar.hip) against tests/lidar_ref.py (float64).

Gates:
  exact cases   dyadic inputs, so float32 arithmetic is exact in any order: everything equal bit for bit
  projection    outside the undecided sets of lidar_ref (a point within 1e-3 px of a half-integer or within 1e-4 of a
                depth bound; the pixels around it): visibility, pixel (through the colour it picks from an image of
                distinct values), colours and indicator exactly, depth to the project's 1e-4 relative gate.  The random
                scenes fail when more than 1 % of the visible points are undecided.
  crop          equal outside the rows within 1e-5 (relative) of a threshold, at most 0.1 % of the rows
  deskew        1e-4 relative (conftest.rel_err) against the float64 restatement; two runs bit-equal
  host reads    pinned through `_lib.sync_counts`
Every reference is float64 from float32 inputs and is computed on the CPU once per case.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lidar_ref as LR
from conftest import GOLDEN, rel_err
from pings_amd import _lib, lidar_ops, neural_map

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def _reads(fn):
    _lib.sync_counts(reset=True)
    out = fn()
    return out, _lib.sync_counts(reset=True)


def _depth_agrees(got, ref64, undecided):
    got = got.detach().cpu().numpy().astype(np.float64)
    ok = ~undecided
    assert np.array_equal((got != 0)[ok], (ref64 != 0)[ok])
    assert rel_err(torch.from_numpy(np.where(ok, got, 0.0)), torch.from_numpy(np.where(ok, ref64, 0.0))) <= 1e-4


def _pyramid_is_interpolate_of_level0(levels, H, W):
    d = levels[0]
    assert tuple(d.shape) == (1, H, W)
    for k in range(1, 4):
        d = F.interpolate(d.unsqueeze(0), scale_factor=0.5, mode="nearest-exact").squeeze(0)
        assert tuple(levels[k].shape) == (1, H >> k, W >> k) == tuple(d.shape)
        assert torch.equal(levels[k], d), k


def _pyramid_mask(und):
    out = [und]
    for _ in range(3):
        und = und[1:(und.shape[0] // 2) * 2:2, 1:(und.shape[1] // 2) * 2:2]
        out.append(und)
    return out


# ================================================================ exact cases
K_EXACT = np.array([[2.0, 0.0, 0.5], [0.0, 2.0, 0.5], [0.0, 0.0, 1.0]])


def _exact_points(H, W):
    """(x, y, z) with d = z and pixel (x', y') = ((2 x + z / 2) / z, (2 y + z / 2) / z): z = 2 puts a point at x + 0.5."""
    rows = [(2.0, 1.0, 2.0),              # x' = 2.5 -> 2 (half to even)
            (3.0, 1.0, 2.0),              # x' = 3.5 -> 4
            (-1.0, 1.0, 2.0),             # x' = -0.5 -> -0, pixel 0
            (1.0, -1.0, 2.0),             # y' = -0.5 -> row 0
            (W - 1.0, 1.0, 2.0),          # x' = W - 0.5: W (outside) for even W, W - 1 for odd W
            (1.0, H - 1.0, 2.0),          # y' = H - 0.5 likewise
            (1.0, 1.0, 0.0),              # d == 0 -> -1e-6
            (1.0, 1.0, -2.0),             # d < 0
            (0.5, 0.5, 1.0),              # d == min_depth: strict
            (100.0, 100.0, 100.0),        # d == max_depth: strict (pixel 2.5, 2.5)
            (0.75, 0.75, 1.5),            # just inside: pixel (1.5, 1.5) -> (2, 2)
            (2.5, 2.5, 2.0), (2.5, 2.5, 2.0), (5.0, 5.0, 4.0),      # pixel (3, 3): minima 2, 2 and a 4 behind them
            (float("nan"), 1.0, 2.0), (1.0, 1.0, float("nan")),
            (float("inf"), 1.0, 2.0)]
    return np.array(rows, np.float32)


@pytest.mark.parametrize("H,W", [(8, 8), (9, 15)])
def test_exact_cases_are_bitwise(H, W):
    pts = _exact_points(H, W)
    n = len(pts)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    img = np.stack([c * 1024.0 + v * 32.0 + u for c in range(3)]).astype(np.float32)       # names its pixel
    rgb_in = np.tile(np.array([[0.25, 0.5, 0.75, 1.0]], np.float32), (n, 1))
    T = np.eye(4)
    ref_rgb, ref_depth, und_pt, _, pr = LR.project_points_to_cam(pts, rgb_in, img, T, K_EXACT, 1.0)
    rgb = _t(rgb_in)
    (out, depth), reads = _reads(lambda: lidar_ops.project_points_to_cam(_t(pts), rgb, _t(img), _t(T), _t(K_EXACT), 1.0))
    assert reads == {} and out is rgb
    assert np.array_equal(out.cpu().numpy().astype(np.float64), ref_rgb)
    assert np.array_equal(depth.cpu().numpy().astype(np.float64), ref_depth)
    got = out.cpu().numpy()
    pix = lambda r: (int(got[r, 0]) // 32, int(got[r, 0]) % 32)  # noqa: E731  (v, u) from the colour of channel 0
    assert pix(0) == (2, 2) and pix(1) == (2, 4) and pix(2) == (2, 0) and pix(3) == (0, 2)
    assert (got[4, 3] == 0.0) == (W % 2 == 1) and (got[5, 3] == 0.0) == (H % 2 == 1)
    if W % 2:
        assert pix(4) == (2, W - 1)
    if H % 2:
        assert pix(5) == (H - 1, 2)
    for r in (6, 7, 8, 9, 14, 15, 16):
        assert np.array_equal(got[r], rgb_in[r]), r                                        # not visible: left alone
    assert pix(10) == (2, 2) and pix(11) == pix(12) == pix(13) == (3, 3)
    d = depth.cpu().numpy()[0]
    assert d[3, 3] == 2.0 and d[2, 2] == 1.5 and d[2, 0] == 2.0 and d[0, 2] == 2.0
    assert (d != 0).sum() == len(set(zip(pr.v[pr.visible].tolist(), pr.u[pr.visible].tolist())))
    lv = lidar_ops.depth_pyramid(depth)
    _pyramid_is_interpolate_of_level0(lv, H, W)


# ================================================================ launch edges
def _run_method(sc, cams, only, **kw):
    ds = LR.Dataset(sc, device=DEV, cams=cams, set_depth_img=lidar_ops.set_depth_img, **kw)
    ref = LR.project_to_cams(LR.Dataset(sc, cams=cams, **kw), only)
    return ds, ref


def _check_method(ds, ref, sc, only, reads, companions=True):
    assert reads == ({"mask_rows_count": 1} if only else {})
    ok = ~ref.undecided
    cloud = ds.cur_point_cloud_torch
    assert cloud.dim() == 2 and cloud.shape[1] == 6 and cloud.dtype is torch.float32
    if only:
        # the kept rows, then every companion, must be the stable compaction of the decided rows
        got_rows = np.nonzero(ref.keep | ref.undecided)[0]
        # the x, y, z of a row identify it: scene points are distinct
        xyz = {tuple(r): i for i, r in enumerate(sc.cloud[:, :3].tolist())}
        rows = np.array([xyz[tuple(r)] for r in cloud[:, :3].cpu().numpy().tolist()], dtype=np.int64)
        assert np.all(np.diff(rows) > 0)
        kept = np.zeros(len(sc.cloud), bool)
        kept[rows] = True
        assert np.array_equal(kept[ok], ref.keep[ok]) and set(rows) <= set(got_rows)
        base = LR.Dataset(sc)
        for name in ("cur_point_ts_torch", "cur_point_normals", "cur_sem_labels_torch", "cur_sem_labels_full"):
            want, got = getattr(base, name), getattr(ds, name)
            assert (got is None) == (not companions), name
            if got is not None:
                assert torch.equal(got.cpu(), want[torch.from_numpy(rows)]), name
        sel = ok[rows]
        assert np.array_equal(cloud.cpu().numpy().astype(np.float64)[sel], ref.cloud[rows][sel])
    else:
        assert cloud.shape[0] == len(sc.cloud)
        assert np.array_equal(cloud.cpu().numpy().astype(np.float64)[ok], ref.cloud[ok])
    for name, cam in ds.cur_cam_img.items():
        if cam is None:
            assert name not in ref.cams
            continue
        assert cam.depth_on
        _pyramid_is_interpolate_of_level0(cam.depth_image_list, sc.H, sc.W)
        for k, und in enumerate(_pyramid_mask(ref.cams[name].undecided)):
            _depth_agrees(cam.depth_image_list[k][0], ref.cams[name].levels[k][0], und)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("H,W", [(8, 8), (9, 15), (33, 70)])
def test_projection_at_launch_edges(n, H, W):
    sc = LR.scene(n, H, W, seed=n + H, ncam=2)
    for cams in ([sc.names[0]], list(sc.names), [sc.names[0], "none", sc.names[1]]):
        for only in (False, True):
            ds, ref = _run_method(sc, cams, only)
            _, reads = _reads(lambda: lidar_ops.project_to_cams(ds, only))
            _check_method(ds, ref, sc, only, reads)


# ================================================================ random scenes
@functools.lru_cache(maxsize=None)
def _random_scene(n, H, W):
    sc = LR.scene(n, H, W, seed=11, ncam=2)
    ref = {only: LR.project_to_cams(LR.Dataset(sc), only) for only in (False, True)}
    return sc, ref


@pytest.mark.parametrize("n,H,W", [(4096, 48, 64), (20000, 240, 320)])
def test_projection_random_scene(n, H, W):
    sc, refs = _random_scene(n, H, W)
    visible = refs[True].keep.sum()
    assert visible > 0.5 * n and refs[True].undecided.sum() <= 0.01 * visible
    for only in (False, True):
        ds = LR.Dataset(sc, device=DEV, set_depth_img=lidar_ops.set_depth_img)
        _, reads = _reads(lambda: lidar_ops.project_to_cams(ds, only))
        _check_method(ds, refs[only], sc, only, reads)
    # one camera through the free function: indicator column, rows that keep what they held
    nm = sc.names[0]
    rgb_in = torch.rand(n, 4, generator=torch.Generator().manual_seed(1))
    ref_rgb, ref_depth, und_pt, und_px, pr = LR.project_points_to_cam(sc.cloud, rgb_in, sc.img[nm], sc.T[nm], sc.K[nm],
                                                                      sc.min_range)
    assert und_pt.sum() <= 0.01 * pr.visible.sum()
    rgb = rgb_in.to(DEV)
    (out, depth), reads = _reads(lambda: lidar_ops.project_points_to_cam(
        _t(sc.cloud), rgb, _t(sc.img[nm]), _t(sc.T[nm]), _t(sc.K[nm]), min_depth=sc.min_range))
    assert reads == {} and out is rgb
    assert np.array_equal(out.cpu().numpy().astype(np.float64)[~und_pt], ref_rgb[~und_pt])
    _depth_agrees(depth[0], ref_depth[0], und_px)
    # twice: bit-equal (the minimum does not depend on the order)
    rgb2 = rgb_in.to(DEV)
    _, depth2 = lidar_ops.project_points_to_cam(_t(sc.cloud), rgb2, _t(sc.img[nm]), _t(sc.T[nm]), _t(sc.K[nm]),
                                                min_depth=sc.min_range)
    assert torch.equal(depth, depth2) and torch.equal(rgb, rgb2)


def test_projection_matches_the_reference_fixture():
    with np.load(GOLDEN / "lidar_project.npz") as z:
        z = {k: np.asarray(z[k]) for k in z.files}
    sc = LR.scene(int(z["n"]), int(z["H"]), int(z["W"]), int(z["seed"]))
    nm = sc.names[0]
    _, _, und_pt, und_px, _ = LR.project_points_to_cam(sc.cloud, z["rgb_in"], sc.img[nm], sc.T[nm], sc.K[nm], sc.min_range)
    out, depth = lidar_ops.project_points_to_cam(_t(sc.cloud), _t(z["rgb_in"]), _t(sc.img[nm]), _t(sc.T[nm]), _t(sc.K[nm]),
                                                 min_depth=sc.min_range)
    assert np.array_equal(out.cpu().numpy()[~und_pt], z["rgb"][~und_pt])
    _depth_agrees(depth[0], z["depth"][0].astype(np.float64), und_px)


def test_camera_time_offsets_move_the_extrinsics_on_the_device():
    sc, _ = _random_scene(4096, 48, 64)
    tran = np.eye(4)
    tran[:3, :3] = LR.rotations(LR.look_along_x(0.3, 0.1)[:3, :3], 0.2)[0]
    tran[:3, 3] = (0.8, 0.1, -0.05)
    tran = tran.astype(np.float32).astype(np.float64)
    stamps = {"lidar": 10.0, sc.names[0]: 9.93, sc.names[1]: 9.98}
    out = {}
    for dev in ("cpu", DEV):
        ds = LR.Dataset(sc, device=dev, companions=False, set_depth_img=lidar_ops.set_depth_img)
        ds.cur_sensor_ts = stamps
        out[dev] = ds
    ref = LR.project_to_cams(out["cpu"], True, tran)
    still = LR.project_to_cams(LR.Dataset(sc, companions=False), True)
    assert (ref.keep != still.keep).sum() > 50                                # the offsets matter in this scene
    assert ref.undecided.sum() <= 0.01 * ref.keep.sum()
    ds = out[DEV]
    _, reads = _reads(lambda: lidar_ops.project_to_cams(ds, True, torch.as_tensor(tran, dtype=torch.float32).to(DEV)))
    _check_method(ds, ref, sc, True, reads, companions=False)
    assert ds.cur_point_ts_torch is None and ds.cur_point_normals is None and ds.cur_sem_labels_torch is None


# ================================================================ depth pyramid
@pytest.mark.parametrize("shape", ["33x70", "9x15"])
def test_depth_pyramid_matches_the_reference_fixture(shape):
    with np.load(GOLDEN / "lidar_depth.npz") as z:
        want = [np.asarray(z[f"{shape}.depth{k}"]) for k in range(4)]
    d = _t(want[0])
    levels, reads = _reads(lambda: lidar_ops.depth_pyramid(d))
    assert reads == {} and levels[0] is d
    for k in range(4):
        assert np.array_equal(levels[k].cpu().numpy(), want[k]), k
    cam = LR.Cam(np.zeros((3, 8, 8), np.float32), DEV, lidar_ops.set_depth_img)
    cam.set_depth_img(torch.from_numpy(want[0]))                              # moved to the camera's device first
    assert cam.depth_on and all(np.array_equal(cam.depth_image_list[k].cpu().numpy(), want[k]) for k in range(4))


# ================================================================ crop and select
def test_crop_thresholds_are_strict():
    rows = np.array([(3.0, 4.0, 0.0, 0.0),      # dist 5 == min_range
                     (3.0, 4.0, 0.5, 0.0),      # 2-D: still 5; 3-D: above
                     (6.0, 8.0, 0.0, 0.0),      # dist 10 == max_range
                     (6.0, 7.5, 0.0, 0.0),      # inside
                     (4.0, 4.0, -1.0, 0.0),     # z == min_z
                     (4.0, 4.0, 2.0, 0.0),      # z == max_z
                     (4.0, 4.0, 1.5, 0.0),      # inside
                     (2.0, 3.0, 6.0, 0.0),      # 3-D: dist 7, z above max_z
                     (np.nan, 4.0, 0.0, 0.0), (4.0, 4.0, np.nan, 0.0)], np.float32)
    for xy in (True, False):
        want, _ = LR.crop(rows, -1.0, 2.0, 5.0, 10.0, xy)
        got, reads = _reads(lambda: lidar_ops.crop_rows(_t(rows), -1.0, 2.0, 5.0, 10.0, xy))
        assert reads == {} and got.dtype is torch.bool
        assert np.array_equal(got.cpu().numpy(), want)
    assert lidar_ops.crop_rows(_t(rows), -1.0, 2.0, 5.0, 10.0, True).cpu().tolist() == \
        [False, False, False, True, False, False, True, False, False, False]
    assert lidar_ops.crop_rows(_t(rows), -1.0, 2.0, 5.0, 10.0, False).cpu().tolist()[1] is True


@pytest.mark.parametrize("n", [1, 64, 65, 3000])
def test_crop_and_select_random(n):
    p = LR.crop_cloud(n, seed=n)
    args = (-3.0, 6.0, 2.75, 40.0)
    for xy in (True, False):
        want, near = LR.crop(p, *args, xy)
        assert near.mean() <= 1e-3
        wide = torch.zeros(n, 7, device=DEV)
        wide[:, 1:5] = _t(p)
        for cloud in (_t(p), wide[:, 1:5]):                                   # contiguous rows and a row-strided view
            got = lidar_ops.crop_rows(cloud, *args, xy).cpu().numpy()
            assert np.array_equal(got[~near], want[~near])
    mask = lidar_ops.crop_rows(_t(p), *args, True)
    g = torch.Generator().manual_seed(n)
    comps = [_t(p), torch.rand(n, 1, generator=g, dtype=torch.float64).to(DEV), None,
             torch.randint(0, 5, (n,), generator=g).to(DEV), torch.rand(n, 2, 3, generator=g).to(DEV).half(),
             torch.rand(n, generator=g).to(DEV) > 0.5]
    outs, reads = _reads(lambda: lidar_ops.select_rows(mask, *comps))
    assert reads == {"mask_rows_count": 1} and len(outs) == len(comps) and outs[2] is None
    for c, o in zip(comps, outs):
        if c is not None:
            assert o.dtype is c.dtype and torch.equal(o, c[mask])
    rows = torch.nonzero(mask).flatten()
    outs, reads = _reads(lambda: lidar_ops.select_rows(rows, comps[0], None, comps[3]))
    assert reads == {} and outs[1] is None and torch.equal(outs[0], comps[0][rows]) and torch.equal(outs[2], comps[3][rows])


# ================================================================ deskew
def _pose(theta, seed=2, t=(0.7, -0.2, 0.05)):
    g = np.random.default_rng(seed)
    a = g.normal(size=3)
    a /= np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(theta) * Kx + (1 - np.cos(theta)) * (Kx @ Kx)
    T[:3, 3] = t
    return T


@pytest.mark.parametrize("n", [1, 64, 65, 4097])
@pytest.mark.parametrize("stride", [3, 6])
@pytest.mark.parametrize("ts_kind", ["f32", "f64_column"])
def test_deskew(n, stride, ts_kind):
    g = np.random.default_rng(n + stride)
    base = g.normal(0, 10.0, (n, stride)).astype(np.float32)
    ts64 = g.uniform(100.0, 100.1, n)
    ts = _t(ts64.astype(np.float32)) if ts_kind == "f32" else _t(ts64, torch.float64).reshape(n, 1)
    pose_dtype = torch.float32 if ts_kind == "f32" else torch.float64
    for theta in (0.0, 0.02, 3.0):
        pose = torch.as_tensor(_pose(theta), dtype=pose_dtype)
        for ref in (0.0, 0.5, 1.0):
            cloud = _t(base)
            pts = cloud[:, :3]                                                # stride 6: a view of the cloud's rows
            (out, reads) = _reads(lambda: lidar_ops.deskew(pts, ts, pose.to(DEV), ts_ref_pose=ref))
            assert out is pts and reads == {}
            want = LR.deskew(base, ts, pose, ref)
            got = cloud.cpu().numpy()
            assert np.array_equal(got[:, 3:], base[:, 3:])                    # only x, y, z are written
            if n == 1:
                assert np.isnan(got[:, :3]).all() and np.isnan(want).all()    # max == min: 0 / 0
                continue
            assert rel_err(torch.from_numpy(got[:, :3]), torch.from_numpy(want)) <= 1e-4, (theta, ref)
            if theta == 0.0:                                                  # R(s) = I exactly: only s t is added
                s = LR.normalised_time(ts, ref).astype(np.float32)
                t32 = pose[:3, 3].numpy().astype(np.float32)
                assert np.array_equal(got[:, :3], base[:, :3] + s[:, None] * t32)
            again = _t(base)
            lidar_ops.deskew(again[:, :3], ts, pose.to(DEV), ts_ref_pose=ref)
            assert torch.equal(again, cloud)


@pytest.mark.parametrize("diffs", [None, (0.125, -0.25)])
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
def test_deskew_multi_lidar(diffs, idx_dtype):
    n = 4097
    g = np.random.default_rng(5)
    base = g.normal(0, 10.0, (n, 4)).astype(np.float32)
    ts = _t(g.random(n).astype(np.float32))
    idx = torch.from_numpy(g.integers(0, 4, n)).to(idx_dtype)                 # 3 names no LiDAR of the rig
    rig = [_pose(1.1, 5, (0.5, 0.2, -0.1)), _pose(2.0, 6, (-1.0, 0.0, 0.3))]
    pose = torch.as_tensor(_pose(0.3, 4), dtype=torch.float32)
    cloud = _t(base)
    out, reads = _reads(lambda: lidar_ops.deskew(cloud, ts, pose.to(DEV), 0.5, idx.to(DEV), rig, diffs))
    assert out is cloud and reads == {}
    want = LR.deskew(base, ts, pose, 0.5, idx, rig, diffs)
    got = cloud.cpu().numpy()
    assert rel_err(torch.from_numpy(got[:, :3]), torch.from_numpy(want)) <= 1e-4
    other = idx.numpy() == 3
    assert other.sum() > 500 and np.array_equal(got[other], base[other])      # untouched, bit for bit
    moved = np.abs(got[~other, :3] - base[~other, :3]).max(1)
    assert (moved > 1e-3).mean() > 0.9
    empty = _t(base)
    assert lidar_ops.deskew(empty, ts, pose.to(DEV), 0.5, idx.to(DEV), [], diffs) is empty
    assert np.array_equal(empty.cpu().numpy(), base)                          # the empty list: nothing moves


def test_deskew_constant_stamps_none_and_empty():
    base = np.random.default_rng(0).normal(0, 5.0, (65, 3)).astype(np.float32)
    pose = _t(_pose(0.02))
    pts = _t(base)
    assert lidar_ops.deskew(pts, None, pose) is pts and np.array_equal(pts.cpu().numpy(), base)
    lidar_ops.deskew(pts, torch.full((65,), 7.5, device=DEV), pose)
    assert torch.isnan(pts).all()
    with pytest.raises(RuntimeError):
        lidar_ops.deskew(torch.zeros(0, 3, device=DEV), torch.zeros(0, device=DEV), pose)


@pytest.mark.parametrize("theta", [0.0, 1e-7, 0.02, 1.0, 3.0])
def test_slerp_pose(theta):
    T = _pose(theta)
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 2e-7)):
        pose = torch.as_tensor(T, dtype=dtype)
        for ratio in (0.0, 0.35, 0.5, 1.0, 1.4):
            got, reads = _reads(lambda: lidar_ops.slerp_pose(pose.to(DEV), ratio, 0.5))
            assert reads == {} and got.dtype is dtype and got.is_cuda and tuple(got.shape) == (4, 4)
            want = LR.slerp_pose(pose, ratio, 0.5)
            assert np.abs(got.cpu().numpy().astype(np.float64) - want).max() <= tol * max(1.0, np.abs(want).max())
            if theta == 0.0:
                assert torch.equal(got[:3, :3].cpu(), torch.eye(3, dtype=dtype))


# ================================================================ the two other methods on a stand-in
def test_filter_and_correct_and_voxel_downsample_on_a_stand_in():
    sc, _ = _random_scene(4096, 48, 64)
    ds = LR.Dataset(sc, device=DEV, companions=False)
    g = torch.Generator().manual_seed(3)
    ts = torch.rand(4096, generator=g)
    lidx = torch.randint(0, 3, (4096,), generator=g)
    ds.cur_point_ts_torch, ds.cur_point_lidar_idx_torch = ts.to(DEV), lidx.to(DEV)
    cfg = ds.config
    want, near = LR.crop(sc.cloud, cfg.min_z, cfg.max_z, cfg.min_range, ds.crop_max_range, True)
    assert near.mean() <= 1e-3 and 0.2 < want.mean() < 0.9
    _, reads = _reads(lambda: lidar_ops.filter_and_correct(ds))
    assert reads == {"mask_rows_count": 1}
    cloud = ds.cur_point_cloud_torch
    assert cloud.shape[1] == 6 and ds.cur_sem_labels_torch is None and ds.cur_point_normals is None
    xyz = {tuple(r): i for i, r in enumerate(sc.cloud[:, :3].tolist())}
    rows = np.array([xyz[tuple(r)] for r in cloud[:, :3].cpu().numpy().tolist()])
    kept = np.zeros(4096, bool)
    kept[rows] = True
    assert np.all(np.diff(rows) > 0) and np.array_equal(kept[~near], want[~near])
    assert torch.equal(ds.cur_point_ts_torch.cpu(), ts[rows]) and torch.equal(ds.cur_point_lidar_idx_torch.cpu(), lidx[rows])
    assert np.array_equal(cloud.cpu().numpy(), sc.cloud[rows])

    ds = LR.Dataset(sc, device=DEV)
    base = LR.Dataset(sc)
    _, alone = _reads(lambda: neural_map.voxel_down_sample(ds.cur_point_cloud_torch[:, :3], ds.train_voxel_m))
    _, reads = _reads(lambda: lidar_ops.voxel_downsample_points_for_mapping(ds))
    assert reads == alone
    rows = LR.voxel_downsample_rows(base)
    assert np.array_equal(ds.cur_point_cloud_torch.cpu().numpy(), sc.cloud[rows])
    for name in ("cur_point_ts_torch", "cur_sem_labels_torch", "cur_sem_labels_full"):
        assert torch.equal(getattr(ds, name).cpu(), getattr(base, name)[torch.from_numpy(rows)]), name
    assert torch.equal(ds.cur_point_normals.cpu(), base.cur_point_normals)    # the reference leaves the normals alone

    ds = LR.Dataset(sc, device=DEV, companions=False)
    lidar_ops.voxel_downsample_points_for_mapping(ds)
    assert ds.cur_point_ts_torch is None and ds.cur_sem_labels_torch is None and ds.cur_sem_labels_full is None
    assert np.array_equal(ds.cur_point_cloud_torch.cpu().numpy(), sc.cloud[rows])


def test_no_images_and_unsupported_inputs():
    sc, _ = _random_scene(4096, 48, 64)
    ds = LR.Dataset(sc, device=DEV)
    ds.cur_cam_img = None
    before = ds.cur_point_cloud_torch.clone()
    assert lidar_ops.project_to_cams(ds) is None and torch.equal(ds.cur_point_cloud_torch, before)
    ds = LR.Dataset(sc, device=DEV)
    ds.cur_point_cloud_torch = ds.cur_point_cloud_torch.double()               # the kept original's, and none is kept
    with pytest.raises(_lib.PingsHipError, match="none was kept"):
        lidar_ops.project_to_cams(ds)
    with pytest.raises(_lib.PingsHipError):
        lidar_ops.crop_rows(torch.zeros(4, 3), -1, 1, 1, 2, True)
