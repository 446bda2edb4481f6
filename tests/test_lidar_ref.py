"""tests/lidar_ref.py (the float64 restatement of the LiDAR frame front-end) against the reference's own results
(tests/golden/lidar_*.npz, tools/make_lidar_golden.py) and against scipy's rotations; `lidar_ops.install` on stand-ins.

CPU only.  Gates: masks, pixel colours, kept rows and the hit pattern of the depth images are equal outside the
undecided sets of lidar_ref (whose sizes are capped here: 1 % of the visible points, 0.1 % of the cropped rows); a depth
value is a float32 result compared with a float64 one, so it is held to the project's 1e-4 relative gate, as on the GPU.
`deskewing` and `slerp_pose` have no fixture (the reference needs `roma`): they are held to scipy at 1e-12.
"""
import types

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

import lidar_ref as LR
from conftest import GOLDEN, rel_err
from pings_amd import lidar_ops

THETAS = (0.0, 1e-7, 0.02, 1.0, 3.0)


def _load(name):
    with np.load(GOLDEN / f"lidar_{name}.npz") as z:
        return {k: np.asarray(z[k]) for k in z.files}


def _depth_agrees(got32, ref64, undecided):
    ok = ~undecided
    assert np.array_equal((got32 != 0)[ok], (ref64 != 0)[ok])
    assert rel_err(torch.from_numpy(np.where(ok, got32, 0.0)), torch.from_numpy(np.where(ok, ref64, 0.0))) <= 1e-4


def _pyramid_mask(und):
    out = [und]
    for _ in range(3):
        und = und[1:(und.shape[0] // 2) * 2:2, 1:(und.shape[1] // 2) * 2:2]
        out.append(und)
    return out


# ================================================================ fixtures
@pytest.mark.parametrize("name", ["xy", "xyz"])
def test_crop_matches_the_reference(name):
    z = _load("crop")
    mask, near = LR.crop(z[f"{name}.points"], z["min_z"], z["max_z"], z["min_range"], z["max_range"],
                         bool(z[f"{name}.on_xy_plane"]))
    assert near.mean() <= 1e-3
    assert np.array_equal(mask[~near], z[f"{name}.mask"][~near])
    assert 0.3 < mask.mean() < 0.7 and not mask[17] and not mask[33]        # both outcomes; the NaN rows are dropped


def test_projection_matches_the_reference():
    z = _load("project")
    sc = LR.scene(int(z["n"]), int(z["H"]), int(z["W"]), int(z["seed"]))
    nm = sc.names[0]
    rgb, depth, und_pt, und_px, pr = LR.project_points_to_cam(sc.cloud, z["rgb_in"], sc.img[nm], sc.T[nm], sc.K[nm],
                                                              sc.min_range)
    assert pr.visible.sum() > 2000 and und_pt.sum() <= 0.01 * pr.visible.sum()
    ok = ~und_pt
    assert np.array_equal(rgb[ok], z["rgb"][ok].astype(np.float64))
    assert (~pr.visible & ok).sum() > 1000                                   # rows that keep what they held
    _depth_agrees(z["depth"][0], depth[0], und_px)
    counts = np.bincount(pr.v[pr.visible] * sc.W + pr.u[pr.visible])
    assert (counts > 1).sum() > 100                                          # the minimum is exercised


@pytest.mark.parametrize("tag", ["all", "colorized"])
def test_method_matches_the_reference(tag):
    z = _load("cams")
    sc = LR.scene(int(z["n"]), int(z["H"]), int(z["W"]), int(z["seed"]), ncam=2)
    ds = LR.Dataset(sc, cams=[sc.names[0], "none", sc.names[1]])
    r = LR.project_to_cams(ds, tag == "colorized")
    seen = LR.project_to_cams(ds, True).keep
    assert seen.sum() > 2000 and r.undecided.sum() <= 0.01 * seen.sum()
    ok = ~r.undecided
    full = z["all.cloud"].astype(np.float64)
    seen32 = full[:, 3] != -1.0
    assert np.array_equal(seen32[ok], seen[ok])
    assert np.array_equal(full[ok], r.cloud[ok])                              # colours, overwrite order and the -1 rows
    assert (full[~seen32, 3:] == -1.0).all() and (~seen32).sum() > 500
    first = LR.project(sc.cloud, sc.T["cam0"], sc.K["cam0"], sc.H, sc.W, sc.min_range).visible
    second = LR.project(sc.cloud, sc.T["cam1"], sc.K["cam1"], sc.H, sc.W, sc.min_range).visible
    assert (first & second & ok).sum() > 500 and (first & ~second & ok).sum() > 100
    if tag == "colorized":                                                    # stable compaction of every companion
        assert np.array_equal(z["colorized.cloud"], z["all.cloud"][seen32])
        for key, t in (("ts", ds.cur_point_ts_torch), ("normals", ds.cur_point_normals),
                       ("sem", ds.cur_sem_labels_torch), ("sem_full", ds.cur_sem_labels_full)):
            assert np.array_equal(z[f"colorized.{key}"], t.numpy()[seen32]), key
    for name, cam in r.cams.items():
        for k, (lvl, und) in enumerate(zip(cam.levels, _pyramid_mask(cam.undecided))):
            got = z[f"{tag}.{name}.depth{k}"]
            assert got.shape == lvl.shape == (1, sc.H >> k, sc.W >> k)
            _depth_agrees(got[0], lvl[0], und)


def test_voxel_downsample_matches_the_reference():
    z = _load("cams")
    sc = LR.scene(int(z["n"]), int(z["H"]), int(z["W"]), int(z["seed"]), ncam=2)
    ds = LR.Dataset(sc)
    assert ds.train_voxel_m == float(z["voxel.size"])
    rows = LR.voxel_downsample_rows(ds)
    assert 0.5 * sc.cloud.shape[0] < len(rows) < 0.9 * sc.cloud.shape[0]
    assert np.array_equal(z["voxel.cloud"], sc.cloud[rows])
    for key, t in (("ts", ds.cur_point_ts_torch), ("sem", ds.cur_sem_labels_torch), ("sem_full", ds.cur_sem_labels_full)):
        assert np.array_equal(z[f"voxel.{key}"], t.numpy()[rows]), key


@pytest.mark.parametrize("shape", ["33x70", "9x15"])
def test_depth_pyramid_matches_the_reference(shape):
    z = _load("depth")
    levels = LR.depth_pyramid(z[f"{shape}.depth0"])
    for k in range(4):
        assert np.array_equal(levels[k], z[f"{shape}.depth{k}"].astype(np.float64)), k
    assert levels[3].shape[1] >= 1 and levels[3].size > 0


# ================================================================ rotation interpolation against scipy
def _pose(theta, seed, t=(0.7, -0.2, 0.05)):
    g = np.random.default_rng(seed)
    a = g.normal(size=3)
    a /= np.linalg.norm(a)
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec(theta * a).as_matrix()
    T[:3, 3] = t
    return T, a


@pytest.mark.parametrize("theta", THETAS)
def test_rotation_interpolation_is_scipys(theta):
    T, a = _pose(theta, 1)
    s = np.linspace(-0.5, 0.5, 11)
    want = Rotation.from_rotvec(s[:, None] * theta * a).as_matrix()
    assert np.abs(LR.rotations(T[:3, :3], s) - want).max() <= 1e-12
    if theta == 0.0:
        assert np.array_equal(LR.rotations(T[:3, :3], s), np.broadcast_to(np.eye(3), (11, 3, 3)))
    for si in (-0.5, 0.0, 0.3, 0.5):
        P = LR.slerp_pose(T, si + 0.5, 0.5)
        assert np.abs(P[:3, :3] - Rotation.from_rotvec(si * theta * a).as_matrix()).max() <= 1e-12
        assert np.abs(P[:3, 3] - si * T[:3, 3]).max() <= 1e-12 and np.array_equal(P[3], [0, 0, 0, 1])


@pytest.mark.parametrize("theta", THETAS)
@pytest.mark.parametrize("ref", [0.0, 0.5, 1.0])
def test_deskew_is_scipys(theta, ref):
    T, a = _pose(theta, 2)
    g = np.random.default_rng(3)
    p = g.normal(0, 10.0, (257, 3)).astype(np.float32)
    ts = g.uniform(100.0, 100.1, 257).astype(np.float32)
    s = (ts.astype(np.float64) - ts.min()) / (np.float64(ts.max()) - ts.min()) - ref
    want = Rotation.from_rotvec(s[:, None] * theta * a).apply(p.astype(np.float64)) + s[:, None] * T[:3, 3]
    assert np.abs(LR.deskew(p, ts, T, ref) - want).max() <= 1e-12 * 10.0
    assert LR.deskew(p, None, T, ref).dtype == np.float64 and np.array_equal(LR.deskew(p, None, T, ref), p)


@pytest.mark.parametrize("diffs", [None, (0.125, -0.25)])
def test_multi_lidar_deskew_is_the_stated_formula(diffs):
    T, _ = _pose(0.3, 4)
    rig = [_pose(1.1, 5, (0.5, 0.2, -0.1))[0], _pose(2.0, 6, (-1.0, 0.0, 0.3))[0]]
    g = np.random.default_rng(7)
    p = g.normal(0, 10.0, (300, 3)).astype(np.float32)
    ts = g.random(300).astype(np.float32)
    idx = g.integers(0, 4, 300)                                               # 3 names no LiDAR of the rig
    got = LR.deskew(p, ts, T, 0.5, idx, rig, diffs)
    s = (ts.astype(np.float64) - ts.min()) / (np.float64(ts.max()) - ts.min()) - 0.5
    p64 = p.astype(np.float64)
    want = p64.copy()
    for k in range(3):
        rows = idx == k
        M = np.eye(4) if k == 0 else rig[k - 1]
        Pk = M @ T @ np.linalg.inv(M)
        sk = s[rows] + (diffs[k - 1] if (k and diffs) else 0.0)
        rv = Rotation.from_matrix(Pk[:3, :3]).as_rotvec()
        q = p64[rows] @ M[:3, :3].T + M[:3, 3]
        q = Rotation.from_rotvec(sk[:, None] * rv).apply(q) + sk[:, None] * Pk[:3, 3]
        Mi = np.linalg.inv(M)
        want[rows] = q @ Mi[:3, :3].T + Mi[:3, 3]
    assert np.abs(got - want).max() <= 1e-11
    assert np.array_equal(got[idx == 3], p64[idx == 3]) and (idx == 3).sum() > 30
    assert np.array_equal(LR.deskew(p, ts, T, 0.5, idx, [], diffs), p64)       # the empty list changes nothing


# ================================================================ install / uninstall
def _stand_in_module():
    mod = types.ModuleType("stand_in_slam_dataset")
    for name in ("deskewing", "slerp_pose", "project_points_to_cam_torch", "intrinsic_correct"):
        setattr(mod, name, (lambda nm: lambda *a, **k: nm)(name))

    class SLAMDataset:
        def filter_and_correct(self):
            return "filter_and_correct"

        def voxel_downsample_points_for_mapping(self):
            return "voxel"

        def project_pointcloud_to_cams(self, use_only_colorized_points=True, tran_in_frame=None):
            return "project"

        def preprocess_source_points(self):
            return "preprocess"

    class CamImage:
        device = "cpu"

        def set_depth_img(self, depth):
            return "set_depth_img"

    mod.SLAMDataset = SLAMDataset
    return mod, CamImage


def test_install_rebinds_and_uninstall_restores():
    mod, cam = _stand_in_module()
    before = {n: getattr(mod, n) for n in ("deskewing", "slerp_pose", "project_points_to_cam_torch")}
    methods = {n: mod.SLAMDataset.__dict__[n] for n in ("filter_and_correct", "voxel_downsample_points_for_mapping",
                                                       "project_pointcloud_to_cams", "preprocess_source_points")}
    depth0 = cam.__dict__["set_depth_img"]
    lidar_ops.install(mod, cam)
    lidar_ops.install(mod, cam)                                               # twice changes nothing
    try:
        assert mod.deskewing is lidar_ops.deskew and mod.slerp_pose is lidar_ops.slerp_pose
        assert mod.project_points_to_cam_torch is lidar_ops.project_points_to_cam
        assert mod.SLAMDataset.filter_and_correct is lidar_ops.filter_and_correct
        assert mod.SLAMDataset.voxel_downsample_points_for_mapping is lidar_ops.voxel_downsample_points_for_mapping
        assert mod.SLAMDataset.project_pointcloud_to_cams is lidar_ops.project_to_cams
        assert mod.SLAMDataset.preprocess_source_points is methods["preprocess_source_points"]
        assert cam.set_depth_img is lidar_ops.set_depth_img
        for n, f in before.items():
            assert getattr(mod, f"_pings_{n}_original") is f
        for n in ("filter_and_correct", "voxel_downsample_points_for_mapping", "project_pointcloud_to_cams"):
            assert getattr(mod.SLAMDataset, f"_pings_{n}_original") is methods[n]
        assert cam._pings_set_depth_img_original is depth0
        # inputs the kernels do not take go to the kept originals: CPU tensors here
        pts, ts = torch.zeros(4, 3), torch.rand(4)
        assert mod.deskewing(pts, ts, torch.eye(4)) == "deskewing"
        assert mod.slerp_pose(torch.eye(4), 0.7, 0.5) == "slerp_pose"
        assert cam().set_depth_img(torch.zeros(1, 8, 8)) == "set_depth_img"
    finally:
        lidar_ops.uninstall(mod, cam)
    for n, f in before.items():
        assert getattr(mod, n) is f and not hasattr(mod, f"_pings_{n}_original")
    for n, f in methods.items():
        assert mod.SLAMDataset.__dict__[n] is f and not hasattr(mod.SLAMDataset, f"_pings_{n}_original")
    assert cam.__dict__["set_depth_img"] is depth0 and not hasattr(cam, "_pings_set_depth_img_original")
    with pytest.raises(RuntimeError, match="none was kept"):
        lidar_ops.deskew(torch.zeros(4, 3), torch.rand(4), torch.eye(4))


def test_deskew_returns_its_input_before_any_launch():
    pts, ts = torch.arange(12.0).reshape(4, 3), torch.rand(4)
    keep = pts.clone()
    assert lidar_ops.deskew(pts, None, torch.eye(4)) is pts
    out = lidar_ops.deskew(pts, ts, torch.eye(4), 0.5, torch.tensor([0, 1, 0, 2]), [], None)
    assert out is pts and torch.equal(pts, keep)                              # the empty list: main LiDAR included
