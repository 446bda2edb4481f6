"""Golden vectors of the LiDAR frame front-end from the reference's own code (CPU, float32):

  lidar_crop.npz      `crop_frame` (dataset/slam_dataset.py:1626-1645) on two random scans, 2-D and 3-D distance
  lidar_project.npz   `project_points_to_cam_torch` (utils/tools.py:1242-1327), one camera, 4,096 points at 64 x 48
  lidar_cams.npz      `SLAMDataset.project_pointcloud_to_cams` (:803-856) unbound on a stand-in (tests/lidar_ref.py) with
                      three cameras, the middle one `None`, `cur_sensor_ts = None`, with and without compaction, and
                      `voxel_downsample_points_for_mapping` (:776-784) on the same stand-in
  lidar_depth.npz     `CamImage.set_depth_img` (gaussian_splatting/utils/cameras.py:233-243) at 33 x 70 and 9 x 15

`deskewing` and `slerp_pose` have no fixture: they call `roma`, which the import shim mocks.  The scenes are those of
tests/lidar_ref.py; the share of undecided points and rows is printed, and asserted in tests/test_lidar_ref.py.

    python tools/make_lidar_golden.py            (needs the reference tree; CPU only)
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import lidar_ref as LR  # noqa: E402
from oracle import ref_shim  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
CROP = dict(min_z=-3.0, max_z=6.0, min_range=2.75, max_range=40.0)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def main():
    ref_shim.load()
    import dataset.slam_dataset as SD  # type: ignore
    from gaussian_splatting.utils.cameras import CamImage  # type: ignore
    from utils.tools import project_points_to_cam_torch  # type: ignore

    # ---- crop
    out = {k: np.float64(v) for k, v in CROP.items()}
    for name, xy, seed in (("xy", True, 1), ("xyz", False, 2)):
        p = LR.crop_cloud(3000, seed)
        mask = SD.crop_frame(torch.from_numpy(p), CROP["min_z"], CROP["max_z"], CROP["min_range"], CROP["max_range"], xy)
        _, near = LR.crop(p, on_xy_plane=xy, **CROP)
        print(f"crop {name}: kept {int(mask.sum())}/{len(p)}, undecided {near.mean():.5f}")
        out.update({f"{name}.points": p, f"{name}.mask": _np(mask), f"{name}.on_xy_plane": np.bool_(xy)})
    np.savez_compressed(GOLDEN / "lidar_crop.npz", **out)

    # ---- one camera
    sc = LR.scene(4096, 48, 64, seed=3)
    nm = sc.names[0]
    g = torch.Generator().manual_seed(0)
    rgb_in = torch.rand(4096, 4, generator=g)
    rgb, depth = project_points_to_cam_torch(torch.from_numpy(sc.cloud), rgb_in.clone(), torch.from_numpy(sc.img[nm]),
                                             torch.tensor(sc.T[nm], dtype=torch.float32),
                                             torch.tensor(sc.K[nm], dtype=torch.float32), min_depth=sc.min_range)
    pr = LR.project(sc.cloud, sc.T[nm], sc.K[nm], sc.H, sc.W, sc.min_range)
    print(f"project: visible {int(pr.visible.sum())}/4096, undecided/visible {pr.undecided.sum() / pr.visible.sum():.4f}")
    np.savez_compressed(GOLDEN / "lidar_project.npz", seed=np.int64(3), n=np.int64(4096), H=np.int64(48), W=np.int64(64),
                        rgb_in=_np(rgb_in), rgb=_np(rgb), depth=_np(depth))

    # ---- the method, three cameras with the middle one None; the down-sampler
    sc = LR.scene(4096, 48, 64, seed=5, ncam=2)
    cams = [sc.names[0], "none", sc.names[1]]
    out = dict(seed=np.int64(5), n=np.int64(4096), H=np.int64(48), W=np.int64(64))
    for tag, only in (("all", False), ("colorized", True)):
        ds = LR.Dataset(sc, cams=cams, set_depth_img=CamImage.set_depth_img)
        SD.SLAMDataset.project_pointcloud_to_cams(ds, only, None)
        out[f"{tag}.cloud"] = _np(ds.cur_point_cloud_torch)
        if only:                                   # without compaction the companions are not touched
            out.update({f"{tag}.ts": _np(ds.cur_point_ts_torch), f"{tag}.normals": _np(ds.cur_point_normals),
                        f"{tag}.sem": _np(ds.cur_sem_labels_torch), f"{tag}.sem_full": _np(ds.cur_sem_labels_full)})
        else:
            assert ds.cur_point_ts_torch.shape[0] == 4096 and ds.cur_point_normals.shape[0] == 4096
        for name, cam in ds.cur_cam_img.items():
            if cam is not None:
                assert cam.depth_on
                for k in range(4):
                    out[f"{tag}.{name}.depth{k}"] = _np(cam.depth_image_list[k])
    r = LR.project_to_cams(LR.Dataset(sc, cams=cams), True)
    print(f"cams: kept {int(r.keep.sum())}/4096, undecided/visible {r.undecided.sum() / max(r.keep.sum(), 1):.4f}")
    ds = LR.Dataset(sc, cams=cams)
    SD.SLAMDataset.voxel_downsample_points_for_mapping(ds)
    out.update({"voxel.cloud": _np(ds.cur_point_cloud_torch), "voxel.ts": _np(ds.cur_point_ts_torch),
                "voxel.sem": _np(ds.cur_sem_labels_torch), "voxel.sem_full": _np(ds.cur_sem_labels_full),
                "voxel.size": np.float64(ds.train_voxel_m)})
    print(f"voxel: kept {ds.cur_point_cloud_torch.shape[0]}/4096")
    np.savez_compressed(GOLDEN / "lidar_cams.npz", **out)

    # ---- set_depth_img
    out = {}
    for H, W in ((33, 70), (9, 15)):
        d = torch.rand(1, H, W, generator=g) * 50.0
        d[torch.rand(1, H, W, generator=g) < 0.3] = 0.0
        cam = LR.Cam(np.zeros((3, H, W), np.float32), set_depth_img=CamImage.set_depth_img)
        cam.set_depth_img(d)
        assert cam.depth_on
        for k in range(4):
            out[f"{H}x{W}.depth{k}"] = _np(cam.depth_image_list[k])
    np.savez_compressed(GOLDEN / "lidar_depth.npz", **out)
    for f in ("lidar_crop", "lidar_project", "lidar_cams", "lidar_depth"):
        print(f, (GOLDEN / f"{f}.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
