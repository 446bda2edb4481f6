"""Golden vectors of the camera frame front-end from the reference's own code (CPU, float32):

  camfront_cam.npz    `CamImage.__init__` (gaussian_splatting/utils/cameras.py:23-186) at 33 x 70 and 9 x 15 with a depth
                      image, a sky mask and a normal image, from a permuted uint8-derived float image (the view the
                      reference's loaders pass), at `img_down_rate` 0 and 1: every level of the four lists, the three
                      flags and `cur_best_level`.  The inputs are `camfront_ref.example(H, W, seed)`.
  camfront_mono_frame.npz   `Mapper.process_frame` (utils/mapper.py:170-526) unbound on the stand-ins of
                      tools/make_frame_pool_golden.py with a mono-depth cloud of 300 rows, `mono_depth_for_high_z` True
                      and False and one cloud the mask keeps nothing of; the tool asserts that no mono point lies within
                      1e-5 (relative) of the quantile threshold.

The mono-depth block of `read_frame_with_loader` needs Open3D and has no fixture: `np.polyfit` and the restatement of
tests/camfront_ref.py stand for it.

    python tools/make_camfront_golden.py            (needs the reference tree; CPU only)
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

import camfront_ref as CR  # noqa: E402
from oracle import ref_shim  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
SIZES = ((33, 70, 11), (9, 15, 12))                    # H, W, seed
K_MAT = np.array([[40.0, 0.0, 34.5], [0.0, 40.0, 16.0], [0.0, 0.0, 1.0]])


def main():
    CamImage = ref_shim.load().CamImage
    out = {"sizes": np.array(SIZES, np.int64), "K": K_MAT}
    for H, W, seed in SIZES:
        u8, depth, sky, normal = CR.example(H, W, seed)
        rgb = (torch.from_numpy(u8).float() / 255.0).permute(2, 0, 1)          # a permuted HWC view, values in [0, 1]
        assert not rgb.is_contiguous()
        for rate in (0, 1):
            cam = CamImage(7, rgb, K_MAT, cam_id="cam0", img_down_rate=rate, depth_image=torch.from_numpy(depth),
                           normal_img=torch.from_numpy(normal), sky_mask=torch.from_numpy(sky), device="cpu",
                           cam_pose=torch.eye(4, dtype=torch.float64))
            tag = f"{H}x{W}.r{rate}"
            out[f"{tag}.flags"] = np.array([cam.depth_on, cam.sky_mask_on, cam.mono_normal_on], np.bool_)
            out[f"{tag}.cur_best_level"] = np.int64(cam.cur_best_level)
            for name, ls in (("rgb", cam.rgb_image_list), ("depth", cam.depth_image_list),
                             ("sky", cam.sky_mask_list), ("normal", cam.normal_img_list)):
                out[f"{tag}.{name}.present"] = np.array([lv is not None for lv in ls], np.bool_)
                for k, lv in enumerate(ls):
                    if lv is not None:
                        out[f"{tag}.{name}.{k}"] = np.ascontiguousarray(lv.detach().numpy())
            print(tag, "cur_best_level", cam.cur_best_level, "levels", [None if lv is None else tuple(lv.shape)
                                                                        for lv in cam.rgb_image_list])
    np.savez_compressed(GOLDEN / "camfront_cam.npz", **out)
    print("wrote", GOLDEN / "camfront_cam.npz", (GOLDEN / "camfront_cam.npz").stat().st_size, "bytes")
    mono_process_frame()


def mono_process_frame():
    """`Mapper.process_frame` unbound on the stand-ins of tools/make_frame_pool_golden.py, frame 0 of the sequence
    `rgb_labels`, with a mono-depth cloud of 300 rows: every input, what the sampler returned, the arguments of both
    `update` calls, the caller's cloud afterwards and every pool tensor."""
    from types import SimpleNamespace as NS

    import frame_pool_ref as FR
    from make_pool_golden import put, reference

    R, _, Mapper = reference()
    seq, seed, rec = FR.SEQUENCES["rgb_labels"], 1, {}
    for tag, (high_z, extent) in CR.MONO_CASES.items():
        cfg = R.make_config(**vars(FR.frame_cfg(seq, **CR.MONO_CFG)))
        m = FR.mapper_state(cfg, seed)
        m.neural_points = CR.MonoMapRecorder()
        m.dataset.loader = NS(mono_depth_for_high_z=high_z)
        pc, label, normal, pose, _ = FR.frame_inputs(seq, 0, seed)
        mono = torch.from_numpy(CR.mono_points(300, seed, extent, seq["color"]))
        for k, t in zip(("pc", "label", "normal", "pose", "mono"), (pc, label, normal, pose, mono.clone())):
            put(rec, f"{tag}_{k}", t)                                        # a copy: the method moves `mono` in place
        Mapper.process_frame(m, pc.clone(), label, normal, pose.clone(), 0, False, mono, None)
        put(rec, f"{tag}_mono_after", mono)                                  # the xyz columns moved in place
        ins, outs = m.sampler.calls[-1]
        for k, t in zip(("points", "normal", "sem", "color"), ins):
            put(rec, f"{tag}_in_{k}", None if t is None else t.contiguous())
        for k, t in zip(("coord", "sdf_label", "normal", "sem", "color", "weight"), outs):
            put(rec, f"{tag}_s_{k}", t)
        ups = m.neural_points.updates
        assert len(ups) == (1 if tag == "none" else 2) and ups[0][6] is False and m.neural_points.memory == 1
        put(rec, f"{tag}_u_points", ups[0][0].contiguous())
        put(rec, f"{tag}_u_colors", ups[0][1].contiguous())
        q = torch.quantile(ups[0][0][:, 2], 0.98 if high_z else 0.2) + cfg.voxel_size_m
        margin = ((mono[:, 2] - q).abs() / q.abs()).min().item()
        assert margin > 1e-5, (tag, margin)                                  # no mono point at the threshold
        if len(ups) == 2:
            pts, col, nrm, origin, orientation, fid, reliable = ups[1]
            assert reliable is True and nrm is None and fid == 0 and torch.equal(origin, pose[:3, 3])
            kept = int(((mono[:, 2] > q) if high_z else (mono[:, 2] < q)).sum())
            assert 5 < pts.shape[0] < kept < 250                             # the down-sampling merges rows
            put(rec, f"{tag}_m_points", pts.contiguous())
            put(rec, f"{tag}_m_colors", col.contiguous())
        for k in FR.POOLS:
            put(rec, f"{tag}_o_{k}", getattr(m, k))
        print(tag, "threshold", float(q), "margin", margin, "mono rows", None if len(ups) < 2 else ups[1][0].shape[0])
    np.savez_compressed(GOLDEN / "camfront_mono_frame.npz", **rec)
    print("wrote", GOLDEN / "camfront_mono_frame.npz", (GOLDEN / "camfront_mono_frame.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
