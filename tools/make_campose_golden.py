"""Golden vectors of the camera pose arithmetic from the reference's own code: `CamImage.set_pose`
(gaussian_splatting/utils/cameras.py:207-219) and `update_pose` (utils/campose_utils.py:79-98) on the CPU.

Three base poses (translation scales 1, 100 and 1000 m, the off-centre intrinsics of G6).  For every base pose and every
tau scale below, a chain of five updates; per step: tau, the five camera tensors and the returned flag.  The scales sit
on either side of the two thresholds of the code and never within 1 % of them, so a norm taken in fp32 and one taken in
fp64 decide alike:
    zero       tau = 0 exactly (pose optimisation off: returns True, touches nothing)
    theta_lo   |theta| = 0.5e-5   (series branch of SO3_exp / V),  |rho| = 1e-3
    theta_hi   |theta| = 2e-5     (closed form),                   |rho| = 1e-3
    tau_lo     |tau| = 0.5e-4     (converged)
    tau_hi     |tau| = 2e-4       (not converged)
    mid        |tau| = 1e-2
    large      |tau| = 0.4
    pi         |theta| = 3.0,  |rho| = 0.4
Writes tests/golden/campose_steps.npz (arrays only); tests/test_camera_ops.py reads only the file.

    python tools/make_campose_golden.py            (needs the reference tree; CPU only)
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import ref_shim  # noqa: E402

W, H, FX, FY, CX, CY = 200, 120, 180.0, 175.0, 87.3, 71.9      # G6 "offcentre" (oracle/make_golden.py)
Z_MIN, Z_MAX = 0.05, 80.0
T_SCALES = (1.0, 100.0, 1000.0)
SCALES = ("zero", "theta_lo", "theta_hi", "tau_lo", "tau_hi", "mid", "large", "pi")
STEPS = 5
THRESHOLD = 1e-4


def _unit(n, gen):
    v = torch.randn(n, generator=gen, dtype=torch.float64)
    return v / v.norm()


def draw_tau(scale, gen):
    """fp32 tau = [rho, theta] of the named scale."""
    if scale == "zero":
        return torch.zeros(6)
    split = {"theta_lo": (1e-3, 0.5e-5), "theta_hi": (1e-3, 2e-5), "pi": (0.4, 3.0)}
    if scale in split:
        r, t = split[scale]
        return torch.cat([_unit(3, gen) * r, _unit(3, gen) * t]).float()
    n = {"tau_lo": 0.5e-4, "tau_hi": 2e-4, "mid": 1e-2, "large": 0.4}[scale]
    return (_unit(6, gen) * n).float()


def _np(t):
    return t.detach().cpu().numpy().copy()


def _state(cam):
    return [_np(cam.world_view_transform), _np(cam.full_proj_transform), _np(cam.camera_center), _np(cam.R),
            _np(cam.T)]


def main():
    R = ref_shim.load()
    gen = torch.Generator().manual_seed(707)
    K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1]], dtype=np.float64)
    poses, set_states, proj = [], [], None
    keys = ("world_view_transform", "full_proj_transform", "camera_center", "R", "T")
    steps = {k: [] for k in keys}
    taus, flags = [], []
    for ts in T_SCALES:
        w = torch.randn(3, generator=gen, dtype=torch.float64) * 0.6
        Wm = torch.tensor([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=torch.float64)
        pose = torch.eye(4, dtype=torch.float64)
        pose[:3, :3] = torch.linalg.matrix_exp(Wm)
        pose[:3, 3] = _unit(3, gen) * ts
        poses.append(_np(pose))
        mk = lambda: R.CamImage(3, None, K, z_min=Z_MIN, z_max=Z_MAX, device="cpu", cam_pose=pose, img_width=W,
                                img_height=H)
        cam0 = mk()
        set_states.append(_state(cam0))
        proj = _np(cam0.projection_matrix)
        per_scale = {k: [] for k in keys}
        tau_s, flag_s = [], []
        for scale in SCALES:
            cam = mk()
            chain = {k: [] for k in keys}
            tau_c, flag_c = [], []
            for _ in range(STEPS):
                tau = draw_tau(scale, gen)
                n64 = float(tau.double().norm())
                assert n64 == 0.0 or abs(n64 / THRESHOLD - 1.0) > 0.01, (scale, n64)
                a64 = float(tau[3:].double().norm())
                assert a64 == 0.0 or abs(a64 / 1e-5 - 1.0) > 0.01, (scale, a64)
                cam.cam_trans_delta.data.copy_(tau[:3])
                cam.cam_rot_delta.data.copy_(tau[3:])
                flag = R.update_pose(cam, THRESHOLD)
                assert bool(flag) == (n64 < THRESHOLD), (scale, n64, flag)
                for k, v in zip(keys, _state(cam)):
                    chain[k].append(v)
                tau_c.append(_np(tau))
                flag_c.append(bool(flag))
            for k in keys:
                per_scale[k].append(np.stack(chain[k]))
            tau_s.append(np.stack(tau_c))
            flag_s.append(np.array(flag_c))
        for k in keys:
            steps[k].append(np.stack(per_scale[k]))
        taus.append(np.stack(tau_s))
        flags.append(np.stack(flag_s))
    out = dict(W=np.int64(W), H=np.int64(H), K=K, z_min=np.float64(Z_MIN), z_max=np.float64(Z_MAX),
               threshold=np.float64(THRESHOLD), t_scales=np.array(T_SCALES), scales=np.array(SCALES),
               projection_matrix=proj, pose=np.stack(poses), tau=np.stack(taus), flag=np.stack(flags))
    for i, k in enumerate(keys):
        out["set_" + k] = np.stack([s[i] for s in set_states])       # [base, ...]
        out["step_" + k] = np.stack(steps[k])                        # [base, scale, step, ...]
    path = ROOT / "tests" / "golden" / "campose_steps.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {path.stat().st_size} bytes, tau {out['tau'].shape}, flags true {int(out['flag'].sum())}")


if __name__ == "__main__":
    main()
