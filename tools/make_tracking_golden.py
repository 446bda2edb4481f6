"""Golden vectors of the odometry loop (`Tracker.tracking`, utils/tracker.py:43-210) from the reference's own code.

A reference `NeuralPoints` map of an axis-aligned room (surface points of its six faces, one frame through
`NeuralPoints.update`) gets its geometric features and SDF decoder fitted on CPU for a few hundred Adam steps with the
reference's own `query_feature` and BCE loss (utils/loss.py) against the room's analytic SDF, so that tracking runs on
a real distance field.  Then the reference `Tracker(cfg, npm, decoders).tracking(...)` runs with `cfg.device = "cpu"`;
`registration_step` is wrapped to record every iteration's dT, valid count and residual.  Each case asserts a
termination margin: every threshold comparison that decided the run is at least 5 % away from its threshold and no
rotation angle is NaN, so a device run can be required to take the same number of iterations.
Writes tests/golden/tracking_<case>.npz (map state in the layout of tests/test_sdf.py: `_gpu_map` / `_Dec`);
tests/test_tracking.py reads only the files.

    python tools/make_tracking_golden.py            (needs the reference tree; CPU only)
"""
import inspect
import math
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import ref_shim  # noqa: E402
from oracle.make_golden import _map_state, _np  # noqa: E402

ROOM = (8.0, 6.0, 3.0)
MAP_KW = dict(voxel_size_m=0.3, search_alpha=0.8, query_nn_k=6, feature_dim=8, color_feature_dim=8,
              weighted_first=False, buffer_size=100003, main_loss_type="bce", sigma_sigmoid_m=0.08,
              surface_sample_range_m=0.25, geo_mlp_hidden_dim=32)


def room_surface(n, gen):
    """n points on the six faces of the box [0, ROOM], area-weighted, with their inward normals."""
    L = torch.tensor(ROOM)
    areas = torch.tensor([L[1] * L[2], L[1] * L[2], L[0] * L[2], L[0] * L[2], L[0] * L[1], L[0] * L[1]])
    face = torch.multinomial(areas / areas.sum(), n, replacement=True, generator=gen)
    p = torch.rand(n, 3, generator=gen) * L
    nrm = torch.zeros(n, 3)
    for f in range(6):
        ax, hi = f // 2, f % 2
        m = face == f
        p[m, ax] = L[ax] if hi else 0.0
        nrm[m, ax] = -1.0 if hi else 1.0
    return p, nrm


def room_sdf(x):
    L = torch.tensor(ROOM, dtype=x.dtype)
    return torch.minimum(x, L - x).min(dim=1).values


def fit_map(R, seed=0):
    from utils.loss import sdf_bce_loss  # type: ignore

    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    cfg = R.make_config(**MAP_KW)
    cfg.local_map_radius = 50.0
    cfg.sorrounding_map_radius = 50.0
    cfg.color_on = True          # the map layout carries colour features (the tracking cases pass no colours)
    npm = R.NeuralPoints(cfg)
    npm.travel_dist = torch.tensor([0.0], dtype=torch.float32)
    pts, _ = room_surface(40000, gen)
    centre = torch.tensor(ROOM) / 2
    npm.update(pts, torch.rand(pts.shape[0], 3, generator=gen), None, centre, torch.eye(3), cur_ts=0)
    npm.reset_local_map(centre, torch.eye(3), cur_ts=0)
    dec = R.Decoder(cfg, cfg.feature_dim, cfg.geo_mlp_hidden_dim, cfg.geo_mlp_level, 1)
    sigma = cfg.logistic_gaussian_ratio * cfg.sigma_sigmoid_m
    opt = torch.optim.Adam([{"params": [npm.local_geo_features], "lr": 0.02},
                            {"params": dec.parameters(), "lr": 0.005}])
    for step in range(400):
        p, nrm = room_surface(4096, gen)
        x = p + nrm * (torch.randn(4096, 1, generator=gen) * 0.3)
        label = room_sdf(x)
        geo, _, w, _, _ = npm.query_feature(x, None, accumulate_stability=False)
        s = torch.sum(dec.sdf(geo) * w, dim=1).squeeze(1)
        loss = sdf_bce_loss(s, label, sigma, None, False)
        opt.zero_grad()
        loss.backward()
        opt.step()
        if step % 100 == 0 or step == 399:
            print(f"fit step {step}: bce {loss.item():.5f}")
    npm.assign_local_to_global()
    npm.reset_local_map(centre, torch.eye(3), cur_ts=0)
    return cfg, npm, dec


def pose(rot_deg_xyz, t):
    a = [math.radians(v) for v in rot_deg_xyz]
    cx, sx, cy, sy, cz, sz = math.cos(a[0]), math.sin(a[0]), math.cos(a[1]), math.sin(a[1]), math.cos(a[2]), math.sin(a[2])
    Rx = torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=torch.float64)
    Ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=torch.float64)
    Rz = torch.tensor([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], dtype=torch.float64)
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = torch.tensor(t, dtype=torch.float64)
    return T


CASES = {
    # shipped defaults: GM on both, LM 1e-4, no normals; 0.3 m / 2 deg off
    "default": dict(cfg={}, n=3000, pert=((1.2, -0.8, 1.5), (0.2, -0.15, 0.16)), normals=False, shift=0.0),
    # normals on, residual divided by |g|, GM on the residual only, the query in batches (infer_bs < N)
    "normals_div_batched": dict(cfg=dict(reg_dist_div_grad_norm=True, reg_GM_grad=0.0, infer_bs=1024), n=3000,
                                pert=((-1.0, 1.4, -1.2), (-0.18, 0.2, -0.14)), normals=True, shift=0.0),
    # the scan far outside the map: fewer than 10 valid points, valid_flag False, the result is init_pose
    "far": dict(cfg={}, n=2000, pert=((0.5, 0.5, 0.5), (0.1, 0.1, 0.1)), normals=False, shift=60.0),
    # (a fourth case ending on the residual-increase rule was sought: no seed / perturbation tried here ended on it
    # with the 5 % margin, so that rule has no fixture)
}


def run_case(R, cfg0, npm, dec, name, c, seed):
    import copy

    import utils.tracker as TR  # type: ignore

    gen = torch.Generator().manual_seed(seed)
    cfg = copy.copy(cfg0)
    for k, v in c["cfg"].items():
        setattr(cfg, k, v)
    T_gt = pose((3.0, -2.0, 25.0), (4.1, 2.9, 1.4))
    world, nrm_w = room_surface(c["n"], gen)
    world = world + torch.tensor([c["shift"], 0.0, 0.0])
    Ti = torch.linalg.inv(T_gt)
    src = (world.double() @ Ti[:3, :3].T + Ti[:3, 3]).float()
    nrm = (nrm_w.double() @ Ti[:3, :3].T).float() if c["normals"] else None
    init = pose(*c["pert"]) @ T_gt
    rec = []

    class Rec(TR.Tracker):
        def registration_step(self, points, *a, **kw):
            out = super().registration_step(points, *a, **kw)
            rec.append((out[0].clone(), int(out[4].shape[0]), float(out[5])))
            return out

    trk = Rec(cfg, npm, {"sdf": dec, "semantic": None, "color": None})
    trk.silence = True
    T, cov, _, valid = trk.tracking(src, init.clone(), source_normals=nrm)
    iters = len(rec)
    # termination margin
    N = src.shape[0]
    last = 1e5
    for i, (dT, cnt, res) in enumerate(rec):
        inc = (res - last) / last
        assert abs(inc / 1.1 - 1.0) > 0.05, (name, i, "residual-increase rule within 5 %", inc)
        if inc <= 1.1:
            last = res
        if cnt >= 10:
            assert cnt >= 10.5 and abs(cnt / N / 0.05 - 1.0) > 0.05, (name, i, "valid-point rule within 5 %")
        rot = math.degrees(math.acos((float(torch.trace(dT[:3, :3])) - 1) / 2)) if cnt >= 10 else 0.0
        assert not math.isnan(rot), (name, i, "NaN rotation angle")
        tran = float(dT[:3, 3].norm())
        if i < iters - 1 and i != cfg.reg_iter_n - 2 and cnt >= 10:
            r1, r2 = abs(rot) / cfg.reg_term_thre_deg, tran / cfg.reg_term_thre_m
            decided_conv = r1 < 1 and r2 < 1
            assert (max(r1, r2) < 0.95) if decided_conv else (r1 > 1.05 or r2 > 1.05), \
                (name, i, "termination rule within 5 %", r1, r2)
    final = rec[-1][2]
    assert abs(final / (cfg.surface_sample_range_m * 60.0) - 1.0) > 0.05, (name, "final-residual rule within 5 %")
    out = _map_state(npm, cfg)
    out.update(nn_k=np.int64(cfg.query_nn_k), weighted_first=np.bool_(cfg.weighted_first),
               sdf_scale=np.float64(dec.sdf_scale))
    for k_, v_ in dec.state_dict().items():
        out["dec." + k_] = _np(v_)
    out.update(
        src=_np(src), init_pose=_np(init), T_gt=_np(T_gt), T=_np(T if T is not None else init),
        returned_init=np.bool_(T is init or (T is not None and torch.equal(T, init) and not valid)),
        valid_flag=np.bool_(valid), iterations=np.int64(iters),
        delta=np.stack([_np(r[0]) for r in rec]), count=np.array([r[1] for r in rec], np.int64),
        residual=np.array([r[2] for r in rec], np.float64),
        sig_tracking=str(inspect.signature(TR.Tracker.tracking)),
        sig_registration_step=str(inspect.signature(TR.Tracker.registration_step)))
    if nrm is not None:
        out["normals"] = _np(nrm)
    for k in ("reg_min_grad_norm", "reg_max_grad_norm", "reg_GM_dist_m", "reg_GM_grad", "reg_lm_lambda", "reg_iter_n",
              "reg_term_thre_deg", "reg_term_thre_m", "surface_sample_range_m", "max_sdf_std_ratio",
              "reg_dist_div_grad_norm", "infer_bs", "track_mask_query_nn_k", "eigenvalue_check"):
        out["cfg." + k] = np.asarray(getattr(cfg, k))
    err = float((T_gt.inverse() @ T)[:3, 3].norm()) if T is not None else float("nan")
    print(f"tracking_{name}: iters {iters} valid {valid} counts {rec[0][1]}..{rec[-1][1]}/{N} "
          f"residual {rec[0][2]:.3f} -> {rec[-1][2]:.3f} cm, |t err| {err:.4f} m")
    return out


def main(argv):
    R = ref_shim.load()
    cfg, npm, dec = fit_map(R)
    out_dir = ROOT / "tests" / "golden"
    for name, c in CASES.items():
        if argv and name not in argv:
            continue
        try:
            z = run_case(R, cfg, npm, dec, name, c, seed=c.get("seed", len(name)))
        except AssertionError as e:
            print(f"tracking_{name}: skipped ({e})")
            continue
        np.savez_compressed(out_dir / f"tracking_{name}.npz", **z)


if __name__ == "__main__":
    main(sys.argv[1:])
