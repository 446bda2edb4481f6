"""Golden vectors of the odometry loop's colour branches (`Tracker.tracking` with `color_on` and `photometric_loss_on`
or `consist_wieght_on`, utils/tracker.py:353-605, :692-737) from the reference's own code.

The room, the map settings and the fit of tools/make_tracking_golden.py, plus the colour side: `local_color_features`
and a colour `Decoder` are fitted in the same 400 Adam steps with an L1 term against a smooth texture (sines of the
coordinates, 0.5 +- 0.4).  The scan carries the texture at its world points, multiplied by 0.2 where world y < 2: about
a third of the scan disagrees with the map's colour, so that the colour terms move the first step by much more than
the tests' tolerance (asserted: at least 10 x TOL_T against a geometry-only run on the same inputs).  The termination
margins of the geometric generator are asserted as well.  Writes tests/golden/tracking_colour_{photo,consist}.npz;
the tests read only the files.

    python tools/make_tracking_colour_golden.py            (needs the reference tree; CPU only)
"""
import copy
import inspect
import math
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import make_tracking_golden as G  # noqa: E402
from oracle import ref_shim  # noqa: E402
from oracle.make_golden import _map_state, _np  # noqa: E402

TOL_T = 1e-4            # tests/test_tracking.py
N_SCAN = 3000
PHOTO_WEIGHT = 1.0


def texture(x):
    """Smooth colour field of the room, [n,3] in [0.1, 0.9]."""
    return torch.stack([0.5 + 0.4 * torch.sin(1.3 * x[:, 0]), 0.5 + 0.4 * torch.sin(1.7 * x[:, 1] + 1.0),
                        0.5 + 0.4 * torch.sin(2.1 * x[:, 2] + 2.0)], 1)


def fit_map(R, seed=0):
    """G.fit_map with the colour features and a colour decoder fitted alongside."""
    from utils.loss import sdf_bce_loss  # type: ignore

    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    cfg = R.make_config(**G.MAP_KW)
    cfg.local_map_radius = 50.0
    cfg.sorrounding_map_radius = 50.0
    cfg.color_on = True
    cfg.color_channel = 3
    npm = R.NeuralPoints(cfg)
    npm.travel_dist = torch.tensor([0.0], dtype=torch.float32)
    pts, _ = G.room_surface(40000, gen)
    centre = torch.tensor(G.ROOM) / 2
    npm.update(pts, torch.rand(pts.shape[0], 3, generator=gen), None, centre, torch.eye(3), cur_ts=0)
    npm.reset_local_map(centre, torch.eye(3), cur_ts=0)
    dec = R.Decoder(cfg, cfg.feature_dim, cfg.geo_mlp_hidden_dim, cfg.geo_mlp_level, 1)
    cdec = R.Decoder(cfg, 8, cfg.color_mlp_hidden_dim, cfg.color_mlp_level, 3)
    sigma = cfg.logistic_gaussian_ratio * cfg.sigma_sigmoid_m
    opt = torch.optim.Adam([{"params": [npm.local_geo_features, npm.local_color_features], "lr": 0.02},
                            {"params": list(dec.parameters()) + list(cdec.parameters()), "lr": 0.005}])
    for step in range(400):
        p, nrm = G.room_surface(4096, gen)
        x = p + nrm * (torch.randn(4096, 1, generator=gen) * 0.3)
        label = G.room_sdf(x)
        geo, colf, w, _, _ = npm.query_feature(x, None, accumulate_stability=False, query_color_feature=True)
        s = torch.sum(dec.sdf(geo) * w, dim=1).squeeze(1)
        col = torch.sum(cdec.regress_color(colf) * w, dim=1)
        l_sdf = sdf_bce_loss(s, label, sigma, None, False)
        l_col = (col - texture(p)).abs().mean()
        loss = l_sdf + l_col
        opt.zero_grad()
        loss.backward()
        opt.step()
        if step % 100 == 0 or step == 399:
            print(f"fit step {step}: bce {l_sdf.item():.5f} colour L1 {l_col.item():.5f}")
    npm.assign_local_to_global()
    npm.reset_local_map(centre, torch.eye(3), cur_ts=0)
    return cfg, npm, dec, cdec


def run(R, cfg0, npm, dec, cdec, src, colours, init, **flags):
    import utils.tracker as TR  # type: ignore

    cfg = copy.copy(cfg0)
    for k, v in flags.items():
        setattr(cfg, k, v)
    rec = []

    class Rec(TR.Tracker):
        def registration_step(self, points, *a, **kw):
            out = super().registration_step(points, *a, **kw)
            rec.append((out[0].clone(), int(out[4].shape[0]), float(out[5]), out[6]))
            return out

    trk = Rec(cfg, npm, {"sdf": dec, "semantic": None, "color": cdec})
    trk.silence = True
    T, _, _, valid = trk.tracking(src, init.clone(), source_colors=colours)
    return cfg, T, valid, rec


def check_margins(name, cfg, rec, N):
    """The termination margins of tools/make_tracking_golden.py:run_case."""
    iters, last = len(rec), 1e5
    for i, (dT, cnt, res, _) in enumerate(rec):
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
    assert abs(rec[-1][2] / (cfg.surface_sample_range_m * 60.0) - 1.0) > 0.05, (name, "final-residual rule within 5 %")


def main():
    R = ref_shim.load()
    import utils.tracker as TR  # type: ignore

    cfg0, npm, dec, cdec = fit_map(R)
    cfg0.photometric_loss_weight = PHOTO_WEIGHT
    gen = torch.Generator().manual_seed(len("default"))
    T_gt = G.pose((3.0, -2.0, 25.0), (4.1, 2.9, 1.4))
    world, _ = G.room_surface(N_SCAN, gen)
    Ti = torch.linalg.inv(T_gt)
    src = (world.double() @ Ti[:3, :3].T + Ti[:3, 3]).float()
    colours = texture(world)
    colours = torch.where(world[:, 1:2] < 2.0, 0.2 * colours, colours).float().contiguous()
    print(f"darkened scan points: {(world[:, 1] < 2.0).float().mean().item():.3f}")
    init = G.pose(*G.CASES["default"]["pert"]) @ T_gt
    _, _, _, geo = run(R, cfg0, npm, dec, cdec, src, None, init)
    for name, flags in (("photo", dict(photometric_loss_on=True)), ("consist", dict(consist_wieght_on=True))):
        cfg, T, valid, rec = run(R, cfg0, npm, dec, cdec, src, colours, init, **flags)
        check_margins(name, cfg, rec, src.shape[0])
        assert valid and T is not None, name
        shift = float((rec[0][0][:3, 3] - geo[0][0][:3, 3]).norm())
        assert shift >= 10 * TOL_T, (name, "the colour term moves the first step by less than 10 TOL_T", shift)
        out = _map_state(npm, cfg)
        out.update(nn_k=np.int64(cfg.query_nn_k), weighted_first=np.bool_(cfg.weighted_first),
                   sdf_scale=np.float64(dec.sdf_scale))
        for k_, v_ in dec.state_dict().items():
            out["dec." + k_] = _np(v_)
        for k_, v_ in cdec.state_dict().items():
            out["cdec." + k_] = _np(v_)
        out.update(
            src=_np(src), src_color=_np(colours), init_pose=_np(init), T_gt=_np(T_gt), T=_np(T),
            valid_flag=np.bool_(valid), iterations=np.int64(len(rec)), delta=np.stack([_np(r[0]) for r in rec]),
            count=np.array([r[1] for r in rec], np.int64), residual=np.array([r[2] for r in rec], np.float64),
            photo_residual=np.array([np.nan if r[3] is None else float(r[3]) for r in rec], np.float64),
            geo_first_delta=_np(geo[0][0]), first_step_shift=np.float64(shift),
            sig_tracking=str(inspect.signature(TR.Tracker.tracking)),
            sig_registration_step=str(inspect.signature(TR.Tracker.registration_step)))
        for k in ("reg_min_grad_norm", "reg_max_grad_norm", "reg_GM_dist_m", "reg_GM_grad", "reg_lm_lambda",
                  "reg_iter_n", "reg_term_thre_deg", "reg_term_thre_m", "surface_sample_range_m", "max_sdf_std_ratio",
                  "reg_dist_div_grad_norm", "infer_bs", "track_mask_query_nn_k", "eigenvalue_check", "color_on",
                  "color_channel", "photometric_loss_on", "consist_wieght_on", "photometric_loss_weight"):
            out["cfg." + k] = np.asarray(getattr(cfg, k))
        err = float((T_gt.inverse() @ T)[:3, 3].norm())
        print(f"tracking_colour_{name}: iters {len(rec)} valid {valid} counts {rec[0][1]}..{rec[-1][1]}/{src.shape[0]} "
              f"residual {rec[0][2]:.3f} -> {rec[-1][2]:.3f} cm, photo {rec[0][3]} first-step shift {shift:.2e} m, "
              f"|t err| {err:.4f} m")
        np.savez_compressed(ROOT / "tests" / "golden" / f"tracking_colour_{name}.npz", **out)


if __name__ == "__main__":
    main()
