"""Time the odometry loop: `pings_amd.tracker_ops.tracking` (pose on the device, one host read per iteration) against
the loop as it stood before it, the restatement tests/tracking_ref.py driven by the HIP drop-ins that `install()`
binds (`query_source_points`, `implicit_reg`: boolean compaction, `.item()` and the host-side convergence tests of the
reference between them), on two maps: bench.py's 1M-point synthetic map (a random decoder, |grad| ~ 0.003: the |grad|
window is opened to (0, 20) and the run ends wherever the loop's rules end it) and the fitted room of
tests/golden/tracking_default.npz (a real distance field; the scan is sampled from the room's faces).

Thresholds are set so that every call runs all `reg_iter_n` = 50 iterations where the field allows it (no
convergence before `i == iter_n - 2`).  The two loops alternate in the same process
(`--rounds`).  Per loop and size: ms per call (median), ms per iteration, iterations run, host reads per iteration
(`_lib.sync_counts` for the package's polled reads, plus torch's sync-debug warnings), and the largest difference
between the two final poses.  Launch counts per iteration come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/tracking_time.py --rounds 1` run.

    python tools/tracking_time.py [--sizes 20000 131072] [--rounds 3] [--out profiles/tracking/tracking_time.json]

`--colour` times the photometric configuration (color_on, photometric_loss_on, three channels) on the fitted room of
tests/golden/tracking_colour_photo.npz instead: the device loop of install(..., loop=True, colour=True), the loop as it
stood before it (the restatement tests/tracking_colour_ref.py on `query_source_points` with the fused colour kernel
switched off, i.e. HIP `query_feature`, the colour decoder in torch and one autograd pass per channel, then torch for
the two systems) and the geometry-only device loop beside them, alternating in one process; it writes
profiles/tracking/tracking_colour_time.json.  `--loops device` runs the colour device loop alone, for the
`rocprofv3 --kernel-trace` run that counts its launches.
"""
import argparse
import json
import statistics
import sys
import time
import warnings
from pathlib import Path
from types import SimpleNamespace as NS

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import bench  # noqa: E402
import tracking_ref as ref  # noqa: E402
from pings_amd import _lib, tracker_ops as TO  # noqa: E402


def make_cfg(bs, min_grad):
    return NS(color_on=False, photometric_loss_on=False, consist_wieght_on=False, weighted_first=False,
              color_channel=3, query_nn_k=6, reg_min_grad_norm=min_grad, reg_max_grad_norm=20.0, reg_GM_dist_m=0.3,
              reg_GM_grad=0.1, reg_lm_lambda=1e-4, reg_iter_n=50, reg_term_thre_deg=0.0, reg_term_thre_m=0.0,
              surface_sample_range_m=0.25, max_sdf_std_ratio=100.0, reg_dist_div_grad_norm=False, infer_bs=bs,
              track_mask_query_nn_k=4, eigenvalue_check=True)


def run_device(trk, src, init, colours=None):
    _lib.sync_counts(reset=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            t0 = time.perf_counter()
            T, _, _, valid = TO.tracking(trk, src, init.clone(), source_colors=colours)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            torch.cuda.set_sync_debug_mode(0)
    iters = int(TO.last_trace.shape[0])
    return dt, iters, T, valid, sum(_lib.sync_counts(reset=True).values()), len(w)


def run_before(trk, cfg, src, init):
    from test_tracking import _hip_query, _hip_solve

    _lib.sync_counts(reset=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            t0 = time.perf_counter()
            T, valid, trace = ref.tracking(_hip_query(trk, cfg), _hip_solve, cfg, src, init.clone())
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            torch.cuda.set_sync_debug_mode(0)
    return dt, len(trace), T, valid, sum(_lib.sync_counts(reset=True).values()), len(w)


def run_before_colour(trk, cfg, src, init, colours):
    """The colour loop before the fused kernels: the restatement on query_source_points' composed colour branch."""
    import tracking_colour_ref as cref
    from pings_amd import neural_points as hnp
    from test_tracking import _hip_solve

    def query(points):
        s, g, col, jac, _, m, _, std = TO.query_source_points(trk, points, int(cfg.infer_bs), True, True, True, True,
                                                              query_locally=True,
                                                              mask_min_nn_count=int(cfg.track_mask_query_nn_k))
        return s, g, m, std, col, jac

    supported = hnp.colour_fused_supported
    hnp.colour_fused_supported = lambda npm, dec: False
    _lib.sync_counts(reset=True)
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                t0 = time.perf_counter()
                T, valid, trace, _ = cref.tracking(query, _hip_solve, cfg, src, init.clone(), colours)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            finally:
                torch.cuda.set_sync_debug_mode(0)
    finally:
        hnp.colour_fused_supported = supported
    return dt, len(trace), T, valid, sum(_lib.sync_counts(reset=True).values()), len(w)


def texture(x):
    """The colour field the fixture's map was fitted to (tools/make_tracking_colour_golden.py)."""
    return torch.stack([0.5 + 0.4 * torch.sin(1.3 * x[:, 0]), 0.5 + 0.4 * torch.sin(1.7 * x[:, 1] + 1.0),
                        0.5 + 0.4 * torch.sin(2.1 * x[:, 2] + 2.0)], 1)


def _summary(runs):
    ms = statistics.median(r[0] for r in runs) * 1e3
    it = runs[-1][1]
    return {"ms_per_call": round(ms, 3), "iterations": it, "ms_per_iteration": round(ms / max(it, 1), 4),
            "package_host_reads_per_iteration": round(runs[-1][4] / max(it, 1), 3),
            "torch_sync_warnings_per_iteration": round(runs[-1][5] / max(it, 1), 3), "valid_flag": bool(runs[-1][3])}


def main_colour(a):
    import types

    from pings_amd import neural_points as hnp
    from test_tracking import _room
    from test_tracking_colour import _fix, _tracker

    dev = torch.device("cuda", 0)
    room = _fix("photo")
    module = NS(Tracker=type("Tracker", (), {"tracking": None, "registration_step": None}), implicit_reg=None)
    result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "mode": "photometric, 3 channels",
              "sizes": []}
    for n in a.sizes:
        cfg = make_cfg(max(n, 4096), 0.4)
        cfg.color_on, cfg.photometric_loss_on, cfg.photometric_loss_weight = True, True, 1.0
        geo_cfg = make_cfg(max(n, 4096), 0.4)
        trk, geo = _tracker(room, cfg), _tracker(room, geo_cfg)
        # the composed colour branch of the "before" loop calls the map's query_feature: the HIP one, as install binds it
        trk.neural_points.query_feature = types.MethodType(hnp.query_feature, trk.neural_points)
        w, _ = _room(n, seed=7)
        Ti = torch.linalg.inv(torch.as_tensor(room["T_gt"]))
        src = (w.double() @ Ti[:3, :3].T + Ti[:3, 3]).float().to(dev)
        colours = torch.where(w[:, 1:2] < 2.0, 0.2 * texture(w), texture(w)).float().to(dev)
        init = torch.as_tensor(room["init_pose"]).to(dev)
        TO.install(module, loop=True, colour=True)
        try:
            loops = {"device_colour": lambda: run_device(trk, src, init, colours)}
            if a.loops == "all":
                loops["before_colour"] = lambda: run_before_colour(trk, cfg, src, init, colours)
                loops["device_geometry"] = lambda: run_device(geo, src, init)
            for f in loops.values():       # warm-up (allocator, first-use reads)
                f()
            rec = {k: [] for k in loops}
            for _ in range(a.rounds):
                for k, f in loops.items():
                    rec[k].append(f())
        finally:
            TO.install(module, loop=True)
            TO._ORIG.clear()
        row = {"map": "room", "source_points": n}
        for k, runs in rec.items():
            row[k] = _summary(runs)
        if a.loops == "all":
            D = (rec["device_colour"][-1][2].double() - rec["before_colour"][-1][2].double()).abs()
            row["max_pose_diff"] = {"rotation": float(D[:3, :3].max()), "translation_m": float(D[:3, 3].max())}
        print(json.dumps(row))
        result["sizes"].append(row)
    if a.loops == "all":
        out = Path(a.out if a.out else ROOT / "profiles" / "tracking" / "tracking_colour_time.json")
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(result, indent=1) + "\n")
        print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[20000, 131072])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--colour", action="store_true", help="the photometric configuration on the fitted room")
    ap.add_argument("--loops", choices=("all", "device"), default="all", help="--colour: which loops run")
    a = ap.parse_args()
    if a.colour:
        return main_colour(a)
    if a.out is None:
        a.out = str(ROOT / "profiles" / "tracking" / "tracking_time.json")
    from test_tracking import _fix, _room, _tracker

    dev = torch.device("cuda", 0)
    npm, dec = bench.sdf_synth_map(1_000_000, dev)
    room = _fix("default")
    result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "sizes": []}
    for map_name, n in [(m, n) for m in ("synthetic_1M", "room") for n in a.sizes]:
        cfg = make_cfg(max(n, 4096), 0.0 if map_name == "synthetic_1M" else 0.4)
        if map_name == "synthetic_1M":
            trk = NS(config=cfg, neural_points=npm, sdf_mlp=dec, silence=True, device=dev)
            src = bench.sdf_queries(npm, n, dev)
            init = torch.eye(4, dtype=torch.float64, device=dev)
            init[:3, 3] = torch.tensor([0.05, -0.03, 0.02], dtype=torch.float64)
        else:
            trk = _tracker(room, cfg)
            w, _ = _room(n, seed=7)
            Ti = torch.linalg.inv(torch.as_tensor(room["T_gt"]))
            src = (w.double() @ Ti[:3, :3].T + Ti[:3, 3]).float().to(dev)
            init = torch.as_tensor(room["init_pose"]).to(dev)
        run_device(trk, src, init)          # warm-up of both (allocator, first-use reads)
        run_before(trk, cfg, src, init)
        rec = {"device": [], "before": []}
        for _ in range(a.rounds):
            rec["device"].append(run_device(trk, src, init))
            rec["before"].append(run_before(trk, cfg, src, init))
        row = {"map": map_name, "source_points": n}
        for k in ("device", "before"):
            runs = rec[k]
            ms = statistics.median(r[0] for r in runs) * 1e3
            it = runs[-1][1]
            row[k] = {"ms_per_call": round(ms, 3), "iterations": it, "ms_per_iteration": round(ms / max(it, 1), 4),
                      "package_host_reads_per_iteration": round(runs[-1][4] / max(it, 1), 3),
                      "torch_sync_warnings_per_iteration": round(runs[-1][5] / max(it, 1), 3),
                      "valid_flag": bool(runs[-1][3])}
        Td, Tb = rec["device"][-1][2], rec["before"][-1][2]
        if Td is not None and Tb is not None:
            D = (Td.double() - Tb.double()).abs()
            row["max_pose_diff"] = {"rotation": float(D[:3, :3].max()), "translation_m": float(D[:3, 3].max())}
        row["speedup_per_call"] = round(row["before"]["ms_per_call"] / row["device"]["ms_per_call"], 3)
        print(json.dumps(row))
        result["sizes"].append(row)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
