"""Wave-steps of occl_budget_kernel on the headline cloud, for three ways of dealing the (rank, tile) pairs to lanes:
python tools/occl_walk_model.py [gaussians] [width] [height]

No GPU: bench.py's synth_cloud on the CPU generator (the same distribution as the device's, not the same draws), the
oracle's restatement of preprocess_kernel's square and tight box (oracle/raster_cpu.py, fp32), the inner margins of
preprocess_kernel restated here in numpy with occ_amin 0.15, the (depth, index) order of the depth sort and
strided_rank of csrc/raster_fwd.hip.  A wave-step is one pass of a wave through the per-pair arithmetic
(tile_min_alpha and the atomic), whatever the number of lanes that hold a pair in it:
  * lanes      PINGS_OCC_WALK=l: a lane walks a rectangle of up to SMALL_RECT = 8 tiles itself (the wave steps until its
               longest such lane is done), the wave walks the larger ones one after the other, 64 tiles per step;
  * wave       the pairs of a wave's 64 ranks packed densely onto its lanes;
  * workgroup  the pairs of a workgroup's 256 ranks packed densely onto its 256 threads (the product)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from oracle import raster_cpu as R

OCC_AMIN, SMALL_RECT, TILE = 0.15, 8, 16


def inner_tiles(g, op):
    """Tiles of the inner rectangle per Gaussian: preprocess_kernel's margin rule in fp32 (0 where it is empty)."""
    f = lambda k: g[k].detach().numpy().astype(np.float32)
    cx, cy, cz, mx, my = f("conic_x"), f("conic_y"), f("conic_z"), f("mx"), f("my")
    xmin, xmax, ymin, ymax = (g[k].numpy() for k in ("xmin", "xmax", "ymin", "ymax"))
    valid = g["valid"].numpy()
    t = np.float32(TILE)
    with np.errstate(all="ignore"):
        det_c = cx * cz - cy * cy
        cxx, cyy, det = cz / det_c, cx / det_c, np.float32(1) / det_c
        mid = np.float32(0.5) * (cxx + cyy)
        lam_min = mid - np.sqrt(np.maximum(mid * mid - det, np.float32(0)))
        thr = np.float32(2) * np.log(op / np.float32(OCC_AMIN))
        ok = valid & (thr * lam_min >= 50)
        ex, ey = np.sqrt(thr * cxx), np.sqrt(thr * cyy)
        z = lambda a: np.where(ok, a, 0).astype(np.int64)
        ix0 = np.maximum(xmin, z(np.ceil((mx - ex) / t - np.float32(0.02))))
        ix1 = np.minimum(xmax, z(np.floor((mx + ex - 15) / t + np.float32(0.02)) + 1))
        iy0 = np.maximum(ymin, z(np.ceil((my - ey) / t - np.float32(0.02))))
        iy1 = np.minimum(ymax, z(np.floor((my + ey - 15) / t + np.float32(0.02)) + 1))
    return np.where(ok & (ix1 > ix0) & (iy1 > iy0), (ix1 - ix0) * (iy1 - iy0), 0)


def main():
    P = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    W = int(sys.argv[2]) if len(sys.argv) > 2 else 1920
    H = int(sys.argv[3]) if len(sys.argv) > 3 else 1080
    fx = 1000.0 * W / 1920.0
    means, _, op, scales, rot = bench.synth_cloud(P, W, H, fx, fx, "cpu", seed=42)
    cam = R.look_at_camera(W, H, fx, fx, W / 2 - 0.5, H / 2 - 0.5, 0.05, 110.0, dtype=torch.float32)
    s = R.Settings(H, W, cam["tanfovx"], cam["tanfovy"], torch.ones(3), 1.0, cam["viewmatrix"], cam["projmatrix"],
                   cam["projmatrix_raw"], cam["prcppoint"], front_only=True)
    with torch.no_grad():
        g = R.preprocess(means, scales, rot, s, opacities=op)
    valid = g["valid"].numpy()
    n_g = inner_tiles(g, op.reshape(-1).numpy())
    idx = np.nonzero(valid)[0]
    order = idx[np.lexsort((idx, g["pz"].numpy()[idx]))]          # the depth sort's stable order
    n = np.zeros(P, dtype=np.int64)                                # inner tiles by depth rank; culled ranks last
    n[:len(order)] = n_g[order]
    nw = 4 * ((P + 255) // 256)                                    # strided_rank
    wave, lane = np.divmod(np.arange(64 * nw), 64)
    r = np.where(lane < 16, lane * nw + wave, ((lane >> 4) * nw + wave) * 16 + (lane & 15))
    nl = np.where(r < P, n[np.minimum(r, P - 1)], 0).reshape(nw, 64)   # [wave, lane]

    small = np.where(nl <= SMALL_RECT, nl, 0)
    big = np.where(nl > SMALL_RECT, nl, 0)
    serial = small.max(1)                                          # the wave steps until its longest small lane is done
    coop = ((big + 63) // 64).sum(1)
    lanes_steps = serial + coop
    wave_steps = (nl.sum(1) + 63) // 64
    tot_wg = nl.reshape(-1, 4, 64).sum((1, 2))
    # wave w of a workgroup holds pairs 256 i + 64 w .. + 63: a step for every i with 256 i + 64 w < total
    wg_wave_steps = np.maximum(0, (tot_wg[:, None] - 64 * np.arange(4)[None, :] + 255) // 256)
    tiles_all = g["tiles_touched"].numpy()
    out = {
        "gaussians": P, "width": W, "height": H,
        "visible_gaussians": int(valid.sum()), "rectangle_pairs": int(tiles_all.sum()),
        "inner_pairs": int(n.sum()), "gaussians_with_inner_tiles": int((n > 0).sum()),
        "pairs_in_small_rectangles": int(small.sum()), "waves": int(nw),
        "lanes": {"wave_steps": int(lanes_steps.sum()), "serial_steps": int(serial.sum()),
                  "serial_active_lanes_per_step": round(float(small.sum()) / max(int(serial.sum()), 1), 2),
                  "coop_steps": int(coop.sum()),
                  "coop_lane_use": round(float(big.sum()) / max(64 * int(coop.sum()), 1), 3),
                  "mean_per_wave": round(float(lanes_steps.mean()), 2), "max_per_wave": int(lanes_steps.max()),
                  "max_per_wave_in_waves_4000_8000": int(lanes_steps[4000:8000].max()) if nw > 8000 else None},
        "wave": {"wave_steps": int(wave_steps.sum()), "max_per_wave": int(wave_steps.max())},
        "workgroup": {"wave_steps": int(wg_wave_steps.sum()), "max_per_workgroup": int(wg_wave_steps.sum(1).max()),
                      "max_per_wave": int(wg_wave_steps.max()),
                      "workgroups_without_a_pair": int((tot_wg == 0).sum()), "workgroups": int(len(tot_wg))},
    }
    print(json.dumps(out, indent=1))
    L, Wv, G = out["lanes"], out["wave"], out["workgroup"]
    print(f"\n| quantity | value |\n|---|---|")
    print(f"| inner-rectangle pairs | {out['inner_pairs'] / 1e6:.2f} M in {out['gaussians_with_inner_tiles']:,} Gaussians |")
    print(f"| pairs in rectangles of <= {SMALL_RECT} tiles | {out['pairs_in_small_rectangles']:,} |")
    print(f"| lanes walk: serial steps | {L['serial_steps']:,} at {L['serial_active_lanes_per_step']} active lanes |")
    print(f"| lanes walk: cooperative steps | {L['coop_steps']:,} at {100 * L['coop_lane_use']:.0f} % lane use |")
    print(f"| lanes walk: total / mean / max per wave | {L['wave_steps']:,} / {L['mean_per_wave']} / {L['max_per_wave']} |")
    print(f"| dense per wave: total / max per wave | {Wv['wave_steps']:,} / {Wv['max_per_wave']} |")
    print(f"| dense per workgroup: total / max per workgroup / per wave | {G['wave_steps']:,} / {G['max_per_workgroup']} / "
          f"{G['max_per_wave']} |")


if __name__ == "__main__":
    main()
