"""Share of the headline's live (record, tile) pairs that the class-2 blend kernels may treat as interior:
python tools/blend_interior_model.py [gaussians] [width] [height] [tiles] [nearest]

No GPU.  As tools/occl_bucket_model.py: bench.py's synth_cloud on the CPU generator (the same distribution as the
device's, NOT the same draws), the oracle's preprocess in fp32, the nearest `nearest` (8,000) survivors in depth order,
`tiles` (400) random tiles blended with the oracle's formulas.  A pair is LIVE when it stands at or before the list
position at which the tile's last pixel stops and passes the alpha tests at some pixel of the tile.  The class of a
pair is what the library's own classifier says (pings_raster_debug_interior -> csrc/raster_common.hpp: blend_interior),
so the shares are the classifier's, not a restatement's.  The two conditions on their own come from the same function
with the other half of the record replaced by a harmless one (a flat footprint far from the tile, opacity 0.5, for the
depth condition alone; a fronto-parallel plane at the centre's depth with a wide range for the alpha condition alone)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from oracle import raster_cpu as R
from pings_amd import _lib

TILE = 16


def interior_flags(recs, orgs, cxp, cyp, fx, fy):
    recs = np.ascontiguousarray(recs, dtype=np.float32)
    orgs = np.ascontiguousarray(orgs, dtype=np.float32)
    out = np.zeros(len(recs), dtype=np.uint8)
    st = _lib.lib().pings_raster_debug_interior(recs.ctypes.data_as(C.c_void_p), orgs.ctypes.data_as(C.c_void_p), len(recs),
                                                float(cxp), float(cyp), float(fx), float(fy), out.ctypes.data_as(C.c_void_p))
    _lib.check(st, "pings_raster_debug_interior")
    return out.astype(bool)


def main():
    a = sys.argv[1:]
    P = int(a[0]) if len(a) > 0 else 1_000_000
    W = int(a[1]) if len(a) > 1 else 1920
    H = int(a[2]) if len(a) > 2 else 1080
    n_tiles = int(a[3]) if len(a) > 3 else 400
    nearest = int(a[4]) if len(a) > 4 else 8000
    fx = 1000.0 * W / 1920.0
    means, _, op, scales, rot = bench.synth_cloud(P, W, H, fx, fx, "cpu", seed=42)
    cam = R.look_at_camera(W, H, fx, fx, W / 2 - 0.5, H / 2 - 0.5, 0.05, 110.0, dtype=torch.float32)
    s = R.Settings(H, W, cam["tanfovx"], cam["tanfovy"], torch.ones(3), 1.0, cam["viewmatrix"], cam["projmatrix"],
                   cam["projmatrix_raw"], cam["prcppoint"], front_only=True)
    with torch.no_grad():
        g = R.preprocess(means, scales, rot, s, opacities=op)
    valid = g["valid"].numpy()
    idx = np.nonzero(valid)[0]
    order = idx[np.lexsort((idx, g["pz"].numpy()[idx]))]          # the depth sort's stable order
    near = order[:nearest]
    f = lambda k: g[k].detach().numpy().astype(np.float32)[near]
    mx, my, pz, cx, cy, cz = f("mx"), f("my"), f("pz"), f("conic_x"), f("conic_y"), f("conic_z")
    nx, ny, nz, q, zhi = f("nx"), f("ny"), f("nz"), f("q"), f("zhi")
    o = op.reshape(-1).numpy().astype(np.float32)[near]
    xmin, xmax, ymin, ymax = (g[k].numpy()[near] for k in ("xmin", "xmax", "ymin", "ymax"))
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    rng = np.random.default_rng(7)
    tiles = rng.choice(gx * gy, size=min(n_tiles, gx * gy), replace=False)

    recs, orgs, blended = [], [], []
    kept = reached = never = 0
    for t in tiles:
        tx, ty = int(t % gx), int(t // gx)
        ranks = np.nonzero((xmin <= tx) & (tx < xmax) & (ymin <= ty) & (ty < ymax))[0]     # ascending = depth order
        if len(ranks) == 0:
            continue
        px, py = np.meshgrid(np.arange(tx * TILE, min(tx * TILE + TILE, W), dtype=np.float32),
                             np.arange(ty * TILE, min(ty * TILE + TILE, H), dtype=np.float32))
        px, py = px.reshape(1, -1), py.reshape(1, -1)
        dx, dy = mx[ranks, None] - px, my[ranks, None] - py
        power = np.float32(-0.5) * (cx[ranks, None] * dx * dx + cz[ranks, None] * dy * dy) - cy[ranks, None] * dx * dy
        al = np.minimum(o[ranks, None] * np.exp(power), np.float32(R.ALPHA_MAX))
        skip = (power > 0) | (al < R.ALPHA_MIN)
        T = np.cumprod(np.where(skip, np.float32(0), al) * np.float32(-1) + np.float32(1), axis=0)
        stopped = np.cumsum((~skip) & (T < R.T_EPS), axis=0) > 0
        if not stopped[-1].all():
            never += 1
            last = len(ranks)
        else:
            last = int(np.argmax(stopped, axis=0).max()) + 1         # list length up to the tile's last stop
        before = ~np.vstack([np.zeros((1, T.shape[1]), bool), stopped[:-1]])
        pix = ((~skip) & before)[:last]                               # (record, pixel) pairs the blend evaluates as valid
        kept += last
        reached += int((~skip[:last]).any(1).sum())
        for k in np.nonzero(pix.any(1))[0]:
            i = ranks[k]
            recs.append([mx[i], my[i], o[i], pz[i], cx[i], cy[i], cz[i], zhi[i] - pz[i], 0, 0, 0, q[i], nx[i], ny[i], nz[i], 0])
            orgs.append([tx * TILE, ty * TILE])
            blended.append(int(pix[k].sum()))
    recs, orgs, blended = np.array(recs, dtype=np.float32), np.array(orgs, dtype=np.float32), np.array(blended)
    cxp, cyp = np.float32(0.5) * np.float32(W) - np.float32(0.5), np.float32(0.5) * np.float32(H) - np.float32(0.5)
    cam_terms = (cxp, cyp, np.float32(fx), np.float32(fx))
    both = interior_flags(recs, orgs, *cam_terms)
    # condition (a) alone: the depth half replaced by a plane facing the camera at the centre's depth, wide range
    ra = recs.copy()
    ra[:, 7] = 1e3
    ra[:, 11] = -ra[:, 3]
    ra[:, 12:15] = [0.0, 0.0, -1.0]
    alpha_only = interior_flags(ra, orgs, *cam_terms)
    # condition (b) alone: the alpha half replaced by a flat footprint whose centre lies far left of the tile
    rb = recs.copy()
    rb[:, 0] = orgs[:, 0] - 1000.0
    rb[:, 1] = orgs[:, 1]
    rb[:, 2] = 0.5
    rb[:, 4:7] = [1e-8, 0.0, 1e-8]
    depth_only = interior_flags(rb, orgs, *cam_terms)
    n = len(recs)
    out = {"gaussians": P, "width": W, "height": H, "survivors": int(len(order)), "nearest_kept": int(len(near)),
           "tiles_blended": int(len(tiles)), "tiles_that_never_stop_within_nearest": never,
           "per_tile": {"kept_to_the_last_stop": round(kept / len(tiles), 1), "reached_by_the_alpha_ellipse": round(reached / len(tiles), 1),
                        "live": round(n / len(tiles), 1)},
           "live_pairs": n,
           "share_of_live_pairs": {"alpha_condition": round(float(alpha_only.mean()), 4),
                                   "depth_condition": round(float(depth_only.mean()), 4),
                                   "interior_both": round(float(both.mean()), 4),
                                   "opacity_above_0.99": round(float((recs[:, 2] >= np.float32(R.ALPHA_MAX)).mean()), 4)},
           "share_of_blended_record_pixel_pairs_held_by_interior_records": round(float(blended[both].sum() / blended.sum()), 4),
           "note": "CPU-generator draws of the headline cloud, not the device's; the class is pings_raster_debug_interior's"}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
