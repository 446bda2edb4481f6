"""Instances per tile on the headline cloud for different rank-bucket maps of the occlusion bound:
python tools/occl_bucket_model.py [gaussians] [width] [height] [tiles] [nearest]

No GPU: bench.py's synth_cloud on the CPU generator (the same distribution as the device's, not the same draws), the
oracle's preprocess in fp32 (oracle/raster_cpu.py), the nearest `nearest` (8,000) survivors in the (depth, index) order
of the depth sort, and `tiles` (600) random tiles blended with the oracle's formulas (alpha = min(0.99, o e^power),
skipped below 1/255 or for power > 0, a pixel stops at T < 1e-4).  The STOP RANK of a tile is the depth rank of the record
at which its last pixel stops; a tile keeps every record up to the end of the bucket that holds its cut rank, and the
real (conservative) bound cuts somewhere between 1.0 and 1.5 times the stop rank, so both are printed.  Maps:
  * equal     floor(nb r / nvalid), nb = 256: every bucket nvalid / nb ranks wide;
  * shift6    r >> 6;
  * loglin    rank_bucket of csrc/raster_common.hpp (w0 = 2^LW ranks per unit, s = 2^LS buckets per octave of the unit
              number, then the ranks behind dealt equally) — restated below, tests/test_rank_buckets.py holds it to the
              library's own function;
  * floor     one rank per bucket."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from oracle import raster_cpu as R

TILE, NB = 16, 256


def loglin(r, nb, nvalid, lw=4, ls=4):
    """rank_bucket (csrc/raster_common.hpp) for an int64 array of ranks below nvalid."""
    eq = (nvalid - 1) // nb + 1
    J = min((eq >> lw).bit_length() + 1, nb >> (ls + 1)) if eq >> lw else 0
    fr, fb = (1 << (lw + ls + J - 1) if J else 0), J << ls
    q = r >> lw
    e = np.zeros_like(q)
    for sh in range(1, 40):
        e += (q >> sh) != 0
    k = np.maximum(e - ls, 0)
    front = np.where(q < (1 << ls), q, (k << ls) + (q >> k))
    behind = fb + (np.maximum(r - fr, 0) * (nb - fb)) // max(nvalid - fr, 1)
    return np.where(r < fr, front, np.minimum(behind, nb - 1))


def main():
    a = sys.argv[1:]
    P = int(a[0]) if len(a) > 0 else 1_000_000
    W = int(a[1]) if len(a) > 1 else 1920
    H = int(a[2]) if len(a) > 2 else 1080
    n_tiles = int(a[3]) if len(a) > 3 else 600
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
    nvalid = len(order)
    near = order[:nearest]                                          # rank r = position in `near`
    f = lambda k: g[k].detach().numpy().astype(np.float32)[near]
    mx, my, cx, cy, cz = f("mx"), f("my"), f("conic_x"), f("conic_y"), f("conic_z")
    o = op.reshape(-1).numpy().astype(np.float32)[near]
    xmin, xmax, ymin, ymax = (g[k].numpy()[near] for k in ("xmin", "xmax", "ymin", "ymax"))
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    rng = np.random.default_rng(7)
    tiles = rng.choice(gx * gy, size=min(n_tiles, gx * gy), replace=False)

    maps = {
        "equal-count, 256 buckets": lambda r: np.minimum(NB - 1, r * NB // nvalid),
        "r >> 6": lambda r: r >> 6,
        "log-linear 16 / 16 (rank_bucket)": lambda r: loglin(r, NB, nvalid),
        "log-linear 32 / 8": lambda r: loglin(r, NB, nvalid, 5, 3),
        "one rank per bucket (floor)": lambda r: r,
    }
    stops, live, per_map = [], [], {k: {1.0: [], 1.5: []} for k in maps}
    never = 0
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
        stop = (~skip) & (T < R.T_EPS)
        stopped = np.cumsum(stop, axis=0) > 0
        if not stopped[-1].all():
            never += 1                                              # keeps its whole list under any map
            continue
        first = np.argmax(stopped, axis=0)                          # list position at which each pixel stops
        stop_rank = int(ranks[first.max()])
        stops.append(stop_rank)
        live.append(int(((~skip) & ~np.vstack([np.zeros((1, T.shape[1]), bool), stopped[:-1]])).any(1).sum()))
        for name, m in maps.items():
            b = m(ranks.astype(np.int64))
            for mult in (1.0, 1.5):
                cut = min(int(mult * stop_rank), nearest - 1)
                per_map[name][mult].append(int((b <= m(np.array([cut], dtype=np.int64))[0]).sum()))
    stops = np.array(stops)
    out = {"gaussians": P, "width": W, "height": H, "survivors": int(nvalid), "nearest_kept": int(len(near)),
           "tiles_blended": int(len(stops) + never), "tiles_that_never_stop_within_nearest": never,
           "stop_rank_p5_p50_p95_max": [int(np.percentile(stops, q)) for q in (5, 50, 95)] + [int(stops.max())],
           "live_records_per_tile": round(float(np.mean(live)), 1),
           "instances_per_tile": {k: {str(m): round(float(np.mean(v[m])), 1) for m in v} for k, v in per_map.items()}}
    print(json.dumps(out, indent=1))
    print("\n| bucket map | 1.0x | 1.5x |\n|---|---|---|")
    for k, v in out["instances_per_tile"].items():
        print(f"| {k} | {v['1.0']} | {v['1.5']} |")


if __name__ == "__main__":
    main()
