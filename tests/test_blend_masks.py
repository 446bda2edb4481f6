"""Footprint class 2 blend kernels at the cases in which a per-pixel decision goes wrong most easily.  The tile FORWARD
keeps valid / stop / contrib as 64-bit lane masks and every select reads its mask; the class-2 BACKWARD decides with
plain booleans (a mask rewrite of it was measured and not kept), and its tests here pin that kernel as it stands.  The
scenes are small (56 x 40: a partial last tile column and row) and are CHECKED to reach the cases — from a restatement of
the kernels' walk over the fp32 oracle's lists (`_walk`), before any output is compared:

forward   a record on which a pixel stops while no pixel of the tile contributes; a pixel that stops on a record to
          which its pair partner (x + 8) contributes, and the reverse; the last live pixel of a tile stopping in the
          middle of a 16-record group with records behind it in the window; lists of more than one 64-entry window and
          a window whose compacted count is no multiple of 16; power > 0 on a live pixel; alpha below 1/255 on one pixel
          of a pair and above it on the other; pairs with one pixel outside the image.
backward  (surfels) the four depth-clamp classes on blended (record, pixel)s with a non-zero upstream depth gradient and
          a pair in two different classes; raw = opacity * G above 0.99 on one pixel of a pair only; pixels whose
          n_contrib lies inside a 64-record batch.

Occlusion culling is off here, so the kernels walk exactly the oracle's lists."""
import numpy as np
import pytest
import torch

from test_blend_class2 import _edge_scene, _forward_outputs, _grads
from test_raster import _assert_grad_gate, _oracle, _oracle_grads, _undecidable

ALPHA_MIN, ALPHA_MAX, T_EPS, DEN_EPS = 1.0 / 255.0, 0.99, 1e-4, 1e-6
W, H = 56, 40
CASES = [("surfel", 71), ("3dgs", 72)]
P = {"surfel": 2500, "3dgs": 700}   # (front-facing surfels only: it takes more of them to saturate a tile)
NEEDLES = 8


def _scene(mode, seed, needles=False):
    """_edge_scene at 56 x 40.  `needles` (forward tests): a few splats 400 m long and 4 mm wide, close to the camera.
    The determinant of such a footprint's 2-D covariance cancels in fp32, the conic that comes out is no longer positive
    definite and the quadratic form is above zero on whole stretches of pixels: the `power > 0` skip.  (The oracle marks
    the pixels these footprints cover as undecidable, so the gradient tests, which are gated against it, do without them.)"""
    sc = _edge_scene(mode, seed, P=P[mode], W=W, H=H)
    if needles:
        i0 = P[mode] // 2
        sc["scales"][i0:i0 + NEEDLES, 0] = 400.0
        sc["scales"][i0:i0 + NEEDLES, 1] = 0.004
        if mode != "surfel":
            sc["scales"][i0:i0 + NEEDLES, 2] = 0.004
        sc["op"][i0:i0 + NEEDLES] = 0.6
        sc["means"][i0:i0 + NEEDLES] *= 0.4          # towards the camera: in front of where the tiles saturate
    return sc


def _edge_min_q(a, b, c, d, lo, hi):
    t = torch.minimum(torch.maximum(-(b * d) / c, lo), hi)
    q0, q1, q2 = a * d * d, 2.0 * b * d * t, c * t * t
    return (q0 + q1 + q2) - 2e-5 * (q0 + q1.abs() + q2)


def _misses_tile(g, op, gi, x0, y0):
    """footprint_misses_rect of the tile kernel (raster_common.hpp) for the closed rectangle [x0, x0+15] x [y0, y0+15]."""
    mx, my, cx, cy, cz = (g[k][gi].double() for k in ("mx", "my", "conic_x", "conic_y", "conic_z"))
    thr = 2.0 * torch.log(255.0 * op[gi].double()) + 2e-3
    x1, y1 = x0 + 15.0, y0 + 15.0
    centre = (mx >= x0) & (mx <= x1) & (my >= y0) & (my <= y1)
    lx, hx, ly, hy = x0 - mx, x1 - mx, y0 - my, y1 - my
    m = _edge_min_q(cx, cy, cz, lx, ly, hy)
    m = torch.minimum(m, _edge_min_q(cx, cy, cz, hx, ly, hy))
    m = torch.minimum(m, _edge_min_q(cz, cy, cx, ly, lx, hx))
    m = torch.minimum(m, _edge_min_q(cz, cy, cx, hy, lx, hx))
    return ~centre & (m > thr)


def _walk(o, sc, surfel):
    """The tile kernels' walk over the oracle's lists, restated: which of the cases above occur (counts)."""
    g, ranges, pl = o["geom"], o["ranges"], torch.from_numpy(np.asarray(o["point_list"])).long()
    op = sc["op"].reshape(-1).to(g["mx"].dtype)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    cam = sc["cam"]
    fx, fy = W / (2.0 * cam["tanfovx"]), H / (2.0 * cam["tanfovy"])
    cxp, cyp = float(cam["prcppoint"][0]) * W - 0.5, float(cam["prcppoint"][1]) * H - 0.5
    ev = dict(stop_without_contrib=0, left_stops_right_contributes=0, right_stops_left_contributes=0,
              tile_done_mid_group=0, second_window=0, window_not_multiple_of_16=0, power_positive=0,
              alpha_min_splits_pair=0, pair_half_outside=0, clamp_lo=0, clamp_hi=0, mid_hit=0, mid_nohit=0,
              pair_two_classes=0, alpha_max_splits_pair=0, last_inside_batch=0)
    nc = np.asarray(o["n_contrib"])
    for t in range(gx * gy):
        ty, tx = divmod(t, gx)
        iy, ix = torch.meshgrid(torch.arange(16), torch.arange(16), indexing="ij")
        px, py = (tx * 16 + ix).reshape(-1), (ty * 16 + iy).reshape(-1)
        inside = (px < W) & (py < H)
        left = (ix.reshape(-1) < 8)
        partner = torch.arange(256) + torch.where(left, 8, -8)
        ev["pair_half_outside"] += int((inside & ~inside[partner]).sum())
        a, b = int(ranges[t, 0]), int(ranges[t, 1])
        if b <= a:
            continue
        gi = pl[a:b]
        dt = g["mx"].dtype
        dx = g["mx"][gi, None] - px[None].to(dt)
        dy = g["my"][gi, None] - py[None].to(dt)
        power = -0.5 * (g["conic_x"][gi, None] * dx * dx + g["conic_z"][gi, None] * dy * dy) - g["conic_y"][gi, None] * dx * dy
        raw = op[gi, None] * torch.exp(power)
        al = raw.clamp(max=ALPHA_MAX)
        skip = (power > 0) | (al < ALPHA_MIN) | ~inside[None]
        Tincl = torch.cumprod(torch.where(skip, torch.ones_like(al), 1.0 - al), dim=0)
        stop = ~skip & (Tincl < T_EPS)
        nstop = torch.cumsum(stop.int(), dim=0)
        first_stop = stop & (nstop == 1)
        done_before = (nstop - stop.int()) > 0            # stopped on an earlier record
        incl = ~skip & (nstop == 0)
        miss = _misses_tile(g, op, gi, float(tx * 16), float(ty * 16))
        live = int(inside.sum())
        for base in range(0, b - a, 64):
            if live == 0:
                break
            kept = [i for i in range(base, min(base + 64, b - a)) if not bool(miss[i])]
            ev["second_window"] += int(base >= 64 and len(kept) > 0)
            ev["window_not_multiple_of_16"] += int(len(kept) % 16 != 0)
            for c, i in enumerate(kept):
                if live == 0:
                    break
                fs, inc = first_stop[i], incl[i]
                alive = inside & ~done_before[i]
                ev["stop_without_contrib"] += int(fs.any() and not inc.any())
                ev["left_stops_right_contributes"] += int((fs & left & inc[partner]).sum())
                ev["right_stops_left_contributes"] += int((fs & ~left & inc[partner]).sum())
                ev["power_positive"] += int((alive & (power[i] > 0)).sum())
                both = alive & alive[partner] & (power[i] <= 0) & (power[i][partner] <= 0)
                ev["alpha_min_splits_pair"] += int((both & left & ((al[i] < ALPHA_MIN) != (al[i][partner] < ALPHA_MIN))).sum())
                ev["alpha_max_splits_pair"] += int((inc & inc[partner] & left & ((raw[i] > ALPHA_MAX) != (raw[i][partner] > ALPHA_MAX))).sum())
                live -= int(fs.sum())
                if live == 0 and c % 16 != 15 and c + 1 < len(kept):
                    ev["tile_done_mid_group"] += 1
        if surfel:
            rx, ry = (px.to(dt) - cxp) / fx, (py.to(dt) - cyp) / fy
            den = (g["nx"][gi, None] * rx[None] + g["ny"][gi, None] * ry[None]) + g["nz"][gi, None]
            hit = den < -DEN_EPS
            d0 = torch.where(hit, g["q"][gi, None] / torch.where(hit, den, -torch.ones_like(den)), g["pz"][gi, None].expand_as(den))
            lo, hi = d0 < g["zlo"][gi, None], d0 > g["zhi"][gi, None]
            cls = torch.where(lo, 0, torch.where(hi, 1, torch.where(hit, 2, 3)))
            for k, name in enumerate(("clamp_lo", "clamp_hi", "mid_hit", "mid_nohit")):
                ev[name] += int((incl & (cls == k)).sum())
            ev["pair_two_classes"] += int((incl & incl[:, partner] & left[None] & (cls != cls[:, partner])).sum())
        nct = np.zeros((16, 16), dtype=np.int64)
        hh, ww = min(16, H - ty * 16), min(16, W - tx * 16)
        nct[:hh, :ww] = nc[ty * 16:ty * 16 + hh, tx * 16:tx * 16 + ww]
        ev["last_inside_batch"] += int(((nct > 0) & (nct < nct.max()) & (nct % 64 != 0)).sum())
    return ev


FWD_CASES = ("stop_without_contrib", "left_stops_right_contributes", "right_stops_left_contributes", "tile_done_mid_group",
             "second_window", "window_not_multiple_of_16", "power_positive", "alpha_min_splits_pair", "pair_half_outside")
BWD_CASES = ("alpha_max_splits_pair", "last_inside_batch")
BWD_SURFEL_CASES = ("clamp_lo", "clamp_hi", "mid_hit", "mid_nohit", "pair_two_classes")


@pytest.mark.gpu
@pytest.mark.parametrize("needles", [False, True])
@pytest.mark.parametrize("mode,seed", CASES)
def test_tile_forward_masks_bit_identical_and_counts_match_the_oracle(mode, seed, needles, monkeypatch):
    """Tile kernel against the wave-per-quadrant forward, bit for bit, and n_contrib against the fp32 oracle wherever fp32
    can decide the stop rule.  The plain scene reaches every forward case but `power > 0` and is decidable on all but
    a few pixels; the needle scene adds `power > 0` (its footprints make most pixels undecidable for the oracle gate,
    not for the comparison of the two kernels, which evaluate the same fp32 operations)."""
    monkeypatch.setenv("PINGS_RASTER_OCCLUSION", "0")
    sc = _scene(mode, seed, needles)
    o32, *_ = _oracle(sc, torch.float32, mode, True, margins=True)
    ev = _walk(o32, sc, mode == "surfel")
    pix_flag, _ = _undecidable(o32)
    print(f"\n[{mode} seed={seed} needles={needles}] cases reached: {ev}; undecidable pixels {int(pix_flag.sum())} of {W * H}")
    for k in FWD_CASES:
        assert ev[k] > 0 or (k == "power_positive" and not needles), (k, ev)
    if not needles:
        assert int(pix_flag.sum()) < W * H // 50
    a = _forward_outputs(sc, mode, "4", monkeypatch)
    b = _forward_outputs(sc, mode, "-1", monkeypatch)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    bad = a["n_contrib"].reshape(H, W) != o32["n_contrib"]
    assert not (bad & ~pix_flag).any()            # a count may differ only where fp32 cannot decide the stop rule


@pytest.mark.gpu
@pytest.mark.parametrize("mode,seed", CASES)
def test_tile_backward_masks_match_scan_backward_and_oracle(mode, seed, monkeypatch):
    """The class-2 backward as it stands (boolean decisions) on a scene that reaches every clamp class, a pair split by the
    0.99 clamp and batches split by `idx < last`: within 1e-4 of the scan backward, under the fp64 oracle gate, and
    bitwise reproducible.  Whoever rewrites that kernel's decisions has these cases pinned."""
    monkeypatch.setenv("PINGS_RASTER_OCCLUSION", "0")
    sc = _scene(mode, seed)
    o64, names, ref64, ups = _oracle_grads(sc, torch.float64, mode, True)
    o32, _, ref32, _ = _oracle_grads(sc, torch.float32, mode, True)
    ev = _walk(o32, sc, mode == "surfel")
    print(f"\n[{mode} seed={seed}] cases reached: {ev}")
    for k in BWD_CASES + (BWD_SURFEL_CASES if mode == "surfel" else ()):
        assert ev[k] > 0, (k, ev)
    # the upstream depth gradient is non-zero on every pixel (so every clamp class above carries one)
    assert bool((ups[2] != 0).all())
    tile = _grads(sc, mode, ups, "tile", monkeypatch)
    again = _grads(sc, mode, ups, "tile", monkeypatch)
    scan = _grads(sc, mode, ups, "scan", monkeypatch)
    for name, a, b, c in zip(names, tile, again, scan):
        assert torch.equal(a, b), name
        scale = max(c.abs().max().item(), 1e-30)
        assert (a - c).abs().max().item() <= 1e-4 * scale, (name, (a - c).abs().max().item() / scale)
    _assert_grad_gate(names, tile, ref64, ref32, f"class-2 masks {mode} seed={seed}", flips_allowed=True)
