"""Restatement of the 2D Gaussian splatting rasteriser (`diff_surfel_rasterization`) — TEST INFRASTRUCTURE.

PARITY UNPINNED.  The reference imports the extension (gaussian_splatting/gaussian_renderer/__init__.py:88-89) but its
CUDA sources are not in the reference tree.  This module restates the published algorithm (Huang et al., "2D Gaussian
Splatting for Geometrically Accurate Radiance Fields", SIGGRAPH 2024) in the conventions of oracle/raster_cpu.py; every
point only the absent CUDA could settle is a numbered assumption in DESIGN.md §3 (2D-1 .. 2D-9).

One torch code path runs in float32 and in float64:
* `preprocess` in float32 follows the HIP preprocess kernel (pings_amd/csrc/raster2d.hip) op for op, so radii, tile
  squares, depth keys and therefore the sorted lists are pinned bit for bit;
* `render` in float64 gives the values and, through autograd, the gradients the kernels are compared against;
* `render` in float32 gives the decisions a float32 evaluation takes; `undecidable` flags the pixels in which one of
  them (alpha ~ 1/255, rho3 ~ rho2, T ~ 0.5 at the median, the stop threshold, the 0.99 clamp, the near test) lies
  within float32 rounding of its threshold.

Not collected by pytest (no `test_` prefix).
"""
from __future__ import annotations

import math

import torch

TILE = 16
NEAR_Z = 0.2
FAR_Z = 100.0
ALPHA_MAX = 0.99
ALPHA_MIN = 1.0 / 255.0
T_EPS = 1e-4
CUTOFF2 = 9.0
FILTER_R = 2.12132034          # c sqrt(2) / 2, as the fp32 constant of the kernel
CHANNELS = ("depth", "alpha", "nx", "ny", "nz", "median", "dist")


def quat_to_rot(q):
    """Un-normalised quaternion (r, x, y, z) -> R [P,3,3], the formula of the HIP preprocess (no normalisation)."""
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one = torch.ones_like(r)
    R = torch.stack([
        one - 2.0 * (y * y + z * z), 2.0 * (x * y - r * z), 2.0 * (x * z + r * y),
        2.0 * (x * y + r * z), one - 2.0 * (x * x + z * z), 2.0 * (y * z - r * x),
        2.0 * (x * z - r * y), 2.0 * (y * z + r * x), one - 2.0 * (x * x + y * y)], 1)
    return R.view(-1, 3, 3)


def _to_pixel_h(Pm, a0, a1, a2, homog, W, H):
    c0 = (a0 * Pm[0, 0] + a1 * Pm[1, 0]) + a2 * Pm[2, 0]
    c1 = (a0 * Pm[0, 1] + a1 * Pm[1, 1]) + a2 * Pm[2, 1]
    c3 = (a0 * Pm[0, 3] + a1 * Pm[1, 3]) + a2 * Pm[2, 3]
    if homog:
        c0 = c0 + Pm[3, 0]
        c1 = c1 + Pm[3, 1]
        c3 = c3 + Pm[3, 3]
    dt = a0.dtype
    hw, hw1 = torch.tensor(0.5 * W, dtype=dt), torch.tensor(0.5, dtype=dt) * (torch.tensor(float(W), dtype=dt) - 1.0)
    hh, hh1 = torch.tensor(0.5 * H, dtype=dt), torch.tensor(0.5, dtype=dt) * (torch.tensor(float(H), dtype=dt) - 1.0)
    return hw * c0 + hw1 * c3, hh * c1 + hh1 * c3, c3


def _rect_lo(v, g):
    return torch.where(v <= 0, torch.zeros_like(v), torch.where(v >= g, torch.full_like(v, float(g)), torch.trunc(v)))


def preprocess(means, scales, rot, opac, view, proj, W, H, scale_modifier=1.0):
    """Per-Gaussian stage in the tensors' dtype.  Returns a dict: T [P,3,3] (rows t_u, t_v, point; columns u, v, w),
    mu [P,2], nc [P,3] (camera-frame normal facing the camera), sign [P], pz [P], radii [P] int, rect [P,4] int
    (xmin, ymin, xmax, ymax tiles), ok [P] bool (kept: radius > 0)."""
    dt = means.dtype
    V, Pm = view.to(dt), proj.to(dt)
    x, y, z = means[:, 0], means[:, 1], means[:, 2]
    px = ((V[0, 0] * x + V[1, 0] * y) + V[2, 0] * z) + V[3, 0]
    py = ((V[0, 1] * x + V[1, 1] * y) + V[2, 1] * z) + V[3, 1]
    pz = ((V[0, 2] * x + V[1, 2] * y) + V[2, 2] * z) + V[3, 2]
    ok = pz > NEAR_Z
    R = quat_to_rot(rot)
    mod = torch.tensor(scale_modifier, dtype=dt)
    s0, s1 = mod * scales[:, 0], mod * scales[:, 1]
    rows = [
        _to_pixel_h(Pm, R[:, 0, 0] * s0, R[:, 1, 0] * s0, R[:, 2, 0] * s0, False, W, H),
        _to_pixel_h(Pm, R[:, 0, 1] * s1, R[:, 1, 1] * s1, R[:, 2, 1] * s1, False, W, H),
        _to_pixel_h(Pm, x, y, z, True, W, H),
    ]
    T = torch.stack([torch.stack(r, 1) for r in rows], 1)     # [P, 3 rows, 3 cols]
    c2 = torch.tensor(CUTOFF2, dtype=dt)
    d = (c2 * (T[:, 0, 2] * T[:, 0, 2]) + c2 * (T[:, 1, 2] * T[:, 1, 2])) + (-1.0) * (T[:, 2, 2] * T[:, 2, 2])
    ok = ok & (d != 0)
    dd = torch.where(d != 0, d, torch.ones_like(d))
    f0, f1, f2 = c2 / dd, c2 / dd, -1.0 / dd
    mx = ((f0 * T[:, 0, 0]) * T[:, 0, 2] + (f1 * T[:, 1, 0]) * T[:, 1, 2]) + (f2 * T[:, 2, 0]) * T[:, 2, 2]
    my = ((f0 * T[:, 0, 1]) * T[:, 0, 2] + (f1 * T[:, 1, 1]) * T[:, 1, 2]) + (f2 * T[:, 2, 1]) * T[:, 2, 2]
    sx = ((f0 * T[:, 0, 0]) * T[:, 0, 0] + (f1 * T[:, 1, 0]) * T[:, 1, 0]) + (f2 * T[:, 2, 0]) * T[:, 2, 0]
    sy = ((f0 * T[:, 0, 1]) * T[:, 0, 1] + (f1 * T[:, 1, 1]) * T[:, 1, 1]) + (f2 * T[:, 2, 1]) * T[:, 2, 1]
    lo = torch.tensor(1e-4, dtype=dt)
    ex = torch.sqrt(torch.maximum(lo, mx * mx - sx).detach())
    ey = torch.sqrt(torch.maximum(lo, my * my - sy).detach())
    radius = torch.ceil(torch.maximum(torch.maximum(ex, ey), torch.tensor(FILTER_R, dtype=dt)))
    ok = ok & torch.isfinite(mx.detach()) & torch.isfinite(my.detach()) & torch.isfinite(radius)
    n = R[:, :, 2]
    nx = (V[0, 0] * n[:, 0] + V[1, 0] * n[:, 1]) + V[2, 0] * n[:, 2]
    ny = (V[0, 1] * n[:, 0] + V[1, 1] * n[:, 1]) + V[2, 1] * n[:, 2]
    nz = (V[0, 2] * n[:, 0] + V[1, 2] * n[:, 1]) + V[2, 2] * n[:, 2]
    cosv = ((nx * px + ny * py) + nz * pz).detach()
    ok = ok & (cosv != 0)
    sign = torch.where(cosv > 0, -torch.ones_like(cosv), torch.ones_like(cosv))
    nc = torch.stack([sign * nx, sign * ny, sign * nz], 1)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    mxd, myd = mx.detach(), my.detach()
    rsafe = torch.where(ok, radius, torch.zeros_like(radius))
    mxs = torch.where(ok, mxd, torch.zeros_like(mxd))
    mys = torch.where(ok, myd, torch.zeros_like(myd))
    t = torch.tensor(float(TILE), dtype=dt)
    xmin = _rect_lo((mxs - rsafe) / t, gx)
    ymin = _rect_lo((mys - rsafe) / t, gy)
    xmax = _rect_lo(((mxs + rsafe) + (TILE - 1)) / t, gx)
    ymax = _rect_lo(((mys + rsafe) + (TILE - 1)) / t, gy)
    rect = torch.stack([xmin, ymin, xmax, ymax], 1).long()
    ntiles = (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])
    ok = ok & (ntiles > 0)
    rect = torch.where(ok[:, None], rect, torch.zeros_like(rect))
    radii = torch.where(ok, radius, torch.zeros_like(radius)).long()
    return dict(T=T, mu=torch.stack([mx, my], 1), nc=nc, sign=sign, pz=pz.detach(), radii=radii, rect=rect, ok=ok)


def build_lists(pre, W, H):
    """Instances sorted by (tile, fp32 view depth, Gaussian index) -> (point_list [I] long, ranges [tiles,2] long)."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    ok = pre["ok"]
    ids = torch.nonzero(ok).view(-1)
    tiles, gids = [], []
    rect = pre["rect"]
    for g in ids.tolist():
        x0, y0, x1, y1 = rect[g].tolist()
        for ty in range(y0, y1):
            for tx in range(x0, x1):
                tiles.append(ty * gx + tx)
                gids.append(g)
    tiles = torch.tensor(tiles, dtype=torch.long)
    gids = torch.tensor(gids, dtype=torch.long)
    depth = pre["pz"].to(torch.float32)
    order = sorted(range(len(gids)), key=lambda i: (int(tiles[i]), float(depth[gids[i]]), int(gids[i])))
    order = torch.tensor(order, dtype=torch.long)
    pl = gids[order] if len(order) else gids
    ts = tiles[order] if len(order) else tiles
    ranges = torch.zeros(gx * gy, 2, dtype=torch.long)
    if len(ts):
        cnt = torch.bincount(ts, minlength=gx * gy)
        end = torch.cumsum(cnt, 0)
        ranges[:, 0] = end - cnt
        ranges[:, 1] = end
    return pl, ranges


def _tile_pixels(tile, W, H, dtype):
    gx = (W + TILE - 1) // TILE
    X0, Y0 = (tile % gx) * TILE, (tile // gx) * TILE
    yy, xx = torch.meshgrid(torch.arange(Y0, Y0 + TILE), torch.arange(X0, X0 + TILE), indexing="ij")
    keep = (xx < W) & (yy < H)
    return xx[keep], yy[keep]


def _eval_tile(T, mu, op, col, nc, x, y):
    """Pairs (n splats of the tile's list) x (m pixels), list order.  Returns every per-pair quantity and the
    per-pixel outputs; decisions are taken in the tensors' dtype."""
    dt = T.dtype
    xf, yf = x.to(dt)[None, :], y.to(dt)[None, :]
    k = [xf * T[:, i, 2:3] - T[:, i, 0:1] for i in range(3)]
    l = [yf * T[:, i, 2:3] - T[:, i, 1:2] for i in range(3)]
    qx = k[1] * l[2] - k[2] * l[1]
    qy = k[2] * l[0] - k[0] * l[2]
    qz = k[0] * l[1] - k[1] * l[0]
    nz = qz != 0
    iqz = 1.0 / torch.where(nz, qz, torch.ones_like(qz))
    su, sv = qx * iqz, qy * iqz
    rho3 = su * su + sv * sv
    dx, dy = mu[:, 0:1] - xf, mu[:, 1:2] - yf
    rho2 = 2.0 * (dx * dx + dy * dy)
    on = rho3 <= rho2
    rho = torch.where(on, rho3, rho2)
    depth = torch.where(on, (su * T[:, 0, 2:3] + sv * T[:, 1, 2:3]) + T[:, 2, 2:3], T[:, 2, 2:3].expand_as(su))
    G = torch.exp(-0.5 * rho)
    a_raw = op[:, None] * G
    clamped = a_raw > ALPHA_MAX
    alpha = torch.where(clamped, torch.full_like(a_raw, ALPHA_MAX), a_raw)
    valid = nz & (depth >= NEAR_Z) & (alpha >= ALPHA_MIN)
    a_v = torch.where(valid, alpha, torch.zeros_like(alpha))
    n = a_v.shape[0]
    one_m = 1.0 - a_v
    Tb = torch.cumprod(torch.cat([torch.ones_like(one_m[:1]), one_m[:-1]], 0), 0) if n else one_m
    test = Tb * one_m
    stop_c = valid & (test < T_EPS)
    idx = torch.arange(n)[:, None].expand_as(stop_c)
    big = torch.full_like(idx, n)
    stop = torch.where(stop_c, idx, big).min(0).values if n else torch.zeros(x.shape[0], dtype=torch.long)
    inc = valid & (idx < stop[None, :])
    a_i = torch.where(inc, alpha, torch.zeros_like(alpha))
    one_m = 1.0 - a_i
    Tb = torch.cumprod(torch.cat([torch.ones_like(one_m[:1]), one_m[:-1]], 0), 0) if n else one_m
    T_fin = Tb[-1] * one_m[-1] if n else torch.ones(x.shape[0], dtype=dt)
    w = a_i * Tb
    m = (FAR_Z / (FAR_Z - NEAR_Z)) * (1.0 - NEAR_Z / torch.where(inc, depth, torch.ones_like(depth)))
    M1c = torch.cumsum(w * m, 0)
    M2c = torch.cumsum(w * m * m, 0)
    M1b, M2b = M1c - w * m, M2c - w * m * m
    A = 1.0 - Tb
    dist = (w * ((m * m * A + M2b) - 2.0 * m * M1b)).sum(0)
    medc = inc & (Tb > 0.5)
    med_idx = torch.where(medc, idx, torch.full_like(idx, -1)).max(0).values if n else torch.full((x.shape[0],), -1)
    sel = torch.where(med_idx >= 0, med_idx, torch.zeros_like(med_idx))
    med = torch.where(med_idx >= 0, depth.gather(0, sel[None, :])[0], torch.zeros_like(T_fin)) if n else T_fin * 0
    out = dict(
        C=(w[:, :, None] * col[:, None, :]).sum(0), D=(w * depth).sum(0), A=1.0 - T_fin,
        N=(w[:, :, None] * nc[:, None, :]).sum(0), med=med, dist=dist, T=T_fin,
        last=torch.where(inc, idx + 1, torch.zeros_like(idx)).max(0).values if n else torch.zeros_like(stop),
        med_idx=med_idx)
    pair = dict(valid=valid, inc=inc, on=on, rho3=rho3, rho2=rho2, depth=depth, a_raw=a_raw, Tb=Tb, test=test,
                stop=stop)
    return out, pair


def render(pre, col, op, pl, ranges, bg, W, H, keep_pairs=False, tiles=None):
    """Images [3,H,W] and allmap [7,H,W] (plus per-pixel final T / last / median index and, with keep_pairs, the
    per-tile pair quantities) in the dtype of pre["T"]."""
    dt = pre["T"].dtype
    nt = ranges.shape[0]
    img = bgd_img = None
    allm = torch.zeros(7, H * W, dtype=dt)
    fT = torch.ones(H * W, dtype=dt)
    last = torch.zeros(H * W, dtype=torch.long)
    medi = torch.full((H * W,), -1, dtype=torch.long)
    pairs = {}
    bgd = bg.to(dt)
    img_parts, all_parts, pix_parts = [], [], []
    for t in (range(nt) if tiles is None else tiles):
        x, y = _tile_pixels(t, W, H, dt)
        if x.numel() == 0:
            continue
        a, b = ranges[t].tolist()
        gids = pl[a:b]
        pix = y * W + x
        if b == a:
            o = dict(C=torch.zeros(x.numel(), 3, dtype=dt), D=torch.zeros(x.numel(), dtype=dt),
                     A=torch.zeros(x.numel(), dtype=dt), N=torch.zeros(x.numel(), 3, dtype=dt),
                     med=torch.zeros(x.numel(), dtype=dt), dist=torch.zeros(x.numel(), dtype=dt),
                     T=torch.ones(x.numel(), dtype=dt), last=torch.zeros(x.numel(), dtype=torch.long),
                     med_idx=torch.full((x.numel(),), -1))
            pr = None
        else:
            o, pr = _eval_tile(pre["T"][gids], pre["mu"][gids], op[gids].reshape(-1), col[gids], pre["nc"][gids], x, y)
        img_parts.append(o["C"].T + o["T"][None, :] * bgd[:, None])
        all_parts.append(torch.stack([o["D"], o["A"], o["N"][:, 0], o["N"][:, 1], o["N"][:, 2], o["med"], o["dist"]]))
        pix_parts.append(pix)
        fT[pix] = o["T"].detach()
        last[pix] = o["last"]
        medi[pix] = o["med_idx"]
        if keep_pairs and pr is not None:
            pairs[t] = (gids, pix, pr)
    if pix_parts:
        pix = torch.cat(pix_parts)
        img = torch.zeros(3, H * W, dtype=dt).index_copy(1, pix, torch.cat(img_parts, 1))
        allm = torch.zeros(7, H * W, dtype=dt).index_copy(1, pix, torch.cat(all_parts, 1))
    return dict(image=img.view(3, H, W), allmap=allm.view(7, H, W), final_T=fT.view(H, W), last=last.view(H, W),
                median=medi.view(H, W), pairs=pairs)


def _near(v32, v64, thr, rel=1e-5):
    """Decision `v >= thr` (or `<=`) that float32 cannot settle: the two precisions disagree, or the fp64 value lies
    within four times their distance (plus a relative 1e-5 of the threshold) of it."""
    d = (v32.double() - v64).abs()
    return ((v32.double() >= thr) != (v64 >= thr)) | ((v64 - thr).abs() <= 4.0 * d + rel * abs(thr))


def undecidable(r32, r64, W, H):
    """Flag [H*W] bool: pixels in which a pair's decision lies within float32 rounding of its threshold; flag_g [P]
    Gaussians that have a pair in a flagged pixel.  Needs renders made with keep_pairs=True."""
    flag = torch.zeros(H * W, dtype=torch.bool)
    for t, (gids, pix, p64) in r64["pairs"].items():
        p32 = r32["pairs"][t][2]
        live = (p64["valid"] | p32["valid"])
        bad = torch.zeros_like(live)
        bad |= live & _near(p32["a_raw"], p64["a_raw"], ALPHA_MIN)
        bad |= live & _near(p32["a_raw"], p64["a_raw"], ALPHA_MAX)
        bad |= live & _near(p32["depth"], p64["depth"], NEAR_Z)
        bad |= (p64["valid"] | p32["valid"]) & _near(p32["rho3"] - p32["rho2"], p64["rho3"] - p64["rho2"], 0.0,
                                                     rel=0.0) & \
            ((p64["rho3"] - p64["rho2"]).abs() <= 1e-4 * (p64["rho3"].abs() + p64["rho2"].abs()) + 1e-12)
        bad |= p64["inc"] & _near(p32["Tb"], p64["Tb"], 0.5)
        bad |= live & _near(p32["test"], p64["test"], T_EPS)
        bad |= p64["inc"] != p32["inc"]
        flag[pix] |= bad.any(0)
    return flag


def flagged_gaussians(r64, flag, P):
    """Gaussians with an included (fp64) pair in a flagged pixel."""
    fg = torch.zeros(P, dtype=torch.bool)
    for t, (gids, pix, p64) in r64["pairs"].items():
        f = flag[pix]
        hit = (p64["valid"] & f[None, :]).any(1)
        fg[gids[hit]] = True
    return fg


def full(sc, dtype, scale_modifier=1.0, keep_pairs=False, tiles=None, requires_grad=False):
    """Preprocess + lists (pinned by the fp32 preprocess) + render in `dtype`.  sc: scene dict of float64 CPU tensors
    (means, scales [P,2], rot, op, col, bg, cam, W, H)."""
    W, H = sc["W"], sc["H"]
    cam = sc["cam"]
    pre32 = preprocess(sc["means"].float(), sc["scales"].float(), sc["rot"].float(), sc["op"].float(),
                       cam["viewmatrix"].float(), cam["projmatrix"].float(), W, H, scale_modifier)
    pl, ranges = build_lists(pre32, W, H)
    leaves = {k: sc[k].to(dtype).clone().requires_grad_(requires_grad) for k in ("means", "scales", "rot", "op", "col")}
    if dtype == torch.float32:
        pre = pre32 if not requires_grad else preprocess(leaves["means"], leaves["scales"], leaves["rot"], leaves["op"],
                                                         cam["viewmatrix"].float(), cam["projmatrix"].float(), W, H,
                                                         scale_modifier)
    else:
        pre = preprocess(leaves["means"], leaves["scales"], leaves["rot"], leaves["op"], cam["viewmatrix"].to(dtype),
                         cam["projmatrix"].to(dtype), W, H, scale_modifier)
    r = render(pre, leaves["col"], leaves["op"], pl, ranges, sc["bg"], W, H, keep_pairs=keep_pairs, tiles=tiles)
    r.update(pre32=pre32, pre=pre, point_list=pl, ranges=ranges, leaves=leaves)
    return r


def make_scene(P, W, H, seed=0, smin=0.02, smax=0.6, edge_frac=0.15, straddle_frac=0.05, faint_frac=0.05, zmax=9.0):
    """Seeded 2DGS scene: tests/scenes.py's Gaussians with two scale columns, plus near-edge-on splats (normal almost
    perpendicular to the viewing ray), splats straddling z = 0.2 and opacities below 1/255."""
    from tests import scenes

    sc = scenes.make_scene(P, W, H, seed=seed, smin=smin, smax=smax, surfel=False, zmax=zmax)
    g = torch.Generator().manual_seed(seed + 1000)
    sc["scales"] = sc["scales"][:, :2].contiguous()
    ne = int(edge_frac * P)
    if ne:
        # rotate the splat so that its normal R[:,2] is perpendicular (within a small angle) to the ray through its
        # centre: quaternion of the rotation taking e_z to a vector orthogonal to the view direction
        T_wc = torch.linalg.inv(sc["cam"]["viewmatrix"].T.double())
        cpos = T_wc[:3, 3]
        ray = torch.nn.functional.normalize(sc["means"][:ne] - cpos, dim=1)
        rnd = torch.randn(ne, 3, generator=g, dtype=torch.float64)
        perp = torch.nn.functional.normalize(rnd - (rnd * ray).sum(1, keepdim=True) * ray, dim=1)
        tilt = (torch.rand(ne, 1, generator=g, dtype=torch.float64) - 0.5) * 0.2
        nrm = torch.nn.functional.normalize(perp + tilt * ray, dim=1)
        ez = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand_as(nrm)
        axis = torch.cross(ez, nrm, dim=1)
        s = axis.norm(dim=1, keepdim=True).clamp_min(1e-12)
        c = (ez * nrm).sum(1, keepdim=True)
        half = torch.atan2(s, c) * 0.5
        sc["rot"][:ne] = torch.cat([torch.cos(half), torch.sin(half) * axis / s], 1)
    ns = int(straddle_frac * P)
    if ns:
        T_cw = sc["cam"]["viewmatrix"].T.double()
        pc = sc["means"][ne:ne + ns] @ T_cw[:3, :3].T + T_cw[:3, 3]
        pc[:, 2] = 0.2 + (torch.rand(ns, generator=g, dtype=torch.float64) - 0.5) * 0.3
        pc[:, 0] *= pc[:, 2] / 5.0
        pc[:, 1] *= pc[:, 2] / 5.0
        T_wc = torch.linalg.inv(T_cw)
        sc["means"][ne:ne + ns] = pc @ T_wc[:3, :3].T + T_wc[:3, 3]
    nf = int(faint_frac * P)
    if nf:
        sc["op"][P - nf:] = torch.rand(nf, 1, generator=g, dtype=torch.float64) * (1.5 / 255.0)
    return sc
