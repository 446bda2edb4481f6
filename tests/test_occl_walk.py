"""occl_budget_kernel deals the (rank, tile) pairs of a workgroup's 256 depth ranks densely to its 256 threads
(csrc/raster_fwd.hip); PINGS_OCC_WALK=l keeps the earlier dealing, one rank per lane (walk_rects).  Both visit the same
pairs with the same arithmetic and add with integer atomics, so the budget table must be the same words.

The frames: isotropic opaque (0.95) Gaussians at strictly ascending depths, so that Gaussian i has depth rank i, on an
image of 65 x 10 and of 130 x 10 tiles.  The pixel sigmas are chosen so that the inner rectangles (half-width about
1.92 sigma; a tile counts if its 15 x 15 pixel square lies inside) cover every case of the dealing; the test counts the
inner tiles itself, from the margin rule of preprocess_kernel restated in float64 on the fp32 inputs, and asserts the
cases on those counts.

Two paddings, because strided_rank deals the first quarter of the ranks round-robin over the waves (every wave holds
rank `wave`), so one frame cannot have both a wave with several visible ranks and a workgroup with none:
  * "dense": 64 culled Gaussians behind the 1,024 visible ones — five workgroups, up to 256 visible ranks each; the
    rectangles of workgroups 0, 1, 2 (a few of 8..64 tiles, then 1-tile ones) are tuned until their pair totals are
    256 k - 1, 256 k, 256 k + 1;
  * "sparse": 65,024 culled Gaussians — 258 workgroups, ranks 4 b .. 4 b + 3 in workgroup b, every workgroup from
    256 on without a pair; workgroups 10, 11, 12 hold four rectangles that add up to 257, 256 and 255 pairs."""
import numpy as np
import pytest
import torch

from oracle import raster_cpu as R
from scenes import hip_settings, make_scene, oracle_settings
from test_raster import _check_list_prefixes

SIZES = {65: (1040, 160), 130: (2080, 160)}     # gx -> (W, H): 10 tile rows
N_VALID = 1024
PADS = {"dense": 64, "sparse": 65024}
OCC_AMIN = 0.15                                  # RasterKnobs::occ_amin
Z0, DZ = 1.0, 0.0005


def _scene(W, H, surfel, u, v, sig, n_culled):
    """Gaussian i < len(u): centre at pixel (u, v), pixel sigma `sig`, depth Z0 + i DZ; then `n_culled` behind the camera."""
    nv, n = len(u), len(u) + n_culled
    sc = make_scene(n, W, H, seed=5, surfel=surfel, behind_frac=0.0)
    fx, cx, cy = 0.9 * W, 0.5 * W - 1.7, 0.5 * H + 0.9     # make_scene's camera
    uu, vv, ss = (torch.cat([torch.as_tensor(a, dtype=torch.float64), torch.full((n_culled,), c, dtype=torch.float64)])
                  for a, c in ((u, 0.5 * W), (v, 0.5 * H), (sig, 2.0)))
    z = Z0 + DZ * torch.arange(n, dtype=torch.float64)
    z[nv:] = -1.0 - z[nv:]
    pc = torch.stack([(uu - cx) / fx * z, (vv - cy) / fx * z, z], 1)
    V = sc["cam"]["viewmatrix"].to(torch.float64)           # X_c = X_w @ V[:3,:3] + V[3,:3]
    sc["means"] = (pc - V[3, :3]) @ torch.linalg.inv(V[:3, :3])
    s = (ss * z.abs() / fx)[:, None].expand(-1, 3).clone()
    if surfel:
        s[:, 2] = 1e-7
    sc["scales"] = s
    sc["rot"][:] = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64)
    sc["op"][:] = 0.95
    return sc


def _inner(sc, mode):
    """Inner rectangle of every Gaussian: preprocess_kernel's margin rule in float64 on the fp32-rounded inputs.
    Returns (tiles, cut, valid): `cut` = the rectangle ends at the image edge although the alpha >= occ_amin box goes on."""
    so = oracle_settings(sc, torch.float64, mode, False)
    f = lambda k: sc[k].to(torch.float32).to(torch.float64)
    g = R.preprocess(f("means"), f("scales"), f("rot"), so, opacities=f("op"))
    W, H = sc["W"], sc["H"]
    gx, gy = (W + 15) // 16, (H + 15) // 16
    valid = g["valid"].numpy()
    cx, cy, cz = (g[k].numpy() for k in ("conic_x", "conic_y", "conic_z"))
    det_c = cx * cz - cy * cy
    with np.errstate(all="ignore"):
        cxx, cyy = cz / det_c, cx / det_c
        det = 1.0 / det_c
        mid = 0.5 * (cxx + cyy)
        lam_min = mid - np.sqrt(np.maximum(mid * mid - det, 0.0))
        thr = 2.0 * np.log(f("op").reshape(-1).numpy() / OCC_AMIN)
        ex, ey = np.sqrt(thr * cxx), np.sqrt(thr * cyy)
        mx, my = g["mx"].numpy(), g["my"].numpy()
        xmin, xmax, ymin, ymax = (g[k].numpy() for k in ("xmin", "xmax", "ymin", "ymax"))
        fx0, fx1 = np.ceil((mx - ex) / 16 - 0.02), np.floor((mx + ex - 15.0) / 16 + 0.02) + 1
        fy0, fy1 = np.ceil((my - ey) / 16 - 0.02), np.floor((my + ey - 15.0) / 16 + 0.02) + 1
    ok = valid & (thr * lam_min >= 50.0)
    z = lambda a: np.where(ok, a, 0).astype(np.int64)
    ix0, ix1 = np.maximum(xmin, z(fx0)), np.minimum(xmax, z(fx1))
    iy0, iy1 = np.maximum(ymin, z(fy0)), np.minimum(ymax, z(fy1))
    tiles = np.where(ok & (ix1 > ix0) & (iy1 > iy0), (ix1 - ix0) * (iy1 - iy0), 0)
    cut = (tiles > 0) & ((z(fx0) < 0) | (z(fx1) > gx) | (z(fy0) < 0) | (z(fy1) > gy))
    return tiles, cut, valid


def _rank_workgroups(P):
    """Workgroup and wave of every depth rank: strided_rank of csrc/raster_fwd.hip."""
    nw = 4 * ((P + 255) // 256)
    wave, lane = np.divmod(np.arange(64 * nw), 64)
    r = np.where(lane < 16, lane * nw + wave, ((lane >> 4) * nw + wave) * 16 + (lane & 15))
    wave_of = np.full(64 * nw, -1)
    wave_of[r] = wave
    assert (wave_of >= 0).all()
    return wave_of[:P] // 4, wave_of[:P]


def _build(gx, mode, pad):
    W, H = SIZES[gx]
    surfel = mode == "surfel"
    g = torch.Generator().manual_seed(100 + gx)
    rnd = lambda k: torch.rand(k, generator=g, dtype=torch.float64).numpy()
    # candidates: centres anywhere in and a little around the image, sigmas 6..60 px and a few of 150..300 px, with the host's inner-tile counts
    n_pool = 6000
    pu, pv = (1.1 * rnd(n_pool) - 0.05) * W, (1.6 * rnd(n_pool) - 0.3) * H
    ps = np.where(np.arange(n_pool) % 20 == 0, 150.0 + 150.0 * rnd(n_pool), 6.0 + 54.0 * rnd(n_pool))
    pt, pcut, pvalid = _inner(_scene(W, H, surfel, pu, pv, ps, 0), mode)
    used = ~pvalid            # a candidate that touches no tile would be culled: it takes no depth rank

    def pick(cond):
        i = int(np.nonzero(cond & ~used)[0][0])
        used[i] = True
        return pu[i], pv[i], ps[i]

    # everything starts as a small Gaussian without an inner tile; the first 200 are the sweep as it comes
    u, v, s = rnd(N_VALID) * W, rnd(N_VALID) * H, 2.0 + rnd(N_VALID)
    sweep = np.nonzero(pvalid)[0][:200]
    u[:200], v[:200], s[:200] = pu[sweep], pv[sweep], ps[sweep]
    used[sweep] = True
    wanted = [pt == 1, pt == 8, pt == 9, pt == 63, pt == 64, pt == 65, pt > 256, pt > 512, pcut & (pt > 0)]
    for j, cond in enumerate(wanted):
        u[200 + 7 * j], v[200 + 7 * j], s[200 + 7 * j] = pick(cond)
    P = N_VALID + PADS[pad]
    wg, wave = _rank_workgroups(P)
    if pad == "sparse":
        assert all(set(np.nonzero(wg[:N_VALID] == b)[0]) == set(range(4 * b, 4 * b + 4)) for b in (10, 11, 12))
        # four rectangles that add up to 257, 256, 255 pairs: two pairs of counts the pool still holds twelve times
        vals = [int(n) for n in np.unique(pt) if ((pt == n) & ~used).sum() >= 12]
        pairs = {a + c: (a, c) for a in vals for c in vals if a >= c}
        for b, want in ((10, 257), (11, 256), (12, 255)):
            s1 = max(x for x in pairs if want - x in pairs)
            for j, n in enumerate(pairs[s1] + pairs[want - s1]):
                u[4 * b + j], v[4 * b + j], s[4 * b + j] = pick(pt == n)
    else:
        # workgroups 0, 1, 2: turn Gaussians without a tile into 1-tile ones until the total is 256 k + (-1, 0, 1)
        tiles, _, _ = _inner(_scene(W, H, surfel, u, v, s, PADS[pad]), mode)
        for b, want in ((0, 255), (1, 0), (2, 1)):
            mine = np.nonzero(wg[:N_VALID] == b)[0]
            need = (want - int(tiles[mine].sum())) % 256
            zeros = list(mine[tiles[mine] == 0])
            while need > 12:          # candidates of 8..64 tiles first: a workgroup has fewer than 255 spare Gaussians
                i = zeros.pop()
                j = int(np.nonzero(~used & (pt >= 8) & (pt <= min(need, 64)))[0][0])
                u[i], v[i], s[i] = pick(np.arange(n_pool) == j)
                need -= int(pt[j])
            for i in zeros[:need]:    # sigma 8 px at the centre of a tile: that tile and no other
                tx, ty = min(max(int(u[i] / 16), 0), gx - 1), min(max(int(v[i] / 16), 0), 9)
                u[i], v[i], s[i] = 16.0 * tx + 7.5, 16.0 * ty + 7.5, 8.0
    sc = _scene(W, H, surfel, u, v, s, PADS[pad])
    tiles, cut, valid = _inner(sc, mode)
    assert valid[:N_VALID].all() and not valid[N_VALID:].any()     # Gaussian i has depth rank i; nvalid = N_VALID
    return sc, tiles, cut, wg, wave


def _assert_coverage(tiles, cut, wg, wave, pad):
    t = tiles[:N_VALID]
    for n in (0, 1, 8, 9, 63, 64, 65):
        assert (t == n).any(), n
    assert ((t >= 60) & (t <= 70)).sum() >= 3 and ((t >= 2) & (t <= 12)).sum() >= 3
    assert (t > 256).sum() >= 2 and (t > 512).any()             # two and three trips of a thread in one rectangle
    assert (cut & (tiles > 0)).any()
    n_wg = int(wg.max()) + 1
    totals = np.bincount(wg[:N_VALID], weights=t, minlength=n_wg).astype(np.int64)
    visible = np.bincount(wg[:N_VALID], minlength=n_wg)
    per_wave = np.bincount(wave[:N_VALID], weights=(t > 0), minlength=4 * n_wg)
    res = {int(x) for x in totals[totals > 0] % 256}
    assert {255, 0, 1} <= res, sorted(res)
    assert (totals[totals > 0] > 256).any()
    if pad == "sparse":
        assert (visible == 0).sum() >= 1 and per_wave.max() == 1  # workgroups wholly behind nvalid
    else:
        assert per_wave.max() >= 8 and (totals > 0).sum() >= 4    # several rectangles per wave, several workgroups
    return totals


def _run(sc, mode, monkeypatch, walk):
    from pings_amd import rasterizer as hr

    monkeypatch.delenv("PINGS_RASTER_OCCLUSION", raising=False)
    if walk:
        monkeypatch.setenv("PINGS_OCC_WALK", walk)
    else:
        monkeypatch.delenv("PINGS_OCC_WALK", raising=False)
    hs = hip_settings(sc, mode, False, 1.0)
    rast = (hr.SurfelGaussianRasterizer if mode == "surfel" else hr.GS3DGaussianRasterizer)(hs)
    leaves = [sc[k].to(torch.float32).cuda().contiguous().requires_grad_(True)
              for k in ("means", "col", "op", "scales", "rot")]
    th = torch.zeros(3, device="cuda", requires_grad=True)
    rh = torch.zeros(3, device="cuda", requires_grad=True)
    out = rast(means3D=leaves[0], means2D=torch.zeros_like(leaves[0]), colors_precomp=leaves[1],
               opacities=leaves[2], scales=leaves[3], rotations=leaves[4], theta=th, rho=rh)
    imgs = [t for t in out if t.is_floating_point() and t.dim() == 3]
    gg = torch.Generator(device="cuda").manual_seed(9)
    torch.autograd.backward(imgs, [torch.randn(t.shape, generator=gg, device="cuda") for t in imgs])
    fs, radii, per_g = hr._forward(rast._prepared(), *[t.detach() for t in leaves])
    pl, rg, _, nc = hr.debug_lists(fs)
    bucket, bsat, nb = hr.debug_occlusion(fs)
    return dict(out=list(out) + [radii, per_g, nc], grads=[t.grad for t in leaves] + [th.grad, rh.grad], I=int(fs.I),
                pl=pl, rg=rg, nc=nc, bucket=bucket, bsat=bsat, nb=nb)


@pytest.mark.gpu
@pytest.mark.parametrize("pad", sorted(PADS))
@pytest.mark.parametrize("gx", sorted(SIZES))
@pytest.mark.parametrize("mode", ["surfel", "3dgs"])
def test_dense_walk_gives_the_lane_walks_budget_bit_for_bit(mode, gx, pad, monkeypatch):
    W, H = SIZES[gx]
    assert (W + 15) // 16 == gx and (H + 15) // 16 == 10
    sc, tiles, cut, wg, wave = _build(gx, mode, pad)
    totals = _assert_coverage(tiles, cut, wg, wave, pad)
    dense = _run(sc, mode, monkeypatch, None)
    lanes = _run(sc, mode, monkeypatch, "l")
    again = _run(sc, mode, monkeypatch, None)
    nt = gx * 10
    sat = dense["bsat"] != 0xFFFF
    print(f"{mode} gx={gx} {pad}: {int(tiles.sum())} inner pairs, largest workgroup {int(totals.max())}, "
          f"{int((dense['bucket'] != 0).sum())} budget words set, {int(sat.sum())} of {nt} tiles saturate, "
          f"instances {dense['I']}")
    assert dense["nb"] == lanes["nb"] == 256 and dense["bucket"].shape == (256, nt) and dense["bsat"].shape == (nt,)
    assert bool((dense["bucket"] != 0).any()) and bool(sat.any())     # or the comparison says nothing
    for other in (lanes, again):
        assert torch.equal(dense["bucket"], other["bucket"]) and torch.equal(dense["bsat"], other["bsat"])
        assert dense["I"] == other["I"]
        assert torch.equal(dense["pl"], other["pl"]) and torch.equal(dense["rg"], other["rg"])
        assert len(dense["out"]) == len(other["out"]) and len(dense["out"]) >= 7
        for x, y in zip(dense["out"] + dense["grads"], other["out"] + other["grads"]):
            assert x.shape == y.shape and torch.equal(x, y)
    assert float(dense["out"][0].detach().abs().sum()) > 0 and all(bool(torch.isfinite(t).all()) for t in dense["grads"])
    so = oracle_settings(sc, torch.float32, mode, False)
    f = lambda k: sc[k].to(torch.float32)
    geom = R.preprocess(f("means"), f("scales"), f("rot"), so, opacities=f("op"))
    pl, rg = R.bin_and_sort(geom, so)
    _check_list_prefixes(dense["pl"], dense["rg"], dense["nc"], dict(point_list=pl, ranges=rg), W, H)
    assert 0 < dense["I"] == len(dense["pl"]) < len(pl)
