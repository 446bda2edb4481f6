"""Binning from per-bucket tile bitmasks (csrc/raster_fwd.hip: occl_scan_kernel's epilogue, count_kept_kernel,
duplicate_kernel): the kept tiles of a rectangle row are a bit range of the rank bucket's mask over tile ids.

The image widths put that bit range on every word-boundary case of the 64-bit mask words: one tile per row (gx = 1),
rows inside one word (4), rows one short of a word, exactly a word and one over (63, 64, 65), rows of two words
(120, the 1080p width) and of three (130).  The heights give one tile row (16) and last rows of partial tiles.

One scene for both modes: sixteen opaque screen-filling Gaussians in front, centred over the left quarter of the image,
so that the tiles near them saturate and the far ones do not; behind them eight thousand small ones, some of which
end at the last tile column or row.  The sixteen are the nearest ranks, all of rank bucket 0 (8016 ranks over 256
buckets), which no tile ever drops: they own the same instances with the occlusion bound on and off.  The small ones
cover at most 4 x 4 tiles (asserted).  A Gaussian's contribution is the sum of its per-instance weights, added
serially up to 16 instances and by a wave above (test_raster.py::test_occlusion_culling_changes_no_output_bit):
with the same instance count in both runs, or at most 16 in both, the culled instances only add zeros in the same
order, and the contributions are bit-identical like everything else."""
import numpy as np
import pytest
import torch

from oracle import raster_cpu as R
from scenes import hip_settings, make_scene, oracle_settings
from test_raster import _check_list_prefixes

N_BIG, N_SMALL, N_EDGE = 16, 8000, 16
# gx -> (W, H)
SIZES = {1: (16, 80), 4: (64, 16), 63: (1008, 40), 64: (1024, 72), 65: (1040, 16), 120: (1920, 80), 130: (2080, 56)}


def _scene(W, H, surfel):
    sc = make_scene(N_BIG + N_SMALL, W, H, seed=5, surfel=surfel, behind_frac=0.0)
    g = torch.Generator().manual_seed(11)
    rnd = lambda n: torch.rand(n, generator=g, dtype=torch.float64)
    fx, cx, cy = 0.9 * W, 0.5 * W - 1.7, 0.5 * H + 0.9     # make_scene's camera
    # pixel centre, depth and pixel sigma of every Gaussian; world scale = sigma z / fx
    u, v = rnd(N_BIG + N_SMALL) * W, rnd(N_BIG + N_SMALL) * H
    z = 3.0 + 6.0 * rnd(N_BIG + N_SMALL)
    sig = 1.5 + 4.0 * rnd(N_BIG + N_SMALL)
    # the front: centres around (W / 4, H / 2), half a tile of jitter so that they do not share a centre tile
    u[:N_BIG] = 0.25 * W + 16.0 * (rnd(N_BIG) - 0.5)
    v[:N_BIG] = 0.5 * H + 16.0 * (rnd(N_BIG) - 0.5)
    z[:N_BIG] = 1.0 + 0.005 * torch.arange(N_BIG, dtype=torch.float64)
    sig[:N_BIG] = 0.3 * W + 40.0
    # small ones whose rectangle ends at the last tile column / the last tile row
    e = N_BIG + N_EDGE // 2
    u[N_BIG:e] = W - 1.0 - 3.0 * rnd(N_EDGE // 2)
    v[e:e + N_EDGE // 2] = H - 1.0 - 3.0 * rnd(N_EDGE // 2)
    pc = torch.stack([(u - cx) / fx * z, (v - cy) / fx * z, z], 1)
    V = sc["cam"]["viewmatrix"].to(torch.float64)           # X_c = X_w @ V[:3,:3] + V[3,:3]
    sc["means"] = (pc - V[3, :3]) @ torch.linalg.inv(V[:3, :3])
    s = (sig * z / fx)[:, None].expand(-1, 3).clone()
    if surfel:
        s[:, 2] = 1e-7
    sc["scales"] = s
    sc["rot"][:N_BIG] = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64)   # facing the (nearly unrotated) camera
    sc["op"][:N_BIG] = 1.0
    return sc


def _oracle_lists(sc, mode):
    """fp32 oracle: rectangles -> tiles per Gaussian and the (tile, depth, index)-sorted unculled lists."""
    so = oracle_settings(sc, torch.float32, mode, False)
    f = lambda k: sc[k].to(torch.float32)
    geom = R.preprocess(f("means"), f("scales"), f("rot"), so, opacities=f("op"))
    pl, rg = R.bin_and_sort(geom, so)
    return geom, geom["tiles_touched"].numpy().astype(np.int64), dict(point_list=pl, ranges=rg)


@pytest.mark.gpu
@pytest.mark.parametrize("gx", sorted(SIZES))
@pytest.mark.parametrize("mode", ["surfel", "3dgs"])
def test_mask_row_walks_keep_every_bit_and_every_list(mode, gx, monkeypatch):
    from pings_amd import rasterizer as hr

    W, H = SIZES[gx]
    assert (W + 15) // 16 == gx
    sc = _scene(W, H, mode == "surfel")
    geom, tiles, o = _oracle_lists(sc, mode)
    assert tiles[N_BIG:].max() <= 16                                  # what the docstring's argument rests on
    gy = (H + 15) // 16
    # some small rectangle ends at the last tile column and some at the last tile row
    small = geom["valid"] & (torch.arange(N_BIG + N_SMALL) >= N_BIG)
    assert bool((geom["xmax"][small] == gx).any()) and bool((geom["ymax"][small] == gy).any())

    def run(flag):
        monkeypatch.setenv("PINGS_RASTER_OCCLUSION", flag)
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
        return list(out) + [radii, per_g], [t.grad for t in leaves] + [th.grad, rh.grad], int(fs.I), (pl, rg, nc)

    out1, g1, I1, (pl1, rg1, nc1) = run("1")
    out0, g0, I0, (pl0, rg0, nc0) = run("0")
    print(f"{mode} gx={gx} {W}x{H}: instances {I1} kept of {I0}, rectangles {int(tiles.sum())}")
    # images, depth, alpha, normal, radii, contributions and all gradients: the same bits
    assert len(out1) == len(out0) and len(out1) >= 5
    for a, b in zip(out1, out0):
        assert a.shape == b.shape and torch.equal(a, b)
    for a, b in zip(g1, g0):
        assert torch.equal(a, b)
    assert float(out1[0].abs().sum()) > 0 and all(bool(torch.isfinite(t).all()) for t in g1)
    # bound off: one instance per tile of every rectangle, in the oracle's order
    assert I0 == int(tiles.sum())
    assert np.array_equal(pl0.cpu().numpy(), o["point_list"])
    assert np.array_equal(rg0.cpu().numpy(), o["ranges"])
    # bound on: every kept list is a prefix of the full one and holds everything a pixel blended; fewer instances
    assert torch.equal(nc1, nc0)
    _check_list_prefixes(pl1, rg1, nc1, o, W, H)
    assert I1 == len(pl1) and I1 < I0, (I1, I0)
    # the front keeps all of its instances (rank bucket 0)
    per_g1 = np.bincount(pl1.cpu().numpy(), minlength=N_BIG)[:N_BIG]
    assert np.array_equal(per_g1, tiles[:N_BIG])
