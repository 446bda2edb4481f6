"""Tile lists gathered from the front depth ranks (csrc/raster_gather.hip) against the sort path of the same library.

The oracle of every GPU case is the same frame with PINGS_BIN=s: `ranges`, the raw slots of `point_list` and `gval`
must be the same words, and so must the images, radii, contributions and every gradient of one forward + backward.
`pings_raster_debug_bin_plan` tells which plan a render took, so every case also proves that the path it targets ran.

Frames.  `_front_scene`: large opaque Gaussians in front and small ones behind, some at exactly the depth of their
neighbour, as the two nearest of the front do (ties go by index), some ending at the last tile column / row.  On the wide images the front covers the
left half only: the tiles there saturate after a few ranks (their occ_bsat cuts the walk in the middle of the front),
the others keep every rank, so the front depth F is nearly the survivor count and many ranks inside it keep nothing.
With `big_sig` beyond the image size the front's rectangles are the whole image and every tile saturates.
`_flat_scene`: N small faint Gaussians inside the image, none of which adds to the occlusion budget, so that F = N
exactly: the F edges (1, 64, 65, the staging chunk +- 1, FRONT_MAX, FRONT_MAX + 1).

The slot formula (first slot of the rectangle row + kept tiles of the row to the left) is checked on the host first,
against the row-major walk, at grid widths on both sides of the 64-bit mask words.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from scenes import hip_settings, make_scene

FRONT_MAX, CHUNK = 8192, 2048          # csrc/raster_common.hpp
# gx -> (W, H): rectangle rows that start and end on both sides of a mask-word boundary; sizes off the 16-pixel grid
SIZES = {1: (13, 75), 4: (60, 20), 63: (1001, 40), 64: (1024, 40), 65: (1030, 16), 120: (1920, 44), 130: (2070, 56),
         256: (4090, 24)}


# ---------------------------------------------------------------- the slot formula, on the host
def _kept_bits(words, s, w):
    """csrc/raster_common.hpp: kept_bits, on Python integers."""
    i, sh = s >> 6, s & 63
    lo, hi = int(words[i]), int(words[i + 1])
    v = ((lo >> sh) | (hi << (64 - sh))) & (2 ** 64 - 1) if sh else lo
    return v & ((2 ** 64 - 1) >> (64 - w))


def _popcount_left(words, s, dx):
    return sum(bin(_kept_bits(words, s + x, min(64, dx - x))).count("1") for x in range(0, dx, 64))


@pytest.mark.parametrize("gx", [1, 4, 63, 64, 65, 120, 130, 256])
def test_slot_formula_is_the_row_major_walk(gx):
    rng = np.random.default_rng(gx)
    gy = 70 if gx <= 4 else 5
    nt = gx * gy
    nwords = (nt + 63) // 64
    for trial in range(40):
        bits = rng.random(nt) < rng.choice([0.1, 0.5, 0.9, 1.0])
        words = np.zeros(nwords + 1, dtype=np.uint64)              # + the spare word behind the table
        for t in np.flatnonzero(bits):
            words[t >> 6] |= np.uint64(1) << np.uint64(t & 63)
        words[nwords] = np.uint64(rng.integers(0, 2 ** 63))        # whatever lies there must not matter
        xmin, ymin = int(rng.integers(0, gx)), int(rng.integers(0, gy))
        wdt, hgt = int(rng.integers(1, gx - xmin + 1)), int(rng.integers(1, gy - ymin + 1))
        if trial == 0:
            xmin, ymin, wdt, hgt = 0, 0, gx, gy                    # the whole image
        first = int(rng.integers(0, 1000))
        # the walk of duplicate_kernel: rows top to bottom, x ascending, one slot per kept tile
        want, o = {}, first
        for y in range(ymin, ymin + hgt):
            for x in range(xmin, xmin + wdt):
                if bits[y * gx + x]:
                    want[(x, y)] = o
                    o += 1
        # front_rows_kernel's row table, then tile_gather_kernel's slot
        rowbase, run = [], first
        for y in range(ymin, ymin + hgt):
            rowbase.append(run)
            run += _popcount_left(words, y * gx + xmin, wdt)
        assert run == o
        for (x, y), slot in want.items():
            dx = x - xmin
            got = rowbase[y - ymin] + (_popcount_left(words, y * gx + x - dx, dx) if dx else 0)
            assert got == slot, (gx, trial, x, y)


# ---------------------------------------------------------------- frames
def _place(sc, u, v, z, sig, surfel):
    W, H = sc["W"], sc["H"]
    fx, cx, cy = 0.9 * W, 0.5 * W - 1.7, 0.5 * H + 0.9              # make_scene's camera
    pc = torch.stack([(u - cx) / fx * z, (v - cy) / fx * z, z], 1)
    V = sc["cam"]["viewmatrix"].to(torch.float64)                   # X_c = X_w @ V[:3,:3] + V[3,:3]
    sc["means"] = (pc - V[3, :3]) @ torch.linalg.inv(V[:3, :3])
    s = (sig * z / fx)[:, None].expand(-1, 3).clone()
    if surfel:
        s[:, 2] = 1e-7
    sc["scales"] = s
    sc["rot"][:] = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64)   # facing the (nearly unrotated) camera
    return sc


def _front_scene(W, H, n_big, n_small, surfel=True, seed=5, big_sig=None):
    n = n_big + n_small
    sc = make_scene(n, W, H, seed=seed, surfel=surfel, behind_frac=0.0)
    g = torch.Generator().manual_seed(seed + 6)
    rnd = lambda k: torch.rand(k, generator=g, dtype=torch.float64)
    u, v = rnd(n) * W, rnd(n) * H
    z = 3.0 + 6.0 * rnd(n)
    sig = 3.0 + 5.0 * rnd(n)
    # the front: centres around (W / 4, H / 2)
    u[:n_big] = 0.25 * W + 8.0 * (rnd(n_big) - 0.5)
    v[:n_big] = 0.5 * H + 8.0 * (rnd(n_big) - 0.5)
    z[:n_big] = 1.0 + 0.005 * torch.arange(n_big, dtype=torch.float64)
    sig[:n_big] = big_sig if big_sig is not None else 0.1 * W + 20.0
    e = n_big + 8
    u[n_big:e] = W - 1.0 - 3.0 * rnd(8)                             # ending at the last tile column
    v[e:e + 8] = H - 1.0 - 3.0 * rnd(8)                             # ... and row
    sc = _place(sc, u, v, z, sig, surfel)
    sc["op"][:n_big] = 1.0
    # equal depth keys inside the front: the two nearest Gaussians at one place
    sc["means"][1] = sc["means"][0]
    # equal depth keys: every fourth small Gaussian of the first thousand sits exactly where its neighbour does
    k = torch.arange(e + 16, min(e + 1016, n - 1), 4)
    sc["means"][k + 1] = sc["means"][k]
    return sc


def _flat_scene(W, H, n, surfel=True):
    sc = make_scene(n, W, H, seed=3, surfel=surfel, behind_frac=0.0)
    g = torch.Generator().manual_seed(17)
    rnd = lambda k: torch.rand(k, generator=g, dtype=torch.float64)
    u, v = 2.0 + rnd(n) * (W - 4.0), 2.0 + rnd(n) * (H - 4.0)
    if n == 1:
        u[0], v[0] = 16.0 * ((W // 16 + 1) // 2), 16.0          # on a tile corner: four tiles (two where gy = 1)
    sc = _place(sc, u, v, 3.0 + 6.0 * rnd(n), 2.5 + 1.5 * rnd(n), surfel)
    sc["op"][:] = (0.2 + 0.25 * rnd(n))[:, None]                    # below what the occlusion budget counts
    return sc


def _binning_field(fs, name):
    from test_raster_glue import _binning_field as field
    return field(fs, name)[:max(int(fs.I), 1)]


def _plan():
    from pings_amd import _lib
    plan, front = C.c_int32(-1), C.c_uint32(0)
    _lib.check(_lib.lib().pings_raster_debug_bin_plan(C.byref(plan), C.byref(front)), "pings_raster_debug_bin_plan")
    return plan.value, front.value


def _run(sc, mode, bin_knob, monkeypatch, env=None):
    """One forward + backward through the autograd function, then one forward whose blobs are read back."""
    from pings_amd import rasterizer as hr

    if bin_knob is None:
        monkeypatch.delenv("PINGS_BIN", raising=False)
    else:
        monkeypatch.setenv("PINGS_BIN", bin_knob)
    for k_, v_ in (env or {}).items():
        monkeypatch.setenv(k_, v_)
    rast = (hr.SurfelGaussianRasterizer if mode == "surfel" else hr.GS3DGaussianRasterizer)(hip_settings(sc, mode, False, 1.0))
    leaves = [sc[k].to(torch.float32).cuda().contiguous().requires_grad_(True) for k in ("means", "col", "op", "scales", "rot")]
    th = torch.zeros(3, device="cuda", requires_grad=True)
    rh = torch.zeros(3, device="cuda", requires_grad=True)
    out = rast(means3D=leaves[0], means2D=torch.zeros_like(leaves[0]), colors_precomp=leaves[1], opacities=leaves[2],
               scales=leaves[3], rotations=leaves[4], theta=th, rho=rh)
    imgs = [t for t in out if t.is_floating_point() and t.dim() == 3]
    gg = torch.Generator(device="cuda").manual_seed(9)
    torch.autograd.backward(imgs, [torch.randn(t.shape, generator=gg, device="cuda") for t in imgs])
    fs, radii, per_g = hr._forward(rast._prepared(), *[t.detach() for t in leaves])
    plan, front = _plan()
    ids, rg, _, nc = hr.debug_lists(fs)
    _, bsat, nb = hr.debug_occlusion(fs)
    bsat = bsat.cpu()
    for k_ in (env or {}):
        monkeypatch.delenv(k_)
    return dict(out=[t.detach() for t in out] + [radii, per_g], grads=[t.grad for t in leaves] + [th.grad, rh.grad],
                I=int(fs.I), plan=plan, front=front, ranges=rg.cpu(), slots=_binning_field(fs, "point_list"),
                gval=_binning_field(fs, "gval"), bsat=bsat, fclass=fs.fclass, ids=ids.cpu(), nb=nb,
                nvalid=int((radii > 0).sum()))


def _assert_same(a, b, what):
    assert a["I"] == b["I"] and a["I"] > 0, what
    assert torch.equal(a["ranges"], b["ranges"]), (what, "ranges")
    assert torch.equal(a["slots"], b["slots"]), (what, "point_list slots")
    assert torch.equal(a["gval"], b["gval"]), (what, "gval")
    assert len(a["out"]) == len(b["out"]) >= 5
    for i, (x, y) in enumerate(zip(a["out"], b["out"])):
        assert x.shape == y.shape and torch.equal(x, y), (what, "output", i)
    for i, (x, y) in enumerate(zip(a["grads"], b["grads"])):
        assert torch.equal(x, y), (what, "gradient", i)
    assert float(a["out"][0].abs().sum()) > 0 and all(bool(torch.isfinite(t).all()) for t in a["grads"])
    # the slots are a permutation of 0 .. I - 1, and every range lies inside the list
    assert torch.equal(a["slots"].to(torch.int64).sort().values, torch.arange(a["I"]))
    assert int(a["ranges"].max()) == a["I"]


@pytest.mark.gpu
@pytest.mark.parametrize("gx", sorted(SIZES))
def test_gathered_lists_are_the_sorted_lists_at_the_mask_word_edges(gx, monkeypatch):
    W, H = SIZES[gx]
    assert (W + 15) // 16 == gx
    # narrow images: the front over the whole image (few ranks, every tile saturates); wide ones: over the left half
    sc = _front_scene(W, H, 16, 6000, big_sig=max(W, H) + 40.0 if gx < 63 else None)
    s = _run(sc, "surfel", "s", monkeypatch)
    g = _run(sc, "surfel", "g", monkeypatch)
    print(f"gx={gx} {W}x{H}: I {g['I']}, F {g['front']}, class {g['fclass']}")
    assert s["plan"] == 0 and s["front"] == 0xFFFFFFFF and g["plan"] == 1     # nobody looks for F of a frame that sorts
    # ties by index: Gaussians 0 and 1 lie at one depth, inside the front, and both keep tiles of the gathered frame;
    # lists that hold both hold 0 right before 1 (the order itself is the sort path's, compared below)
    ids = g["ids"]
    assert bool((ids == 0).any()) and bool((ids == 1).any()) and bool((ids[1:][ids[:-1] == 0] == 1).any())
    _assert_same(g, s, f"gx={gx}")
    # a tile whose last needed bucket cuts the walk inside the front, and ranks inside the front that keep nothing
    assert bool((g["bsat"] < 0xFFFF).any())
    if gx >= 63:
        lens = g["ranges"][:, 1] - g["ranges"][:, 0]
        assert bool((g["bsat"] == 0xFFFF).any()) and g["front"] > CHUNK
        # a tile whose last needed bucket ends inside the front, and not on a 64-rank step of the walk
        from pings_amd import _lib
        ranks = np.arange(g["front"], dtype=np.int32)
        bk = np.zeros(g["front"], dtype=np.uint32)
        _lib.check(_lib.lib().pings_raster_rank_bucket(ranks.ctypes.data_as(C.c_void_p), len(ranks), g["nb"], g["nvalid"],
                                                              bk.ctypes.data_as(C.c_void_p)),
                   "pings_raster_rank_bucket")
        sat = g["bsat"].numpy()
        cut = np.searchsorted(bk, sat[sat < 0xFFFF], side="right")        # first rank behind the tile's last bucket
        assert bool(((cut < g["front"]) & (cut % 64 != 0)).any())
        assert int(g["gval"].unique().numel()) < g["front"] and int(lens.max()) > int(lens[lens > 0].min())


@pytest.mark.gpu
def test_more_than_64_tile_rows_and_an_uncovered_tile(monkeypatch):
    """68 tile rows (the 1080p height), the front's rectangles cover all of them (the row loop of front_rows_kernel
    runs twice).  Then a few Gaussians on a wide image: a tile nobody covers keeps the zeros of the clear, and the tiles
    behind it start where the sort puts them."""
    W, H = 40, 1085
    sc = _front_scene(W, H, 12, 1500, big_sig=max(W, H) + 40.0)
    s = _run(sc, "surfel", "s", monkeypatch)
    g = _run(sc, "surfel", "g", monkeypatch)
    assert (H + 15) // 16 == 68 and s["plan"] == 0 and g["plan"] == 1
    _assert_same(g, s, "68 rows")
    sc = _flat_scene(640, 48, 40)
    s = _run(sc, "surfel", "s", monkeypatch)
    g = _run(sc, "surfel", "g", monkeypatch)
    assert s["plan"] == 0 and g["plan"] == 1 and g["front"] == 40
    _assert_same(g, s, "sparse")
    lens = g["ranges"][:, 1] - g["ranges"][:, 0]
    empty = (lens == 0).nonzero().flatten()
    assert 0 < empty.numel() < lens.numel() and bool((g["ranges"][empty] == 0).all())
    assert int(empty.min()) < int((lens > 0).nonzero().max())      # an empty tile in front of a non-empty one


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, FRONT_MAX, FRONT_MAX + 1])
def test_front_depth_edges(n, monkeypatch):
    """F = n exactly.  Up to FRONT_MAX the forced plan gathers; one more and both the default and PINGS_BIN=g sort."""
    sc = _flat_scene(128, 32, n)
    s = _run(sc, "surfel", "s", monkeypatch)
    g = _run(sc, "surfel", "g", monkeypatch)
    d = _run(sc, "surfel", None, monkeypatch)
    print(f"n={n}: I {g['I']}, F {g['front']}, class {d['fclass']}, default plan {d['plan']}")
    assert g["front"] == n and s["plan"] == 0
    assert g["plan"] == (1 if n <= FRONT_MAX else 0)
    if n > FRONT_MAX:
        assert d["plan"] == 0
    _assert_same(g, s, f"F={n} forced")
    _assert_same(d, s, f"F={n} default")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["surfel", "3dgs"])
def test_default_plan_gathers_a_saturated_class_2_frame(mode, monkeypatch):
    """Every tile saturates behind a front of large footprints: footprint class 2, a front of a few dozen ranks, and the
    default rule takes the gather plan on its own."""
    sc = _front_scene(200, 150, 48, 150, surfel=mode == "surfel", big_sig=240.0)
    s = _run(sc, mode, "s", monkeypatch)
    d = _run(sc, mode, None, monkeypatch)
    print(f"{mode}: I {d['I']}, F {d['front']}, class {d['fclass']}")
    assert d["fclass"] == 2 and d["plan"] == 1 and s["plan"] == 0
    _assert_same(d, s, mode)


@pytest.mark.gpu
def test_occlusion_off_sorts(monkeypatch):
    """With the bound off every survivor keeps its tiles: F is the survivor count, beyond FRONT_MAX here."""
    sc = _front_scene(320, 64, 16, 9000)
    env = {"PINGS_RASTER_OCCLUSION": "0"}
    s = _run(sc, "surfel", "s", monkeypatch, env)
    g = _run(sc, "surfel", "g", monkeypatch, env)
    d = _run(sc, "surfel", None, monkeypatch, env)
    assert g["front"] > FRONT_MAX and g["plan"] == 0 and d["plan"] == 0
    _assert_same(g, s, "occlusion off, forced")
    _assert_same(d, s, "occlusion off, default")


@pytest.mark.gpu
def test_a_render_of_another_blob_than_the_last_geometry_call_sorts(monkeypatch):
    """Geometry of frame A, geometry of frame B into another blob, then the render of A: the thread's record is B's, so
    A is sorted, and its outputs are those of an undisturbed forward of A."""
    from pings_amd import _lib, rasterizer as hr

    monkeypatch.setenv("PINGS_BIN", "g")
    scA, scB = _front_scene(200, 150, 48, 150, big_sig=240.0), _flat_scene(200, 150, 100)
    L = _lib.lib()

    def tensors(sc):
        return [sc[k].to(torch.float32).cuda().contiguous() for k in ("means", "col", "op", "scales", "rot")]

    def geometry(prep, t):
        P = t[0].shape[0]
        geom = torch.empty(L.pings_raster_geom_bytes(P, prep.H, prep.W), dtype=torch.uint8, device="cuda")
        radii = torch.empty(P, dtype=torch.int32, device="cuda")
        n_inst, fclass = C.c_int64(0), C.c_int32(1)
        _lib.check(L.pings_raster_preprocess(prep.ref(), P, *[_lib.ptr(x) for x in t], _lib.ptr(geom), _lib.ptr(radii),
                                             C.byref(n_inst), C.byref(fclass), _lib.stream_ptr(t[0].device)), "preprocess")
        return geom, n_inst.value, fclass.value

    rast = hr.SurfelGaussianRasterizer(hip_settings(scA, "surfel", False, 1.0))
    prep, tA, tB = rast._prepared(), tensors(scA), tensors(scB)
    fs, _, per_g = hr._forward(prep, *tA)
    assert _plan()[0] == 1
    want = [fs.color.clone(), fs.depth.clone(), fs.alpha.clone(), fs.normal.clone(), per_g.clone()]
    want_slots, want_ranges = _binning_field(fs, "point_list"), hr.debug_lists(fs)[1].cpu()

    geomA, IA, fcA = geometry(prep, tA)
    geomB, IB, _ = geometry(prep, tB)
    assert IA == fs.I and IB > 0
    H, W, P = prep.H, prep.W, tA[0].shape[0]
    f32 = dict(dtype=torch.float32, device="cuda")
    binning = torch.empty(L.pings_raster_binning_bytes(IA, H, W), dtype=torch.uint8, device="cuda")
    image = torch.empty(L.pings_raster_image_bytes(H, W), dtype=torch.uint8, device="cuda")
    color, normal, depth, alpha = (torch.empty(c, H, W, **f32) for c in (3, 3, 1, 1))
    pg = torch.empty(P, **f32)
    _lib.check(L.pings_raster_render(prep.ref(), P, IA, _lib.ptr(geomA), _lib.ptr(binning), _lib.ptr(image),
                                     _lib.ptr(color), _lib.ptr(normal), _lib.ptr(depth), _lib.ptr(alpha), _lib.ptr(pg),
                                     fcA, _lib.stream_ptr(pg.device)), "render")
    assert _plan()[0] == 0
    for a, b in zip(want, [color, depth, alpha, normal, pg]):
        assert torch.equal(a, b)
    fs.binning = binning
    assert torch.equal(_binning_field(fs, "point_list"), want_slots)
    assert torch.equal(hr.debug_lists(fs)[1].cpu(), want_ranges)
