"""Long tile lists at the thresholds the product uses: the segmented forward (csrc/raster_blend_fwd.hip, seg_plan_kernel,
blend_fwd_wave_segT_kernel / blend_fwd_seg_kernel / blend_fwd_seg_combine_kernel) and the four-wave split of long
tiles in the Gaussian-per-lane backward (csrc/raster_bwd.hip, blend_bwd_scan_kernel), against the fp64 / fp32 oracle
with no threshold forced.  Every default-threshold test first proves from `debug_lists` that the path it targets ran
(`long_paths`): a test that silently exercised the serial kernels fails there, not in a numeric gate."""
import os

import numpy as np
import pytest
import torch

from conftest import rel_err
from scenes import scene_as_dict
from test_raster import (_assert_grad_gate, _hip_forward, _hip_grads, _last_contributor, _oracle, _oracle_grads,
                         _undecidable)

# ------------------------------------------------------------------ the library's predicates, restated
SEG_ENTRIES = 512        # raster_layout.hip read_knobs(): entries per unit (PINGS_BLEND_SEG overrides, 0 = off)
SEG_FRAME_DIV = 4        # seg_on: I > num_tiles * (seg / 4) and I > 2 * seg
SEG_TILE_UNITS = 2       # seg_plan_kernel: a list longer than 2 * seg is cut into ceil(L / seg) units
BWD_LONG = 3072          # raster_layout.hip read_knobs() (PINGS_BWD_LONG overrides, <= 0 = never), rounded up to 16
LONG_TILES_MAX = 2048    # raster_bwd.hip: cap on split tiles, taken in whole bins of tile_order_kernel
TOP_BIN = 1023           # tile_order_kernel: bin = min(work >> 4, 1023)


def _env_int(name, default):
    e = os.environ.get(name)
    return default if e is None else int(e)


def _tile_work(nc, W, H):
    """Largest per-pixel n_contrib of every tile (tile_max_contrib_kernel)."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    ncp = torch.zeros(gy * 16, gx * 16, dtype=torch.int64)
    ncp[:H, :W] = torch.as_tensor(nc).cpu().long()
    return ncp.view(gy, 16, gx, 16).permute(0, 2, 1, 3).reshape(-1, 256).max(1).values


def split_tiles(work, thr_env=None):
    """(tiles the scan backward splits [bool per tile], tiles at or above the threshold) under the library's rule:
    whole bins from the top down while their total stays within LONG_TILES_MAX."""
    v = BWD_LONG if thr_env is None else thr_env
    thr = 0xFFFFFFF0 if v <= 0 else ((v + 15) // 16 * 16) & 0xFFFFFFFF
    bins = torch.clamp(work >> 4, max=TOP_BIN)
    b = thr >> 4
    none = torch.zeros_like(work, dtype=torch.bool)
    if b > TOP_BIN:
        return none, 0
    want = bins >= b
    counts = torch.bincount(bins, minlength=TOP_BIN + 1).flip(0).cumsum(0)[:TOP_BIN + 1 - b]   # bins 1023 .. b
    ok = torch.nonzero(counts <= LONG_TILES_MAX).flatten()
    if ok.numel() == 0:
        return none, int(want.sum())
    return bins >= TOP_BIN - int(ok[-1]), int(want.sum())


def long_paths(fs, rg, nc):
    """Which long-list kernels the frame `fs` ran, recomputed from its lists and counts the way the library decides
    (reads PINGS_BLEND_SEG, PINGS_BWD_LONG, PINGS_BLEND_PPL and PINGS_BLEND_BWD like the library does)."""
    W, H = fs.prep.W, fs.prep.H
    num_tiles = ((W + 15) // 16) * ((H + 15) // 16)
    lens = (rg[:, 1] - rg[:, 0]).cpu().long()
    I = int(lens.sum())
    assert I == fs.I
    ppl = _env_int("PINGS_BLEND_PPL", 0)
    bwd = os.environ.get("PINGS_BLEND_BWD")
    scan = fs.fclass != 2 if bwd is None else bwd != "pixel"
    wave_fwd = ppl != 4 and not (ppl == 0 and fs.fclass == 2 and not scan)
    seg = _env_int("PINGS_BLEND_SEG", SEG_ENTRIES) & 0xFFFFFFFF
    seg_on = wave_fwd and seg > 0 and I > num_tiles * (seg // SEG_FRAME_DIV) and I > 2 * seg
    seg_mask = lens > SEG_TILE_UNITS * seg if seg_on else torch.zeros_like(lens, dtype=torch.bool)
    work = _tile_work(nc, W, H)
    split, at_thr = split_tiles(work, _env_int("PINGS_BWD_LONG", BWD_LONG)) if scan else (torch.zeros_like(work, dtype=torch.bool), 0)
    p = dict(I=I, num_tiles=num_tiles, longest=int(lens.max()), seg_on=seg_on, seg_tiles=int(seg_mask.sum()),
             seg_units=int(((lens[seg_mask] + seg - 1) // max(seg, 1)).sum()), max_work=int(work.max()),
             n_long=int(split.sum()), at_threshold=at_thr, seg_mask=seg_mask, long_mask=split, work=work, lens=lens)
    print(f"\n[long paths] I={I} tiles={num_tiles} longest list {p['longest']} seg_on={seg_on} "
          f"(I > {num_tiles * (seg // SEG_FRAME_DIV)}) segmented tiles {p['seg_tiles']} units {p['seg_units']}; "
          f"max tile work {p['max_work']}, long tiles split {p['n_long']} of {at_thr} at the threshold")
    return p


def assert_long_paths_ran(p, seg=True, split=True):
    if seg:
        assert p["seg_on"] and p["seg_tiles"] > 0, ("segmented forward did not run", p["I"], p["longest"])
    if split:
        assert p["n_long"] > 0, ("no tile was split four ways", p["max_work"])


def test_split_tiles_takes_whole_bins():
    """The cap on split tiles cuts between bins only (tile_order_kernel orders a bin by arrival)."""
    work = torch.cat([torch.full((1500,), 4000), torch.full((1000,), 3500), torch.full((10,), 100)])
    s, at = split_tiles(work)
    assert at == 2500 and int(s.sum()) == 1500 and bool(s[:1500].all())
    s, at = split_tiles(torch.full((3000,), 3100))
    assert at == 3000 and int(s.sum()) == 0
    assert int(split_tiles(torch.tensor([20000, 16368, 5]), 0)[0].sum()) == 0
    assert int(split_tiles(torch.tensor([20000, 16368, 5]), 20000)[0].sum()) == 0
    assert int(split_tiles(torch.tensor([20000, 16368, 5]), 16368)[0].sum()) == 2
    assert split_tiles(torch.tensor([3071, 3072, 3073, 3135]))[0].tolist() == [False, True, True, True]


# ------------------------------------------------------------------ boundary scenes: every list length exact by design
FILL_X, FILL_Y = range(3, 13), range(3, 9)   # tile-local pixels of the filler records (their 1-pixel rings stay in y < 10)
Q_IN = (600, 650, 700, 750, 800, 900)                           # list positions (0-based) at PX_Q: alpha 0.856 each
Q_AFTER = (1100, 1300, 1530, 1600, 2000, 2040, 3000, 3070)     # near-opaque records at Q in units 3 and later
R_ONLY = (1150, 1250, 1700, 2500)                               # pixel R: blended only from unit 3 on
PX_Q, PX_R, PX_LAST = (5, 12), (8, 12), (11, 12)                # the deepest record of a tile lands on PX_LAST alone
SUBPIX = (0.2, 0.15)      # splat centres sit off the pixel centres: power = 0 at a pixel would be a discrete decision


def _fill_op(n_fill):
    """Filler opacity: about 2.5 of optical depth per filler pixel, from a ladder of values at least 15 % away from
    every alpha = 1/255 boundary of the ring (lowpass 0.3 px^2, centre offset SUBPIX: the ring sees G = 0.331, 0.280,
    0.103, 0.087, 0.038, 0.027, 0.010; a boundary lies at op = (1/255) / G)."""
    target = 2.5 / max(1.0, n_fill / 60.0)
    return max([v for v in (0.006, 0.009, 0.02, 0.03, 0.06, 0.08, 0.12) if v <= target] or [0.006])


def _tile_scene(lengths, gx, gy, mode, seed=0):
    """A frame of gx x gy tiles whose tile t holds exactly lengths[t] records: sub-pixel, camera-facing splats whose
    footprint (lowpass 0.3 px^2: the centre pixel and its ring of eight) stays inside one tile, at depths increasing
    with their list position.  Per tile: the deepest record alone on PX_LAST (max n_contrib == the list length); at
    PX_Q records of alpha 0.856 in unit 2 (T = 4.3e-4 after four, the fifth stops the pixel at position 751)
    and near-opaque ones in units 3+ that must blend nothing there; at PX_R records from unit 3 on only."""
    W, H, fx = 16 * gx, 16 * gy, 100.0
    cx, cy = W / 2 - 0.5, H / 2 - 0.5
    g = torch.Generator().manual_seed(seed)
    pix, zs, ops = [], [], []
    for t, L in enumerate(lengths):
        ty, tx = divmod(t, gx)
        k_fill = 0
        n_fill = L - 1 - sum(k < L - 1 for k in Q_IN + Q_AFTER + R_ONLY)
        fop = _fill_op(n_fill)
        for k in range(L):
            if k == L - 1:
                (lx, ly), op = PX_LAST, 0.5
            elif k in Q_IN or k in Q_AFTER:
                (lx, ly), op = PX_Q, 0.95
            elif k in R_ONLY:
                (lx, ly), op = PX_R, 0.3
            else:
                lx, ly = FILL_X[k_fill % len(FILL_X)], FILL_Y[(k_fill // len(FILL_X)) % len(FILL_Y)]
                op, k_fill = fop, k_fill + 1
            pix.append((tx * 16 + lx + SUBPIX[0], ty * 16 + ly + SUBPIX[1]))
            zs.append(2.0 + 2.0 * k / L)
            ops.append(op)
    P = len(zs)
    f64 = torch.float64
    uv = torch.tensor(pix, dtype=f64).reshape(P, 2)
    z = torch.tensor(zs, dtype=f64)
    # (the projection puts a point at pixel fx X / Z + cx - 0.5: scene_as_dict's principal point is at W / 2 - 0.5)
    means = torch.stack([(uv[:, 0] - cx + 0.5) * z / fx, (uv[:, 1] - cy + 0.5) * z / fx, z], 1)
    scales = torch.full((P, 3), 1e-3, dtype=f64)
    if mode == "surfel":
        scales[:, 2] = 1e-7
    rot = torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=f64).expand(P, 4).contiguous()   # normal -z: faces the camera
    col = torch.rand(P, 3, generator=g, dtype=f64)
    op = torch.tensor(ops, dtype=f64).reshape(P, 1)
    return scene_as_dict(means, col, op, scales, rot, W, H, fx)


# name: (gx, gy, list length per tile, seg_on, tiles split four ways)
FRAMES = {
    # not segmented / segmented / exactly three units / a last unit of one entry; tile work 3,071 / 3,072 / 3,073
    "lists": (4, 2, [1024, 1025, 1536, 1537, 2049, 3071, 3072, 3073], True, 2),
    # tile work 3,135 and 16,368: the clamped top bin of tile_order_kernel
    "top_bin": (2, 1, [3135, 16368], True, 2),
    # I == num_tiles * 128 (serial walk) and one more (segmented)
    "frame_below": (8, 4, [3100, 996] + [0] * 30, False, 1),
    "frame_above": (8, 4, [3100, 997] + [0] * 30, True, 1),
}


def test_boundary_scenes_have_the_designed_lists():
    """The oracle (fp32) builds exactly the designed lists, and the designed pixels stop / start where intended."""
    for name, (gx, gy, lengths, _, _) in FRAMES.items():
        if name == "top_bin":
            continue                                 # (the 16k-entry tile is covered by the GPU test's own asserts)
        for mode in ("surfel", "3dgs"):
            sc = _tile_scene(lengths, gx, gy, mode)
            o, *_ = _oracle(sc, torch.float32, mode, True)
            assert ((o["ranges"][:, 1] - o["ranges"][:, 0]).tolist() == lengths), (name, mode)
            assert (o["tiles_touched"] == 1).all()
            _check_designed_counts(o["n_contrib"], lengths, gx)


def _check_designed_counts(nc, lengths, gx):
    nc = torch.as_tensor(nc).cpu()
    for t, L in enumerate(lengths):
        if L == 0:
            continue
        ty, tx = divmod(t, gx)
        at = lambda px: int(nc[ty * 16 + px[1], tx * 16 + px[0]])
        assert int(nc[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16].max()) == L == at(PX_LAST), (t, L)
        if L - 1 > Q_IN[-1]:
            assert at(PX_Q) == Q_IN[3] + 1, (t, at(PX_Q))          # stopped inside unit 2
        r = [k for k in R_ONLY if k < L - 1]
        assert at(PX_R) == (r[-1] + 1 if r else 0), (t, at(PX_R))


def _img_err(t, ref, flag):
    """Per-pixel max-norm error over channels / max|ref| (pixels in `flag` reported apart)."""
    ref = ref.double()
    err = (t.detach().double().cpu() - ref).abs().reshape(-1, *ref.shape[-2:]).amax(0) / max(ref.abs().max().item(), 1e-30)
    return err[~flag].max().item(), (err[flag].max().item() if flag.any() else 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["surfel", "3dgs"])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_boundary_lists_match_the_oracle_at_default_thresholds(frame, mode):
    """Lists of 1,024 / 1,025 / 1,536 / 1,537 / 2,049 / 3,07x / 16,368 entries, frames on both sides of the seg_on
    predicate, a pixel stopping inside unit 2 with near-opaque records behind it, and pixels whose last contributor is
    in a later unit than anything blended into them: images and final_T within 1e-4 of the fp64 and fp32 oracles,
    n_contrib and the last contributor exact, every gradient under the oracle gate — with no threshold forced."""
    gx, gy, lengths, want_seg, want_long = FRAMES[frame]
    sc = _tile_scene(lengths, gx, gy, mode)
    hr, prep, fs, radii, per_g = _hip_forward(sc, mode, True)
    pl, rg, fT, nc = hr.debug_lists(fs)
    p = long_paths(fs, rg, nc)
    assert p["seg_on"] == want_seg and p["n_long"] == want_long, (p["seg_on"], p["n_long"])
    if want_seg:
        assert p["seg_tiles"] == sum(L > SEG_TILE_UNITS * SEG_ENTRIES for L in lengths)
    assert p["lens"].tolist() == lengths                     # nothing culled: the lengths are the designed ones
    _check_designed_counts(nc, lengths, gx)
    o32, *_ = _oracle(sc, torch.float32, mode, True, margins=True)
    o64, names, ref64, ups = _oracle_grads(sc, torch.float64, mode, True)
    _, _, ref32, _ = _oracle_grads(sc, torch.float32, mode, True)
    pix_flag, g_flag = _undecidable(o32, o64)
    print(f"[{frame} {mode}] undecidable: {int(pix_flag.sum())} pixels, {int(g_flag.sum())} of {g_flag.numel()} Gaussians")
    assert (radii.cpu() == o32["radii"]).all()
    assert np.array_equal(pl.cpu().numpy(), o32["point_list"])
    lo = torch.as_tensor(o32["ranges"])
    assert torch.equal(p["lens"], lo[:, 1] - lo[:, 0]) and torch.equal(rg.cpu()[p["lens"] > 0], lo[p["lens"] > 0])
    for o in (o32, o64):
        assert torch.equal(nc.cpu()[~pix_flag], o["n_contrib"][~pix_flag])
        last_o = _last_contributor(o)
        last_h = _last_contributor(dict(point_list=pl.cpu().numpy(), ranges=rg.cpu().numpy(), n_contrib=nc.cpu().numpy()))
        assert np.array_equal(last_h[~pix_flag.numpy()], last_o[~pix_flag.numpy()])
        imgs = [("color", fs.color), ("depth", fs.depth), ("alpha", fs.alpha)] + ([("normal", fs.normal)] if mode == "surfel" else [])
        for k, t in imgs + [("final_T", fT)]:
            ref = 1.0 - o["alpha"][0] if k == "final_T" else o[k]
            e, ef = _img_err(t, ref, pix_flag)
            assert e <= 1e-4 and ef <= 1.1 / 255, (k, e, ef)
    if mode == "surfel":
        assert rel_err(per_g, o64["contributions"]) <= 1e-4
    else:
        assert torch.equal(per_g.cpu()[~g_flag], o32["n_touched"][~g_flag])
    _, got, _ = _hip_grads(sc, mode, True, ups)
    _assert_grad_gate(names, got, ref64, ref32, f"{frame} {mode}", flips_allowed=bool(g_flag.any()))


# ------------------------------------------------------------------ the timed sizes
def _bench_frame(workload, P, W, H, fx):
    """The bench's inputs and settings of a BASELINE.json workload (as test_raster.py::test_full_size_properties)."""
    import bench
    from pings_amd import rasterizer as hr
    from scenes import room_scene, street_scene

    dev = torch.device("cuda")
    if workload == "metric1_cloud":
        parts = bench.synth_cloud(P, W, H, fx, fx, dev)
    else:
        parts = (room_scene if workload == "c2_room" else street_scene)(P, device=dev, seed=1)
    cam = bench.camera(W, H, fx, fx, W / 2 - 0.5, H / 2 - 0.5, 0.05, 110.0, 0, dev)
    rs = hr.SurfelRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=torch.ones(3, device=dev),
        scale_modifier=1.0, viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"],
        projmatrix_raw=cam["projmatrix_raw"], patch_bbox=torch.tensor([0, 0, H - 1, W - 1], dtype=torch.float32, device=dev),
        prcppoint=cam["prcppoint"], sh_degree=0, campos=cam["campos"], prefiltered=False, debug=False,
        config=torch.tensor([1, 1, 1, 1, 1], dtype=torch.float32, device=dev))
    return parts, rs


def _run_frame(parts, rs, ups):
    """Forward + backward through the autograd op, and the frame's lists; everything needed to compare two runs."""
    from pings_amd import rasterizer as hr

    rast = hr.SurfelGaussianRasterizer(rs)
    leaves = [t.detach().clone().requires_grad_(True) for t in parts]
    th = torch.zeros(3, device="cuda", requires_grad=True)
    rh = torch.zeros(3, device="cuda", requires_grad=True)
    out = rast(means3D=leaves[0], means2D=torch.zeros_like(leaves[0]), colors_precomp=leaves[1], opacities=leaves[2],
               scales=leaves[3], rotations=leaves[4], theta=th, rho=rh)
    img, nrm, dep, alp, radii, contrib = out
    torch.autograd.backward([img, nrm, dep, alp], list(ups))
    fs, _, _ = hr._forward(rast._prepared(), *[t.detach() for t in leaves])
    pl, rg, fT, nc = hr.debug_lists(fs)
    p = long_paths(fs, rg, nc)
    last = _last_contributor(dict(point_list=pl.cpu().numpy(), ranges=rg.cpu().numpy(), n_contrib=nc.cpu().numpy()))
    return dict(I=fs.I, p=p, radii=radii.detach().clone(), contrib=contrib.detach().clone(),
                imgs=[t.detach().clone() for t in (img, nrm, dep, alp, fT)], last=last,
                grads=[t.grad.clone() for t in leaves] + [th.grad.clone(), rh.grad.clone()])


def _assert_runs_identical(t, q):
    assert torch.equal(t["radii"], q["radii"])
    assert rel_err(t["contrib"], q["contrib"]) <= 1e-6
    for a, b in zip(t["imgs"], q["imgs"]):
        assert torch.equal(a, b)
    assert np.array_equal(t["last"], q["last"])
    for k, (a, b) in enumerate(zip(t["grads"], q["grads"])):
        assert torch.equal(a, b), (k, (a - b).abs().max().item())


FULL_SIZE = [("metric1_cloud", 1_000_000, 1920, 1080, 1000.0), ("c2_room", 200_000, 640, 480, 600.0),
             ("c3_street", 1_000_000, 1392, 512, 720.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("workload,P,W,H,fx", FULL_SIZE)
def test_tight_rectangle_is_lossless_at_the_timed_sizes(workload, P, W, H, fx, monkeypatch):
    """test_raster.py::test_default_rectangle_is_lossless at the sizes the bench times, default kernels: tight == the
    published 3 sigma square bit for bit (radii, images, final_T, last contributor, every gradient; `contributions` to
    fp32 summation order) where the frame runs neither the segmented forward nor the four-wave split.  Where it does
    (C3), bit for bit with both switched off, and at defaults within the bounds test_raster.py's
    test_long_lists_blended_in_parallel_segments allows between segmented and serial walks: the two rules' lists differ
    in length, so the segments cut at other records and the fp32 sums regroup."""
    parts, rs = _bench_frame(workload, P, W, H, fx)
    g = torch.Generator(device="cuda").manual_seed(1)
    ups = [torch.randn(c, H, W, generator=g, device="cuda") for c in (3, 3, 1, 1)]

    def both():
        res = {}
        for rule in ("tight", "3sigma"):
            monkeypatch.setenv("PINGS_RASTER_RECT", rule)
            res[rule] = _run_frame(parts, rs, ups)
        print(f"[{workload}] instances tight {res['tight']['I']}, 3sigma {res['3sigma']['I']}")
        assert res["tight"]["I"] <= res["3sigma"]["I"]
        return res["tight"], res["3sigma"]

    t, q = both()
    # (seg_on with no list longer than 2 x 512 runs the short-list walk of the segmented launch only: serial, bitwise)
    long_run = any(r["p"]["seg_tiles"] > 0 or r["p"]["n_long"] > 0 for r in (t, q))
    print(f"[{workload}] long tiles split: tight {t['p']['n_long']} (of {t['p']['at_threshold']} at the threshold), "
          f"segmented tiles {t['p']['seg_tiles']}")
    if not long_run:
        _assert_runs_identical(t, q)
        return
    assert workload == "c3_street", workload       # only the street view reaches the long-list kernels
    npix = t["last"].size
    for a, b in zip(t["imgs"], q["imgs"]):
        assert rel_err(a, b) <= 1e-5
    assert int((t["last"] != q["last"]).sum()) <= 1e-3 * npix
    for a, b in zip(t["grads"], q["grads"]):
        assert rel_err(a, b) <= 2e-4
    monkeypatch.setenv("PINGS_BLEND_SEG", "0")
    monkeypatch.setenv("PINGS_BWD_LONG", "1000000000")
    t0, q0 = both()
    assert not t0["p"]["seg_on"] and t0["p"]["n_long"] == 0 and q0["p"]["n_long"] == 0
    _assert_runs_identical(t0, q0)


@pytest.mark.gpu
def test_long_tile_selection_is_deterministic(monkeypatch):
    """More tiles reach the long-list threshold than LONG_TILES_MAX (2,304 tiles, threshold 16): tile_order_kernel
    caps the split set at a whole bin, so it does not depend on the arrival order of its LDS atomics.  Three backward
    runs are bitwise equal, and within 1e-5 of the one-wave-per-quadrant walk (PINGS_BWD_LONG=0)."""
    import bench

    W, H, fx = 1024, 576, 600.0
    parts, rs = _bench_frame("metric1_cloud", 300_000, W, H, fx)
    g = torch.Generator(device="cuda").manual_seed(2)
    ups = [torch.randn(c, H, W, generator=g, device="cuda") for c in (3, 3, 1, 1)]
    monkeypatch.setenv("PINGS_BLEND_BWD", "scan")
    monkeypatch.setenv("PINGS_BWD_LONG", "16")
    runs = [_run_frame(parts, rs, ups) for _ in range(3)]
    p = runs[0]["p"]
    assert p["at_threshold"] > LONG_TILES_MAX and 0 < p["n_long"] <= LONG_TILES_MAX, (p["at_threshold"], p["n_long"])
    print(f"[selection] {p['at_threshold']} of {p['num_tiles']} tiles at the threshold, {p['n_long']} split")
    for r in runs[1:]:
        for a, b in zip(runs[0]["grads"], r["grads"]):
            assert torch.equal(a, b)
    monkeypatch.setenv("PINGS_BWD_LONG", "0")
    one = _run_frame(parts, rs, ups)
    assert one["p"]["n_long"] == 0
    for a, b in zip(runs[0]["grads"], one["grads"]):
        assert rel_err(a, b) <= 1e-5


@pytest.mark.gpu
def test_c3_shape_gradients_match_the_oracle_on_long_tiles():
    """An oracle-checked gradient test on the C3 shape at default thresholds: street scene at the full 1392x512 with
    the bench's fx = 720, density 300k surfels (of the bench's 1M) so that both long-list kernels run — lists past
    2 x 512 entries (segmented forward) and tiles with a pixel walking 3,072+ records (four-wave backward) — while the
    oracle stays affordable.  It blends every such tile plus a sparse sample of the others (`tile_subset`), upstream
    gradients zero elsewhere, as test_raster.py::test_c2_shape_gradients_match_the_oracle_on_a_tile_subset.  The
    oracle runs in chunks of about 40k list entries (the gradients of disjoint tile sets add up).  Measured: 210 tiles /
    269k entries in 7 chunks, fp32 + fp64 autograd in 43 s (65 s on an 8-core host), 6.4 GB peak resident memory of
    the whole test process (4.2 GB for the oracle alone).
    The undecidable pixel fraction (0.00158 measured) is capped at 2x that, 0.0032, above the street ceiling of the bench
    (0.001): that ceiling was set on the 24k-surfel street view, whose horizon lists are a fraction as long as these.
    PINGS_TEST_FULL=1 samples every fourth tile of the others instead of every 32nd."""
    import resource
    import time

    import bench
    from scenes import street_scene
    from test_raster import _assert_grad_gate_identified, _check_list_prefixes, _errs

    P, W, H, fx = 300_000, 1392, 512, 720.0
    sc = scene_as_dict(*street_scene(P, device="cpu", seed=2), W, H, fx)
    hr, prep, fs, radii, per_g = _hip_forward(sc, "surfel", True)
    pl, rg, fT, nc = hr.debug_lists(fs)
    p = long_paths(fs, rg, nc)
    assert_long_paths_ran(p)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    tid = torch.arange(gx * gy)
    every = 4 if os.environ.get("PINGS_TEST_FULL", "0") == "1" else 32
    sub = (p["lens"] > SEG_TILE_UNITS * SEG_ENTRIES) | (p["work"] >= BWD_LONG) | ((tid % gx + 3 * (tid // gx)) % every == 0)
    chunks, cur, acc = [], [], 0
    for t in torch.nonzero(sub).flatten().tolist():
        if cur and acc + int(p["lens"][t]) > 40_000:
            chunks.append(cur)
            cur, acc = [], 0
        cur.append(t)
        acc += int(p["lens"][t])
    chunks.append(cur)
    tile_pix = lambda m: m.view(gy, gx).repeat_interleave(16, 0).repeat_interleave(16, 1)[:H, :W]
    in_sub = tile_pix(sub)
    t0 = time.time()
    o32s, o64s, ref32, ref64, ups, pix_flag, g_flag = {}, {}, None, None, None, None, None
    for c in chunks:
        cs = set(c)
        f = lambda tx, ty: ty * gx + tx in cs
        m = torch.zeros(gx * gy, dtype=torch.bool)
        m[c] = True
        m = tile_pix(m)
        o32, names, r32, u = _oracle_grads(sc, torch.float32, "surfel", True, margins=True, tile_subset=f, pix_mask=m)
        o64, _, r64, _ = _oracle_grads(sc, torch.float64, "surfel", True, tile_subset=f, pix_mask=m)
        pf, gf = _undecidable(o32, o64)
        acc_ = lambda a, b: b.detach().clone() if a is None else a + b.detach()
        ref32 = [acc_(a, b) for a, b in zip(ref32 or [None] * len(r32), r32)]
        ref64 = [acc_(a, b) for a, b in zip(ref64 or [None] * len(r64), r64)]
        ups = [acc_(a, b) for a, b in zip(ups or [None] * 4, u)]
        pix_flag = pf if pix_flag is None else pix_flag | pf
        g_flag = gf if g_flag is None else g_flag | gf
        for k in ("color", "normal", "depth", "alpha", "n_contrib"):
            o32s[k] = acc_(o32s.get(k), o32[k] * m if k != "n_contrib" else o32[k])
            if k != "n_contrib":
                o64s[k] = acc_(o64s.get(k), o64[k] * m)
        o32s["radii"], o32s["point_list"], o32s["ranges"] = o32["radii"], o32["point_list"], o32["ranges"]
    print(f"\n[C3 shape {P}@{W}x{H}] oracle: {len(chunks)} chunks, {int(sub.sum())} tiles, {int(p['lens'][sub].sum())} "
          f"list entries, fp32 + fp64 autograd {time.time() - t0:.1f} s, peak resident memory "
          f"{resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6:.2f} GB")
    # the Gaussian fraction under the street ceiling of the bench; the pixel fraction measured 0.00158 on this view (the
    # bench's 0.001 is set for its own 24k-surfel street test): a cap of the test's own, 2x the measured value
    g_cap = bench.UNDECIDABLE_CEILING["street"][1]
    pix_cap = 0.0032
    pix_frac, g_frac = float(pix_flag.float().mean()), float(g_flag.float().mean())
    print(f"[C3 shape] undecidable: {pix_frac:.5f} of the pixels (cap {pix_cap}), {g_frac:.4f} of the Gaussians (ceiling {g_cap})")
    assert pix_frac <= pix_cap and g_frac <= g_cap
    assert (radii.cpu() == o32s["radii"]).all()
    o_lists = dict(o32s)
    o_lists["n_contrib"] = torch.where(in_sub, o32s["n_contrib"], nc.cpu())
    _check_list_prefixes(pl, rg, nc, o_lists, W, H)
    assert not ((nc.cpu() != o32s["n_contrib"]) & in_sub & ~pix_flag).any()
    _, got, _ = _hip_grads(sc, "surfel", True, ups)
    out = (fs.color, fs.normal, fs.depth, fs.alpha)
    for k, t in zip(("color", "normal", "depth", "alpha"), out):
        tm = t.detach().double().cpu() * in_sub
        r32, r64 = o32s[k].double(), o64s[k].double()
        err = (tm - r32).abs().amax(0) / max(r32.abs().max().item(), 1e-30)
        assert err[in_sub & ~pix_flag].max().item() <= 1e-4, (k, err[in_sub & ~pix_flag].max().item())
        e64 = _errs(tm, r64)
        print(f"  {k:7s} vs fp64 oracle: max-norm {e64[0]:.2e}, rel-L2 {e64[1]:.2e}, entries > 1e-4: {e64[2]}")
        assert e64[1] <= 1e-4 and e64[2] <= max(16, 5e-5 * tm.numel()), (k, e64)
        assert e64[0] <= (1e-2 if k == "depth" else 1.1 / 255), (k, e64)
    _assert_grad_gate_identified(names, got, ref64, ref32, f"C3 shape {P}@{W}x{H}, long tiles + sample", g_flag)
