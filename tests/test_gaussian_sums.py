"""The per-Gaussian sums and the frame statistics after the per-rank kernels stopped working behind the last needed
depth rank (csrc/raster_fwd.hip, csrc/raster_blend_fwd.hip):

  * per_gaussian_sum_kernel stores a sum only for a rank that kept a tile; the zeros of every other Gaussian are
    streamed out by duplicate_kernel of the same render call (a fill when the frame has no instance at all);
  * the footprint statistic behind `footprint_class` is accumulated by preprocess_kernel and has to survive the clear
    of a depth-sort retry; count_kept_kernel keeps only the kept total (`num_instances`).

Forward only, through the C ABI the way rasterizer.py drives it, with the per-Gaussian buffer handed over as NaN bit
patterns so that an entry nobody wrote is seen.  Reference: the run with the occlusion bound switched off (the sums of
the same non-zero terms in another association: rtol 1e-5, atol 1e-7 as in tests/test_occl_buckets.py) and
oracle/raster_cpu.py in fp32 for the set of culled Gaussians."""
import ctypes as C
import functools

import pytest
import torch

from conftest import rel_err
from oracle import raster_cpu as R
from scenes import hip_settings, make_scene, oracle_settings
from test_gaussian_passes import _nan, _scene
from test_raster import _oracle

FRONT_ONLY = False
SMALL_RUN = 16          # csrc/raster_blend_fwd.hip: runs up to this length are summed by their lane, longer ones by the wave
KNOBS = ("PINGS_RASTER_OCCLUSION", "PINGS_DEPTH_SORT", "PINGS_BLEND_PPL", "PINGS_BLEND_SEG")
# forward kernels in front of the sums: by footprint class, wave per tile, wave per quadrant with 16-entry segments
FORWARD = {"class": {}, "tile": {"PINGS_BLEND_PPL": "4"}, "segments": {"PINGS_BLEND_PPL": "-1", "PINGS_BLEND_SEG": "16"}}


def _forward(sc, mode, monkeypatch, env):
    """preprocess + render -> dict(contributions, radii, I, fclass, owners of the kept instances)"""
    from pings_amd import _lib
    from pings_amd import rasterizer as hr

    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    L = _lib.lib()
    dev = torch.device("cuda")
    prep = hr._Prepared(hip_settings(sc, mode, FRONT_ONLY), hr.MODE_SURFEL if mode == "surfel" else hr.MODE_3DGS)
    d = lambda t: t.to(torch.float32).to(dev).contiguous()
    means, col, op, scales, rot = (d(sc[k]) for k in ("means", "col", "op", "scales", "rot"))
    P, H, W = means.shape[0], prep.H, prep.W
    stream = _lib.stream_ptr(dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    geom = torch.empty(L.pings_raster_geom_bytes(P, H, W), **u8)
    image = torch.empty(L.pings_raster_image_bytes(H, W), **u8)
    radii = torch.empty(P, dtype=torch.int32, device=dev)
    color, depth, alpha = _nan(3, H, W), _nan(1, H, W), _nan(1, H, W)
    normal = _nan(3, H, W) if mode == "surfel" else None
    per_g = _nan(P) if mode == "surfel" else _nan(P, dtype=torch.int32)
    n_inst, fclass = C.c_int64(0), C.c_int32(1)
    _lib.check(L.pings_raster_preprocess(prep.ref(), P, _lib.ptr(means), _lib.ptr(col), _lib.ptr(op), _lib.ptr(scales),
                                         _lib.ptr(rot), _lib.ptr(geom), _lib.ptr(radii), C.byref(n_inst),
                                         C.byref(fclass), stream), "pings_raster_preprocess")
    I = n_inst.value
    binning = torch.empty(L.pings_raster_binning_bytes(I, H, W), **u8)
    _lib.check(L.pings_raster_render(prep.ref(), P, I, _lib.ptr(geom), _lib.ptr(binning), _lib.ptr(image),
                                     _lib.ptr(color), _lib.ptr(normal), _lib.ptr(depth), _lib.ptr(alpha),
                                     _lib.ptr(per_g), fclass.value, stream), "pings_raster_render")
    torch.cuda.synchronize()
    fs = hr._ForwardState()
    fs.prep, fs.P, fs.I, fs.fclass = prep, P, I, int(fclass.value)
    fs.geom, fs.binning, fs.image = geom, binning, image
    owners = hr.debug_lists(fs)[0] if I > 0 else torch.zeros(0, dtype=torch.int64, device=dev)
    return dict(contributions=per_g, radii=radii, I=I, fclass=int(fclass.value), owners=owners, color=color,
                words=_frame_words(L, geom, P, H, W))


STAT_SHARDS, DS_FLAG = 256, 130      # csrc/raster_common.hpp


def _frame_words(L, geom, P, H, W):
    """The frame statistics and the depth sort's overflow flag, read out of the geometry blob by the layout of
    carve_geom (csrc/raster_layout.hip): fields in declaration order, each on a 256-byte boundary.  -> dict(pairs,
    visible, kept: the sums over the shards; overflow: the flag a depth bucket of more than DS_LIMIT leaves — the
    frame's one clear zeroes it, the bucket sort alone sets it and the retry does not clear it).  The caller checks the
    sums against known values, which guards the offsets."""
    nt = ((W + 15) // 16) * ((H + 15) // 16)
    nb = C.c_int32(0)
    assert L.pings_raster_debug_occlusion(None, P, H, W, None, None, C.byref(nb), None) == 0
    al = lambda n: (n + 255) // 256 * 256
    off = al(64 * P) + al(16 * P) + 7 * al(4 * P) + al(4 * nt * nb.value)
    stats = geom[off:off + 8 * 3 * STAT_SHARDS].view(torch.int64).view(3, STAT_SHARDS).sum(1).tolist()
    off += al(8 * (3 * STAT_SHARDS + 1))
    flag = int(geom[off + 4 * DS_FLAG:off + 4 * DS_FLAG + 4].view(torch.int32)[0])
    return dict(pairs=stats[0], visible=stats[1], kept=stats[2], overflow=flag)


@functools.lru_cache(maxsize=None)
def _reference(kind, P, size, mode):
    """Scene and the oracle's per-Gaussian outputs, once per scene (never modified): radii and the 3DGS counts from
    the fp32 oracle (exact), the surfel sums from the fp64 one."""
    sc = _scene(kind, P, size, mode)
    o32, *_ = _oracle(sc, torch.float32, mode, FRONT_ONLY)
    ref = {k: o32[k].detach() for k in ("n_touched", "radii") if k in o32}
    ref["tiles"] = o32["geom"]["tiles_touched"].detach()
    if mode == "surfel":
        o64, *_ = _oracle(sc, torch.float64, mode, FRONT_ONLY)
        ref["contributions"] = o64["contributions"].detach()
    return sc, ref


def _check_sums(sc, ref, mode, monkeypatch, env, what):
    off = _forward(sc, mode, monkeypatch, {**env, "PINGS_RASTER_OCCLUSION": "0"})
    on = _forward(sc, mode, monkeypatch, env)
    lib = _forward(sc, mode, monkeypatch, {**env, "PINGS_DEPTH_SORT": "l"})
    for run in (off, on, lib):
        c = run["contributions"]
        if mode == "surfel":
            assert not bool(torch.isnan(c).any()), (what, "an entry nobody wrote")
        else:
            assert int(c.min()) >= 0 and int(c.max()) <= sc["W"] * sc["H"], (what, "an entry nobody wrote")
        assert bool((run["radii"].cpu() == ref["radii"]).all()), what
        # exactly zero, bit for bit, for every Gaussian the oracle culls and for every one without a kept instance
        idle = torch.ones(c.shape[0], dtype=torch.bool, device=c.device)
        idle[run["owners"].long()] = False
        assert bool((run["radii"][idle.logical_not()] > 0).all()), what
        assert int(c.view(torch.int32)[idle | (run["radii"] == 0)].long().abs().sum()) == 0, what
    # exactly zero wherever the reference sum (bound off) is zero; equal to it up to the association of the terms
    a, b = on["contributions"], off["contributions"]
    assert int(a.view(torch.int32)[b == 0].long().abs().sum()) == 0, what
    if mode == "surfel":
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-7), what
        if "contributions" in ref:      # the gate tests/test_gaussian_passes.py applies against the fp64 oracle
            assert rel_err(a, ref["contributions"]) <= 1e-4, what
    else:
        assert torch.equal(a, b) and bool((a.cpu() == ref["n_touched"]).all()), what
    assert 0 <= on["I"] <= off["I"]
    # the statistics of the frame against the oracle's rectangles: pairs before culling, Gaussians with a tile, the
    # class they decide (2 = more than 16 pairs per Gaussian with a tile), and the kept total
    pairs, visible = int(ref["tiles"].sum()), int((ref["tiles"] > 0).sum())
    fclass = 2 if visible > 0 and pairs > 16 * visible else 1
    for run in (off, on, lib):
        w = run["words"]
        assert (w["pairs"], w["visible"], w["kept"]) == (pairs, visible, run["I"]), (what, w)
        assert run["fclass"] == fclass, (what, run["fclass"], pairs, visible)
    assert off["I"] == pairs and lib["words"]["overflow"] == 0, what
    # ... against the library-sort knob, and the sums bit for bit
    assert (on["fclass"], on["I"]) == (lib["fclass"], lib["I"]), what
    assert torch.equal(on["contributions"].view(torch.int32), lib["contributions"].view(torch.int32)), what
    return on, off, fclass


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["surfel", "3dgs"])
@pytest.mark.parametrize("P", [1, 255, 257, 1027])
def test_zero_fill_with_unaligned_tails(P, mode, monkeypatch):
    sc, ref = _reference("small", P, "s", mode)
    on, _, _ = _check_sums(sc, ref, mode, monkeypatch, {}, f"small P={P} {mode}")
    assert on["I"] > 0 and int((on["radii"] > 0).sum()) == P


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["surfel", "3dgs"])
@pytest.mark.parametrize("P,size", [(1, "s"), (257, "l")])
def test_frame_without_an_instance_is_all_zeros(P, size, mode, monkeypatch):
    sc = _scene("behind", P, size, mode)
    for env in ({}, {"PINGS_RASTER_OCCLUSION": "0"}, {"PINGS_DEPTH_SORT": "l"}):
        run = _forward(sc, mode, monkeypatch, env)
        assert run["I"] == 0 and run["fclass"] == 1 and int((run["radii"] != 0).sum()) == 0
        assert int(run["contributions"].view(torch.int32).abs().max()) == 0
        assert run["words"] == dict(pairs=0, visible=0, kept=0, overflow=0)


@pytest.mark.gpu
@pytest.mark.parametrize("forward", list(FORWARD))
@pytest.mark.parametrize("mode", ["surfel", "3dgs"])
@pytest.mark.parametrize("kind,P", [("cover", 65), ("occluders", 256), ("alternating", 1000)])
def test_short_and_long_runs_behind_every_forward_kernel(kind, P, mode, forward, monkeypatch):
    """`cover`: one surfel with an instance in each of the 70 tiles (a run summed by the whole wave) among small ones
    (runs of at most SMALL_RUN, summed by their lane); `occluders`: every tile saturates, survivors without a kept tile;
    `alternating`: culled and visible Gaussians side by side in a wave."""
    sc, ref = _reference(kind, P, "l", mode)
    on, off, _ = _check_sums(sc, ref, mode, monkeypatch, FORWARD[forward], f"{kind} {mode} {forward}")
    runs = torch.bincount(on["owners"].long(), minlength=P)
    if kind == "cover":
        big = sc["big"][0]
        assert int(runs[big]) == 70 > SMALL_RUN
        small = runs[(runs > 0) & (torch.arange(P, device=runs.device) != big)]
        assert small.numel() > 0 and int(small.max()) <= SMALL_RUN
        if mode == "surfel":
            assert float(on["contributions"][big]) > 0
    if kind == "occluders":
        assert 0 < on["I"] < off["I"]
        assert int((runs > 0).sum()) < int((on["radii"] > 0).sum())      # survivors that keep nothing


@pytest.mark.gpu
def test_statistics_survive_the_depth_sort_retry(monkeypatch):
    """More than DS_LIMIT = 4096 surviving Gaussians at exactly one depth overflow a depth bucket: the frame is redone
    with the library sort after a clear that must leave preprocess_kernel's footprint statistic alone.  The scene is
    class 2 (27 pairs per Gaussian with a tile): with the statistic cleared the host would see no visible Gaussian and
    answer class 1.  That the retry was taken is read from the device: the overflow flag in the geometry blob."""
    W, H = 160, 96
    sc = make_scene(12000, W, H, seed=123, surfel=True, behind_frac=0.0)
    V = sc["cam"]["viewmatrix"].to(sc["means"].dtype)
    pc = sc["means"] @ V[:3, :3] + V[3, :3]
    pc[:, 2] = 3.0
    sc["means"] = (pc - V[3, :3]) @ torch.linalg.inv(V[:3, :3])
    sc["scales"] = sc["scales"] * 3.0
    f = lambda k: sc[k].to(torch.float32)
    geom = R.preprocess(f("means"), f("scales"), f("rot"), oracle_settings(sc, torch.float32, "surfel", FRONT_ONLY),
                        opacities=f("op"))
    tiles = geom["tiles_touched"]
    # the view transform in fp32 leaves a few neighbouring key values: one of them alone must overflow its bucket
    assert int(geom["pz"][geom["valid"]].unique(return_counts=True)[1].max()) > 4096
    assert int(tiles.sum()) > 20 * int((tiles > 0).sum())
    ref = {"radii": geom["radii"], "tiles": tiles}
    on, off, fclass = _check_sums(sc, ref, "surfel", monkeypatch, {}, "single depth plane")
    assert fclass == 2 and on["fclass"] == 2 and off["fclass"] == 2
    # both default-sort runs overflowed a bucket on the device and were redone (the library-sort run never sets the flag:
    # _check_sums)
    assert on["words"]["overflow"] != 0 and off["words"]["overflow"] != 0


