"""The per-Gaussian passes of the raster step (per_gaussian_sum_kernel, row_chunk_sum_kernel, grad_zero_kernel,
gaussian_bwd_kernel, tau_reduce_kernel), which run over depth ranks and leave the Gaussians without a live row to a
zero fill: driven through the C ABI the way rasterizer.py drives it, with every output buffer pre-filled with NaN bit
patterns so that an entry nobody wrote is seen.

Per scene, mode and backward plan: no NaN left, +0.0 bit for bit in every gradient entry of a Gaussian that contributed
nothing, zero `contributions` for culled Gaussians, two runs bit-identical, PINGS_ROWSUM_WGS=1 (one workgroup strides
over all pairs) and PINGS_DEPTH_SORT=l (library depth sort) bit-equal to the default, and gradients / contributions
against oracle/raster_cpu.py in fp64 under the gates tests/test_raster.py applies to the same quantities."""
import ctypes as C
import functools
import math
import os

import pytest
import torch

from conftest import rel_err
from oracle import raster_cpu as R
from scenes import hip_settings, random_pose
from test_raster import _assert_grad_gate, _oracle, _oracle_grads

FRONT_ONLY = False
SIZES = {"s": (64, 48), "l": (160, 112)}   # 12 and 70 tiles


def _scene(kind, P, size, mode):
    """fp64 scene dict (tests/scenes.py layout).  Gaussians are placed in the camera frame and moved to the world."""
    W, H = SIZES[size]
    g = torch.Generator().manual_seed(1000 * P + 7 * len(kind) + (size == "l"))
    f64 = torch.float64
    fx = fy = 0.9 * W
    T_cw = random_pose(g)
    cam = R.look_at_camera(W, H, fx, fy, 0.5 * W - 1.7, 0.5 * H + 0.9, 0.05, 100.0, T_cw=T_cw, dtype=f64)
    r = lambda *s: torch.rand(*s, generator=g, dtype=f64)
    z = 2.0 + 7.0 * r(P)
    x = (r(P) - 0.5) * 0.9 * W / fx * z
    y = (r(P) - 0.5) * 0.9 * H / fy * z
    scales = torch.exp(math.log(0.02) + (math.log(0.15) - math.log(0.02)) * r(P, 3))
    rot = torch.nn.functional.normalize(torch.randn(P, 4, generator=g, dtype=f64), dim=1)
    op = 0.05 + 0.95 * r(P, 1)
    col = r(P, 3)
    big = []
    if kind == "behind":
        z = -z
    elif kind == "alternating":          # culled and visible Gaussians alternate in the index: a wave holds both
        z[0::2] = -z[0::2]
    elif kind == "occluders":            # four screen-filling surfels of opacity 0.99 in front of all others
        big = [i % P for i in (5, 70, 130, 200)]
        for k, i in enumerate(big):
            z[i] = 1.0 + 0.05 * k
            op[i] = 0.99
    elif kind == "cover":                # one surfel over every tile: more than CH = 64 gradient rows for one Gaussian
        big = [7 % P]
        z[big[0]] = 1.5
        op[big[0]] = 0.6
    else:
        assert kind == "small"
    for k, i in enumerate(big):
        # centred off the image: the occlusion budget leaves out the tiles around a footprint's centre
        x[i], y[i] = (3.0 if k & 1 else -3.0), (2.0 if k & 2 else -2.0)
        scales[i] = torch.tensor([30.0, 30.0, 0.01], dtype=f64)
        rot[i] = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=f64)
    if mode == "surfel":
        scales[:, 2] = 1e-7
    T_wc = torch.linalg.inv(T_cw)
    means = torch.stack([x, y, z], 1) @ T_wc[:3, :3].T + T_wc[:3, 3]
    return dict(means=means, scales=scales, rot=rot, op=op, col=col, bg=torch.tensor([1.0, 0.9, 0.8], dtype=f64),
                cam=cam, W=W, H=H, big=big)


# kind, P, image size
SCENES = ([("small", P, "s") for P in (1, 63, 64, 65, 255, 256, 257, 1000)] +
          [("behind", 1, "s"), ("behind", 65, "l"), ("alternating", 257, "s"), ("alternating", 1000, "l"),
           ("small", 257, "l"), ("occluders", 256, "l"), ("cover", 65, "l")])


@functools.lru_cache(maxsize=None)
def _reference(kind, P, size, mode):
    """The scene and its oracle results, computed once and shared by the backward plans (never modified)."""
    sc = _scene(kind, P, size, mode)
    if kind == "behind":
        return sc, None
    o64, names, ref64, ups = _oracle_grads(sc, torch.float64, mode, FRONT_ONLY)
    o32, _, ref32, _ = _oracle_grads(sc, torch.float32, mode, FRONT_ONLY)
    keep = lambda o: {k: o[k].detach() for k in ("contributions", "n_touched", "radii") if k in o}
    return sc, (keep(o64), keep(o32), names, [t.detach() for t in ref64], [t.detach() for t in ref32], ups)


def _nan(*shape, dtype=torch.float32):
    """A buffer of 0xFFFFFFFF words: a NaN as float, and no count or sum an integer kernel would produce."""
    return torch.full(shape, -1, dtype=torch.int32, device="cuda").view(dtype)


def _run(sc, mode, ups):
    """preprocess, render and backward through the C ABI; every output starts as NaN bit patterns.
    -> dict of outputs (fresh tensors), the forward state for the debug taps"""
    from pings_amd import _lib
    from pings_amd import rasterizer as hr

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
    gc, gn, gd, ga = (t.to(torch.float32).to(dev).contiguous() for t in ups)
    scratch = torch.empty(L.pings_raster_backward_bytes(P, I), **u8)
    grads = [_nan(P, c) for c in (3, 3, 3, 1, 3, 4)]   # means3D, means2D, colors, opacities, scales, rotations
    d_tau = _nan(6)
    _lib.check(L.pings_raster_backward(
        prep.ref(), P, I, _lib.ptr(means), _lib.ptr(col), _lib.ptr(op), _lib.ptr(scales), _lib.ptr(rot), _lib.ptr(geom),
        _lib.ptr(binning), _lib.ptr(image), _lib.ptr(color), _lib.ptr(normal), _lib.ptr(depth), _lib.ptr(alpha),
        _lib.ptr(gc), _lib.ptr(gn) if mode == "surfel" else None, _lib.ptr(gd), _lib.ptr(ga), _lib.ptr(scratch),
        *[_lib.ptr(t) for t in grads], _lib.ptr(d_tau), fclass.value, stream), "pings_raster_backward")
    torch.cuda.synchronize()
    fs = hr._ForwardState()
    fs.prep, fs.P, fs.I, fs.fclass = prep, P, I, int(fclass.value)
    fs.geom, fs.binning, fs.image = geom, binning, image
    out = dict(radii=radii, contributions=per_g, d_means3D=grads[0], d_means2D=grads[1], d_colors=grads[2],
               d_opacities=grads[3], d_scales=grads[4], d_rotations=grads[5], d_tau=d_tau)
    return out, fs


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_same_bits(a, b, what):
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k)


PER_GAUSSIAN = ("d_means3D", "d_means2D", "d_colors", "d_opacities", "d_scales", "d_rotations")


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["pixel", "scan"])
@pytest.mark.parametrize("mode", ["surfel", "3dgs"])
@pytest.mark.parametrize("kind,P,size", SCENES)
def test_per_gaussian_passes(kind, P, size, mode, plan, monkeypatch):
    from pings_amd import rasterizer as hr

    monkeypatch.setenv("PINGS_BLEND_BWD", plan)
    sc, ref = _reference(kind, P, size, mode)
    W, H = sc["W"], sc["H"]
    if ref is None:
        g = torch.Generator().manual_seed(5)
        ups = tuple(torch.randn(c, H, W, generator=g, dtype=torch.float64) for c in (3, 3, 1, 1))
    else:
        ups = ref[5]
    out, fs = _run(sc, mode, ups)

    # every entry was written by someone
    for k, t in out.items():
        if t.dtype.is_floating_point:
            assert not torch.isnan(t).any(), (k, "NaN left")
    if mode == "3dgs":
        assert int(out["contributions"].min()) >= 0 and int(out["contributions"].max()) <= W * H
    # A Gaussian that contributed nothing has +0.0 in every gradient entry; a culled one contributed nothing.  Surfel
    # `contributions` is the sum of the blend weights: zero means never blended.  The 3DGS count (pixels reached with a
    # transmittance above one half) can be zero for a Gaussian that did blend, so there only the culled ones are idle.
    culled = out["radii"] == 0
    assert bool((out["contributions"][culled] == 0).all())
    idle = (out["contributions"] == 0) if mode == "surfel" else culled
    if bool(idle.any()):
        for k in PER_GAUSSIAN:
            assert int(_bits(out[k])[idle].abs().max()) == 0, k
    assert int(_bits(out["d_means2D"])[:, 2].abs().max()) == 0

    if kind == "behind":
        assert fs.I == 0 and int((out["radii"] != 0).sum()) == 0
        assert int(_bits(out["d_tau"]).abs().max()) == 0
    if kind == "alternating":
        assert int((out["radii"][0::2] != 0).sum()) == 0 and int((out["radii"][1::2] > 0).sum()) > 0
    if kind == "small":
        assert int((out["radii"] > 0).sum()) == P
    if kind == "occluders":
        # every tile saturates behind the four sheets, so survivors that keep no tile exist
        _, bsat, nb = hr.debug_occlusion(fs)
        assert bool((bsat != 0xFFFF).all()) and int(bsat.max()) < nb - 1
        owners = torch.unique(hr.debug_lists(fs)[0])
        assert owners.numel() < int((out["radii"] > 0).sum())
    if kind == "cover":
        # the covering surfel owns a row in every one of the 70 tiles: two chunks of CH = 64 rows in the tile plan,
        # five (a row per quadrant) in the scan plan
        owners = hr.debug_lists(fs)[0]
        assert int((owners == sc["big"][0]).sum()) == 70
        assert float(out["d_colors"][sc["big"][0]].abs().max()) > 0
        if mode == "surfel":
            assert float(out["contributions"][sc["big"][0]]) > 0

    # two runs, one workgroup striding over all (Gaussian, chunk) pairs, the library depth sort: the same bits
    again, _ = _run(sc, mode, ups)
    _assert_same_bits(out, again, "second run")
    monkeypatch.setenv("PINGS_ROWSUM_WGS", "1")
    one_wg, _ = _run(sc, mode, ups)
    _assert_same_bits(out, one_wg, "PINGS_ROWSUM_WGS=1")
    monkeypatch.delenv("PINGS_ROWSUM_WGS")
    monkeypatch.setenv("PINGS_DEPTH_SORT", "l")
    lib_sort, _ = _run(sc, mode, ups)
    _assert_same_bits(out, lib_sort, "PINGS_DEPTH_SORT=l")

    if ref is None:
        return
    o64, o32, names, ref64, ref32, _ = ref
    assert (out["radii"].cpu() == o32["radii"]).all()
    if mode == "surfel":
        assert rel_err(out["contributions"], o64["contributions"]) <= 1e-4
    else:
        assert (out["contributions"].cpu() == o32["n_touched"]).all()
    got = [out["d_means3D"], out["d_colors"], out["d_opacities"], out["d_scales"], out["d_rotations"],
           out["d_tau"][3:], out["d_tau"][:3]]
    assert names == ["means", "col", "op", "scales", "rot", "theta", "rho"]
    _assert_grad_gate(names, got, ref64, ref32, f"{kind} P={P} {W}x{H} {mode} {plan}")
