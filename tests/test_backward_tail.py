"""The tail of the raster backward behind the pixel-per-lane blend: the zeros of the six per-Gaussian gradient arrays,
written by trailing workgroups of the blend launch (PINGS_GRAD_FILL=l: by grad_zero_kernel, a launch of its own), and
the sums of an owner's chunk partials in gaussian_bwd_rank_kernel, formed by 16-lane groups (PINGS_CHAIN_SUM=l: by the
owner's lane alone).  Driven through the C ABI by the helpers of test_gaussian_passes.py, every output pre-filled with
0xFFFFFFFF words, both modes, the pixel plan forced the way that file forces it.

Fill: array sizes below the number of fill slices and above the number of tiles, the six gradient pointers at offsets
of 0 .. 3 floats inside larger NaN buffers (the 1-float and 3-float arrays then take the head-only and tail-only
paths), and a frame without instances, which has no blend launch.  Chain sums: one screen-filling surfel owns one live
row per tile, so the image size sets the length of its loop over chunk partials (1, 2, 8, 9, 16, 18: around the rows
a lane and a group keep in flight), and a scene whose two long loops cross pair 256 and pair 512, the workgroup
boundaries.  The knobs' other branch must give the same bits; the sizes up to 160x112 also pass the fp64 oracle
gates of test_gaussian_passes.py."""
import functools
import math

import pytest
import torch

import test_gaussian_passes as gp
from oracle import raster_cpu as R
from scenes import hip_settings, random_pose
from test_gaussian_passes import PER_GAUSSIAN, _assert_same_bits, _bits, _run
from test_raster import _assert_grad_gate, _oracle_grads

CH = 64   # gradient rows per chunk partial (raster_common.hpp)


def _scene(W, H, P, mode, seed, covers=(), behind=False, pose=True, near=None):
    """fp64 scene dict (tests/scenes.py layout): P - len(covers) small Gaussians, and screen-filling surfels `covers` =
    ((index, z, opacity), ...) centred off the image.  near = ((index range, z_lo, z_hi), ...) puts small Gaussians
    that face the camera in a depth band."""
    g = torch.Generator().manual_seed(seed)
    f64 = torch.float64
    fx = fy = 0.9 * W
    T_cw = random_pose(g) if pose else torch.eye(4, dtype=f64)
    cam = R.look_at_camera(W, H, fx, fy, 0.5 * W - 1.7, 0.5 * H + 0.9, 0.05, 100.0, T_cw=T_cw, dtype=f64)
    r = lambda *s: torch.rand(*s, generator=g, dtype=f64)
    z = 2.5 + 6.5 * r(P)
    scales = torch.exp(math.log(0.02) + (math.log(0.15) - math.log(0.02)) * r(P, 3))
    rot = torch.nn.functional.normalize(torch.randn(P, 4, generator=g, dtype=f64), dim=1)
    op = 0.05 + 0.95 * r(P, 1)
    for idx, lo, hi in (near or ()):
        z[idx] = lo + (hi - lo) * r(len(z[idx]))
        scales[idx] = 0.004 + 0.004 * r(len(z[idx]), 3)   # a few tiles each: one chunk
        rot[idx] = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=f64)
        op[idx] = 0.3 + 0.3 * r(len(z[idx]), 1)
    x = (r(P) - 0.5) * 0.8 * W / fx * z
    y = (r(P) - 0.5) * 0.8 * H / fy * z
    if behind:
        z = -z
    for k, (i, zi, oi) in enumerate(covers):
        x[i], y[i], z[i] = (3.0 if k & 1 else -3.0), (2.0 if k & 2 else -2.0), zi
        op[i] = oi
        scales[i] = torch.tensor([30.0, 30.0, 0.01], dtype=f64)
        rot[i] = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=f64)
    if mode == "surfel":
        scales[:, 2] = 1e-7
    T_wc = torch.linalg.inv(T_cw)
    means = torch.stack([x, y, z], 1) @ T_wc[:3, :3].T + T_wc[:3, 3]
    return dict(means=means, scales=scales, rot=rot, op=op, col=r(P, 3), bg=torch.tensor([1.0, 0.9, 0.8], dtype=f64),
                cam=cam, W=W, H=H)


def _ups(W, H, seed=5):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(c, H, W, generator=g, dtype=torch.float64) for c in (3, 3, 1, 1))


def _idle(out, mode):
    """Gaussians without a live row, as test_gaussian_passes.py tells them"""
    return (out["contributions"] == 0) if mode == "surfel" else (out["radii"] == 0)


# ------------------------------------------------------------------ the zero fill
class _Guarded:
    """Stands in for test_gaussian_passes._nan: a gradient array (the two-dimensional requests of _run) becomes a view at
    4 + `offset` floats into a larger buffer of 0xFFFFFFFF words, so its first byte sits `offset` floats behind a
    16-byte boundary."""
    FRONT, BACK = 4, 8

    def __init__(self, offset):
        self.offset, self.bufs, self.plain = offset, [], gp._nan

    def __call__(self, *shape, dtype=torch.float32):
        if len(shape) != 2:
            return self.plain(*shape, dtype=dtype)
        n, at = shape[0] * shape[1], self.FRONT + self.offset
        big = self.plain(n + at + self.BACK)
        assert big.data_ptr() % 16 == 0
        self.bufs.append((big, at, n))
        return big[at:at + n].view(*shape)

    def assert_guards_kept(self):
        assert len(self.bufs) == 6
        for big, at, n in self.bufs:
            words = _bits(big)
            assert bool((words[:at] == -1).all()) and bool((words[at + n:] == -1).all())


def _run_guarded(monkeypatch, sc, mode, ups, offset):
    guard = _Guarded(offset)
    monkeypatch.setattr(gp, "_nan", guard)
    try:
        out, fs = _run(sc, mode, ups)
    finally:
        monkeypatch.setattr(gp, "_nan", guard.plain)
    guard.assert_guards_kept()
    return {k: t.clone() for k, t in out.items()}, fs


def _check_fill(monkeypatch, sc, mode, expect_instances):
    monkeypatch.setenv("PINGS_BLEND_BWD", "pixel")
    ups = _ups(sc["W"], sc["H"])
    for offset in range(4):
        monkeypatch.delenv("PINGS_GRAD_FILL", raising=False)
        out, fs = _run_guarded(monkeypatch, sc, mode, ups, offset)
        assert (fs.I > 0) == expect_instances
        for k, t in out.items():
            if t.dtype.is_floating_point:
                assert not torch.isnan(t).any(), (k, "NaN left", offset)
        idle = _idle(out, mode)
        if bool(idle.any()):
            for k in PER_GAUSSIAN:
                assert int(_bits(out[k])[idle].abs().max()) == 0, (k, offset)
        if not expect_instances:
            assert bool(idle.all()) and int(_bits(out["d_tau"]).abs().max()) == 0
        again, _ = _run_guarded(monkeypatch, sc, mode, ups, offset)
        _assert_same_bits(out, again, f"second run, offset {offset}")
        monkeypatch.setenv("PINGS_GRAD_FILL", "l")
        own_launch, _ = _run_guarded(monkeypatch, sc, mode, ups, offset)
        _assert_same_bits(out, own_launch, f"PINGS_GRAD_FILL=l, offset {offset}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["surfel", "3dgs"])
@pytest.mark.parametrize("P", [1, 2, 3, 13, 257, 4099])
@pytest.mark.parametrize("W,H", [(16, 16), (64, 48)])
def test_fill_in_blend_launch(W, H, P, mode, monkeypatch):
    # a covering surfel of opacity 0.3 at index 0, so that the smallest scenes have instances too
    _check_fill(monkeypatch, _scene(W, H, P, mode, seed=100 * P + W, covers=((0, 1.5, 0.3),)), mode, expect_instances=True)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["surfel", "3dgs"])
def test_fill_without_instances(mode, monkeypatch):
    """every Gaussian behind the camera: I == 0, no blend launch, the fill kernel runs"""
    _check_fill(monkeypatch, _scene(64, 48, 13, mode, seed=3, behind=True), mode, expect_instances=False)


# ------------------------------------------------------------------ the chain's sums of chunk partials
def _pair_off(sc, mode):
    """pair_off[P + 1] of the chunk scan (by depth rank), read out of the backward blob where tools/frame_counts.py
    reads it: carve_bwd puts cidx[I + 2] first and pair_off behind it, each field on a 256-byte boundary."""
    from pings_amd import _lib
    from pings_amd import rasterizer as hr

    L = _lib.lib()
    dev = torch.device("cuda")
    prep = hr._Prepared(hip_settings(sc, mode, gp.FRONT_ONLY), hr.MODE_SURFEL if mode == "surfel" else hr.MODE_3DGS)
    d = lambda t: t.to(torch.float32).to(dev).contiguous()
    fs, _, _ = hr._forward(prep, *(d(sc[k]) for k in ("means", "col", "op", "scales", "rot")))
    P, I = fs.P, fs.I
    ups = [d(t) for t in _ups(sc["W"], sc["H"])]
    scratch = torch.empty(L.pings_raster_backward_bytes(P, I), dtype=torch.uint8, device=dev)
    grads = [torch.empty(P, c, dtype=torch.float32, device=dev) for c in (3, 3, 3, 1, 3, 4)]
    d_tau = torch.empty(6, dtype=torch.float32, device=dev)
    _lib.check(L.pings_raster_backward(
        prep.ref(), P, I, _lib.ptr(fs.means3D), _lib.ptr(fs.colors), _lib.ptr(fs.opacities), _lib.ptr(fs.scales),
        _lib.ptr(fs.rotations), _lib.ptr(fs.geom), _lib.ptr(fs.binning), _lib.ptr(fs.image), _lib.ptr(fs.color),
        _lib.ptr(fs.normal), _lib.ptr(fs.depth), _lib.ptr(fs.alpha), _lib.ptr(ups[0]),
        _lib.ptr(ups[1]) if mode == "surfel" else None, _lib.ptr(ups[2]), _lib.ptr(ups[3]), _lib.ptr(scratch),
        *[_lib.ptr(t) for t in grads], _lib.ptr(d_tau), fs.fclass, _lib.stream_ptr(dev)), "pings_raster_backward")
    torch.cuda.synchronize()
    at = (4 * (I + 2) + 255) // 256 * 256
    return scratch[at:at + 4 * (P + 1)].view(torch.int32).long().cpu()


def _check_chain(monkeypatch, sc, mode, ups):
    monkeypatch.delenv("PINGS_CHAIN_SUM", raising=False)
    out, _ = _run(sc, mode, ups)
    for k, t in out.items():
        if t.dtype.is_floating_point:
            assert not torch.isnan(t).any(), (k, "NaN left")
    again, _ = _run(sc, mode, ups)
    _assert_same_bits(out, again, "second run")
    monkeypatch.setenv("PINGS_CHAIN_SUM", "l")
    by_lane, _ = _run(sc, mode, ups)
    _assert_same_bits(out, by_lane, "PINGS_CHAIN_SUM=l")
    monkeypatch.delenv("PINGS_CHAIN_SUM")
    return out


@functools.lru_cache(maxsize=None)
def _loop_reference(W, H, mode):
    """The one-cover scene and, up to 160x112, its oracle gradients: computed once, never modified."""
    sc = _scene(W, H, 14, mode, seed=W + H, covers=((7, 1.5, 0.3),))
    if W * H > 160 * 112:
        return sc, _ups(W, H), None
    _, names, ref64, ups = _oracle_grads(sc, torch.float64, mode, gp.FRONT_ONLY)
    _, _, ref32, _ = _oracle_grads(sc, torch.float32, mode, gp.FRONT_ONLY)
    return sc, ups, (names, [t.detach() for t in ref64], [t.detach() for t in ref32])


# image size -> tiles -> chunk partials of the covering surfel
LOOPS = [(64, 48, 1), (160, 112, 2), (512, 256, 8), (528, 272, 9), (1024, 256, 16), (1040, 272, 18)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["surfel", "3dgs"])
@pytest.mark.parametrize("W,H,partials", LOOPS)
def test_chain_sum_loop_lengths(W, H, partials, mode, monkeypatch):
    monkeypatch.setenv("PINGS_BLEND_BWD", "pixel")
    sc, ups, ref = _loop_reference(W, H, mode)
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    assert (tiles + CH - 1) // CH == partials
    pair_off = _pair_off(sc, mode)
    chunks = pair_off[1:] - pair_off[:-1]
    # the cover is the nearest Gaussian: depth rank 0, one live row per tile
    assert int(chunks[0]) == partials and int(chunks.max()) == partials and int((chunks > 0).sum()) > 1
    out = _check_chain(monkeypatch, sc, mode, ups)
    assert float(out["d_colors"][7].abs().max()) > 0
    if ref is None:
        return
    names, ref64, ref32 = ref
    got = [out["d_means3D"], out["d_colors"], out["d_opacities"], out["d_scales"], out["d_rotations"],
           out["d_tau"][3:], out["d_tau"][:3]]
    assert names == ["means", "col", "op", "scales", "rot", "theta", "rho"]
    _assert_grad_gate(names, got, ref64, ref32, f"cover {W}x{H} {mode}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["surfel", "3dgs"])
def test_chain_sum_across_workgroups(mode, monkeypatch):
    """248 small Gaussians, a cover (16 partials), 240 small Gaussians, a second cover: the two long loops start in
    one workgroup of 256 pairs and end in the next."""
    monkeypatch.setenv("PINGS_BLEND_BWD", "pixel")
    W, H, P = 1024, 256, 490
    sc = _scene(W, H, P, mode, seed=11, covers=((488, 1.5, 0.3), (489, 2.0, 0.3)), pose=False,
                near=((slice(0, 248), 1.0, 1.4), (slice(248, 488), 1.6, 1.9)))
    pair_off = _pair_off(sc, mode)
    chunks = pair_off[1:] - pair_off[:-1]
    long_ranks = torch.nonzero(chunks == 16).flatten().tolist()
    assert len(long_ranks) == 2 and int(chunks.max()) == 16 and int(pair_off[P]) > 512
    for rank, boundary in zip(long_ranks, (256, 512)):
        assert int(pair_off[rank]) < boundary < int(pair_off[rank + 1]), (rank, boundary, pair_off[rank:rank + 2])
    out = _check_chain(monkeypatch, sc, mode, _ups(W, H))
    assert float(out["d_colors"][488].abs().max()) > 0 and float(out["d_colors"][489].abs().max()) > 0
