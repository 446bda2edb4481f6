"""The camera frame front-end on the device (pings_amd/camfront_ops.py, csrc/camfront.hip).

Gates:
  pyramid       every level bit-equal to the chain of `F.interpolate` run by torch ON THE SAME DEVICE from the same level
                0 (that is what the reference executes); level 0 of a uint8 image equal to float32(u) / float32(255)
                formed by numpy (IEEE division), of a float image to `torch.clamp` on the device.  One launch (the
                library's out-parameter), no host read (`_lib.sync_counts`).
  constructor   flags, shapes and `cur_best_level` of tests/golden/camfront_cam.npz (the reference's own constructor on
                the CPU); depth and sky levels equal, RGB and normal levels to the project's 1e-4 relative gate, since
                torch's CPU kernel sums the four 0.25-weighted terms serially and differs in the last bit.
  fit           count exact; k and b within 1e-8 (relative) of `np.polyfit` in float64, a bound derived in the test; the
                two rmse figures within 1e-4
  cloud         exact cases (one pixel at and on each side of every threshold): rows, sky mask and gated depth bit-equal
                to the float64 restatement.  Random case: the dense outputs equal outside the pixels within 1e-5
                (relative) of a threshold, at most 0.1 % of them; rows at 1e-4 on an input nudged until none is undecided
  voxel average count and order exact, values at 1e-4, on points kept 1e-3 voxel away from every cell face; two runs
                bit-equal; the extent and the capacity status bits
  mono_frame    one host read; bit-equal to the stage functions chained by hand; the cloud is assigned as the reference
                assigns it
Every reference is computed on the CPU once per case (tests/camfront_ref.py).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import camfront_ref as CR
from conftest import GOLDEN, rel_err
from pings_amd import _abi, _lib, camfront_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE_H, TILE_W = _abi.CAMFRONT_TILE_H, _abi.CAMFRONT_TILE_W
# the edge sizes of the issue, two tiles and a rest, and one width the 16-byte path takes (two tiles wide and high)
SIZES = [(8, 8), (9, 15), (15, 9), (33, 70), (2 * TILE_H + 9, 2 * TILE_W + 15), (TILE_H + 8, TILE_W + 16)]


def _reads(fn):
    _lib.sync_counts(reset=True)
    out = fn()
    return out, _lib.sync_counts(reset=True)


def _same(a, b):
    """Bit-equal, NaNs in the same places."""
    return (a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.isnan(a), torch.isnan(b))
            and torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)))


def _chain(level0, mode):
    out = [level0]
    for _ in range(3):
        x = out[-1].float().unsqueeze(0)
        kw = dict(align_corners=False) if mode == "bilinear" else {}
        out.append(F.interpolate(x, scale_factor=0.5, mode=mode, **kw).squeeze(0).to(level0.dtype))
    return out


def _check_levels(got, want, first_level, H, W, channels):
    for k in range(4):
        if k < first_level:
            assert got[k] is None
            continue
        assert tuple(got[k].shape) == (channels, H >> k, W >> k) and got[k].is_contiguous()
        assert got[k].untyped_storage().nbytes() == got[k].numel() * got[k].element_size()     # a tensor of its own
        assert _same(got[k], want[k]), k


def _inputs(H, W, seed):
    u8, depth, sky, normal = CR.example(H, W, seed)
    return (torch.from_numpy(u8).to(DEV), torch.from_numpy(depth).to(DEV), torch.from_numpy(sky).to(DEV),
            torch.from_numpy(normal).to(DEV), torch.from_numpy(CR.u8_level0(u8)).to(DEV))


def _float_image(H, W, seed, permuted):
    g = torch.Generator().manual_seed(seed)
    hwc = torch.rand(H, W, 3, generator=g) * 1.5 - 0.25                      # below 0 and above 1
    hwc[H // 2, W // 3, 1] = float("nan")
    hwc[0, 0, 0], hwc[H - 1, W - 1, 2] = -0.0, 1.0
    hwc = hwc.to(DEV)
    return hwc.permute(2, 0, 1) if permuted else hwc.permute(2, 0, 1).contiguous()


# ================================================================ pyramid
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("first_level", [0, 1, 3])
def test_uint8_image_with_every_map(H, W, first_level):
    u8, depth, sky, normal, l0 = _inputs(H, W, seed=H + W)
    if H * W * 3 >= 4096:
        assert torch.unique(u8).numel() == 256
    (rgb_l, depth_l, sky_l, normal_l), reads = _reads(
        lambda: camfront_ops.image_pyramid(u8, depth, sky, normal, first_level=first_level))
    assert reads == {} and camfront_ops.last_launches == 1
    _check_levels(rgb_l, _chain(l0, "bilinear"), first_level, H, W, 3)
    _check_levels(normal_l, _chain(normal, "bilinear"), first_level, H, W, 3)
    _check_levels(depth_l, _chain(depth, "nearest-exact"), first_level, H, W, 1)
    _check_levels(sky_l, _chain(sky, "nearest"), first_level, H, W, 1)
    if first_level == 0:                                                     # level 0 is the input object itself
        assert depth_l[0] is depth and sky_l[0] is sky and normal_l[0] is normal
        assert rgb_l[0].min() >= 0.0 and rgb_l[0].max() <= 1.0


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("permuted", [True, False])
def test_float_image_is_clamped_and_a_nan_stays(H, W, permuted):
    rgb = _float_image(H, W, seed=3 * H + W, permuted=permuted)
    assert rgb.is_contiguous() != permuted and (rgb < 0).any() and (rgb > 1).any()
    before = rgb.clone()
    (rgb_l, depth_l, sky_l, normal_l), reads = _reads(lambda: camfront_ops.image_pyramid(rgb))
    assert reads == {} and camfront_ops.last_launches == 1
    assert depth_l == sky_l == normal_l == [None] * 4
    assert _same(rgb, before) and rgb_l[0] is not rgb                         # the input is left alone
    want = _chain(before.clamp(0.0, 1.0).contiguous(), "bilinear")
    assert torch.isnan(want[0]).sum() == 1 and torch.isnan(rgb_l[0]).sum() == 1
    _check_levels(rgb_l, want, 0, H, W, 3)


def test_maps_may_be_absent_one_by_one():
    H, W = 33, 70
    u8, depth, sky, normal, l0 = _inputs(H, W, seed=1)
    for keep in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1)):
        args = [m if on else None for m, on in zip((depth, sky, normal), keep)]
        lists = camfront_ops.image_pyramid(u8, *args)
        assert camfront_ops.last_launches == 1
        _check_levels(lists[0], _chain(l0, "bilinear"), 0, H, W, 3)
        for got, src, on, mode, ch in zip(lists[1:], (depth, sky, normal), keep, ("nearest-exact", "nearest", "bilinear"),
                                          (1, 1, 3)):
            if on:
                _check_levels(got, _chain(src, mode), 0, H, W, ch)
            else:
                assert got == [None] * 4


@pytest.mark.parametrize("H,W", [(33, 70), (TILE_H + 8, TILE_W + 16)])
def test_strided_views_of_the_planar_maps(H, W):
    """depth, sky mask and normal as views with a row pitch: level 0 stays the view, the levels below are contiguous."""
    _, depth, sky, normal, _ = _inputs(H, W, seed=2)
    wide = lambda t: torch.cat([t, t.flip(2)], dim=2)[:, :, :W]              # noqa: E731  row pitch 2 W
    d, s, n = wide(depth), wide(sky), wide(normal)
    assert not d.is_contiguous() and not n.is_contiguous()
    rgb = _float_image(H, W, seed=9, permuted=True)
    _, depth_l, sky_l, normal_l = camfront_ops.image_pyramid(rgb, d, s, n)
    assert depth_l[0] is d and sky_l[0] is s and normal_l[0] is n
    for got, want in ((depth_l, _chain(depth, "nearest-exact")), (sky_l, _chain(sky, "nearest")),
                      (normal_l, _chain(normal, "bilinear"))):
        for k in range(1, 4):
            assert got[k].is_contiguous() and _same(got[k], want[k])


def test_two_cameras_of_different_sizes_share_one_launch():
    a = _inputs(2 * TILE_H + 9, 2 * TILE_W + 15, seed=4)
    b = _inputs(TILE_H + 8, TILE_W + 16, seed=5)
    rgb_b = _float_image(9, 15, seed=6, permuted=True)
    frames = [(a[0], a[1], a[2], a[3]), (b[0], None, b[2], None), (rgb_b,)]
    out, reads = _reads(lambda: camfront_ops.image_pyramids(frames))
    assert reads == {} and camfront_ops.last_launches == 1 and len(out) == 3
    for (rgb_l, depth_l, sky_l, normal_l), src in zip(out[:2], (a, b)):
        H, W = src[0].shape[:2]
        _check_levels(rgb_l, _chain(src[4], "bilinear"), 0, H, W, 3)
        _check_levels(sky_l, _chain(src[2], "nearest"), 0, H, W, 1)
    _check_levels(out[0][1], _chain(a[1], "nearest-exact"), 0, *a[0].shape[:2], 1)
    _check_levels(out[0][3], _chain(a[3], "bilinear"), 0, *a[0].shape[:2], 3)
    assert out[1][1] == out[1][3] == [None] * 4
    _check_levels(out[2][0], _chain(rgb_b.clamp(0.0, 1.0).contiguous(), "bilinear"), 0, 9, 15, 3)
    again = camfront_ops.image_pyramids(frames)                               # bitwise the same from run to run
    for x, y in zip(out, again):
        for lx, ly in zip(x, y):
            assert all((p is None and q is None) or _same(p, q) for p, q in zip(lx, ly))


def test_inputs_the_kernel_does_not_take_raise():
    ok = torch.zeros(3, 8, 8, device=DEV)
    for bad in (torch.zeros(3, 7, 8, device=DEV), torch.zeros(3, 8, 8, device=DEV, dtype=torch.float64),
                torch.zeros(8, 8, 3, device=DEV, dtype=torch.uint8)[:, ::2], torch.zeros(3, 8, 8)):
        with pytest.raises(_lib.PingsHipError):
            camfront_ops.image_pyramid(bad)
    with pytest.raises(_lib.PingsHipError):
        camfront_ops.image_pyramid(ok, depth=torch.zeros(1, 8, 9, device=DEV))
    with pytest.raises(_lib.PingsHipError):
        camfront_ops.image_pyramid(ok, sky_mask=torch.zeros(1, 8, 8, device=DEV))          # not bool
    with pytest.raises(_lib.PingsHipError):
        camfront_ops.image_pyramids([(ok,)] * 9)
    assert camfront_ops.image_pyramid(ok, first_level=4)[0] == [None] * 4 and camfront_ops.last_launches == 0


# ================================================================ the constructor
@pytest.fixture()
def cam_cls():
    camfront_ops.install(cam_cls=CR.Cam)
    yield CR.Cam
    camfront_ops.uninstall(cam_cls=CR.Cam)


@pytest.mark.parametrize("rate", [0, 1])
@pytest.mark.parametrize("as_uint8", [True, False])
def test_rebound_constructor_gives_the_fixture(cam_cls, rate, as_uint8):
    with np.load(GOLDEN / "camfront_cam.npz") as z:
        z = {k: np.asarray(z[k]) for k in z.files}
    for H, W, seed in z["sizes"]:
        H, W = int(H), int(W)
        u8, depth, sky, normal, l0 = _inputs(H, W, int(seed))
        rgb = u8 if as_uint8 else (u8.float() / 255.0).permute(2, 0, 1)
        cam, reads = _reads(lambda: cam_cls(7, rgb, z["K"], cam_id="cam0", img_down_rate=rate, depth_image=depth,
                                            normal_img=normal, sky_mask=sky, device=DEV))
        tag = f"{H}x{W}.r{rate}"
        assert reads == {} and not cam.fell_back and (cam.image_height, cam.image_width) == (H, W)
        assert [cam.depth_on, cam.sky_mask_on, cam.mono_normal_on] == z[f"{tag}.flags"].tolist()
        assert cam.cur_best_level == int(z[f"{tag}.cur_best_level"])
        for name, ls in (("rgb", cam.rgb_image_list), ("depth", cam.depth_image_list), ("sky", cam.sky_mask_list),
                         ("normal", cam.normal_img_list)):
            assert [lv is not None for lv in ls] == z[f"{tag}.{name}.present"].tolist()
            for k, lv in enumerate(ls):
                if lv is None:
                    continue
                ref = torch.from_numpy(z[f"{tag}.{name}.{k}"])
                assert tuple(lv.shape) == tuple(ref.shape) and lv.dtype == ref.dtype and lv.is_contiguous()
                if name in ("depth", "sky"):
                    assert torch.equal(lv.cpu(), ref)
                else:
                    assert rel_err(lv, ref) <= 1e-4
        if rate == 0:
            assert cam.depth_image_list[0] is depth and cam.rgb_image_list[0].is_contiguous()
        held = cam.rgb_image_list[1].untyped_storage().nbytes()
        assert held == 3 * (H >> 1) * (W >> 1) * 4                            # freeing a level frees its memory


def test_constructor_fallbacks_on_the_device(cam_cls):
    K = np.eye(3)
    assert cam_cls(1, torch.rand(3, 7, 16, device=DEV), K, device=DEV).fell_back              # under 8 x 8
    assert cam_cls(1, torch.rand(3, 16, 16, device=DEV), K, device=DEV, pyramid_level=3).fell_back
    assert cam_cls(1, torch.rand(3, 16, 16, device=DEV).half(), K, device=DEV).fell_back
    assert cam_cls(1, torch.rand(3, 16, 16), K, device=DEV).fell_back                         # a CPU image
    assert not cam_cls(1, torch.rand(3, 16, 16, device=DEV), K, device=DEV).fell_back


# ================================================================ the fit
RANGE = dict(min_range=2.75, max_range=60.0)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def test_fit_matches_polyfit():
    """k and b to 1e-8: float64 sums of positive terms in another order differ by at most n 2^-53 relative, the slope
    amplifies that by E[x^2] / Var[x] (about 4 here), which is under 1e-10 at n < 2^12; two orders of margin."""
    pred, lidar = CR.fit_example()
    n, k, b, before, after = CR.align(pred, lidar, **RANGE)
    assert 300 < n < 2 ** 12
    rec, reads = _reads(lambda: camfront_ops.align_mono_depth(_dev(pred)[None], _dev(lidar)[None], **RANGE))
    assert reads == {} and rec.dtype is torch.float64 and tuple(rec.shape) == (_abi.CAMFRONT_FIT_RECORD,)
    got = rec.tolist()
    print("fit", got, (n, k, b, before, after))
    assert got[0] == n
    assert abs(got[1] - k) <= 1e-8 * abs(k) and abs(got[2] - b) <= 1e-8 * abs(b)
    assert abs(got[3] - before) <= 1e-4 * before and abs(got[4] - after) <= 1e-4 * after
    again = camfront_ops.align_mono_depth(_dev(pred), _dev(lidar), **RANGE)
    assert torch.equal(rec, again)


@pytest.mark.parametrize("valid", [0, 100, 101])
def test_fit_needs_more_than_100_pixels(valid):
    pred, lidar = CR.fit_example(seed=1, valid=valid)
    n, k, b, before, after = CR.align(pred, lidar, **RANGE)
    assert n == valid
    got = camfront_ops.align_mono_depth(_dev(pred), _dev(lidar), **RANGE).tolist()
    assert got[0] == valid
    if valid <= 100:
        assert got[1] == 1.0 and got[2] == 0.0 and np.isnan(got[4])
        assert np.isnan(got[3]) if valid == 0 else abs(got[3] - before) <= 1e-4 * before
    else:
        assert abs(got[1] - k) <= 1e-8 * abs(k) and abs(got[2] - b) <= 1e-8 * abs(b)
        assert abs(got[4] - after) <= 1e-4 * after


def test_fit_over_more_pixels_than_one_pass_of_the_partial_grid():
    """300 x 300 pixels: more than 256 workgroups of 256, so the grid-stride loop runs twice for some."""
    rng = np.random.default_rng(3)
    pred = rng.uniform(1.0, 80.0, (300, 300)).astype(np.float32)
    lidar = (0.93 * pred + 1.5 + rng.normal(0.0, 0.3, pred.shape)).astype(np.float32)
    n, k, b, before, after = CR.align(pred, lidar, **RANGE)
    got = camfront_ops.align_mono_depth(_dev(pred), _dev(lidar), **RANGE).tolist()
    assert got[0] == n > 30000
    assert abs(got[1] - k) <= 1e-8 * abs(k) and abs(got[2] - b) <= 1e-8 * abs(b)       # n 2^-53 * 4 < 1e-10 still
    assert abs(got[3] - before) <= 1e-4 * before and abs(got[4] - after) <= 1e-4 * after


# ================================================================ the cloud
def _record(k, b):
    return torch.tensor([1000.0, k, b, 0.0, 0.0], dtype=torch.float64, device=DEV)


def _pred_for(d, k, b):
    """A float32 prediction whose fitted depth is exactly the float32 d."""
    p = np.float32((np.float64(d) - b) / k)
    assert CR.fitted_depth(np.array([p]), k, b)[0] == np.float32(d)
    return p


@pytest.mark.parametrize("high_z", [True, False])
def test_cloud_exact_cases_are_bitwise(high_z):
    """min_range 2, max_range 40, depth_trunc 24: thresholds 48 (sky), 32 and 4 (high_z) or 8, and 24; one pixel at,
    one below and one above each; k = 1.25, b = -0.5 as the record; K and T_c_l dyadic."""
    k, b, lim = 1.25, -0.5, dict(min_range=2.0, max_range=40.0, depth_trunc=24.0)
    depths = [t + s for t in (48.0, 32.0, 24.0, 8.0, 4.0) for s in (-0.25, 0.0, 0.25)] + [0.5, -1.0, 16.0, 100.0]
    H, W = 3, len(depths)
    pred = np.stack([np.array([_pred_for(d, k, b) for d in depths], np.float32)] * H)
    pred[2, 5] = np.nan
    u8 = (np.arange(H * W * 3) * 7 % 256).astype(np.uint8).reshape(H, W, 3)
    K = np.array([[4.0, 0.0, 2.5], [0.0, 8.0, 1.25], [0.0, 0.0, 1.0]])
    T = np.array([[0.0, -1.0, 0.0, 0.5], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 1.0, 0.25], [0.0, 0.0, 0.0, 1.0]])
    rows, sky, gated, _ = CR.mono_cloud(pred, u8, K, T, high_z=high_z, k=k, b=b, **lim)
    near = 4.0 if high_z else 8.0
    want = [d if near <= d < 24.0 else None for d in depths]                # d == near stays, d == depth_trunc goes
    assert [None if g == 0 or g >= 24.0 else float(g) for g in gated[0]] == want        # the restatement itself
    assert sky[0].tolist() == [d > 48.0 for d in depths]
    (got_rows, count, got_sky, got_depth), reads = _reads(lambda: camfront_ops.mono_cloud(
        _dev(pred)[None], _dev(u8), K, T, high_z=high_z, record=_record(k, b), with_depth=True, **lim))
    assert reads == {}
    m = int(count)
    assert m == len(rows) == H * sum(w is not None for w in want) - (1 if want[5] is not None else 0)
    assert np.array_equal(got_sky.cpu().numpy()[0], sky) and got_sky.dtype is torch.bool
    assert np.array_equal(got_depth.cpu().numpy()[0], gated, equal_nan=True) and np.isnan(gated[2, 5])
    assert np.array_equal(got_rows[:m].cpu().numpy(), rows.astype(np.float32))


@pytest.mark.parametrize("high_z", [True, False])
@pytest.mark.parametrize("H,W", [(33, 70), (9, 15)])
def test_cloud_random_case(H, W, high_z):
    lim = dict(depth_trunc=50.0, **RANGE)
    k, b, T = 1.07, -0.6, CR.rig_pose(H)
    pred, u8, K = CR.cloud_example(H, W, seed=W, high_z=high_z, k=k, b=b, **lim)
    _, sky, gated, und = CR.mono_cloud(pred, u8, K, T, high_z=high_z, k=k, b=b, **lim)
    assert und.mean() <= 1e-3
    _, _, got_sky, got_depth = camfront_ops.mono_cloud(_dev(pred), _dev(u8), K, T, high_z=high_z, record=_record(k, b),
                                                       with_depth=True, **lim)
    ok = ~und
    assert np.array_equal(got_sky.cpu().numpy()[0][ok], sky[ok])
    assert np.array_equal(got_depth.cpu().numpy()[0][ok], gated[ok])
    assert 0.05 < sky.mean() < 0.6 and 0.1 < (gated > 0).mean() < 0.9
    # rows: an input nudged until no pixel is undecided
    pred, u8, K = CR.cloud_example(H, W, seed=W, high_z=high_z, k=k, b=b, nudge=True, **lim)
    rows, _, _, und = CR.mono_cloud(pred, u8, K, T, high_z=high_z, k=k, b=b, **lim)
    assert not und.any()
    got_rows, count, _, none = camfront_ops.mono_cloud(_dev(pred), _dev(u8), K, T, high_z=high_z, record=_record(k, b),
                                                       **lim)
    assert none is None and int(count) == len(rows) > 0 and tuple(got_rows.shape) == (H * W, 6)
    assert rel_err(got_rows[:len(rows), :3], torch.from_numpy(rows[:, :3])) <= 1e-4
    assert rel_err(got_rows[:len(rows), 3:], torch.from_numpy(rows[:, 3:])) <= 1e-4


def test_cloud_without_a_record_keeps_the_prediction():
    lim = dict(depth_trunc=50.0, **RANGE)
    pred, u8, K = CR.cloud_example(33, 70, seed=8, high_z=False, nudge=True, **lim)
    rows, sky, gated, _ = CR.mono_cloud(pred, u8, K, np.eye(4), high_z=False, **lim)
    got_rows, count, got_sky, got_depth = camfront_ops.mono_cloud(_dev(pred), _dev(u8), K, np.eye(4), high_z=False,
                                                                  with_depth=True, **lim)
    assert int(count) == len(rows)
    assert np.array_equal(got_depth.cpu().numpy()[0], gated) and np.array_equal(got_sky.cpu().numpy()[0], sky)
    kept = gated > 0
    assert np.array_equal(gated[kept], pred[kept])                           # k = 1, b = 0 changes no bit


# ================================================================ the coloured voxel average
VOXEL = 0.8


def _average_agrees(got, rows, voxel=VOXEL):
    want = CR.voxel_average(rows, voxel)
    assert tuple(got.shape) == want.shape                                    # count; the order shows in the values
    assert rel_err(got[:, :3], torch.from_numpy(want[:, :3])) <= 1e-4
    assert rel_err(got[:, 3:], torch.from_numpy(want[:, 3:])) <= 1e-4
    return want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_voxel_average_matches_the_restatement(n):
    rows = CR.voxel_rows(n, VOXEL, seed=n, extent=1.0 if n < 100 else 6.0)
    (out, count, status), reads = _reads(lambda: camfront_ops.voxel_average(_dev(rows), VOXEL))
    assert reads == {} and int(status) == 0
    m = int(count)
    want = _average_agrees(out[:m], rows)
    assert m == len(want) and (n < 60 or m < n)                              # cells hold several rows
    again = camfront_ops.voxel_average(_dev(rows), VOXEL)
    assert int(again[1]) == m and torch.equal(out[:m], again[0][:m])          # two runs bit-equal


def test_voxel_average_takes_a_device_count_and_appends_at_a_device_offset():
    a, b = CR.voxel_rows(700, VOXEL, seed=21), CR.voxel_rows(300, VOXEL, seed=22, extent=3.0)
    buf = torch.full((1000, 6), float("nan"), device=DEV)
    buf[:700] = _dev(a)
    live = torch.tensor([500], dtype=torch.int64, device=DEV)
    merged = torch.full((1500, 6), -7.0, device=DEV)
    (_, c1, s1), reads = _reads(lambda: camfront_ops.voxel_average(buf, VOXEL, n_dev=live, out=merged))
    _, c2, s2 = camfront_ops.voxel_average(_dev(b), VOXEL, out=merged, offset=c1)
    assert reads == {}
    m1, m2 = int(c1), int(c2)
    wa, wb = _average_agrees(merged[:m1], a[:500]), _average_agrees(merged[m1:m2], b)
    assert m1 == len(wa) and m2 == m1 + len(wb) and int(s1) == int(s2) == 0
    assert (merged[m2:] == -7.0).all()                                       # nothing behind the count is written
    small = torch.full((m1 + 5, 6), -7.0, device=DEV)                        # no room for every cell of b
    small[:m1] = merged[:m1]
    _, c3, s3 = camfront_ops.voxel_average(_dev(b), VOXEL, out=small, offset=c1)
    assert int(c3) == m1 + 5 and int(s3) == _abi.CAMFRONT_FULL
    assert torch.equal(small[:m1 + 5], merged[:m1 + 5])


def test_voxel_average_reports_an_extent_it_cannot_file():
    rows = np.zeros((4, 6), np.float32)
    rows[1, 0], rows[2, 1], rows[3, 2] = 3.0e6, 0.5, 0.5                     # 3e6 cells of 1 m on x: more than 2^21
    _, _, status = camfront_ops.voxel_average(_dev(rows), 1.0)
    assert int(status) & _abi.EVAL_EXTENT
    _, count, status = camfront_ops.voxel_average(_dev(rows), 2.0)           # 1.5e6 cells fit
    assert int(status) == 0 and int(count) == 2


# ================================================================ the frame
def _frame(last_valid=None, is_rgbd=False):
    cams, images, preds, lidars = [], {}, {}, {}
    for name, (H, W), seed in (("cam0", (9, 15), 31), ("cam1", (33, 70), 32)):  # cam0 has too few pixels for a fit
        pred, u8, K = CR.cloud_example(H, W, seed, 2.75, 60.0, 50.0, False)
        lidar = (1.07 * pred - 0.6).astype(np.float32)
        if name == "cam1" and last_valid is not None:
            ok = np.flatnonzero(CR.fit_mask(pred, lidar, 2.75, 60.0).reshape(-1))
            lidar.reshape(-1)[ok[last_valid:]] = 0.0
        cams.append((name, K, CR.rig_pose(seed)))
        images[name], preds[name], lidars[name] = _dev(u8), _dev(pred)[None], _dev(lidar)[None]
    return CR.Dataset(cams, is_rgbd=is_rgbd), images, preds, lidars


def test_mono_frame_is_the_stages_chained_with_one_read():
    ds, images, preds, lidars = _frame()
    ds.cam_names = ["cam0", "none", "cam1"]                                  # a camera without an image is skipped
    skies, reads = _reads(lambda: camfront_ops.mono_frame(ds, images, preds, lidars))
    assert reads == {"camfront_mono_frame": 1} and list(skies) == ["cam0", "cam1"]
    cfg, merged, offset = ds.config, torch.empty(33 * 70 + 9 * 15, 6, device=DEV), None
    for name in ("cam0", "cam1"):
        rec = camfront_ops.align_mono_depth(preds[name], lidars[name], cfg.min_range, cfg.max_range)
        assert (rec[0] > 100) == (name == "cam1")
        rows, count, sky, _ = camfront_ops.mono_cloud(preds[name], images[name], ds.K_mats[name], ds.T_c_l_mats[name],
                                                      cfg.min_range, cfg.max_range, cfg.local_map_radius, False, rec)
        _, offset, _ = camfront_ops.voxel_average(rows, cfg.vox_down_m, n_dev=count, out=merged, offset=offset)
        assert torch.equal(skies[name], sky) and tuple(sky.shape) == (1,) + tuple(preds[name].shape[-2:])
    cloud = ds.cur_point_cloud_mono_depth
    assert cloud.dtype is torch.float32 and tuple(cloud.shape) == (int(offset), 6) and int(offset) > 100
    assert torch.equal(cloud, merged[:int(offset)])
    assert cloud.untyped_storage().nbytes() == cloud.numel() * 4              # not a view of the frame's buffer


@pytest.mark.parametrize("last_valid,is_rgbd,assigned", [(100, False, False), (101, False, True), (None, True, False)])
def test_mono_frame_assigns_the_cloud_as_the_reference_does(last_valid, is_rgbd, assigned):
    ds, images, preds, lidars = _frame(last_valid, is_rgbd)
    skies, reads = _reads(lambda: camfront_ops.mono_frame(ds, images, preds, lidars))
    assert reads == {"camfront_mono_frame": 1} and len(skies) == 2
    assert (ds.cur_point_cloud_mono_depth is not None) == assigned


def test_mono_frame_without_lidar_depth_keeps_the_prediction_and_the_flag():
    ds, images, preds, _ = _frame()
    skies = camfront_ops.mono_frame(ds, images, preds, None, high_z=True)
    cfg, merged, offset = ds.config, torch.empty(33 * 70 + 9 * 15, 6, device=DEV), None
    for name in ("cam0", "cam1"):
        rows, count, sky, _ = camfront_ops.mono_cloud(preds[name], images[name], ds.K_mats[name], ds.T_c_l_mats[name],
                                                      cfg.min_range, cfg.max_range, cfg.local_map_radius, True)
        _, offset, _ = camfront_ops.voxel_average(rows, cfg.vox_down_m, n_dev=count, out=merged, offset=offset)
        assert torch.equal(skies[name], sky)
    assert torch.equal(ds.cur_point_cloud_mono_depth, merged[:int(offset)])
