"""fused SSIM (csrc/ssim.hip) at the edges of its launch geometry, in every forward x backward kernel pairing, on
content where fp32 cancels, and at the sizes the product runs — against the fp64 oracle (oracle/ssim_cpu.py).

The sliding-window kernels (`ssim_{fwd,bwd}_{sw,vf}_kernel`) give a wave a strip of 54 output columns and a band of
`ssim_plan().rb` rows; odd bands walk bottom-up, units are renumbered per XCD; the backward also has the LDS-tile
kernel `ssim_bwd_kernel`.  `sw_geometry` restates that
geometry (checked against the library's `pings_ssim_partials_count` without a GPU), and every sweep case first proves
from it the edge it claims to hit: a case that quietly stops hitting its edge fails there, not in a numeric gate."""
import functools
import os

import pytest
import torch

from conftest import rel_err
from oracle import ssim_cpu

# ------------------------------------------------------------------ the library's launch geometry, restated
SW_OUT = 54              # ssim.hip SW_OUT = 64 - 2 * HALO: output columns per wave (strip width)
HALO = 5                 # window radius
WAVES_PER_WG = 4         # 256-thread workgroups, one unit per wave
FILL_WAVES = 256 * 4 * 3  # ssim_plan(): want_bands = FILL_WAVES / (strips * planes)
RB_MIN = 16              # ssim_plan(): at least 16 rows per band (unless the image is shorter)
ENV = ("PINGS_SSIM_RB", "PINGS_SSIM_ALT", "PINGS_SSIM_FWD", "PINGS_SSIM_BWD")


def _cdiv(a, b):
    return -(-a // b)


def _atoi(s):
    """C atoi on the strings the tests set (optional sign, leading digits, 0 when there are none)."""
    s = s.strip()
    n = len(s) - len(s.lstrip("+-"))
    d = s[n:]
    k = len(d) - len(d.lstrip("0123456789"))
    return int(s[:n] + d[:k]) if k else 0


def sw_rows_per_band(planes, H, W, rb_env=None):
    """ssim.hip ssim_plan().rb: PINGS_SSIM_RB > 0 overrides (not clamped to H); else about three waves per SIMD."""
    if rb_env is not None and _atoi(rb_env) > 0:
        return _atoi(rb_env)
    strips = _cdiv(W, SW_OUT)
    want_bands = FILL_WAVES // (strips * planes)
    rb = _cdiv(H, want_bands if want_bands > 0 else 1)
    return min(max(rb, RB_MIN), H)


def sw_geometry(planes, H, W):
    """The sliding-window launch plan of pings_ssim_forward / _backward (ssim.hip ssim_plan()), reading PINGS_SSIM_RB
    and PINGS_SSIM_ALT like the library does."""
    rb = sw_rows_per_band(planes, H, W, os.environ.get("PINGS_SSIM_RB"))
    alt_env = os.environ.get("PINGS_SSIM_ALT")
    alt = True if alt_env is None else _atoi(alt_env) != 0
    strips, bands = _cdiv(W, SW_OUT), _cdiv(H, rb)
    units = planes * bands * strips
    nblk = (_cdiv(units, WAVES_PER_WG) + 7) & ~7       # a multiple of eight: the per-XCD renumbering
    return dict(planes=planes, H=H, W=W, rb=rb, alt=alt, strips=strips, bands=bands, units=units, nblk=nblk,
                up=[alt and (b & 1) == 1 for b in range(bands)],
                last_rows=H - (bands - 1) * rb, last_cols=W - (strips - 1) * SW_OUT)


# the edges a sweep case can claim; every one must be claimed by some case (test_sweep_covers_every_edge)
EDGES = {
    "one_band": lambda g: g["bands"] == 1,
    "one_strip": lambda g: g["strips"] == 1,
    "last_band_1row": lambda g: g["bands"] > 1 and g["last_rows"] == 1,
    "band_under_halo": lambda g: g["rb"] < HALO,                 # a band shorter than the 5-row halo
    "band_under_window": lambda g: g["rb"] < 2 * HALO + 1,      # ... than the 11-slot register ring
    "odd_bands_alt": lambda g: g["alt"] and g["bands"] >= 3 and g["bands"] % 2 == 1,
    "last_band_up_short": lambda g: g["up"][-1] and g["last_rows"] < g["rb"],   # a partial band that walks upwards
    "last_strip_1col": lambda g: g["strips"] > 1 and g["last_cols"] == 1,
    "units_not_mult4": lambda g: g["units"] % WAVES_PER_WG != 0,                  # a partly idle last workgroup
    "idle_workgroups": lambda g: g["nblk"] * WAVES_PER_WG - g["units"] >= WAVES_PER_WG,   # whole ones, from the x8
}
ALT_EDGES = {"odd_bands_alt", "last_band_up_short"}      # hit only with the alternation on (PINGS_SSIM_ALT != 0)

# (B, C, H, W, forced PINGS_SSIM_RB or None, edges claimed)
SWEEP = [
    (1, 1, 1, 1, None, {"one_band", "one_strip", "band_under_halo", "units_not_mult4", "idle_workgroups"}),
    (1, 1, 4, 10, None, {"one_band", "one_strip", "band_under_halo"}),
    (1, 3, 11, 55, 5, {"last_band_1row", "band_under_window", "odd_bands_alt", "last_strip_1col",
                       "units_not_mult4"}),
    (1, 1, 31, 109, 4, {"band_under_halo", "last_band_up_short", "last_strip_1col"}),
    (2, 3, 67, 163, 11, {"last_band_1row", "odd_bands_alt", "last_strip_1col"}),
    (1, 3, 130, 53, 16, {"one_strip", "odd_bands_alt", "units_not_mult4"}),
    (1, 1, 67, 108, 17, {"last_band_up_short"}),
    (1, 3, 130, 54, 1, {"one_strip", "band_under_halo", "units_not_mult4", "idle_workgroups"}),
    (2, 3, 130, 163, None, {"odd_bands_alt"}),
    (1, 3, 4, 109, 1, {"last_band_1row", "band_under_halo", "last_strip_1col", "idle_workgroups"}),
    (1, 1, 1, 163, None, {"one_band", "last_strip_1col", "idle_workgroups"}),
    (1, 3, 31, 11, 5, {"one_strip", "last_band_1row", "band_under_window", "units_not_mult4"}),
    (1, 1, 4, 54, 17, {"one_band", "one_strip"}),                      # a forced band taller than the image
    (2, 3, 11, 10, 4, {"one_strip", "band_under_halo", "odd_bands_alt", "units_not_mult4"}),
]


def _sweep_id(c):
    B, C, H, W, rb, _ = c
    return f"{B}x{C}x{H}x{W}-rb{rb if rb is not None else 'def'}"


def _set_env(mp, rb=None, alt=None, fwd=None, bwd=None):
    for name, v in zip(ENV, (rb, alt, fwd, bwd)):
        if v is None:
            mp.delenv(name, raising=False)
        else:
            mp.setenv(name, str(v))


def _geometry_claims(B, C, H, W, edges):
    g = sw_geometry(B * C, H, W)
    missed = sorted(e for e in edges if not EDGES[e](g))
    assert not missed, (f"the case no longer hits {missed}", {k: v for k, v in g.items() if k != "up"})
    return g


# ------------------------------------------------------------------ CPU: the restatement and the sweep's claims
def test_sweep_covers_every_edge():
    claimed = set().union(*(c[5] for c in SWEEP))
    assert claimed == set(EDGES), sorted(set(EDGES) - claimed)


@pytest.mark.parametrize("case", SWEEP, ids=_sweep_id)
def test_sweep_case_hits_its_edges(monkeypatch, case):
    B, C, H, W, rb, edges = case
    _set_env(monkeypatch, rb=rb)
    _geometry_claims(B, C, H, W, edges)


# (planes, H, W, PINGS_SSIM_RB or None); the last two have few, tall bands: 3 x 3 = 9 and 3 x 17 x 36 = 1836 units, fewer
# than the 20 and 6120 tiles of 32 x 32 pixels that the count also made room for while a tile forward existed
PARTIALS_GRID = [
    (1, 130, 11, None), (3, 130, 11, None), (6, 544, 860, None),   # 6 x 544 x 860: rb = 17, the derived branch
    (1, 4, 1, 1), (3, 67, 163, 4), (6, 130, 109, 5), (2, 31, 55, 11), (1, 67, 10, 17), (3, 1080, 1920, 16),
    (6, 67, 163, 1), (1, 11, 55, 5), (1, 64, 11, 4), (3, 300, 11, "0"), (6, 130, 10, "-3"), (1, 1080, 1920, 2),
    (1, 130, 109, 64), (3, 1080, 1920, 64),
]


@pytest.mark.parametrize("planes,H,W,rb", PARTIALS_GRID)
def test_geometry_restatement_matches_partials_count(monkeypatch, planes, H, W, rb):
    """`pings_ssim_partials_count` = the units of the library's own plan: one partial sum per wave.  The library loads
    without a GPU."""
    from pings_amd import _lib

    _set_env(monkeypatch, rb=rb)
    g = sw_geometry(planes, H, W)
    assert _lib.lib().pings_ssim_partials_count(planes, H, W) == g["units"]


def test_default_band_height_is_not_just_the_floor(monkeypatch):
    """The grid above reaches the derived branch of the band height (not only the 16-row floor and the clamp to H)."""
    _set_env(monkeypatch)
    assert sw_rows_per_band(6, 544, 860) == 17
    assert sw_rows_per_band(3, 1080, 1920) == 39          # the bench shape: 28 bands of 39 rows
    assert sw_rows_per_band(1, 4, 10) == 4 and sw_rows_per_band(1, 130, 11) == 16


# ------------------------------------------------------------------ images and the fp64 / fp32 oracle (cached)
@functools.lru_cache(maxsize=None)
def _images(kind, shape, seed=7):
    g = torch.Generator().manual_seed(seed)
    B, C, H, W = shape
    if kind == "noise":
        a = torch.rand(shape, generator=g)
        b = (a + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
    elif kind == "flat":                 # 0.9 plus 1e-3 noise: sigma^2 ~ 1e-6 under E[x^2] ~ 0.81
        a = 0.9 + 1e-3 * torch.randn(shape, generator=g)
        b = 0.9 + 1e-3 * torch.randn(shape, generator=g)
    elif kind == "sky":                  # smooth field, the top 40 % saturated at 1.0; img2 within 1e-3 of img1
        yy = torch.arange(H, dtype=torch.float32).view(H, 1)
        xx = torch.arange(W, dtype=torch.float32).view(1, W)
        f = 0.45 + 0.25 * torch.sin(xx / 37.0 + 0.3) * torch.cos(yy / 53.0) + 0.1 * torch.cos((xx + 2 * yy) / 91.0)
        a = (f + 0.02 * torch.rand(shape, generator=g)).clone()
        a[..., : (2 * H) // 5, :] = 1.0
        b = (a + 1e-3 * torch.randn(shape, generator=g)).clamp(0, 1)
    elif kind == "binary":
        a = (torch.rand(shape, generator=g) > 0.5).float()
        flip = torch.rand(shape, generator=g) < 0.1
        b = torch.where(flip, 1.0 - a, a)
    elif kind == "zeros":
        a, b = torch.zeros(shape), torch.zeros(shape)
    elif kind == "constants":
        a, b = torch.full(shape, 0.3), torch.full(shape, 0.7)
    elif kind == "region":               # equal on the left half only
        a = torch.rand(shape, generator=g)
        b = a.clone()
        b[..., W // 2:] = torch.rand(B, C, H, W - W // 2, generator=g)
    else:
        raise ValueError(kind)
    return a.contiguous(), b.contiguous()


@functools.lru_cache(maxsize=None)
def _oracle(kind, shape, dtype=torch.float64, rows=None):
    """(value, d value / d img1) of oracle/ssim_cpu in `dtype` on `_images(kind, shape)` (rows: a row crop of both)."""
    a, b = _images(kind, shape)
    if rows is not None:
        a, b = a[..., rows[0]:rows[1], :], b[..., rows[0]:rows[1], :]
    x = a.to(dtype, copy=True).requires_grad_(True)      # copy: never mark the cached image itself
    v = ssim_cpu.ssim(x, b.to(dtype))
    (gr,) = torch.autograd.grad(v, x)
    return v.item(), gr


def _hip(a, b):
    """Value and gradient of fused_ssim on the device, under whatever PINGS_SSIM_* the caller set."""
    from pings_amd.ssim import fused_ssim

    x = a.detach().cuda().requires_grad_(True)
    v = fused_ssim(x, b.cuda())
    v.backward()
    return v.item(), x.grad.cpu()


def _assert_fp64_gate(what, vh, gh, v64, g64):
    """Item-2 gate: value within 1e-5 relative, gradient max-abs within 1e-4 of the reference's max-abs."""
    ev, eg = abs(vh - v64) / abs(v64), rel_err(gh, g64)
    assert ev <= 1e-5, (what, "value", vh, v64, ev)
    assert eg <= 1e-4, (what, "gradient rel_err", eg)


# ------------------------------------------------------------------ GPU: geometry sweep of the default kernels
@pytest.mark.gpu
@pytest.mark.parametrize("case", SWEEP, ids=_sweep_id)
def test_default_kernels_geometry_sweep_vs_fp64(monkeypatch, case):
    B, C, H, W, rb, edges = case
    _set_env(monkeypatch, rb=rb)
    _geometry_claims(B, C, H, W, edges)
    a, b = _images("noise", (B, C, H, W))
    v64, g64 = _oracle("noise", (B, C, H, W))
    vh, gh = _hip(a, b)
    _assert_fp64_gate(_sweep_id(case), vh, gh, v64, g64)
    vh2, gh2 = _hip(a, b)
    assert vh2 == vh and torch.equal(gh2, gh), "not bitwise repeatable run to run"


# ------------------------------------------------------------------ GPU: every forward x backward pairing
KERNELS = ("vf", "sw", "tile")            # "tile" exists as a backward only
PAIRINGS = [(f, bw, alt) for f in KERNELS for bw in KERNELS for alt in (0, 1) if f != "tile"]
VARIANT_CASES = [c for c in SWEEP if _sweep_id(c) in ("1x3x11x55-rb5", "1x1x31x109-rb4", "2x3x67x163-rb11",
                                                       "1x3x130x53-rb16", "2x3x130x163-rbdef")]


def _pair_id(p):
    return f"{p[0]}-{p[1]}-alt{p[2]}"


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRINGS, ids=_pair_id)
@pytest.mark.parametrize("case", VARIANT_CASES, ids=_sweep_id)
def test_every_kernel_pairing_vs_fp64(monkeypatch, case, pair):
    """The three derivative maps are the interface between forward and backward: every pairing, mixed ones included,
    meets the fp64 gate."""
    B, C, H, W, rb, edges = case
    fwd, bwd, alt = pair
    _set_env(monkeypatch, rb=rb, alt=alt, fwd=fwd, bwd=bwd)
    _geometry_claims(B, C, H, W, edges if alt else edges - ALT_EDGES)
    a, b = _images("noise", (B, C, H, W))
    v64, g64 = _oracle("noise", (B, C, H, W))
    vh, gh = _hip(a, b)
    _assert_fp64_gate(f"{_sweep_id(case)} {_pair_id(pair)}", vh, gh, v64, g64)


@pytest.mark.gpu
@pytest.mark.parametrize("case", VARIANT_CASES, ids=_sweep_id)
def test_sw_without_alternation_is_bit_identical_to_tile(monkeypatch, case):
    """the horizontal-first sliding-window backward with every band top-down (PINGS_SSIM_ALT=0) adds every
    tap in the tile backward's order with the same operations, so on the same derivative maps (the horizontal-first
    forward's) the gradient is bit-identical."""
    B, C, H, W, rb, _ = case
    a, b = _images("noise", (B, C, H, W))
    _set_env(monkeypatch, rb=rb, alt=0, fwd="sw", bwd="tile")
    _, gt = _hip(a, b)
    _set_env(monkeypatch, rb=rb, alt=0, fwd="sw", bwd="sw")
    _, gs = _hip(a, b)
    assert torch.equal(gs, gt), ("sw/sw ALT=0 gradient differs from sw/tile", (gs - gt).abs().max().item())


# ------------------------------------------------------------------ GPU: content where fp32 cancels
CONTENT = ("flat", "sky", "binary", "zeros", "constants", "region")
CONTENT_SHAPE = (1, 3, 270, 480)


def _assert_content_gate(what, vh, gh, v64, g64, v32, g32):
    """The shape of test_raster._assert_grad_gate: the HIP error against fp64 may not exceed max(1e-4 x scale, 3 x the
    fp32 oracle's own error), for the value (scale |value|) and the gradient (scale max |gradient|)."""
    ev32, evh = abs(v32 - v64), abs(vh - v64)
    g64 = g64.double()
    eg32 = (g32.double() - g64).abs().max().item()
    egh = (gh.double() - g64).abs().max().item()
    vs, gsc = abs(v64), g64.abs().max().item()
    msg = (f"[{what}] value: HIP {evh:.3e} | fp32 oracle {ev32:.3e} (|ref| {vs:.3e}); "
           f"gradient max-abs: HIP {egh:.3e} | fp32 oracle {eg32:.3e} (max|ref| {gsc:.3e}, "
           f"HIP rel {egh / max(gsc, 1e-30):.3e}, fp32 rel {eg32 / max(gsc, 1e-30):.3e})")
    print("\n" + msg)
    assert evh <= max(1e-4 * vs, 3 * ev32), msg
    assert egh <= max(1e-4 * gsc, 3 * eg32), msg


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CONTENT)
def test_content_where_fp32_cancels(monkeypatch, kind):
    _set_env(monkeypatch)
    a, b = _images(kind, CONTENT_SHAPE)
    v64, g64 = _oracle(kind, CONTENT_SHAPE)
    v32, g32 = _oracle(kind, CONTENT_SHAPE, torch.float32)
    vh, gh = _hip(a, b)
    _assert_content_gate(kind, vh, gh, v64, g64, v32, g32)
    if kind == "zeros":   # SSIM(0, 0) = 1 (to the 1-ulp reciprocals of the kernels) with a gradient of exactly zero
        assert abs(vh - 1.0) <= 2.0 ** -23 and not gh.any(), (vh, gh.abs().max().item())


# ------------------------------------------------------------------ GPU: the sizes that run
HD = (1, 3, 1080, 1920)                  # bench.py bench_ssim; fp64 references at this size: noise, sky, the crop
CROP = (173, 1001)                       # the mapper's row crop x[:, v0:v1, :] (utils/mapper.py:1237-1243)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["noise", "sky"])
def test_1080p_vs_fp64(monkeypatch, kind):
    _set_env(monkeypatch)
    a, b = _images(kind, HD)
    v64, g64 = _oracle(kind, HD)
    vh, gh = _hip(a, b)
    if kind == "noise":
        _assert_fp64_gate("1080p noise", vh, gh, v64, g64)
    else:
        v32, g32 = _oracle(kind, HD, torch.float32)
        _assert_content_gate("1080p sky", vh, gh, v64, g64, v32, g32)


@pytest.mark.gpu
def test_mapper_row_crop_of_a_1080p_leaf(monkeypatch):
    """fused_ssim(x[:, v0:v1, :][None], gt[:, v0:v1, :][None]) of a [3, 1080, 1920] leaf: the gradient matches fp64
    on the crop and is exactly zero on every other row."""
    from pings_amd.ssim import fused_ssim

    _set_env(monkeypatch)
    a, b = _images("noise", HD)
    v0, v1 = CROP
    v64, g64 = _oracle("noise", HD, rows=CROP)
    x = a[0].cuda().requires_grad_(True)
    y = b[0].cuda()
    v = fused_ssim(x[:, v0:v1, :].unsqueeze(0), y[:, v0:v1, :].unsqueeze(0))
    v.backward()
    gr = x.grad.cpu()
    _assert_fp64_gate("mapper crop", v.item(), gr[:, v0:v1, :].unsqueeze(0), v64, g64)
    assert not gr[:, :v0, :].any() and not gr[:, v1:, :].any()


@pytest.mark.gpu
def test_512x1392_vs_fp64(monkeypatch):
    _set_env(monkeypatch)
    shape = (1, 3, 512, 1392)
    a, b = _images("noise", shape)
    v64, g64 = _oracle("noise", shape)
    vh, gh = _hip(a, b)
    _assert_fp64_gate("512x1392", vh, gh, v64, g64)


@pytest.mark.gpu
def test_1080p_train_flag_and_retained_graph(monkeypatch):
    from pings_amd.ssim import fused_ssim

    _set_env(monkeypatch)
    a, b = _images("noise", HD)
    x, y = a.cuda().requires_grad_(True), b.cuda()
    v = fused_ssim(x, y)
    ve = fused_ssim(x, y, train=False)
    assert v.requires_grad and not ve.requires_grad
    assert ve.item() == v.item()
    v.backward(retain_graph=True)
    g1 = x.grad.clone()
    x.grad = None
    v.backward()
    assert torch.equal(x.grad, g1)


@pytest.mark.gpu
def test_1080p_every_pairing_repeatable_and_vs_fp64(monkeypatch):
    a, b = _images("noise", HD)
    v64, g64 = _oracle("noise", HD)
    got = {}
    for pair in PAIRINGS:
        fwd, bwd, alt = pair
        _set_env(monkeypatch, alt=alt, fwd=fwd, bwd=bwd)
        vh, gh = _hip(a, b)
        vh2, gh2 = _hip(a, b)
        assert vh2 == vh and torch.equal(gh2, gh), (_pair_id(pair), "not bitwise repeatable")
        _assert_fp64_gate(f"1080p {_pair_id(pair)}", vh, gh, v64, g64)
        got[pair] = vh, gh
    assert torch.equal(got[("sw", "sw", 0)][1], got[("sw", "tile", 0)][1])      # DESIGN §2.2 at the bench shape
