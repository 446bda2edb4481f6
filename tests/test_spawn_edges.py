"""csrc/spawn.hip against fp64 with per-element bounds, at the edges of its groups, counts and clamps.

tests/test_spawn.py runs `renderer.spawn_gaussians` at one shape with random decoder weights and gates the error
normalised by the largest reference value.  This file calls the two stages without the MLPs, so that the raw values
are chosen exactly:
  * gather: row counts around one 16-lane group, one wave and one workgroup, feature widths that are no multiple of
    16, every combination of `sel`, view / distance columns, `xy_only`, colour and free mask, into sentinel-filled
    buffers; the scatter back;
  * activate: surfel (two and three scale columns) and 3d_gs at K = 1, 3, 8 and n = 10, 33, 100, every filter /
    dist_ratio / base / residual combination, with planted Gaussians on and beyond every branch of the kernels
    (`_inputs`), each upstream gradient alone (null pointers for the others) and all together, a NaN rotation row,
    a NaN orientation, and everything dropped (count 0);
  * the device-counted entry points (`*_dyn`) at capacity 64 with 0, 1, 10, 63, 64 and 100 rows counted.
Every comparison with fp64 asserts |hip - fp64| <= E per element, E from tests/spawn_ref.py (no factor on top), AND
test_spawn.py's `rel_err` <= 1e-4, and prints the worst err / E as a line `EDGE ...`.  The bounds need fp32 and fp64 to
take the same branches: a CPU test requires every decision input of every case to lie farther from its threshold
than its bound, or on it exactly where it was planted there, so no element is ever excluded.

Worst err / E per quantity on the MI355X: unmeasured.  No GPU run was possible: none of the tests of this file marked
`gpu` has executed on a device (test_gather_and_its_scatter_at_ragged_groups_and_widths,
test_activate_outputs_compaction_and_gradients_at_every_option, test_a_scale_exactly_on_max_scale_passes_its_gradient,
test_activate_with_every_gaussian_dropped, test_spawn_gaussians_returns_an_empty_view_when_the_alpha_decoder_is_negative,
test_nan_rotation_rows_give_zeros_and_a_nan_orientation_sets_the_flag,
test_device_counted_entry_points_against_the_plain_ones), and neither has the count-0 fix of pings_amd/spawn.py nor the
NaN-norm fix of csrc/spawn.hip.  The CPU tests of this file pass.  Evaluated in fp32 on the CPU (torch operators in
place of the kernels) the same formulas stay within the bounds: worst err / E 0.81 xyz, 0.26 scale, 0.50 rot, 0.10 alpha
and alpha_all, 0.87 colour, 0.54 d_xyz_raw, 0.53 d_rot_raw, 0.29 d_scale_raw, 0.71 d_alpha_raw, 0.63 d_color_raw over
every activate case, so the bounds are neither slack nor short for an honest fp32 evaluation.
"""
import ctypes as C
import itertools
import math

import pytest
import torch

import spawn_ref
from conftest import rel_err

PRM = dict(displacement_range=0.5, unit_scale=0.125, max_scale=0.375, scale_filter_thr=0.1875)     # fp32 numbers
MODES = {"surfel2": (True, 2), "surfel3": (True, 3), "gs3d": (False, 3)}
ACT_K, ACT_N = (1, 3, 8), (10, 33, 100)
# (alpha filter, scale filter, dist_ratio, base, colour residual); the residual needs the base colour
OPTS = [o for o in itertools.product((1, 0), repeat=5) if o[3] or not o[4]]
ALL_ON, ALL_OFF = (1, 1, 1, 1, 1), (0, 0, 0, 0, 0)
OUTS = ("xyz", "scale", "rot", "alpha", "color", "alpha_all")       # the order of the upstream gradients at the C ABI
RAWS = ("xyz_raw", "rot_raw", "scale_raw", "alpha_raw", "color_raw")
GATHER_N = (10, 15, 16, 17, 63, 64, 65, 257)
GATHER_F = ((8, 8), (32, 16), (20, 5))
DYN_CAP, DYN_K, DYN_COUNTS = 64, 3, (0, 1, 10, 63, 64, 100)
SENTINEL = 7.5


# ---------------------------------------------------------------- inputs
def _inputs(mode, k, n):
    """fp32 CPU inputs of `activate` for n neural points with k Gaussians each.  Gaussians 0..9 are planted:
      0, 1, 2, 3  alpha_raw +0.0, -0.0, +1e-30, -1e-30: kept only where the value is positive
      4           alpha / xyz / colour raws +-20 (saturated tanh and sigmoid), base colour (1, 0, 0.5) so that two
                  residual colours leave [0, 1]; scale raw with e = 4 max_scale: output max_scale, gradient 0
      5           alpha_raw -20: dropped, gradient through alpha_all only
      6           rot_raw = 0; one scale column above the filter threshold, the others below
      7           |rot_raw| = 1e-13: the eps branch of normalize
      8           every scale column far below the filter threshold and below max_scale: gradient g e
      9           colour raws (0, 0, -3) on base colour (0, 1, 0): on the lower edge, on the upper edge, below
    """
    surfel, sd = MODES[mode]
    nk = n * k
    g = torch.Generator().manual_seed(1000 * n + 10 * k + sd + int(surfel))
    xyz, rot, scale = torch.randn(nk, 3, generator=g), torch.randn(nk, 4, generator=g), 0.8 * torch.randn(nk, sd, generator=g)
    alpha, color = torch.randn(nk, generator=g), 1.5 * torch.randn(nk, 3, generator=g)
    pos = (torch.rand(n, 3, generator=g) - 0.5) * 40
    quat = torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=1)
    base, dr, free = torch.rand(n, 3, generator=g), 0.5 * torch.rand(n, 1, generator=g), torch.rand(n, generator=g) < 0.3
    alpha[:10] = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0, 1.0, 0.5, 1.0, 0.75])
    xyz[4], color[4] = torch.tensor([20.0, -20.0, 20.0]), torch.tensor([20.0, -20.0, 20.0])
    xyz[5] = torch.tensor([-20.0, 20.0, -20.0])
    scale[4] = math.log(4 * PRM["max_scale"] / PRM["unit_scale"])
    rot[6] = 0.0
    scale[6] = torch.tensor([0.5, -3.0, -3.0])[:sd]
    rot[7] = torch.tensor([5e-14, -5e-14, 5e-14, 5e-14])
    scale[8] = -3.0
    scale[[0, 1, 2, 3, 5, 7, 9], 0] = 0.5                 # these pass the scale filter (and stay below max_scale)
    color[9] = torch.tensor([0.0, 0.0, -3.0])
    base[4 // k], base[9 // k] = torch.tensor([1.0, 0.0, 0.5]), torch.tensor([0.0, 1.0, 0.0])
    return dict(xyz_raw=xyz.reshape(n, 3 * k), rot_raw=rot.reshape(n, 4 * k), scale_raw=scale.reshape(n, sd * k),
                alpha_raw=alpha.reshape(n, k), color_raw=color.reshape(n, 3 * k), pos=pos, quat=quat, base=base,
                dist_ratio=dr, free=free)


def _args(ins, opt, n=None, conv=lambda t: t):
    """Positional arguments of `activate` for an option tuple (the first n rows of every tensor)."""
    _, _, use_dr, use_base, _ = opt
    pick = lambda name: conv(ins[name] if n is None else ins[name][:n])
    return ([pick(r) for r in RAWS]
            + [pick("pos"), pick("quat"), pick("base") if use_base else None, pick("dist_ratio") if use_dr else None,
               pick("free")])


def _kw(mode, k, n, opt):
    return dict(n=n, k=k, surfel=MODES[mode][0], color_residual=bool(opt[4]), alpha_filter_on=bool(opt[0]),
                scale_filter_on=bool(opt[1]), **PRM)


def _weights(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return {name: torch.randn(shape, generator=g) for name, shape in shapes.items()}


def _full(w, keep, nk):
    """Upstream gradient of the kept Gaussians [count, d] -> rows of all n*k Gaussians."""
    out = torch.zeros(nk, w.shape[1], dtype=torch.float64)
    out[keep] = w.double()
    return out


def _reference(ins, mode, k, n, opt, rows=None):
    """fp64 outputs, bounds, and a function (names of the upstream gradients) -> raw gradients and their bounds."""
    kw = _kw(mode, k, n, opt)
    leaves = [t.double().requires_grad_(True) for t in _args(ins, opt, rows)[:5]]
    rest = _args(ins, opt, rows)[5:]
    ref = spawn_ref.activate(*leaves, *rest, **kw)
    bounds = spawn_ref.activate_v(*_args(ins, opt, rows), **kw)
    vals = dict(xyz=ref.xyz, scale=ref.scale, rot=ref.rot, alpha=ref.alpha, color=ref.color, alpha_all=ref.alpha_all)

    def grads(w):
        loss = sum((vals[name] * w[name].double()).sum() for name in w)
        got = torch.autograd.grad(loss, leaves, allow_unused=True, retain_graph=True)
        got = [torch.zeros_like(l) if t is None else t for l, t in zip(leaves, got)]
        gfull = {name: (w[name].double() if name == "alpha_all" else _full(w[name], ref.keep, n * k)) for name in w}
        a = _args(ins, opt, rows)
        return dict(zip(RAWS, got)), spawn_ref.backward_v(*a[:5], a[6], a[7], a[8], ref.keep, gfull, **kw)

    return ref, vals, bounds, grads


def _out_bounds(bounds, keep):
    E = {name: bounds[name][1][keep] for name in ("xyz", "scale", "rot", "alpha", "color")}
    E["alpha_all"] = bounds["alpha"][1]
    return E


def _gate(label, got, ref, E, worst):
    """The two assertions of every comparison; `worst` collects err / E per quantity."""
    assert tuple(got.shape) == tuple(ref.shape), label
    ratio = spawn_ref.worst_ratio(got, ref, E)
    worst[label] = max(worst.get(label, 0.0), ratio)
    assert ratio <= 1.0, f"{label}: err / E = {ratio:.3g}"
    assert rel_err(got, ref) <= 1e-4, label


def _report(title, worst):
    print(f"EDGE {title} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


# ---------------------------------------------------------------- CPU: the reference and the case lists
CASES = ["surfel_res_view", "surfel_direct", "surfel_view_dist", "gs3d_res_view"]


class _Stub:
    """A decoder whose `mlp_batch` returns chosen raws, plus a fixed linear map of its input so that the gradient of
    the features goes through the gather stage as well.  Both sides see the same raws."""

    def __init__(self, raw, fin, k, seed):
        self.raw = raw
        self.P = torch.randn(fin, raw.shape[1], generator=torch.Generator().manual_seed(seed), dtype=torch.float64) / 8
        self.out_k, self.mlp_out_dim = k, raw.shape[1]

    def mlp_batch(self, x):
        return self.raw + x @ self.P


@pytest.mark.parametrize("extra", [dict(), dict(dist_adaptive_scale=True, scale_filter_on=True)], ids=["plain", "dr_sf"])
@pytest.mark.parametrize("name", CASES)
def test_fp64_stages_match_the_oracle_on_the_golden_cases(golden_dir, name, extra):
    import numpy as np
    from oracle.spawn_cpu import spawn_gaussians

    z = np.load(golden_dir / f"spawn_{name}.npz")
    T = lambda key: torch.from_numpy(z[key])
    D = lambda key: T(key).double()
    k, res = int(z["K"]), float(z["resolution"])
    dist_c, view_c, resid = bool(z["dist_concat_on"]), bool(z["view_concat_on"]), bool(z["learn_color_residual"])
    gs_type = str(z["gs_type"])
    mask = T("visible_mask") & T("valid_mask")
    sel = torch.nonzero(mask).view(-1)
    n = int(sel.shape[0])
    Fg, Fc = T("geo_feature").shape[1], T("color_feature").shape[1]
    g = torch.Generator().manual_seed(3)
    dims = dict(gauss_xyz=(3, Fg), gauss_rot=(4, Fg), gauss_scale=(3, Fg), gauss_alpha=(1, Fg + dist_c),
                gauss_color=(3, Fc + 3 * view_c))
    raws = {d: torch.randn(n, o * k, generator=g, dtype=torch.float64).requires_grad_(True) for d, (o, _) in dims.items()}
    decs = {d: _Stub(raws[d], fin, k, 7 + i) for i, (d, (_, fin)) in enumerate(dims.items())}
    geo, cfe = D("geo_feature").requires_grad_(True), D("color_feature").requires_grad_(True)
    ratios = dict(displacement_range_ratio=float(z["displacement_range_ratio"]), max_scale_ratio=float(z["max_scale_ratio"]),
                  unit_scale_ratio=float(z["unit_scale_ratio"]), scale_filter_ratio=0.2)
    data = {"position": D("position"), "orientation": D("orientation"), "color": D("color"), "geo_feature": geo,
            "color_feature": cfe, "resolution": res, "free_mask": T("free_mask"), "valid_mask": T("valid_mask")}
    want = spawn_gaussians(data, decs, T("visible_mask"), D("cam_origin"), dist_c, view_c, z_far=float(z["z_far"]),
                           learn_color_residual=resid, gs_type=gs_type, **ratios, **extra)
    # the same through the two stages of spawn_ref
    geo_in, col_in, pos, quat, base, free, vdist = spawn_ref.gather(
        geo, cfe, sel, D("position"), D("orientation"), D("color"), T("free_mask"), D("cam_origin"), True, view_c, dist_c)
    geo_plain = geo_in[:, :Fg]
    ins = [geo_plain, geo_plain, geo_plain, geo_in, col_in]
    r = [decs[d].mlp_batch(x) for d, x in zip(("gauss_xyz", "gauss_rot", "gauss_scale", "gauss_alpha", "gauss_color"), ins)]
    got = spawn_ref.activate(*r, pos, quat, base if resid else None,
                             vdist / float(z["z_far"]) if extra.get("dist_adaptive_scale") else None, free, n=n, k=k,
                             surfel=gs_type == "gaussian_surfel", color_residual=resid, alpha_filter_on=True,
                             scale_filter_on=bool(extra.get("scale_filter_on")),
                             displacement_range=ratios["displacement_range_ratio"] * res,
                             unit_scale=ratios["unit_scale_ratio"] * res, max_scale=ratios["max_scale_ratio"] * res,
                             scale_filter_thr=0.2 * res)
    pairs = [(got.xyz, "gaussian_xyz"), (got.scale, "gaussian_scale"), (got.rot, "gaussian_rot"),
             (got.alpha, "gaussian_alpha"), (got.color, "gaussian_color"), (got.alpha_all, "alpha_all")]
    assert got.count == want["local_view_gaussian_count"] and 0 < got.count < n * k
    assert torch.equal(got.free_mask, want["gaussian_free_mask"])
    leaves = [geo, cfe] + list(raws.values())
    gw = torch.Generator().manual_seed(5)
    loss_a = loss_b = 0
    for a, key in pairs:
        assert a.shape == want[key].shape and rel_err(a, want[key]) <= 1e-12, key
        w = torch.randn(a.shape, generator=gw, dtype=torch.float64)
        loss_a, loss_b = loss_a + (a * w).sum(), loss_b + (want[key] * w).sum()
    for leaf, a, b in zip(leaves, torch.autograd.grad(loss_a, leaves), torch.autograd.grad(loss_b, leaves)):
        assert b.abs().max() > 0 and rel_err(a, b) <= 1e-12


@pytest.mark.parametrize("mode", MODES)
def test_every_decision_input_is_farther_from_its_threshold_than_its_bound(mode):
    """Keep flags (alpha sign, scale against the filter threshold), the clamp masks (scale against max_scale, residual
    colour against 0 and 1) and the eps branch of normalize, over every activate case of this file.  Only the planted
    values sit on a threshold, exactly (distance 0 in fp32 as in fp64, every operation involved being exact): two
    alpha raws of +-0 and one colour on each clamp edge.  The share of elements a GPU case has to exclude is zero."""
    planted = dict(alpha_keep=2, color_lo=1, color_hi=1)
    for k, n in itertools.product(ACT_K, ACT_N):
        ins = _inputs(mode, k, n)
        for opt in OPTS:
            dec = spawn_ref.activate_v(*_args(ins, opt), **_kw(mode, k, n, opt))["decisions"]
            assert set(dec) == ({"rot_eps", "scale_max"} | ({"alpha_keep"} if opt[0] else set())
                                | ({"scale_thr"} if opt[1] else set()) | ({"color_lo", "color_hi"} if opt[4] else set()))
            for name, (dist, E) in dec.items():
                on = dist == 0
                assert int(on.sum()) == planted.get(name, 0), (name, k, n, opt)
                assert (on | (dist > E)).all(), (name, k, n, opt, float((E / dist)[~on].max()))


@pytest.mark.parametrize("mode", MODES)
def test_the_restated_backward_agrees_with_autograd_and_the_plants_reach_their_branches(mode):
    """`backward_v` walks `backward_kernel`'s formulas; its values must be the autograd gradients of `activate`."""
    k, n = 3, 33
    ins = _inputs(mode, k, n)
    surfel, sd = MODES[mode]
    for opt in (ALL_ON, ALL_OFF, (1, 0, 0, 1, 0), (0, 1, 1, 1, 1)):
        ref, vals, bounds, grads = _reference(ins, mode, k, n, opt)
        assert torch.equal(ref.keep[:10], torch.tensor([not opt[0], not opt[0], True, not opt[0], True, not opt[0],
                                                        True, True, not opt[1], True])), opt
        full = spawn_ref.activate(*[t.double() for t in _args(ins, opt)[:5]], *_args(ins, opt)[5:],
                                  **{**_kw(mode, k, n, opt), "alpha_filter_on": False, "scale_filter_on": False})
        for name in ("xyz", "scale", "rot", "alpha", "color"):
            assert rel_err(bounds[name][0], getattr(full, name)) <= 1e-12, name
        assert (full.scale[4, :2] == PRM["max_scale"]).all() and (full.scale[8, :2] < PRM["scale_filter_thr"]).all()
        assert full.rot[6].abs().max() == 0 and 0.049 < full.rot[7].abs().max() < 0.101    # |raw / eps| = 0.1
        if opt[4]:
            assert full.color[4].tolist() == [1.0, 0.0, pytest.approx(0.6)] and full.color[9].tolist() == [0.0, 1.0, 0.0]
        w = _weights({name: vals[name].shape for name in OUTS}, 17)
        for names in [OUTS] + [(name,) for name in OUTS]:
            auto, rest = grads({name: w[name] for name in names})
            for r in RAWS:
                assert rel_err(rest[r][0], auto[r]) <= 1e-12, (opt, names, r)
                assert (rest[r][1] >= 0).all() and torch.isfinite(rest[r][1]).all()


def test_the_case_lists_hold_what_they_are_meant_to():
    assert all(n * k % 256 for n in ACT_N for k in ACT_K)                       # nk never a multiple of one workgroup
    assert any(n * k > 256 for n in ACT_N for k in ACT_K)                       # more than one workgroup
    assert len(OPTS) == 24 and ALL_ON in OPTS and ALL_OFF in OPTS
    assert all(PRM[key] == torch.tensor(PRM[key], dtype=torch.float32).item() for key in PRM)    # fp32 numbers
    assert {n % 16 for n in GATHER_N} >= {0, 1, 15} and any(n % 4 for n in GATHER_N) and max(GATHER_N) > 256
    assert any(Fg % 16 and Fc % 16 for Fg, Fc in GATHER_F) and any(Fg > 16 for Fg, _ in GATHER_F)
    assert {0, DYN_CAP - 1, DYN_CAP} < set(DYN_COUNTS) and max(DYN_COUNTS) > DYN_CAP


# ---------------------------------------------------------------- GPU: gather
def _gather_abi(L, n, n_dev, sel, m, cam, xy_only, view_c, dist_c, color, free, rows):
    """pings_spawn_gather[_dyn] into sentinel-filled buffers of `rows` rows; -> the buffers."""
    from pings_amd import _lib

    dev = m["position"].device
    Fg, Fc = m["geo"].shape[1], m["col"].shape[1]
    f = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device=dev)
    b = dict(pos=f(rows, 3), quat=f(rows, 4), base=f(rows, 3), free=torch.full((rows,), 9, dtype=torch.uint8, device=dev),
             geo_in=f(rows, Fg + int(dist_c)), col_in=f(rows, Fc + 3 * int(view_c)), vdist=f(rows, 1))
    args = (_lib.ptr(sel), _lib.ptr(m["position"]), _lib.ptr(m["orientation"]), _lib.ptr(m["color"]) if color else None,
            _lib.ptr(m["free"]) if free else None, _lib.ptr(m["geo"]), Fg, _lib.ptr(m["col"]), Fc, _lib.ptr(cam),
            int(xy_only), int(view_c), int(dist_c), _lib.ptr(b["pos"]), _lib.ptr(b["quat"]), _lib.ptr(b["base"]),
            _lib.ptr(b["free"]), _lib.ptr(b["geo_in"]), _lib.ptr(b["col_in"]), _lib.ptr(b["vdist"]), _lib.stream_ptr(dev))
    if n_dev is None:
        _lib.check(L.pings_spawn_gather(n, *args), "pings_spawn_gather")
    else:
        _lib.check(L.pings_spawn_gather_dyn(n, _lib.ptr(n_dev), *args), "pings_spawn_gather_dyn")
    return b


def _map(n_map, Fg, Fc, seed, dev):
    g = torch.Generator().manual_seed(seed)
    m = dict(position=(torch.rand(n_map, 3, generator=g) - 0.5) * 40,
             orientation=torch.nn.functional.normalize(torch.randn(n_map, 4, generator=g), dim=1),
             color=torch.rand(n_map, 3, generator=g), free=(torch.rand(n_map, generator=g) < 0.4).to(torch.uint8),
             geo=torch.randn(n_map + 1, Fg, generator=g), col=torch.randn(n_map + 1, Fc, generator=g))   # + padding row
    return m, {key: t.to(dev) for key, t in m.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("widths", GATHER_F, ids=lambda w: f"F{w[0]}_{w[1]}")
@pytest.mark.parametrize("n", GATHER_N)
def test_gather_and_its_scatter_at_ragged_groups_and_widths(n, widths):
    from pings_amd import _lib, spawn

    L, dev = _lib.lib(), torch.device("cuda")
    Fg, Fc = widths
    cam = torch.tensor([1.0, -2.0, 0.5])
    worst = {}
    for use_sel in (True, False):
        n_map = n + 7 if use_sel else n
        m, md = _map(n_map, Fg, Fc, 31 * n + Fg + use_sel, dev)
        sel = None
        if use_sel:     # a shuffled subset that holds the first and the last row of the map
            perm = torch.randperm(n_map - 2, generator=torch.Generator().manual_seed(n)) + 1
            sel = torch.cat((perm[:n - 2], torch.tensor([0, n_map - 1])))[torch.randperm(n, generator=torch.Generator().manual_seed(n + 1))]
            assert sel.unique().numel() == n and 0 in sel and n_map - 1 in sel
        idx = sel if use_sel else torch.arange(n)
        seld = None if sel is None else sel.to(dev)
        for view_c, dist_c, xy_only, attrs in itertools.product((0, 1), (0, 1), (0, 1), (0, 1)):
            rows = n + 3
            b = _gather_abi(L, n, None, seld, md, cam.to(dev), xy_only, view_c, dist_c, attrs, attrs, rows)
            b = {key: t.cpu() for key, t in b.items()}
            # copies: bit-equal to indexing; nothing behind the rows or beside the columns changes
            assert torch.equal(b["pos"][:n], m["position"][idx]) and torch.equal(b["quat"][:n], m["orientation"][idx])
            assert torch.equal(b["geo_in"][:n, :Fg], m["geo"][idx]) and torch.equal(b["col_in"][:n, :Fc], m["col"][idx])
            if attrs:
                assert torch.equal(b["base"][:n], m["color"][idx]) and torch.equal(b["free"][:n], m["free"][idx])
            else:
                assert (b["base"] == SENTINEL).all() and (b["free"] == 9).all()
            for key, t in b.items():
                assert (t[n:] == (9 if key == "free" else SENTINEL)).all(), key
            assert b["geo_in"].shape[1] == Fg + dist_c and b["col_in"].shape[1] == Fc + 3 * view_c
            # view distance and direction against fp64
            (dist, E_dist), (vdir, E_dir) = spawn_ref.gather_v(sel, m["position"], m["orientation"], cam, xy_only)
            ref = spawn_ref.gather(m["geo"], m["col"], sel, m["position"], m["orientation"], None, None, cam, xy_only,
                                   view_c, dist_c)
            assert rel_err(dist, ref[6]) <= 1e-12
            _gate("view_dist", b["vdist"][:n], ref[6], E_dist, worst)
            if dist_c:
                assert torch.equal(b["geo_in"][:n, Fg], b["vdist"][:n, 0])
            if view_c:
                assert rel_err(vdir, ref[1][:, Fc:]) <= 1e-12
                _gate("view_dir", b["col_in"][:n, Fc:], ref[1][:, Fc:], E_dir, worst)
            # the autograd wrapper returns the same, and scatters the upstream rows back bit for bit
            geo, col = md["geo"].clone().requires_grad_(True), md["col"].clone().requires_grad_(True)
            out = spawn.gather(geo, col, seld, md["position"], md["orientation"], md["color"] if attrs else None,
                               md["free"] if attrs else None, cam.to(dev), bool(xy_only), bool(view_c), bool(dist_c))
            for got, key in zip(out, ("geo_in", "col_in", "pos", "quat", "base", "free", "vdist")):
                assert (got is None and not attrs) if got is None else torch.equal(got.cpu(), b[key][:n]), key
            w = _weights(dict(geo=out[0].shape, col=out[1].shape), n + view_c)
            d_geo, d_col = torch.autograd.grad((out[0] * w["geo"].to(dev)).sum() + (out[1] * w["col"].to(dev)).sum(), [geo, col])
            for d, up, F in ((d_geo.cpu(), w["geo"], Fg), (d_col.cpu(), w["col"], Fc)):
                want = torch.zeros(n_map + 1, F)
                want[idx] = up[:, :F]
                assert torch.equal(d, want) and (d[n_map] == 0).all()
    # without cam_origin no view output is written
    m, md = _map(n, Fg, Fc, n, dev)
    b = _gather_abi(L, n, None, None, md, None, 1, 0, 0, 1, 1, n + 3)
    assert (b["vdist"] == SENTINEL).all() and torch.equal(b["geo_in"][:n].cpu(), m["geo"][:n])
    _report(f"gather n={n} F={Fg}/{Fc}", worst)


# ---------------------------------------------------------------- GPU: activate
def _params(mode, k, n, opt):
    from pings_amd import _abi

    kw = _kw(mode, k, n, opt)
    return _abi.SpawnParams(scale_dim=MODES[mode][1], **{key: (int(v) if isinstance(v, bool) else v) for key, v in kw.items()})


def _plan_abi(L, p, a, n_dev=None, flag=None):
    """pings_spawn_plan[_dyn] -> dest [n*k] (pre-filled with -7), count word."""
    from pings_amd import _lib

    dev = a[0].device
    nk = p.n * p.k
    dest = torch.full((max(nk, 1),), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), -7, dtype=torch.int32, device=dev)
    scratch = torch.empty(L.pings_spawn_plan_scratch_bytes(nk), dtype=torch.uint8, device=dev)
    common = (_lib.ptr(a[3]), _lib.ptr(a[2]), _lib.ptr(a[8]), _lib.ptr(scratch), _lib.ptr(dest), _lib.ptr(cnt))
    if n_dev is None:
        _lib.check(L.pings_spawn_plan(C.byref(p), *common, _lib.stream_ptr(dev)), "pings_spawn_plan")
    else:
        _lib.check(L.pings_spawn_plan_dyn(C.byref(p), _lib.ptr(n_dev), *common, _lib.ptr(flag), _lib.stream_ptr(dev)),
                   "pings_spawn_plan_dyn")
    return dest, cnt


def _forward_abi(L, p, a, dest, rows, n_dev=None, flag=None):
    """pings_spawn_forward[_dyn] into sentinel-filled buffers of `rows` Gaussians."""
    from pings_amd import _lib

    dev = a[0].device
    f = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device=dev)
    sdim = 3 if p.surfel else p.scale_dim
    o = dict(xyz=f(rows, 3), scale=f(rows, sdim), rot=f(rows, 4), alpha=f(rows, 1), color=f(rows, 3), alpha_all=f(rows, 1),
             free=torch.full((rows,), 9, dtype=torch.uint8, device=dev))
    free_in = a[9].to(torch.uint8)
    args = (*[_lib.ptr(t) for t in a[:9]], _lib.ptr(free_in), _lib.ptr(dest), *[_lib.ptr(o[key]) for key in OUTS],
            _lib.ptr(o["free"]))
    if n_dev is None:
        _lib.check(L.pings_spawn_forward(C.byref(p), *args, _lib.stream_ptr(dev)), "pings_spawn_forward")
    else:
        _lib.check(L.pings_spawn_forward_dyn(C.byref(p), _lib.ptr(n_dev), *args, _lib.ptr(flag), _lib.stream_ptr(dev)),
                   "pings_spawn_forward_dyn")
    return o


def _backward_abi(L, p, a, dest, ups, rows):
    """pings_spawn_backward with the upstream gradients `ups` (name -> tensor; the others are null pointers) into
    sentinel-filled buffers of `rows` neural points."""
    from pings_amd import _lib

    dev = a[0].device
    outs = [torch.full((rows, t.shape[1]), SENTINEL, dtype=torch.float32, device=dev) for t in a[:5]]
    st = L.pings_spawn_backward(C.byref(p), *[_lib.ptr(t) for t in a[:5]], _lib.ptr(a[6]), _lib.ptr(a[7]), _lib.ptr(a[8]),
                                _lib.ptr(dest), *[_lib.ptr(ups.get(name)) for name in OUTS], *[_lib.ptr(t) for t in outs],
                                _lib.stream_ptr(dev))
    _lib.check(st, "pings_spawn_backward")
    return dict(zip(RAWS, outs))


def _exact_zeros(ref, d, k, opt, kept4):
    """What has to be exactly zero in the raw gradients `d` (CPU, [n, d*k])."""
    nk = ref.keep.numel()
    drop = ~ref.keep
    for r in ("xyz_raw", "rot_raw", "scale_raw", "color_raw"):      # a dropped Gaussian: gradient through alpha_all only
        assert (d[r].reshape(nk, -1)[drop] == 0).all(), r
    if kept4:                                                        # Gaussian 4: scale clamped, colours 0 and 1 outside
        assert (d["scale_raw"].reshape(nk, -1)[4] == 0).all()
        if opt[4]:
            assert (d["color_raw"].reshape(nk, 3)[4, :2] == 0).all() and d["color_raw"].reshape(nk, 3)[9, 2] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", ACT_N)
@pytest.mark.parametrize("k", ACT_K)
@pytest.mark.parametrize("mode", MODES)
def test_activate_outputs_compaction_and_gradients_at_every_option(mode, k, n):
    from pings_amd import _lib, spawn

    L, dev = _lib.lib(), torch.device("cuda")
    ins = _inputs(mode, k, n)
    nk = n * k
    conv = lambda t: t.to(dev)
    worst = {}
    for opt in OPTS:
        ref, vals, bounds, grads = _reference(ins, mode, k, n, opt)
        a = _args(ins, opt, conv=conv)
        leaves = [t.clone().requires_grad_(True) for t in a[:5]]
        sp = spawn.activate(*leaves, *a[5:], **_kw(mode, k, n, opt))
        # compaction: exact
        assert sp.count == ref.count and 0 < sp.count <= nk
        assert torch.equal(sp.free_mask.cpu(), ref.free_mask)
        assert torch.equal(sp.alpha.cpu(), sp.alpha_all.cpu()[ref.keep])         # the kept order
        got = dict(xyz=sp.xyz, scale=sp.scale, rot=sp.rot, alpha=sp.alpha, color=sp.color, alpha_all=sp.alpha_all)
        E = _out_bounds(bounds, ref.keep)
        for name in OUTS:
            _gate(name, got[name], vals[name], E[name], worst)
        kept4 = bool(ref.keep[4])
        if kept4:
            row = int(ref.keep[:4].sum())
            assert (sp.scale[row, :2].cpu() == PRM["max_scale"]).all()
            if opt[4]:
                assert sp.color[row, :2].tolist() == [1.0, 0.0]
        # all six upstream gradients, through autograd
        w = _weights({name: vals[name].shape for name in OUTS}, 100 * n + k)
        d_hip = torch.autograd.grad(sum((got[name] * w[name].to(dev)).sum() for name in OUTS), leaves)
        d_hip = {r: t.cpu() for r, t in zip(RAWS, d_hip)}
        d_ref, d_E = grads(w)
        for r in RAWS:
            _gate("d_" + r, d_hip[r], d_ref[r], d_E[r][1], worst)
        _exact_zeros(ref, d_hip, k, opt, kept4)
        if opt not in (ALL_ON, ALL_OFF):
            continue
        # each upstream gradient alone, the other five null, at the C ABI; with all filters off `dest` is null too
        p = _params(mode, k, n, opt)
        dest = None
        if opt[0] or opt[1]:
            dest, cnt = _plan_abi(L, p, a)
            assert int(cnt.item()) == ref.count
            want = torch.full((nk,), -1, dtype=torch.int32)
            want[ref.keep] = torch.arange(ref.count, dtype=torch.int32)
            assert torch.equal(dest.cpu(), want)
        for name in OUTS:
            d = _backward_abi(L, p, a, dest, {name: w[name].to(dev).contiguous()}, n)
            d = {r: t.cpu() for r, t in d.items()}
            d_ref, d_E = grads({name: w[name]})
            for r in RAWS:
                _gate(f"d_{r}<-{name}", d[r], d_ref[r], d_E[r][1], worst)
            _exact_zeros(ref, d, k, opt, kept4)
            only = {"xyz": "xyz_raw", "scale": "scale_raw", "rot": "rot_raw", "alpha": "alpha_raw", "color": "color_raw",
                    "alpha_all": "alpha_raw"}[name]
            assert all((d[r] == 0).all() for r in RAWS if r != only) and d[only].abs().max() > 0
    _report(f"activate {mode} k={k} n={n}", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_a_scale_exactly_on_max_scale_passes_its_gradient(mode):
    """max_scale = unit_scale and scale_raw = 0 without dist_ratio: e = unit expf(0) = max_scale exactly, in fp32 as
    in fp64.  torch's clamp passes the gradient on the edge (mask e <= max), so d scale_raw = g e there."""
    from pings_amd import spawn

    k, n, dev = 3, 33, torch.device("cuda")
    opt = (1, 0, 0, 1, 1)
    ins = _inputs(mode, k, n)
    sd = MODES[mode][1]
    on = [6, 12, 40]
    ins["scale_raw"].reshape(n * k, sd)[on] = 0.0
    ins["alpha_raw"].reshape(n * k)[on] = 1.0
    kw = {**_kw(mode, k, n, opt), "max_scale": PRM["unit_scale"]}
    leaves64 = [t.double().requires_grad_(True) for t in _args(ins, opt)[:5]]
    ref = spawn_ref.activate(*leaves64, *_args(ins, opt)[5:], **kw)
    dec = spawn_ref.activate_v(*_args(ins, opt), **kw)["decisions"]["scale_max"]
    assert ref.keep[on].all() and int((dec[0] == 0).sum()) == len(on) * sd and ((dec[0] == 0) | (dec[0] > dec[1])).all()
    a = _args(ins, opt, conv=lambda t: t.to(dev))
    leaves = [t.clone().requires_grad_(True) for t in a[:5]]
    sp = spawn.activate(*leaves, *a[5:], **kw)
    w = _weights(dict(scale=ref.scale.shape), 9)["scale"]
    (d_hip,) = torch.autograd.grad((sp.scale * w.to(dev)).sum(), [leaves[2]])
    (d_ref,) = torch.autograd.grad((ref.scale * w.double()).sum(), [leaves64[2]])
    a64 = _args(ins, opt)
    E = spawn_ref.backward_v(*a64[:5], a64[6], a64[7], a64[8], ref.keep, {"scale": _full(w, ref.keep, n * k)}, **kw)
    worst = {}
    _gate("scale", sp.scale, ref.scale, spawn_ref.activate_v(*a64, **kw)["scale"][1][ref.keep], worst)
    _gate("d_scale_raw", d_hip.cpu(), d_ref, E["scale_raw"][1], worst)
    rows = torch.tensor(on)
    live = 2 if MODES[mode][0] else sd
    assert (d_ref.reshape(n * k, sd)[rows, :live] != 0).all()
    assert (sp.scale.cpu()[ref.keep.cumsum(0)[rows] - 1, :live] == PRM["unit_scale"]).all()
    _report(f"scale on max {mode}", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_activate_with_every_gaussian_dropped(mode):
    """count 0: empty outputs, a full alpha_all, and its gradient."""
    from pings_amd import spawn

    k, n, dev = 3, 33, torch.device("cuda")
    ins = _inputs(mode, k, n)
    ins["alpha_raw"] = -ins["alpha_raw"].abs() - 0.1
    worst = {}
    ref, vals, bounds, grads = _reference(ins, mode, k, n, ALL_ON)
    assert ref.count == 0
    a = _args(ins, ALL_ON, conv=lambda t: t.to(dev))
    leaves = [t.clone().requires_grad_(True) for t in a[:5]]
    sp = spawn.activate(*leaves, *a[5:], **_kw(mode, k, n, ALL_ON))
    assert sp.count == 0 and sp.free_mask.shape == (0,)
    for name, t in (("xyz", sp.xyz), ("scale", sp.scale), ("rot", sp.rot), ("alpha", sp.alpha), ("color", sp.color)):
        assert tuple(t.shape) == tuple(vals[name].shape) and t.shape[0] == 0, name
    _gate("alpha_all", sp.alpha_all, vals["alpha_all"], bounds["alpha"][1], worst)
    w = _weights({name: vals[name].shape for name in OUTS}, 3)
    loss = sum((t * w[name].to(dev)).sum() for name, t in (("xyz", sp.xyz), ("alpha", sp.alpha), ("alpha_all", sp.alpha_all)))
    d_hip = dict(zip(RAWS, (t.cpu() for t in torch.autograd.grad(loss, leaves))))
    d_ref, d_E = grads({"alpha_all": w["alpha_all"]})
    _gate("d_alpha_raw", d_hip["alpha_raw"], d_ref["alpha_raw"], d_E["alpha_raw"][1], worst)
    assert d_hip["alpha_raw"].abs().max() > 0
    assert all((d_hip[r] == 0).all() for r in RAWS if r != "alpha_raw")
    _report(f"count0 {mode}", worst)


@pytest.mark.gpu
def test_spawn_gaussians_returns_an_empty_view_when_the_alpha_decoder_is_negative():
    """An alpha decoder with zero output weights and a negative bias drops every Gaussian."""
    from pings_amd.renderer import spawn_gaussians
    from test_spawn import DEC, Dec

    n, k, Fg, Fc, hid, dev = 40, 3, 8, 8, 32, "cuda"
    g = torch.Generator().manual_seed(2)
    st = {}
    for name, out in (("gauss_xyz", 3), ("gauss_rot", 4), ("gauss_scale", 3), ("gauss_alpha", 1), ("gauss_color", 3)):
        fin = Fc if name == "gauss_color" else Fg
        st[f"dec.{name}.layers.0.weight"] = (torch.randn(hid, fin, generator=g) / fin ** 0.5).numpy()
        st[f"dec.{name}.layers.0.bias"] = (0.1 * torch.randn(hid, generator=g)).numpy()
        st[f"dec.{name}.lout.weight"] = (torch.randn(out * k, hid, generator=g) / hid ** 0.5).numpy()
        st[f"dec.{name}.lout.bias"] = (0.1 * torch.randn(out * k, generator=g)).numpy()
    st["dec.gauss_alpha.lout.weight"] *= 0
    st["dec.gauss_alpha.lout.bias"] = st["dec.gauss_alpha.lout.bias"] * 0 - 1
    decs = {name: Dec(st, name, k, dev) for name in DEC}
    m, md = _map(n, Fg, Fc, 4, torch.device(dev))
    data = {"position": md["position"], "orientation": md["orientation"], "color": md["color"],
            "geo_feature": md["geo"].requires_grad_(True), "color_feature": md["col"], "resolution": 0.25,
            "free_mask": md["free"].bool()}
    res = spawn_gaussians(data, decs, None, None)
    assert res["local_view_gaussian_count"] == 0
    assert res["gaussian_xyz"].shape == (0, 3) and res["gaussian_scale"].shape == (0, 3)
    assert res["gaussian_rot"].shape == (0, 4) and res["gaussian_alpha"].shape == (0, 1)
    assert res["gaussian_color"].shape == (0, 3) and res["gaussian_free_mask"].shape == (0,)
    assert torch.allclose(res["alpha_all"].cpu(), torch.full((n * k, 1), math.tanh(-1.0)), rtol=0, atol=5 * 2.0 ** -23)
    (d_bias,) = torch.autograd.grad(res["alpha_all"].sum(), [decs["gauss_alpha"].lout.bias])
    assert torch.allclose(d_bias.cpu(), torch.full((k,), n * (1 - math.tanh(-1.0) ** 2)), rtol=1e-5)


@pytest.mark.gpu
def test_nan_rotation_rows_give_zeros_and_a_nan_orientation_sets_the_flag():
    from pings_amd import _lib

    L, dev = _lib.lib(), torch.device("cuda")
    mode, k, n = "surfel3", 3, 33
    ins = _inputs(mode, k, n)
    rot = ins["rot_raw"].reshape(n * k, 4)
    rot[10] = float("nan")
    rot[11, 2] = float("nan")          # one component: the norm is NaN, so torch zeroes the whole row
    ins["alpha_raw"].reshape(n * k)[10:12] = 1.0
    ins["scale_raw"].reshape(n * k, 3)[10:12, 0] = 0.5
    opt = ALL_ON
    p = _params(mode, k, n, opt)
    n_dev = torch.tensor([n], dtype=torch.int32, device=dev)
    worst = {}

    def run(ins):
        a = _args(ins, opt, conv=lambda t: t.to(dev))
        flag = torch.ones(1, dtype=torch.int32, device=dev)
        dest, cnt = _plan_abi(L, p, a, n_dev, flag)
        assert int(flag.item()) == 0
        flag.fill_(0)
        return _forward_abi(L, p, a, dest, n * k, n_dev, flag), int(cnt.item()), int(flag.item()), dest.cpu()

    o, count, flag, dest = run(ins)
    ref, vals, bounds, _ = _reference(ins, mode, k, n, opt)
    assert flag == 0 and count == ref.count and ref.keep[10] and ref.keep[11]
    E = _out_bounds(bounds, ref.keep)
    for name in OUTS:
        rows = n * k if name == "alpha_all" else count
        _gate(name, o[name][:rows].cpu(), vals[name], E[name], worst)
    assert (o["rot"][int(dest[10])] == 0).all() and (o["rot"][int(dest[11])] == 0).all()
    # a NaN orientation of neural point 5: the flag, and no other Gaussian changes
    bad = {key: t.clone() for key, t in ins.items()}
    bad["quat"][5, 1] = float("nan")
    o2, count2, flag2, dest2 = run(bad)
    assert flag2 == 1 and count2 == count and torch.equal(dest, dest2)
    other = torch.ones(n * k, dtype=torch.bool)
    other[5 * k:6 * k] = False
    rows = dest[other & ref.keep].long()
    for name in ("xyz", "scale", "rot", "alpha", "color"):
        assert torch.equal(o[name].cpu()[rows], o2[name].cpu()[rows]), name
    assert torch.isnan(o2["rot"].cpu()[dest[5 * k:6 * k][ref.keep[5 * k:6 * k]].long()]).any()
    _report("nan rows", worst)


# ---------------------------------------------------------------- GPU: the device-counted entry points
@pytest.mark.gpu
@pytest.mark.parametrize("counted", DYN_COUNTS)
def test_device_counted_entry_points_against_the_plain_ones(counted):
    from pings_amd import _lib

    L, dev = _lib.lib(), torch.device("cuda")
    cap, k, mode, opt = DYN_CAP, DYN_K, "surfel3", ALL_ON
    live = min(cap, counted)
    n_dev = torch.tensor([counted], dtype=torch.int32, device=dev)
    worst = {}
    # gather: capacity-sized sel, the count on the device
    m, md = _map(cap + 16, 20, 5, 77, dev)
    sel = torch.randperm(cap + 16, generator=torch.Generator().manual_seed(8))[:cap].to(dev)
    cam = torch.tensor([1.0, -2.0, 0.5], device=dev)
    dyn = _gather_abi(L, cap, n_dev, sel, md, cam, 1, 1, 1, 1, 1, cap)
    plain = _gather_abi(L, live, None, sel, md, cam, 1, 1, 1, 1, 1, cap)
    for key in dyn:             # live rows bit-equal, the sentinel behind them untouched
        assert torch.equal(dyn[key], plain[key]), key
        assert (dyn[key][live:] == (9 if key == "free" else SENTINEL)).all(), key
    if live:
        assert torch.equal(dyn["pos"][:live].cpu(), m["position"][sel.cpu()[:live]])
    # plan + forward
    ins = _inputs(mode, k, cap)
    a = _args(ins, opt, conv=lambda t: t.to(dev))
    p_cap, p_live = _params(mode, k, cap, opt), _params(mode, k, live, opt)
    flag = torch.ones(1, dtype=torch.int32, device=dev)
    dest, cnt = _plan_abi(L, p_cap, a, n_dev, flag)
    dest_p, cnt_p = _plan_abi(L, p_live, a)
    count = int(cnt.item())
    assert count == int(cnt_p.item()) and int(flag.item()) == 0
    assert torch.equal(dest[:live * k], dest_p[:live * k]) and (dest[live * k:] == -1).all()
    o = _forward_abi(L, p_cap, a, dest, cap * k, n_dev, flag)
    o_p = _forward_abi(L, p_live, a, dest_p if live else None, cap * k)
    assert int(flag.item()) == 0
    for key in o:
        rows = live * k if key == "alpha_all" else count
        assert torch.equal(o[key], o_p[key]), key
        assert (o[key][rows:] == (9 if key == "free" else SENTINEL)).all(), key
    if not live:
        d = _backward_abi(L, p_live, a, dest, {}, cap)
        assert all((t == SENTINEL).all() for t in d.values())
        return
    keep = dest.cpu()[:live * k] >= 0
    gs = torch.nonzero(keep).view(-1)
    assert count == int(keep.sum()) and torch.equal(dest.cpu()[:live * k][keep], torch.arange(count, dtype=torch.int32))
    assert torch.equal(o["free"][:count].cpu(), ins["free"].to(torch.uint8)[gs % live])      # tiled by the device count
    # against fp64 on the live rows, forward and (n = live, capacity-sized dest) backward
    ref, vals, bounds, grads = _reference(ins, mode, k, live, opt, rows=live)
    assert torch.equal(ref.keep, keep)
    E = _out_bounds(bounds, ref.keep)
    for name in OUTS:
        rows = live * k if name == "alpha_all" else count
        _gate(name, o[name][:rows].cpu(), vals[name], E[name], worst)
    w = _weights({name: (cap * k, vals[name].shape[1]) for name in OUTS}, counted)
    d = _backward_abi(L, p_live, a, dest, {name: t.to(dev) for name, t in w.items()}, cap)
    d_ref, d_E = grads({name: w[name][:vals[name].shape[0]] for name in OUTS})
    for r in RAWS:
        assert (d[r][live:] == SENTINEL).all(), r
        _gate("d_" + r, d[r][:live].cpu(), d_ref[r], d_E[r][1], worst)
    _report(f"dyn counted={counted}", worst)
