"""SDF-sample loss block (pings_amd.sdf_losses, csrc/sdf_loss.hip) against the fp64 restatement of
utils/mapper.py:836-930 / 1493-1544 (tests/sdf_losses_ref.py) on the oracle's SDF maps."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import sdf_losses_ref as ref
from conftest import rel_err
from oracle import sdf_cpu

LOSS_W = [1.0, 0.5, 0.8]            # lambda_sdf, weight_e, weight_i of the tests' total
STATES = ["gs_f32", "pin_f8"]       # per-neighbour decoder (k rows) / weighted_first


def _state(name):
    from pathlib import Path

    z = np.load(Path(__file__).parent / "golden" / f"sdf_{name}.npz")
    return {k: z[k] for k in z.files}


def _cfg(st, d=3, loss_weight_on=False, **kw):
    c = NS(main_loss_type="bce", numerical_grad=True, gradient_decimation=d, free_sample_end_dist_m=0.3,
           surface_sample_range_m=0.3, voxel_size_m=float(st["resolution"]), num_grad_step_ratio=0.2,
           loss_weight_on=loss_weight_on, weighted_first=bool(st["weighted_first"]))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _sigma(st):
    return 1.5 * float(st["sdf_scale"])          # the mapper's sdf_scale, kept apart from the decoder's on purpose


def _batch(st, B=600, seed=0):
    """Samples around the golden query points: coord, sdf_label, ts, weight, colour label (CPU, float32)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.as_tensor(st["x"], dtype=torch.float32)
    coord = x[torch.randint(0, x.shape[0], (B,), generator=g)] + 0.03 * torch.randn(B, 3, generator=g)
    label = 0.4 * torch.randn(B, generator=g)
    ts = torch.randint(0, int(st["cur_ts"]) + 1, (B,), generator=g, dtype=torch.int32)
    weight = torch.randn(B, generator=g)
    color_label = torch.rand(B, 3, generator=g)
    color_label[torch.rand(B, generator=g) < 0.2, 0] = -1.0
    return coord, label, ts, weight, color_label


def _cmlp_params(st, seed=5, H=64, C=3):
    g = torch.Generator().manual_seed(seed)
    IN = int(st["local_color_features"].shape[1]) + 3
    return [0.4 * torch.randn(H, IN, generator=g), 0.1 * torch.randn(H, generator=g),
            0.3 * torch.randn(C, H, generator=g), 0.1 * torch.randn(C, generator=g)]


def _dec_params(st):
    return [torch.as_tensor(st["dec." + k]) for k in ("layers.0.weight", "layers.0.bias", "lout.weight", "lout.bias")]


# ------------------------------------------------------------------ CPU
def _golden(name):
    from pathlib import Path

    z = np.load(Path(__file__).parent / "golden" / f"sdfloss_{name}.npz")
    return {k: z[k] for k in z.files}


def _ref_run(st, gd_or_inputs, cfg, eikonal, color, color_weighted, dec_p, cm_p):
    """fp64 restatement: values and the gradients of LOSS_W . values w.r.t. both tables and both decoders."""
    coord, label, ts, weight, color_label = gd_or_inputs
    geo = torch.as_tensor(st["local_geo_features"]).double().requires_grad_(True)
    col = torch.as_tensor(st["local_color_features"]).double().requires_grad_(True)
    p64 = [torch.as_tensor(p).detach().double().requires_grad_(True) for p in list(dec_p) + list(cm_p)]
    npm = ref.map64(st, geo, col)
    dec = sdf_cpu.MLP(*p64[:4], float(st["sdf_scale"]))
    cm = sdf_cpu.MLP(*p64[4:])
    bce, eik, colv, n_eik, n_col, pred = ref.block(cfg, _sigma(st), npm, dec, cm, coord.double(), label.double(), ts,
                                                   weight.double(), color_label.double(), eikonal, color,
                                                   color_weighted)
    vals = [torch.as_tensor(v, dtype=torch.float64) for v in (bce, eik, colv)]
    tot = sum(w * v for w, v in zip(LOSS_W, vals) if v.requires_grad and bool(torch.isfinite(v)))
    grads = torch.autograd.grad(tot, [geo, col] + p64, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for t, g in zip([geo, col] + p64, grads)]
    return vals, (n_eik, n_col), grads, npm


GOLDEN_CASES = {"gs_f32": dict(eikonal=True, color=True, color_weighted=True, loss_weight_on=True, d=3),
                "pin_f8": dict(eikonal=True, color=True, color_weighted=False, loss_weight_on=False, d=4)}
GRAD_NAMES = ["local_geo_features", "local_color_features", "dec.W1", "dec.b1", "dec.W2", "dec.b2", "color.W1",
              "color.b1", "color.W2", "color.b2"]


@pytest.mark.parametrize("name", STATES)
def test_restatement_matches_reference_helpers_golden(name):
    """tests/sdf_losses_ref.py against vectors made with the reference's sdf_bce_loss / color_diff_loss and the inline
    lines of the SDF loop (tools/make_sdfloss_golden.py)."""
    gd = _golden(name)
    st = _state(name)
    c = GOLDEN_CASES[name]
    cfg = _cfg(st, d=c["d"], loss_weight_on=c["loss_weight_on"])
    ins = tuple(torch.as_tensor(gd[k]) for k in ("coord", "label", "ts", "weight", "color_label"))
    cm_p = [torch.as_tensor(gd["cmlp." + k]) for k in ("W1", "b1", "W2", "b2")]
    vals, counts, grads, _ = _ref_run(st, ins, cfg, c["eikonal"], c["color"], c["color_weighted"], _dec_params(st),
                                      cm_p)
    assert np.allclose([float(v.detach()) for v in vals], gd["values"], rtol=1e-10, atol=1e-12, equal_nan=True)
    assert list(counts) == list(gd["counts"])
    for k, g in zip(GRAD_NAMES, grads):
        assert np.allclose(g.numpy(), gd["d_" + k], rtol=1e-9, atol=1e-12), k


def test_restatement_empty_subsets_are_nan():
    st = _state("gs_f32")
    cfg = _cfg(st)
    coord, label, ts, weight, cl = _batch(st, B=40)
    label = torch.full_like(label, 2.0)             # outside both bands
    vals, counts, _, _ = _ref_run(st, (coord, label, ts, weight, cl), cfg, True, True, False, _dec_params(st),
                                  _cmlp_params(st))
    assert counts == (0, 0)
    assert bool(torch.isnan(vals[1])) and bool(torch.isnan(vals[2])) and bool(torch.isfinite(vals[0]))


def _cpu_mapper(st, cfg):
    npm = sdf_cpu.NeuralPointMap(st)
    npm.config = NS(query_nn_k=npm.nn_k, weighted_first=npm.weighted_first, layer_norm_on=False)
    t = [torch.nn.Parameter(p.clone()) for p in _dec_params(st)]
    dec = NS(layers=[NS(weight=t[0], bias=t[1])], lout=NS(weight=t[2], bias=t[3]), sdf_scale=float(st["sdf_scale"]),
             use_leaky_relu=False)
    c = [torch.nn.Parameter(p) for p in _cmlp_params(st)]
    cm = NS(layers=[NS(weight=c[0], bias=c[1])], lout=NS(weight=c[2], bias=c[3]), use_leaky_relu=False)
    return NS(config=cfg, neural_points=npm, sdf_mlp=dec, color_mlp=cm, sdf_scale=_sigma(st), require_gradient=False)


def test_argument_validation():
    from pings_amd.sdf_losses import sdf_losses

    st = _state("gs_f32")
    m = _cpu_mapper(st, _cfg(st))
    coord, label, ts, weight, cl = _batch(st, B=32)
    with pytest.raises(Exception, match="HIP device only"):
        sdf_losses(m, coord, label, ts, weight, cl, color=True)
    m.config.main_loss_type = "l1"
    with pytest.raises(NotImplementedError, match="main_loss_type"):
        sdf_losses(m, coord, label, ts, weight)
    m.config.main_loss_type = "bce"
    m.require_gradient = True
    with pytest.raises(NotImplementedError, match="not have been used in the graph"):
        sdf_losses(m, coord, label, ts, weight)
    m.require_gradient = False
    with pytest.raises(ValueError, match="coord"):
        sdf_losses(m, coord[:, :2], label, ts, weight)
    with pytest.raises(ValueError, match="sdf_label"):
        sdf_losses(m, coord, label[:-1], ts, weight)
    with pytest.raises(ValueError, match="weight"):
        sdf_losses(m, coord, label, ts, weight.view(-1, 1))
    with pytest.raises(ValueError, match="color_label"):
        sdf_losses(m, coord, label, ts, weight, cl[:, :2], color=True)
    with pytest.raises(TypeError, match="coord"):
        sdf_losses(m, coord.double(), label, ts, weight)
    with pytest.raises(TypeError, match="sdf_label"):
        sdf_losses(m, coord, label.half(), ts, weight)
    with pytest.raises(TypeError, match="ts"):
        sdf_losses(m, coord, label, ts.float(), weight)
    with pytest.raises(TypeError, match="color_label"):
        sdf_losses(m, coord, label, ts, weight, cl.double(), color=True)


# ------------------------------------------------------------------ GPU
def _gpu_mapper(st, cfg, cm_p=None):
    npm = sdf_cpu.NeuralPointMap(st, device="cuda")
    npm.config = NS(query_nn_k=npm.nn_k, weighted_first=npm.weighted_first, layer_norm_on=False)
    npm.color_feature_dim = npm.color_features.shape[1]
    npm.local_geo_features.requires_grad_(True)
    npm.local_color_features.requires_grad_(True)
    t = [torch.nn.Parameter(p.clone().cuda()) for p in _dec_params(st)]
    dec = NS(layers=[NS(weight=t[0], bias=t[1])], lout=NS(weight=t[2], bias=t[3]), sdf_scale=float(st["sdf_scale"]),
             use_leaky_relu=False)
    c = [torch.nn.Parameter(p.clone().cuda()) for p in (cm_p if cm_p is not None else _cmlp_params(st))]
    cm = NS(layers=[NS(weight=c[0], bias=c[1])], lout=NS(weight=c[2], bias=c[3]), use_leaky_relu=False)
    return NS(config=cfg, neural_points=npm, sdf_mlp=dec, color_mlp=cm, sdf_scale=_sigma(st), require_gradient=False,
              dtype=torch.float32, device="cuda")


def _params(m):
    npm, dec, cm = m.neural_points, m.sdf_mlp, m.color_mlp
    return [npm.local_geo_features, npm.local_color_features, dec.layers[0].weight, dec.layers[0].bias,
            dec.lout.weight, dec.lout.bias, cm.layers[0].weight, cm.layers[0].bias, cm.lout.weight, cm.lout.bias]


def _hip_run(m, ins, eikonal, color, color_weighted):
    from pings_amd.sdf_losses import sdf_losses

    coord, label, ts, weight, cl = (t.cuda() for t in ins)
    S = sdf_losses(m, coord, label, ts, weight, cl, eikonal=eikonal, color=color, color_weighted=color_weighted)
    vals = [S.bce, S.eikonal, S.color]
    tot = sum(w * v for w, v in zip(LOSS_W, vals))
    grads = torch.autograd.grad(tot, _params(m), allow_unused=True)
    return S, vals, grads


def _close(a, b, tol=1e-4):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    if torch.isnan(b).all():
        return bool(torch.isnan(a).all())
    return rel_err(a, b) <= tol


@pytest.mark.gpu
@pytest.mark.parametrize("name", STATES)
@pytest.mark.parametrize("colour", ["off", "unweighted", "weighted"])
@pytest.mark.parametrize("eikonal", [True, False])
def test_values_and_gradients_match_fp64_restatement(name, colour, eikonal):
    st = _state(name)
    cfg = _cfg(st, d=3, loss_weight_on=(colour != "unweighted"))
    ins = _batch(st, B=600, seed=1)
    color, cw = colour != "off", colour == "weighted"
    m = _gpu_mapper(st, cfg)
    S, vals, gh = _hip_run(m, ins, eikonal, color, cw)
    rv, rc, gr, _ = _ref_run(st, ins, cfg, eikonal, color, cw, _dec_params(st), _cmlp_params(st))
    assert [float(x) for x in S.counts] == [float(x) for x in rc]
    assert rc[0] > 0 or not eikonal
    assert rc[1] > 0 or not color
    for n, a, b in zip(("bce", "eikonal", "color"), vals, rv):
        assert _close(a, b), (n, float(a), float(b))
    for n, a, b in zip(GRAD_NAMES, gh, gr):
        a = torch.zeros_like(b) if a is None else a.detach().cpu().double().reshape(b.shape)
        if not color and n.startswith("color") or (not color and n == "local_color_features"):
            assert float(a.abs().max()) == 0.0, n
            continue
        assert float(b.abs().max()) > 0, n
        assert rel_err(a, b) <= 1e-4, (n, rel_err(a, b))


def _subset(S):
    st = S.bce.grad_fn.st
    live = int(S.counts[0])
    return st["keep"]["idx"].long().cpu(), live, st


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["none", "fewer_than_d", "not_multiple", "all", "d1"])
def test_eikonal_subset_is_nonzero_decimated(case):
    from pings_amd.sdf_losses import sdf_losses

    st = _state("gs_f32")
    B = 301
    d = 1 if case == "d1" else 4
    cfg = _cfg(st, d=d)
    m = _gpu_mapper(st, cfg)
    coord, label, ts, weight, cl = _batch(st, B=B, seed=3)
    if case == "none":
        label = torch.full_like(label, 1.0)
    elif case == "fewer_than_d":
        label = torch.full_like(label, 1.0)
        label[[17, 200, 250]] = 0.05
    elif case == "all":
        label = 0.1 * torch.rand(B) - 0.05
    mask = torch.abs(label) < cfg.free_sample_end_dist_m
    want = torch.nonzero(mask)[::d].view(-1)
    if case == "not_multiple":
        assert int(mask.sum()) % d != 0
    S = sdf_losses(m, coord.cuda(), label.cuda(), ts.cuda(), weight.cuda(), cl.cuda(), eikonal=True, color=True)
    idx, live, _ = _subset(S)
    assert idx.shape[0] == (B + d - 1) // d
    assert live == len(want)
    assert torch.equal(idx[:live], want)
    assert bool((idx[live:] == -1).all())
    if case == "none":
        assert bool(torch.isnan(S.eikonal)) and bool(torch.isnan(S.color))
        assert float(S.counts[1]) == 0
        # the padded rows carry no gradient: only BCE reaches the tables and the decoder
        g = torch.autograd.grad(S.bce + torch.nan_to_num(S.eikonal, 0.0), _params(m)[:1])[0]
        g0 = torch.autograd.grad(sdf_losses(m, coord.cuda(), label.cuda(), ts.cuda(), weight.cuda(), eikonal=False).bce,
                                 _params(m)[:1])[0]
        assert torch.equal(g, g0)
    else:
        assert bool(torch.isfinite(S.eikonal))


@pytest.mark.gpu
@pytest.mark.parametrize("name", STATES)
def test_gradient_rows_bit_equal_numerical_gradient(name):
    from pings_amd import mapper_ops

    st = _state(name)
    cfg = _cfg(st, d=3)
    m = _gpu_mapper(st, cfg)
    from pings_amd.sdf_losses import sdf_losses

    coord, label, ts, weight, cl = (t.cuda() for t in _batch(st, B=500, seed=2))
    S = sdf_losses(m, coord, label, ts, weight, eikonal=True)
    idx, live, bst = _subset(S)
    g = bst["keep"]["g"][:live]
    x = coord[idx[:live].cuda()]
    with torch.no_grad():
        want = mapper_ops.get_numerical_gradient(m, x, None, cfg.voxel_size_m * cfg.num_grad_step_ratio)
    assert live > 10
    assert torch.equal(g, want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", STATES)
def test_side_effects_match_plain_query(name):
    from pings_amd import neural_points as hnp
    from pings_amd.sdf_losses import sdf_losses

    st = _state(name)
    cfg = _cfg(st)
    coord, label, ts, weight, cl = (t.cuda() for t in _batch(st, B=500, seed=4))
    ts = torch.full_like(ts, int(st["cur_ts"]) + 3)      # newer than every stored update: the amax must show
    a, b = _gpu_mapper(st, cfg), _gpu_mapper(st, cfg)
    sdf_losses(a, coord, label, ts, weight, cl, eikonal=True, color=True)
    hnp.query_feature(b.neural_points, coord, ts)
    na, nb = a.neural_points, b.neural_points
    assert torch.equal(na.local_point_ts_update, nb.local_point_ts_update)
    assert not torch.equal(na.local_point_ts_update.cpu(), torch.as_tensor(st["local_point_ts_update"]))
    # the certainty sum is the one float-atomic accumulation of the query (DESIGN): equal up to the summation order
    assert torch.allclose(na.local_point_certainties, nb.local_point_certainties, rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
def test_no_host_waits_deterministic_and_no_growth():
    import gc

    from pings_amd import _lib
    from pings_amd.sdf_losses import sdf_losses

    st = _state("gs_f32")
    cfg = _cfg(st, d=3, loss_weight_on=True)
    m = _gpu_mapper(st, cfg)
    coord, label, ts, weight, cl = (t.cuda() for t in _batch(st, B=600, seed=6))
    params = _params(m)
    cert0 = m.neural_points.local_point_certainties.clone()

    def step():
        m.neural_points.local_point_certainties.copy_(cert0)
        S = sdf_losses(m, coord, label, ts, weight, cl, eikonal=True, color=True)
        tot = S.bce + 0.5 * S.eikonal + 0.8 * S.color
        return [S.bce.detach().clone(), S.eikonal.detach().clone(), S.color.detach().clone(),
                S.counts.clone()], torch.autograd.grad(tot, params)

    step()                                       # first query of the map builds its search index (cached)
    torch.cuda.synchronize()
    _lib.sync_counts(reset=True)
    probe = torch.ones(1, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):        # positive control: the mode catches a device-to-host read
            probe.sum().item()
        v1, g1 = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert _lib.sync_counts() == {}
    v2, g2 = step()
    for x, y in zip(v1 + list(g1), v2 + list(g2)):
        assert torch.equal(x, y)
    gc.disable()
    try:
        step()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() <= base
    finally:
        gc.enable()


@pytest.mark.gpu
def test_render_image_gaussian_and_sdf_blocks_record_only_the_render_sync():
    """render -> image_losses -> gaussian_losses -> sdf_losses (colour on) -> backward(): the host waits of the whole
    joint iteration are the render's own."""
    import warnings

    from pings_amd import _lib
    from pings_amd.gaussian_losses import gaussian_losses
    from pings_amd.image_losses import image_losses
    from pings_amd.renderer import render
    from pings_amd.sdf_losses import sdf_losses
    from test_render import _scene as render_scene

    dev = "cuda"
    data, decs, cam, geo, cfe = render_scene(dev, "gaussian_surfel", hidden=128)
    bg = torch.tensor([0.2, 0.4, 0.6], device=dev)
    gg = torch.Generator(device=dev).manual_seed(1)
    gt = torch.rand(3, 96, 160, generator=gg, device=dev)
    gtd = 3.0 + torch.rand(1, 96, 160, generator=gg, device=dev)
    sky = torch.zeros(1, 96, 160, dtype=torch.bool, device=dev)
    st = _state("gs_f32")
    cfg = _cfg(st, d=3, bs=512, gaussian_bs_ratio=1.0, min_alpha=0.05, gs_contribution_threshold=0.1,
               gs_consist_shift_count=1, gs_consist_shift_range_m=0.05, valid_grad_min_thre=0.05,
               valid_grad_max_thre=50.0)
    m = _gpu_mapper(st, cfg)
    coord, label, ts, weight, cl = (t.cuda() for t in _batch(st, B=512, seed=8))
    gen = torch.Generator(device=dev).manual_seed(4)

    def step(with_losses):
        pkg = render(cam, None, data, decs, None, bg, view_concat_on=True, learn_color_residual=True, d2n_on=True,
                     gs_type="gaussian_surfel")
        if not with_losses:
            return
        il = image_losses(pkg["render"], gt, pkg["surf_depth"], gtd, pkg["rend_alpha"], pkg["rend_normal"],
                          pkg["surf_normal"], sky, depth_min=0.3, depth_max=80.0, depth_min_accu_alpha=0.4)
        G = gaussian_losses(m, pkg, gs_type="gaussian_surfel", generator=gen)
        S = sdf_losses(m, coord, label, ts, weight, cl, eikonal=True, color=True, color_weighted=False)
        loss = 0.8 * il.rgb_l1 + 0.5 * il.depth_l1 + G.opacity + G.area + torch.nan_to_num(G.sdf_cons) + \
            torch.nan_to_num(G.sdf_normal_cons) + S.bce + 0.5 * S.eikonal + 0.8 * S.color
        loss.backward()

    step(True)                                   # warm-up: map search index, size tables
    torch.cuda.synchronize()
    counts = {}
    for with_losses in (False, True):
        _lib.sync_counts(reset=True)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                step(with_losses)
            finally:
                torch.cuda.set_sync_debug_mode(0)
        torch.cuda.synchronize()
        sc = _lib.sync_counts()
        sc.pop("settings_tensor_readback", None)
        counts[with_losses] = (sc, sum("synchroniz" in str(x.message).lower() for x in w))
    assert counts[False][0] == {"raster_instance_count": 1}
    assert counts[True] == counts[False]
