"""Gaussian-space loss block (pings_amd.gaussian_losses, csrc/gauss_loss.hip) against the fp64 restatement of
utils/mapper.py:1331-1483 (tests/gauss_losses_ref.py) on the oracle's SDF map."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import gauss_losses_ref as ref
from conftest import rel_err
from oracle import sdf_cpu

NAMES = ["opacity", "opacity_ent", "isotropic", "area", "sdf_cons", "sdf_normal_cons", "invalid_opacity"]
WEIGHTS = [0.7, 1.3, 0.9, 1.1, 2.0, 1.7, 0.6]
SCOLS = {"gaussian_surfel": 3, "3d_gs": 3, "2d_gs": 2}


def _state(name="gs_f32"):
    from pathlib import Path

    z = np.load(Path(__file__).parent / "golden" / f"sdf_{name}.npz")
    return {k: z[k] for k in z.files}


def _cfg(R=1, cap=256, **kw):
    c = NS(bs=cap, gaussian_bs_ratio=1.0, min_alpha=0.05, gs_contribution_threshold=0.1, gs_consist_shift_count=R,
           gs_consist_shift_range_m=0.05, valid_grad_min_thre=0.05, valid_grad_max_thre=50.0, voxel_size_m=0.3)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _scene(st, P=600, gs_type="gaussian_surfel", seed=0, contrib=True, free=True, dev="cpu"):
    """Gaussians around the golden query points (so that they have map neighbours), as render_pkg tensors."""
    g = torch.Generator().manual_seed(seed)
    x = torch.as_tensor(st["x"], dtype=torch.float32)
    base = x[torch.randint(0, x.shape[0], (P,), generator=g)]
    xyz = base + 0.02 * torch.randn(P, 3, generator=g)
    rot = torch.randn(P, 4, generator=g)
    scale = 0.05 + 0.2 * torch.rand(P, SCOLS[gs_type], generator=g)
    alpha = torch.rand(P, 1, generator=g) * 1.3 - 0.2
    alpha_all = torch.cat((alpha[:, 0], torch.rand(200, generator=g) * 1.4 - 0.3))
    pkg = {"gaussian_xyz": xyz, "gaussian_rot": rot, "gaussian_scale": scale, "gaussian_alpha": alpha,
           "alpha_all": alpha_all, "visibility_filter": torch.rand(P + 50, generator=g) < 0.85,
           "local_view_gaussian_count": P,
           "gaussian_free_mask": (torch.rand(P, generator=g) < 0.1) if free else None}
    if contrib:
        pkg["contributions"] = torch.rand(P + 50, generator=g)
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in pkg.items()}


def _ref_mask(pkg, cfg):
    P = pkg["gaussian_xyz"].shape[0]
    m = pkg["visibility_filter"][:P] & (pkg["gaussian_alpha"] > cfg.min_alpha).squeeze(-1)
    if pkg.get("contributions") is not None:
        m = m & (pkg["contributions"][:P] > cfg.gs_contribution_threshold)
    if pkg.get("gaussian_free_mask") is not None:
        m = m & ~pkg["gaussian_free_mask"]
    return m


# ------------------------------------------------------------------ CPU
def test_restatement_normal_is_third_rotation_column_and_entropy_closed_form():
    q = torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.5, 0.5, 0.5, 0.5]], dtype=torch.float64)
    n = ref.rotation2normal(q)
    # R(q) for a unit quaternion: the third column is R e_z
    want = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]], dtype=torch.float64)
    assert torch.allclose(n, want, atol=1e-12)
    p = torch.tensor([0.5, 1e-9, 0.99], dtype=torch.float64)
    c = p.clamp(1e-6, 1 - 1e-6)
    assert float(ref.opacity_entropy_loss(p)) == pytest.approx(float((-(c * c.log()) - (1 - c) * (1 - c).log()).mean()))


def test_restatement_gate_and_empty_means():
    st = _state()
    cfg = _cfg(R=0)
    pkg = _scene(st, P=40, contrib=False, free=False)
    pkg["visibility_filter"][:] = False
    pkg["visibility_filter"][:5] = True
    pkg["gaussian_alpha"][:5] = 0.5
    out = ref.block(cfg, "gaussian_surfel", pkg["alpha_all"], pkg["visibility_filter"][:40], None, None,
                    pkg["gaussian_xyz"], pkg["gaussian_rot"], pkg["gaussian_scale"], pkg["gaussian_alpha"],
                    lambda x: (x.sum(1), torch.ones(len(x), dtype=torch.bool)), torch.arange(5), torch.zeros(0),
                    isotropic=True)
    assert out[2:] == [0.0] * 5                # constraint count 5 <= 10: every sampled term is 0


def test_argument_validation():
    from pings_amd import gaussian_losses as gl

    st = _state()
    m = NS(config=_cfg())
    pkg = _scene(st, P=30)
    with pytest.raises(ValueError, match="gs_type"):
        gl.gaussian_losses(m, pkg, gs_type="4d_gs")
    with pytest.raises(Exception, match="HIP device only"):
        gl.gaussian_losses(m, pkg, gs_type="gaussian_surfel")
    bad = dict(pkg, gaussian_scale=pkg["gaussian_scale"][:, :2])
    with pytest.raises(ValueError, match="gaussian_scale"):
        gl.gaussian_losses(m, bad, gs_type="3d_gs")
    with pytest.raises(ValueError, match="gaussian_scale"):
        gl.gaussian_losses(m, pkg, gs_type="2d_gs")
    nolocal = {k: v for k, v in pkg.items() if k != "local_view_gaussian_count"}
    with pytest.raises(ValueError, match="local_view_gaussian_count"):
        gl.gaussian_losses(m, nolocal, gs_type="gaussian_surfel")


# ------------------------------------------------------------------ GPU
def _gpu_map(st):
    npm = sdf_cpu.NeuralPointMap(st, device="cuda")
    npm.config = NS(query_nn_k=npm.nn_k, weighted_first=npm.weighted_first, layer_norm_on=False)
    npm.color_feature_dim = npm.color_features.shape[1] if npm.color_features is not None else 0
    return npm


def _mapper(st, cfg):
    gpu = _gpu_map(st)
    gpu.local_geo_features.requires_grad_(True)
    t = lambda k: torch.nn.Parameter(torch.as_tensor(st["dec." + k]).cuda())
    dec = NS(layers=[NS(weight=t("layers.0.weight"), bias=t("layers.0.bias"))],
             lout=NS(weight=t("lout.weight"), bias=t("lout.bias")), sdf_scale=float(st["sdf_scale"]),
             use_leaky_relu=False)
    return NS(config=cfg, neural_points=gpu, sdf_mlp=dec, dtype=torch.float32, device="cuda")


def _ref_sdf(st, feats64, dec64):
    cpu = sdf_cpu.NeuralPointMap(st)
    for k, v in list(vars(cpu).items()):
        if torch.is_tensor(v) and v.dtype == torch.float32:
            setattr(cpu, k, v.double())
    cpu.dtype = torch.float64
    cpu.local_geo_features = feats64

    def sdf(x):
        s, cnt = sdf_cpu.mapper_sdf(cpu, dec64, x)
        return s, cnt >= 3
    return sdf


def _run_both(st, gs_type, R, contrib=True, free=True, cap=256, P=600, seed=0, flags=None, weights=WEIGHTS):
    """HIP block with an injected sample vs the fp64 restatement: (values hip, values ref, grads hip, grads ref)."""
    from pings_amd.gaussian_losses import gaussian_losses

    flags = flags or dict(opacity=True, opacity_ent=True, isotropic=True, area=True, sdf_consistency=True)
    cfg = _cfg(R=R, cap=cap)
    m = _mapper(st, cfg)
    pkg = _scene(st, P=P, gs_type=gs_type, seed=seed, contrib=contrib, free=free, dev="cuda")
    for k in ("gaussian_xyz", "gaussian_rot", "gaussian_scale", "gaussian_alpha", "alpha_all"):
        pkg[k] = pkg[k].clone().requires_grad_(True)
    mask = _ref_mask(pkg, cfg).cpu()
    true_idx = torch.where(mask)[0]
    g = torch.Generator().manual_seed(seed + 7)
    S = min(len(true_idx), cap)
    idx = true_idx[torch.randperm(len(true_idx), generator=g)[:S]]
    z = torch.randn(R * S, generator=g)
    G = gaussian_losses(m, pkg, gs_type=gs_type, _sample=(idx.cuda(), z.cuda()), **flags)
    dec, npm = m.sdf_mlp, m.neural_points
    params = [pkg[k] for k in ("gaussian_xyz", "gaussian_rot", "gaussian_scale", "gaussian_alpha", "alpha_all")] + \
             [npm.local_geo_features, dec.layers[0].weight, dec.layers[0].bias, dec.lout.weight, dec.lout.bias]
    vals = list(G[:7])
    tot = sum(w * v for w, v in zip(weights, vals) if bool(torch.isfinite(v)))
    gh = torch.autograd.grad(tot, params, allow_unused=True)
    # fp64 reference on the CPU
    p64 = [p.detach().cpu().double().requires_grad_(True) for p in params]
    dec64 = sdf_cpu.MLP(p64[6], p64[7], p64[8], p64[9], float(st["sdf_scale"]))
    sdf = _ref_sdf(st, p64[5], dec64)
    pk = {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in pkg.items()}
    P_ = pk["gaussian_xyz"].shape[0]
    rv = ref.block(cfg, gs_type, p64[4], pk["visibility_filter"][:P_],
                   pk["contributions"][:P_].double() if contrib else None, pk["gaussian_free_mask"], p64[0], p64[1],
                   p64[2], p64[3], sdf, idx, z.double(), **flags)
    rv = [torch.as_tensor(v, dtype=torch.float64) for v in rv]
    rtot = sum(w * v for w, v in zip(weights, rv) if bool(torch.isfinite(v)) and v.requires_grad)
    gr = torch.autograd.grad(rtot, p64, allow_unused=True)
    return G, vals, rv, gh, gr


def _close(a, b, tol=1e-4):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    if torch.isnan(b).all():
        return torch.isnan(a).all()
    return rel_err(a, b) <= tol


@pytest.mark.gpu
@pytest.mark.parametrize("gs_type", ["gaussian_surfel", "3d_gs", "2d_gs"])
@pytest.mark.parametrize("R", [0, 1, 2])
def test_values_and_gradients_match_fp64_restatement(gs_type, R):
    st = _state()
    cap = 256 if R == 0 else 512                       # R = 0: the sample is cut at cap; else S < cap (dead rows)
    G, vals, rv, gh, gr = _run_both(st, gs_type, R, contrib=(R != 1), free=(R != 2), cap=cap)
    assert (float(G.counts[2]) == cap) if R == 0 else (float(G.counts[2]) < cap)
    for n, a, b in zip(NAMES, vals, rv):
        assert _close(a, b), (n, float(a), float(b))
    for i, (a, b) in enumerate(zip(gh, gr)):
        if b is None:
            continue
        a = torch.zeros_like(b) if a is None else a.reshape(b.shape)
        assert rel_err(a.cpu().double(), b) <= 1e-4, (i, rel_err(a.cpu().double(), b))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gs_f32", "pgo_f32"])
def test_sdf_normal_term_reaches_the_gaussian_centres(name):
    """sdf_normal_cons alone: its xyz gradient is H_S(x) v (pings_sdf_hvp_x) and matches fp64 autograd."""
    st = _state(name)
    w = [0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    G, vals, rv, gh, gr = _run_both(st, "gaussian_surfel", 1, weights=w)
    assert float(gr[0].abs().max()) > 0
    assert float(gh[0].abs().max()) > 0
    assert rel_err(gh[0].cpu().double(), gr[0]) <= 1e-4


@pytest.mark.gpu
@pytest.mark.xfail(strict=True, raises=AssertionError, reason="Mapper.sdf + get_gradient on the fused node drops d/dx of dS/dx (DESIGN §8)")
def test_fused_mapper_sdf_second_order_misses_the_query_gradient():
    from pings_amd import mapper_ops

    st = _state()
    m = _mapper(st, _cfg())
    m.config.weighted_first = False
    x = torch.as_tensor(st["x"][:200]).cuda().requires_grad_(True)
    s, _, _ = mapper_ops.sdf(m, x, min_nn_count=1)
    g = ref.get_gradient(x, s)
    (gx,) = torch.autograd.grad(g.norm(dim=1).sum(), x, allow_unused=True)
    gx = torch.zeros_like(x) if gx is None else gx             # the fused node returns no gradient to x
    dec = m.sdf_mlp
    p64 = [t.detach().cpu().double() for t in (dec.layers[0].weight, dec.layers[0].bias, dec.lout.weight, dec.lout.bias)]
    sdf = _ref_sdf(st, m.neural_points.local_geo_features.detach().cpu().double(), sdf_cpu.MLP(*p64, float(st["sdf_scale"])))
    x64 = x.detach().cpu().double().requires_grad_(True)
    g64 = ref.get_gradient(x64, sdf(x64)[0])
    (gx64,) = torch.autograd.grad(g64.norm(dim=1).sum(), x64)
    assert rel_err(gx.cpu().double(), gx64) <= 1e-4


@pytest.mark.gpu
def test_gate_no_low_alpha_and_nan_invalid():
    from pings_amd.gaussian_losses import gaussian_losses

    st = _state()
    m = _mapper(st, _cfg(R=1))
    pkg = _scene(st, P=300, dev="cuda")
    pkg["gaussian_xyz"].requires_grad_(True)
    pkg["gaussian_scale"].requires_grad_(True)
    # constraint count <= 10: exact zeros and zero gradients
    pkg["visibility_filter"][:] = False
    pkg["visibility_filter"][:10] = True
    pkg["gaussian_alpha"][:10] = 0.5
    pkg["contributions"] = None
    pkg["gaussian_free_mask"] = None
    G = gaussian_losses(m, pkg, gs_type="gaussian_surfel", isotropic=True)
    assert float(G.counts[1]) == 10 and float(G.counts[2]) == 0
    assert all(float(v) == 0.0 for v in G[2:7])
    gx, gs = torch.autograd.grad(sum(G[2:7]), [pkg["gaussian_xyz"], pkg["gaussian_scale"]])
    assert float(gx.abs().max()) == 0 and float(gs.abs().max()) == 0
    # no alpha below min_alpha: opacity loss 0
    pkg["alpha_all"] = torch.rand(500, device="cuda") + 0.1
    G = gaussian_losses(m, pkg, gs_type="gaussian_surfel")
    assert float(G.opacity) == 0.0 and float(G.counts[0]) == 0
    # every sample valid: invalid_opacity is the mean of an empty selection, NaN as torch
    # (R = 0, no gradient-norm bounds, and a sample of Gaussians whose centre has at least 3 map neighbours; a zero
    # SDF gradient is then a valid row and its backward stays finite)
    from pings_amd import mapper_ops

    m.config.valid_grad_min_thre, m.config.valid_grad_max_thre, m.config.gs_consist_shift_count = -1.0, 1e30, 0
    pkg["visibility_filter"][:] = True
    pkg["gaussian_alpha"][:] = 0.5
    with torch.no_grad():
        _, _, ok = mapper_ops.sdf(m, pkg["gaussian_xyz"].detach(), min_nn_count=3)
    ids = torch.where(ok)[0][:64]
    assert len(ids) > 10
    G = gaussian_losses(m, pkg, gs_type="gaussian_surfel", _sample=(ids, torch.zeros(0, device="cuda")))
    assert float(G.counts[4]) == 0 and float(G.counts[3]) == len(ids)
    assert torch.isnan(G.invalid_opacity)
    (gx,) = torch.autograd.grad(G.sdf_cons + G.sdf_normal_cons, [pkg["gaussian_xyz"]])
    assert bool(torch.isfinite(gx).all())


@pytest.mark.gpu
def test_sampler_subset_uniform_and_seeded():
    from pings_amd.gaussian_losses import gaussian_losses

    st = _state()
    cap = 64
    m = _mapper(st, _cfg(R=0, cap=cap))
    pkg = _scene(st, P=400, dev="cuda")
    pkg["alpha_all"].requires_grad_(True)                 # a graph node, so that the draw can be read from it
    mask = _ref_mask(pkg, m.config)
    count = int(mask.sum())
    assert count > cap
    freq = torch.zeros(400, dtype=torch.float64)
    draws = 300
    for i in range(draws):
        gen = torch.Generator(device="cuda").manual_seed(1000 + i)
        G = gaussian_losses(m, pkg, gs_type="gaussian_surfel", sdf_consistency=False, generator=gen)
        # the drawn set (through the autograd state of the node)
        idx = G.opacity.grad_fn.B["idx"][:int(G.counts[2])].long().cpu()
        assert len(idx) == min(count, cap) and len(torch.unique(idx)) == len(idx)
        assert bool(mask.cpu()[idx].all())
        freq[idx] += 1
    e = draws * cap / count
    chi2 = float((((freq[mask.cpu()] - e) ** 2) / e).sum())
    dof = count - 1
    assert chi2 < dof + 5 * (2 * dof) ** 0.5, (chi2, dof)
    a = [gaussian_losses(m, pkg, gs_type="gaussian_surfel", generator=torch.Generator(device="cuda").manual_seed(5))
         for _ in range(2)]
    assert torch.equal(a[0].opacity.grad_fn.B["idx"], a[1].opacity.grad_fn.B["idx"])


@pytest.mark.gpu
def test_no_host_waits_deterministic_and_no_growth():
    import gc

    from pings_amd import _lib
    from pings_amd.gaussian_losses import gaussian_losses

    st = _state()
    m = _mapper(st, _cfg(R=1))
    pkg = _scene(st, P=600, dev="cuda")
    for k in ("gaussian_xyz", "gaussian_rot", "gaussian_scale", "gaussian_alpha", "alpha_all"):
        pkg[k] = pkg[k].clone().requires_grad_(True)
    params = [pkg["gaussian_xyz"], pkg["gaussian_rot"], m.neural_points.local_geo_features]

    def step():
        G = gaussian_losses(m, pkg, gs_type="gaussian_surfel", isotropic=True,
                            generator=torch.Generator(device="cuda").manual_seed(3))
        tot = G.opacity + G.area + G.isotropic + torch.nan_to_num(G.sdf_cons) + torch.nan_to_num(G.sdf_normal_cons)
        return [G[i].detach().clone() for i in range(7)], torch.autograd.grad(tot, params)

    step()                                       # first query of the map builds its search index (one read-back, cached)
    torch.cuda.synchronize()
    _lib.sync_counts(reset=True)
    # positive control: the mode does catch a device-to-host read on this torch build
    probe = torch.ones(1, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.sum().item()
        v1, g1 = step()                          # raises on any synchronising call inside the block
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert _lib.sync_counts() == {}
    v2, g2 = step()
    for a, b in zip(v1 + list(g1), v2 + list(g2)):
        assert torch.equal(a.nan_to_num(), b.nan_to_num())
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


# ------------------------------------------------------------------ golden vectors of the reference's own helpers
GOLDEN = ["surfel_r1", "gs3d_r2", "gs2d_r0"]
LEAVES = ["gaussian_xyz", "gaussian_rot", "gaussian_scale", "gaussian_alpha", "alpha_all"]


def _golden(name):
    from pathlib import Path

    z = np.load(Path(__file__).parent / "golden" / f"gaussloss_{name}.npz")
    return {k: z[k] for k in z.files}


def _golden_pkg(gd, dev):
    P = gd["gaussian_xyz"].shape[0]
    pkg = {k: torch.as_tensor(gd[k]).to(dev) for k in LEAVES}
    pkg.update(visibility_filter=torch.as_tensor(gd["visible"]).to(dev), local_view_gaussian_count=P,
               gaussian_free_mask=torch.as_tensor(gd["free_mask"]).to(dev) if "free_mask" in gd else None)
    if "contributions" in gd:
        pkg["contributions"] = torch.as_tensor(gd["contributions"]).to(dev)
    return pkg


@pytest.mark.parametrize("name", GOLDEN)
def test_restatement_matches_reference_helpers_golden(name):
    """tests/gauss_losses_ref.py against vectors made with the reference's rotation2normal, opacity_entropy_loss,
    get_gradient and the inline lines of utils/mapper.py:1331-1483 (tools/make_gaussloss_golden.py)."""
    gd = _golden(name)
    st = _state()
    gs_type, R = str(gd["gs_type"]), int(gd["R"])
    cfg = _cfg(R=R, cap=512)
    pkg = _golden_pkg(gd, "cpu")
    leaves = [pkg[k].double().requires_grad_(True) for k in LEAVES]
    feats = torch.as_tensor(st["local_geo_features"]).double().requires_grad_(True)
    dec = sdf_cpu.MLP(*(torch.as_tensor(st["dec." + k]).double() for k in
                        ("layers.0.weight", "layers.0.bias", "lout.weight", "lout.bias")), float(st["sdf_scale"]))
    P = leaves[0].shape[0]
    vals = ref.block(cfg, gs_type, leaves[4], pkg["visibility_filter"][:P],
                     pkg["contributions"][:P].double() if "contributions" in pkg else None, pkg["gaussian_free_mask"],
                     leaves[0], leaves[1], leaves[2], leaves[3], _ref_sdf(st, feats, dec),
                     torch.as_tensor(gd["idx"]), torch.as_tensor(gd["randn"]).double(), opacity=True, opacity_ent=True,
                     isotropic=True, area=True, sdf_consistency=True)
    vals = [torch.as_tensor(v, dtype=torch.float64) for v in vals]
    assert np.allclose([float(v) for v in vals], gd["values"], rtol=1e-10, atol=1e-12, equal_nan=True)
    tot = sum(w * v for w, v in zip(gd["weights"], vals) if bool(torch.isfinite(v)) and v.requires_grad)
    grads = torch.autograd.grad(tot, leaves + [feats])
    for k, g in zip(LEAVES + ["local_geo_features"], grads):
        assert np.allclose(g.numpy(), gd["d_" + k], rtol=1e-9, atol=1e-12), k


@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDEN)
def test_fused_block_matches_reference_helpers_golden(name):
    from pings_amd.gaussian_losses import gaussian_losses

    gd = _golden(name)
    st = _state()
    m = _mapper(st, _cfg(R=int(gd["R"]), cap=512))
    pkg = _golden_pkg(gd, "cuda")
    for k in LEAVES:
        pkg[k].requires_grad_(True)
    G = gaussian_losses(m, pkg, gs_type=str(gd["gs_type"]), opacity=True, opacity_ent=True, isotropic=True, area=True,
                        sdf_consistency=True, _sample=(torch.as_tensor(gd["idx"]).cuda(),
                                                       torch.as_tensor(gd["randn"]).cuda()))
    for n, v, want in zip(NAMES, G[:7], gd["values"]):
        assert _close(v, torch.as_tensor(want)), (n, float(v), float(want))
    tot = sum(float(w) * v for w, v in zip(gd["weights"], G[:7]) if bool(torch.isfinite(v)))
    grads = torch.autograd.grad(tot, [pkg[k] for k in LEAVES] + [m.neural_points.local_geo_features])
    for k, g in zip(LEAVES + ["local_geo_features"], grads):
        assert rel_err(g.cpu().double(), torch.as_tensor(gd["d_" + k])) <= 1e-4, k


@pytest.mark.gpu
def test_render_losses_and_gaussian_block_record_only_the_render_sync():
    """render -> image_losses -> fused_ssim -> gaussian_losses -> backward(): the host waits of the whole iteration are
    the render's own (the library's instrumented count and torch's sync-debug warnings both)."""
    import warnings

    from pings_amd import _lib
    from pings_amd.image_losses import image_losses
    from pings_amd.renderer import render
    from pings_amd.ssim import fused_ssim
    from test_render import _scene as render_scene

    dev = "cuda"
    data, decs, cam, geo, cfe = render_scene(dev, "gaussian_surfel", hidden=128)   # the one-sync decoders
    bg = torch.tensor([0.2, 0.4, 0.6], device=dev)
    gg = torch.Generator(device=dev).manual_seed(1)
    gt = torch.rand(3, 96, 160, generator=gg, device=dev)
    gtd = 3.0 + torch.rand(1, 96, 160, generator=gg, device=dev)
    sky = torch.zeros(1, 96, 160, dtype=torch.bool, device=dev)
    st = _state()
    m = _mapper(st, _cfg(R=1, cap=512))
    gen = torch.Generator(device=dev).manual_seed(4)

    def step(with_losses):
        pkg = render(cam, None, data, decs, None, bg, view_concat_on=True, learn_color_residual=True, d2n_on=True,
                     gs_type="gaussian_surfel")
        if not with_losses:
            return
        il = image_losses(pkg["render"], gt, pkg["surf_depth"], gtd, pkg["rend_alpha"], pkg["rend_normal"],
                          pkg["surf_normal"], sky, depth_min=0.3, depth_max=80.0, depth_min_accu_alpha=0.4)
        ssim = fused_ssim(pkg["render"].unsqueeze(0), gt.unsqueeze(0))
        G = gaussian_losses(m, pkg, gs_type="gaussian_surfel", generator=gen)
        loss = 0.8 * il.rgb_l1 + 0.2 * (1.0 - ssim) + 0.5 * il.depth_l1 + G.opacity + G.area + \
            torch.nan_to_num(G.sdf_cons) + torch.nan_to_num(G.sdf_normal_cons)
        loss.backward()

    from pings_amd.gaussian_losses import gaussian_losses

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
        sc.pop("settings_tensor_readback", None)     # the camera's principal point, read once per camera tensor
        counts[with_losses] = (sc, sum("synchroniz" in str(x.message).lower() for x in w))
    assert counts[False][0] == {"raster_instance_count": 1}
    assert counts[True] == counts[False]
