"""The small launches around the blend kernels that were folded into their neighbours: the depth-key
range inside preprocess_kernel, the range fold inside ds_hist_kernel, the host read-back ahead of the instance scan,
the forward tile order straight from `ranges`, the per-tile contributor maximum from blend_fwd_tile_kernel's epilogue,
the chunk counts read by the scan itself, the clears rounded to one fill launch each.

Every knob setting runs in a fresh child process (this file is its own worker: `python test_raster_glue.py SPEC OUT`).
Comparisons against oracle/raster_cpu.py go through the checks of test_raster.py themselves, so the tolerances are
theirs; reproducibility is checked against a second run of the same build."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

HERE = Path(__file__).resolve().parent

# knobs that force the kernels: class-2 pair (wave-per-tile forward, 4-pixels-per-lane backward), class-1 pair (wave per
# quadrant, scan backward), the scan backward with every tile split over four waves, and the defaults
SETTINGS = {
    "class2": {"PINGS_BLEND_PPL": "4", "PINGS_BLEND_BWD": "pixel"},
    "class1": {"PINGS_BLEND_PPL": "-1", "PINGS_BLEND_BWD": "scan"},
    "class1_long": {"PINGS_BLEND_PPL": "-1", "PINGS_BLEND_BWD": "scan", "PINGS_BWD_LONG": "16"},
    "default": {},
}
KNOBS = ("PINGS_BLEND_PPL", "PINGS_BLEND_BWD", "PINGS_BWD_LONG", "PINGS_DEPTH_SORT", "PINGS_RASTER_OCCLUSION",
         "PINGS_BLEND_SEG")


def _child(spec, env, tmp_path, tag):
    """Runs the worker below in a fresh process with exactly `env` of the rasteriser's knobs set; returns what it saved."""
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(env)
    sp, out = tmp_path / f"{tag}.json", tmp_path / f"{tag}.pt"
    sp.write_text(json.dumps(spec))
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(sp), str(out)], env=e, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, f"{tag} {env}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return torch.load(out)


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


# ---------------------------------------------------------------- the tests (parent process)
@pytest.mark.gpu
@pytest.mark.parametrize("mode,seed,W,H", [("surfel", 63, 156, 108), ("3dgs", 62, 150, 100)])
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_folded_launches_match_the_oracle(setting, mode, seed, W, H, tmp_path):
    """Partial tiles in both directions, both modes, both footprint classes' kernels: forward lists / images and the
    gradients under test_raster.py's own checks, the per-tile contributor maximum against torch, backward twice on one
    forward, and a second run of the whole step — all inside the child."""
    got = _child({"what": "step", "mode": mode, "seed": seed, "W": W, "H": H}, SETTINGS[setting], tmp_path, "step")
    assert int(got["n_tiles_checked"]) == ((W + 15) // 16) * ((H + 15) // 16)


@pytest.mark.gpu
@pytest.mark.parametrize("survivors", [0, 1])
def test_empty_and_single_key_range(survivors, tmp_path):
    """Every Gaussian culled (no key reaches the range shards: kmin = 0xFFFFFFFF, shift 0) and exactly one survivor
    (max key = min key), through the bucket sort and through the library sort: same bits, and the oracle's image."""
    spec = {"what": "degenerate", "survivors": survivors}
    a = _child(spec, {}, tmp_path, "bucket")
    b = _child(spec, {"PINGS_DEPTH_SORT": "l"}, tmp_path, "library")
    _assert_same(a, b, f"survivors={survivors}")
    assert int((a["radii"] > 0).sum()) == survivors


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["random_with_ties", "single_depth_plane"])
def test_library_sort_and_overflow_retry_give_the_bucket_sort_bits(scene, tmp_path):
    """test_bucket_depth_sort_is_the_library_sort's scenes across processes: the default path (bucket sort; the plane
    overflows a bucket and the frame is redone with the library sort, after a summary that was queued ahead of the
    instance scan) against PINGS_DEPTH_SORT=l, and against a second run."""
    spec = {"what": "depth_sort", "scene": scene}
    a = _child(spec, {}, tmp_path, "bucket")
    a2 = _child(spec, {}, tmp_path, "bucket2")
    b = _child(spec, {"PINGS_DEPTH_SORT": "l"}, tmp_path, "library")
    _assert_same(a, a2, scene)
    _assert_same(a, b, scene)
    assert float(a["out0"].abs().sum()) > 0


# ---------------------------------------------------------------- the worker (child process)
def _binning_field(fs, name):
    """A uint32 array of the binning blob, by the layout of carve_binning (csrc/raster_layout.hip): 256-byte aligned
    fields in declaration order.  Guarded below by fields whose contents are known (ranges, the forward tile order)."""
    nt = ((fs.prep.W + 15) // 16) * ((fs.prep.H + 15) // 16)
    n = max(int(fs.I), 1)
    fields = [("point_list", 4 * n), ("ranges", 8 * nt), ("inst_w", 4 * (n + 1)), ("inst_qmask", n + 1),
              ("inst_cnt", 4 * n), ("inst_wq", 16 * n), ("inst_cntq", 16 * n), ("tile_key", 4 * n),
              ("tile_key_sorted", 4 * n), ("gval", 4 * n), ("slot_val", 4 * n), ("tile_order", 4 * (2 * nt + 4)),
              ("tile_work", 4 * nt), ("tile_maxc", 4 * nt)]
    off = 0
    for f, size in fields:
        if f == name:
            return fs.binning[off:off + size].view(torch.int32).cpu()
        off = (off + size + 255) // 256 * 256
    raise KeyError(name)


def _tile_max(nc, W, H):
    gx, gy = (W + 15) // 16, (H + 15) // 16
    pad = torch.zeros(gy * 16, gx * 16, dtype=torch.int64)
    pad[:H, :W] = nc.reshape(H, W).cpu().to(torch.int64)
    return pad.view(gy, 16, gx, 16).permute(0, 2, 1, 3).reshape(gy * gx, 256).amax(1)


def _worker_step(spec):
    import test_raster as TR
    from pings_amd import rasterizer as hr
    from scenes import hip_settings
    from test_blend_class2 import _edge_scene

    mode, seed, W, H = spec["mode"], spec["seed"], spec["W"], spec["H"]
    mp = pytest.MonkeyPatch()
    res = {}
    # forward lists, n_contrib and images against the oracle: test_raster.py's own check with this process' knobs
    ppl = os.environ.get("PINGS_BLEND_PPL", "0")
    TR.test_forward_indices_bit_exact_and_images_close(mode, True, seed, (700, W, H), "1", ppl, mp)
    # large footprints over partial tiles: gradients under test_raster.py's gate, twice
    sc = _edge_scene(mode, seed, W=W, H=H)
    _, names, ref64, ups = TR._oracle_grads(sc, torch.float64, mode, True)
    _, _, ref32, _ = TR._oracle_grads(sc, torch.float32, mode, True)
    _, got, _ = TR._hip_grads(sc, mode, True, ups)
    TR._assert_grad_gate(names, got, ref64, ref32, f"glue {mode} {W}x{H} {ppl}", flips_allowed=True)
    _, again, _ = TR._hip_grads(sc, mode, True, ups)
    for n_, a, b in zip(names, got, again):
        assert torch.equal(a, b), ("second run", n_)
    # the per-tile maximum the wave-per-tile forward leaves equals torch's, for every tile
    _, prep, fs, _, _ = TR._hip_forward(sc, mode, True)
    _, rg, _, nc = hr.debug_lists(fs)
    want = _tile_max(nc, W, H)
    nt = want.numel()
    assert torch.equal(_binning_field(fs, "ranges").view(nt, 2).to(torch.int64), rg.cpu())   # layout guard
    order = _binning_field(fs, "tile_order")[:nt].to(torch.int64)
    assert torch.equal(order.sort().values, torch.arange(nt))                                              # layout guard
    lens = (rg[:, 1] - rg[:, 0]).cpu()
    assert bool((lens[order][:-1] // 16 >= lens[order][1:] // 16).all())      # forward order: descending by list length / 16
    wave_per_tile = ppl == "4" or (ppl == "0" and fs.fclass == 2 and os.environ.get("PINGS_BLEND_BWD", "pixel") == "pixel")
    if wave_per_tile:
        assert torch.equal(_binning_field(fs, "tile_maxc").to(torch.int64), want)
    assert int(want.max()) > 0
    res["n_tiles_checked"] = torch.tensor(nt)
    # backward twice on ONE forward (retain_graph) gives the same bits, d_theta / d_rho included
    Rz = hr.SurfelGaussianRasterizer if mode == "surfel" else hr.GS3DGaussianRasterizer
    rast = Rz(hip_settings(sc, mode, True))
    d = lambda t: t.to(torch.float32).cuda().contiguous().requires_grad_(True)
    leaves = [d(sc[k]) for k in ("means", "col", "op", "scales", "rot")]
    th = torch.zeros(3, device="cuda", requires_grad=True)
    rh = torch.zeros(3, device="cuda", requires_grad=True)
    out = rast(means3D=leaves[0], means2D=torch.zeros_like(leaves[0]), colors_precomp=leaves[1], opacities=leaves[2],
               scales=leaves[3], rotations=leaves[4], theta=th, rho=rh)
    imgs = [t for t in out if t.is_floating_point() and t.dim() == 3]
    gg = torch.Generator(device="cuda").manual_seed(9)
    ups2 = [torch.randn(t.shape, generator=gg, device="cuda") for t in imgs]
    g1 = torch.autograd.grad(imgs, leaves + [th, rh], ups2, retain_graph=True)
    g2 = torch.autograd.grad(imgs, leaves + [th, rh], ups2)
    for n_, a, b in zip(names, g1, g2):
        assert torch.equal(a, b), ("backward twice", n_)
    assert float(g1[-1].abs().sum()) > 0 and float(g1[-2].abs().sum()) > 0
    return res


def _rast_step(sc, mode, front_only):
    """forward + backward against fixed upstream gradients; every output and gradient on the CPU"""
    from pings_amd import rasterizer as hr
    from scenes import hip_settings

    Rz = hr.SurfelGaussianRasterizer if mode == "surfel" else hr.GS3DGaussianRasterizer
    rast = Rz(hip_settings(sc, mode, front_only, 1.0))
    leaves = [sc[k].to(torch.float32).cuda().contiguous().requires_grad_(True) for k in ("means", "col", "op", "scales", "rot")]
    th = torch.zeros(3, device="cuda", requires_grad=True)
    rh = torch.zeros(3, device="cuda", requires_grad=True)
    out = rast(means3D=leaves[0], means2D=torch.zeros_like(leaves[0]), colors_precomp=leaves[1], opacities=leaves[2],
               scales=leaves[3], rotations=leaves[4], theta=th, rho=rh)
    imgs = [t for t in out if t.is_floating_point() and t.dim() == 3]
    gg = torch.Generator(device="cuda").manual_seed(9)
    torch.autograd.backward(imgs, [torch.randn(t.shape, generator=gg, device="cuda") for t in imgs])
    res = {f"out{i}": t.detach().cpu() for i, t in enumerate(out)}
    res.update({f"grad{i}": t.grad.detach().cpu() for i, t in enumerate(leaves + [th, rh])})
    return res


def _worker_degenerate(spec):
    import test_raster as TR
    from scenes import make_scene

    P, W, H = 300, 150, 100
    sc = make_scene(P, W, H, seed=77, surfel=True)
    V = sc["cam"]["viewmatrix"].to(sc["means"].dtype)
    pc = sc["means"] @ V[:3, :3] + V[3, :3]
    pc[:, 2] = -5.0                      # behind the camera: culled
    if spec["survivors"]:
        pc[0] = torch.tensor([0.0, 0.0, 2.0], dtype=pc.dtype)   # on the optical axis
        sc["op"].view(-1)[0] = 0.8
    sc["means"] = (pc - V[3, :3]) @ torch.linalg.inv(V[:3, :3])
    res = _rast_step(sc, "surfel", False)
    again = _rast_step(sc, "surfel", False)
    for k in res:
        assert torch.equal(res[k], again[k]), ("second run", k)
    o, *_ = TR._oracle(sc, torch.float32, "surfel", False)
    hr, prep, fs, radii, per_g = TR._hip_forward(sc, "surfel", False)
    assert (radii.cpu() == o["radii"]).all()
    _, _, _, nc = hr.debug_lists(fs)
    assert (nc.cpu() == o["n_contrib"]).all()
    assert torch.equal(fs.color.cpu(), res["out0"])
    if spec["survivors"]:
        assert int(nc.max()) == 1
    else:
        assert fs.I == 0 and torch.equal(res["out0"], sc["bg"].float()[:, None, None].expand_as(res["out0"]))
    res["radii"] = radii.cpu()
    return res


def _worker_depth_sort(spec):
    from scenes import make_scene

    W, H = 160, 96
    sc = make_scene(6000, W, H, seed=123, surfel=True)
    V = sc["cam"]["viewmatrix"].to(sc["means"].dtype)
    pc = sc["means"] @ V[:3, :3] + V[3, :3]
    if spec["scene"] == "random_with_ties":
        pc[:, 2] = torch.round(pc[:, 2].abs() * 8) / 8 + 1.0
    else:
        pc[:, 2] = 3.0
    sc["means"] = (pc - V[3, :3]) @ torch.linalg.inv(V[:3, :3])
    return _rast_step(sc, "surfel", False)


if __name__ == "__main__":
    for p in (str(HERE), str(HERE.parent)):
        if p not in sys.path:
            sys.path.insert(0, p)
    spec = json.loads(Path(sys.argv[1]).read_text())
    result = {"step": _worker_step, "degenerate": _worker_degenerate, "depth_sort": _worker_depth_sort}[spec["what"]](spec)
    torch.save(result, sys.argv[2])
