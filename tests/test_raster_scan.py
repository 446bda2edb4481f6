"""The rasteriser's prefix sums (csrc/raster_scan.hip): a reduce and an apply launch in place of hipcub::DeviceScan for
the depth-sort offsets, the instance offsets, the live rows and the chunk offsets, with the backward's tile order riding
in the live scan's reduce launch.  All of it is integer
arithmetic, so every check is exact: the direct entry pings_raster_scan_u32 against torch.cumsum on the CPU, the public
rasteriser against the library scans (PINGS_RASTER_SCAN=l) and against a second run, and the backward's tile order
against the rule it implements.

The public-path runs happen in fresh child processes with the knob in their environment (this file is its own
worker: `python test_raster_scan.py SPEC OUT`)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
KNOBS = ("PINGS_RASTER_SCAN", "PINGS_BLEND_PPL", "PINGS_BLEND_BWD", "PINGS_BWD_LONG", "PINGS_DEPTH_SORT",
         "PINGS_TILE_SORT", "PINGS_RASTER_OCCLUSION", "PINGS_BLEND_SEG")

BLOCK = 4096                    # SCAN_BLOCK of csrc/raster_common.hpp: elements per workgroup, 4 per thread
LONG_TILES_MAX, TOP_BIN = 2048, 1023   # raster_bwd.hip, tile_order_body
U32, LIVE, POP = 0, 1, 2        # `kind` of pings_raster_scan_u32
# lane, wave, workgroup and vector-tail edges; an in-front sum that crosses a wave (more than 64 totals); more totals
# than threads (more than 1,024)
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193, BLOCK * 64 + 1, BLOCK * 1025 + 7)
GUARD = 64


# ---------------------------------------------------------------- the direct entry against torch.cumsum
def _input(kind, n, rng):
    """(what the device reads, what it sums [int64])"""
    if kind == U32:
        v = rng.integers(0, 1001, n, dtype=np.int64)
        return torch.from_numpy(v.astype(np.int32)), torch.from_numpy(v)
    if kind == LIVE:
        pool = np.array([0.0, -0.0, -1.5, -3e-7, 2.0, 7e-6, 1000.0, -1000.0], dtype=np.float32)
        w = pool[rng.integers(0, pool.size, n)]
        return torch.from_numpy(w), torch.from_numpy((w > 0).astype(np.int64))
    m = rng.integers(0, 256, n, dtype=np.int64).astype(np.uint8)
    pop = np.array([bin(x & 15).count("1") for x in range(256)], dtype=np.int64)
    return torch.from_numpy(m), torch.from_numpy(pop[m])


def _device_scan(L, dev_in, n, kind, inclusive, temp):
    from pings_amd import _lib

    out = torch.full((n + GUARD,), -1431655766, dtype=torch.int32, device="cuda")
    _lib.check(L.pings_raster_scan_u32(_lib.ptr(dev_in), n, kind, int(inclusive), _lib.ptr(out), _lib.ptr(temp),
                                       temp.numel(), _lib.stream_ptr(out.device)), "pings_raster_scan_u32")
    out = out.cpu()
    assert bool((out[n:] == -1431655766).all()), "wrote past the output"
    return torch.from_numpy(out[:n].numpy().view(np.uint32).astype(np.int64))


def _check_all_sizes(kind, what):
    from pings_amd import _lib

    L = _lib.lib()
    rng = np.random.default_rng(11 + kind)
    for n in SIZES:
        host, vals = _input(kind, n, rng)
        incl = torch.cumsum(vals, 0)
        want = {True: incl % (1 << 32), False: (incl - vals) % (1 << 32)}
        dev = host.cuda()
        temp = torch.empty(L.pings_raster_scan_bytes(n), dtype=torch.uint8, device="cuda")
        for inclusive in (False, True):
            got = _device_scan(L, dev, n, kind, inclusive, temp)
            assert torch.equal(got, want[inclusive]), (what, kind, n, inclusive)
        assert torch.equal(dev.cpu().view(torch.uint8), host.view(torch.uint8)), (what, kind, n, "input changed")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [U32, LIVE, POP])
def test_direct_entry_is_torch_cumsum(kind, monkeypatch):
    """Exclusive and inclusive sums of every kind at every size of SIZES, values in [0, 1000] (floats: 0.0, -0.0,
    negative and positive; bytes: anything), equal torch.cumsum in int64 taken modulo 2^32, and nothing is written
    behind the output."""
    monkeypatch.delenv("PINGS_RASTER_SCAN", raising=False)
    _check_all_sizes(kind, "own")


@pytest.mark.gpu
def test_direct_entry_library_path_gives_the_same(monkeypatch):
    """The same expectation with PINGS_RASTER_SCAN=l (hipcub::DeviceScan behind the same entry)."""
    monkeypatch.setenv("PINGS_RASTER_SCAN", "l")
    for kind in (U32, LIVE, POP):
        _check_all_sizes(kind, "library")


@pytest.mark.gpu
def test_sums_wrap_modulo_2_to_32(monkeypatch):
    """Elements near 2^32 over two workgroups: sums wrap like the library's."""
    from pings_amd import _lib

    monkeypatch.delenv("PINGS_RASTER_SCAN", raising=False)
    L = _lib.lib()
    n = 2 * BLOCK + 5
    v = np.random.default_rng(5).integers((1 << 32) - 1000, 1 << 32, n, dtype=np.int64)
    dev = torch.from_numpy(v.astype(np.uint32).view(np.int32)).cuda()
    temp = torch.empty(L.pings_raster_scan_bytes(n), dtype=torch.uint8, device="cuda")
    incl = torch.cumsum(torch.from_numpy(v), 0)       # below 2^46: exact in int64
    assert torch.equal(_device_scan(L, dev, n, U32, True, temp), incl % (1 << 32))
    assert torch.equal(_device_scan(L, dev, n, U32, False, temp), (incl - torch.from_numpy(v)) % (1 << 32))


# ---------------------------------------------------------------- through the public rasteriser (child processes)
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


SCENES = ("class2_front", "class1_surfel", "3dgs", "single", "culled")


@pytest.fixture(scope="module")
def public_runs(tmp_path_factory):
    """every scene of SCENES in three processes: default, default again, PINGS_RASTER_SCAN=l"""
    tmp = tmp_path_factory.mktemp("raster_scan")
    spec = {"what": "scenes"}
    return (_child(spec, {}, tmp, "own"), _child(spec, {}, tmp, "own2"), _child(spec, {"PINGS_RASTER_SCAN": "l"}, tmp, "library"))


@pytest.mark.gpu
@pytest.mark.parametrize("scene", SCENES)
def test_public_path_equals_the_library_scans(scene, public_runs):
    """A class-2 frame of 160x128 whose front Gaussian fills the screen (80 tiles: more than 64 live rows, so two
    chunks and owner ranges longer than one), a class-1 surfel frame of 5,000 Gaussians (scan backward: popcount rows;
    chunk scan over two workgroups), 3DGS mode, a single Gaussian, and a frame with everything culled (no instance): every output, every gradient, the sorted list and the
    ranges of the default build equal those of PINGS_RASTER_SCAN=l and of a second default run, bit for bit."""
    a, a2, b = public_runs
    keys = [k for k in a if k.startswith(scene + "/")]
    assert keys and [k for k in b if k.startswith(scene + "/")] == keys == [k for k in a2 if k.startswith(scene + "/")]
    for k in keys:
        assert torch.equal(a[k], a2[k]), ("second run", k)
        assert torch.equal(a[k], b[k]), ("library scans", k)
    I = int(a[scene + "/I"])
    assert (I == 0) == (scene == "culled")
    if scene == "class2_front":
        assert int(a[scene + "/front_tiles"]) > 64 and int(a[scene + "/fclass_bwd_scan"]) == 0
    if scene == "class1_surfel":
        assert int(a[scene + "/fclass_bwd_scan"]) == 1
    if scene != "culled":
        assert float(a[scene + "/grad0"].abs().sum()) > 0


@pytest.mark.gpu
def test_backward_tile_order_after_a_step(tmp_path):
    """The tile order the extra workgroup of the live scan's reduce launch leaves (class-1 frame, split threshold 96):
    a permutation of the tiles, min(work >> 4, 1023) non-increasing along it, and n_long = the tiles of the longest
    prefix of whole bins, from the top down to the threshold's, that holds at most LONG_TILES_MAX."""
    got = _child({"what": "order"}, {"PINGS_BLEND_PPL": "-1", "PINGS_BLEND_BWD": "scan", "PINGS_BWD_LONG": "96"},
                 tmp_path, "order")
    work, order, n_long = got["work"].to(torch.int64), got["order"].to(torch.int64), int(got["n_long"])
    nt = work.numel()
    assert torch.equal(order.sort().values, torch.arange(nt))
    bins = torch.clamp(work >> 4, max=TOP_BIN)
    along = bins[order]
    assert bool((along[:-1] >= along[1:]).all())
    b = 96 >> 4
    counts = torch.bincount(bins, minlength=TOP_BIN + 1).flip(0).cumsum(0)[:TOP_BIN + 1 - b]      # bins 1023 .. b
    ok = torch.nonzero(counts <= LONG_TILES_MAX).flatten()
    want = int(counts[ok[-1]]) if ok.numel() else 0
    assert n_long == want
    assert 0 < n_long < nt, (n_long, nt)      # the threshold does split the frame's tiles


# ---------------------------------------------------------------- the worker (child process)
def _front_scene():
    """_edge_scene at 160x128 with Gaussian 0 moved in front of everything, facing the camera, wider than the image"""
    from test_blend_class2 import _edge_scene

    W, H = 160, 128
    sc = _edge_scene("surfel", 45, W=W, H=H)
    V = sc["cam"]["viewmatrix"].to(sc["means"].dtype)
    pc = sc["means"] @ V[:3, :3] + V[3, :3]
    pc[0] = torch.tensor([0.0, 0.0, 0.7], dtype=pc.dtype)
    sc["means"] = (pc - V[3, :3]) @ torch.linalg.inv(V[:3, :3])
    sc["scales"][0] = torch.tensor([3.0, 3.0, 1e-7], dtype=sc["scales"].dtype)
    sc["op"].view(-1)[0] = 0.3
    # make_scene's cameras are within 0.15 rad of the world axes: half a turn about x faces the surfel's front to the camera
    sc["rot"][0] = torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=sc["rot"].dtype)
    return sc


def _culled(sc):
    V = sc["cam"]["viewmatrix"].to(sc["means"].dtype)
    pc = sc["means"] @ V[:3, :3] + V[3, :3]
    pc[:, 2] = -5.0
    sc["means"] = (pc - V[3, :3]) @ torch.linalg.inv(V[:3, :3])
    return sc


def _step_with_state(sc, mode):
    """test_raster_glue._rast_step, and the forward state its backward ran on"""
    from pings_amd import rasterizer as hr
    from test_raster_glue import _rast_step

    seen, orig = [], hr._forward

    def spy(*a, **k):
        r = orig(*a, **k)
        seen.append(r)
        return r

    hr._forward = spy
    try:
        res = _rast_step(sc, mode, True)
    finally:
        hr._forward = orig
    fs, radii, per_g = seen[-1]
    torch.cuda.synchronize()
    return res, fs, radii, per_g


def _worker_scenes(spec):
    from pings_amd import rasterizer as hr
    from scenes import make_scene
    from test_raster_glue import _binning_field

    class2 = {"PINGS_BLEND_PPL": "4", "PINGS_BLEND_BWD": "pixel"}
    class1 = {"PINGS_BLEND_PPL": "-1", "PINGS_BLEND_BWD": "scan"}
    one = make_scene(1, 96, 64, seed=3, surfel=True, behind_frac=0.0)
    V = one["cam"]["viewmatrix"].to(one["means"].dtype)
    one["means"] = (torch.tensor([[0.0, 0.0, 2.0]], dtype=V.dtype) - V[3, :3]) @ torch.linalg.inv(V[:3, :3])   # on the optical axis
    one["rot"][0] = torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=one["rot"].dtype)
    cases = {
        "class2_front": (_front_scene(), "surfel", class2),
        "class1_surfel": (make_scene(5000, 160, 96, seed=21, surfel=True), "surfel", class1),
        "3dgs": (make_scene(4500, 160, 96, seed=22, surfel=False), "3dgs", {}),
        "single": (one, "surfel", {}),
        "culled": (_culled(make_scene(300, 160, 96, seed=23, surfel=True)), "surfel", {}),
    }
    out = {}
    for name, (sc, mode, env) in cases.items():
        mp = pytest.MonkeyPatch()
        for k, v in env.items():
            mp.setenv(k, v)
        try:
            res, fs, radii, per_g = _step_with_state(sc, mode)
            res["radii"], res["per_gaussian"], res["I"] = radii.cpu(), per_g.cpu(), torch.tensor(fs.I)
            res["ranges"] = _binning_field(fs, "ranges")
            bwd = os.environ.get("PINGS_BLEND_BWD")
            res["fclass_bwd_scan"] = torch.tensor(int(fs.fclass != 2 if bwd is None else bwd != "pixel"))
            if fs.I > 0:
                res["point_list"] = _binning_field(fs, "point_list")
                res["bwd_order_sorted"] = _binning_field(fs, "tile_order")[ranges_nt(fs):2 * ranges_nt(fs)].sort().values
                pl, _, _, _ = hr.debug_lists(fs)
                res["front_tiles"] = (pl == 0).sum().cpu()
        finally:
            mp.undo()
        out.update({f"{name}/{k}": v for k, v in res.items()})
    return out


def ranges_nt(fs):
    return ((fs.prep.W + 15) // 16) * ((fs.prep.H + 15) // 16)


def _worker_order(spec):
    from pings_amd import rasterizer as hr
    from scenes import make_scene
    from test_raster_glue import _binning_field, _tile_max

    W, H = 400, 300
    sc = make_scene(6000, W, H, seed=31, surfel=True)
    _, fs, _, _ = _step_with_state(sc, "surfel")
    nt = ranges_nt(fs)
    _, _, _, nc = hr.debug_lists(fs)
    field = _binning_field(fs, "tile_order")
    work = _binning_field(fs, "tile_work")
    assert torch.equal(work.to(torch.int64), _tile_max(nc, W, H))       # layout guard: tile_max_contrib_kernel's numbers
    return {"work": work, "order": field[nt:2 * nt], "n_long": field[2 * nt]}


if __name__ == "__main__":
    for p in (str(HERE), str(HERE.parent)):
        if p not in sys.path:
            sys.path.insert(0, p)
    spec = json.loads(Path(sys.argv[1]).read_text())
    result = {"scenes": _worker_scenes, "order": _worker_order}[spec["what"]](spec)
    torch.save(result, sys.argv[2])
