"""Marching cubes on the device (pings_amd/csrc/mc.hip, pings_amd/mesher_ops.py: marching_cubes).

The CPU tests check the numpy restatement (tests/mc_ref.py) against the geometry it promises; the GPU tests compare
the device output with the restatement array for array (same order, same bits)."""
import ctypes
import warnings
from collections import Counter
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import abi_header as hdr
import mc_ref
from pings_amd import _abi

MC_SYMBOLS = ["pings_mc_scratch_bytes", "pings_mc_count", "pings_mc_emit"]


def _centred(n):
    x = np.arange(n, dtype=np.float32) - np.float32((n - 1) / 2)
    return np.meshgrid(x, x, x, indexing="ij")


def sphere(n=24, r=8.3):
    X, Y, Z = _centred(n)
    return (np.sqrt(X * X + Y * Y + Z * Z) - np.float32(r)).astype(np.float32)


def torus(n=24, R=7.0, r=2.6):
    X, Y, Z = _centred(n)
    return ((np.sqrt(X * X + Y * Y) - np.float32(R)) ** 2 + Z * Z - np.float32(r * r)).astype(np.float32)


def noise(n=32, seed=0):
    """Random values padded by positive ones: ambiguous faces everywhere, surface closed inside the box."""
    v = np.ones((n, n, n), np.float32)
    v[2:-2, 2:-2, 2:-2] = np.random.default_rng(seed).standard_normal((n - 4,) * 3).astype(np.float32)
    return v


def int_zeros(n=16, seed=1):
    v = np.ones((n, n, n), np.float32)
    v[2:-2, 2:-2, 2:-2] = np.random.default_rng(seed).integers(-1, 2, (n - 4,) * 3)
    return v


def waves(shape=(160, 130, 110)):
    i, j, k = (np.arange(s, dtype=np.float32) for s in shape)
    return (np.sin(i[:, None, None] * np.float32(0.3)) * np.cos(j[None, :, None] * np.float32(0.27))
            + np.sin(k[None, None, :] * np.float32(0.31))).astype(np.float32)


def directed_edges(f):
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return Counter(map(tuple, e[e[:, 0] != e[:, 1]]))


def unbalanced(f):
    """Directed edges not matched by as many uses in the opposite direction (0 for a watertight mesh)."""
    c = directed_edges(f)
    return sum(1 for (a, b), k in c.items() if c.get((b, a), 0) != k)


def euler(v, f):
    c = directed_edges(f)
    assert all(k == 1 and c.get((b, a)) == 1 for (a, b), k in c.items())     # 2-manifold, consistently oriented
    return len(v) - len(c) // 2 + len(f)


def signed_volume(v, f):
    t = v[f].astype(np.float64)
    return np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6


# ---------------------------------------------------------------- CPU: the restatement and the ABI
def test_abi_declares_marching_cubes():
    assert set(MC_SYMBOLS) <= set(hdr.header_symbols())
    assert set(MC_SYMBOLS) <= set(_abi.SIGNATURES)
    d = hdr.defines()
    assert d["PINGS_MC_ALLOW_DEGENERATE"] == _abi.MC_ALLOW_DEGENERATE and d["PINGS_MC_ASCENT"] == _abi.MC_ASCENT


@pytest.mark.parametrize("field,chi", [(sphere, 2), (torus, 0)])
def test_ref_closed_surfaces(field, chi):
    v, f = mc_ref.marching_cubes(field())
    assert f.dtype == np.int64 and v.dtype == np.float32 and len(f) > 1000
    assert euler(v, f) == chi
    assert np.array_equal(np.unique(f), np.arange(len(v)))                    # no unreferenced vertex


def test_ref_vertices_lie_on_their_edges():
    vol, level = sphere(), np.float32(0.25)
    v, _ = mc_ref.marching_cubes(vol, level)
    frac = v != np.floor(v)
    assert (frac.sum(1) <= 1).all()                                           # at most one non-integer coordinate
    on = np.nonzero(frac.any(1))[0]
    a = np.argmax(frac[on], 1)
    lo = np.floor(v[on]).astype(np.int64)
    hi = lo.copy()
    hi[np.arange(len(on)), a] += 1
    v0, v1 = vol[tuple(lo.T)], vol[tuple(hi.T)]
    assert ((v0 < level) != (v1 < level)).all()
    t = (v[on, a] - lo[np.arange(len(on)), a]).astype(np.float64)
    assert np.abs(v0 + t * (v1.astype(np.float64) - v0) - level).max() < 1e-4
    pts = np.nonzero(~frac.any(1))[0]                                          # grid-point vertices: value == level
    assert np.all(np.abs(vol[tuple(v[pts].astype(np.int64).T)] - level) <= 1e-6)


def test_ref_winding_follows_gradient_direction():
    vol = sphere()                                   # values decrease inwards
    vd, fd = mc_ref.marching_cubes(vol)
    va, fa = mc_ref.marching_cubes(vol, gradient_direction="ascent")
    assert np.array_equal(vd, va) and np.array_equal(fd[:, [0, 2, 1]], fa)
    assert signed_volume(vd, fd) < 0 < signed_volume(va, fa)                  # 'descent': normals point inwards


def test_ref_noise_is_watertight():
    v, f = mc_ref.marching_cubes(noise())
    assert len(f) > 10000 and unbalanced(f) == 0
    assert np.array_equal(np.unique(f), np.arange(len(v)))


@pytest.mark.parametrize("allow_degenerate", [False, True])
def test_ref_exact_zeros(allow_degenerate):
    vol = int_zeros()
    v, f = mc_ref.marching_cubes(vol, allow_degenerate=allow_degenerate)
    assert unbalanced(f) == 0 and np.array_equal(np.unique(f), np.arange(len(v)))
    deg = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
    assert deg.any() == allow_degenerate
    assert (v == np.round(v)).all(1).sum() > 100                              # grid-point vertices


def test_ref_mask_opens_the_surface():
    vol = sphere()
    m = np.ones(vol.shape, bool)
    m[:12] = False
    v, f = mc_ref.marching_cubes(vol, mask=m)
    assert unbalanced(f) > 0 and v[:, 0].min() >= 12
    full_v, full_f = mc_ref.marching_cubes(vol)
    assert 0.3 < len(f) / len(full_f) < 0.7


# ---------------------------------------------------------------- GPU: exact equality with the restatement
def _golden_grids():
    from pathlib import Path

    z = np.load(Path(__file__).resolve().parent / "golden" / "mesher_grid.npz")
    out = {}
    for name in ("gs_f32", "pin_f8"):
        shape = tuple(int(k) for k in z[f"{name}_num"])
        out[name] = (z[f"{name}_sdf"].reshape(shape).astype(np.float32), z[f"{name}_mask"].reshape(shape))
    return out


def _nonfinite():
    v = sphere()
    v[5, 7, 12], v[12, 12, 4], v[18, 10, 10] = np.nan, np.inf, -np.inf
    return v


def _half_mask():
    m = np.ones((24, 24, 24), np.float32)
    m[:12] = 0
    return m


CASES = {
    "sphere": lambda: (sphere(), {}),
    "torus": lambda: (torus(), {}),
    "noise32": lambda: (noise(32), {}),
    "int_zeros": lambda: (int_zeros(), {}),
    "int_zeros_degenerate": lambda: (int_zeros(), {"allow_degenerate": True}),
    "level": lambda: (sphere(), {"level": 1.7}),
    "ascent": lambda: (noise(20, 3), {"gradient_direction": "ascent"}),
    "half_mask": lambda: (sphere(), {"mask": _half_mask()}),
    "nonfinite": lambda: (_nonfinite(), {}),
    "dims_1": lambda: (noise(8)[:1], {}),
    "dims_2": lambda: (np.random.default_rng(5).standard_normal((2, 2, 2)).astype(np.float32), {}),
    "dims_2x9x2": lambda: (np.random.default_rng(6).standard_normal((2, 9, 2)).astype(np.float32), {}),
    "g11_gs_f32": lambda: (_golden_grids()["gs_f32"][0], {"mask": _golden_grids()["gs_f32"][1]}),
    "g11_pin_f8": lambda: (_golden_grids()["pin_f8"][0], {"mask": _golden_grids()["pin_f8"][1]}),
    "g11_gs_f32_nomask": lambda: (_golden_grids()["gs_f32"][0], {}),
}


def _device_mc(vol, kw):
    from pings_amd import mesher_ops as MO

    kw = dict(kw)
    if "mask" in kw:
        kw["mask"] = torch.from_numpy(kw["mask"]).cuda()
    return MO.marching_cubes(torch.from_numpy(vol).cuda(), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_gpu_matches_restatement(case):
    vol, kw = CASES[case]()
    v, f = _device_mc(vol, kw)
    rv, rf = mc_ref.marching_cubes(vol, **kw)
    assert v.is_cuda and f.is_cuda and v.dtype == torch.float32 and f.dtype == torch.int64
    assert v.shape == (len(rv), 3) and f.shape == (len(rf), 3)
    assert torch.equal(v.cpu(), torch.from_numpy(rv)) and torch.equal(f.cpu(), torch.from_numpy(rf))
    if case.startswith("g11") or case in ("sphere", "noise32"):
        assert len(rf) > 0


@pytest.mark.gpu
def test_gpu_large_grid_matches_restatement_and_is_deterministic():
    vol = waves()
    assert np.prod([s - 1 for s in vol.shape]) >= 2_000_000
    code = sum((vol[(c & 1):vol.shape[0] - 1 + (c & 1), (c >> 1 & 1):vol.shape[1] - 1 + (c >> 1 & 1),
                    (c >> 2 & 1):vol.shape[2] - 1 + (c >> 2 & 1)] < 0).astype(np.int32) << c for c in range(8))
    assert ((code != 0) & (code != 255)).sum() >= 100_000
    v1, f1 = _device_mc(vol, {})
    v2, f2 = _device_mc(vol, {})
    assert torch.equal(v1, v2) and torch.equal(f1, f2)
    rv, rf = mc_ref.marching_cubes(vol)
    assert torch.equal(v1.cpu(), torch.from_numpy(rv)) and torch.equal(f1.cpu(), torch.from_numpy(rf))


@pytest.mark.gpu
def test_gpu_cap_sized_grid():
    """5e8 points (the reference's cap): keys pass 2^31.  A tilted sheet between z = 250 and 251 crosses every vertical
    edge there and nothing else, so V = nx*ny and F = 2 (nx-1)(ny-1) exactly."""
    from pings_amd import mesher_ops as MO

    nx, ny, nz = 1000, 1000, 500
    i = torch.arange(nx, device="cuda", dtype=torch.float32)[:, None]
    j = torch.arange(ny, device="cuda", dtype=torch.float32)[None, :]
    zc = 250.2 + 0.3 * torch.sin(i * 0.01) ** 2 + 0.3 * torch.cos(j * 0.013) ** 2
    vol = torch.arange(nz, device="cuda", dtype=torch.float32)[None, None, :] - zc[:, :, None]
    assert vol.numel() == 500_000_000
    vs = []
    for e in range(3):                               # crossing edges along each axis: the expected vertex count
        a, b = vol.narrow(e, 0, vol.shape[e] - 1), vol.narrow(e, 1, vol.shape[e] - 1)
        vs.append(int(((a < 0) != (b < 0)).sum()))
    assert vs == [0, 0, nx * ny]
    v1, f1 = MO.marching_cubes(vol)
    assert v1.shape == (nx * ny, 3) and f1.shape == (2 * (nx - 1) * (ny - 1), 3)
    v2, f2 = MO.marching_cubes(vol)
    assert torch.equal(v1, v2) and torch.equal(f1, f2)
    assert int(f1.min()) == 0 and int(f1.max()) == nx * ny - 1
    # vertex of column (i, j) sits at index i*ny + j, between z = 250 and 251
    assert torch.equal(v1[:, 0].long() * ny + v1[:, 1].long(), torch.arange(nx * ny, device="cuda"))
    assert bool(((v1[:, 2] > 250) & (v1[:, 2] < 251)).all())
    g = torch.Generator(device="cpu").manual_seed(0)
    cells = torch.randint(0, (nx - 1) * (ny - 1), (4096,), generator=g).cuda()
    f = f1.view(-1, 2, 3)[cells]                     # the two faces of cell (ci, cj): one quad of its 4 columns
    ci, cj = cells // (ny - 1), cells % (ny - 1)
    quad = torch.stack([ci * ny + cj, ci * ny + cj + 1, (ci + 1) * ny + cj, (ci + 1) * ny + cj + 1], 1)
    six = f.reshape(-1, 6)
    assert bool((six.unsqueeze(2) == quad.unsqueeze(1)).any(2).all())        # only the cell's four vertices ...
    assert bool((quad.unsqueeze(2) == six.unsqueeze(1)).any(2).all())        # ... and all of them
    e0 = f[:, 0, [[0, 1], [1, 2], [2, 0]]]                                      # [n, 3 edges, 2]
    e1 = f[:, 1, [[1, 0], [2, 1], [0, 2]]]                                      # the second face's edges, reversed
    shared = (e0.unsqueeze(2) == e1.unsqueeze(1)).all(-1).sum((1, 2))
    assert bool((shared == 1).all())                 # the quad's diagonal, once in each direction


@pytest.mark.gpu
def test_gpu_one_host_read_per_call():
    from pings_amd import _lib, mesher_ops as MO

    vol = torch.from_numpy(noise(24)).cuda()
    mask = torch.ones(vol.shape, device="cuda")
    MO.marching_cubes(vol, mask=mask)
    torch.cuda.synchronize()
    _lib.sync_counts(reset=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            v, f = MO.marching_cubes(vol, mask=torch.ones(vol.shape, device="cuda"))
        finally:
            torch.cuda.set_sync_debug_mode(0)
    assert _lib.sync_counts() == {"mc_count": 1}
    assert [str(x.message) for x in w if "called a synchronizing" in str(x.message)] == []   # torch saw no wait
    assert f.shape[0] > 0


@pytest.mark.gpu
def test_gpu_rejects_bad_arguments():
    from pings_amd import _lib, mesher_ops as MO

    with pytest.raises(_lib.PingsHipError):
        MO.marching_cubes(torch.zeros(4, 4, 4))
    with pytest.raises(ValueError):
        MO.marching_cubes(torch.zeros(4, 4, device="cuda"))
    with pytest.raises(ValueError):
        MO.marching_cubes(torch.zeros(4, 4, 4, device="cuda"), gradient_direction="up")
    L = _lib.lib()
    assert L.pings_mc_scratch_bytes(0, 4, 4) == 0 and L.pings_mc_scratch_bytes(4, -1, 4) == 0
    tot = (ctypes.c_int64 * 2)()
    vol = torch.zeros(4, 4, 4, device="cuda")
    assert L.pings_mc_count(None, None, 4, 4, 4, 0.0, 0, None, tot, None) != 0                 # null volume
    assert L.pings_mc_count(vol.data_ptr(), None, 4, -4, 4, 0.0, 0, vol.data_ptr(), tot, None) != 0   # negative shape
    assert L.pings_mc_count(vol.data_ptr(), None, 4, 4, 4, 0.0, 8, vol.data_ptr(), tot, None) != 0    # unknown flag
    v, f = MO.marching_cubes(torch.zeros(0, 4, 4, device="cuda"))
    assert v.shape == (0, 3) and f.shape == (0, 3) and f.dtype == torch.int64


# ---------------------------------------------------------------- GPU: the Mesher drop-ins
@pytest.mark.gpu
def test_gpu_mc_mesh_dropin():
    from pings_amd import mesher_ops as MO

    vol, m = _golden_grids()["gs_f32"]
    origin, vs = np.array([1.5, -2.0, 0.25]), 0.15
    verts, faces = MO.mc_mesh(NS(), vol.astype(np.float64), m.astype(bool), vs, origin)
    rv, rf = mc_ref.marching_cubes(vol, mask=m)
    assert verts.dtype == np.float64 and faces.dtype == np.int64 and len(rf) > 0
    assert np.array_equal(verts, origin + rv * vs) and np.array_equal(faces, rf)
    ev, ef = MO.mc_mesh(NS(), np.ones((5, 5, 5)), None, vs, origin)            # no surface: the reference's except
    assert ev.shape == (0, 3) and ev.dtype == np.float64 and ef.shape == (0, 3) and ef.dtype == np.float64


@pytest.mark.gpu
def test_gpu_mc_mesh_torch_dropin():
    from pings_amd import mesher_ops as MO

    vol, m = sphere(), _half_mask()
    origin = torch.tensor(np.array([0.5, 1.0, -3.0])).to(torch.from_numpy(vol))
    verts, faces = MO.mc_mesh_torch(NS(), torch.from_numpy(vol), torch.from_numpy(m), 0.2, origin)
    assert verts.is_cuda and faces.is_cuda and verts.dtype == torch.float32 and faces.dtype == torch.int64
    rv, rf = mc_ref.marching_cubes(vol, mask=m)
    want = origin.cuda() + torch.from_numpy(rv).cuda() * 0.2
    assert torch.equal(verts, want) and torch.equal(faces.cpu(), torch.from_numpy(rf))


@pytest.mark.gpu
def test_install_binds_the_mc_methods_only_on_request():
    from pings_amd import mesher_ops as MO

    plain, with_mc = NS(Mesher=type("Mesher", (), {})), NS(Mesher=type("Mesher", (), {}))
    MO.install(plain)
    MO.install(with_mc, mc=True)
    assert plain.Mesher.query_points is MO.query_points
    assert not hasattr(plain.Mesher, "mc_mesh") and not hasattr(plain.Mesher, "mc_mesh_torch")
    assert with_mc.Mesher.mc_mesh is MO.mc_mesh and with_mc.Mesher.mc_mesh_torch is MO.mc_mesh_torch


@pytest.mark.gpu
def test_gpu_mesh_bbx_equals_query_then_marching_cubes(golden_dir):
    from pings_amd import mesher_ops as MO
    from test_sdf import T, _Dec, _gpu_map, load

    name = "gs_f32"
    st = load(golden_dir, name)
    z = np.load(golden_dir / "mesher_grid.npz")
    fake = NS(neural_points=_gpu_map(st), sdf_mlp=_Dec(st), sem_mlp=None, color_mlp=None,
              config=NS(weighted_first=bool(st["weighted_first"]), color_channel=3, pad_voxel=1, skip_top_voxel=1,
                        infer_bs=1000, mc_mask_on=True))
    vs = float(z[f"{name}_voxel"])
    coord, num, origin = MO.grid_from_bbx(z[f"{name}_min"], z[f"{name}_max"], vs, 1, 1, torch.device("cuda"))
    assert torch.equal(coord.cpu(), T(z[f"{name}_coord"])) and np.array_equal(num, z[f"{name}_num"])
    verts, faces = MO.mesh_bbx(fake, z[f"{name}_min"], z[f"{name}_max"], vs, mesh_min_nn=4)
    sdf, _, _, mask = MO.query_points(fake, coord, 1000, True, False, False, True, mask_min_nn_count=4, out_torch=True)
    shape = tuple(int(k) for k in num)
    rv, rf = MO.marching_cubes(sdf.view(shape).cuda(), 0.0, mask.view(shape).cuda())
    want = torch.tensor(origin, dtype=torch.float32, device="cuda") + rv * vs
    assert faces.shape[0] > 0
    assert torch.equal(verts, want) and torch.equal(faces, rf)
