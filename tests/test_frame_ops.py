"""The mapper's per-frame point tests (pings_amd/frame_ops.py, csrc/frame.hip) against the reference.

Yardsticks: tests/frame_ref.py (the reference's lines on oracle.sdf_cpu, in float32 op for op and in float64) and
tests/golden/frame_*.npz (inputs, config scalars and outputs of the reference's own `Mapper` functions on the maps of
tests/golden/sdf_*.npz; tools/make_frame_golden.py).

Gates:
  new_samples   decided on copied float32 values: `new_idx` is torch.equal to the restatement at every size and to the
                fixture at the fixture's size; ratio and iteration offset equal.
  masks         a row is undecidable when the float64 value of sdf, |sdf| or |grad| lies within 1e-4 * max |ref| of the
                threshold it is compared with (the parity gate of the SDF query); every other row must agree
                exactly.  At most 1 % of a case's rows are undecidable and each outcome holds at least 5 % of the rows
                among the decidable ones: properties of the scenario, asserted on the CPU from float64 alone.
The large cases are computed once per process and sliced: a row's decision does not depend on the batch around it.
"""
import ctypes
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import abi_header as hdr
import frame_ref as FR
from conftest import GOLDEN
from oracle import sdf_cpu

FRAME_SYMBOLS = ["pings_frame_new_scratch_bytes", "pings_frame_new_count", "pings_frame_new_rows",
                 "pings_frame_static_mask", "pings_frame_valid_scatter"]
N_MAX = FR.SIZES[-1]


# ================================================================ scenario
@functools.lru_cache(maxsize=None)
def _state(case):
    return FR.load_state(GOLDEN, case)


@functools.lru_cache(maxsize=None)
def _fixture(case):
    with np.load(GOLDEN / f"frame_{case}.npz") as z:
        return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def _config(case, **kw):
    """The stand-in's config with the scalars the fixture holds (asserted equal to the scenario's)."""
    z, st = _fixture(case), _state(case)
    cfg = FR.make_config(case, st, **kw)
    for k in z:
        if k.startswith("cfg_") and k != "cfg_check_ratio" and k[4:] not in kw:
            assert getattr(cfg, k[4:]) == z[k].item(), k
    assert FR.CHECK_RATIO[case] == z["cfg_check_ratio"].item()
    return cfg


def _oracle_map(case, cfg, device="cpu"):
    st, z = _state(case), _fixture(case)
    npm = sdf_cpu.NeuralPointMap(st, device=device)
    npm.local_valid_gs_mask = torch.as_tensor(st["local_valid_gs_mask"]).clone().to(device)
    npm.local_mask = torch.as_tensor(st["local_mask"]).clone().to(device)
    return FR.dress(npm, z["cert_global"], z["cert_local"], cfg)


def _cpu_mapper(case, cfg=None, **pool):
    cfg = cfg or _config(case)
    return FR.stand_in(_oracle_map(case, cfg), sdf_cpu.MLP.from_state(_state(case)), cfg, **pool)


def _mapper64(case, cfg=None):
    st, z = _state(case), _fixture(case)
    cfg = cfg or _config(case)
    return FR.stand_in(FR.map64(st, z["cert_global"], z["cert_local"], cfg), FR.dec64(st), cfg)


@functools.lru_cache(maxsize=None)
def _dyn_points(case):
    return FR.frame_points(_state(case), N_MAX, seed=11)


@functools.lru_cache(maxsize=None)
def _dyn_decisions(case, type_2_on):
    """float64 (mask, undecidable) of the N_MAX query points: computed once, sliced by the tests."""
    return FR.decisions(_mapper64(case), _dyn_points(case), type_2_on)


@functools.lru_cache(maxsize=None)
def _local_decisions(case):
    m = _mapper64(case)
    return FR.decisions(m, m.neural_points.local_neural_points.float(), False)


@functools.lru_cache(maxsize=None)
def _check_decisions(case, min_nn, threshold=FR.STABILITY_THRESHOLD):
    """float64 expectation of check_invalid_neural_points: (local_valid, valid, undecidable local rows, stable rows)."""
    cfg = _config(case, dynamic_sdf_ratio_thre=FR.CHECK_RATIO[case])
    m = _mapper64(case, cfg)
    npm = m.neural_points
    stable = npm.local_point_certainties > threshold
    lv, gv = npm.local_valid_gs_mask.clone(), npm.valid_gs_mask.clone()
    near = torch.zeros_like(stable)
    if stable.any():
        v, nr = FR.decisions(m, npm.local_neural_points[stable].float(), False, absolute=True, min_nn=min_nn)
        lv[stable], near[stable] = v, nr
    gv[npm.local_mask[:-1]] = lv
    return lv, gv, near, stable


def _local_rows(case):
    return torch.nonzero(torch.as_tensor(_state(case)["local_mask"])[:-1]).flatten()


def _single_cell_lookup(npm, coord):
    """(table entry, squared distance) of each sample's own cell: the oracle's search with the one-cell offsets."""
    keep = npm.neighbor_dx, npm.max_valid_dist2
    npm.neighbor_dx, npm.max_valid_dist2 = torch.zeros(1, 3, dtype=torch.int64), float("inf")
    d2, idx = npm.radius_neighborhood_search(coord)
    npm.neighbor_dx, npm.max_valid_dist2 = keep
    return idx[:, 0], d2[:, 0]


# ================================================================ CPU: the restatement against the fixtures
@pytest.mark.parametrize("case", FR.CASES)
def test_new_samples_restatement_reproduces_the_reference_fixture(case):
    z = _fixture(case)
    hist = int(z["new_history"])
    for frame_id in (0, 31):
        m = _cpu_mapper(case, **FR.pool_of(z["new_coord"], z["new_label"], hist))
        dx = m.neural_points.neighbor_dx.clone()
        FR.new_samples(m, frame_id)
        assert m.new_idx.dtype == torch.int64 and torch.equal(m.new_idx, z[f"o_new_idx_f{frame_id}"])
        assert m.new_obs_ratio == z[f"o_new_obs_ratio_f{frame_id}"].item()
        assert m.adaptive_iter_offset == z[f"o_adaptive_iter_offset_f{frame_id}"].item()
        assert torch.equal(m.neural_points.neighbor_dx, dx)
    assert z["o_adaptive_iter_offset_f0"].item() == 5 and z["o_adaptive_iter_offset_f31"].item() == 10
    assert int(z["o_new_idx_f0"].min()) >= hist
    k = z["o_new_idx_f0"].shape[0]
    assert 0.05 * FR.FIXTURE_ROWS < k < 0.95 * FR.FIXTURE_ROWS


@pytest.mark.parametrize("case", FR.CASES)
def test_new_sample_scenario_has_empty_cells_collisions_and_negative_coordinates(case):
    z = _fixture(case)
    npm = _oracle_map(case, _config(case))
    idx, d2 = _single_cell_lookup(npm, z["new_coord"])
    one_cell = 3 * ((1 + 1) * npm.resolution) ** 2
    assert (idx < 0).sum() > 100, "samples in cells without a point"
    hit = (idx >= 0) & (d2 > one_cell)
    assert hit.sum() > 100, "cells whose table slot holds a far point (hash collision)"
    assert (z["new_coord"][hit, 0] > 1e4).any() and (z["new_coord"][hit, 0] < -1e4).any()
    assert ((idx >= 0) & (d2 <= one_cell)).sum() > 1000
    assert (z["new_coord"] < 0).any(dim=0).all() and (z["new_coord"] > 0).any(dim=0).all()
    lab = z["new_label"].abs()
    thr = 3.0 * _config(case).surface_sample_range_m
    assert (lab < thr).float().mean() > 0.05 and (lab > thr).float().mean() > 0.05
    cert = z["cert_global"]
    assert (cert < 1.0).float().mean() > 0.2 and (cert > 1.0).float().mean() > 0.2


@pytest.mark.parametrize("case", FR.CASES)
def test_dynamic_filter_restatement_reproduces_the_reference_fixture(case):
    z = _fixture(case)
    m = _cpu_mapper(case)
    for on in (True, False):
        x = z["dyn_points"].clone()
        got = FR.dynamic_filter(m, x, on)
        assert x.requires_grad == on
        assert got.dtype == torch.bool and torch.equal(got, z[f"o_static_type2_{int(on)}"])
    assert torch.equal(FR.dynamic_filter_neural_points(m), z["o_static_neural_points"])


@pytest.mark.parametrize("case", FR.CASES)
def test_check_invalid_restatement_reproduces_the_reference_fixture(case):
    z = _fixture(case)
    for min_nn in FR.CHECK_MIN_NN:
        m = _cpu_mapper(case, _config(case, dynamic_sdf_ratio_thre=FR.CHECK_RATIO[case]))
        before = m.neural_points.local_valid_gs_mask.clone()
        FR.check_invalid_neural_points(m, FR.STABILITY_THRESHOLD, min_nn)
        assert torch.equal(m.neural_points.local_valid_gs_mask, z[f"o_local_valid_nn{min_nn}"])
        assert torch.equal(m.neural_points.valid_gs_mask, z[f"o_valid_nn{min_nn}"])
        assert not torch.equal(before, z[f"o_local_valid_nn{min_nn}"])
    assert not torch.equal(z["o_local_valid_nn6"], z["o_local_valid_nn14"]), "the neighbour count decides no row"


# ================================================================ CPU: the scenario meets its gates in float64
@pytest.mark.parametrize("case", FR.CASES)
@pytest.mark.parametrize("type_2_on", [True, False])
def test_dynamic_filter_scenario_is_decidable_in_float64(case, type_2_on):
    mask, near = _dyn_decisions(case, type_2_on)
    FR.check_gates(mask, near, f"{case} dynamic_filter type_2_on={type_2_on} (N = {N_MAX})")
    z = _fixture(case)                                  # and the fixture's own points, against the reference's fp32
    mask, near = FR.decisions(_mapper64(case), z["dyn_points"], type_2_on)
    FR.check_gates(mask, near, f"{case} dynamic_filter fixture type_2_on={type_2_on}")
    assert torch.equal(mask[~near], z[f"o_static_type2_{int(type_2_on)}"][~near])


@pytest.mark.parametrize("case", FR.CASES)
def test_dynamic_filter_neural_points_scenario_is_decidable_in_float64(case):
    mask, near = _local_decisions(case)
    FR.check_gates(mask, near, f"{case} dynamic_filter_neural_points")
    assert torch.equal(mask[~near], _fixture(case)["o_static_neural_points"][~near])


@pytest.mark.parametrize("case", FR.CASES)
@pytest.mark.parametrize("min_nn", FR.CHECK_MIN_NN)
def test_check_invalid_scenario_is_decidable_in_float64(case, min_nn):
    z = _fixture(case)
    lv, gv, near, stable = _check_decisions(case, min_nn)
    FR.check_gates(lv[stable], near[stable], f"{case} check_invalid_neural_points min_nn={min_nn}")
    assert 0 < stable.sum() < stable.numel() and stable.sum() % _config(case).infer_bs != 0
    assert torch.equal(lv[~near], z[f"o_local_valid_nn{min_nn}"][~near])
    rows = _local_rows(case)
    ok = torch.ones_like(gv)
    ok[rows[near]] = False
    assert torch.equal(gv[ok], z[f"o_valid_nn{min_nn}"][ok])


# ================================================================ CPU: entries, install, argument errors
def test_library_exports_the_frame_entries_and_rejects_bad_arguments():
    from pings_amd import _abi, _lib

    L = _lib.lib()
    assert set(FRAME_SYMBOLS) <= set(hdr.header_symbols()) and set(FRAME_SYMBOLS) <= set(_abi.SIGNATURES)
    assert all(hasattr(L, n) for n in FRAME_SYMBOLS)
    assert L.pings_abi_version() == 11
    count = ctypes.c_int64(-1)
    some = 64                                           # an address that is never dereferenced: no call below launches

    def knn(resolution=0.25, table=some, size=1000):
        return _abi.KnnMap(table, size, some, None, None, 0, 0, 0.0, None, None, 0, 0, None, None, 1, 1, resolution, 0.0,
                           None, 0, None, None, None, 0)

    new_count = L.pings_frame_new_count
    assert new_count(None, some, 10, some, some, 4, 0.75, 1.0, 0.75, some, ctypes.byref(count), None) == 1
    assert new_count(ctypes.byref(knn()), some, 10, some, some, 4, 0.75, 1.0, 0.75, some, None, None) == 1
    for bad in (knn(resolution=0.0), knn(resolution=-0.25), knn(table=None), knn(size=0)):
        assert new_count(ctypes.byref(bad), some, 10, some, some, 4, 0.75, 1.0, 0.75, some, ctypes.byref(count), None) == 1
    ok = knn()
    assert new_count(ctypes.byref(ok), some, 10, some, some, -1, 0.75, 1.0, 0.75, some, ctypes.byref(count), None) == 1
    assert new_count(ctypes.byref(ok), some, -1, some, some, 4, 0.75, 1.0, 0.75, some, ctypes.byref(count), None) == 1
    assert new_count(ctypes.byref(ok), some, 10, None, some, 4, 0.75, 1.0, 0.75, some, ctypes.byref(count), None) == 1
    assert new_count(ctypes.byref(ok), some, 10, some, None, 4, 0.75, 1.0, 0.75, some, ctypes.byref(count), None) == 1
    assert new_count(ctypes.byref(ok), some, 10, some, some, 4, 0.75, 1.0, 0.75, None, ctypes.byref(count), None) == 1
    assert new_count(ctypes.byref(ok), None, 10, some, some, 4, 0.75, 1.0, 0.75, some, ctypes.byref(count), None) == 1
    assert b"invalid argument" in L.pings_last_error()
    assert new_count(ctypes.byref(ok), some, 10, None, None, 0, 0.75, 1.0, 0.75, None, ctypes.byref(count), None) == 0
    assert count.value == 0                             # no row: no launch
    assert L.pings_frame_new_rows(None, 4, 0, some, 4, None) == 1
    assert L.pings_frame_new_rows(some, 4, 0, None, 4, None) == 1
    assert L.pings_frame_new_rows(some, -1, 0, some, 4, None) == 1
    assert L.pings_frame_new_rows(some, 4, 0, some, -1, None) == 1
    assert L.pings_frame_new_rows(None, 4, 0, None, 0, None) == 0
    assert L.pings_frame_static_mask(None, some, None, 4, 1.0, 0.2, 0.25, some, some, None) == 1
    assert L.pings_frame_static_mask(some, None, None, 4, 1.0, 0.2, 0.25, some, some, None) == 1
    assert L.pings_frame_static_mask(some, some, None, 4, 1.0, 0.2, 0.25, None, some, None) == 1
    assert L.pings_frame_static_mask(some, some, None, 4, 1.0, 0.2, 0.25, some, None, None) == 1
    assert L.pings_frame_static_mask(some, some, None, -1, 1.0, 0.2, 0.25, some, some, None) == 1
    scatter = L.pings_frame_valid_scatter
    assert scatter(None, 4, some, some, 0.2, 6, some, 8, 9, some, some, None) == 1
    assert scatter(some, 4, some, some, 0.2, 6, None, 8, 9, some, some, None) == 1
    assert scatter(some, 4, some, some, 0.2, 6, some, 8, 9, None, some, None) == 1
    assert scatter(some, 4, some, some, 0.2, 6, some, 8, 9, some, None, None) == 1
    assert scatter(some, -1, some, some, 0.2, 6, some, 8, 9, some, some, None) == 1
    assert scatter(some, 4, some, some, 0.2, 6, some, -8, 9, some, some, None) == 1
    assert scatter(None, 0, None, None, 0.2, 6, None, 8, 9, None, None, None) == 0
    # a bit per row and a few words per wave: no per-row array of indices or flags
    assert L.pings_frame_new_scratch_bytes(10_000_000) < 10_000_000 // 8 + 500_000
    assert L.pings_frame_new_scratch_bytes(0) > 0


def _stand_in_class():
    calls = []

    class Mapper:
        def dynamic_filter(self, points_torch, type_2_on=True):
            calls.append(("dynamic_filter", type_2_on))
            return "original dynamic_filter"

        def dynamic_filter_neural_points(self):
            calls.append(("dynamic_filter_neural_points",))
            return "original dynamic_filter_neural_points"

        def check_invalid_neural_points(self, stability_threshold=1.0, render_min_nn_count=6):
            calls.append(("check_invalid_neural_points", stability_threshold, render_min_nn_count))

    return Mapper, calls


NAMES = ("dynamic_filter", "dynamic_filter_neural_points", "check_invalid_neural_points")


def test_install_rebinds_and_uninstall_restores():
    from pings_amd import frame_ops

    Mapper, _ = _stand_in_class()
    orig = tuple(getattr(Mapper, n) for n in NAMES)
    frame_ops.install(Mapper)
    frame_ops.install(Mapper)                           # twice changes nothing
    assert all(getattr(Mapper, n) is getattr(frame_ops, n) for n in NAMES)
    assert tuple(getattr(Mapper, f"_pings_{n}_original") for n in NAMES) == orig
    frame_ops.uninstall(Mapper)
    assert tuple(getattr(Mapper, n) for n in NAMES) == orig
    assert not any(k.startswith("_pings_") for k in vars(Mapper))
    frame_ops.uninstall(Mapper)                         # nothing installed: nothing happens
    assert tuple(getattr(Mapper, n) for n in NAMES) == orig


def test_fallbacks_route_to_the_original_methods_and_never_to_torch():
    from pings_amd import frame_ops

    Mapper, calls = _stand_in_class()
    frame_ops.install(Mapper)
    try:
        m = Mapper()
        for k, v in vars(_cpu_mapper("pin_f8")).items():        # a CPU map: the kernels do not take it
            setattr(m, k, v)
        x = _fixture("pin_f8")["dyn_points"][:5].clone()
        assert m.dynamic_filter(x) == "original dynamic_filter"
        assert m.dynamic_filter(x.double(), False) == "original dynamic_filter"
        assert not x.requires_grad                              # the side effect belongs to whoever runs the query
        assert m.dynamic_filter_neural_points() == "original dynamic_filter_neural_points"
        m.check_invalid_neural_points(2.0, 3)
        assert calls == [("dynamic_filter", True), ("dynamic_filter", False), ("dynamic_filter_neural_points",),
                         ("check_invalid_neural_points", 2.0, 3)]
    finally:
        frame_ops.uninstall(Mapper)
    bare = _cpu_mapper("pin_f8")
    for call in (lambda: frame_ops.dynamic_filter(bare, x), lambda: frame_ops.dynamic_filter_neural_points(bare),
                 lambda: frame_ops.check_invalid_neural_points(bare)):
        with pytest.raises(RuntimeError, match="none was kept"):
            call()
    z = _fixture("pin_f8")
    pooled = _cpu_mapper("pin_f8", **FR.pool_of(z["new_coord"], z["new_label"], 10))
    with pytest.raises(RuntimeError, match="no torch path"):
        frame_ops.new_samples(pooled)


def test_new_samples_raises_zero_division_before_any_launch():
    from pings_amd import frame_ops

    m = NS(config=NS(bs_new_sample=2048), cur_sample_count=0)   # nothing else is touched before the division
    with pytest.raises(ZeroDivisionError):
        frame_ops.new_samples(m)
    m = NS(config=NS(bs_new_sample=0), cur_sample_count=0, new_idx="kept")
    frame_ops.new_samples(m)                                    # the block is off: nothing happens
    assert m.new_idx == "kept"


# ================================================================ GPU
DEV = "cuda"


class _Dec:
    """Duck-typed `Decoder` (model/decoder.py) from the fixture's state dict."""

    def __init__(self, st):
        t = lambda k: torch.as_tensor(st["dec." + k]).to(DEV)  # noqa: E731
        self.layers = [NS(weight=t("layers.0.weight"), bias=t("layers.0.bias"))]
        self.lout = NS(weight=t("lout.weight"), bias=t("lout.bias"))
        self.sdf_scale = float(st["sdf_scale"])
        self.use_leaky_relu = False


def _gpu_mapper(case, cfg=None, with_local_rows=True, warm=False, **pool):
    cfg = cfg or _config(case)
    npm = _oracle_map(case, cfg, device=DEV)
    npm.color_feature_dim = npm.color_features.shape[1] if npm.color_features is not None else 0
    if with_local_rows:                                          # what neural_map.reset_local_map leaves on the map
        npm._local_idx = torch.nonzero(npm.local_mask).flatten()
    pool = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in pool.items()}
    m = FR.stand_in(npm, _Dec(_state(case)), cfg, device=DEV, **pool)
    if warm:    # a map in use: its search index is built (the first query of a neighbourhood tensor reads its extent)
        from pings_amd import neural_points as hnp

        hnp.sdf_fused(npm, m.sdf_mlp, npm.local_neural_points[:1])
    return m


def _new_samples_both(case, coord, label, history, frame_id=0, **cfg_kw):
    from pings_amd import _lib, frame_ops

    cfg = _config(case, **cfg_kw)
    ref = _cpu_mapper(case, cfg, **FR.pool_of(coord, label, history))
    FR.new_samples(ref, frame_id)
    m = _gpu_mapper(case, cfg, **FR.pool_of(coord, label, history))
    npm = m.neural_points
    held = (npm.neighbor_dx, npm.max_valid_dist2, getattr(npm, "neighbor_K", None))
    torch.cuda.synchronize()
    _lib.sync_counts(reset=True)
    frame_ops.new_samples(m, frame_id)
    assert _lib.sync_counts(reset=True) == {"frame_new_samples": 1}
    assert npm.neighbor_dx is held[0] and npm.max_valid_dist2 == held[1] and getattr(npm, "neighbor_K", None) == held[2]
    assert m.new_idx.dtype == torch.int64 and m.new_idx.dim() == 1 and m.new_idx.is_cuda
    assert torch.equal(m.new_idx.cpu(), ref.new_idx), f"{case} n={coord.shape[0]}"
    assert m.new_obs_ratio == ref.new_obs_ratio and m.adaptive_iter_offset == ref.adaptive_iter_offset
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("case", FR.CASES)
def test_new_samples_kernel_matches_the_reference_fixture(case):
    z = _fixture(case)
    for frame_id in (0, 31):
        m = _new_samples_both(case, z["new_coord"], z["new_label"], int(z["new_history"]), frame_id)
        assert torch.equal(m.new_idx.cpu(), z[f"o_new_idx_f{frame_id}"])
        assert m.new_obs_ratio == z[f"o_new_obs_ratio_f{frame_id}"].item()
        assert m.adaptive_iter_offset == z[f"o_adaptive_iter_offset_f{frame_id}"].item()


@pytest.mark.gpu
@pytest.mark.parametrize("n", FR.SIZES)
def test_new_samples_kernel_equals_the_restatement(n):
    """Sample counts at the lane, wave and scan edges; samples in empty cells, behind hash collisions and at negative
    coordinates are part of every frame of the scenario (asserted on the CPU for the fixture's frame)."""
    for case in FR.CASES:
        coord, label = FR.frame_samples(_state(case), n, seed=100 + n)
        m = _new_samples_both(case, coord, label, FR.HISTORY if n % 2 else 0)
        if n >= FR.CHUNK:
            assert 0 < m.new_idx.shape[0] < n


@pytest.mark.gpu
@pytest.mark.parametrize("n", [FR.CHUNK + 1, N_MAX])
def test_new_samples_kernel_none_kept_and_all_kept(n):
    case = "gs_f32"
    coord, label = FR.frame_samples(_state(case), n, seed=7)
    m = _new_samples_both(case, coord, label, 11, new_certainty_thre=-1.0)          # no certainty is below -1
    assert m.new_idx.shape == (0,) and m.new_obs_ratio == 0.0 and m.adaptive_iter_offset == -5
    m = _new_samples_both(case, coord, torch.zeros_like(label), 11, frame_id=31, new_certainty_thre=10.0)
    assert torch.equal(m.new_idx.cpu(), torch.arange(n) + 11) and m.adaptive_iter_offset == 10
    # every sample far from the map: no point within the one-cell distance, all kept by their certainty of 0
    m = _new_samples_both(case, coord + 50.0, torch.zeros_like(label), 0)
    assert m.new_idx.shape == (n,)


@functools.lru_cache(maxsize=None)
def _dyn_gpu(case):
    return _gpu_mapper(case, warm=True), _dyn_points(case).to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("n", FR.SIZES)
@pytest.mark.parametrize("type_2_on", [True, False])
def test_dynamic_filter_kernel_agrees_with_float64_on_every_decidable_row(n, type_2_on):
    from pings_amd import _lib, frame_ops

    for case in FR.CASES:
        ref, near = (t[:n] for t in _dyn_decisions(case, type_2_on))
        m, x_all = _dyn_gpu(case)
        x = x_all[:n].clone()
        torch.cuda.synchronize()
        _lib.sync_counts(reset=True)
        got = frame_ops.dynamic_filter(m, x, type_2_on)
        count = frame_ops.last_dynamic_count()
        assert _lib.sync_counts(reset=True) == {}, "a host read inside dynamic_filter"
        assert x.requires_grad == type_2_on
        assert got.dtype == torch.bool and got.shape == (n,) and got.is_cuda
        assert count.dim() == 0 and count.is_cuda and int(count) == int((~got).sum())
        bad = (got.cpu() != ref) & ~near
        print(f"{case} n={n} type_2_on={type_2_on}: undecidable {int(near.sum())}, differing decidable rows {int(bad.sum())}")
        assert not bad.any()
    if n == N_MAX:
        assert torch.equal(frame_ops.dynamic_filter(m, x_all.clone(), type_2_on), got), "not reproducible"


@pytest.mark.gpu
@pytest.mark.parametrize("case", FR.CASES)
def test_dynamic_filter_kernel_matches_the_reference_fixture_on_decidable_rows(case):
    from pings_amd import frame_ops

    z = _fixture(case)
    m = _gpu_mapper(case)
    for on in (True, False):
        _, near = FR.decisions(_mapper64(case), z["dyn_points"], on)
        got = frame_ops.dynamic_filter(m, z["dyn_points"].to(DEV), on).cpu()
        assert torch.equal(got[~near], z[f"o_static_type2_{int(on)}"][~near])


@pytest.mark.gpu
@pytest.mark.parametrize("case", FR.CASES)
def test_dynamic_filter_neural_points_kernel_agrees_with_float64(case):
    from pings_amd import _lib, frame_ops

    ref, near = _local_decisions(case)
    m = _gpu_mapper(case, warm=True)
    torch.cuda.synchronize()
    _lib.sync_counts(reset=True)
    got = frame_ops.dynamic_filter_neural_points(m)
    count = frame_ops.last_dynamic_count()
    assert _lib.sync_counts(reset=True) == {}
    assert got.dtype == torch.bool and got.shape == ref.shape and int(count) == int((~got).sum())
    assert not m.neural_points.local_neural_points.requires_grad
    assert torch.equal(got.cpu()[~near], ref[~near])
    assert torch.equal(got.cpu()[~near], _fixture(case)["o_static_neural_points"][~near])


def _valid_query(npm, x, locally):
    from pings_amd import neural_points as hnp

    with torch.no_grad():
        geo, _, w, cnt, _ = hnp.query_feature(npm, x, accumulate_stability=False, query_locally=locally,
                                              use_only_valid_points=True)
    return geo, w, cnt


@pytest.mark.gpu
@pytest.mark.parametrize("case", FR.CASES)
@pytest.mark.parametrize("min_nn", FR.CHECK_MIN_NN)
def test_check_invalid_kernel_agrees_with_float64_and_the_next_query_sees_the_mask(case, min_nn):
    from pings_amd import _lib, frame_ops

    cfg = _config(case, dynamic_sdf_ratio_thre=FR.CHECK_RATIO[case])
    lv_ref, gv_ref, near, stable = _check_decisions(case, min_nn)
    assert stable.sum() % cfg.infer_bs != 0 and (case != "gs_f32" or stable.sum() > 3 * cfg.infer_bs)   # ragged chunks
    m = _gpu_mapper(case, cfg)
    npm = m.neural_points
    lv0, gv0 = npm.local_valid_gs_mask.clone(), npm.valid_gs_mask.clone()
    x = _fixture(case)["dyn_points"][:2000].to(DEV)
    before = [_valid_query(npm, x, loc) for loc in (True, False)]   # the search index now holds the old mask
    torch.cuda.synchronize()
    _lib.sync_counts(reset=True)
    frame_ops.check_invalid_neural_points(m, FR.STABILITY_THRESHOLD, min_nn)
    assert _lib.sync_counts(reset=True) == {"mask_rows_count": 1}
    lv, gv = npm.local_valid_gs_mask.cpu(), npm.valid_gs_mask.cpu()
    assert lv.dtype == torch.bool and gv.dtype == torch.bool
    assert torch.equal(lv[~stable].view(torch.uint8), lv0.cpu()[~stable].view(torch.uint8)), "an unstable row changed"
    assert torch.equal(lv[~near], lv_ref[~near])
    rows = _local_rows(case)
    ok = torch.ones_like(gv)
    ok[rows[near]] = False
    assert torch.equal(gv[ok], gv_ref[ok])
    outside = torch.ones_like(gv)
    outside[rows[stable]] = False
    assert torch.equal(gv[outside].view(torch.uint8), gv0.cpu()[outside].view(torch.uint8))
    assert torch.equal(gv[rows], lv), "the global mask does not mirror the local one"
    assert not torch.equal(lv, lv0.cpu())
    # the generation bump: a query through the cached search index equals one on a map built from scratch
    fresh = _gpu_mapper(case, cfg).neural_points
    fresh.local_valid_gs_mask, fresh.valid_gs_mask = lv.to(DEV), gv.to(DEV)
    changed = False
    for loc, old in zip((True, False), before):
        now, want = _valid_query(npm, x, loc), _valid_query(fresh, x, loc)
        for a, b in zip(now, want):
            assert torch.equal(a, b), f"query_locally={loc}: the query does not see the new mask"
        changed |= not torch.equal(now[2], old[2])
    assert changed, "the new mask changes no neighbour count: the query proves nothing"


@pytest.mark.gpu
def test_check_invalid_kernel_without_stable_rows_and_without_the_row_list():
    from pings_amd import _lib, frame_ops

    case = "pin_f8"
    cfg = _config(case, dynamic_sdf_ratio_thre=FR.CHECK_RATIO[case], infer_bs=100)
    m = _gpu_mapper(case, cfg, with_local_rows=False, warm=True)
    npm = m.neural_points
    lv0, gv0 = npm.local_valid_gs_mask.clone(), npm.valid_gs_mask.clone()
    gen = getattr(npm, "_pings_table_gen", 0)
    _lib.sync_counts(reset=True)
    frame_ops.check_invalid_neural_points(m, 100.0)             # no certainty is above 100
    assert _lib.sync_counts(reset=True) == {"mask_rows_count": 1}
    assert torch.equal(npm.local_valid_gs_mask, lv0) and torch.equal(npm.valid_gs_mask, gv0)
    assert getattr(npm, "_pings_table_gen", 0) == gen
    # the row list rebuilt from local_mask (one more read), five chunks of 100 rows
    lv_ref, gv_ref, near, stable = _check_decisions(case, 6)
    assert 400 < stable.sum() < 500
    frame_ops.check_invalid_neural_points(m)
    assert _lib.sync_counts(reset=True) == {"mask_rows_count": 1, "frame_local_rows": 1}
    assert getattr(npm, "_pings_table_gen", 0) == gen + 1
    assert torch.equal(npm.local_valid_gs_mask.cpu()[~near], lv_ref[~near])
    ok = torch.ones_like(gv_ref)
    ok[_local_rows(case)[near]] = False
    assert torch.equal(npm.valid_gs_mask.cpu()[ok], gv_ref[ok])
