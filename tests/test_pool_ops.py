"""The SDF training-sample pool (pings_amd/pool_ops.py, csrc/pool.hip) against the reference.

Yardsticks: tests/pool_ref.py (a torch restatement that takes the random draws as arguments) and
tests/golden/pool_*.npz (inputs, draws and outputs of the reference's own functions, tools/make_pool_golden.py).

Gates, with u = 2^-24 and dist = |point|:
  sampler   copies (normal, label, colour) exact;  |d sdf_label| <= 8u (dist + |ref|);
            |d coord|_inf <= 8u (dist + |ref|_inf);  |d weight| <= 8u (1 + dist / (0.8 free_sample_end_dist_m)), the
            dist term only with the drop-off on.  8: at most seven fp32 roundings of quantities <= 1 before the
            multiplication by dist and one after; (ratio - 1) * dist cancels, so a gate relative to the tensor's
            maximum does not hold.  The library and the fixtures are the same fp32 operations, so the library is held
            to the same bound against the fixtures.
  get_batch every output torch.equal.
  transform |d_i| <= 4u (sum_j |R_ij| |p_j| + |t_i|): three products and three sums.
  window    points with |d - radius| <= 1e-6 radius (more than 5x the 3u error of a reordered fp32 norm) are removed
            from the INPUT (at most 0.1 % of it); the row list is then torch.equal.
"""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import abi_header as hdr
import pool_ref as PR
from conftest import GOLDEN

U = PR.U
POOL_SYMBOLS = ["pings_pool_sample", "pings_pool_draw", "pings_pool_ts_range", "pings_pool_transform",
                "pings_pool_window_scratch_bytes", "pings_pool_window_count", "pings_pool_window"]


def _npz(name):
    with np.load(GOLDEN / f"{name}.npz") as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


def _same_special(a, b, what):
    """NaN at the same places, infinities at the same places with the same sign; returns the finite mask."""
    assert torch.equal(torch.isnan(a), torch.isnan(b)), f"{what}: NaN positions differ"
    inf = torch.isinf(b)
    assert torch.equal(torch.isinf(a), inf), f"{what}: inf positions differ"
    assert torch.equal(torch.sign(a[inf]).double(), torch.sign(b[inf]).double()), f"{what}: inf signs differ"
    return torch.isfinite(b)


def _check_sample(cfg, pts, got, ref, what):
    """The sampler gates of the module docstring; `ref` in float64 or float32, `got` float32."""
    S = cfg.surface_sample_n + cfg.free_front_n + cfg.free_behind_n + 1
    dist = torch.linalg.norm(pts.double(), dim=1).repeat_interleave(S)
    coord, label, normal, sem, color, weight = got
    r_coord, r_label, r_normal, r_sem, r_color, r_weight = ref
    assert coord.dtype == label.dtype == weight.dtype == torch.float32
    assert coord.shape == (pts.shape[0] * S, 3) and label.shape == weight.shape == (pts.shape[0] * S,)
    for g, r, name in ((normal, r_normal, "normal"), (sem, r_sem, "sem"), (color, r_color, "color")):
        assert (g is None) == (r is None), name
        if g is not None:
            assert g.dtype == r.dtype and torch.equal(g, r), f"{what}: {name} is not an exact copy"
    if sem is not None:
        assert sem.dtype == torch.int32
    worst = []
    ok = _same_special(label, r_label, what + " sdf_label")
    e = ((label.double() - r_label.double()).abs() / (8 * U * (dist + r_label.double().abs())).clamp_min(1e-300))[ok]
    worst.append(float(e.max()) if e.numel() else 0.0)
    ok = _same_special(coord, r_coord, what + " coord").all(dim=1)
    rc = r_coord.double()[ok]
    e = (coord.double()[ok] - rc).abs().amax(dim=1) / (8 * U * (dist[ok] + rc.abs().amax(dim=1))).clamp_min(1e-300)
    worst.append(float(e.max()) if e.numel() else 0.0)
    ok = _same_special(weight, r_weight, what + " weight")
    bound = 8 * U * (1 + (dist / (0.8 * cfg.free_sample_end_dist_m) if cfg.behind_dropoff_on else 0 * dist))
    e = ((weight.double() - r_weight.double()).abs() / bound)[ok]
    worst.append(float(e.max()) if e.numel() else 0.0)
    print(f"{what}: worst error / gate  sdf_label {worst[0]:.3f}  coord {worst[1]:.3f}  weight {worst[2]:.3f}")
    assert max(worst) <= 1.0, f"{what}: error / gate (sdf_label, coord, weight) = {worst}"


def _sample_case(name):
    P, (ns, nf, nb), dw, drop, ch, normals, labels, origin = PR.GOLDEN_SAMPLE[name]
    z = _npz(f"pool_sample_{name}")
    cfg = PR.sample_cfg(ns, nf, nb, dw, drop)
    inputs = tuple(z.get(k) for k in ("points", "normal", "sem", "color"))
    noise = tuple(z[k] for k in ("noise_surface", "noise_front", "noise_behind"))
    outs = tuple(z.get(k) for k in ("o_coord", "o_sdf_label", "o_normal", "o_sem", "o_color", "o_weight"))
    return cfg, inputs, noise, outs


def _batch_case(name, device="cpu"):
    m = PR.batch_state(*PR.GOLDEN_BATCH[name], seed=len(name), device=device)
    z = _npz(f"pool_batch_{name}")
    outs = tuple(z.get(k) for k in ("o_coord", "o_sdf_label", "o_ts", "o_normal", "o_sem", "o_color", "o_weight"))
    return m, z["r_hist"], z.get("r_new"), outs


def _equal_tuple(got, ref, what):
    for i, (g, r) in enumerate(zip(got, ref)):
        assert (g is None) == (r is None), f"{what}[{i}]"
        if g is not None:
            assert g.dtype == r.dtype and g.shape == r.shape and torch.equal(g.cpu(), r.cpu()), f"{what}[{i}]"


def _transform_bound(pts, ts, pose):
    tr = pose[ts.long()].to(torch.float32).double()
    return 4 * U * ((tr[:, :3, :3].abs() @ pts.double().abs().unsqueeze(-1)).squeeze(-1) + tr[:, :3, 3].abs())


# ================================================================ CPU: restatement against the fixtures
@pytest.mark.parametrize("name", list(PR.GOLDEN_SAMPLE))
def test_sample_restatement_matches_the_reference_fixture(name):
    cfg, (pts, nrm, sem, col), noise, outs = _sample_case(name)
    assert outs[1].shape[0] == pts.shape[0] * (cfg.surface_sample_n + cfg.free_front_n + cfg.free_behind_n + 1)
    _check_sample(cfg, pts, PR.sample(cfg, pts, nrm, sem, col, noise), outs, f"restatement fp32 {name}")
    # and the reference's own fp32 against the float64 restatement, under the same gates
    _check_sample(cfg, pts, outs, PR.sample(cfg, pts, nrm, sem, col, noise, torch.float64), f"fixture vs fp64 {name}")


def test_sample_fixture_has_an_origin_point_with_non_finite_rows():
    cfg, (pts, *_), _, outs = _sample_case("p63_320_origin")
    assert (pts.abs().sum(dim=1) == 0).sum() == 1
    assert torch.isnan(outs[0]).any() and torch.isnan(outs[5]).any()


@pytest.mark.parametrize("name", list(PR.GOLDEN_BATCH))
def test_get_batch_restatement_matches_the_reference_fixture(name):
    m, r_hist, r_new, outs = _batch_case(name)
    sizes = PR.draw_sizes(m)
    assert r_hist.shape[0] == sizes[0][0] and (r_new is None) == (sizes[1] is None)
    assert int(r_hist.max()) < sizes[0][1]
    _equal_tuple(PR.get_batch(m, r_hist, r_new), outs, name)


@pytest.mark.parametrize("name", list(PR.GOLDEN_TRANSFORM))
def test_transform_restatement_matches_the_reference_fixture(name):
    z = _npz(f"pool_transform_{name}")
    assert (z["ts"] < 0).any() and z["pose"].dtype == getattr(torch, PR.GOLDEN_TRANSFORM[name][1])
    got = PR.transform(z["points"], z["ts"], z["pose"])
    bound = _transform_bound(z["points"], z["ts"], z["pose"])
    assert ((got.double() - z["o_points"].double()).abs() <= bound).all()
    ref64 = PR.transform(z["points"], z["ts"], z["pose"], torch.float64)
    assert ((z["o_points"].double() - ref64).abs() <= bound).all()


# ================================================================ CPU: install / uninstall and the fallbacks
def _stand_ins():
    calls = []

    class Sampler:
        def __init__(self):
            self.config, self.dev = PR.sample_cfg(3, 2, 1, True, True), "cpu"

        def sample(self, points_torch, normal_torch, sem_label_torch, color_torch, color_valid_mask=None):
            calls.append(("sample", color_valid_mask is not None))
            return "original sample"

    class Mapper:
        def get_batch(self, global_coord=True):
            calls.append(("get_batch", global_coord))
            return "original get_batch"

        def transform_data_pool(self, pose_diff_torch):
            calls.append(("transform_data_pool", tuple(pose_diff_torch.shape)))

    return Sampler, Mapper, calls


def test_install_rebinds_and_uninstall_restores():
    from pings_amd import pool_ops

    Sampler, Mapper, _ = _stand_ins()
    orig = (Sampler.sample, Mapper.get_batch, Mapper.transform_data_pool)
    pool_ops.install(Sampler, Mapper)
    pool_ops.install(Sampler, Mapper)                   # twice changes nothing
    assert Sampler.sample is pool_ops.sample and Mapper.get_batch is pool_ops.get_batch
    assert Mapper.transform_data_pool is pool_ops.transform_data_pool
    assert (Sampler._pings_sample_original, Mapper._pings_get_batch_original,
            Mapper._pings_transform_data_pool_original) == orig
    pool_ops.uninstall(Sampler, Mapper)
    assert (Sampler.sample, Mapper.get_batch, Mapper.transform_data_pool) == orig
    assert not any(k.startswith("_pings_") for k in list(vars(Sampler)) + list(vars(Mapper)))
    pool_ops.uninstall(Sampler, Mapper)                 # nothing installed: nothing happens
    assert (Sampler.sample, Mapper.get_batch, Mapper.transform_data_pool) == orig


def test_fallbacks_route_to_the_original_methods():
    from pings_amd import pool_ops

    Sampler, Mapper, calls = _stand_ins()
    pool_ops.install(Sampler, Mapper)
    try:
        s = Sampler()
        pts = torch.rand(5, 3) + 1.0
        mask = torch.ones(5, dtype=torch.bool)
        assert s.sample(pts, None, None, torch.rand(5, 3), mask) == "original sample"   # color_valid_mask
        assert s.sample(pts, None, None, None) == "original sample"                       # CPU tensors
        assert s.sample(pts.double(), None, None, None) == "original sample"              # non-fp32 points
        assert s.sample(pts[:0], None, None, None) == "original sample"                   # P == 0
        assert calls == [("sample", True)] + [("sample", False)] * 3
        del calls[:]
        m = Mapper()
        for k, v in vars(PR.batch_state(16, 4, True, 8, False, True, True, True, seed=3)).items():
            setattr(m, k, v)
        assert m.get_batch() == "original get_batch"                                      # a CPU pool
        m.transform_data_pool(torch.eye(4).repeat(PR.POSES, 1, 1))                        # a CPU pool
        assert calls == [("get_batch", True), ("transform_data_pool", (PR.POSES, 4, 4))]
    finally:
        pool_ops.uninstall(Sampler, Mapper)
    with pytest.raises(RuntimeError, match="none was kept"):                              # never a silent torch path
        pool_ops.sample(NS(config=PR.sample_cfg(1, 1, 1, True, True)), torch.rand(5, 3), None, None, None)


def test_window_rows_is_one_dimensional_for_a_single_row_on_the_cpu_path():
    from pings_amd import pool_ops

    pool = torch.tensor([[0.0, 0.0, 0.0], [5.0, 0.0, 0.0], [0.0, 0.0, 9.0]])
    rows = pool_ops.window_rows(pool, torch.zeros(3), 1.0, False)
    assert rows.dtype == torch.int64 and rows.shape == (1,) and rows.tolist() == [0]
    assert pool_ops.window_rows(pool, torch.zeros(3), 1.0, True).tolist() == [0, 2]
    assert pool_ops.window_rows(pool + 100.0, torch.zeros(3), 1.0, True).shape == (0,)


def test_library_exports_the_pool_entries_and_rejects_null_pointers():
    from pings_amd import _abi, _lib

    L = _lib.lib()
    assert set(POOL_SYMBOLS) <= set(hdr.header_symbols()) and set(POOL_SYMBOLS) <= set(_abi.SIGNATURES)
    assert all(hasattr(L, n) for n in POOL_SYMBOLS)
    assert L.pings_abi_version() == 11
    assert L.pings_pool_sample(None, None) == 1
    a = _abi.PoolSampleArgs(P=4, surface_sample_n=1)
    assert L.pings_pool_sample(ctypes.byref(a), None) == 1
    assert L.pings_pool_draw(None, 1, None, 4, None, 0, None, 0, None, 0, 10, None, None) == 1
    jobs = (_abi.GatherJob * 1)(_abi.GatherJob(None, None, 4, 4))
    assert L.pings_pool_draw(jobs, 1, None, 4, None, 0, None, 0, None, 0, 10, None, None) == 1
    assert L.pings_pool_ts_range(None, 0, 4, None, None) == 1
    assert L.pings_pool_transform(4, None, None, 0, None, 0, 2, None, None) == 1
    count = ctypes.c_int64(-1)
    assert L.pings_pool_window_count(None, 4, None, 1.0, 0, None, ctypes.byref(count), None) == 1
    assert L.pings_pool_window(None, 4, None, 1.0, 0, None, None, 4, None) == 1
    assert L.pings_pool_window_scratch_bytes(10_000_000) < 100_000     # a few words per 2048 rows, no per-row array


# ================================================================ GPU
DEV = "cuda"


class _Sampler:
    def __init__(self, cfg):
        from pings_amd import pool_ops

        self.config, self.dev = cfg, torch.device(DEV)
        self._fn = pool_ops.sample

    def sample(self, *a, **k):
        return self._fn(self, *a, **k)


def _to(ts, dev=DEV):
    return tuple(None if t is None else t.to(dev) for t in ts)


def _cpu(ts):
    return tuple(None if t is None else t.cpu() for t in ts)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PR.GOLDEN_SAMPLE))
def test_sample_kernel_matches_the_reference_fixture(name):
    cfg, inputs, noise, outs = _sample_case(name)
    got = _cpu(_Sampler(cfg).sample(*_to(inputs), _noise=_to(noise)))
    _check_sample(cfg, inputs[0], got, outs, f"kernel vs fixture {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("sections", [(3, 2, 0), (3, 2, 1), (0, 0, 0), (0, 1, 2), (4, 0, 3)])
def test_sample_kernel_against_float64(sections):
    """P at the block edges (P*S = 255, 256, 257 among them), every weight switch, colour None / 1 / 3 / 4 channels,
    normals and labels on and off, one point at the origin where P > 1."""
    ns, nf, nb = sections
    n = 0
    for P in (1, 63, 64, 65, 257):
        for dw in (False, True):
            for drop in (False, True):
                ch = (None, 1, 3, 4)[n % 4]
                normals, labels = bool((n // 4) % 2), bool((n // 2) % 2)
                n += 1
                cfg = PR.sample_cfg(ns, nf, nb, dw, drop)
                inputs = PR.sample_inputs(P, ch, normals, labels, P > 1, seed=1000 * P + n)
                g = torch.Generator().manual_seed(n)
                noise = (torch.randn(P * ns, 1, generator=g), torch.rand(P * nf, 1, generator=g),
                         torch.rand(P * nb, 1, generator=g))
                if labels and n % 3 == 0:
                    inputs = inputs[:2] + (inputs[2].long(),) + inputs[3:]
                d_in, d_noise = _to(inputs), _to(noise)
                got = _cpu(_Sampler(cfg).sample(*d_in, _noise=d_noise))
                ref = _cpu(PR.sample(cfg, *d_in, d_noise, torch.float64))
                _check_sample(cfg, inputs[0], got, ref, f"P={P} {sections} dw={dw} drop={drop} C={ch}")
                if P > 1:
                    assert torch.isnan(got[0]).any() or (ns == 0 and nf == 0 and nb == 0)


@pytest.mark.gpu
def test_sample_draws_are_the_references_and_leave_the_generator_where_it_does():
    for (ns, nf, nb) in ((3, 2, 1), (0, 2, 0), (0, 0, 0)):
        P = 257
        cfg = PR.sample_cfg(ns, nf, nb, True, True)
        inputs = _to(PR.sample_inputs(P, 3, True, True, False, seed=5))
        s = _Sampler(cfg)
        torch.manual_seed(1234)
        got = s.sample(*inputs)
        state = torch.cuda.get_rng_state()
        torch.manual_seed(1234)
        noise = (torch.randn(P * ns, 1, device=DEV), torch.rand(P * nf, 1, device=DEV),
                 torch.rand(P * nb, 1, device=DEV))
        assert torch.equal(state, torch.cuda.get_rng_state())
        _equal_tuple(got, s.sample(*inputs, _noise=noise), f"sample {ns, nf, nb}")


def _mapper(m):
    from pings_amd import pool_ops

    m.get_batch = lambda *a, **k: pool_ops.get_batch(m, *a, **k)
    m.transform_data_pool = lambda pose: pool_ops.transform_data_pool(m, pose)
    return m


def _hand_draws(m):
    (nh, hh), new = PR.draw_sizes(m)
    r_hist = torch.randint(0, hh, (nh,), device=DEV)
    return r_hist, (None if new is None else torch.randint(0, new[1], (new[0],), device=DEV))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PR.GOLDEN_BATCH))
def test_get_batch_kernel_matches_the_reference_fixture(name):
    from pings_amd import pool_ops

    m, r_hist, r_new, outs = _batch_case(name, DEV)
    got = _mapper(m).get_batch(_draws=(r_hist.to(DEV), None if r_new is None else r_new.to(DEV)))
    _equal_tuple(got, outs, name)
    assert pool_ops.last_status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("bs", [1, 255, 256, 257, 1024])
def test_get_batch_kernel_equals_the_restatement(bs):
    from pings_amd import pool_ops

    n = 0
    for bs_new in (0, 1, bs - 1):
        for local in (False, True):
            color, normals, labels = bool(n % 2), bool((n // 2) % 2), bool((n // 3) % 2)
            n += 1
            m = _mapper(PR.batch_state(bs, bs_new, local, None, False, color, normals, labels, seed=bs + n, device=DEV))
            m.new_idx = torch.randint(0, PR.POOL_ROWS, (1100,), device=DEV)
            torch.manual_seed(bs + n)
            got = m.get_batch()
            state = torch.cuda.get_rng_state()
            torch.manual_seed(bs + n)
            draws = _hand_draws(m)
            assert torch.equal(state, torch.cuda.get_rng_state()), "the randint calls are not the reference's"
            assert (draws[1] is None) == (bs_new == 0) and got[0].shape == (bs, 3)
            _equal_tuple(got, PR.get_batch(m, *draws), f"bs={bs} bs_new={bs_new} local={local}")
            _equal_tuple(got, m.get_batch(_draws=draws), "library with the hand-drawn indices")
    assert pool_ops.last_status() == 0


@pytest.mark.gpu
def test_get_batch_kernel_keeps_the_reference_branches():
    """`lose_track` / `stop_status` switch the new-sample part off; an empty `new_idx` draws from `pool_sample_count`
    rows and ignores `local_sample_indices`."""
    for lose, stop, empty in ((True, False, False), (False, True, False), (False, False, True)):
        m = _mapper(PR.batch_state(257, 31, True, 0 if empty else 40, lose, True, True, True, seed=9, device=DEV))
        m.dataset.stop_status = stop
        if empty:
            m.pool_sample_count = 700       # the branch reads the attribute, not the local list
        torch.manual_seed(77)
        got = m.get_batch()
        torch.manual_seed(77)
        r = torch.randint(0, 700 if empty else m.local_sample_indices.shape[0], (257,), device=DEV)
        _equal_tuple(got, PR.get_batch(m, r), f"lose={lose} stop={stop} empty={empty}")
        if empty:
            assert torch.equal(got[0], m.global_coord_pool[r])


@pytest.mark.gpu
def test_get_batch_kernel_flags_a_stale_index_and_zero_fills_that_row():
    from pings_amd import pool_ops

    m = _mapper(PR.batch_state(256, 16, True, 40, False, True, True, True, seed=4, device=DEV))
    assert pool_ops.last_status() == 0
    draws = (torch.randint(0, m.local_sample_indices.shape[0], (240,), device=DEV),
             torch.randint(0, 40, (16,), device=DEV))
    ref = PR.get_batch(m, *draws)
    stale = int(draws[0][100])
    m.local_sample_indices = m.local_sample_indices.clone()
    m.local_sample_indices[stale] = PR.POOL_ROWS        # one past the last row
    got = m.get_batch(_draws=draws)
    assert pool_ops.last_status() == 1 and pool_ops.last_status() == 0      # read and cleared
    hit = torch.zeros(256, dtype=torch.bool, device=DEV)
    hit[:240] = draws[0] == stale
    assert hit[100] and hit.sum() >= 1
    for g, r in zip(got, ref):
        assert torch.equal(g[~hit], r[~hit]) and not g[hit].any()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 255, 256, 257, 200_000])
def test_transform_kernel_against_float64(N):
    for pdt in (torch.float32, torch.float64):
        for tdt in (torch.int32, torch.int64):
            m = _mapper(PR.pool_state(N, False, False, False, seed=N, device=DEV))
            ts = m.time_pool.long() - PR.POSES * (torch.arange(N, device=DEV) % 3 == 0)     # negative wraps
            m.time_pool = ts.to(tdt)
            pose = PR.rigid_poses(PR.POSES, pdt, seed=N + 1).to(DEV)
            before = m.global_coord_pool.clone()
            ref = PR.transform(before, m.time_pool, pose, torch.float64)
            storage = m.global_coord_pool.data_ptr()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            m.transform_data_pool(pose)
            rise = torch.cuda.max_memory_allocated() - base
            assert m.global_coord_pool.data_ptr() == storage, "not in place"
            err = (m.global_coord_pool.double() - ref).abs()
            bound = _transform_bound(before, m.time_pool, pose)
            print(f"N={N} {pdt} {tdt}: worst error / gate {float((err / bound).max()):.3f}, memory rise {rise} B")
            assert (err <= bound).all()
            assert rise < 1 << 20, f"{rise} bytes allocated across the call"


@pytest.mark.gpu
def test_transform_kernel_matches_the_reference_fixture():
    for name in PR.GOLDEN_TRANSFORM:
        z = _npz(f"pool_transform_{name}")
        m = _mapper(NS(global_coord_pool=z["points"].to(DEV), time_pool=z["ts"].to(DEV)))
        m.transform_data_pool(z["pose"].to(DEV))
        bound = _transform_bound(z["points"], z["ts"], z["pose"])
        assert ((m.global_coord_pool.cpu().double() - z["o_points"].double()).abs() <= bound).all()


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [PR.POSES, -PR.POSES - 1])
def test_transform_raises_before_any_row_moves(bad):
    m = _mapper(PR.pool_state(257, False, False, False, seed=2, device=DEV))
    m.time_pool[200] = bad
    before = m.global_coord_pool.clone()
    with pytest.raises(IndexError):
        m.transform_data_pool(PR.rigid_poses(PR.POSES, torch.float64, seed=3).to(DEV))
    assert torch.equal(m.global_coord_pool.view(torch.int32), before.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 255, 256, 257, 4097, 100_000])
def test_window_rows_equal_the_restatement(N):
    from pings_amd import pool_ops

    radius = 60.0
    for two_d in (False, True):
        for far in (0.0, 1000.0):
            g = torch.Generator().manual_seed(N + int(far) + two_d)
            origin = torch.full((3,), far) + (torch.rand(3, generator=g) if far else 0.0)
            pool = (origin + (torch.rand(N, 3, generator=g) - 0.5) * 2.4 * radius).float()
            d = PR.window_dist(pool, origin, two_d)
            keep = (d - radius).abs() > 1e-6 * radius
            assert (~keep).sum() <= 1e-3 * N, "too many points at the window's edge"
            pool = pool[keep].contiguous().to(DEV)
            ref = PR.window(pool, origin.to(DEV), radius, two_d)
            got = pool_ops.window_rows(pool, origin.to(DEV), radius, two_d)
            assert got.dtype == torch.int64 and got.dim() == 1 and torch.equal(got, ref)
            assert N < 4097 or 0 < got.shape[0] < pool.shape[0]
    origin = torch.tensor([3.0, -2.0, 1.0])
    g = torch.Generator().manual_seed(N)
    inside = (origin + (torch.rand(N, 3, generator=g) - 0.5) * 0.5 * radius).to(DEV)
    assert torch.equal(pool_ops.window_rows(inside, origin.to(DEV), radius, False), torch.arange(N, device=DEV))
    outside = pool_ops.window_rows(inside + 10 * radius, origin.to(DEV), radius, True)
    assert outside.shape == (0,) and outside.dtype == torch.int64
