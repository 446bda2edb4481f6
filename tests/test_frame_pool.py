"""The pool part of `Mapper.process_frame` (pings_amd/pool_ops.py, csrc/pool_frame.hip) against the reference.

Yardsticks: tests/frame_pool_ref.py (a torch restatement that takes the capacity filter's draw as an argument) and
tests/golden/frame_pool_*.npz (inputs, draws, `update` arguments and the pool after every frame of the reference's own
`Mapper.process_frame`, tools/make_frame_pool_golden.py).

Gates, with u = 2^-24: copies, integers, row order and counters exact; a transformed coordinate within
4u (sum_j |R_ij| |p_j| + |t_i|) (three products and three sums; no |t_i| for a rotated normal), the gate of the
transform test of tests/test_pool_ops.py.
"""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import abi_header as hdr
import frame_pool_ref as FR
import pool_ref as PR
from conftest import GOLDEN

FRAME_SYMBOLS = ["pings_pool_append", "pings_pool_discard_mark", "pings_pool_compact_scratch_bytes",
                 "pings_pool_compact_count", "pings_pool_compact", "pings_pool_select_scratch_bytes",
                 "pings_pool_select_count", "pings_pool_select_update"]
DEV = "cuda"
CHUNK = 2048                    # rows per wave of the count / scan / emit kernels


def _npz(name):
    with np.load(GOLDEN / f"frame_pool_{name}.npz") as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


def _to(t, dev):
    return None if t is None else t.to(dev)


class ReplaySampler:
    """Returns the fixture's samples and checks that it was given the fixture's (static) frame tensors."""

    def __init__(self, z, dev):
        self.z, self.dev, self.frame = z, dev, 0

    def sample(self, points, normal, sem, color, color_valid_mask=None):
        f = self.frame
        for k, t in zip(("points", "normal", "sem", "color"), (points, normal, sem, color)):
            want = self.z.get(f"f{f}_in_{k}")
            assert (t is None) == (want is None), f"frame {f}: sampler input {k}"
            if t is not None:
                assert torch.equal(t.cpu(), want), f"frame {f}: sampler input {k}"
        return tuple(_to(self.z.get(f"f{f}_s_{k}"), self.dev)
                     for k in ("coord", "sdf_label", "normal", "sem", "color", "weight"))


def _close(got, ref, bound, what):
    assert got.shape == ref.shape, what
    err = (got.cpu().double() - ref.cpu().double()).abs()
    worst = float((err / bound.cpu().clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: worst error / gate {worst:.3f}")
    assert worst <= 1.0, f"{what}: error / gate = {worst}"


def _same(got, ref, what):
    assert (got is None) == (ref is None), what
    if got is not None:
        assert got.dtype == ref.dtype and got.shape == ref.shape and torch.equal(got.cpu(), ref.cpu()), what


def _run_sequence(name, dev, step, dtype=torch.float32, check=None):
    """Feeds the fixture's frames to `step(m, pc, label, normal, pose, frame, dynamic, draw)`; `check(m, z, f)` after
    each."""
    seq, z = FR.SEQUENCES[name], _npz(name)
    m = FR.mapper_state(FR.frame_cfg(seq, device=dev, bs=64), 0, device=dev, dtype=dtype)
    m.sampler = ReplaySampler(z, dev)
    for f in range(FR.FRAMES):
        m.sampler.frame = f
        m.next_static = z[f"f{f}_static"].to(dev)
        step(m, z[f"f{f}_pc"].to(dev), _to(z.get(f"f{f}_label"), dev), _to(z.get(f"f{f}_normal"), dev),
             z[f"f{f}_pose"].to(dev), f, seq["dynamic"] and f >= 1, _to(z.get(f"f{f}_draw"), dev))
        if check is not None:
            check(m, z, f)
    return m, z


def _pose_bound(points_local, pose, rotate_only=False):
    return FR.transform_bound(points_local, pose, rotate_only)


def _check_frame(m, z, f):
    """Every pool tensor, counter, mask and `update` argument after frame `f` against the fixture."""
    for k in FR.POOLS[1:]:
        _same(getattr(m, k), z.get(f"f{f}_o_{k}"), f"frame {f}: {k}")
    ref = z[f"f{f}_o_global_coord_pool"]
    got = m.global_coord_pool
    assert got.shape == ref.shape and got.is_contiguous()
    # the bound of each pool row, from the frame that made it (time_pool) and its sensor-frame sample: the samples
    # are kept next to the pool and filtered with the fixture's draws
    local = z[f"f{f}_s_coord"] if f == 0 else torch.cat((m.local_rows, z[f"f{f}_s_coord"]), 0)
    if f"f{f}_draw" in z:
        local = local[FR.filter_mask(local.shape[0], m.config.pool_capacity, z[f"f{f}_draw"])]
    m.local_rows = local
    bound = torch.zeros_like(ref, dtype=torch.float64)
    ts = z[f"f{f}_o_time_pool"]
    for g in range(f + 1):
        rows = ts == g
        bound[rows] = _pose_bound(local[rows], z[f"f{g}_pose"])
    _close(got, ref, bound, f"frame {f}: global_coord_pool")
    counts = z[f"f{f}_counts"].tolist()
    assert [m.cur_sample_count, m.pool_sample_count, m.sdf_train_frame_count, len(m.neural_points.resets),
            m.neural_points.memory] == counts, f"frame {f}: counters"
    _same(m.static_mask, z[f"f{f}_o_static"], f"frame {f}: static_mask")
    assert m.dataset.static_mask is m.static_mask
    assert m.local_sample_indices.dim() == 1
    _same(m.local_sample_indices, z[f"f{f}_o_local"], f"frame {f}: local_sample_indices")
    pts, col, nrm, origin, orientation, fid = m.neural_points.updates[-1]
    pose = z[f"f{f}_pose"]
    assert fid == f and torch.equal(origin.cpu(), pose[:3, 3]) and torch.equal(orientation.cpu(), pose[:3, :3])
    _same(col, z.get(f"f{f}_u_colors"), f"frame {f}: update colours")
    cfg = m.config
    if cfg.from_sample_points:
        local, nlocal = z[f"f{f}_s_coord"], z.get(f"f{f}_s_normal")
        if not cfg.from_all_samples:
            sel = z[f"f{f}_s_sdf_label"].abs() < cfg.surface_sample_range_m * cfg.map_surface_ratio
            local, nlocal = local[sel], None if nlocal is None else nlocal[sel]
    else:
        local, nlocal = z[f"f{f}_in_points"], z.get(f"f{f}_in_normal")
    _close(pts, z[f"f{f}_u_points"], _pose_bound(local, pose), f"frame {f}: update points")
    if f"f{f}_u_normals" in z:
        _close(nrm, z[f"f{f}_u_normals"], _pose_bound(nlocal, pose, True), f"frame {f}: update normals")
    else:
        assert nrm is None


# ================================================================ CPU: restatement against the fixtures
@pytest.mark.parametrize("name", list(FR.SEQUENCES))
def test_restatement_matches_the_reference_fixture(name):
    def step(m, pc, label, normal, pose, f, dynamic, draw):
        assert (draw is not None) == (FR.discard_count(m, f, m.sampler.z[f"f{f}_s_coord"].shape[0]) > 0)
        FR.process_frame(m, pc, label, normal, pose, f, dynamic, draw)

    m, z = _run_sequence(name, "cpu", step, check=_check_frame)
    assert sum(f"f{f}_draw" in z for f in range(FR.FRAMES)) >= 2, "fewer than two filter calls discard rows"
    assert m.global_coord_pool.shape[0] > m.config.pool_capacity        # duplicates in the draws: fewer rows went
    seq = FR.SEQUENCES[name]
    assert (m.color_pool is None) == (seq["color"] == 0) and (m.sem_label_pool is None) == (not seq["labels"])
    assert (m.normal_label_pool is None) == (not seq["normals"])


def test_float64_restatement_is_within_the_gate_of_the_fixture():
    def step(m, pc, label, normal, pose, f, dynamic, draw):
        FR.process_frame(m, pc, label, normal, pose, f, dynamic, draw, dtype=torch.float64)

    _run_sequence("dynamic_gray_normals", "cpu", step, dtype=torch.float64, check=_check_frame)


def test_fixtures_cover_what_the_issue_lists():
    seqs = FR.SEQUENCES.values()
    assert any(s["color"] for s in seqs) and any(not s["color"] for s in seqs)
    assert any(s["labels"] for s in seqs) and any(not s["labels"] for s in seqs)
    assert any(s["dynamic"] for s in seqs) and any(s["all_samples"] for s in seqs)
    z = _npz("dynamic_gray_normals")
    assert not z["f1_o_static"].all() and z["f0_o_static"].all()


def test_library_exports_the_frame_entries_and_rejects_null_pointers():
    from pings_amd import _abi, _lib

    L = _lib.lib()
    assert set(FRAME_SYMBOLS) <= set(hdr.header_symbols()) and set(FRAME_SYMBOLS) <= set(_abi.SIGNATURES)
    assert all(hasattr(L, n) for n in FRAME_SYMBOLS)
    assert L.pings_abi_version() == 11
    assert L.pings_pool_append(None, None) == 1
    assert L.pings_pool_append(ctypes.byref(_abi.PoolAppendArgs(n=0, m=4, capacity=8)), None) == 1
    assert b"null" in L.pings_last_error()
    assert L.pings_pool_append(ctypes.byref(_abi.PoolAppendArgs(n=6, m=4, capacity=8)), None) == 1     # does not fit
    assert L.pings_pool_discard_mark(None, 4, 10, None, None, None) == 1
    counts = (ctypes.c_int64 * 2)(-1, -1)
    assert L.pings_pool_compact_count(None, 4, 2, None, counts, None) == 1
    assert L.pings_pool_compact_count(None, 4, 2, None, None, None) == 1
    assert L.pings_pool_compact(None, 1, None, 4, None, None) == 1
    jobs = (_abi.GatherJob * 1)(_abi.GatherJob(None, None, 4, 4))
    assert L.pings_pool_compact(jobs, 1, None, 4, None, None) == 1
    count = ctypes.c_int64(-1)
    assert L.pings_pool_select_count(None, 4, 0.1, None, ctypes.byref(count), None) == 1
    assert L.pings_pool_select_update(None, None) == 1
    assert L.pings_pool_select_update(ctypes.byref(_abi.PoolSelectArgs(n=4, capacity=4, select_all=1)), None) == 1
    # a few words per 2048 rows, no per-row array
    assert L.pings_pool_compact_scratch_bytes(10_000_000) < 100_000
    assert L.pings_pool_select_scratch_bytes(10_000_000) < 100_000


def _stand_ins():
    calls = []

    class Sampler:
        def sample(self, *a, **k):
            return "original sample"

    class Mapper:
        def get_batch(self, global_coord=True):
            return "original get_batch"

        def transform_data_pool(self, pose_diff_torch):
            pass

        def process_frame(self, point_cloud_torch, frame_label_torch, frame_normal_torch, cur_pose_torch, frame_id,
                          filter_dynamic=False, mono_depth_point_cloud_torch=None,
                          mono_depth_point_normals_torch=None):
            calls.append((frame_id, filter_dynamic, mono_depth_point_cloud_torch is not None))
            return "original process_frame"

    return Sampler, Mapper, calls


def test_install_with_frame_rebinds_process_frame_and_uninstall_restores():
    from pings_amd import pool_ops

    Sampler, Mapper, _ = _stand_ins()
    orig = Mapper.process_frame
    pool_ops.install(Sampler, Mapper)                   # the default leaves process_frame alone
    assert Mapper.process_frame is orig and "_pings_process_frame_original" not in vars(Mapper)
    pool_ops.install(Sampler, Mapper, frame=True)
    pool_ops.install(Sampler, Mapper, frame=True)       # twice changes nothing
    assert Mapper.process_frame is pool_ops.process_frame and Mapper._pings_process_frame_original is orig
    assert Mapper.get_batch is pool_ops.get_batch
    pool_ops.uninstall(Sampler, Mapper)
    assert Mapper.process_frame is orig
    assert not any(k.startswith("_pings_") for k in list(vars(Sampler)) + list(vars(Mapper)))


def test_fallbacks_reach_the_original_process_frame():
    from pings_amd import pool_ops

    Sampler, Mapper, calls = _stand_ins()
    pool_ops.install(Sampler, Mapper, frame=True)
    try:
        seq = FR.SEQUENCES["rgb_labels"]
        m = Mapper()
        for k, v in vars(FR.mapper_state(FR.frame_cfg(seq), 1)).items():
            setattr(m, k, v)
        pc, label, normal, pose, _ = FR.frame_inputs(seq, 0, 1)
        assert m.process_frame(pc, label, normal, pose, 3) == "original process_frame"                # CPU tensors
        assert m.process_frame(pc.double(), label, normal, pose, 4, True) == "original process_frame"  # non-float32
        m.config.monodepth_on = True
        assert m.process_frame(pc, label, normal, pose, 5, False, pc.clone()) == "original process_frame"
        assert calls == [(3, False, False), (4, True, False), (5, False, True)]
    finally:
        pool_ops.uninstall(Sampler, Mapper)
    state = FR.mapper_state(FR.frame_cfg(seq), 1)
    with pytest.raises(RuntimeError, match="none was kept"):                # never a silent torch path
        pool_ops.process_frame(state, pc, label, normal, pose, 0)


# ================================================================ GPU
def _pool(n, C, normals, labels, seed, dev=DEV):
    """A pool of `n` rows as the mapper holds it, with `C` colour channels (0: no colour pool)."""
    m = PR.pool_state(n, bool(C), normals, labels, seed, dev)
    if C and C != 3:
        m.color_pool = m.color_pool[:, :C].contiguous()
    m.config = NS(pool_capacity=10 ** 9)
    m.cur_sample_count = 0
    return m


def _clone(m):
    c = NS(**vars(m))
    for k in FR.POOLS:
        t = getattr(m, k)
        setattr(c, k, None if t is None else t.clone())
    return c


def _frame(mrows, C, normals, labels, seed, dev=DEV):
    g = torch.Generator().manual_seed(seed)
    t = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    return (t(mrows, 3) * 20.0, t(mrows), t(mrows, 3) if normals else None,
            torch.randint(0, 20, (mrows,), generator=g, dtype=torch.int32).to(dev) if labels else None,
            torch.rand(mrows, C, generator=g).to(dev) if C else None, t(mrows))


def _check_views(m, store):
    for k in FR.POOLS:
        t = getattr(m, k)
        if t is None:
            assert k not in store.front
        else:
            assert t.is_contiguous() and t.shape[0] == store.rows
            assert store.rows == 0 or t.data_ptr() == store.front[k].data_ptr()     # a view of no rows has no pointer


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2049])
@pytest.mark.parametrize("rows", [1, 255, 256, 257])
def test_append_kernel_against_float64(rows, n):
    from pings_amd import pool_ops

    for case, (C, normals, labels, pdt) in enumerate(((3, True, True, torch.float64), (1, False, False, torch.float32),
                                                     (0, False, True, torch.float64), (3, True, False, torch.float32),
                                                     (0, False, False, torch.float32))):
        m = _pool(n, C, normals, labels, seed=n + case)
        before = _clone(m)
        coord, sdf, normal, sem, color, weight = _frame(rows, C, normals, labels, seed=rows + case)
        pose = PR.rigid_poses(1, pdt, seed=rows + n)[0].to(DEV)
        pool_ops.append_frame(m, coord, sdf, normal, sem, color, weight, pose, 17)
        ref = _clone(before)
        FR.append(ref, coord, sdf, normal, sem, color, weight, pose, 17, torch.float64)
        for k in FR.POOLS[1:]:
            _same(getattr(m, k), getattr(ref, k), f"{k} rows={rows} n={n} case={case}")
        assert torch.equal(m.global_coord_pool[:n], before.global_coord_pool), "old rows were touched"
        assert (m.time_pool[n:] == 17).all() and m.time_pool.dtype == torch.int32
        _close(m.global_coord_pool[n:], ref.global_coord_pool[n:], _pose_bound(coord, pose),
               f"append rows={rows} n={n} case={case}")
        _check_views(m, m._pings_pool_store)


@pytest.mark.gpu
def test_append_drops_a_pool_without_its_label_and_refuses_a_label_without_its_pool():
    from pings_amd import pool_ops

    m = _pool(300, 3, True, True, seed=1)
    coord, sdf, normal, sem, color, weight = _frame(64, 3, True, True, seed=2)
    pose = torch.eye(4, device=DEV)
    pool_ops.append_frame(m, coord, sdf, None, None, color, weight, pose, 1)
    assert m.normal_label_pool is None and m.sem_label_pool is None and m.color_pool.shape == (364, 3)
    with pytest.raises(TypeError):                      # the reference's torch.cat((None, sem_label)) raises
        pool_ops.append_frame(m, coord, sdf, None, sem, color, weight, pose, 2)
    assert m.global_coord_pool.shape[0] == 364


@pytest.mark.gpu
def test_append_across_a_regrow_keeps_the_rows_and_repoints_the_views():
    from pings_amd import pool_ops

    m = _pool(0, 3, False, True, seed=3)
    ref = _clone(m)
    pose = PR.rigid_poses(1, torch.float64, seed=4)[0].to(DEV)
    ptrs, caps = set(), []
    for f in range(4):                                  # 4 x 1500 rows: the first buffers hold 4096
        fr = _frame(1500, 3, False, True, seed=10 + f)
        held = m.global_coord_pool
        pool_ops.append_frame(m, *fr, pose, f)
        FR.append(ref, *fr, pose, f, torch.float64)
        store = m._pings_pool_store
        _check_views(m, store)
        ptrs.add(m.global_coord_pool.data_ptr())
        caps.append(store.capacity)
        assert held.shape[0] == 1500 * f                # a view handed out earlier keeps its rows
        assert torch.equal(m.global_coord_pool[: 1500 * f], held)
    assert caps[0] == caps[1] == 4096 and caps[2] > 4096 and caps[2] == caps[3] and len(ptrs) == 2
    for k in FR.POOLS[1:]:
        _same(getattr(m, k), getattr(ref, k), k)
    again = m.global_coord_pool.clone()
    m.sdf_label_pool = m.sdf_label_pool.clone()         # a user assignment: taken in again with one copy
    fr = _frame(10, 3, False, True, seed=20)
    pool_ops.append_frame(m, *fr, pose, 9)
    FR.append(ref, *fr, pose, 9, torch.float64)
    _check_views(m, m._pings_pool_store)
    _same(m.sdf_label_pool, ref.sdf_label_pool, "sdf_label_pool after re-adoption")
    assert torch.equal(m.global_coord_pool[:6000], again)
    again = m.global_coord_pool.clone()
    for k in FR.POOLS:                                  # shifted slices of the store's own buffers
        for s in (m, ref):
            t = getattr(s, k)
            setattr(s, k, None if t is None else t[7:])
    pool_ops.append_frame(m, *fr, pose, 10)
    FR.append(ref, *fr, pose, 10, torch.float64)
    _check_views(m, m._pings_pool_store)
    for k in FR.POOLS[1:]:
        _same(getattr(m, k), getattr(ref, k), f"{k} after a shifted slice")
    assert torch.equal(m.global_coord_pool[:6003], again[7:])


def _filter_case(n, C, normals, labels, draw, tail, seed):
    """filter_pool with a given draw against the restatement: every tensor torch.equal, both counts equal."""
    from pings_amd import pool_ops

    m = _pool(n, C, normals, labels, seed)
    m.config.pool_capacity = n - draw.shape[0]
    m.cur_sample_count = tail
    ref = _clone(m)
    pool_ops.filter_pool(m, _draws=draw.to(DEV))
    FR.filter_pool(ref, draw.to(DEV))
    for k in FR.POOLS:
        _same(getattr(m, k), getattr(ref, k), f"{k} n={n}")
    assert (m.cur_sample_count, m.pool_sample_count) == (ref.cur_sample_count, ref.pool_sample_count)
    assert m.pool_sample_count == m.global_coord_pool.shape[0]
    _check_views(m, m._pings_pool_store)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 1])
def test_compaction_equals_the_restatement(n):
    from pings_amd import pool_ops

    assert CHUNK == 2048
    g = torch.Generator().manual_seed(n)
    tail = max(n // 3, 1)
    head = n - tail
    opts = ((3, True, True), (1, False, False), (0, False, True))
    # nothing discarded: at the capacity nothing moves; and the kernels with an all-ones mask
    m = _pool(n, 3, True, True, seed=n)
    m.config.pool_capacity, m.cur_sample_count = n, tail
    ref = _clone(m)
    pool_ops.filter_pool(m)
    for k in FR.POOLS:
        _same(getattr(m, k), getattr(ref, k), f"{k} untouched")
    assert (m.cur_sample_count, m.pool_sample_count) == (tail, n)
    store = pool_ops.pool_store(m)
    store.adopt(m)
    assert pool_ops._compact_by(store, torch.ones(n, dtype=torch.uint8, device=DEV), tail) == (n, tail)
    store.publish(m)
    for k in FR.POOLS:
        _same(getattr(m, k), getattr(ref, k), f"{k} all kept")
    # one row discarded: the first, the last, one in the middle
    for i, row in enumerate((0, n - 1, n // 2)):
        _filter_case(n, *opts[i % 3], torch.tensor([row]), tail, seed=n + i)
    # heavy duplicates: many draws of three rows
    d = min(n, 40)
    draw = torch.tensor([0, n - 1, n // 2])[torch.randint(0, 3, (d,), generator=g)]
    m = _filter_case(n, 3, False, True, draw, tail, seed=n + 5)
    assert m.pool_sample_count == n - int(draw.unique().numel()) > n - d or d <= 3
    # every tail row discarded: cur_sample_count becomes 0
    m = _filter_case(n, 1, True, False, torch.arange(head, n), tail, seed=n + 6)
    assert m.cur_sample_count == 0 and m.pool_sample_count == head
    # discards only in the head, a random half of it with duplicates
    if head:
        draw = torch.randint(0, head, (max(head // 2, 1),), generator=g)
        m = _filter_case(n, 3, True, True, draw, tail, seed=n + 7)
        assert m.cur_sample_count == tail
    # a random draw over the whole pool
    _filter_case(n, 0, False, False, torch.randint(0, n, (max(n // 4, 1),), generator=g), tail, seed=n + 8)


@pytest.mark.gpu
def test_an_out_of_range_draw_sets_the_status_bit_and_moves_nothing_wrongly():
    from pings_amd import pool_ops

    n = 2049
    assert pool_ops.last_filter_status() == 0
    m = _pool(n, 3, True, True, seed=8)
    draw = torch.tensor([5, n, -1, 2048, n + 10 ** 12, 5])
    m.config.pool_capacity, m.cur_sample_count = n - draw.shape[0], 100
    ref = _clone(m)
    pool_ops.filter_pool(m, _draws=draw.to(DEV))
    assert pool_ops.last_filter_status() == 1 and pool_ops.last_filter_status() == 0     # read and cleared
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[[5, 2048]] = False
    for k in FR.POOLS:
        _same(getattr(m, k), getattr(ref, k)[keep], k)
    assert (m.cur_sample_count, m.pool_sample_count) == (99, n - 2)


@pytest.mark.gpu
def test_filter_pool_draws_as_the_reference_and_leaves_the_generator_where_it_does():
    from pings_amd import pool_ops

    n, capacity = 5000, 4000
    m = _pool(n, 3, False, True, seed=9)
    m.config.pool_capacity, m.cur_sample_count, m.device = capacity, 700, torch.device(DEV)
    ref = _clone(m)
    torch.manual_seed(4321)
    pool_ops.filter_pool(m)
    state = torch.cuda.get_rng_state()
    torch.manual_seed(4321)
    draw = torch.randint(0, n, (n - capacity,), device=DEV)
    assert torch.equal(state, torch.cuda.get_rng_state()), "the randint call is not the reference's"
    FR.filter_pool(ref, draw)
    for k in FR.POOLS:
        _same(getattr(m, k), getattr(ref, k), k)
    assert (m.cur_sample_count, m.pool_sample_count) == (ref.cur_sample_count, ref.pool_sample_count)
    assert capacity < m.pool_sample_count < n


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 2049, 2 * 2048 + 1])
def test_select_update_against_float64(n):
    from pings_amd import pool_ops

    for case, (C, normals, pdt) in enumerate(((3, True, torch.float64), (0, False, torch.float32),
                                              (1, True, torch.float32))):
        coord, sdf, normal, _, color, _ = _frame(n, C, normals, False, seed=n + case)
        pose = PR.rigid_poses(1, pdt, seed=n + 3)[0].to(DEV)
        for thr in (0.7, 0.0, 1e30, None):              # about half the rows, none, every row, every row unread
            got = pool_ops.select_update(coord, sdf, color, normal, pose, thr)
            ref = FR.select_update(coord, sdf, color, normal, pose, thr, torch.float64)
            sel = torch.ones(n, dtype=torch.bool, device=DEV) if thr is None else sdf.abs() < thr
            assert got[0].shape[0] == int(sel.sum()) and (thr != 0.0 or got[0].shape[0] == 0)
            assert thr not in (1e30, None) or got[0].shape[0] == n
            _same(got[1], ref[1], f"colours n={n} thr={thr}")           # exact copies: the row order as well
            _close(got[0], ref[0], _pose_bound(coord[sel], pose), f"points n={n} thr={thr} case={case}")
            assert (got[2] is None) == (not normals)
            if normals:
                _close(got[2], ref[2], _pose_bound(normal[sel], pose, True), f"normals n={n} thr={thr}")
                if got[2].shape[0]:                     # rotated, not translated: the length is kept
                    assert torch.allclose(got[2].norm(dim=1), normal[sel].norm(dim=1), rtol=1e-5)
    if n > 1:                                           # ascending rows without colours: a monotone coordinate
        coord = torch.stack((torch.arange(n, device=DEV).float(),) * 3, 1).contiguous()
        got = pool_ops.select_update(coord, sdf, None, None, torch.eye(4, device=DEV), 0.7)[0]
        assert torch.equal(got, coord[sdf.abs() < 0.7])


def _library_step(monkeypatch):
    from pings_amd import pool_ops

    real = torch.randint

    def step(m, pc, label, normal, pose, f, dynamic, draw):
        def fake(low, high, size, **kw):                # the capacity filter's call, answered with the fixture's draw
            assert draw is not None and (low, high, tuple(size)) == (0, m.global_coord_pool.shape[0], tuple(draw.shape))
            return draw
        monkeypatch.setattr(torch, "randint", fake)
        try:
            pool_ops.process_frame(m, pc, label, normal, pose, f, dynamic)
        finally:
            monkeypatch.setattr(torch, "randint", real)

    return step


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FR.SEQUENCES))
def test_process_frame_over_the_fixture_sequence(name, monkeypatch):
    from pings_amd import _lib, pool_ops

    step = _library_step(monkeypatch)
    seq = FR.SEQUENCES[name]

    def counted(m, pc, label, normal, pose, f, dynamic, draw):
        _lib.sync_counts(reset=True)
        step(m, pc, label, normal, pose, f, dynamic, draw)
        reads = _lib.sync_counts(reset=True)
        want = {"pool_window_count": 1}
        if dynamic:
            want["mask_rows_count"] = 1
        if seq["from_samples"] and not seq["all_samples"]:
            want["pool_update_rows"] = 1
        if draw is not None:
            want["pool_filter_counts"] = 1
        assert reads == want and sum(reads.values()) <= 5, f"frame {f}: host reads {reads}"

    m, z = _run_sequence(name, DEV, counted, check=_check_frame)
    _check_views(m, m._pings_pool_store)
    # the views are what the other pool methods take
    m.local_sample_indices, m.new_idx = m.local_sample_indices, None
    batch = pool_ops.get_batch(m)
    assert batch[0].shape == (64, 3) and pool_ops.last_status() == 0
    storage = m.global_coord_pool.data_ptr()
    before = m.global_coord_pool.clone()
    pool_ops.transform_data_pool(m, torch.eye(4, dtype=torch.float64, device=DEV).repeat(FR.FRAMES, 1, 1))
    assert m.global_coord_pool.data_ptr() == storage and torch.equal(m.global_coord_pool, before)
    _check_views(m, m._pings_pool_store)


@pytest.mark.gpu
def test_two_runs_of_one_sequence_are_bit_equal(monkeypatch):
    step = _library_step(monkeypatch)
    a, _ = _run_sequence("all_samples_rgb_normals", DEV, step)
    b, _ = _run_sequence("all_samples_rgb_normals", DEV, step)
    for k in FR.POOLS:
        ta, tb = getattr(a, k), getattr(b, k)
        assert torch.equal(ta.view(torch.int32), tb.view(torch.int32)), k
    for ua, ub in zip(a.neural_points.updates, b.neural_points.updates):
        for ta, tb in zip(ua[:3], ub[:3]):
            assert (ta is None and tb is None) or torch.equal(ta.view(torch.int32), tb.view(torch.int32))


@pytest.mark.gpu
def test_filter_pool_allocates_at_most_two_bytes_per_row():
    """10^6 rows with both buffer sets in place: room for the keep mask (1 B per row) and the draw (8 B per discarded
    row, 7 % of the rows here), not for the reference's 8-byte-per-row index or a third copy of the pool."""
    from pings_amd import pool_ops

    n, capacity = 1_000_000, 930_000
    m = _pool(n, 3, False, False, seed=11)
    m.config.pool_capacity, m.cur_sample_count = capacity, 70_000
    store = pool_ops.pool_store(m)
    store.adopt(m)
    store.reserve(store.capacity, back=True)
    draw = torch.randint(0, n, (n - capacity,), device=DEV)
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[draw] = False
    want = (int(keep.sum()), int(keep[-70_000:].sum()), m.sdf_label_pool[keep])
    del keep
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    pool_ops.filter_pool(m, _draws=draw)
    rise = torch.cuda.max_memory_allocated() - base
    print(f"filter_pool of {n} rows: memory rise {rise} B = {rise / n:.3f} B per row")
    assert (m.pool_sample_count, m.cur_sample_count) == want[:2] and torch.equal(m.sdf_label_pool, want[2])
    assert rise <= 2 * n, f"{rise} bytes allocated across the call"
