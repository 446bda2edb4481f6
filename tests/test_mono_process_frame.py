"""The mono-depth branch of `pool_ops.process_frame` (utils/mapper.py:297-331) over tests/golden/camfront_mono_frame.npz:
the reference's own `Mapper.process_frame` on the stand-ins of tests/frame_pool_ref.py with a mono-depth cloud of 300
rows (tools/make_camfront_golden.py).

Gates: the second `update` receives the fixture's rows, same count and order (the fixture has no mono point within 1e-5
of the quantile threshold), values at the project's 1e-4 relative gate, colours equal (they are copied), with
`is_reliable=True`; the caller's cloud ends up transformed at 1e-4; the pool tensors equal those of the same frame
without a mono cloud bit for bit; two runs are bit-equal.
"""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import camfront_ref as CR
import frame_pool_ref as FR
from conftest import GOLDEN, rel_err
from pings_amd import _lib, pool_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEQ = FR.SEQUENCES["rgb_labels"]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN / "camfront_mono_frame.npz") as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


class _Replay:
    """Returns the fixture's samples (the reference's sampler stand-in draws seeded noise on the CPU)."""

    def __init__(self, z, tag):
        self.z, self.tag = z, tag

    def sample(self, points, normal, sem, color, color_valid_mask=None):
        assert torch.equal(points.cpu(), self.z[f"{self.tag}_in_points"])
        return tuple(None if f"{self.tag}_s_{k}" not in self.z else self.z[f"{self.tag}_s_{k}"].to(DEV)
                     for k in ("coord", "sdf_label", "normal", "sem", "color", "weight"))


class _Original:
    calls = []

    def process_frame(self, *a, **k):
        _Original.calls.append(a)
        return "original process_frame"


def _run(z, tag, mono="fixture", normals=None):
    high_z, _ = CR.MONO_CASES[tag]
    m = FR.mapper_state(FR.frame_cfg(SEQ, device=DEV, bs=64, **CR.MONO_CFG), 0, device=DEV)
    m.neural_points, m.sampler = CR.MonoMapRecorder(), _Replay(z, tag)
    m.dataset.loader = NS(mono_depth_for_high_z=high_z)
    cloud = z[f"{tag}_mono"].clone().to(DEV) if isinstance(mono, str) else mono
    _lib.sync_counts(reset=True)
    out = pool_ops.process_frame(m, z[f"{tag}_pc"].to(DEV), z[f"{tag}_label"].to(DEV), None, z[f"{tag}_pose"].to(DEV),
                                 0, False, cloud, normals)
    return m, cloud, _lib.sync_counts(reset=True), out


@pytest.mark.parametrize("tag", list(CR.MONO_CASES))
def test_mono_branch_over_the_fixture(golden, tag):
    z = golden
    m, cloud, reads, _ = _run(z, tag)
    ups = m.neural_points.updates
    assert m.neural_points.memory == 1
    # the main update is the one of the frame without a mono cloud
    assert ups[0][6] is False and rel_err(ups[0][0], z[f"{tag}_u_points"]) <= 1e-4
    assert torch.equal(ups[0][1].cpu(), z[f"{tag}_u_colors"])
    # the caller's tensor: xyz transformed in place, the colours untouched
    after = z[f"{tag}_mono_after"]
    assert tuple(cloud.shape) == tuple(after.shape) and rel_err(cloud[:, :3], after[:, :3]) <= 1e-4
    assert torch.equal(cloud[:, 3:].cpu(), after[:, 3:]) and not torch.equal(cloud[:, :3].cpu(), z[f"{tag}_mono"][:, :3])
    if tag == "none":
        assert len(ups) == 1                                                 # nothing is updated on the empty case
    else:
        assert len(ups) == 2
        pts, col, nrm, origin, orientation, fid, reliable = ups[1]
        want = z[f"{tag}_m_points"]
        assert reliable is True and nrm is None and fid == 0
        assert torch.equal(origin.cpu(), z[f"{tag}_pose"][:3, 3]) and torch.equal(orientation.cpu(), z[f"{tag}_pose"][:3, :3])
        assert tuple(pts.shape) == tuple(want.shape) and pts.dtype is torch.float32
        assert rel_err(pts, want) <= 1e-4                                    # same count, same order
        assert torch.equal(col.cpu(), z[f"{tag}_m_colors"])
    assert reads.get("mask_rows_count") == 1 and reads.get("pool_update_rows") == 1 and reads.get("pool_window_count") == 1
    assert sum(reads.values()) == 3, reads
    # the pool is the pool of the same frame without a mono cloud
    plain, _, _, _ = _run(z, tag, mono=None)
    assert len(plain.neural_points.updates) == 1
    for k in FR.POOLS:
        a, b = getattr(m, k), getattr(plain, k)
        if a is None or b is None:                                           # a pool the frame has no label for
            assert a is None and b is None, k
            continue
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), k
        ref = z[f"{tag}_o_{k}"]
        assert tuple(a.shape) == tuple(ref.shape), k
    assert rel_err(m.global_coord_pool, z[f"{tag}_o_global_coord_pool"]) <= 1e-4


def test_two_runs_are_bit_equal(golden):
    a, ca, _, _ = _run(golden, "low")
    b, cb, _, _ = _run(golden, "low")
    assert torch.equal(ca.view(torch.int32), cb.view(torch.int32))
    for ua, ub in zip(a.neural_points.updates, b.neural_points.updates):
        for ta, tb in zip(ua[:2], ub[:2]):
            assert torch.equal(ta.view(torch.int32), tb.view(torch.int32))
    assert len(a.neural_points.updates) == len(b.neural_points.updates) == 2


def test_normals_and_a_cpu_cloud_reach_the_original(golden):
    z = golden

    def through(mono, normals):
        m = _Original()
        for k, v in vars(FR.mapper_state(FR.frame_cfg(SEQ, device=DEV, bs=64, **CR.MONO_CFG), 0, device=DEV)).items():
            setattr(m, k, v)
        return m.process_frame(z["low_pc"].to(DEV), z["low_label"].to(DEV), None, z["low_pose"].to(DEV), 0, False,
                               mono, normals)

    pool_ops.install(None, _Original, frame=True)
    try:
        _Original.calls.clear()
        mono = z["low_mono"].clone()
        assert through(mono.to(DEV), torch.zeros(300, 3, device=DEV)) == "original process_frame"   # normals
        assert through(mono, None) == "original process_frame"                                       # a CPU cloud
        assert through(mono.to(DEV).double(), None) == "original process_frame"                      # not float32
        assert through(mono.to(DEV)[:, :5].contiguous(), None) == "original process_frame"           # columns
        assert len(_Original.calls) == 4
    finally:
        pool_ops.uninstall(None, _Original)
