"""Golden vectors of the pool part of `Mapper.process_frame` from the reference's own method.

`Mapper.process_frame` (utils/mapper.py:170-526) is called unbound on a stand-in `self` on the CPU over the short
sequences of tests/frame_pool_ref.py: a recording stub for `neural_points`, a sampler that is the restatement of
tests/pool_ref.py under seeded noise, a `dynamic_filter` that returns the frame's stored mask.  `torch.randint` is
wrapped while it runs, so the files hold the capacity filter's draws next to the inputs, the arguments `update`
received and every pool tensor and counter after each frame.  Writes tests/golden/frame_pool_*.npz (data only);
tests/test_frame_pool.py reads only the files.

    python tools/make_frame_pool_golden.py            (needs the reference tree; CPU only)
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

from make_pool_golden import Recorder, put, reference  # noqa: E402


def main():
    import frame_pool_ref as FR
    import pool_ref as PR

    R, _, Mapper = reference()
    out_dir = ROOT / "tests" / "golden"
    for seed, (name, seq) in enumerate(FR.SEQUENCES.items(), start=1):
        cfg = R.make_config(**vars(FR.frame_cfg(seq)))
        m = FR.mapper_state(cfg, seed)
        rec, discards = {}, 0
        for f in range(FR.FRAMES):
            pc, label, normal, pose, static = FR.frame_inputs(seq, f, seed)
            dynamic = seq["dynamic"] and f >= 1
            m.next_static = static
            for k, t in zip(("pc", "label", "normal", "pose", "static"), (pc, label, normal, pose, static)):
                put(rec, f"f{f}_{k}", t)
            with Recorder() as r:
                Mapper.process_frame(m, pc.clone(), label, normal, pose.clone(), f, dynamic)
            draws = [t for n, t in r.draws if n == "randint"]       # the sampler stand-in draws its noise as well
            assert len(draws) <= 1
            if draws:
                put(rec, f"f{f}_draw", draws[0])
                discards += 1
            ins, outs = m.sampler.calls[-1]
            for k, t in zip(("points", "normal", "sem", "color"), ins):
                put(rec, f"f{f}_in_{k}", None if t is None else t.contiguous())
            for k, t in zip(("coord", "sdf_label", "normal", "sem", "color", "weight"), outs):
                put(rec, f"f{f}_s_{k}", t)
            upd = m.neural_points.updates[-1]
            assert upd[5] == f and torch.equal(upd[3], pose[:3, 3]) and torch.equal(upd[4], pose[:3, :3])
            for k, t in zip(("points", "colors", "normals"), upd[:3]):
                put(rec, f"f{f}_u_{k}", None if t is None else t.contiguous())
            for k in FR.POOLS:
                put(rec, f"f{f}_o_{k}", getattr(m, k))
            put(rec, f"f{f}_o_static", m.static_mask)
            assert m.dataset.static_mask is m.static_mask
            put(rec, f"f{f}_o_local", m.local_sample_indices.reshape(-1))
            rec[f"f{f}_counts"] = np.array([m.cur_sample_count, m.pool_sample_count, m.sdf_train_frame_count,
                                            len(m.neural_points.resets), m.neural_points.memory], dtype=np.int64)
            # no pool row at the window's edge: the library tests it in float32, the reference in the pose's dtype
            d = PR.window_dist(m.global_coord_pool, pose[:3, 3].float(), cfg.range_filter_2d)
            assert ((d - cfg.window_radius).abs() > 1e-5 * cfg.window_radius).all(), (name, f)
            assert 0 < m.local_sample_indices.numel() < m.global_coord_pool.shape[0], (name, f)
            thr = cfg.surface_sample_range_m * cfg.map_surface_ratio
            assert ((outs[1].abs() - thr).abs() > 1e-6).all(), (name, f)
        assert discards >= 2 and len(m.neural_points.updates) == FR.FRAMES, (name, discards)
        np.savez_compressed(out_dir / f"frame_pool_{name}.npz", **rec)
        print(name, "rows", m.global_coord_pool.shape[0], "filter calls that discard", discards)


if __name__ == "__main__":
    main()
