"""Golden vectors of the mapper's sample-pool code from the reference's own functions.

`DataSampler.sample` (utils/data_sampler.py) runs as it is; `Mapper.get_batch` and `Mapper.transform_data_pool`
(utils/mapper.py:704-778) are called unbound on stand-ins that hold the pool tensors.  `torch.randn`, `torch.rand` and
`torch.randint` are wrapped while they run, so the files hold the draws next to the inputs and the outputs.  Writes
tests/golden/pool_*.npz; tests/test_pool_ops.py reads only the files.

    python tools/make_pool_golden.py            (needs the reference tree; CPU only)
"""
import sys
from pathlib import Path
from unittest.mock import MagicMock

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from oracle import ref_shim  # noqa: E402


def reference():
    R = ref_shim.load()                  # stubs the reference's non-arithmetic imports, puts the tree on sys.path
    from utils.data_sampler import DataSampler  # type: ignore

    for _ in range(20):                  # utils/mapper.py's image-metric and logging imports: stubs (no arithmetic)
        try:
            from utils.mapper import Mapper  # type: ignore
            break
        except ModuleNotFoundError as e:
            if e.name in sys.modules or e.name.split(".")[0] in ("utils", "model", "dataset", "gaussian_splatting"):
                raise
            sys.modules[e.name] = MagicMock()
    else:
        raise RuntimeError("could not import utils.mapper")
    return R, DataSampler, Mapper


class Recorder:
    """Wraps the three random functions of torch and keeps what they returned, in call order."""

    def __enter__(self):
        self.draws, self._orig = [], {}
        for name in ("randn", "rand", "randint"):
            self._orig[name] = getattr(torch, name)
            setattr(torch, name, self._wrap(name))
        return self

    def _wrap(self, name):
        def f(*a, **k):
            out = self._orig[name](*a, **k)
            self.draws.append((name, out.clone()))
            return out
        return f

    def __exit__(self, *exc):
        for name, fn in self._orig.items():
            setattr(torch, name, fn)


def put(rec, key, t):
    if t is not None:
        rec[key] = t.detach().cpu().numpy()


def main():
    import pool_ref as ref

    R, DataSampler, Mapper = reference()
    out_dir = ROOT / "tests" / "golden"
    for name, (P, (ns, nf, nb), dw, drop, ch, normals, labels, origin) in ref.GOLDEN_SAMPLE.items():
        cfg = R.make_config(surface_sample_n=ns, free_front_n=nf, free_behind_n=nb, dist_weight_on=dw,
                            behind_dropoff_on=drop, **ref.SAMPLE_CFG)
        pts, nrm, sem, col = ref.sample_inputs(P, ch, normals, labels, origin, seed=len(name) + P)
        torch.manual_seed(P)
        with Recorder() as r:
            out = DataSampler(cfg).sample(pts, nrm, sem, col)
        assert [n for n, _ in r.draws] == ["randn", "rand", "rand"]
        rec = {}
        for k, t in zip(("points", "normal", "sem", "color"), (pts, nrm, sem, col)):
            put(rec, k, t)
        for k, (_, t) in zip(("noise_surface", "noise_front", "noise_behind"), r.draws):
            put(rec, k, t)
        for k, t in zip(("o_coord", "o_sdf_label", "o_normal", "o_sem", "o_color", "o_weight"), out):
            put(rec, k, t)
        np.savez_compressed(out_dir / f"pool_sample_{name}.npz", **rec)
        print("sample", name, tuple(out[0].shape))
    for name, case in ref.GOLDEN_BATCH.items():
        m = ref.batch_state(*case, seed=len(name))
        torch.manual_seed(len(name))
        with Recorder() as r:
            out = Mapper.get_batch(m)
        assert all(n == "randint" for n, _ in r.draws)
        rec = {"r_hist": r.draws[0][1].numpy()}
        if len(r.draws) > 1:
            rec["r_new"] = r.draws[1][1].numpy()
        for k, t in zip(("o_coord", "o_sdf_label", "o_ts", "o_normal", "o_sem", "o_color", "o_weight"), out):
            put(rec, k, t)
        np.savez_compressed(out_dir / f"pool_batch_{name}.npz", **rec)
        print("batch", name, len(r.draws), tuple(out[0].shape))
    for name, (N, pdt, tdt) in ref.GOLDEN_TRANSFORM.items():
        m = ref.pool_state(N, False, False, False, seed=N)
        m.time_pool = (m.time_pool.long() - ref.POSES * (torch.arange(N) % 3 == 0)).to(getattr(torch, tdt))
        pose = ref.rigid_poses(ref.POSES, pdt, seed=N + 1)
        rec = {"points": m.global_coord_pool.numpy(), "ts": m.time_pool.numpy(), "pose": pose.numpy()}
        Mapper.transform_data_pool(m, pose)
        put(rec, "o_points", m.global_coord_pool)
        np.savez_compressed(out_dir / f"pool_transform_{name}.npz", **rec)
        print("transform", name, tuple(m.global_coord_pool.shape))


if __name__ == "__main__":
    main()
